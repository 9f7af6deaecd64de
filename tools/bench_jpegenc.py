"""
JPEG encode on the GPU against PIL on the host, on the same pixels in the same run: `python tools/bench_jpegenc.py [--out FILE]`.

  24 images of 4096 x 3008 and 24 of 512 x 376 at quality 95, in 4:4:4 and 4:2:0, with photograph-like content (smooth colour
  fields plus fine noise, the generator of the tests at size) and with uniform random content: eight cases.
  prepare: one frame of 24 raw 4096 x 3008 photographs through topo4d_amd.prepare end to end (read, decode, undistort, box mean,
  encode, write), against the same frame with --encoder pil.

GPU figures: HIP events around jpeg.encode_jpeg - the launches, the read of the lengths and the copy of the files into host memory,
i.e. the time to bytes in host memory - the minimum of --reps runs after a warm-up; "wall" is a host clock around the same call.
PIL figures: a host clock around Image.fromarray(a).save(BytesIO, "JPEG", quality=95, subsampling=s) of the same arrays, in a loop on
one thread and on a pool of 16 threads.  Every GPU file is compared with PIL's.  One JSON object is printed and written.
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from topo4d_amd import jpeg, prepare  # noqa: E402

POOL = 16


def photo(h: int, w: int, seed: int, dev) -> torch.Tensor:
    """uint8 [h,w,3]: tests/jpegenc_cases.py's "smooth" content at size, made on the device"""
    g = torch.Generator(device=dev).manual_seed(seed)
    y, x = torch.meshgrid(torch.linspace(-1, 1, h, device=dev), torch.linspace(-1, 1, w, device=dev), indexing="ij")
    f = torch.stack([0.5 + 0.4 * torch.sin(5 * x + seed), 0.5 + 0.4 * torch.cos(4 * y), 0.5 + 0.3 * torch.sin(3 * (x + y))], -1)
    f = f + 0.02 * torch.randn((h, w, 3), generator=g, device=dev)
    return (f.clamp(0, 1) * 255).to(torch.uint8).contiguous()


def noise(h: int, w: int, seed: int, dev) -> torch.Tensor:
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(0, 256, (h, w, 3), generator=g, device=dev, dtype=torch.uint8)


def pil_encode(a: np.ndarray, subsampling: int) -> bytes:
    return jpeg.pil_bytes(a, 95, subsampling)


def host_seconds(fn, reps: int) -> float:
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


def one_case(images, subsampling: int, reps: int, pil_reps: int) -> dict:
    files = jpeg.encode_jpeg(images, 95, subsampling)                       # warm-up
    events, walls = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        a.record()
        files = jpeg.encode_jpeg(images, 95, subsampling)
        b.record()
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t) * 1e3)
        events.append(a.elapsed_time(b))
    arrays = [im.cpu().numpy() for im in images]
    want = [pil_encode(a, subsampling) for a in arrays]
    r = {"images": len(images), "pixel_bytes": sum(a.size for a in arrays), "file_bytes": sum(len(f) for f in files),
         "gpu_event_ms": min(events), "gpu_wall_ms": min(walls), "reps": reps, "equal_pil": files == want}
    r["pil_1_thread_ms"] = host_seconds(lambda: [pil_encode(a, subsampling) for a in arrays], pil_reps) * 1e3
    with ThreadPoolExecutor(max_workers=POOL) as pool:
        r["pil_16_threads_ms"] = host_seconds(lambda: list(pool.map(lambda a: pil_encode(a, subsampling), arrays)), pil_reps) * 1e3
    r["speedup_over_16_threads"] = r["pil_16_threads_ms"] / r["gpu_event_ms"]
    return r


def raw_frame(root: str, views: int, h: int, w: int, dev) -> None:
    """<root>/seq/cameras.xml and 000001/<name>.jpg: `views` photographs with a mild lens each"""
    from PIL import Image
    os.makedirs(os.path.join(root, "seq", "000001"))
    sensors, cams = [], []
    for i in range(views):
        name = "K%08d" % i
        Image.fromarray(photo(h, w, i, dev).cpu().numpy()).save(os.path.join(root, "seq", "000001", name + ".jpg"), "JPEG", quality=95,
                                                               subsampling=0)
        sensors.append(f'<sensor id="{i}" type="frame"><resolution width="{w}" height="{h}"/><calibration type="frame">'
                       f'<resolution width="{w}" height="{h}"/><f>{w * 2.7}</f><cx>{i - 12.5}</cx><cy>{7.25 - i}</cy><k1>-0.03</k1>'
                       f'<k2>0.1</k2><p1>0.0003</p1><p2>-0.0002</p2></calibration></sensor>')
        cams.append(f'<camera id="{i}" sensor_id="{i}" label="{name}"><transform>1 0 0 0 0 1 0 0 0 0 1 1 0 0 0 1</transform></camera>')
    with open(os.path.join(root, "seq", "cameras.xml"), "w") as f:
        f.write('<?xml version="1.0" encoding="UTF-8"?>\n<document version="1.4.0"><chunk><sensors>' + "".join(sensors)
                + "</sensors><cameras>" + "".join(cams) + "</cameras></chunk></document>\n")


def prepare_case(views: int, h: int, w: int, dev) -> dict:
    r = {"views": views, "height": h, "width": w, "down_ratio": 8, "quality": 95, "subsampling": 0}
    with tempfile.TemporaryDirectory() as root:
        raw_frame(root, views, h, w, dev)
        for enc in ("gpu", "gpu", "pil"):                                   # the first run warms the allocator and the pinned buffer
            out = os.path.join(root, "out_" + enc)
            torch.cuda.synchronize()
            t = time.perf_counter()
            written = prepare.prepare_tree(root, "seq", os.path.join(out, "low"), os.path.join(out, "dense"), down_ratio=8, encoder=enc)
            torch.cuda.synchronize()
            r[f"frame_{enc}_ms"] = (time.perf_counter() - t) * 1e3
            r["files"] = len(written)
        r["gpu_equals_pil_tree"] = all(open(p, "rb").read() == open(p.replace("out_pil", "out_gpu"), "rb").read() for p in written)
    return r


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None, help="also write the JSON here")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--pil_reps", type=int, default=2)
    p.add_argument("--images", type=int, default=24)
    p.add_argument("--skip", default="", help="comma-separated parts to leave out: full, low, prepare")
    args = p.parse_args(argv)
    skip = set(args.skip.split(","))
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "quality": 95, "pool": POOL, "batch_bytes": jpeg.batch_bytes}
    for size, (h, w) in (("low", (376, 512)), ("full", (3008, 4096))):
        if size in skip:
            continue
        for kind, make in (("photo", photo), ("random", noise)):
            images = [make(h, w, i, dev) for i in range(args.images)]
            for s in (0, 2):
                name = f"{size}_{h}x{w}_{kind}_{'444' if s == 0 else '420'}"
                res[name] = one_case(images, s, args.reps, args.pil_reps)
                print(name, json.dumps(res[name]), flush=True)
            del images
    if "prepare" not in skip:
        res["prepare_one_frame"] = prepare_case(args.images, 3008, 4096, dev)
        print("prepare_one_frame", json.dumps(res["prepare_one_frame"]), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
