"""
PNG decode on the GPU against PIL on the host, on the same bytes in the same run: `python tools/bench_pngdecode.py [--out FILE]`.

  (a) an 8192 x 8192 x 3 texture written by png.encode_png, and its 8192 x 8192 weight image: the chunk-parallel schedule
  (b) the same pixels written by PIL: the serial schedule
  (c) 24 RGB label masks of 512 x 376 written by PIL, one batch: against PIL in a loop and on ingest.pool_size() threads
  (d) the read phase of seqtex (seqtex._read of every frame) over 16 frames at 2048 x 2048, --png_decoder gpu against pil

GPU figures: HIP events around png.decode_png with the headers parsed ahead (upload of the file bytes, the kernels, no read-back),
the minimum of --reps runs after a warm-up; "wall" figures are a host clock around the whole call, parse included, ending in a
synchronise.  PIL figures: a host clock around np.array(Image.open(io.BytesIO(data))).  One JSON object is printed and written.
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
from topo4d_amd import ingest, png, seqtex  # noqa: E402


def texture(res: int, seed: int, dev) -> torch.Tensor:
    """uint8 [res,res,3]: smooth colour fields plus fine noise, black outside a disc (a baked texture's islands and background)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    low = torch.rand((1, 3, res // 64, res // 64), generator=g, device=dev)
    img = torch.nn.functional.interpolate(low, size=(res, res), mode="bicubic", align_corners=False)[0].permute(1, 2, 0)
    img = img + 0.02 * torch.randn((res, res, 3), generator=g, device=dev)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, res, device=dev), torch.linspace(-1, 1, res, device=dev), indexing="ij")
    img = img * ((yy * yy + xx * xx) < 0.9).unsqueeze(-1)
    return (img.clamp(0, 1) * 255).to(torch.uint8).contiguous()


def pil_decode(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


def pil_encode(a: np.ndarray) -> bytes:
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a).save(b, "PNG")
    return b.getvalue()


def host_seconds(fn, reps: int) -> float:
    best = float("inf")
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


def gpu_decode(files, reps: int, dev, slow_after: float = 20.0) -> dict:
    """event and wall milliseconds of png.decode_png(files), the schedules it took, and the tensors of the last run"""
    headers = [png.parse_png(f) for f in files]
    t = time.perf_counter()
    out, paths = png.decode_png(files, device=dev, headers=headers, return_path=True)       # warm-up
    torch.cuda.synchronize()
    warm = time.perf_counter() - t
    if warm > slow_after:                                      # a serial decode of a very large file: one timed run
        reps = 1
    events, walls = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = png.decode_png(files, device=dev, headers=headers)
        b.record()
        torch.cuda.synchronize()
        events.append(a.elapsed_time(b))
        t = time.perf_counter()
        png.decode_png(files, device=dev)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t) * 1e3)
    return {"gpu_event_ms": min(events), "gpu_wall_with_parse_ms": min(walls), "reps": reps, "paths": sorted(set(paths)),
            "file_bytes": sum(len(f) for f in files), "pixel_bytes": sum(h.out_bytes for h in headers)}, out


def equal(t: torch.Tensor, a: np.ndarray) -> bool:
    return tuple(t.shape) == a.shape and bool(torch.equal(t.cpu(), torch.from_numpy(a)))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None, help="also write the JSON here")
    p.add_argument("--res", type=int, default=8192, help="side of the texture of (a) and (b)")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--pil_reps", type=int, default=2, help="host runs of the large files (each takes about a second)")
    p.add_argument("--skip", default="", help="letters of the parts to leave out, e.g. 'b'")
    args = p.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "res": args.res, "pool_size": ingest.pool_size()}

    tex = texture(args.res, 1, dev)
    weight = ((tex.sum(-1) > 0).to(torch.uint8) * 7).contiguous()
    if "a" not in args.skip:
        for name, img in (("a_texture_own_encoder", tex), ("a_weight_own_encoder", weight)):
            data = png.encode_png(img)
            r, out = gpu_decode([data], args.reps, dev)
            assert r["paths"] == [1] and torch.equal(out[0], img)
            want = pil_decode(data)
            r["pil_ms"] = host_seconds(lambda: pil_decode(data), args.pil_reps) * 1e3
            r["equal_pil"] = equal(out[0], want)
            res[name] = r
            print(name, json.dumps(r), flush=True)
    if "b" not in args.skip:
        data = pil_encode(tex.cpu().numpy())
        r, out = gpu_decode([data], args.reps, dev)
        r["pil_ms"] = host_seconds(lambda: pil_decode(data), args.pil_reps) * 1e3
        r["equal_pil"] = bool(torch.equal(out[0], tex))
        res["b_texture_pil_written"] = r
        print("b_texture_pil_written", json.dumps(r), flush=True)
    if "c" not in args.skip:
        rng = np.random.default_rng(3)
        files = []
        for k in range(24):                                    # label masks: a few flat regions with ragged borders
            yy, xx = np.mgrid[0:376, 0:512]
            m = np.zeros((376, 512, 3), np.uint8)
            for lab, (cy, cx, ry, rx) in enumerate(((188, 256, 150, 120), (230, 256, 30, 50), (140, 210, 15, 25), (140, 300, 15, 25))):
                d = ((yy - cy - k) / ry) ** 2 + ((xx - cx + k) / rx) ** 2 + 0.02 * rng.standard_normal((376, 512))
                m[d < 1] = ((lab * 60 + 40) % 256, (lab * 90 + 10) % 256, (lab * 30 + 70) % 256)
            files.append(pil_encode(m))
        r, out = gpu_decode(files, args.reps, dev)
        want = [pil_decode(f) for f in files]
        r["equal_pil"] = all(equal(t, a) for t, a in zip(out, want))
        r["pil_loop_ms"] = host_seconds(lambda: [pil_decode(f) for f in files], args.reps) * 1e3
        with ThreadPoolExecutor(max_workers=ingest.pool_size()) as pool:
            r["pil_pool_ms"] = host_seconds(lambda: list(pool.map(pil_decode, files)), args.reps) * 1e3
        res["c_24_masks_pil_written"] = r
        print("c_24_masks_pil_written", json.dumps(r), flush=True)
    if "d" not in args.skip:
        with tempfile.TemporaryDirectory() as root:
            n, side = 16, 2048
            entries = []
            for t in range(1, n + 1):
                d = os.path.join(root, "%06d" % t)
                os.makedirs(d)
                img = texture(side, 100 + t, dev)
                png.write_png(os.path.join(d, "face_proj_stab.png"), img)
                png.write_png(os.path.join(d, "face_proj_stab_weight.png"), ((img.sum(-1) > 0).to(torch.uint8) * 255).contiguous())
                entries.append(("%06d" % t, "face_proj_stab.png", "face_proj_stab_weight.png"))
            r = {"frames": n, "side": side}
            loaded = {}
            for which, decode_on in (("gpu", dev), ("pil", None), ("gpu", dev), ("pil", None)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loaded[which] = [seqtex._read(root, e, dev, decode_on) for e in entries]
                torch.cuda.synchronize()
                key = f"read_phase_{which}_ms"
                r[key] = min(r.get(key, float("inf")), (time.perf_counter() - t0) * 1e3)
            r["equal"] = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(loaded["gpu"], loaded["pil"]))
            res["d_seqtex_read_phase"] = r
            print("d_seqtex_read_phase", json.dumps(r), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
