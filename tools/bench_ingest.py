#!/usr/bin/env python
"""A frame's views from file bytes in host memory to float32 device targets (topo4d_amd/ingest.py, csrc/t4d_ingest.hip), as
get_dataset runs it at geometry resolution (24 views of 512x375 JPEG plus 24 RGB PNG masks) and on a --gen_tex frame (24 views
of 4096x3008).  Prints one JSON line.
    python tools/bench_ingest.py [--views 24] [--reps 5] [--no-cpu]
frame_ms / view_ms: decode_jpeg + the warp of every view, GPU time between two HIP events (min of --reps); the views are
synthetic q95 4:2:0 JPEGs of a smooth field with 2 % noise, rotated by +-90 as rotate_mask does.  warp: the warp launches alone
and their share of 6.3 TB/s for 2 reads of the uint8 source plus one float32 write.  cpu: the reference's host steps that can
be timed without skimage (PIL decode, /255.0, .float(), H2D of the float32 target) per 4096x3008 view; skimage's own rotate is
not timed.  The kernel split comes from a separate rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from topo4d_amd import ingest

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=24)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-cpu", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")
HBM = 6.3e12


def view(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    f = np.stack([0.5 + 0.4 * np.sin(5 * x + seed), 0.5 + 0.4 * np.cos(4 * y), 0.5 + 0.3 * np.sin(3 * (x + y))], -1)
    f = np.clip(f + rng.normal(0, 0.02, f.shape), 0, 1)
    return (f * 255).astype(np.uint8)


def encode(img, fmt="JPEG"):
    b = io.BytesIO()
    Image.fromarray(img).save(b, fmt, **({"quality": 95} if fmt == "JPEG" else {}))
    return b.getvalue()


def gpu_ms(fn, reps):
    best = float("inf")
    for _ in range(reps + 1):                                  # the first run warms up
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        best = min(best, s.elapsed_time(e))
    return best


def frame(files, angles, masks=None):
    dec = ingest.decode_jpeg(files)
    srcs, angs, crops = list(dec), list(angles), [None] * len(dec)
    if masks is not None:
        for m, d, ang in zip(masks, dec, angles):
            srcs.append(torch.from_numpy(m).to(dev))
            angs.append(ang)
            crops.append(tuple(d.shape[:2]))
    return ingest._rotate_all(srcs, angs, crops, None)


res = {"views": a.views}
for name, (h, w) in (("geom_512x375", (375, 512)), ("tex_4096x3008", (3008, 4096))):
    base = [view(h, w, s) for s in range(min(a.views, 4))]
    files = [encode(base[i % len(base)]) for i in range(a.views)]
    angles = [90 if i % 2 else -90 for i in range(a.views)]
    masks = None
    if h == 375:
        masks = [np.array(np.asarray(Image.open(io.BytesIO(encode((base[i % len(base)] > 128).astype(np.uint8) * 255,
                                                                                 "PNG"))))) for i in range(a.views)]
    ms = gpu_ms(lambda: frame(files, angles, masks), a.reps)
    dec = ingest.decode_jpeg(files)
    mats, shapes = zip(*[ingest.rotate_matrix(h, w, ang) for ang in angles])
    outs = [torch.empty((3,) + s, dtype=torch.float32, device=dev) for s in shapes]
    wms = gpu_ms(lambda: ingest.warp_views(dec, mats, shapes, out=outs), a.reps)
    dms = gpu_ms(lambda: ingest.decode_jpeg(files), a.reps)
    nbytes = a.views * h * w * 3 * (2 + 4)
    res[name] = {"frame_ms": round(ms, 3), "view_ms": round(ms / a.views, 3), "decode_ms": round(dms, 3), "warp_ms": round(wms, 3),
                 "warp_tb_s": round(nbytes / (wms * 1e-3) / 1e12, 3), "warp_hbm_share": round(nbytes / (wms * 1e-3) / HBM, 3),
                 "jpeg_mb_per_view": round(sum(len(f) for f in files) / a.views / 1e6, 3)}

if not a.no_cpu:
    img = view(3008, 4096, 0)
    data = encode(img)
    t = {}
    t0 = time.perf_counter(); arr = np.array(Image.open(io.BytesIO(data))); t["pil_decode_ms"] = time.perf_counter() - t0
    t0 = time.perf_counter(); f64 = arr / 255.0; t["div255_ms"] = time.perf_counter() - t0
    t0 = time.perf_counter(); f32 = torch.tensor(f64).float(); t["float_ms"] = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter(); f32.cuda(); torch.cuda.synchronize(); t["h2d_float32_ms"] = time.perf_counter() - t0
    res["cpu_per_4k_view"] = {k: round(v * 1e3, 1) for k, v in t.items()}
    res["cpu_per_4k_view"]["skimage_rotate"] = "not timed (skimage not installed)"
print(json.dumps(res))
