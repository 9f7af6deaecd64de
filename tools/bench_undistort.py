#!/usr/bin/env python
"""24 views of 4096x3008 from JPEG bytes in host memory to float32 device targets (topo4d_amd/ingest.py), three ways:
    a  today's path: decode_jpeg + t4d_warp_views (the +-90 turn)
    b  with lenses: decode_jpeg + t4d_undistort_views (undistortion and the turn in one resampling), full-size targets
    c  with lenses and supersample 8: the same launch writing 512x376 targets (what --low_from_full feeds the geometry stage)
Prints one JSON line.
    python tools/bench_undistort.py [--views 24] [--reps 5] [--wide]
frame_ms: the whole path, GPU time between two HIP events (min of --reps); decode_ms and kernel_ms: decode_jpeg and the
resampling launches alone, on already-decoded views and into preallocated targets; kernel_tb_s: 2 reads of the uint8 source
plus one float32 write (a, b) or one read and the small write (c) over kernel_ms.  The views are bench_ingest.py's synthetic q95
4:2:0 JPEGs.  The lens is the golden rig's (f 11,021, k1 -0.0312, k2 0.127) or, with --wide, f 3,500 with k1 -0.08, k2 0.05,
k3 -0.01, p1 3e-4, p2 -2e-4, b1 1.5, b2 -0.7."""
import argparse
import io
import json
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from topo4d_amd import cameras, ingest

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=24)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--wide", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")
H, W, S = 3008, 4096, 8


def view(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    f = np.stack([0.5 + 0.4 * np.sin(5 * x + seed), 0.5 + 0.4 * np.cos(4 * y), 0.5 + 0.3 * np.sin(3 * (x + y))], -1)
    f = np.clip(f + rng.normal(0, 0.02, f.shape), 0, 1)
    return (f * 255).astype(np.uint8)


def encode(img):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=95)
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


if a.wide:
    lens = cameras.Lens(f=3500.0, cxa=W / 2 + 6.0, cya=H / 2 - 4.0, k1=-0.08, k2=0.05, k3=-0.01, p1=3e-4, p2=-2e-4, b1=1.5, b2=-0.7,
                        width=W, height=H)
else:
    lens = cameras.Lens(f=11021.0, cxa=W / 2 + 6.0, cya=H / 2 - 4.0, k1=-0.0312, k2=0.127, width=W, height=H)
base = [view(H, W, s) for s in range(min(a.views, 4))]
files = [encode(base[i % len(base)]) for i in range(a.views)]
angles = [90 if i % 2 else -90 for i in range(a.views)]
lenses = [lens] * a.views
none = [None] * a.views
mats, shapes = zip(*[ingest.rotate_matrix(H, W, ang) for ang in angles])
low = [(r // S, c // S) for r, c in shapes]

res = {"views": a.views, "lens": "wide" if a.wide else "golden rig", "jpeg_mb_per_view": round(sum(len(f) for f in files) / a.views / 1e6, 3)}
res["decode_ms"] = round(gpu_ms(lambda: ingest.decode_jpeg(files), a.reps), 3)
dec = ingest.decode_jpeg(files)
full_out = [torch.empty((3,) + s, dtype=torch.float32, device=dev) for s in shapes]
low_out = [torch.empty((3,) + s, dtype=torch.float32, device=dev) for s in low]
src = a.views * H * W * 3
paths = {
    "a_today": (lambda: ingest._rotate_all(ingest.decode_jpeg(files), angles, none, None),
                lambda: ingest.warp_views(dec, mats, shapes, out=full_out), 2 * src + 4 * src),
    "b_lenses": (lambda: ingest._resample_all(ingest.decode_jpeg(files), angles, none, None, lenses, [1] * a.views, [False] * a.views),
                 lambda: ingest.undistort_views(dec, mats, shapes, lenses, out=full_out), 2 * src + 4 * src),
    "c_lenses_supersample_8": (lambda: ingest._resample_all(ingest.decode_jpeg(files), angles, none, None, lenses, [S] * a.views,
                                                           [False] * a.views),
                               lambda: ingest.undistort_views(dec, mats, low, lenses, out=low_out, supersample=S),
                               src + 4 * src // (S * S)),
}
for name, (whole, kernel, nbytes) in paths.items():
    ms, kms = gpu_ms(whole, a.reps), gpu_ms(kernel, a.reps)
    res[name] = {"frame_ms": round(ms, 3), "view_ms": round(ms / a.views, 3), "kernel_ms": round(kms, 3),
                 "kernel_tb_s": round(nbytes / (kms * 1e-3) / 1e12, 3)}
print(json.dumps(res))
