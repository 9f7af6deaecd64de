#!/usr/bin/env python
"""The displacement-map finishing steps of topo4d_amd/dispmap.py at 4096 x 4096 (evaluate's --bake_res default) and 8192 x 8192, on a
synthetic bake: a smooth displacement field over three UV islands with a gutter between them, 3 % of the rays missed at random and
a few discs knocked out.  Prints one JSON line.
    python tools/bench_dispmap.py [--reps 5] [--sizes 4096,8192] [--host_sizes 4096]
Per size, GPU time between two HIP events, min of --reps after one warm-up:
    quantize_ms      dispmap.quantize
    fill_ms          texfinish.fill16_islands (one push-pull pass per island, and its one read of two flags per label)
    smooth4_ms       dispmap.smooth, 4 rounds
    normals_ms       dispmap.normals
    png_grey_ms      png.encode_png16 of the codes (with its synchronisation and the copy of the file to the host)
    png_rgb_ms       png.encode_png16 of the normal map
    png_grey_bytes, png_rgb_bytes: the files' sizes
For the sizes in --host_sizes the yardsticks on the host, one run each (wall clock): host_*_ms are the numpy restatements of
tests/dispmap_ref.py on the same inputs, same_*: their output equals the device's bit for bit; pil_grey_ms is PIL writing the same
16-bit grey image to memory (compress_level 6, its default), pil_grey_bytes that file's size.  A size not in --host_sizes carries
no host_* keys: not measured."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topo4d_amd import dispmap, png, texfinish  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[4096, 8192])
ap.add_argument("--host_sizes", type=lambda s: [int(x) for x in s.split(",") if x], default=[4096])
a = ap.parse_args()
dev = torch.device("cuda")
DIST = 0.004


def bake(n):
    """(disp float32, hit uint8, labels uint8, pos float32 [n,n,3]) on the device"""
    g = torch.Generator(device=dev).manual_seed(n)
    f = torch.rand(1, 1, n // 16, n // 16, device=dev, generator=g)
    f = F.interpolate(f, size=(n, n), mode="bicubic", align_corners=False)[0, 0]
    disp = ((f - 0.5) * 1.6 * DIST + (torch.rand(n, n, device=dev, generator=g) - 0.5) * 0.02 * DIST).to(torch.float32)
    labels = torch.zeros(n, n, dtype=torch.uint8, device=dev)
    m = n // 64
    labels[m:n // 2 - m, m:n - m] = 1
    labels[n // 2 + m:n - m, m:n // 2 - m] = 2
    labels[n // 2 + m:n - m, n // 2 + m:n - m] = 3
    hit = ((torch.rand(n, n, device=dev, generator=g) > 0.03) & (labels != 0))
    y, x = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
    for cy, cx, r in ((n // 4, n // 3, n // 40), (3 * n // 4, n // 4, n // 25), (3 * n // 4, 3 * n // 4, n // 60)):
        hit &= (y - cy) ** 2 + (x - cx) ** 2 > r * r
    pos = torch.stack([x / n, 1.0 - y / n, 0.05 * torch.sin(6.0 * x / n) * torch.cos(5.0 * y / n)], -1).to(torch.float32)
    return disp.contiguous(), hit.to(torch.uint8), labels, pos.contiguous()


def timed(fn, reps):
    times = []
    for _ in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return round(min(times[1:]), 3), out


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return round((time.perf_counter() - t) * 1e3, 1), out


result = {"bench": "dispmap", "dist": DIST, "sizes": {}}
for n in a.sizes:
    disp, hit, labels, pos = bake(n)
    unit = dispmap.code_unit(DIST)
    row = {}
    row["quantize_ms"], (code, has) = timed(lambda: dispmap.quantize(disp, hit, DIST), a.reps)
    row["fill_ms"], (filled_code, filled) = timed(lambda: texfinish.fill16_islands(code, has, labels), a.reps)
    has2 = has | filled
    row["filled_texels"] = int(filled.sum())
    row["smooth4_ms"], smooth = timed(lambda: dispmap.smooth(filled_code, has2, labels, 4), a.reps)
    row["normals_ms"], normal = timed(lambda: dispmap.normals(smooth, has2, labels, pos, unit), a.reps)
    row["png_grey_ms"], grey = timed(lambda: png.encode_png16(smooth), a.reps)
    row["png_rgb_ms"], rgb = timed(lambda: png.encode_png16(normal), a.reps)
    row["png_grey_bytes"], row["png_rgb_bytes"] = len(grey), len(rgb)
    if n in a.host_sizes:
        from PIL import Image
        from tests import dispmap_ref as ref
        h = {k: v.cpu().numpy() for k, v in dict(disp=disp, hit=hit, labels=labels, pos=pos, code=code, has=has, fc=filled_code,
                                                 has2=has2, smooth=smooth, normal=normal).items()}
        row["host_quantize_ms"], q = wall(lambda: ref.quantize(h["disp"], h["hit"], DIST))
        row["same_quantize"] = bool(np.array_equal(q[0], h["code"]) and np.array_equal(q[1], h["has"]))
        row["host_fill_ms"], f16 = wall(lambda: ref.fill16_islands(h["code"], h["has"], h["labels"]))
        row["same_fill"] = bool(np.array_equal(f16[0], h["fc"]))
        row["host_smooth4_ms"], s4 = wall(lambda: ref.smooth(h["fc"], h["has2"], h["labels"], 4))
        row["same_smooth"] = bool(np.array_equal(s4, h["smooth"]))
        row["host_normals_ms"], nm = wall(lambda: ref.normals(h["smooth"], h["has2"], h["labels"], h["pos"], unit))
        row["same_normals"] = bool(np.array_equal(nm, h["normal"]))
        buf = io.BytesIO()
        image = Image.fromarray(h["smooth"].astype(np.uint16))
        row["pil_grey_ms"], _ = wall(lambda: image.save(buf, format="PNG"))
        row["pil_grey_bytes"] = buf.getbuffer().nbytes
        row["same_pil_decode"] = bool(np.array_equal(np.asarray(Image.open(io.BytesIO(grey))).astype(np.int32), h["smooth"]))
        del h, q, f16, s4, nm
    result["sizes"][str(n)] = row
    print(json.dumps({str(n): row}), file=sys.stderr, flush=True)
    del disp, hit, labels, pos, code, has, filled_code, filled, has2, smooth, normal
    torch.cuda.empty_cache()
print(json.dumps(result))
