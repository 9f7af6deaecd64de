#!/usr/bin/env python
"""Texture finishing on the GPU (topo4d_amd/texfinish.py, csrc/t4d_texfinish.hip) on the uv_mesh(1025) bake of tools/bench_bake.py.
Prints one JSON line.
    python tools/bench_texfinish.py [--res 8192] [--n 1025] [--no-cpu]
For quantise + coverage, for the gutter at R = 4 / 16 / 64 and for the halving chain down to 1024: kernel_ms, the launches alone
between HIP events on preallocated buffers (min of 6), and to_bytes_ms, from the device-resident float32 bake and its depth buffer to
the PNG files of the result as bytes in host memory (quantise, coverage, the step, png.encode_png of every level; min of 3) - to be
read against plain_to_bytes_ms, the same without any finishing.  finish_r16_kernel_ms is what an export with --tex_pad 16 adds
before the encoder: quantise + coverage + the gutter.  cpu_baseline: what a user would otherwise write, scipy's
distance_transform_edt(return_indices=True) plus the gather on the host (one run; left out without scipy or with --no-cpu)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scaffold.scene import uv_mesh
from topo4d_amd import _lib, png, texfinish, texture

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=8192)
ap.add_argument("--n", type=int, default=1025)
ap.add_argument("--no-cpu", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")
lib = _lib.load()
P = lambda t: C.c_void_p(t.data_ptr())


def events_ms(launch, repeats=6):
    stream = torch.cuda.current_stream()
    best = 1e9
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch(C.c_void_p(stream.cuda_stream))
        e1.record(stream)
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return round(best, 3)


def wall_ms(fn, repeats=3):
    fn()
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        runs.append(time.perf_counter() - t0)
    return round(min(runs) * 1e3, 2)


def ok(rc):
    assert rc == 0, _lib.last_error()


res = a.res
verts, tris, colors = uv_mesh(a.n, res, res, seed=0)
bake, depth = texture.render_colors(verts, tris, colors, res, res, return_depth=True)
u8 = torch.empty(res, res, 3, dtype=torch.uint8, device=dev)
cov = torch.empty(res, res, dtype=torch.uint8, device=dev)
out, out_cov = torch.empty_like(u8), torch.empty_like(cov)
scratch = torch.empty(int(lib.t4d_texture_pad_scratch_bytes(res, res)), dtype=torch.uint8, device=dev)


def quantise_and_coverage(s):
    ok(lib.t4d_texture_quantize(P(bake), res, res, 3, P(u8), s))
    ok(lib.t4d_texture_coverage(P(depth), res, res, P(cov), s))


def gutter(R):
    return lambda s: ok(lib.t4d_texture_pad(P(u8), P(cov), res, res, 3, R, P(out), P(out_cov), P(scratch), scratch.numel(), s))


sizes = []
while res >> (len(sizes) + 1) >= 1024 and (res >> len(sizes)) % 2 == 0:
    sizes.append(res >> (len(sizes) + 1))
chain = [(u8, cov)] + [(torch.empty(s, s, 3, dtype=torch.uint8, device=dev), torch.empty(s, s, dtype=torch.uint8, device=dev)) for s in sizes]


def halving_chain(s):
    for (src, src_cov), (dst, dst_cov) in zip(chain[:-1], chain[1:]):
        ok(lib.t4d_texture_halve(P(src), P(src_cov), int(src.shape[0]), int(src.shape[1]), 3, P(dst), P(dst_cov), s))


def to_bytes(pad=0, levels=()):
    def run():
        q, c = texfinish.quantize(bake), texfinish.coverage_from_depth(depth)
        done = texfinish.finish(q, c, pad=pad, sizes=levels)
        return [png.encode_png(done[k]) for k in sorted(done, reverse=True)]
    return run


result = {"metric": "texture finishing of a baked texture", "res": res, "channels": 3}
result["quantise_coverage"] = {"kernel_ms": events_ms(quantise_and_coverage), "to_bytes_ms": wall_ms(to_bytes())}
result["covered_fraction"] = round(float((cov != 0).float().mean()), 4)
for R in (4, 16, 64):
    result[f"pad_r{R}"] = {"kernel_ms": events_ms(gutter(R)), "filled_texels": int((out_cov != 0).sum() - (cov != 0).sum()),
                           "to_bytes_ms": wall_ms(to_bytes(pad=R))}
result["halve_to_1024"] = {"sizes": sizes, "kernel_ms": events_ms(halving_chain), "to_bytes_ms": wall_ms(to_bytes(levels=sizes))}
result["finish_r16_kernel_ms"] = round(result["quantise_coverage"]["kernel_ms"] + result["pad_r16"]["kernel_ms"], 3)
result["plain_to_bytes_ms"] = wall_ms(lambda: png.encode_png(bake))
result["png_kernel_budget_ms"] = 8.6
if not a.no_cpu:
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        h_u8, h_cov = u8.cpu().numpy(), cov.cpu().numpy() != 0
        t0 = time.perf_counter()
        dist, (iy, ix) = ndimage.distance_transform_edt(~h_cov, return_indices=True)
        t1 = time.perf_counter()
        fill = (dist <= 16) & ~h_cov
        padded = h_u8.copy()
        padded[fill] = h_u8[iy[fill], ix[fill]]
        t2 = time.perf_counter()
        result["cpu_baseline"] = {"value": round((t2 - t0) * 1e3, 1), "unit": "ms", "edt_ms": round((t1 - t0) * 1e3, 1),
                                  "gather_ms": round((t2 - t1) * 1e3, 1), "cores": 1, "kind": "scipy",
                                  "sample": "distance_transform_edt(return_indices=True) + gather at R = 16, one run"}
        ok(lib.t4d_texture_pad(P(u8), P(cov), res, res, 3, 16, P(out), P(out_cov), P(scratch), scratch.numel(),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        result["cpu_baseline"]["same_filled_set"] = bool(np.array_equal(fill | h_cov, out_cov.cpu().numpy() != 0))
        result["speedup_r16"] = round(result["cpu_baseline"]["value"] / result["pad_r16"]["kernel_ms"], 1)
print(json.dumps(result))
