#!/usr/bin/env python
"""PNG encoding of a baked texture on the GPU (topo4d_amd/png.py, csrc/t4d_png.hip) against PIL on one core, on the uv_mesh(1025)
bake of tools/bench_bake.py and on a smooth synthetic texture.  Prints one JSON line.
    python tools/bench_png.py [--res 8192] [--n 1025] [--no-cpu]
encode_ms: device-resident float32 image -> PNG bytes in host memory (min of 5); kernel_ms: the four encoder launches alone, HIP
events (min of 5); mb / ratio_to_pil: compressed size, and over PIL's default-level size of the same uint8 image; cpu_baseline:
numpy's quantise plus PIL's encode (write_texture's encoder="pil" path after the bake); write_texture_gpu_ms: the whole
write_texture(encoder="gpu") into a temporary directory (min of 3)."""
import argparse
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scaffold.scene import uv_mesh
from topo4d_amd import _lib, png, texture

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=8192)
ap.add_argument("--n", type=int, default=1025)
ap.add_argument("--no-cpu", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")


def smooth_texture(res, seed=0):
    """Smooth colour field, 1 % noise, black outside a disc (the same recipe as tests/test_gpu_png.py)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(-1, 1, res), np.linspace(-1, 1, res), indexing="ij")
    f = np.stack([0.5 + 0.4 * np.sin(3 * x + 1), 0.5 + 0.4 * np.cos(2 * y), 0.5 + 0.3 * np.sin(2 * (x + y))], -1)
    f = f + rng.normal(0, 0.01, f.shape)
    f[(x * x + y * y) > 0.9] = 0
    return np.clip(f, 0, 1).astype(np.float32)


def kernel_ms(img):
    lib = _lib.load()
    h, w, c = img.shape
    cap, ns = png.max_encoded_bytes(h, w, c), int(lib.t4d_png_scratch_bytes(h, w, c))
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    scratch = torch.empty(ns, dtype=torch.uint8, device=dev)
    length = torch.empty(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream()
    best = 1e9
    for _ in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = lib.t4d_png_encode(C.c_void_p(img.data_ptr()), 1, h, w, c, C.c_void_p(out.data_ptr()), cap,
                                C.c_void_p(length.data_ptr()), C.c_void_p(scratch.data_ptr()), ns, C.c_void_p(stream.cuda_stream))
        e1.record(stream)
        assert rc == 0, _lib.last_error()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def measure(img):
    data = png.encode_png(img)                                   # warm-up
    runs = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = png.encode_png(img)
        runs.append(time.perf_counter() - t0)
    r = {"encode_ms": round(min(runs) * 1e3, 3), "kernel_ms": round(kernel_ms(img), 3), "mb": round(len(data) / 1e6, 3)}
    if not a.no_cpu:
        from PIL import Image
        t0 = time.perf_counter()
        u8 = (img.cpu().numpy() * 255).astype(np.uint8)
        t1 = time.perf_counter()
        b = io.BytesIO()
        Image.fromarray(u8).save(b, format="PNG")
        t2 = time.perf_counter()
        pil = b.getvalue()
        decoded = np.asarray(Image.open(io.BytesIO(data)))
        r.update({"pil_mb": round(len(pil) / 1e6, 3), "ratio_to_pil": round(len(data) / len(pil), 4),
                  "pixels_equal": bool(np.array_equal(decoded, u8)),
                  "cpu_baseline": {"value": round((t2 - t1) * 1e3, 1), "unit": "ms", "quantise_ms": round((t1 - t0) * 1e3, 1),
                                   "cores": 1, "kind": "port", "sample": "PIL save at the default level, one run"},
                  "speedup": round((t2 - t1) * 1e3 / r["encode_ms"], 1)})
    return r


verts, tris, colors = uv_mesh(a.n, a.res, a.res, seed=0)
bake = texture.render_colors(verts, tris, colors, a.res, a.res)
smooth = torch.as_tensor(smooth_texture(a.res)).to(dev)
out = {"metric": "PNG encode of a baked texture", "res": a.res, "channels": 3,
       "bake": measure(bake), "smooth": measure(smooth)}
uvs = np.stack([verts[:, 0] / (a.res - 1), (a.res - 1 - verts[:, 1]) / (a.res - 1)], 1)
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "tex.png")
    texture.write_texture(path, uvs, colors, tris, res=a.res, encoder="gpu")
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        texture.write_texture(path, uvs, colors, tris, res=a.res, encoder="gpu")
        runs.append(time.perf_counter() - t0)
out["write_texture_gpu_ms"] = round(min(runs) * 1e3, 1)
out["includes"] = "encode_ms: launches, one sync, D2H of the file through pinned memory, copy to a bytes object"
print(json.dumps(out))
