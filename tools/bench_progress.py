#!/usr/bin/env python
"""One progress snapshot of train.py (report_progress / report_progress_dense -> torchvision's save_image) against
progress.save_image, on a scaffold render at the geometry loop's 512x376 and at the full capture resolution 4096x3008.  Prints
one JSON line.
    python tools/bench_progress.py [--reps 5] [--sizes 512x376,4096x3008]
reference_ms: the restated torchvision path - x.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8) then
PIL's PNG save into a BytesIO (min of --reps; to_host_ms / pil_ms are its two parts in the same run); gpu_ms:
progress.save_image into a BytesIO (min of --reps: the four encoder launches, one sync, the file through pinned memory);
kernel_ms: the encoder's launches alone (HIP events, min of --reps); size_ratio_to_pil: our file over PIL's, same pixels."""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scaffold import reference_boundary as boundary, scene
from diff_gaussian_rasterization import GaussianRasterizer
from topo4d_amd import _lib, png, progress

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="512x376,4096x3008")
a = ap.parse_args()
dev = torch.device("cuda")


def render(W, H):
    params = {k: v.to(dev) for k, v in scene.make_gaussians(40, 64, opacity="B", seed=1).items()}
    cam = scene.camera_rig(H, W, n_views=1, device=dev)[0]
    with torch.no_grad():
        return GaussianRasterizer(raster_settings=cam)(**boundary.params2rendervar(params))[0]


def reference(x):
    from PIL import Image
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nd = x.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()
    t1 = time.perf_counter()
    b = io.BytesIO()
    Image.fromarray(nd).save(b, format="PNG")
    t2 = time.perf_counter()
    return b.getvalue(), nd, t1 - t0, t2 - t1


def ours(x):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = io.BytesIO()
    progress.save_image(x, b)
    return b.getvalue(), time.perf_counter() - t0


def kernel_ms(x):
    lib = _lib.load()
    _, h, w = x.shape
    cap, ns = png.max_encoded_bytes(h, w, 3), int(lib.t4d_png_scratch_bytes(h, w, 3))
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    scratch = torch.empty(ns, dtype=torch.uint8, device=dev)
    length = torch.empty(1, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream()
    best = 1e9
    for _ in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = lib.t4d_png_encode_chw(C.c_void_p(x.data_ptr()), h, w, C.c_void_p(out.data_ptr()), cap, C.c_void_p(length.data_ptr()),
                                    C.c_void_p(scratch.data_ptr()), ns, C.c_void_p(stream.cuda_stream))
        e1.record(stream)
        assert rc == 0, _lib.last_error()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def measure(W, H):
    from PIL import Image
    x = render(W, H).contiguous()
    data, _ = ours(x)                                              # warm-up
    ref, nd, _, _ = reference(x)
    best_ref = min((reference(x) for _ in range(a.reps)), key=lambda r: r[2] + r[3])
    gpu = min(ours(x)[1] for _ in range(a.reps))
    decoded = np.asarray(Image.open(io.BytesIO(data)))
    return {"size": f"{W}x{H}", "reference_ms": round((best_ref[2] + best_ref[3]) * 1e3, 2),
            "to_host_ms": round(best_ref[2] * 1e3, 2), "pil_ms": round(best_ref[3] * 1e3, 2),
            "gpu_ms": round(gpu * 1e3, 3), "kernel_ms": round(kernel_ms(x), 3), "speedup": round((best_ref[2] + best_ref[3]) / gpu, 1),
            "mb": round(len(data) / 1e6, 3), "pil_mb": round(len(ref) / 1e6, 3), "size_ratio_to_pil": round(len(data) / len(ref), 4),
            "black_fraction": round(float((x == 0).all(0).float().mean()), 3), "pixels_equal": bool(np.array_equal(decoded, nd))}


out = {"metric": "progress snapshot: render -> PNG file bytes", "reps": a.reps,
       "results": [measure(*map(int, s.split("x"))) for s in a.sizes.split(",")],
       "includes": "gpu_ms: launches, one sync, D2H of the file through pinned memory, copy to a bytes object; "
                   "reference_ms: torchvision's device ops, the float32 copy to the host and the uint8 cast there, PIL at its default level"}
print(json.dumps(out))
