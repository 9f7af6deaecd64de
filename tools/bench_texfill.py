#!/usr/bin/env python
"""The push-pull hole fill on the GPU (topo4d_amd/texfinish.py: fill, fill_islands; csrc/t4d_texfill.hip).  Prints one JSON line.
    python tools/bench_texfill.py [--res 8192] [--missing 0.05,0.3]
The domain is four rectangular islands (about 80 % of the image); the missing texels are the blobs where a smooth random field
falls below the quantile that gives the share asked for.  Per share:
  fill_kernel_ms          t4d_texture_fill alone between HIP events on preallocated buffers (min of 6)
  fill_ms                 texfinish.fill, allocations included, to a synchronise (min of 3)
  fill_islands_ms         texfinish.fill_islands over the 4 islands, its read of the per-label flags included (min of 3)
  torch_ms                the same rule written level by level in plain torch on the same device (min of 3), asserted bit-equal:
                          what a user would write without the kernel, and what the fused pass is to be read against
  pad_r64_kernel_ms       texfinish.pad at radius 64 (the remedy before this), launches alone (min of 6)
bytes_per_texel is what the pass must move at the least (image and valid in, image and filled out, the pyramid written once and
read once), gbytes_per_s that over fill_kernel_ms."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from topo4d_amd import _lib, texfinish

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=8192)
ap.add_argument("--missing", type=lambda s: [float(x) for x in s.split(",")], default=[0.05, 0.3])
a = ap.parse_args()
dev = torch.device("cuda")
lib = _lib.load()
P = lambda t: C.c_void_p(t.data_ptr())
res = a.res


def events_ms(launch, repeats=6):
    stream = torch.cuda.current_stream()
    best = 1e9
    launch(C.c_void_p(stream.cuda_stream))
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
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    return round(min(runs) * 1e3, 2)


def ok(rc):
    assert rc == 0, _lib.last_error()


def torch_fill(image, valid, domain):
    """the rule of include/topo4d_raster.h, one level per step"""
    v = valid != 0
    cs, vs = [torch.where(v[..., None], image.to(torch.int32) * 256, 0)], [v]
    while tuple(vs[-1].shape) != (1, 1):
        c, v = cs[-1], vs[-1]
        h, w = v.shape
        h2, w2 = (h + 1) // 2, (w + 1) // 2
        cp = F.pad(c, (0, 0, 0, 2 * w2 - w, 0, 2 * h2 - h))
        vp = F.pad(v.to(torch.int32), (0, 2 * w2 - w, 0, 2 * h2 - h))
        s, n = cp.view(h2, 2, w2, 2, -1).sum((1, 3)), vp.view(h2, 2, w2, 2).sum((1, 3))[..., None]
        cs.append(torch.where(n > 0, (2 * s + n) // (2 * n).clamp_min(1), 0))
        vs.append(n[..., 0] > 0)
    if not bool(vs[-1][0, 0]):
        return image.clone(), torch.zeros_like(valid)
    up = cs[-1]
    for k in range(len(cs) - 2, -1, -1):
        h, w = vs[k].shape
        y, x = torch.arange(h, device=image.device), torch.arange(w, device=image.device)
        py, px = y >> 1, x >> 1
        ny = (py + torch.where((y & 1) != 0, 1, -1)).clamp(0, up.shape[0] - 1)[:, None]
        nx = (px + torch.where((x & 1) != 0, 1, -1)).clamp(0, up.shape[1] - 1)
        py = py[:, None]
        mix = (9 * up[py, px] + 3 * up[py, nx] + 3 * up[ny, px] + up[ny, nx] + 8) >> 4
        up = torch.where(vs[k][..., None], cs[k], mix)
    take = (domain != 0) & ~vs[0]
    return torch.where(take[..., None], ((up + 128) >> 8).to(torch.uint8), image), take.to(torch.uint8)


g = torch.Generator(device="cpu").manual_seed(0)
image = torch.randint(0, 256, (res, res, 3), dtype=torch.uint8, generator=g).to(dev)
labels = torch.zeros(res, res, dtype=torch.uint8, device=dev)
q = res // 32
for k, (y0, y1, x0, x1) in enumerate([(q, 15 * q, q, 15 * q), (q, 15 * q, 17 * q, 31 * q), (17 * q, 31 * q, q, 15 * q), (17 * q, 31 * q, 17 * q, 31 * q)]):
    labels[y0:y1, x0:x1] = k + 1
domain = (labels != 0).to(torch.uint8)
field = F.interpolate(torch.rand(1, 1, 64, 64, generator=g), size=(res, res), mode="bicubic", align_corners=False)[0, 0].to(dev)
inside = field[domain != 0]
out, filled = torch.empty_like(image), torch.empty_like(domain)
scratch = torch.empty(int(lib.t4d_texture_fill_scratch_bytes(res, res, 3)), dtype=torch.uint8, device=dev)
pad_scratch = torch.empty(int(lib.t4d_texture_pad_scratch_bytes(res, res)), dtype=torch.uint8, device=dev)
out_cov = torch.empty_like(domain)

levels = 0
while (res - 1) >> levels:
    levels += 1
pyramid_texels = sum((((res - 1) >> k) + 1) ** 2 for k in range(1, levels + 1))
bytes_per_texel = (3 + 1 + 1) + (3 + 1) + 2 * 6 * pyramid_texels / (res * res)       # in (image, valid, domain), out, pyramid
result = {"metric": "push-pull hole fill of a projected texture", "res": res, "channels": 3, "islands": 4,
          "domain_fraction": round(float((domain != 0).float().mean()), 4), "bytes_per_texel": round(bytes_per_texel, 2), "cases": {}}
for share in a.missing:
    cut = torch.quantile(inside[:: max(1, inside.numel() // (1 << 20))], share)
    valid = ((domain != 0) & (field >= cut)).to(torch.uint8)
    case = {"missing_fraction_of_domain": round(float(((domain != 0) & (valid == 0)).sum() / (domain != 0).sum()), 4)}
    case["fill_kernel_ms"] = events_ms(lambda s: ok(lib.t4d_texture_fill(P(image), P(valid), P(domain), res, res, 3, P(out), P(filled),
                                                                         P(scratch), scratch.numel(), s)))
    case["gbytes_per_s"] = round(bytes_per_texel * res * res / case["fill_kernel_ms"] / 1e6, 1)
    case["fill_ms"] = wall_ms(lambda: texfinish.fill(image, valid, domain))
    case["fill_islands_ms"] = wall_ms(lambda: texfinish.fill_islands(image, valid, labels))
    case["torch_ms"] = wall_ms(lambda: torch_fill(image, valid, domain))
    want, want_filled = torch_fill(image, valid, domain)
    assert torch.equal(out, want) and torch.equal(filled, want_filled), "the kernel and the torch restatement differ"
    got, got_filled = texfinish.fill_islands(image, valid, labels)
    case["filled_texels"] = int(filled.sum())
    assert int(got_filled.sum()) == case["filled_texels"] and torch.equal(got[valid != 0], image[valid != 0])
    case["speedup_over_torch"] = round(case["torch_ms"] / case["fill_ms"], 1)
    case["pad_r64_kernel_ms"] = events_ms(lambda s: ok(lib.t4d_texture_pad(P(image), P(valid), res, res, 3, 64, P(out), P(out_cov),
                                                                           P(pad_scratch), pad_scratch.numel(), s)))
    result["cases"][f"missing_{share:g}"] = case
    del want, want_filled, got, got_filled
print(json.dumps(result))
