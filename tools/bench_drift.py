#!/usr/bin/env python
"""The census block matcher of topo4d_amd/drift.py (t4d_drift_match, csrc/t4d_drift.hip) at 2048 x 2048 and 8192 x 8192, block 32,
stride 16, radius 8, on a smooth random texture moved by (3, -2) texels under a gain, against the same rule in plain torch on the
same device: the census words by 48 shifted comparisons, then per candidate displacement one XOR, a byte-table population count
and avg_pool2d over the blocks, and the best of the rule's order by one compare per candidate.  Prints one JSON line.
    python tools/bench_drift.py [--reps 5] [--sizes 2048,8192] [--torch_sizes 2048]
match_ms: drift.match on device tensors (luma, both kernels; GPU time between two HIP events, min of --reps after one warm-up).
torch_ms: the plain-torch path (one run after a warm-up at the smallest size); same_best: its (dy, dx, c, n) of the best equal the
table's."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topo4d_amd import drift  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[2048, 8192])
ap.add_argument("--torch_sizes", type=lambda s: [int(x) for x in s.split(",") if x], default=[2048])
a = ap.parse_args()
dev = torch.device("cuda")
B, S, R = 32, 16, 8
MIN = B * B // 2


def textures(n):
    g = torch.Generator(device=dev).manual_seed(n)
    f = torch.rand(1, 1, n, n, device=dev, generator=g)
    for _ in range(2):
        f = F.avg_pool2d(F.pad(f, (1, 1, 1, 1), mode="circular"), 3, 1)
    f = (f - f.min()) / (f.max() - f.min())
    a_img = (f[0, 0] * 255).round().to(torch.uint8)
    b_img = (torch.roll(f[0, 0], (3, -2), (0, 1)) * 0.8 * 255).round().to(torch.uint8)
    valid = torch.ones(n, n, dtype=torch.uint8, device=dev)
    labels = torch.ones(n, n, dtype=torch.uint8, device=dev)
    labels[:, n // 2] = 0
    labels[:, n // 2 + 1:] = 2
    return a_img, valid, b_img, valid, labels


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


POP = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.uint8, device=dev)


def torch_census(L, valid, labels):
    h, w = L.shape
    Li = L.to(torch.int16)
    inner = Li[3:h - 3, 3:w - 3]
    word = torch.zeros(h - 6, w - 6, dtype=torch.int64, device=dev)
    ok = labels[3:h - 3, 3:w - 3] != 0
    k = 0
    for j in range(-3, 4):
        for i in range(-3, 4):
            ok = ok & (valid[3 + j:h - 3 + j, 3 + i:w - 3 + i] != 0)
            if j == 0 and i == 0:
                continue
            word |= (Li[3 + j:h - 3 + j, 3 + i:w - 3 + i] < inner).to(torch.int64) << k
            k += 1
    C = torch.zeros(h, w, dtype=torch.int64, device=dev)
    O = torch.zeros(h, w, dtype=torch.bool, device=dev)
    C[3:h - 3, 3:w - 3], O[3:h - 3, 3:w - 3] = word, ok
    return C, O


def torch_match(a_img, va, b_img, vb, labels):
    """(dy, dx, c, n) int64 [nby,nbx] of the best by the rule, in plain torch"""
    h, w = a_img.shape
    Ca, oka = torch_census(a_img, va, labels)
    Cb, okb = torch_census(b_img, vb, labels)
    nby, nbx = drift.blocks(h, w, B, S)
    best = None
    order = sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda d: (d[0] * d[0] + d[1] * d[1], d[0], d[1]))
    for dy, dx in order:
        ya, yb, xa, xb = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        pair = torch.zeros(h, w, dtype=torch.float32, device=dev)
        ham = torch.zeros(h, w, dtype=torch.float32, device=dev)
        p, q = (slice(ya, yb), slice(xa, xb)), (slice(ya + dy, yb + dy), slice(xa + dx, xb + dx))
        pr = oka[p] & okb[q] & (labels[p] == labels[q])
        x = (Ca[p] ^ Cb[q]).contiguous()
        bits = POP[x.view(torch.uint8).reshape(x.shape + (8,)).long()].sum(-1, dtype=torch.float32)
        pair[p], ham[p] = pr.float(), torch.where(pr, bits, torch.zeros_like(bits))
        n = (F.avg_pool2d(pair[None, None], B, S)[0, 0] * (B * B)).round().long()
        c = (F.avg_pool2d(ham[None, None], B, S)[0, 0] * (B * B)).round().long()
        adm = n >= MIN
        if best is None:
            z = torch.zeros(nby, nbx, dtype=torch.int64, device=dev)
            best = [z.clone(), z.clone(), z.clone(), z.clone(), torch.zeros(nby, nbx, dtype=torch.bool, device=dev)]
        take = adm & (~best[4] | (c * best[3] < best[2] * n))
        best[0], best[1] = torch.where(take, dy, best[0]), torch.where(take, dx, best[1])
        best[2], best[3] = torch.where(take, c, best[2]), torch.where(take, n, best[3])
        best[4] = best[4] | take
    return torch.stack(best[:4], -1)


result = {"bench": "drift", "block": B, "stride": S, "radius": R, "sizes": {}}
if a.torch_sizes:
    torch_match(*textures(256))                               # warm-up: kernels and allocator
for n in a.sizes:
    inputs = textures(n)
    row = {}
    row["match_ms"], table = timed(lambda: drift.match(*inputs, block=B, stride=S, radius=R), a.reps)
    d, kept = drift.flow(table, R)
    row["blocks"] = int(kept.numel())
    row["kept_fraction"] = float(kept.double().mean())
    row["mean_d"] = d[kept].mean(0).cpu().tolist() if bool(kept.any()) else None
    if n in a.torch_sizes:
        row["torch_ms"], best = timed(lambda: torch_match(*inputs), 1)
        row["same_best"] = bool(torch.equal(best, table[..., :4].long()))
        del best
    result["sizes"][str(n)] = row
    del inputs, table, d, kept
    torch.cuda.empty_cache()
print(json.dumps(result))
