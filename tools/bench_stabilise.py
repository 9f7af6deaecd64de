#!/usr/bin/env python
"""The stabilisation kernels of topo4d_amd/drift.py (t4d_drift_dense, t4d_drift_warp, csrc/t4d_stabilise.hip) at 2048 x 2048 and
8192 x 8192: the nodes of block 32, stride 16 at level 2, reach 1, a smooth displacement field of up to 6 level texels, two islands,
an RGB texture, against the same rule in plain torch on the same device: per texel the (2 reach)^2 nodes by index arithmetic and
gathers in int64, then the four taps by whole-image gathers.  Prints one JSON line.
    python tools/bench_stabilise.py [--reps 5] [--sizes 2048,8192] [--torch_sizes 2048] [--reach 1]
dense_ms, warp_ms, both_ms: drift.dense_flow (check=False, as stabilise_pair calls it: the test of d's values would wait for the
device), drift.warp and one after the other on device tensors (GPU time between two HIP events, min of --reps after one warm-up);
*_gbs: the bytes the rule needs (dense: labels in, flow and support out = 10 B per texel; warp: flow, labels and one of validity, image and labels per texel in, image and validity out = 17 B per texel at c = 3)
over that time.  torch_*_ms: the plain-torch path (one run after a warm-up at a small size); same: its results equal the kernels'."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topo4d_amd import drift  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[2048, 8192])
ap.add_argument("--torch_sizes", type=lambda s: [int(x) for x in s.split(",") if x], default=[2048])
ap.add_argument("--reach", type=int, default=1)
a = ap.parse_args()
dev = torch.device("cuda")
B, S, L = 32, 16, 2


def inputs(n):
    g = torch.Generator(device=dev).manual_seed(n)
    nby, nbx = drift.blocks(n >> L, n >> L, B, S)
    d = torch.rand(1, 2, nby, nbx, device=dev, generator=g, dtype=torch.float64)
    for _ in range(2):
        d = F.avg_pool2d(F.pad(d, (1, 1, 1, 1), mode="replicate"), 3, 1)
    d = ((d - d.mean()) * 24.0).clamp(-6.0, 6.0)[0].permute(1, 2, 0).contiguous()
    kept = torch.rand(nby, nbx, device=dev, generator=g) < 0.9
    labels = torch.ones(n, n, dtype=torch.uint8, device=dev)
    labels[:, n // 2] = 0
    labels[:, n // 2 + 1:] = 2
    image = torch.randint(0, 256, (n, n, 3), device=dev, generator=g, dtype=torch.uint8)
    valid = (torch.rand(n, n, device=dev, generator=g) < 0.98).to(torch.uint8)
    return d, kept, labels, image, valid


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


def torch_dense(d, kept, labels, reach):
    H, W = labels.shape
    nby, nbx = kept.shape
    q = drift.node_values(d, L).to(torch.int64)
    P, c0, T = S << (L + 1), ((B // 2) << (L + 1)) - 1, reach * (S << (L + 1))
    cy = ((torch.arange(nby, device=dev) * S + B // 2) << L)
    cx = ((torch.arange(nbx, device=dev) * S + B // 2) << L)
    node_label = labels[cy[:, None], cx[None, :]].to(torch.int64)
    part = torch.where(kept & (node_label != 0), node_label, torch.zeros_like(node_label))
    y2, x2 = 2 * torch.arange(H, device=dev)[:, None], 2 * torch.arange(W, device=dev)[None, :]
    fy, fx = torch.div(y2 - T - c0 + P, P, rounding_mode="floor"), torch.div(x2 - T - c0 + P, P, rounding_mode="floor")
    lab = labels.to(torch.int64)
    num = torch.zeros(H, W, 2, dtype=torch.int64, device=dev)
    den = torch.zeros(H, W, dtype=torch.int64, device=dev)
    for j in range(2 * reach):
        by = fy + j
        wy = (T - (y2 - (P * by + c0)).abs()).clamp(min=0) * ((by >= 0) & (by < nby))
        byc = by.clamp(0, nby - 1).expand(H, W)
        for i in range(2 * reach):
            bx = fx + i
            wx = (T - (x2 - (P * bx + c0)).abs()).clamp(min=0) * ((bx >= 0) & (bx < nbx))
            bxc = bx.clamp(0, nbx - 1).expand(H, W)
            w = wy * wx * ((part[byc, bxc] == lab) & (lab != 0))
            den += w
            num += w[..., None] * q[byc, bxc]
    has = den > 0
    safe = torch.where(has, den, torch.ones_like(den))[..., None]
    flow = torch.where(has[..., None], torch.div(2 * num + den[..., None], 2 * safe, rounding_mode="floor"), torch.zeros_like(num))
    return flow.to(torch.int32), has.to(torch.uint8)


def torch_warp(image, valid, labels, flow):
    H, W = labels.shape
    y, x = torch.arange(H, device=dev)[:, None], torch.arange(W, device=dev)[None, :]
    Y, X = 256 * y + flow[..., 0].long(), 256 * x + flow[..., 1].long()
    y0, x0, ty, tx = Y >> 8, X >> 8, Y & 255, X & 255
    total = torch.zeros(H, W, dtype=torch.int64, device=dev)
    s = torch.zeros(image.shape, dtype=torch.int64, device=dev)
    for k, wa in ((0, 256 - ty), (1, ty)):
        for m, wb in ((0, 256 - tx), (1, tx)):
            yy, xx = y0 + k, x0 + m
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            yc, xc = yy.clamp(0, H - 1), xx.clamp(0, W - 1)
            w = wa * wb * (inside & (valid[yc, xc] != 0) & (labels[yc, xc] == labels) & (labels != 0))
            total += w
            s += w[..., None] * image[yc, xc]
    has = total > 0
    safe = torch.where(has, total, torch.ones_like(total))[..., None]
    out = torch.where(has[..., None], torch.div(2 * s + total[..., None], 2 * safe, rounding_mode="floor"), torch.zeros_like(s))
    return out.to(torch.uint8), has.to(torch.uint8)


result = {"bench": "stabilise", "block": B, "stride": S, "level": L, "reach": a.reach, "sizes": {}}
if a.torch_sizes:
    small = inputs(256)                                       # warm-up: kernels and allocator
    torch_warp(small[3], small[4], small[2], torch_dense(small[0], small[1], small[2], a.reach)[0])
for n in a.sizes:
    d, kept, labels, image, valid = inputs(n)
    row = {}
    row["dense_ms"], (flow, support) = timed(lambda: drift.dense_flow(d, kept, labels, B, S, L, a.reach, check=False), a.reps)
    row["warp_ms"], (out, out_valid) = timed(lambda: drift.warp(image, valid, labels, flow), a.reps)
    row["both_ms"], _ = timed(lambda: drift.warp(image, valid, labels, drift.dense_flow(d, kept, labels, B, S, L, a.reach, check=False)[0]), a.reps)
    row["dense_gbs"] = round(10.0 * n * n / row["dense_ms"] / 1e6, 1)
    row["warp_gbs"] = round(17.0 * n * n / row["warp_ms"] / 1e6, 1)
    row["support_fraction"] = float(support.double().mean())
    row["valid_fraction"] = float(out_valid.double().mean())
    if n in a.torch_sizes:
        row["torch_dense_ms"], (t_flow, t_support) = timed(lambda: torch_dense(d, kept, labels, a.reach), 1)
        row["torch_warp_ms"], (t_out, t_valid) = timed(lambda: torch_warp(image, valid, labels, flow), 1)
        row["same"] = bool(torch.equal(t_flow, flow) and torch.equal(t_support, support) and torch.equal(t_out, out)
                           and torch.equal(t_valid, out_valid))
        del t_flow, t_support, t_out, t_valid
    result["sizes"][str(n)] = row
    del d, kept, labels, image, valid, flow, support, out, out_valid
    torch.cuda.empty_cache()
print(json.dumps(result))
