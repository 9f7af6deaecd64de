#!/usr/bin/env python
"""The temporal fusion kernels of topo4d_amd/seqtex.py (t4d_seqtex_select, t4d_seqtex_complete, csrc/t4d_seqtex.hip) at 2048 x 2048
and 8192 x 8192: random RGB frames, validity 0.9, the lower median of F = 16 and F = 64 frames, and one frame completed from the
base (tol 40), against the same rule in plain torch on the same device (stack, sort with the invalid samples keyed above 255,
gather).  Prints one JSON line.
    python tools/bench_seqtex.py [--reps 5] [--sizes 2048,8192] [--torch_sizes 2048] [--frames 16,64]
select_ms, complete_ms: seqtex.select and seqtex.complete on device tensors (GPU time between two HIP events, min of --reps after
one warm-up); *_gbs: the bytes the rule needs (select: F h w (c + 1) read, h w (c + 1) written; complete: the frame, its validity,
the base and the count read, the frame and its source written = 3 h w (c + 1)) over that time.  torch_ms: the plain-torch path
(one run after a warm-up at a small size); same: its results equal the kernel's.  The frames of the larger size are F distinct
tensors only while they fit `--max_gib` (default 24); beyond that the F pointers cycle through fewer tensors, which the entry
point allows and which changes what the caches see: "distinct" records how many there were."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topo4d_amd import seqtex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[2048, 8192])
ap.add_argument("--torch_sizes", type=lambda s: [int(x) for x in s.split(",") if x], default=[2048])
ap.add_argument("--frames", type=lambda s: [int(x) for x in s.split(",")], default=[16, 64])
ap.add_argument("--max_gib", type=float, default=24.0)
a = ap.parse_args()
dev = torch.device("cuda")
C = 3


def inputs(n, F):
    g = torch.Generator(device=dev).manual_seed(n + F)
    distinct = max(1, min(F, int(a.max_gib * 2 ** 30 / (n * n * (C + 1)))))
    images = [torch.randint(0, 256, (n, n, C), device=dev, generator=g, dtype=torch.uint8) for _ in range(distinct)]
    valids = [(torch.rand(n, n, device=dev, generator=g) < 0.9).to(torch.uint8) for _ in range(distinct)]
    return [images[t % distinct] for t in range(F)], [valids[t % distinct] for t in range(F)], distinct


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


def torch_select(images, valids, num=1, den=2):
    v = torch.stack(valids) != 0
    n = v.sum(0)
    k = (torch.clamp(n - 1, min=0) * num) // den
    keyed = torch.where(v[..., None], torch.stack(images).to(torch.int16), torch.full((), 256, dtype=torch.int16, device=dev))
    srt = torch.sort(keyed, dim=0).values
    out = torch.gather(srt, 0, k[None, ..., None].expand(1, *srt.shape[1:]))[0]
    return torch.where(n[..., None] > 0, out, torch.zeros_like(out)).to(torch.uint8), n.to(torch.uint8)


def torch_complete(image, valid, base, count, min_count, min_votes, tol):
    v = valid != 0
    far = (image.to(torch.int16) - base.to(torch.int16)).abs().amax(-1)
    own = v & ~((count >= min_votes) & (far > tol))
    fused = ~own & (count >= min_count)
    source = torch.where(own, 1, torch.where(fused, torch.where(v, 3, 2), 0)).to(torch.uint8)
    pick = source[..., None]
    return torch.where(pick == 1, image, torch.where(pick != 0, base, torch.zeros_like(base))), source


result = {"bench": "seqtex", "channels": C, "validity": 0.9, "quantile": [1, 2], "sizes": {}}
if a.torch_sizes:
    small = inputs(256, 4)                                     # warm-up: kernels and allocator
    torch_complete(small[0][0], small[1][0], *torch_select(small[0], small[1]), 1, 3, 40)
for n in a.sizes:
    row = {}
    for F in a.frames:
        images, valids, distinct = inputs(n, F)
        r = {"distinct": distinct}
        r["select_ms"], (base, count) = timed(lambda: seqtex.select(images, valids, (1, 2)), a.reps)
        r["select_gbs"] = round((F + 1.0) * n * n * (C + 1) / r["select_ms"] / 1e6, 1)
        r["complete_ms"], (full, source) = timed(lambda: seqtex.complete(images[0], valids[0], base, count, 1, 3, 40), a.reps)
        r["complete_gbs"] = round(3.0 * n * n * (C + 1) / r["complete_ms"] / 1e6, 1)
        r["covered_fraction"] = float((count > 0).double().mean())
        if n in a.torch_sizes:
            r["torch_select_ms"], (t_base, t_count) = timed(lambda: torch_select(images, valids), 1)
            r["torch_complete_ms"], (t_full, t_source) = timed(lambda: torch_complete(images[0], valids[0], base, count, 1, 3, 40), 1)
            r["same"] = bool(torch.equal(t_base, base) and torch.equal(t_count, count) and torch.equal(t_full, full) and torch.equal(t_source, source))
            r["select_speedup"] = round(r["torch_select_ms"] / r["select_ms"], 1)
            del t_base, t_count, t_full, t_source
        row[f"F{F}"] = r
        del images, valids, base, count, full, source
        torch.cuda.empty_cache()
    result["sizes"][str(n)] = row
print(json.dumps(result))
