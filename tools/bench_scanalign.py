#!/usr/bin/env python
"""Aligning one frame's 3D scan to its mesh (topo4d_amd/scanalign.py over csrc/t4d_align.hip and csrc/t4d_closest.hip): a 90 x 92
bumpy sphere (8,280 vertices, 16,376 triangles: G15's size) and 2,000,000 seeded scan points within 0.2 % of its surface, turned
by 1 degree and moved by 1 % of its radius.  Writes profiles/scanalign_bench.json and prints it as one JSON line.
    python tools/bench_scanalign.py [--reps 5] [--points 2000000] [--out profiles/scanalign_bench.json] [--rocprof]
Per stride (1: all points, 8: every eighth) the three device steps of one iteration at the starting pose - transform_ms, query_ms,
accumulate_ms - as GPU time between two HIP events, min of --reps after one warm-up, the same record's sums stated in plain torch
(torch_accumulate_ms: gathers, elementwise float64, one sum per entry; it agrees with the kernel to rounding, not to the bit), and
align_scan_ms: a whole align_scan from numpy arrays to the Alignment on the host (wall clock, the second of two runs: index build,
upload, every iteration with its read-back and host solve).  --rocprof: the per-kernel split of the three device steps, per
stride, from a rocprofv3 --kernel-trace --stats run of those steps alone (a child process each)."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topo4d_amd import scanalign, scanscore  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--points", type=int, default=2_000_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scanalign_bench.json"))
ap.add_argument("--rocprof", action="store_true")
ap.add_argument("--kernels-only", type=int, default=0, metavar="STRIDE", help=argparse.SUPPRESS)   # (the child of --rocprof)
a = ap.parse_args()
dev = torch.device("cuda")


def radius(T, P):
    return 1.0 + 0.03 * np.sin(5 * T) * np.cos(7 * P)


def bumpy_sphere(n_lat=90, n_lon=92):
    th = (np.arange(n_lat) + 0.5) / n_lat * np.pi
    ph = np.arange(n_lon) / n_lon * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = radius(T, P)
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    p, q = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    f = np.concatenate([np.stack([p, p + n_lon, q], -1).reshape(-1, 3), np.stack([q, p + n_lon, q + n_lon], -1).reshape(-1, 3)])
    return np.ascontiguousarray(v), f.astype(np.int32)


def scan_points(n, seed=31):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    T, P = np.arccos(np.clip(d[:, 2], -1.0, 1.0)), np.arctan2(d[:, 1], d[:, 0])
    return d * (radius(T, P) * (1.0 + rng.normal(size=n) * 0.002))[:, None]


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


def torch_record(tri, p, d2, idx, cl, origin, gate2, cos2):
    """the record's sums in plain torch: tri float64 [F,3,3] corners"""
    matched = idx >= 0
    t = tri[torch.where(matched, idx, torch.zeros_like(idx)).long()]
    n = torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nn = (n * n).sum(1)
    e = p - cl
    en = (e * n).sum(1)
    gated = (d2 > gate2) if gate2 >= 0 else torch.zeros_like(matched)
    off = (d2 > 0) & (en * en < cos2 * d2 * nn)
    cls = torch.where(~matched, 0, torch.where(gated, 1, torch.where(nn == 0, 2, torch.where(off, 3, 4))))
    keep = cls == 4
    nh = n / torch.sqrt(nn)[:, None]
    r = (e * nh).sum(1)
    q, g = p - origin, cl - origin
    J = torch.cat([torch.linalg.cross(q, nh), nh], 1)
    iu = torch.triu_indices(6, 6, device=p.device)
    cols = [d2[:, None], (r * r)[:, None], r[:, None] * J, J[:, iu[0]] * J[:, iu[1]], q, g, (q[:, :, None] * g[:, None, :]).reshape(-1, 9),
            (q * q).sum(1, keepdim=True), (g * g).sum(1, keepdim=True)]
    terms = torch.where(keep[:, None], torch.cat(cols, 1), torch.zeros((), dtype=p.dtype, device=p.device))
    return torch.cat([torch.bincount(cls, minlength=5).to(p.dtype), terms.sum(0)])


v, f = bumpy_sphere()
pts = scan_points(a.points)
move = np.eye(4)
move[:3, :3] = scanalign.rodrigues(np.radians([0.6, -0.5, 0.6]))
move[:3, 3] = (0.006, -0.005, 0.006)
scan = pts @ move[:3, :3].T + move[:3, 3]
origin = v.mean(0)
index = scanscore.ClosestPointIndex(torch.from_numpy(v).to(dev), f, device=dev)
tri = torch.from_numpy(v[f]).to(dev)
od = torch.from_numpy(origin).to(dev)
result = {"bench": "scanalign", "triangles": int(len(f)), "points": int(a.points), "reps": a.reps, "strides": {}}
for stride in ((a.kernels_only,) if a.kernels_only else (1, 8)):
    p0 = torch.from_numpy(np.ascontiguousarray(scan[::stride])).to(dev)
    moved = torch.empty_like(p0)
    row = {"points": int(p0.shape[0])}
    row["transform_ms"], _ = timed(lambda: scanalign.transform_points(p0, np.eye(4), out=moved), a.reps)
    row["query_ms"], (d2, idx, cl) = timed(lambda: index.query(moved), a.reps)
    gate2, cos2 = 0.03 ** 2, 0.25
    row["accumulate_ms"], rec = timed(lambda: scanalign.accumulate(index, moved, d2, idx, cl, origin, gate2, cos2), a.reps)
    if a.kernels_only:
        torch.cuda.synchronize()
        sys.exit(0)
    row["torch_accumulate_ms"], trec = timed(lambda: torch_record(tri, moved, d2, idx, cl, od, gate2, cos2), a.reps)
    rec, trec = rec.cpu().numpy(), trec.cpu().numpy()
    row["counts"] = dict(zip(scanalign.CLASSES, (int(x) for x in rec[:5])))
    row["torch_counts_equal"] = bool((rec[:5] == trec[:5]).all())
    row["torch_max_rel_diff"] = float(np.max(np.abs(rec[5:] - trec[5:]) / np.maximum(np.abs(rec[5:]), 1e-300)))
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = scanalign.align_scan(v, f, scan, stride=stride, device=dev)
        walls.append(1e3 * (time.perf_counter() - t0))
    row["align_scan_ms"], row["align_scan_first_run_ms"] = round(walls[1], 1), round(walls[0], 1)
    row["alignment"] = {k: out.as_dict()[k] for k in ("iterations", "converged", "counts", "rms_before", "rms_after", "rotation_deg")}
    truth = np.linalg.inv(move)
    row["translation_error"] = float(np.linalg.norm(out.matrix[:3, 3] - truth[:3, 3]))
    row["rotation_error_rad"] = float(np.linalg.norm(out.matrix[:3, :3] @ truth[:3, :3].T - np.eye(3)) / np.sqrt(2.0))
    result["strides"][str(stride)] = row
if a.rocprof:
    for stride in (1, 8):
        d = tempfile.mkdtemp(prefix="t4d_bench_sa_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
               sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--points", str(a.points), "--kernels-only", str(stride)]
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600).returncode
        stats = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for r in csv.DictReader(fh):
                    m = re.search(r"(k_align_\w+|k_closest_\w+)", r["Name"])
                    if m:
                        stats[m.group(1)] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 1),
                                                 min_us=round(float(r["MinNs"]) / 1e3, 1))
        result["strides"][str(stride)]["rocprof"] = dict(rc=rc, kernels=stats, note="reps + 1 launches of each step; the index's build included")
line = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(line + "\n")
print(line)
