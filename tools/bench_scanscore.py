#!/usr/bin/env python
"""Scoring one frame's mesh against its 3D scan (topo4d_amd/scanscore.py over csrc/t4d_closest.hip): a 90 x 92 bumpy sphere
(8,280 vertices, 16,376 triangles: G15's size) and 2,000,000 seeded scan points at 0.9 - 1.1 of its radius.  Prints one JSON line.
    python tools/bench_scanscore.py [--reps 5] [--points 2000000] [--no-cpu] [--rocprof]
Two cases: scan_to_mesh (16 k triangles indexed, 2 M queries) and mesh_to_scan (2 M points indexed, 8,280 queries).  Per case
build_ms (t4d_closest_build, wall: it synchronises), query_ms with the queries grouped by cell and in input order (GPU time between
two HIP events, min of --reps after one warm-up), and signed_ms.  wall_ms: scanscore.score_scan from numpy arrays to host numbers
(upload, both indices, both queries, statistics; the second of two runs).  cpu: what exists without this feature, for context -
scipy's cKDTree on 16 threads, which answers an easier question (the nearest VERTEX, not the nearest point of a triangle), and
the numpy yardstick (tests/scanscore_ref.py) on 256 queries, scaled to all of them.  --rocprof: the per-kernel split from a
rocprofv3 --kernel-trace --stats run of the query loop (a child process)."""
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
from topo4d_amd import scanscore  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--points", type=int, default=2_000_000)
ap.add_argument("--no-cpu", action="store_true")
ap.add_argument("--rocprof", action="store_true")
ap.add_argument("--kernels-only", action="store_true", help=argparse.SUPPRESS)   # (the child of --rocprof)
a = ap.parse_args()
dev = torch.device("cuda")


def bumpy_sphere(n_lat=90, n_lon=92):
    th = (np.arange(n_lat) + 0.5) / n_lat * np.pi
    ph = np.arange(n_lon) / n_lon * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = 1.0 + 0.03 * np.sin(5 * T) * np.cos(7 * P)
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    p, q = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    f = np.concatenate([np.stack([p, p + n_lon, q], -1).reshape(-1, 3), np.stack([q, p + n_lon, q + n_lon], -1).reshape(-1, 3)])
    return np.ascontiguousarray(v), f.astype(np.int32)


def scan_points(n, seed=31):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * rng.uniform(0.9, 1.1, (n, 1))


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


def case(prim_v, prim_f, queries, reps):
    pv, qd = torch.from_numpy(prim_v).to(dev), torch.from_numpy(queries).to(dev)
    builds = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = scanscore.ClosestPointIndex(pv, prim_f, device=dev)
        torch.cuda.synchronize()
        builds.append(1e3 * (time.perf_counter() - t0))
    res = {"primitives": index.n_prims, "triangles": index.is_tri, "queries": len(queries), "list_entries": index.entries,
           "build_ms": round(min(builds[1:]), 3)}
    res["query_ms"], out = timed(lambda: index.query(qd), reps)
    res["query_input_order_ms"], out2 = timed(lambda: index.query(qd, input_order=True), reps)
    res["same_results"] = all(torch.equal(x, y) for x, y in zip(out, out2))
    res["signed_ms"], _ = timed(lambda: index.signed_distance(qd, *out), reps)
    res["mean_distance"] = float(torch.sqrt(out[0]).mean())
    return res


v, f = bumpy_sphere()
pts = scan_points(a.points)
if a.kernels_only:
    case(v, f, pts, a.reps)
    case(pts, None, v, a.reps)
    torch.cuda.synchronize()
    sys.exit(0)

result = {"bench": "scanscore", "scan_to_mesh": case(v, f, pts, a.reps), "mesh_to_scan": case(pts, None, v, a.reps)}
walls = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    score = scanscore.score_scan(v, f, scanscore.Scan(pts, None), device=dev)
    walls.append(1e3 * (time.perf_counter() - t0))
result["wall_ms"] = {"score_scan": round(walls[-1], 1), "first_run": round(walls[0], 1)}
result["score"] = {d: {k: score[d][k] for k in ("count", "mean", "rms", "max")} for d in score}

if not a.no_cpu:
    from scipy.spatial import cKDTree
    from tests import scanscore_ref as ref
    t0 = time.perf_counter()
    tree = cKDTree(v)
    tree.query(pts, workers=16)
    t1 = time.perf_counter()
    cKDTree(pts).query(v, workers=16)
    t2 = time.perf_counter()
    sub = 256
    ref.closest_point(pts[:sub], v, f)
    t3 = time.perf_counter()
    result["cpu"] = {"ckdtree_nearest_vertex_scan_to_mesh_ms": round(1e3 * (t1 - t0), 1),
                     "ckdtree_nearest_point_mesh_to_scan_ms": round(1e3 * (t2 - t1), 1),
                     "yardstick_scan_to_mesh_scaled_s": round((t3 - t2) * len(pts) / sub, 1), "yardstick_queries": sub,
                     "note": "cKDTree finds the nearest vertex, not the nearest point of a triangle"}

if a.rocprof:
    d = tempfile.mkdtemp(prefix="t4d_bench_ss_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
           sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--points", str(a.points), "--kernels-only"]
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600).returncode
    stats = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"(k_closest_\w+)", row["Name"])
                if m:
                    stats[m.group(1)] = dict(calls=int(row["Calls"]), total_ms=round(float(row["TotalDurationNs"]) / 1e6, 3),
                                             avg_us=round(float(row["AverageNs"]) / 1e3, 1))
    result["rocprof"] = dict(rc=rc, kernels=stats, note="totals over both cases: 3 builds and 3 x (reps + 1) launches each")
print(json.dumps(result))
