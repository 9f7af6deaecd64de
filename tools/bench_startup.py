#!/usr/bin/env python
"""Fitting the startup mesh to a scan (topo4d_amd/startup.py over csrc/t4d_nricp.hip and csrc/t4d_closest.hip): a 90 x 92 bumpy
sphere as template (8,280 vertices, 16,376 triangles: G15's size) and 2,000,000 seeded points on a smoothly deformed copy of
it as the scan, a cloud.  Writes profiles/startup_bench.json and prints it as one JSON line.
    python tools/bench_startup.py [--reps 5] [--points 2000000] [--out profiles/startup_bench.json] [--no-host]
GPU time between two HIP events, min of --reps after one warm-up, at the first outer step of the default schedule (stiffness 50):
classify_ms (t4d_nricp_classify on a finished query), query_ms (the closest-point query it follows), cg_iteration_ms (a run of
64 iterations / 64: three launches each), solve_ms (startup.solve to tol 1e-8: start, runs of 32 iterations, the read-backs of
the 40-double record between them) with its iteration count; fit_ms: a whole fit_template from numpy arrays (wall clock, the
second of two runs, init given, scoring off).  The host yardstick is the same outer step with scipy: the same system assembled
as a sparse matrix and solved by scipy.sparse.linalg.spsolve for the three columns (host_spsolve_ms, wall clock, once), and the
largest difference between the two solutions."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topo4d_amd import scanscore, startup  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--points", type=int, default=2_000_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "startup_bench.json"))
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")


def radius(T, P, bump):
    return 1.0 + 0.03 * np.sin(5 * T) * np.cos(7 * P) + bump * np.sin(2 * T + 0.3) * np.cos(3 * P - 0.2)


def bumpy_sphere(n_lat=90, n_lon=92):
    th = (np.arange(n_lat) + 0.5) / n_lat * np.pi
    ph = np.arange(n_lon) / n_lon * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = radius(T, P, 0.0)
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
    return d * radius(T, P, 0.02)[:, None]


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


class Mesh:
    pass


mesh = Mesh()
mesh.vertices, mesh.faces = bumpy_sphere()
scan = scanscore.Scan(scan_points(a.points), None)
n = len(mesh.vertices)
result = {"bench": "startup", "vertices": n, "triangles": int(len(mesh.faces)), "points": int(a.points), "reps": a.reps}

# the first outer step, piece by piece, in the normalised frame of fit_template
centre, diag = startup.frame_of(mesh.vertices)
on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
v = on((mesh.vertices - centre) / diag)
off_np, nbr_np = startup.neighbour_csr(mesh.faces, n)
off, nbr = on(off_np), on(nbr_np)
index = scanscore.ClosestPointIndex(on((scan.vertices - centre) / diag), None, device=dev)
result["query_ms"], (d2, prim, closest) = timed(lambda: index.query(v), a.reps)
result["classify_ms"], (cls, w, target, record) = timed(lambda: startup.classify(index, v, d2, prim, closest, None, None, -1.0, 0.25, 0.5), a.reps)
result["counts"] = dict(zip(startup.CLASSES, (int(x) for x in record.cpu().numpy()[:7])))
a2 = 50.0 * 50.0
s, b, chol = startup.assemble(v, off, w, target, None, None, a2, a2, 0.0)
x = startup.identity_field(n, dev)
cg = startup.cg_start(v, off, nbr, s, a2, a2, chol, b, x.clone())
ms, _ = timed(lambda: startup.cg_run(v, off, nbr, s, a2, a2, chol, cg, 0, 64), a.reps)
result["cg_iteration_ms"] = round(ms / 64, 5)


def one_solve():
    xs = x.clone()
    return xs, startup.solve(v, off, nbr, s, a2, a2, chol, b, xs, 1e-8, 4000, 32)


result["solve_ms"], (xs, (iters, rel)) = timed(one_solve, a.reps)
result["solve_iterations"], result["solve_residuals"] = iters, rel
walls = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = startup.fit_template(mesh, scan, init=np.eye(4), score=False, device=dev)
    walls.append(1e3 * (time.perf_counter() - t0))
result["fit_ms"], result["fit_first_run_ms"] = round(walls[1], 1), round(walls[0], 1)
result["fit_steps"] = len(fit.steps)
result["fit_cg_iterations"] = int(sum(max(r["cg_iterations"]) for r in fit.steps))
result["fit_rms_first_last"] = [fit.steps[0]["rms"], fit.steps[-1]["rms"]]
result["fit_turned_triangles"] = len(fit.flipped_triangles)

if not a.no_host:
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    t0 = time.perf_counter()
    deg = np.diff(off_np).astype(np.float64)
    rows = np.repeat(np.arange(n), np.diff(off_np))
    lap = sp.diags(deg) - sp.coo_matrix((np.ones(len(nbr_np)), (rows, nbr_np)), shape=(n, n))
    vt = np.concatenate([v.cpu().numpy(), np.ones((n, 1))], 1)
    sn = s.cpu().numpy()
    data = sp.block_diag([sn[i] * np.outer(vt[i], vt[i]) for i in range(n)], format="csc")
    K = (sp.kron(lap, sp.diags([a2, a2, a2, a2])) + data).tocsc()
    B = np.transpose(b.cpu().numpy(), (2, 1, 0)).reshape(-1, 3)
    t1 = time.perf_counter()
    X = spsolve(K, B)
    t2 = time.perf_counter()
    result["host_assemble_ms"], result["host_spsolve_ms"] = round(1e3 * (t1 - t0), 1), round(1e3 * (t2 - t1), 1)
    result["host_max_abs_diff"] = float(np.abs(X - np.transpose(xs.cpu().numpy(), (2, 1, 0)).reshape(-1, 3)).max())
line = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write(line + "\n")
print(line)
