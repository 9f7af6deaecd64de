#!/usr/bin/env python
"""Baking one frame's scan into a displacement map (topo4d_amd/scanbake.py over t4d_closest_raycast, csrc/t4d_closest.hip): the
90 x 92 bumpy sphere (8,280 vertices: G15's size) with a latitude-longitude UV layout, baked at 8192 x 8192 against a
1000 x 1000 bumpy sphere (1,998,000 triangles) with a reach of three mean scan edge lengths.  Prints one JSON line.
    python tools/bench_scanbake.py [--reps 3] [--res 8192] [--scan 1000]
build_ms: t4d_closest_build over the scan (wall: it synchronises).  raycast_ms: the cast of every covered texel's ray, grouped
by cell and in input order (GPU time between two HIP events, min of --reps after one warm-up), and closest_query_ms: the
existing closest-point query over the same origins, the yardstick for the cast.  wall_ms: scanbake.bake_displacement from
numpy arrays to the three maps on the device (surface maps, upload, index, cast; the second of two runs)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topo4d_amd import meshrender, projtex, scanbake, scanscore  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--res", type=int, default=8192)
ap.add_argument("--scan", type=int, default=1000, help="the scan is a SCAN x SCAN bumpy sphere: 2 (SCAN - 1) SCAN triangles")
a = ap.parse_args()
dev = torch.device("cuda")


def bumpy_sphere(n_lat, n_lon):
    th = (np.arange(n_lat) + 0.5) / n_lat * np.pi
    ph = np.arange(n_lon) / n_lon * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = 1.0 + 0.03 * np.sin(5 * T) * np.cos(7 * P)
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    p, q = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    f = np.concatenate([np.stack([p, p + n_lon, q], -1).reshape(-1, 3), np.stack([q, p + n_lon, q + n_lon], -1).reshape(-1, 3)])
    return np.ascontiguousarray(v), f.astype(np.int32)


def sphere_obj(n_lat, n_lon):
    """The sphere as a FaceObj with UV = (longitude, latitude) and a second column of UV vertices at u = 1."""
    v, f = bumpy_sphere(n_lat, n_lon)
    uvs = np.stack(np.meshgrid((np.arange(n_lat) + 0.5) / n_lat, np.arange(n_lon + 1) / n_lon, indexing="ij")[::-1], -1).reshape(-1, 2)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    p, q = i * (n_lon + 1) + j, i * (n_lon + 1) + j + 1
    uv_f = np.concatenate([np.stack([p, p + n_lon + 1, q], -1).reshape(-1, 3), np.stack([q, p + n_lon + 1, q + n_lon + 1], -1).reshape(-1, 3)])
    return meshrender.FaceObj(v, uvs, f.tolist(), uv_f.tolist())


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


obj = sphere_obj(90, 92)
sv, sf = bumpy_sphere(a.scan, a.scan)
c = sv[sf]
edge = float(np.mean([np.linalg.norm(c[:, i] - c[:, j], axis=1).mean() for i, j in ((0, 1), (1, 2), (2, 0))]))
dist = 3.0 * edge
del c
verts = torch.from_numpy(obj.vertices).to(dev)
svd = torch.from_numpy(sv).to(dev)
builds = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = scanscore.ClosestPointIndex(svd, sf, device=dev)
    torch.cuda.synchronize()
    builds.append(1e3 * (time.perf_counter() - t0))
texel, o, d = scanbake.texel_rays(*projtex.surface_maps(obj, verts, a.res, device=dev))
result = {"bench": "scanbake", "res": a.res, "rays": int(texel.numel()), "scan_triangles": index.n_prims, "list_entries": index.entries,
          "dist": dist, "mean_scan_edge": edge, "build_ms": round(min(builds[1:]), 3)}
result["raycast_ms"], out = timed(lambda: index.raycast(o, d, -dist, dist, same_side=True), a.reps)
result["raycast_input_order_ms"], out2 = timed(lambda: index.raycast(o, d, -dist, dist, same_side=True, input_order=True), a.reps)
result["same_results"] = all(torch.equal(x, y) for x, y in zip(out, out2))
result["hit_fraction"] = float((out[1] >= 0).double().mean())
result["mean_abs_t"] = float(out[0].abs().mean())
del out2
result["closest_query_ms"], _ = timed(lambda: index.query(o, max_dist=dist), a.reps)
result["closest_query_input_order_ms"], _ = timed(lambda: index.query(o, max_dist=dist, input_order=True), a.reps)
del index, out, o, d, texel, _
walls = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    maps = scanbake.bake_displacement(obj, verts, scanscore.Scan(sv, sf), a.res, dist, device=dev)
    torch.cuda.synchronize()
    walls.append(1e3 * (time.perf_counter() - t0))
    del maps
result["wall_ms"] = {"bake_displacement": round(walls[-1], 1), "first_run": round(walls[0], 1)}
print(json.dumps(result))
