#!/usr/bin/env python
"""Applying a displacement map with topo4d_amd/tessellate.py (csrc/t4d_tessellate.hip) at the size of a tracked head: a
latitude-longitude sphere of 8,280 vertices and 16,376 triangles with a seam column in its UV layout, a 4096 x 4096 code map (a
smooth field over the whole layout, every island texel with a value), levels 4, 8 and 16, scored against a scan of 65,160 triangles.
Prints one JSON line.
    python tools/bench_tessellate.py [--reps 5] [--levels 4,8,16] [--res 4096]
Per level, time between two HIP events, min of --reps after one warm-up:
    topology_ms    tessellate.Tessellation (the host's edge tables, their upload, the index lists and the fine UVs)
    displace_ms    Tessellation.displace (the vertex normals and the displacement kernel)
    obj_ms         the bytes of face_hi.obj (objexport's "v", "vt" and "f" blocks, with their synchronisations and copies to the host)
    score_ms       scanscore.score_scan of the displaced mesh against the scan (both indices built, both directions)
    vertices, faces, unsampled, obj_bytes: the sizes
labels_ms is projtex.island_labels at the map's size, once."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from topo4d_amd import meshrender, objexport, projtex, scanscore, tessellate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--levels", type=lambda s: [int(x) for x in s.split(",")], default=[4, 8, 16])
ap.add_argument("--res", type=int, default=4096)
a = ap.parse_args()
dev = torch.device("cuda")
DIST = 0.01


def sphere(n_lat, n_lon, bump):
    """(vertices, faces) of a sphere without poles, radius 1 + bump sin(5 theta) cos(7 phi)"""
    th = (np.arange(n_lat) + 0.5) / n_lat * np.pi
    ph = np.arange(n_lon) / n_lon * 2 * np.pi
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = 1.0 + bump * np.sin(5 * T) * np.cos(7 * P)
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    p, q = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    f = np.concatenate([np.stack([p, p + n_lon, q], -1).reshape(-1, 3), np.stack([q, p + n_lon, q + n_lon], -1).reshape(-1, 3)])
    return np.ascontiguousarray(v), f.astype(np.int32)


def face_obj(n_lat, n_lon):
    """the sphere as a FaceObj: UV = (longitude, latitude), a second column of UV vertices at u = 1"""
    v, f = sphere(n_lat, n_lon, 0.0)
    u, w = np.arange(n_lon + 1) / n_lon, (np.arange(n_lat) + 0.5) / n_lat
    uvs = np.stack(np.meshgrid(w, u, indexing="ij")[::-1], -1).reshape(-1, 2)
    i, j = np.meshgrid(np.arange(n_lat - 1), np.arange(n_lon), indexing="ij")
    p = i * (n_lon + 1) + j
    q, r, s = p + 1, p + n_lon + 1, p + n_lon + 2
    uv_f = np.concatenate([np.stack([p, r, q], -1).reshape(-1, 3), np.stack([q, r, s], -1).reshape(-1, 3)])
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


def obj_bytes(tess, fine):
    return objexport._float_lines(fine, objexport.T4D_OBJ_V) + objexport._float_lines(tess.uvs, objexport.T4D_OBJ_VT) + \
        objexport._face_lines(tess.faces, tess.uv_faces, dev)


obj = face_obj(90, 92)
scan = scanscore.Scan(*sphere(180, 182, 0.004))
n = a.res
y, x = torch.meshgrid(torch.arange(n, device=dev), torch.arange(n, device=dev), indexing="ij")
code = (32768 + 13000 * torch.sin(5 * np.pi * (1.0 - y / (n - 1))) * torch.cos(14 * np.pi * x / (n - 1))).round().to(torch.int32)
del y, x
result = {"bench": "tessellate", "triangles": len(obj.faces_ori), "res": n, "dist": DIST, "scan_triangles": int(len(scan.faces)), "levels": {}}
result["labels_ms"], labels = timed(lambda: projtex.island_labels(obj, n, n, device=dev), 1)
has = (labels != 0).to(torch.uint8)
verts = torch.from_numpy(obj.vertices).to(dev)
unit = DIST / 32767
for level in a.levels:
    row = {}
    row["topology_ms"], tess = timed(lambda: tessellate.Tessellation(obj, level, device=dev), a.reps)
    row["displace_ms"], (fine, sampled) = timed(lambda: tess.displace(verts, code, has, labels, unit), a.reps)
    row["vertices"], row["faces"], row["unsampled"] = tess.n_vertices, tess.n_faces, tess.n_vertices - int(sampled.sum())
    row["obj_ms"], data = timed(lambda: obj_bytes(tess, fine), a.reps)
    row["obj_bytes"] = len(data)
    del data
    row["score_ms"], score = timed(lambda: scanscore.score_scan(fine, tess.faces, scan, unit=1000.0, device=dev), a.reps)
    row["scan_to_mesh_rms"] = score["scan_to_mesh"]["rms"]
    result["levels"][str(level)] = row
    print(json.dumps({str(level): row}), file=sys.stderr, flush=True)
    del tess, fine, sampled
    torch.cuda.empty_cache()
print(json.dumps(result))
