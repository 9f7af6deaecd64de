#!/usr/bin/env python
"""face.obj export on the GPU (topo4d_amd/objexport.py, csrc/t4d_obj.hip) against the restated Python path of helpers.save_mesh
(tests/objexport_ref.py: trimesh's normals restated in numpy, build_rotation / torch.linalg.inv / the clamp in torch, the float64
transform and the f-string writer) on an 8,280-vertex scaffold head: 69 x 120 lat-long vertices, 8,160 quads with a UV seam and
8,349 UVs.  Prints one JSON line.
    python tools/bench_objexport.py [--reps 20] [--no-cpu]
gpu_bytes_ms[frame]: device-resident params -> the whole face.obj as bytes in host memory (MeshExporter.obj_bytes, median of
--reps); gpu_file_ms[frame]: MeshExporter.save_mesh(gen_texture=False) into a temporary directory (median); setup_ms: building
the MeshExporter (checks, CSR, the static vt / f bytes); cpu_bytes_ms / cpu_file_ms: the restated Python path on the host
(params already on the host, median of 3); obj_bytes: the size of the frame-2 file; frame1_lines_differing_from_cpu: "v" lines
whose last digits differ (numpy's matrix product may round the transform differently; the tests bound it by 4 ulp)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import objexport_ref as ref  # noqa: E402
from topo4d_amd import objexport  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-cpu", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda")


def head(n_lat=69, n_lon=120, seed=11):
    from scaffold import scene
    params = scene.make_gaussians(n_lat, n_lon, opacity="A", seed=seed)
    v = lambda i, j: i * n_lon + (j % n_lon)
    uvs = [[j / n_lon, i / (n_lat - 1)] for i in range(n_lat) for j in range(n_lon)] + [[1.0, i / (n_lat - 1)] for i in range(n_lat)]
    u = lambda i, j: n_lat * n_lon + i if j == n_lon else v(i, j)
    faces = [[v(i, j), v(i + 1, j), v(i + 1, j + 1), v(i, j + 1)] for i in range(n_lat - 1) for j in range(n_lon)]
    uv_faces = [[u(i, j), u(i + 1, j), u(i + 1, j + 1), u(i, j + 1)] for i in range(n_lat - 1) for j in range(n_lon)]
    tri = np.asarray([t for f in faces for t in ([f[0], f[1], f[2]], [f[0], f[2], f[3]])], np.int64)
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    trans_g = np.eye(4)
    trans_g[:3, :3], trans_g[:3, 3] = q, rng.normal(size=3)
    variables = {"faces": tri, "trans_g": trans_g, "faces_ori": faces, "uvs_ori": np.asarray(uvs), "uv_faces_ori": uv_faces}
    p = {"means3D": params["means3D"].float(), "log_scales": params["log_scales"].float(),
         "unnorm_rotations": params["unnorm_rotations"].float()}
    return p, variables


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


params, variables = head()
dparams = {k: v.to(dev).contiguous() for k, v in params.items()}
t0 = time.perf_counter()
exp = objexport.MeshExporter(variables)
torch.cuda.synchronize()
out = {"bench": "objexport", "n_vert": int(params["means3D"].shape[0]), "n_faces_ori": len(variables["faces_ori"]),
       "n_uvs": int(variables["uvs_ori"].shape[0]), "setup_ms": round((time.perf_counter() - t0) * 1e3, 3)}
for frame in (1, 2):
    exp.obj_bytes(dparams, frame)                                   # warm-up
with tempfile.TemporaryDirectory() as d:
    for frame in (1, 2):
        out[f"gpu_bytes_ms_frame{frame}"] = round(median_ms(lambda: exp.obj_bytes(dparams, frame), a.reps), 3)
        out[f"gpu_file_ms_frame{frame}"] = round(median_ms(lambda: exp.save_mesh(d, dparams, frame, gen_texture=False), a.reps), 3)
    out["obj_bytes"] = len(exp.obj_bytes(dparams, 2))
    if not a.no_cpu:
        def cpu(frame, path):
            verts = ref.save_mesh_vertices(params["means3D"], params["log_scales"], params["unnorm_rotations"], variables["faces"],
                                           variables["trans_g"], frame)
            return ref.write_obj_with_uv(path, verts, variables["faces_ori"], variables["uvs_ori"], variables["uv_faces_ori"])
        for frame in (1, 2):
            out[f"cpu_bytes_ms_frame{frame}"] = round(median_ms(lambda: cpu(frame, None), 3), 3)
            out[f"cpu_file_ms_frame{frame}"] = round(median_ms(lambda: cpu(frame, os.path.join(d, "ref.obj")), 3), 3)
        got, want = exp.obj_bytes(dparams, 1).split(b"\n"), cpu(1, None).split(b"\n")
        out["frame1_lines_differing_from_cpu"] = sum(x != y for x, y in zip(got, want)) + abs(len(got) - len(want))
print(json.dumps(out))
