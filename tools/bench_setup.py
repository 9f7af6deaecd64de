#!/usr/bin/env python
"""The coarse setup of a run (topo4d_amd/coarse.py, csrc/t4d_setup.hip) on golden G15's 8,280-vertex scene: wall time of
read_obj + the coarse params (colours, normals, quaternions, kNN scales) + the one-ring + initialize_losses' topology and region
weights, against plain-Python restatements of the reference's loops where they can run here (the neighbour loop of
train.py:177-200 and the FlattenLoss constructors' loop, loss_util.py:114-170, over the same host set orders).  The dense half is
not timed.  Prints one JSON line.
    python tools/bench_setup.py [--reps 5] [--no-cpu]
gpu_*_ms: medians of --reps after one warm-up, synchronised; cpu_*_ms: one run of each restated loop."""
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
from tests.test_setup_host import golden, write_scene  # noqa: E402
from topo4d_amd import coarse  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-cpu", action="store_true")
a = ap.parse_args()
g = golden()
fr = g["facial_regions"]


def timed(fn):
    ts = []
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r:
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


with tempfile.TemporaryDirectory() as tmp:
    from pathlib import Path
    path = write_scene(Path(tmp), g)
    res = {}
    res["gpu_read_obj_ms"], mesh = timed(lambda: coarse.read_obj(path))
    res["gpu_coarse_params_ms"], (params, variables, _) = timed(lambda: coarse.coarse_params(mesh, g["trans_g"]))
    P = mesh.vertices.shape[0]
    res["gpu_one_ring_host_ms"], (ori, padded) = timed(lambda: coarse.one_ring(mesh.faces_ori, P))
    res["gpu_neighbor_priors_ms"], (w, d) = timed(lambda: coarse.neighbor_priors(params["means3D"], padded, fr["eye_del_masks"]))
    variables.update(facial_regions=fr, neighbor_indices_ori=ori, neighbor_indices=torch.from_numpy(padded).cuda(),
                     neighbor_weight=w, neighbor_dist=d)
    res["gpu_initialize_losses_ms"], _ = timed(lambda: coarse.initialize_losses(variables))
    res["gpu_total_ms"] = sum(v for k, v in res.items())

if not a.no_cpu:
    # train.py:177-200 as written, over the same ordered neighbour lists
    x = params["means3D"].detach().cpu().numpy().astype(np.float64)
    eye = fr["eye_del_masks"]
    t0 = time.perf_counter()
    sq, wh = [], []
    for vi, nb in enumerate(padded.tolist()):
        ds, ws = [], []
        for ni in nb:
            dist = np.sum((x[vi] - x[ni]) ** 2)
            ds.append(dist)
            ws.append(np.sum(((x[vi] - x[ni]) * 1000) ** 2) if ni in eye and vi not in eye else dist)
        sq.append(np.array(ds))
        wh.append(np.array(ws))
    weight = np.exp(-2000 * np.array(wh))
    weight[weight == 1] = 0.0
    res["cpu_neighbor_loop_ms"] = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(weight.astype(np.float32), w.cpu().numpy())
    # the FlattenLoss / SoftFlattenLoss constructors' loop, six terms
    t0 = time.perf_counter()
    for t, key in coarse.FLAT_EDGE_TERMS.items():
        f = np.asarray(fr[key])
        edges = coarse.flatten_candidate_edges(f)
        vf = {}
        for k, face in enumerate(f):
            for vx in face:
                vf.setdefault(vx, []).append(k)
        for v0, v1 in edges:
            for fid in sorted(list(set(vf[v0]) & set(vf[v1]))):
                v = np.copy(f[fid])
                v = v[v != v0]
                v = v[v != v1]
    res["cpu_flatten_constructors_ms"] = (time.perf_counter() - t0) * 1e3
res["n_vertices"] = int(P)
res["device"] = torch.cuda.get_device_name(0)
print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))
