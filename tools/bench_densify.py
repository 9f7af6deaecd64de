"""
Benchmark of the dense-mesh setup (train.py:213-269 on the device, topo4d_amd/densify.py): a seeded lat-long head of about 5k
frontal quads at density 30 (about 5.1 M dense points).  Prints one JSON line: host planning time, the build (upload + generator
launches) and the k = 4 kNN with dense_log_scales, each as the median of --reps runs with the stream synchronised, and the
generator's algorithmic bytes (what it must write plus the quad records it reads).  Kernel-only times come from a separate run
under `rocprofv3 --kernel-trace --stats -- python tools/bench_densify.py --reps 1`.

    python tools/bench_densify.py [--lat 51 --lon 200 --density 30 --reps 5]
    python tools/bench_densify.py --reference-quads 8      # CPU only: the reference's build_dense_vertices_2, ms per quad
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def reference_ms_per_quad(n_quads, density):
    """The reference's own build_dense_vertices_2 on the CPU (where the reference tree exists), on a grid of n_quads quads."""
    from oracle import gen_golden
    from tools.gen_golden_dense import synthetic_mesh
    helpers, _ = gen_golden.import_reference_helpers()
    P, faces, uv_faces, uvs, texture, masks = synthetic_mesh(2, max(2, n_quads // 2), 7)
    quads = np.array([f for f in faces if len(f) == 4])
    idx = np.array([i for i, f in enumerate(faces) if len(f) == 4])
    variables = {'uv_faces_ori': uv_faces, 'uvs_ori': uvs}
    t = time.perf_counter()
    helpers.build_dense_vertices_2(variables, P.copy(), quads, idx, density, texture)
    return (time.perf_counter() - t) * 1e3 / quads.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lat", type=int, default=51)
    ap.add_argument("--lon", type=int, default=200)
    ap.add_argument("--density", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference-quads", type=int, default=0)
    a = ap.parse_args()
    if a.reference_quads:
        print(json.dumps({"reference_build_dense_vertices_2_ms_per_quad": reference_ms_per_quad(a.reference_quads, a.density),
                          "density": a.density, "device": "cpu"}))
        return
    import torch
    from topo4d_amd import densify
    from tests.test_gpu_densify import head_mesh
    params, faces, uv_faces, uvs, uv_counts, masks = head_mesh(a.lat, a.lon, seed=1)
    means = params["means3D"].cuda()
    t_plan = []
    for _ in range(a.reps):
        t = time.perf_counter()
        plan = densify.plan_dense_mesh(faces, uv_faces, uv_counts, masks, a.density, means.shape[0], uvs.shape[0])
        t_plan.append(time.perf_counter() - t)
    t_build, t_knn = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        mesh = densify.build_dense_mesh(means, faces, uv_faces, uvs, uv_counts, masks, a.density, plan=plan)
        torch.cuda.synchronize()
        t_build.append(time.perf_counter() - t)
        t = time.perf_counter()
        scales = densify.knn_mean_sq_dist(mesh["dense_vertex"], 4, log_scales=True)
        torch.cuda.synchronize()
        t_knn.append(time.perf_counter() - t)
    n, nq, nf = plan["n_points"], plan["quad_faces"].shape[0], int(mesh["dense_faces"].shape[0])
    gen_bytes = n * (3 * 8 + 4 + 4 * 8 + 2 * 8) + 2 * nf * 3 * 4 + nq * (4 + 4 + 2 + 4) * 4
    med = lambda x: float(np.median(x)) * 1e3
    print(json.dumps({"frontal_quads": int(nq), "density": a.density, "dense_points": int(n) + int(means.shape[0]),
                      "faces": nf, "plan_ms": med(t_plan), "build_ms": med(t_build), "knn_log_scales_ms": med(t_knn),
                      "generator_bytes": int(gen_bytes), "log_scales_finite": bool(torch.isfinite(scales).all())}))


if __name__ == "__main__":
    main()
