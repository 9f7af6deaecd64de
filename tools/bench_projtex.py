#!/usr/bin/env python
"""Projection of the capture photographs into the UV texture (topo4d_amd/projtex.py, csrc/t4d_projtex.hip).  Prints one JSON line.
    python tools/bench_projtex.py [--res 8192] [--n 513] [--views 24] [--height 3008] [--width 4096] [--equalize | --twoband [--radius 8] | --reject]
The scene: scaffold.scene.uv_mesh(n) as the UV layout, its vertices lifted onto the front of the scaffold's head-sized ellipsoid,
seen by scaffold.scene.camera_rig (24 views at 4096 x 3008) with random photographs.  kernel_ms: t4d_project_texture alone between
HIP events on preallocated buffers (min of 6), for both modes.  frame_ms: what one frame costs from the mesh and the photographs
on the device to the PNG file as bytes in host memory - the depth render, the two texel maps and the coverage, the projection,
the quantisation and png.encode_png (min of 3).  parts_ms times three of its steps on their own, each between two device
synchronisations, so they add up to a little more than the frame, where the steps queue behind one another; quantise_encode
is timed on the weighted result, the one the frame encodes.  The texture loop this stands beside is timed by tools/bench_train.py.
--equalize times the camera equalisation instead of the frame, in the same run as kernel_ms: pair_stats_ms is
t4d_projtex_pair_stats alone on zeroed outputs and project_gains_ms t4d_project_texture_gains (weighted) with the solved gains,
both between HIP events (min of 6); solve_ms is projtex.solve_gains on the host, the copy of the two tables included (min of 3).
The photographs are random, so the solved gains say nothing; pair_counts describes the overlap they were solved from.
--twoband times mode "twoband" instead of the frame, in the same run as kernel_ms: low_band_ms is t4d_projtex_low_band over all
views and project_bands_ms t4d_project_texture_bands, both between HIP events (min of 6); twoband_frame_ms is the frame as above
with the low bands, the two-band projection and the sum of the bands in the place of the projection, and frame_ms the weighted
frame of the same run (min of 3 each).
--reject times the photo-consistency check instead of the frame, in the same run as kernel_ms: consistency_ms is
t4d_projtex_consistency over all views, project_skip_ms t4d_project_texture_skip (weighted) and project_bands_skip_ms
t4d_project_texture_bands_skip under its mask, and project_bands_ms the two-band projection without a mask, all between HIP events
(min of 6); the yardstick is the unmasked projection of the same run.  Random photographs over the whole range never agree, so
with --reject they are drawn from [0.35, 0.65]: most views agree within the default tolerance and some do not; `rejected` describes
the mask."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scaffold.scene import SEMI_AXES, camera_rig, uv_mesh
from topo4d_amd import _lib, meshrender, png, projtex, texfinish, texture

ap = argparse.ArgumentParser()
ap.add_argument("--res", type=int, default=8192)
ap.add_argument("--n", type=int, default=513)
ap.add_argument("--views", type=int, default=24)
ap.add_argument("--height", type=int, default=3008)
ap.add_argument("--width", type=int, default=4096)
ap.add_argument("--equalize", action="store_true")
ap.add_argument("--twoband", action="store_true")
ap.add_argument("--reject", action="store_true")
ap.add_argument("--radius", type=int, default=projtex.BAND_DEFAULTS["band_radius"])
a = ap.parse_args()
dev = torch.device("cuda", torch.cuda.current_device())
lib = _lib.load()
P = lambda t: C.c_void_p(t.data_ptr())


def events_ms(launch, repeats=6):
    stream = torch.cuda.current_stream()
    best = 1e9
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch(C.c_void_p(stream.cuda_stream))
        e1.record(stream)
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return round(best, 3)


def wall_ms(fn, repeats=3):
    fn()
    runs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    return round(min(runs) * 1e3, 2)


res, V, H, W = a.res, a.views, a.height, a.width
uv_px, tris, _ = uv_mesh(a.n, res, res, seed=0)
u, v = uv_px[:, 0] / (res - 1), (res - 1 - uv_px[:, 1]) / (res - 1)
lon, lat = (u - 0.5) * 0.9 * np.pi, (v - 0.5) * 0.9 * np.pi
unit = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], 1)
verts = torch.from_numpy((unit * np.array(SEMI_AXES)).astype(np.float32)).to(dev)
normals = torch.from_numpy((unit / np.array(SEMI_AXES)).astype(np.float32)).to(dev)
cams = camera_rig(H, W, V, device=dev)
photos = torch.rand(V, 3, H, W, device=dev)
if a.reject:
    photos.mul_(0.3).add_(0.35)
uvs = np.stack([u, v], 1)
renderer = meshrender.MeshRenderer(tris, tris, uvs, np.zeros((1, 1, 3), np.uint8), device=dev)


def depth_maps():
    return renderer.render(verts, cams)[1]


def maps():
    pos, d = texture.render_colors(uv_px, tris, verts, res, res, device=dev, return_depth=True)
    nrm = texture.render_colors(uv_px, tris, normals, res, res, device=dev)
    return pos, nrm, texfinish.coverage_from_depth(d)


depth = depth_maps()
pos, nrm, cov = maps()
views = meshrender._views(cams, dev)[0]
color = torch.empty(res, res, 3, dtype=torch.float32, device=dev)
weight = torch.empty(res, res, dtype=torch.float32, device=dev)
count = torch.empty(res, res, dtype=torch.uint8, device=dev)


def kernel(mode):
    def launch(s):
        rc = lib.t4d_project_texture(P(pos), P(nrm), P(cov), res, res, P(views), V, H, W, P(photos), P(depth), 2, 0.1, 16.0, 0.002,
                                     mode, P(color), P(weight), P(count), s)
        assert rc == 0, _lib.last_error()
    return launch


def frame():
    d = depth_maps()
    p, n, c = maps()
    col, _, _ = projtex.project(p, n, c, cams, photos, d)
    return png.encode_png(texfinish.quantize(col))


result = {"metric": "photographs projected into the UV texture", "res": res, "views": V, "image": [H, W], "triangles": int(len(tris))}
result["kernel_ms"] = {"weighted": events_ms(kernel(0)), "best": events_ms(kernel(1))}
result["covered_fraction"] = round(float((cov != 0).float().mean()), 4)
result["seen_fraction_of_covered"] = round(float(((count != 0) & (cov != 0)).float().sum() / (cov != 0).float().sum()), 4)
result["mean_views_per_seen_texel"] = round(float(count[count != 0].float().mean()), 2)
result["projections_per_s"] = round(float((cov != 0).sum()) * V / (result["kernel_ms"]["weighted"] * 1e-3), 0)
if a.equalize:
    pair_count = torch.zeros(V, V, dtype=torch.int64, device=dev)
    pair_sum = torch.zeros(V, V, 3, dtype=torch.int64, device=dev)
    sizes = torch.tensor([[H, W]] * V, dtype=torch.int32, device=dev)
    tables = torch.tensor([[photos[k].data_ptr() for k in range(V)], [depth[k].data_ptr() for k in range(V)]], dtype=torch.int64, device=dev)

    def stats(s):
        rc = lib.t4d_projtex_pair_stats(P(pos), P(nrm), P(cov), res, res, P(views), V, P(sizes), P(tables[0]), P(tables[1]), 2, 0.1, 16.0,
                                        0.002, 0.5, 0.02, 0.98, None, P(pair_count), P(pair_sum), s)
        assert rc == 0, _lib.last_error()

    result["pair_stats_ms"] = events_ms(stats)
    pair_count.zero_()
    pair_sum.zero_()
    stats(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        gains = projtex.solve_gains(pair_count, pair_sum)
        runs.append(time.perf_counter() - t0)
    result["solve_ms"] = round(min(runs) * 1e3, 3)
    g = torch.from_numpy(gains).to(dev)

    def with_gains(s):
        rc = lib.t4d_project_texture_gains(P(pos), P(nrm), P(cov), res, res, P(views), V, H, W, P(photos), P(depth), P(g), 2, 0.1, 16.0,
                                           0.002, 0, P(color), P(weight), P(count), s)
        assert rc == 0, _lib.last_error()

    result["project_gains_ms"] = events_ms(with_gains)
    result["kernel_ms_again"] = events_ms(kernel(0))             # the plain kernel once more, after the others: the run's own spread
    off = pair_count.cpu().numpy()[~np.eye(V, dtype=bool)]
    result["pair_counts"] = {"pairs_with_overlap": int((off > 0).sum() // 2), "max": int(off.max()), "diagonal_mean": int(pair_count.diagonal().float().mean())}
    result["pair_stats_over_kernel"] = round(result["pair_stats_ms"] / result["kernel_ms"]["weighted"], 2)
    print(json.dumps(result))
    sys.exit(0)
if a.reject:
    if V > projtex.MAX_STAT_VIEWS:
        sys.exit(f"--reject: at most {projtex.MAX_STAT_VIEWS} views")
    skip = torch.zeros(res, res, dtype=torch.int32, device=dev)
    votes = torch.zeros(res, res, dtype=torch.uint8, device=dev)
    sizes = torch.tensor([[H, W]] * V, dtype=torch.int32, device=dev)
    tables = torch.tensor([[photos[k].data_ptr() for k in range(V)], [depth[k].data_ptr() for k in range(V)]], dtype=torch.int64, device=dev)
    low = torch.empty_like(photos)
    high = torch.empty_like(color)
    best_weight = torch.empty_like(weight)
    c = projtex.CONSIST_DEFAULTS

    def consist(s):
        rc = lib.t4d_projtex_consistency(P(pos), P(nrm), P(cov), res, res, P(views), V, P(sizes), P(tables[0]), P(tables[1]), 2, 0.1, 16.0,
                                         0.002, None, c["reject_tol"], c["vote_cos_min"], c["min_votes"], P(skip), P(votes), s)
        assert rc == 0, _lib.last_error()

    def masked(mask):
        def launch(s):
            rc = lib.t4d_project_texture_skip(P(pos), P(nrm), P(cov), res, res, P(views), V, H, W, P(photos), P(depth), None, 2, 0.1, 16.0,
                                              0.002, 0, P(color), P(weight), P(count), mask, 0, s)
            assert rc == 0, _lib.last_error()
        return launch

    def bands(mask):
        def launch(s):
            rc = lib.t4d_project_texture_bands_skip(P(pos), P(nrm), P(cov), res, res, P(views), V, H, W, P(photos), P(low), P(depth), None, 2,
                                                    0.1, 16.0, 0.002, P(color), P(weight), P(count), P(high), P(best_weight), mask, 0, s)
            assert rc == 0, _lib.last_error()
        return launch

    rc = lib.t4d_projtex_low_band(P(photos), P(depth), V, H, W, a.radius, P(low), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    result["consistency_ms"] = events_ms(consist)
    result["project_skip_ms"] = events_ms(masked(P(skip)))
    result["kernel_ms_again"] = events_ms(kernel(0))             # the plain kernel once more, after the others: the run's own spread
    result["project_bands_ms"] = events_ms(bands(None))
    result["project_bands_skip_ms"] = events_ms(bands(P(skip)))
    live = votes > 0
    n = projtex.rejected_count(skip)
    result["rejected"] = {"texels_with_min_votes": round(float((votes >= c["min_votes"]).sum() / live.sum()), 4),
                          "texels_with_a_rejected_view": round(float((n > 0).sum() / live.sum()), 4),
                          "mean_rejected_views_there": round(float(n[n > 0].float().mean()), 2) if bool((n > 0).any()) else 0.0}
    result["consistency_over_kernel"] = round(result["consistency_ms"] / result["kernel_ms"]["weighted"], 2)
    result["skip_over_kernel"] = round(result["project_skip_ms"] / result["kernel_ms"]["weighted"], 2)
    result["bands_skip_over_bands"] = round(result["project_bands_skip_ms"] / result["project_bands_ms"], 2)
    print(json.dumps(result))
    sys.exit(0)
if a.twoband:
    low = torch.empty_like(photos)
    high = torch.empty_like(color)
    best_weight = torch.empty_like(weight)

    def low_pass(s):
        rc = lib.t4d_projtex_low_band(P(photos), P(depth), V, H, W, a.radius, P(low), s)
        assert rc == 0, _lib.last_error()

    def bands(s):
        rc = lib.t4d_project_texture_bands(P(pos), P(nrm), P(cov), res, res, P(views), V, H, W, P(photos), P(low), P(depth), None, 2, 0.1,
                                           16.0, 0.002, P(color), P(weight), P(count), P(high), P(best_weight), s)
        assert rc == 0, _lib.last_error()

    def twoband_frame():
        d = depth_maps()
        p, n, c = maps()
        lc, _, _, hi, _ = projtex.project_bands(p, n, c, cams, photos, projtex.low_band(photos, d, a.radius), d)
        return png.encode_png(texfinish.quantize((lc + hi).clamp_(0.0, 1.0)))

    result["radius"] = a.radius
    result["low_band_ms"] = events_ms(low_pass)
    result["project_bands_ms"] = events_ms(bands)
    result["kernel_ms_again"] = events_ms(kernel(0))             # the plain kernel once more, after the others: the run's own spread
    result["bands_over_kernel"] = round(result["project_bands_ms"] / result["kernel_ms"]["weighted"], 2)
    del low, high, best_weight
    result["frame_ms"] = wall_ms(frame)
    result["twoband_frame_ms"] = wall_ms(twoband_frame)
    print(json.dumps(result))
    sys.exit(0)
kernel(0)(C.c_void_p(torch.cuda.current_stream().cuda_stream))        # `color` holds the weighted result again
result["parts_ms"] = {"depth_render": wall_ms(depth_maps), "texel_maps": wall_ms(maps),
                      "quantise_encode": wall_ms(lambda: png.encode_png(texfinish.quantize(color)))}
result["frame_ms"] = wall_ms(frame)
result["png_bytes"] = len(frame())
print(json.dumps(result))
