#!/usr/bin/env python
"""Projection of the capture photographs into the UV texture (topo4d_amd/projtex.py, csrc/t4d_projtex.hip).  Prints one JSON line.
    python tools/bench_projtex.py [--res 8192] [--n 513] [--views 24] [--height 3008] [--width 4096] [--equalize | --twoband [--radius 8] | --reject | --register]
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
the mask.
--register times the registration of the views instead of the frame, in the same run as kernel_ms, everything between HIP events,
min of 5 after a warm-up: view_flows_ms is projtex.view_flows over all views with its default options (its report's copies to the
host included); project_ms / project_flow_ms are t4d_project_texture (weighted) without and with the flows it found, alternating,
and project_bands_ms / project_bands_flow_ms the two-band projection likewise; registered_frame_ms is the frame as above with the
consensus (weighted projection, quantisation, hole fill over the coverage as one island), its render into every camera,
view_flows and the weighted projection through the flows in the place of the projection, and frame_ms the plain frame of the same
run.  A matcher needs photographs that show the mesh: with --register they are the renders of a blurred random 2048 x 2048
texture into the cameras, each moved by up to a pixel either way, not noise; `flows` describes what was found.  The result is also
written to profiles/projtex_register_bench.json."""
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
ap.add_argument("--register", action="store_true")
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
if a.register:
    def events_min5(fn):
        """min of 5 between HIP events on the current stream, after one warm-up"""
        stream = torch.cuda.current_stream()
        fn()
        best = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1))
        return round(best, 3)

    g = torch.Generator(device=dev).manual_seed(0)
    noise = torch.rand(1, 3, 2048, 2048, device=dev, generator=g)
    noise = torch.nn.functional.avg_pool2d(noise, 5, stride=1, padding=2)
    noise = ((noise - noise.min()) / (noise.max() - noise.min()))[0].permute(1, 2, 0).contiguous()
    painted = meshrender.MeshRenderer(tris, tris, uvs, noise, device=dev).render(verts, cams)[0]
    for k in range(V):                                          # every camera a little off, up to a pixel either way
        photos[k] = torch.roll(painted[k], (k % 3 - 1, (k // 3) % 3 - 1), (1, 2))
    del painted, noise
    labels = (cov != 0).to(torch.uint8)                         # the coverage as one island
    stream_ptr = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def consensus_renders(d, p, n, c):
        col, _, cnt = projtex.project(p, n, c, cams, photos, d)
        tex, _ = texfinish.fill_islands(texfinish.quantize(col), (cnt > 0).to(torch.uint8), labels)
        return meshrender.MeshRenderer(tris, tris, uvs, tex, device=dev).render(verts, cams, mapping="bilinear")[0]

    renders = consensus_renders(depth, pos, nrm, cov)
    found = {}

    def flows_of_all_views():
        found["flows"], found["support"], found["report"] = projtex.view_flows(renders, photos, depth)

    result["view_flows_ms"] = events_min5(flows_of_all_views)
    flows, report = found["flows"], found["report"]
    low = torch.empty_like(photos)
    high = torch.empty_like(color)
    best_weight = torch.empty_like(weight)
    rc = lib.t4d_projtex_low_band(P(photos), P(depth), V, H, W, a.radius, P(low), stream_ptr())
    assert rc == 0, _lib.last_error()

    def project_with(f):
        def launch():
            rc = lib.t4d_project_texture_flow(P(pos), P(nrm), P(cov), res, res, P(views), V, H, W, P(photos), P(depth), None, 2, 0.1, 16.0,
                                              0.002, 0, P(color), P(weight), P(count), None, 0, stream_ptr(), f)
            assert rc == 0, _lib.last_error()
        return launch

    def bands_with(f):
        def launch():
            rc = lib.t4d_project_texture_bands_flow(P(pos), P(nrm), P(cov), res, res, P(views), V, H, W, P(photos), P(low), P(depth), None, 2,
                                                    0.1, 16.0, 0.002, P(color), P(weight), P(count), P(high), P(best_weight), None, 0,
                                                    stream_ptr(), f)
            assert rc == 0, _lib.last_error()
        return launch

    for name, launch in (("project", project_with), ("project_bands", bands_with)):
        runs = {"": [], "_flow": []}
        for _ in range(2):                                      # the two alternate, so that both see the same machine
            for key, f in (("", None), ("_flow", P(flows))):
                runs[key].append(events_min5(launch(f)))
        for key, r in runs.items():
            result[name + key + "_ms"] = min(r)
    result["flow_over_project"] = round(result["project_flow_ms"] / result["project_ms"], 3)
    result["bands_flow_over_bands"] = round(result["project_bands_flow_ms"] / result["project_bands_ms"], 3)
    result["kernel_ms_again"] = events_ms(kernel(0))             # the plain kernel once more, after the others: the run's own spread
    kept = [r["kept"] for r in report]
    result["flows"] = {"blocks_per_view": report[0]["blocks"], "kept_blocks_mean": round(float(np.mean(kept)), 1),
                       "mean_length_px": round(float(np.mean([r.get("mean", 0.0) for r in report])), 3),
                       "supported_fraction": round(float(found["support"].float().mean()), 4)}
    del low, high, best_weight, renders, found

    def registered_frame():
        d = depth_maps()
        p, n, c = maps()
        f, _, _ = projtex.view_flows(consensus_renders(d, p, n, c), photos, d)
        col, _, _ = projtex.project(p, n, c, cams, photos, d, flows=f)
        return png.encode_png(texfinish.quantize(col))

    result["frame_ms"] = events_min5(frame)
    result["registered_frame_ms"] = events_min5(registered_frame)
    result["registered_over_frame"] = round(result["registered_frame_ms"] / result["frame_ms"], 2)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "projtex_register_bench.json")
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
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
