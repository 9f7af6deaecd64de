#!/usr/bin/env python
"""A whole capture run (topo4d_amd.train.train, train.py:590-755) on a synthetic sequence with the reference's shapes: 24 views
under the rig's serial labels, geometry views of 512 x 376 (a 4096 x 3008 rig at --down_ratio 8) with label-PNG masks, texture
views of 4096 x 3008, golden G15's head of 8,280 vertices, --gen_tex --density 30 --tex_res 8192, and the reference's iteration
counts (7000 / 1100 / 301, progress every 500 / 300 iterations).  Prints one JSON line.

    python tools/bench_train.py [--frames 3] [--keep DIR]

seconds_per_frame: wall time of every frame (frame 0's includes the setup).  split: seconds per phase over the run (synchronised
at every phase boundary; a phase excludes the progress renders nested in it) - setup (cameras, initialize_params with the
density-30 mesh, initialize_losses, priors), ingest (views and masks onto the device), geometry (the geometry loop),
transition (initialize_per_timestep, update_dense_states, pin and rate switches), texture (the texture loop), progress
(report_progress[_dense]), export (params2cpu, checkpoints, face.obj and the 8K face.png).  geometry_it_s / texture_it_s:
iterations per second of the two loops.  optimise_views_it_s: loop.optimise_views alone for --opt_num iterations on the last
frame's views with the run's optimiser and priors (a later frame's settings), the yardstick of the geometry loop's rate.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.capture_scene import write_sequence  # noqa: E402
from tests.test_setup_host import golden  # noqa: E402
from topo4d_amd import cameras as C, ingest, loop, train as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--keep", default=None, help="write the sequence and the outputs here (default: a temporary directory)")
a = ap.parse_args()

dev = torch.device("cuda", torch.cuda.current_device())
g = golden()
root = a.keep or tempfile.mkdtemp(prefix="bench_train_")
t0 = time.perf_counter()
dirs = write_sequence(root, g, n_frames=a.frames, size=(4096, 3008), down_ratio=8, labels=tuple(C.ROTATE_MASK))
write_s = time.perf_counter() - t0
args = T.build_parser().parse_args(["-e", "bench", "-s", "seq", "-id", dirs["input_dir"], "-did", dirs["dense_input_dir"],
                                    "-od", os.path.join(root, "out"), "-fn", str(a.frames + 1), "-t", "-tr", "8192", "-dn", "30",
                                    "-dr", "8"])
frame_end = []


def on_frame(t, state):
    torch.cuda.synchronize(dev)
    frame_end.append(time.perf_counter())


timings = {}
torch.cuda.synchronize(dev)
t_start = time.perf_counter()
state = T.train(args, facial_regions=g["facial_regions"], device=dev, on_frame=on_frame, timings=timings)
torch.cuda.synchronize(dev)
t_end = time.perf_counter()
per_frame = [e - s for s, e in zip([t_start] + frame_end[:-1], frame_end)]      # frame 0 includes the setup

params, variables, opt = state["params"], state["variables"], state["optimizer"]
n_geo = args.init_opt_num + args.opt_num * (a.frames - 1)
n_tex = args.dense_opt_num * a.frames

# the yardstick: optimise_views alone on the last frame's views, a later frame's branch, the same optimiser and priors
cams, _, _ = C.get_cameras(args.input_dir, args.seq, resize_factor=args.down_ratio)
data = ingest.get_dataset(args.input_dir, args.seq, a.frames, cams, use_mask=True, rotate_mask=C.ROTATE_MASK,
                          setup_camera=lambda *p, **k: C.setup_camera(*p, device=dev, **k), device=dev)
inner = C.parsing_colormap_bgr(14)[[C.CMAP_INDEX["inner_mouth"]]]
state["pins"].install(opt, "later")
kw = dict(use_mask=True, is_initial_timestep=False, label_colors=inner, max_2D_radius=variables["max_2D_radius"],
          priors=state["priors"])
loop.optimise_views(params, data, opt, 50, **kw)                      # warm-up (masked targets, arenas)
torch.cuda.synchronize(dev)
t1 = time.perf_counter()
loop.optimise_views(params, data, opt, args.opt_num, **kw)
torch.cuda.synchronize(dev)
ov_s = time.perf_counter() - t1

dense_n = int(params["dense_rgb_colors"].shape[0])
print(json.dumps({
    "tool": "bench_train", "frames": len(frame_end), "views": len(data), "geometry_view": list(map(int, data[0]["im"].shape[1:])),
    "texture_view": [4096, 3008], "gaussians": int(params["means3D"].shape[0]), "dense_gaussians": dense_n,
    "iterations": {"geometry": n_geo, "texture": n_tex},
    "run_s": round(t_end - t_start, 3), "seconds_per_frame": [round(x, 3) for x in per_frame],
    "split": {k: round(timings.get(k, 0.0), 3) for k in ("setup", "ingest", "geometry", "transition", "texture", "progress",
                                                                 "export")},
    "geometry_it_s": round(n_geo / timings["geometry"], 1), "texture_it_s": round(n_tex / timings["texture"], 1),
    "optimise_views_it_s": round(args.opt_num / ov_s, 1),
    "write_sequence_s": round(write_s, 1),
}))
