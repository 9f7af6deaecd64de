#!/usr/bin/env python
"""Scoring one frame (topo4d_amd/evaluate.py over csrc/t4d_meshrender.hip): G15's 8,280-vertex head with an 8192^2 face.png,
rendered into 24 views at 4096x3008 (the texture inputs) and 24 at 512x376 (the geometry inputs) of tests/capture_scene.py's
synthetic rig, and compared with them.  Prints one JSON line.
    python tools/bench_meshrender.py [--reps 5] [--no-ref] [--rocprof]
kernel_ms: t4d_mesh_render + t4d_image_metrics of one frame's 24 views, GPU time between two HIP events (min of --reps; the
render's one pair-count synchronisation included), per view size.  wall_ms: `python -m topo4d_amd.evaluate --set both` for the
frame, from the files to eval.json (warm: the second of two runs in this process), and the ingest of the frame's views alone
for comparison.  ref_ms: the numpy yardstick (tests/meshrender_ref.py) on one 512x376 view.  --rocprof: the per-kernel split
from a rocprofv3 --kernel-trace --stats run of this script's kernel loop (a child process)."""
import argparse
import csv
import functools
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
from topo4d_amd import cameras as C, evaluate as E, ingest, meshrender  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-ref", action="store_true")
ap.add_argument("--rocprof", action="store_true")
ap.add_argument("--kernels-only", default=None, help=argparse.SUPPRESS)   # (the child of --rocprof: a prepared tree)
a = ap.parse_args()
dev = torch.device("cuda")
LABELS = tuple(sorted(C.ROTATE_MASK))


def prepare(root):
    """the capture tree (frame 1 + the empty frame 2) and the run tree (frame 1's face.obj + 8192^2 face.png)"""
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    from topo4d_amd import coarse, objexport, png
    g = golden()
    dirs = write_sequence(root, g, n_frames=1, size=(4096, 3008), down_ratio=8, labels=LABELS)
    mesh = coarse.read_obj(os.path.join(dirs["input_dir"], "seq", "face_v5.obj"))
    run = os.path.join(root, "out", "exp", "seq", "000001")
    os.makedirs(run, exist_ok=True)
    # save_mesh writes trans_g applied to means3D, and means3D starts as inv(trans_g) applied to the OBJ: the file holds the OBJ's vertices
    objexport.write_obj_with_uv(os.path.join(run, "face.obj"), mesh.vertices, mesh.faces_ori, mesh.tex_coords, mesh.uv_faces_ori)
    y, x = torch.meshgrid(torch.linspace(0, 1, 8192, device=dev), torch.linspace(0, 1, 8192, device=dev), indexing="ij")
    tex = torch.stack([0.5 + 0.4 * torch.sin(40 * x), 0.5 + 0.4 * torch.cos(33 * y), 0.5 + 0.3 * torch.sin(25 * (x + y))], -1)
    png.write_png(os.path.join(run, "face.png"), tex.contiguous())
    return dirs, os.path.join(root, "out")


def frame_state(dirs, which):
    cams, _, trans_g = C.get_cameras(dirs["input_dir"], "seq", resize_factor=8 if which == "low" else 1)
    data = dirs["input_dir"] if which == "low" else dirs["dense_input_dir"]
    ds = ingest.get_dataset(data, "seq", 1, cams, use_mask=which == "low", rotate_mask=C.ROTATE_MASK,
                            setup_camera=functools.partial(C.setup_camera, device=dev), device=dev)
    return ds, trans_g


def kernel_loop(dirs, out, reps):
    """{which: min ms} of render + metrics over the frame's views"""
    from PIL import Image
    run = os.path.join(out, "exp", "seq", "000001")
    obj = meshrender.read_face_obj(os.path.join(run, "face.obj"))
    tex = np.array(Image.open(os.path.join(run, "face.png")).convert("RGB"))
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, tex, device=dev)
    res = {}
    for which in ("low", "dense"):
        ds, trans_g = frame_state(dirs, which)
        verts = torch.from_numpy(E.training_vertices(obj.vertices, trans_g)).to(dev)
        cams = [e["cam"] for e in ds]
        target = torch.stack([e["im"] for e in ds])
        masks = E.pixel_masks(ds)
        times = []
        for _ in range(reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            img, _, idx = r.render(verts, cams)
            meshrender.image_metrics(img, target, idx, masks)
            t1.record()
            torch.cuda.synchronize()
            times.append(t0.elapsed_time(t1))
        res[which] = dict(views=len(ds), H=int(img.shape[2]), W=int(img.shape[3]), ms=round(min(times[1:]), 3),
                          covered=round(float((idx >= 0).float().mean()), 4), faces=int(faces.shape[0]))
        del img, idx, target
    return res, (r, obj)


if a.kernels_only:
    dirs = json.loads(a.kernels_only)
    kernel_loop(dirs, dirs["out"], a.reps)
    torch.cuda.synchronize()
    sys.exit(0)

root = tempfile.mkdtemp(prefix="t4d_bench_mr_")
dirs, out = prepare(root)
torch.cuda.synchronize()
result = {"bench": "meshrender", "texture": 8192}
result["kernel"], (renderer, obj) = kernel_loop(dirs, out, a.reps)

argv = ["-e", "exp", "-s", "seq", "-id", dirs["input_dir"], "-did", dirs["dense_input_dir"], "-od", out, "-dr", "8", "--set", "both"]
walls = []
for _ in range(2):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    E.main(argv)
    torch.cuda.synchronize()
    walls.append(time.perf_counter() - t0)
result["wall_ms"] = {"evaluate_frame_both_sets": round(1e3 * walls[-1], 1), "first_run": round(1e3 * walls[0], 1)}
for which in ("low", "dense"):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    frame_state(dirs, which)
    torch.cuda.synchronize()
    result["wall_ms"][f"ingest_{which}"] = round(1e3 * (time.perf_counter() - t0), 1)
with open(os.path.join(out, "exp", "seq", "eval.json")) as f:
    ev = json.load(f)
result["eval_summary"] = {w: ev[w]["summary"] for w in ("low", "dense")}

if not a.no_ref:
    from tests import meshrender_ref as ref
    from topo4d_amd.rasterizer import pack_views
    ds, trans_g = frame_state(dirs, "low")
    view = pack_views([ds[0]["cam"]], dev)[0].cpu().numpy()
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    verts = E.training_vertices(obj.vertices, trans_g).astype(np.float32)
    tex = renderer.texture.cpu().numpy()
    H, W = int(ds[0]["cam"].image_height), int(ds[0]["cam"].image_width)
    t0 = time.perf_counter()
    c, d, i = ref.render(verts, faces, uv_faces, obj.uvs, tex, view, H, W)
    result["ref_ms_one_view"] = {"H": H, "W": W, "ms": round(1e3 * (time.perf_counter() - t0), 1)}
    img, depth, idx = renderer.render(torch.from_numpy(verts).to(dev), [ds[0]["cam"]])
    result["ref_bit_equal"] = bool(np.array_equal(i, idx[0].cpu().numpy()) and
                                   np.array_equal(c.view(np.uint32), img[0].cpu().numpy().view(np.uint32)))

if a.rocprof:
    d = os.path.join(root, "prof")
    child = json.dumps(dict(dirs, out=out))
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--",
           sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--kernels-only", child]
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600).returncode
    stats = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                m = re.search(r"(k_(?:mr|im)_\w+(?:<\w+>)?)", row["Name"])
                if m:
                    stats[m.group(1)] = dict(calls=int(row["Calls"]), total_ms=round(float(row["TotalDurationNs"]) / 1e6, 3),
                                      avg_us=round(float(row["AverageNs"]) / 1e3, 1))
    result["rocprof"] = dict(rc=rc, kernels=stats, note="totals over the low + dense frames of reps + 1 iterations")
print(json.dumps(result))
