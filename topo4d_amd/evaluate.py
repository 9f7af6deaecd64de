"""
Score a finished run: `python -m topo4d_amd.evaluate -e EXP -s SEQ [-id ... -did ... -od ...] [--frames 1-10] [--views A,B]
[--set low|dense|both|none] [--save_renders] [--scans DIR [--scan_max_dist X] [--scan_unit S] [--scan_thresholds a,b,c]
[--scan_transform FILE] [--scan_align first|each] [--save_scan_errors] [--bake_disp DIST [--bake_res N] [--bake_both_sides] [--disp_png] [--disp_fill]
[--disp_smooth K] [--disp_normals] [--disp_apply N [--disp_save_obj]]]] [--tex_pad R [--tex_erode E]]
[--texture NAME] [--drift [--drift_texture NAME] [--drift_ref first|previous] [--drift_level K] [--drift_block B] [--drift_stride S]
[--drift_radius R] [--drift_ratio Q] [--drift_unit U]]`.

For every frame of <od>/<exp>/<seq>: read %06d/face.obj (save_mesh's vertices: the training frame mapped by the trans_g of
cameras.get_cameras, whose inverse maps them back, in float64) and %06d/face.png (PIL, on the host; frame t+1's files are read on a thread
while frame t is scored), load the frame's views as training does (ingest.get_dataset, face-parsing masks where they exist),
render the textured mesh into every camera (meshrender.MeshRenderer) and compare it with the photograph
(meshrender.image_metrics).  The pixel mask drops the labels training masks out of its photometric loss (get_loss: inner_mouth,
loss.get_mask).  Writes <od>/<exp>/<seq>/eval.json; with --save_renders also %06d/mesh_<cam>.png.  Works on output trees of the
reference's train.py as well: the layout and save_mesh's formats are the same.

With --scans DIR every frame's face.obj is also measured against that frame's 3D scan, DIR/%06d.ply or else DIR/%06d.obj
(scanscore.score_scan: scan -> mesh and mesh -> scan distances).  face.obj is compared as written: save_mesh writes world
coordinates, the frame Metashape exports its scans in.  eval.json gains the key "scan"; --set none scores scans alone.

With --scan_align first|each the scan is first aligned rigidly to the mesh (scanalign.align_scan: iterated closest points from the
pose of --scan_transform; --scan_align_scale, --scan_align_metric, --scan_align_iters, --scan_align_stride): per frame (each), or
by the first scored frame's transform for all (first: an offset between the scanner's frame and the tracking's is constant).
Scoring, the bake and scan_score.npz see the aligned scan.  The frame's row gains "alignment", the scan block "align", and the
composed matrix is written at %.17g to %06d/scan_align.txt (each) or scan_align.txt (first): given back as --scan_transform
without --scan_align, it reproduces the scores.

With --bake_disp DIST (scan file units) every scored frame's scan detail is also baked into the UV layout of its face.obj
(scanbake.bake_displacement: per texel a ray along the surface normal, both ways, within DIST; --scan_transform applies first):
%06d/face_disp.npy (float32 [N,N], scan file units, positive outward, N = --bake_res) and %06d/face_disp_hit.png (255 where the
ray met the scan).  The frame's "scan" row gains "displacement" (scanbake.displacement_stats, in --scan_unit) and
"mesh_to_scan_normal" (every mesh vertex shot along its normal within DIST: the normal-shooting distance), the summary their
means.  --bake_both_sides also counts scan triangles that face away from the texel's normal.

With --disp_png the map is also finished into %06d/face_disp.png, a 16-bit grey PNG a renderer loads (dispmap.finish: code 32768 is
no displacement, one step is DIST / 32767 scan file units); --disp_fill fills the texels whose ray missed from their UV island
(push-pull), --disp_smooth K smooths K rounds (0..8) within the islands, --disp_normals also writes %06d/face_disp_normal.png, the
16-bit tangent-space normal map; each of the three implies --disp_png, and all need --bake_disp with DIST > 0.  eval.json's "bake"
gains "png" (zero, unit and the steps taken) and each frame's "displacement" gains "filled", the texels filled.

With --disp_apply N (1..64, implies --disp_png) the finished map is also applied: the frame's mesh is tessellated into N segments per
edge, every fine vertex is pushed along its interpolated normal by the map sampled at its UV (tessellate.Tessellation.displace), and
the displaced mesh is scored against the scan under the frame's own options.  The frame's row gains "scan_displaced" (scan_to_mesh
and mesh_to_scan, to be read next to the tracked mesh's) and "tessellation" (level, vertices, faces, unsampled: the fine vertices no
texel of their island gave a value), "bake" gains "apply", the summary the mean of scan_displaced.scan_to_mesh.mean.
--disp_save_obj also writes %06d/face_hi.obj, the displaced mesh in the tracked topology's UV layout.

With --tex_pad R every face.png is padded in memory before it is sampled (texfinish.finish: a gutter of R texels round the UV
islands of face.obj, whose coverage is first eroded --tex_erode rounds, 1 by default), so that the bilinear taps on the UV seams
no longer mix in the file's black background.  The files stay as they are; eval.json gains "tex_pad" and "tex_erode".

With --texture NAME that file of every frame directory is sampled instead of face.png, e.g. face_proj.png (projtex); eval.json
gains "texture_file".

With --drift the tracking drift between the frames' UV textures is measured too (topo4d_amd.drift.drift_tree, the --drift_* flags
being that module's flags): eval.json gains "drift", the dictionary `python -m topo4d_amd.drift` writes to drift.json.  --set none
with --drift measures the drift alone.
"""
from __future__ import annotations

import argparse
import functools
import json
import math
import os
import sys
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _run
from . import cameras as C
from . import meshrender

MASK_LABELS = ["inner_mouth"]                 # train.py get_loss's target_labels


TEXTURE_FILE = "face.png"


def training_vertices(vertices: np.ndarray, trans_g) -> np.ndarray:
    """face.obj's vertices back in the training frame, in float64.  save_mesh writes its variables['trans_g'] inverted and applied
    to means3D (helpers.py:981-983); variables['trans_g'] is itself the inverse of the trans_g that cameras.get_cameras returns
    (train.py:124-126), so the file holds trans_g applied to means3D and inv(trans_g) maps it back."""
    v = np.asarray(vertices, dtype=np.float64)
    if trans_g is None:
        return v
    inv = np.linalg.inv(np.asarray(trans_g, dtype=np.float64))
    return v @ inv[:3, :3].T + inv[:3, 3]


def pixel_masks(dataset) -> Optional[torch.Tensor]:
    """[V,1,H,W]: 1 where the photograph is scored; None when the views carry no parsing mask."""
    if not dataset or any(e.get("mask") is None for e in dataset):
        return None
    from .loss import label_mask_target
    cmap = C.parsing_colormap_bgr(14)
    colors = cmap[[C.CMAP_INDEX[l] for l in MASK_LABELS]]
    masks = torch.stack([e["mask"] for e in dataset])
    filtered, _ = label_mask_target(masks, colors)
    return (1.0 - filtered[:, :1]).contiguous()


def evaluate_frame(renderer: meshrender.MeshRenderer, vertices: torch.Tensor, dataset, masks: Optional[torch.Tensor] = None,
                   keep_renders: bool = False):
    """Render and score every view of `dataset` (get_dataset's entries).  vertices [N,3] in the training frame, on the renderer's
    device; masks [V,1,H,W] or None.  Returns {cam_name: {metric: value, ..., "covered": pixels}} and, with keep_renders,
    {cam_name: image [3,H,W]} too.  Views of one size go in one launch."""
    groups: Dict[tuple, List[int]] = {}
    for k, e in enumerate(dataset):
        groups.setdefault((int(e["cam"].image_height), int(e["cam"].image_width)), []).append(k)
    scores, renders = {}, {}
    for (H, W), ks in groups.items():
        image, _, index = renderer.render(vertices, [dataset[k]["cam"] for k in ks])
        target = torch.stack([dataset[k]["im"] for k in ks]).to(torch.float32)
        m = None if masks is None else masks[ks]
        vals = meshrender.image_metrics(image, target, index, m).cpu().numpy()
        covered = (index >= 0).reshape(len(ks), -1).sum(1).cpu().numpy()
        for j, k in enumerate(ks):
            name = dataset[k]["cam_name"]
            row = {n: float(vals[j, q]) for q, n in enumerate(meshrender.METRIC_NAMES)}
            row["count"] = int(row["count"])
            row["covered"] = int(covered[j])
            scores[name] = row
            if keep_renders:
                renders[name] = image[j]
    return (scores, renders) if keep_renders else scores


def _finite(x):
    return x if isinstance(x, (int, bool)) or (isinstance(x, float) and math.isfinite(x)) else None


def _summary(frames: dict) -> dict:
    per = {n: [] for n in ("psnr_full", "l1", "mse", "psnr", "ssim")}
    for fr in frames.values():
        for row in fr.get("views", {}).values():
            for n in per:
                if row.get(n) is not None:
                    per[n].append(row[n])
    out = {"frames": len([f for f in frames.values() if "views" in f])}
    for n, xs in per.items():
        out[f"mean_{n}"] = float(np.mean(xs)) if xs else None
    worst = [(f, min((r["psnr"] for r in fr["views"].values() if r.get("psnr") is not None), default=None))
             for f, fr in frames.items() if fr.get("views")]
    worst = [w for w in worst if w[1] is not None]
    out["worst_frame_psnr"] = min(worst, key=lambda w: w[1])[0] if worst else None
    return out


def score_set(args, which: str, device) -> dict:
    from . import ingest
    run_dir = _run.run_dir_of(args)
    # every camera without --views; the photographs are undistorted as training loaded them
    cameras, trans_g, lenses, data_dir, chosen, skip = _run.select_cameras(args, which, absent="all")
    trained = {n: not any(n.startswith(b) for b in C.BLACKLIST) for n in chosen}
    cam_fn = functools.partial(C.setup_camera, device=device)
    texture_file = getattr(args, "texture", TEXTURE_FILE)
    result, use_mask = {}, {}

    def views_ahead(t):                                        # the frame's views with their masks where every view has one
        md = os.path.join(data_dir, args.seq, "mask", _run.frame_key(t))
        use_mask[t] = all(os.path.exists(os.path.join(md, n + ".png")) for n in chosen)
        pf[use_mask[t]].prefetch(t)

    pf = {flag: ingest.FramePrefetcher(data_dir, args.seq, cameras, use_mask=flag, blacklist=skip, rotate_mask=C.ROTATE_MASK,
                                       setup_camera=cam_fn, device=device, lenses=lenses) for flag in (False, True)}
    try:
        with _run.prefetched(_run.frames_of(args, run_dir), lambda t: _run.read_textured_frame(_run.frame_dir(run_dir, t), texture_file),
                             ahead=views_ahead, thread_name="t4d-eval") as walk:
            for t, (obj, tex) in walk:
                dataset = pf[use_mask[t]].get(t)
                key = _run.frame_key(t)
                if obj is None:
                    result[key] = {"skipped": "no face.obj"}
                    continue
                if not dataset:
                    result[key] = {"skipped": "no views"}
                    continue
                faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
                texture = tex if tex is not None else np.full((2, 2, 3), 128, np.uint8)
                if tex is not None and getattr(args, "tex_pad", None) is not None:
                    from . import texfinish
                    th, tw = int(tex.shape[0]), int(tex.shape[1])
                    texture = texfinish.finish(torch.from_numpy(tex).to(device), texfinish.coverage_from_obj(obj, th, tw, device=device),
                                               pad=args.tex_pad, erode=getattr(args, "tex_erode", 1))[th]
                renderer = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, texture, device=device)
                verts = torch.from_numpy(training_vertices(obj.vertices, trans_g)).to(device)
                masks = pixel_masks(dataset)
                scores, renders = evaluate_frame(renderer, verts, dataset, masks, keep_renders=True)
                for name, row in scores.items():
                    row["trained"] = trained.get(name, True)
                    for n in list(row):
                        if isinstance(row[n], float):
                            row[n] = _finite(row[n])
                result[key] = {"texture": tex is not None, "masked": masks is not None, "views": scores}
                if args.save_renders:
                    from .png import write_png
                    tag = "" if args.set != "both" else f"_{which}"
                    for name, img in renders.items():
                        write_png(os.path.join(run_dir, key, f"mesh{tag}_{name}.png"), img, chw=True)
    finally:
        for p in pf.values():
            p.close()
    return {"frames": result, "summary": _summary(result)}


def _read_scan_files(run_dir: str, scan_dir: str, t: int, transform):
    """(FaceObj or None, Scan or None) of frame t: the host half, run on the prefetch thread."""
    from . import scanscore
    obj = _run.read_frame_obj(_run.frame_dir(run_dir, t))
    scan = None
    for ext in (".ply", ".obj"):
        path = os.path.join(scan_dir, "%06d%s" % (t, ext))
        if os.path.exists(path):
            scan = scanscore.read_scan(path)
            break
    if scan is not None and transform is not None:
        scan = scanscore.Scan(scan.vertices @ transform[:3, :3].T + transform[:3, 3], scan.faces)
    return obj, scan


def _align_scan(args, vertices, faces, scan, transform, device):
    """scanalign.align_scan of one frame under the --scan_align_* options, --scan_transform as the starting pose and
    --scan_max_dist as the first gate; what it refuses ends the run with the frame's message."""
    from . import scanalign
    try:
        return scanalign.align_scan(vertices, faces, scan, init=transform, metric=args.scan_align_metric, scale=args.scan_align_scale,
                                    max_iter=args.scan_align_iters, max_dist=args.scan_max_dist, stride=args.scan_align_stride, device=device)
    except ValueError as e:
        raise SystemExit(f"--scan_align: {e}") from None


def texfinish_coverage(obj, res: int, device) -> torch.Tensor:
    """The coverage the displacement bake walked: projtex.surface_maps' (texfinish.coverage_from_obj), uint8 [res,res]."""
    from . import texfinish
    return texfinish.coverage_from_obj(obj, int(res), int(res), device=device)


def _scan_summary(frames: dict) -> dict:
    scored = {f: fr for f, fr in frames.items() if "scan_to_mesh" in fr}
    out = {"frames": len(scored)}
    for d in ("scan_to_mesh", "mesh_to_scan"):
        rows = [fr[d] for fr in scored.values() if fr[d].get("count")]
        part = {n: float(np.mean([r[n] for r in rows])) if rows else None for n in ("mean", "rms")}
        keys = list(rows[0]["within"]) if rows else []
        part["within"] = {k: float(np.mean([r["within"][k] for r in rows])) for k in keys}
        out[d] = part
    shot = [fr["mesh_to_scan_normal"] for fr in scored.values() if fr.get("mesh_to_scan_normal", {}).get("count")]
    if any("mesh_to_scan_normal" in fr for fr in scored.values()):
        part = {n: float(np.mean([r[n] for r in shot])) if shot else None for n in ("mean", "rms")}
        part["within"] = {k: float(np.mean([r["within"][k] for r in shot])) for k in (list(shot[0]["within"]) if shot else [])}
        out["mesh_to_scan_normal"] = part
    if any("scan_displaced" in fr for fr in scored.values()):
        xs = [fr["scan_displaced"]["scan_to_mesh"]["mean"] for fr in scored.values()
              if fr.get("scan_displaced", {}).get("scan_to_mesh", {}).get("count")]
        out["scan_displaced"] = {"scan_to_mesh": {"mean": float(np.mean(xs)) if xs else None}}
    baked = [fr["displacement"] for fr in scored.values() if "hit_fraction" in fr.get("displacement", {})]
    if any("displacement" in fr for fr in scored.values()):
        out["displacement"] = {"hit_fraction": float(np.mean([r["hit_fraction"] for r in baked])) if baked else None}
        for n in ("mean", "rms"):
            xs = [r[n] for r in baked if r.get(n) is not None]
            out["displacement"][n] = float(np.mean(xs)) if xs else None
    worst = [(f, fr["scan_to_mesh"]["mean"]) for f, fr in scored.items() if fr["scan_to_mesh"].get("count")]
    out["worst_frame"] = max(worst, key=lambda w: w[1])[0] if worst else None
    return out


def score_scans(args, device) -> dict:
    """The "scan" block of eval.json: per frame the two directions of scanscore.score_scan, and their summary."""
    from . import scanscore
    run_dir = _run.run_dir_of(args)
    transform = None
    if args.scan_transform is not None:
        transform = np.loadtxt(args.scan_transform, dtype=np.float64)
        if transform.shape != (4, 4) or not np.isfinite(transform).all():
            raise SystemExit(f"--scan_transform: {args.scan_transform} does not hold a finite 4x4 matrix")
    result = {}
    bake_disp = getattr(args, "bake_disp", None)
    disp_png = disp_png_options(args)
    disp_apply = getattr(args, "disp_apply", None) if disp_png is not None else None
    tess = None
    align = getattr(args, "scan_align", "none")
    shared = None                                               # --scan_align first: (frame key, composed matrix)
    with _run.prefetched(_run.frames_of(args, run_dir),
                         lambda t: _read_scan_files(run_dir, args.scans, t, transform if align == "none" else None),
                         thread_name="t4d-eval-scan") as walk:
        for t, (obj, scan) in walk:
            key = _run.frame_key(t)
            if obj is None:
                result[key] = {"skipped": "no face.obj"}
                continue
            if scan is None:
                result[key] = {"skipped": "no scan"}
                continue
            faces, _ = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
            alignment = None
            if align != "none":
                # the scan as read, then the composed matrix exactly as a later --scan_transform of the written file applies it
                if align == "each" or shared is None:
                    alignment, path = _align_scan(args, obj.vertices, faces, scan, transform, device), "scan_align.txt"
                    if align == "first":
                        shared = (key, alignment.matrix)
                    if not alignment.converged:
                        print(f"--scan_align: frame {key} ended at --scan_align_iters {args.scan_align_iters} without converging"
                              + (" (--scan_align_scale approaches a scale only linearly)" if args.scan_align_scale else ""), file=sys.stderr)
                    np.savetxt(os.path.join(run_dir, path if align == "first" else os.path.join(key, path)), alignment.matrix, fmt="%.17g")
                matrix = alignment.matrix if align == "each" else shared[1]
                scan = scanscore.Scan(scan.vertices @ matrix[:3, :3].T + matrix[:3, 3], scan.faces)
            bake = bake_disp is not None and scan.faces is not None
            score = scanscore.score_scan(obj.vertices, faces, scan, max_dist=args.scan_max_dist, thresholds=args.scan_thresholds,
                                         unit=args.scan_unit, device=device, per_element=args.save_scan_errors,
                                         **({"shoot": bake_disp} if bake else {}))
            if bake:
                from . import scanbake
                disp, hit, _ = scanbake.bake_displacement(obj, obj.vertices, scan, args.bake_res, bake_disp,
                                                          same_side=not args.bake_both_sides, device=device)
                scanbake.write_frame(os.path.join(run_dir, key), disp, hit)
                score["displacement"] = scanbake.displacement_stats(disp, hit, texfinish_coverage(obj, args.bake_res, device),
                                                                    unit=args.scan_unit)
                if disp_png is not None:
                    from . import dispmap
                    finished = dispmap.finish(obj, obj.vertices, disp, hit, bake_disp, fill=disp_png["fill"], smooth=disp_png["smooth"],
                                              normals=disp_png["normals"], device=device)
                    dispmap.write_frame(os.path.join(run_dir, key), finished)
                    score["displacement"]["filled"] = int(finished["filled"].sum())
                    if disp_apply is not None:
                        from . import projtex, tessellate
                        if tess is None or not tess.matches(obj):
                            tess = tessellate.Tessellation(obj, disp_apply, device=device)
                        labels = projtex.island_labels(obj, args.bake_res, args.bake_res, device=device)
                        fine, sampled = tess.displace(obj.vertices, finished["code"], finished["has"], labels, disp_png["unit"])
                        hi = scanscore.score_scan(fine, tess.faces, scan, max_dist=args.scan_max_dist, thresholds=args.scan_thresholds,
                                                  unit=args.scan_unit, device=device)
                        score["scan_displaced"] = {d: {n: (_finite(v) if isinstance(v, float) else v) for n, v in hi[d].items()}
                                                   for d in ("scan_to_mesh", "mesh_to_scan")}
                        score["tessellation"] = {"level": tess.level, "vertices": tess.n_vertices, "faces": tess.n_faces,
                                                 "unsampled": tess.n_vertices - int(sampled.sum())}
                        if getattr(args, "disp_save_obj", False):
                            tessellate.write_frame(os.path.join(run_dir, key), tess, fine)
            elif bake_disp is not None:
                score["displacement"] = {"skipped": "scan has no faces"}
            arrays = score.pop("arrays", None)
            if arrays is not None:
                np.savez(os.path.join(run_dir, key, "scan_score.npz"), **arrays)
            row = {"scan_vertices": int(len(scan.vertices)), "scan_faces": 0 if scan.faces is None else int(len(scan.faces))}
            for d, stats in score.items():
                row[d] = {n: (_finite(v) if isinstance(v, float) else v) for n, v in stats.items()}
            if alignment is not None:
                row["alignment"] = alignment.as_dict()
            result[key] = row
    out = {"unit": args.scan_unit, "max_dist": args.scan_max_dist, "frames": result, "summary": _scan_summary(result)}
    if align != "none":
        out["align"] = {"mode": align, "metric": args.scan_align_metric, "scale": bool(args.scan_align_scale),
                        "iters": int(args.scan_align_iters), "stride": int(args.scan_align_stride)}
        if align == "first":
            out["align"]["frame"] = None if shared is None else shared[0]
    if bake_disp is not None:
        out["bake"] = {"dist": bake_disp, "res": args.bake_res, "same_side": not args.bake_both_sides}
        if disp_png is not None:
            out["bake"]["png"] = disp_png
            if disp_apply is not None:
                out["bake"]["apply"] = int(disp_apply)
    return out


def disp_png_options(args) -> Optional[dict]:
    """dispmap.png_info for --disp_png / --disp_fill / --disp_smooth / --disp_normals / --disp_apply (the last four imply the
    first); None without any of them."""
    fill, rounds, normals = (getattr(args, n, d) for n, d in (("disp_fill", False), ("disp_smooth", 0), ("disp_normals", False)))
    apply = getattr(args, "disp_apply", None) is not None
    if not (getattr(args, "disp_png", False) or fill or rounds or normals or apply) or getattr(args, "bake_disp", None) is None:
        return None
    from . import dispmap
    return dispmap.png_info(args.bake_disp, fill, rounds, normals)


def _floats(spec: str) -> List[float]:
    try:
        out = [float(x) for x in spec.split(",") if x.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"{spec!r} is not a comma-separated list of numbers") from None
    if not out or len(out) > 8 or any(not (x >= 0.0) for x in out):
        raise argparse.ArgumentTypeError(f"{spec!r}: need 1 to 8 thresholds >= 0")
    return out


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.evaluate",
                                description="Render each frame's face.obj + face.png into the capture views and score it.")
    _run.add_run_flags(p, "exp", "seq", "input_dir", "dense_input_dir", "output_dir", "down_ratio",
                       frames_help="Frames to score: '1-10', '1,5,9' (default: every frame directory).")
    p.add_argument("--views", type=_run.view_list, default=None,
                   help="Cameras to score, comma-separated (default: every camera, blacklisted ones included).")
    p.add_argument("--set", choices=("low", "dense", "both", "none"), default="low",
                   help="Views to score against: the geometry inputs (-id), the texture inputs (-did), both, or none (scans only).")
    p.add_argument("--save_renders", action="store_true", help="Also write %%06d/mesh_<cam>.png.")
    p.add_argument("--undistort", action="store_true",
                   help="Undistort the photographs by the lens calibration of cameras.xml, as topo4d_amd.train --undistort does.")
    p.add_argument("--tex_pad", type=int, default=None, metavar="R",
                   help="Pad the UV islands of every face.png by R texels (0..64) in memory before sampling it (texfinish.finish).")
    p.add_argument("--tex_erode", type=int, default=1, metavar="E",
                   help="With --tex_pad: rounds of erosion (0..4) of the face.obj coverage before padding (default 1).")
    p.add_argument("--texture", default=TEXTURE_FILE, metavar="NAME",
                   help="The file of every frame directory that is sampled (default face.png), e.g. face_proj.png.")
    p.add_argument("--scans", default=None, metavar="DIR",
                   help="Also score each frame's face.obj against its 3D scan DIR/%%06d.ply (else DIR/%%06d.obj).")
    p.add_argument("--scan_max_dist", type=float, default=None,
                   help="Scan scoring: leave out pairs farther apart than this, in file units (default: none left out).")
    p.add_argument("--scan_unit", type=float, default=1.0, help="Scan scoring: reported unit per file unit, e.g. 1000 for metres -> mm.")
    p.add_argument("--scan_thresholds", type=_floats, default=[0.5, 1.0, 2.0],
                   help="Scan scoring: report the fraction of distances under each, in reported units (default 0.5,1,2).")
    p.add_argument("--scan_transform", default=None, metavar="FILE", help="Scan scoring: a 4x4 text matrix applied to every scan.")
    p.add_argument("--save_scan_errors", action="store_true",
                   help="Scan scoring: also write %%06d/scan_score.npz (face_count, face_mean, vertex_dist).")
    p.add_argument("--scan_align", choices=("none", "first", "each"), default="none",
                   help="Scan scoring: align each scan rigidly to its frame's mesh before it is scored (scanalign.align_scan, with "
                        "--scan_transform as the starting pose): 'each' frame on its own, or the 'first' scored frame's transform for "
                        "all frames.  Writes scan_align.txt (first) or %%06d/scan_align.txt (each), which --scan_transform reads.")
    p.add_argument("--scan_align_scale", action="store_true", help="--scan_align: also estimate one scale (a similarity).  The scale is approached only linearly: more than a few "
                        "per cent off needs hundreds of --scan_align_iters, and a change of unit belongs in --scan_transform; a phase "
                        "that ends at the limit is reported (\"converged\": false, and a warning).")
    p.add_argument("--scan_align_metric", choices=("plane", "point"), default="plane",
                   help="--scan_align: distances along the mesh normals (default) or to the closest points.")
    p.add_argument("--scan_align_iters", type=int, default=30, metavar="N", help="--scan_align: iterations at the most (default 30).")
    p.add_argument("--scan_align_stride", type=int, default=1, metavar="K", help="--scan_align: use every K-th scan vertex (default 1).")
    p.add_argument("--bake_disp", type=float, default=None, metavar="DIST",
                   help="With --scans: bake each frame's scan into %%06d/face_disp.npy and face_disp_hit.png, a displacement map in the "
                        "UV layout of face.obj, with rays of reach DIST (scan file units) along the surface normal, both ways.")
    p.add_argument("--bake_res", type=int, default=4096, metavar="N",
                   help="--bake_disp: the side of the displacement map (default 4096; evaluate has no texture size of its own).")
    p.add_argument("--bake_both_sides", action="store_true",
                   help="--bake_disp: also count scan triangles whose normal points against the texel's normal.")
    p.add_argument("--disp_png", action="store_true",
                   help="--bake_disp: also write %%06d/face_disp.png, the map as a 16-bit grey PNG (32768 = none, step DIST / 32767).")
    p.add_argument("--disp_fill", action="store_true",
                   help="--bake_disp: fill the texels whose ray missed from their UV island before writing the PNG (implies --disp_png).")
    p.add_argument("--disp_smooth", type=int, default=0, metavar="K",
                   help="--bake_disp: smooth the map K rounds (0..8) within the UV islands (K > 0 implies --disp_png).")
    p.add_argument("--disp_normals", action="store_true",
                   help="--bake_disp: also write %%06d/face_disp_normal.png, the 16-bit tangent-space normal map (implies --disp_png).")
    p.add_argument("--disp_apply", type=int, default=None, metavar="N",
                   help="--bake_disp: tessellate each frame's mesh into N segments per edge (1..64), displace it by the finished map and "
                        "score it against the scan too (implies --disp_png).")
    p.add_argument("--disp_save_obj", action="store_true", help="--disp_apply: also write %%06d/face_hi.obj, the displaced mesh.")
    p.add_argument("--drift", action="store_true",
                   help="Also measure the tracking drift between the frames' UV textures (topo4d_amd.drift); eval.json gains \"drift\".")
    from . import drift
    drift.add_options(p, prefix="drift_")
    return p


def evaluate(args, device=None) -> dict:
    dev = torch.device(device if device is not None else "cuda")
    run_dir = _run.run_dir_of(args)
    sets ={"both": ["low", "dense"], "none": []}.get(args.set, [args.set])
    scans = getattr(args, "scans", None)
    if scans is not None and not os.path.isdir(scans):
        raise SystemExit(f"--scans: no directory {scans}")
    with_drift = bool(getattr(args, "drift", False))
    if not sets and scans is None and not with_drift:
        raise SystemExit("--set none scores nothing without --scans or --drift")
    if getattr(args, "scan_align", "none") != "none":
        if scans is None:
            raise SystemExit("--scan_align needs --scans")
        from . import scanalign
        try:
            scanalign.check_options(args.scan_align_metric, args.scan_align_iters, args.scan_max_dist, stride=args.scan_align_stride)
        except ValueError as e:
            raise SystemExit(f"--scan_align: {e}") from None
    bake_disp = getattr(args, "bake_disp", None)
    if bake_disp is not None:
        if scans is None:
            raise SystemExit("--bake_disp needs --scans")
        if not (math.isfinite(bake_disp) and bake_disp >= 0.0) or not 1 <= args.bake_res <= 16384:
            raise SystemExit("--bake_disp needs a finite DIST >= 0 and --bake_res in 1..16384")
    disp_apply = getattr(args, "disp_apply", None)
    if getattr(args, "disp_save_obj", False) and disp_apply is None:
        raise SystemExit("--disp_save_obj needs --disp_apply")
    if any(getattr(args, n, 0) for n in ("disp_png", "disp_fill", "disp_smooth", "disp_normals")) or disp_apply is not None:
        if bake_disp is None or not bake_disp > 0.0:
            raise SystemExit("--disp_png, --disp_fill, --disp_smooth, --disp_normals and --disp_apply need --bake_disp with DIST > 0")
        if disp_apply is not None:
            from . import tessellate
            try:
                tessellate.check_level(disp_apply)
            except ValueError as e:
                raise SystemExit(f"--disp_apply: {e}") from None
        from . import dispmap
        try:
            dispmap.check_options(bake_disp, args.disp_smooth)
        except ValueError as e:
            raise SystemExit(f"--disp_smooth: {e}") from None
    tex_pad = getattr(args, "tex_pad", None)
    if tex_pad is not None:
        from . import texfinish
        try:
            texfinish.check_options(tex_pad, getattr(args, "tex_erode", 1), (), 1)
        except ValueError as e:
            raise SystemExit(f"--tex_pad / --tex_erode: {e}") from None
    with torch.cuda.device(dev):
        out = {"exp": args.exp, "seq": args.seq, "blacklist": sorted(C.BLACKLIST), "mask_labels": MASK_LABELS}
        if tex_pad is not None:
            out["tex_pad"], out["tex_erode"] = int(tex_pad), int(getattr(args, "tex_erode", 1))
        if getattr(args, "texture", TEXTURE_FILE) != TEXTURE_FILE:
            out["texture_file"] = args.texture
        for which in sets:
            out[which] = score_set(args, which, dev)
        if scans is not None:
            out["scan"] = score_scans(args, dev)
        if with_drift:
            from . import drift
            out["drift"] = drift.drift_tree(args, dev, options=drift.options_of(args, "drift_"))
    with open(os.path.join(run_dir, "eval.json"), "w") as f:
        json.dump(out, f, indent=1)
    return out


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    out = evaluate(args)
    for which in ("low", "dense"):
        if which in out:
            print(which, json.dumps(out[which]["summary"]))
    if "scan" in out:
        print("scan", json.dumps(out["scan"]["summary"]))
    if "drift" in out:
        print("drift", json.dumps(out["drift"]["summary"]))


if __name__ == "__main__":
    main()
