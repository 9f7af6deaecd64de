"""
The capture photographs projected into a frame's UV texture on the GPU, over csrc/t4d_projtex.hip (include/topo4d_raster.h
states the per-texel rule; tests/projtex_ref.py restates it in numpy bit for bit):

    project(pos, nrm, coverage, cams, photos, depth, ...)   -> (color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8)
    surface_maps(face_obj, vertices, res, device)           -> (pos [h,w,3], nrm [h,w,3], coverage [h,w]) of a face.obj's UV layout
    project_frame(face_obj, vertices, dataset, res, ...)    -> (texture [h,w,3] uint8, weight, count): one frame from its views

Every texel is coloured from the cameras that see it: a view counts when the texel's point projects inside its photograph,
in front of the near plane, is not hidden (the depth map of meshrender.MeshRenderer.render, within depth_tol) and faces the
camera (cos of the angle between normal and viewing direction >= cos_min).  mode="weighted" blends the views by cos^power,
faded over fade_px pixels towards the image edge; mode="best" keeps the single view of largest weight.  The four defaults are
conventional choices, not tuned on a capture.  Unlike face.png (the texture loop's Gaussian-filtered
colour field) this is the photographs themselves.  There is no CPU path.

`python -m topo4d_amd.projtex -e EXP -s SEQ [-id ... -did ... -od ... -dr N] [--frames 1-10] [--views A,B] [--set low|dense]
[--undistort] [--tex_res R] [--mode weighted|best] [--power P --cos_min C --fade_px F --depth_tol T] [--tex_pad R]
[--tex_sizes 2048,1024] [--save_weight]` works on an output tree that already exists (the reference's too): it writes
%06d/face_proj.png (and face_proj_<size>.png) beside every frame's face.obj, with --save_weight also face_proj_weight.png (the
8-bit count of contributing views).  By default it projects the full-size photographs of the cameras training uses.
`python -m topo4d_amd.train --tex_project` writes the same file while the run is made.
"""
from __future__ import annotations

import argparse
import functools
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ptr

T4D_PROJTEX_WEIGHTED, T4D_PROJTEX_BEST = 0, 1
_MODES = {"weighted": T4D_PROJTEX_WEIGHTED, "best": T4D_PROJTEX_BEST}
MAX_POWER, MAX_VIEWS = 8, 255
DEFAULTS = dict(power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002, mode="weighted")
FILE_NAME, WEIGHT_NAME = "face_proj.png", "face_proj_weight.png"


def check_options(power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002, mode="weighted") -> None:
    """ValueError for a parameter project would refuse (callable without a device)."""
    if mode not in _MODES:
        raise ValueError(f"mode must be 'weighted' or 'best', got {mode!r}")
    if isinstance(power, bool) or int(power) != power or not 0 <= int(power) <= MAX_POWER:
        raise ValueError(f"power must be an integer in [0, {MAX_POWER}], got {power!r}")
    if not -1.0 <= float(cos_min) <= 1.0:
        raise ValueError(f"cos_min must be in [-1, 1], got {cos_min!r}")
    if not 0.0 <= float(fade_px) <= 65536.0:
        raise ValueError(f"fade_px must be in [0, 65536], got {fade_px!r}")
    if not 0.0 <= float(depth_tol) <= 1.0:
        raise ValueError(f"depth_tol must be in [0, 1], got {depth_tol!r}")


def _map(t, what: str, shape, dtype) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be a {str(dtype).split('.')[-1]} tensor of shape {list(shape)}, got "
                         f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', ()))}")
    return t


def project(pos: torch.Tensor, nrm: torch.Tensor, coverage: torch.Tensor, cams, photos: torch.Tensor, depth: torch.Tensor, *,
            power: int = 2, cos_min: float = 0.1, fade_px: float = 16.0, depth_tol: float = 0.002,
            mode: str = "weighted") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8).  pos / nrm [h,w,3] float32: each texel's point in the
    training world frame and its normal (any length; a zero normal switches the texel off); coverage [h,w] uint8 or bool;
    cams: a sequence of GaussianRasterizationSettings of one size, or (packed view records, H, W), as MeshRenderer.render takes
    them; photos [V,3,H,W] float32; depth [V,1,H,W] float32, MeshRenderer.render's (0: empty).  Everything on one HIP device."""
    check_options(power, cos_min, fade_px, depth_tol, mode)
    if not isinstance(pos, torch.Tensor) or pos.dim() != 3 or pos.shape[2] != 3 or pos.shape[0] < 1 or pos.shape[1] < 1:
        raise ValueError(f"pos must be a float32 [h,w,3] tensor, got {list(getattr(pos, 'shape', ()))}")
    h, w = int(pos.shape[0]), int(pos.shape[1])
    _map(pos, "pos", (h, w, 3), torch.float32)
    _map(nrm, "nrm", (h, w, 3), torch.float32)
    if not isinstance(coverage, torch.Tensor) or coverage.dtype not in (torch.uint8, torch.bool) or tuple(coverage.shape) != (h, w):
        raise ValueError(f"coverage must be a uint8 or bool [{h},{w}] tensor")
    dev = pos.device
    from .meshrender import _views
    views, H, W = _views(cams, dev)
    V = int(views.shape[0])
    if V > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views per call, got {V}")
    _map(photos, "photos", (V, 3, H, W), torch.float32)
    _map(depth, "depth", (V, 1, H, W), torch.float32)
    for name, t in (("nrm", nrm), ("coverage", coverage), ("photos", photos), ("depth", depth)):
        if t.device != dev:
            raise ValueError(f"{name} must live on pos's device {dev}, got {t.device}")
    if not pos.is_cuda:                                        # argument errors first, with or without a device
        raise RuntimeError("topo4d_amd has no CPU path: the maps, the photographs and the depth must live on a HIP device")
    cov = (coverage.to(torch.uint8) if coverage.dtype == torch.bool else coverage).contiguous()
    pos, nrm, photos, depth = pos.contiguous(), nrm.contiguous(), photos.contiguous(), depth.contiguous()
    color = torch.empty(h, w, 3, dtype=torch.float32, device=dev)
    weight = torch.empty(h, w, dtype=torch.float32, device=dev)
    count = torch.empty(h, w, dtype=torch.uint8, device=dev)
    _lib.call("t4d_project_texture", ptr(pos), ptr(nrm), ptr(cov), h, w, ptr(views), V, H, W, ptr(photos), ptr(depth), int(power),
              float(cos_min), float(fade_px), float(depth_tol), _MODES[mode], ptr(color), ptr(weight), ptr(count), _lib.stream(dev))
    return color, weight, count


def _size(res) -> Tuple[int, int]:
    h, w = (res, res) if isinstance(res, (int, np.integer)) else res
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"res must be a positive size or (h, w), got {res!r}")
    return h, w


def uv_vertex_owner(faces: np.ndarray, uv_faces: np.ndarray, n_uv: int) -> np.ndarray:
    """int64 [n_uv]: the mesh vertex at each UV vertex, through the matching corners of faces / uv_faces; where several mesh
    vertices share one UV vertex the corner of the lowest face index (then the lowest corner) wins; -1 for a UV vertex no face
    names."""
    fv, ft = np.asarray(faces, np.int64).reshape(-1), np.asarray(uv_faces, np.int64).reshape(-1)
    owner = np.full(int(n_uv), -1, dtype=np.int64)
    uniq, first = np.unique(ft, return_index=True)
    owner[uniq] = fv[first]
    return owner


def surface_maps(face_obj, vertices: torch.Tensor, res, device=None):
    """(pos [h,w,3] float32, nrm [h,w,3] float32, coverage [h,w] uint8) of `face_obj` (meshrender.FaceObj) at res (a size, or
    (h, w)): per texel the point on the surface and its normal.  vertices [N,3]: the mesh vertices in the training world frame,
    on the device.  Each UV vertex carries the position and the objexport.vertex_normals normal of its mesh vertex, found through
    the matching corners of the triangulated faces / uv_faces; if several mesh vertices share a UV vertex, the one in the lowest
    face index wins.  texture.render_colors interpolates them over texture.process_uv's UVs, exactly as the bake interpolates
    colours (float32; the normal is not of unit length afterwards), and the coverage is texfinish.coverage_from_obj's."""
    from . import meshrender, objexport, texfinish, texture
    h, w = _size(res)
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_floating_point():
        raise ValueError("vertices must be a float [N,3] tensor")
    dev = meshrender._device(device if device is not None else (vertices.device if vertices.is_cuda else None))
    if vertices.device != dev:
        raise RuntimeError(f"topo4d_amd has no CPU path: vertices must live on {dev}, got {vertices.device}")
    faces, uv_faces = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
    n_uv = len(face_obj.uvs)
    if faces.size and (faces.min() < 0 or faces.max() >= int(vertices.shape[0])):
        raise ValueError(f"faces name vertex {int(faces.max())} but only {int(vertices.shape[0])} vertices were given")
    owner = uv_vertex_owner(faces, uv_faces, n_uv)
    idx = torch.from_numpy(np.maximum(owner, 0)).to(dev)
    v = vertices.detach()
    normals = objexport.vertex_normals(v, faces)
    uv_verts = texture.process_uv(face_obj.uvs, h, w)
    pos = texture.render_colors(uv_verts, uv_faces, v.to(torch.float32)[idx], h, w, c=3, device=dev)
    nrm = texture.render_colors(uv_verts, uv_faces, normals.to(torch.float32)[idx], h, w, c=3, device=dev)
    return pos, nrm, texfinish.coverage_from_obj(face_obj, h, w, device=dev)


def project_frame(face_obj, vertices: torch.Tensor, dataset, res, *, power: int = 2, cos_min: float = 0.1, fade_px: float = 16.0,
                  depth_tol: float = 0.002, mode: str = "weighted", device=None):
    """(texture [h,w,3] uint8, weight [h,w] float32, count [h,w] uint8) of one frame: `dataset` holds ingest.get_dataset's entries
    ("cam", "im"), vertices [N,3] the mesh in the training world frame.  The mesh is rendered once for the depth maps
    (meshrender.MeshRenderer over a 1x1 dummy texture), surface_maps gives the texel maps, project gathers, texfinish.quantize
    rounds as the PNG encoder does.  Views of one size go in one launch; a rig with several sizes (turned cameras) is merged
    per size: weighted sums add up, "best" keeps the larger weight, the earlier size on ties."""
    from . import meshrender, texfinish
    check_options(power, cos_min, fade_px, depth_tol, mode)
    if not dataset:
        raise ValueError("project_frame: no views")
    faces, uv_faces = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
    dev = meshrender._device(device if device is not None else (vertices.device if vertices.is_cuda else None))
    renderer = meshrender.MeshRenderer(faces, uv_faces, face_obj.uvs, np.zeros((1, 1, 3), np.uint8), device=dev)
    pos, nrm, cov = surface_maps(face_obj, vertices, res, device=dev)
    groups = {}
    for k, e in enumerate(dataset):
        groups.setdefault((int(e["cam"].image_height), int(e["cam"].image_width)), []).append(k)
    total = None
    for ks in groups.values():
        cams = [dataset[k]["cam"] for k in ks]
        _, depth, _ = renderer.render(vertices, cams)
        photos = torch.stack([dataset[k]["im"] for k in ks]).to(torch.float32)
        color, weight, count = project(pos, nrm, cov, cams, photos, depth, power=power, cos_min=cos_min, fade_px=fade_px,
                                       depth_tol=depth_tol, mode=mode)
        if total is None:
            total = [color, weight, count]
            continue
        c0, w0, n0 = total
        if mode == "best":
            take = weight > w0
            total = [torch.where(take[..., None], color, c0), torch.where(take, weight, w0), n0 + count]
        else:
            ws = w0 + weight
            mixed = (c0 * w0[..., None] + color * weight[..., None]) / ws.clamp_min(torch.finfo(torch.float32).tiny)[..., None]
            total = [torch.where((ws > 0)[..., None], mixed, torch.zeros_like(mixed)), ws, n0 + count]
    color, weight, count = total
    return texfinish.quantize(color), weight, count


def write_frame(frame_dir, face_obj, trans_g, dataset, res, options: dict, pad: int = 0, sizes=(), save_weight: bool = False,
                device=None) -> list:
    """One frame's face_proj.png (and face_proj_<size>.png, face_proj_weight.png) in `frame_dir`, from the face.obj read there:
    what the command line and train --tex_project both call.  Returns the files written.  The gutter of `pad` texels is filled
    from the texels some view contributed to (count > 0), through texfinish.finish."""
    from . import texfinish
    from .evaluate import training_vertices
    from .png import write_png
    dev = torch.device(device if device is not None else "cuda")
    verts = torch.from_numpy(training_vertices(face_obj.vertices, trans_g)).to(dev)
    tex, _, count = project_frame(face_obj, verts, dataset, res, device=dev, **options)
    levels = texfinish.finish(tex, (count > 0).to(torch.uint8), pad=pad, erode=0, sizes=sizes)
    written = texfinish.write_levels(os.path.join(frame_dir, FILE_NAME), levels)
    if save_weight:
        path = os.path.join(frame_dir, WEIGHT_NAME)
        write_png(path, count)
        written.append(path)
    return written


# ---- command line ----------------------------------------------------------------------------------------------------------
def add_options(p: argparse.ArgumentParser, suppress: bool = False) -> None:
    """--mode and the four parameters, on the parser of this module and (suppress=True: absent unless given) of train."""
    d = (lambda v: argparse.SUPPRESS) if suppress else (lambda v: v)
    p.add_argument("--mode", choices=tuple(_MODES), default=d(DEFAULTS["mode"]),
                   help="Projection: blend the views that see a texel by their weights, or keep the best one (default weighted).")
    p.add_argument("--power", type=int, default=d(DEFAULTS["power"]), help=f"Projection: weight = cos^power, 0..{MAX_POWER} (default 2).")
    p.add_argument("--cos_min", type=float, default=d(DEFAULTS["cos_min"]),
                   help="Projection: drop a view whose viewing direction makes a cosine below this with the normal (default 0.1).")
    p.add_argument("--fade_px", type=float, default=d(DEFAULTS["fade_px"]),
                   help="Projection: fade a view's weight over this many pixels towards the image edge; 0: no fade (default 16).")
    p.add_argument("--depth_tol", type=float, default=d(DEFAULTS["depth_tol"]),
                   help="Projection: relative slack of the occlusion test against the mesh's depth map (default 0.002).")


def options_of(args) -> dict:
    return {k: getattr(args, k, v) for k, v in DEFAULTS.items()}


def build_parser() -> argparse.ArgumentParser:
    from .evaluate import _frames
    from .train import _size_list, build_parser as train_parser
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.projtex",
                                description="Project the capture photographs into every frame's UV texture: face_proj.png.")
    for a in train_parser()._actions:                         # -e/-s/-id/-did/-od/-dr/-tr exactly as topo4d_amd.train has them
        if a.dest in ("exp", "seq", "input_dir", "dense_input_dir", "output_dir", "down_ratio", "tex_res"):
            p.add_argument(*a.option_strings, type=a.type, default=a.default, help=a.help)
    p.add_argument("--frames", type=_frames, default=None, help="Frames to project: '1-10', '1,5,9' (default: every frame directory).")
    p.add_argument("--views", type=lambda s: [v.strip() for v in s.split(",") if v.strip()], default=None,
                   help="Cameras to project, comma-separated (default: the cameras training uses).")
    p.add_argument("--set", choices=("low", "dense"), default="dense",
                   help="Photographs to project: the texture inputs (-did, the default) or the geometry inputs (-id).")
    p.add_argument("--undistort", action="store_true",
                   help="Undistort the photographs by the lens calibration of cameras.xml, as topo4d_amd.train --undistort does.")
    add_options(p)
    p.add_argument("--tex_pad", type=int, default=0, metavar="R",
                   help="Fill a gutter of R texels (0..64) round the projected texels (texfinish.finish).")
    p.add_argument("--tex_sizes", type=_size_list, default=[],
                   help="Smaller levels to write too, comma-separated, each tex_res / 2^k: face_proj_<size>.png.")
    p.add_argument("--save_weight", action="store_true", help="Also write %%06d/face_proj_weight.png: the number of views per texel.")
    return p


def _check_args(args, res: int) -> dict:
    from . import texfinish
    opts = options_of(args)
    try:
        check_options(**opts)
        texfinish.check_options(getattr(args, "tex_pad", 0), 0, getattr(args, "tex_sizes", ()), res)
    except ValueError as e:
        raise SystemExit(f"projection options: {e}") from None
    return opts


def _read_obj(frame_dir: str):
    from . import meshrender
    path = os.path.join(frame_dir, "face.obj")
    return meshrender.read_face_obj(path) if os.path.exists(path) else None


def project_tree(args, device=None) -> list:
    """The files written for the run <od>/<exp>/<seq>; frames without face.obj or without views are left alone."""
    from . import cameras as C, ingest
    dev = torch.device(device if device is not None else "cuda")
    run_dir = os.path.join(args.output_dir, args.exp, args.seq)
    if not os.path.isdir(run_dir):
        raise SystemExit(f"no run at {run_dir}")
    opts = _check_args(args, args.tex_res)
    low = args.set == "low"
    data_dir = args.input_dir if low else args.dense_input_dir
    cameras, _, trans_g = C.get_cameras(args.input_dir, args.seq, resize_factor=args.down_ratio if low else 1)
    lenses = C.get_lenses(args.input_dir, args.seq, args.down_ratio)[0 if low else 1] if args.undistort else None
    names = [n.split(".")[0] for n in cameras]
    if args.views is None:
        skip = C.BLACKLIST
    else:
        if set(args.views) - set(names):
            raise SystemExit(f"--views: {sorted(set(args.views) - set(names))} not among the cameras of {data_dir}/{args.seq}")
        skip = [n for n in cameras if n.split(".")[0] not in args.views]
    frames = args.frames or sorted(int(d) for d in os.listdir(run_dir) if d.isdigit() and len(d) == 6)
    written = []
    pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="t4d-projtex")
    with torch.cuda.device(dev):
        pf = ingest.FramePrefetcher(data_dir, args.seq, cameras, use_mask=False, blacklist=skip, rotate_mask=C.ROTATE_MASK,
                                    setup_camera=functools.partial(C.setup_camera, device=dev), device=dev, lenses=lenses)
        try:
            pending = {}

            def prefetch(t):
                if t not in pending:
                    pending[t] = pool.submit(_read_obj, os.path.join(run_dir, "%06d" % t))
                    pf.prefetch(t)

            for i, t in enumerate(frames):
                prefetch(t)
                if i + 1 < len(frames):
                    prefetch(frames[i + 1])
                obj = pending.pop(t).result()
                dataset = pf.get(t)
                if obj is None or not dataset:
                    continue
                written += write_frame(os.path.join(run_dir, "%06d" % t), obj, trans_g, dataset, args.tex_res, opts,
                                       pad=args.tex_pad, sizes=args.tex_sizes, save_weight=args.save_weight, device=dev)
        finally:
            pool.shutdown(wait=True)
            pf.close()
    return written


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    for p in project_tree(args):
        print(p)


if __name__ == "__main__":
    main()
