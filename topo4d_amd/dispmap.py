"""
Finishing a baked displacement map (scanbake.bake_displacement) into files a renderer loads, on the GPU, over csrc/t4d_dispmap.hip,
t4d_texture_fill16 and t4d_png_encode16 (include/topo4d_raster.h states the exact rules, tests/dispmap_ref.py restates them):

    quantize(disp, hit, dist)                  -> (code int32 [h,w], has uint8 [h,w]): 16-bit codes, 32768 = no displacement, one
                                               step = dist / 32767 scan units; has = hit and a finite value
    smooth(code, has, labels, rounds)          rounds (0..8) of a 5x5 binomial filter over the texels of the same UV island that
                                               have a value
    normals(code, has, labels, pos, unit)      int32 [h,w,3]: the tangent-space normal map (+u right, +v up: the OpenGL convention),
                                               16 bits a component, (32768, 32768, 65535) where there is no value
    finish(face_obj, vertices, disp, hit, dist, fill=False, smooth=0, normals=False)
                                               -> {"code", "has", "filled"[, "normal"]}: quantise, fill, smooth, normals, in that order
    write_frame(frame_dir, result)             face_disp.png (16-bit grey) and, with a normal map, face_disp_normal.png (16-bit RGB)

A code map is a torch.int32 tensor holding 0..65535 (torch.uint16 has too few device ops).  The fill is texfinish.fill16_islands
over projtex.island_labels: every texel of an island that the bake's ray missed takes the push-pull interpolation of that island's
values, and counts as having a value afterwards.  The displacement in scan units is (code - 32768) * dist / 32767.

Known limits: the normal map takes the slope of the displacement along u and along v separately, each through the surface's own
texel length (projtex.surface_maps' points), so a stretched UV layout is handled; the shear between dp/du and dp/dv and the
curvature terms are ignored (no shear-aware tangent frame, no MikkTSpace).  The 16-bit maps get no gutter round their islands
(texfinish.pad is 8-bit), and there is no EXR.  There is no CPU path.

`python -m topo4d_amd.dispmap -e EXP -s SEQ -od DIR [--frames 1-10] --dist DIST [--fill] [--smooth K] [--normals]` finishes an
output tree that already holds %06d/face_disp.npy, face_disp_hit.png and face.obj (evaluate --bake_disp DIST wrote them): the files
are those `evaluate --bake_disp DIST --disp_png ...` writes.  Frames without all three files are left alone.
"""
from __future__ import annotations

import argparse
import math
import os
from typing import Tuple

import numpy as np
import torch

from . import _args, _lib, _run
from ._lib import on_device, ptr

ZERO = 32768
STEPS = 32767
MAX_ROUNDS = 8
PNG_NAME = "face_disp.png"
NORMAL_NAME = "face_disp_normal.png"


def code_unit(dist: float) -> float:
    """Scan units per code step."""
    return float(dist) / STEPS


def check_options(dist, smooth=0) -> None:
    """ValueError for a reach or a round count that finish would refuse (callable without a device)."""
    try:
        d = float(dist)
    except (TypeError, ValueError):
        raise ValueError(f"dist must be a finite distance > 0, got {dist!r}") from None
    if not (math.isfinite(d) and d > 0.0):
        raise ValueError(f"dist must be a finite distance > 0, got {dist}")
    if isinstance(smooth, bool) or int(smooth) != smooth or not 0 <= int(smooth) <= MAX_ROUNDS:
        raise ValueError(f"smooth must be a whole number of rounds in [0, {MAX_ROUNDS}], got {smooth}")


def _map(t, what: str, dtypes, tail=()) -> Tuple[int, int]:
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != 2 + len(tail) or tuple(t.shape[2:]) != tuple(tail):
        names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{what} must be a {names} [h,w{''.join(',%d' % n for n in tail)}] tensor, got "
                         f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', ()))}")
    h, w = int(t.shape[0]), int(t.shape[1])
    if h < 1 or w < 1:
        raise ValueError(f"{what} must have h, w >= 1, got {tuple(t.shape)}")
    return h, w


def quantize(disp: torch.Tensor, hit: torch.Tensor, dist: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(code int32 [h,w], has uint8 [h,w]) of a displacement map (float32 [h,w], scan units) and its hit mask under the reach
    `dist`: where hit and disp is finite, code = 32768 + clamp(rint(disp / dist * 32767), -32767, 32767) in float64 with ties to
    even, and has = 1; elsewhere 32768 and 0."""
    h, w = _map(disp, "disp", (torch.float32,))
    _args.mask(hit, "hit", h, w)
    check_options(dist)
    d = on_device(disp, "disp")
    m = on_device(hit, "hit", d.device)
    code = torch.empty(h, w, dtype=torch.int32, device=d.device)
    has = torch.empty(h, w, dtype=torch.uint8, device=d.device)
    _lib.call("t4d_disp_quantize", ptr(d), ptr(m), h, w, float(dist), ptr(code), ptr(has), _lib.stream(d.device))
    return code, has


def _code_args(code, has, labels) -> Tuple[int, int]:
    h, w = _map(code, "code", (torch.int32,))
    _args.mask(has, "has", h, w)
    _args.mask(labels, "labels", h, w, (torch.uint8,))
    return h, w


def smooth(code: torch.Tensor, has: torch.Tensor, labels: torch.Tensor, rounds: int) -> torch.Tensor:
    """`rounds` rounds of t4d_disp_smooth: a texel with a value and a label takes the (1, 4, 6, 4, 1)^2 weighted mean, rounded
    half up, of the taps inside the image that have a value and carry its label; every other texel is copied through."""
    h, w = _code_args(code, has, labels)
    check_options(1.0, rounds)
    c = on_device(code, "code")
    m, lab = on_device(has, "has", c.device), on_device(labels, "labels", c.device)
    scratch, nbytes = _lib.scratch("t4d_disp_smooth_scratch_bytes", c.device, h, w)
    out = torch.empty_like(c)
    _lib.call("t4d_disp_smooth", ptr(c), ptr(m), ptr(lab), h, w, int(rounds), ptr(out), ptr(scratch), nbytes, _lib.stream(c.device))
    return out


def normals(code: torch.Tensor, has: torch.Tensor, labels: torch.Tensor, pos: torch.Tensor, unit: float) -> torch.Tensor:
    """int32 [h,w,3]: t4d_disp_normals' tangent-space normal map of the surface `pos` (float32 [h,w,3], projtex.surface_maps)
    displaced by (code - 32768) * unit along its normal; see the module's known limits."""
    h, w = _code_args(code, has, labels)
    _map(pos, "pos", (torch.float32,), (3,))
    if tuple(pos.shape[:2]) != (h, w):
        raise ValueError(f"pos {tuple(pos.shape)} does not match the map's [{h},{w}]")
    u = float(unit)
    if not (math.isfinite(u) and u > 0.0):
        raise ValueError(f"unit must be finite and > 0, got {unit}")
    c = on_device(code, "code")
    m, lab, p = on_device(has, "has", c.device), on_device(labels, "labels", c.device), on_device(pos, "pos", c.device)
    out = torch.empty(h, w, 3, dtype=torch.int32, device=c.device)
    _lib.call("t4d_disp_normals", ptr(c), ptr(m), ptr(lab), ptr(p), h, w, u, ptr(out), _lib.stream(c.device))
    return out


_smooth, _normals = smooth, normals                           # finish's keyword arguments carry the same names


def finish(face_obj, vertices, disp: torch.Tensor, hit: torch.Tensor, dist: float, fill: bool = False, smooth: int = 0,
           normals: bool = False, device=None) -> dict:
    """{"code": int32 [h,w], "has": uint8 [h,w], "filled": uint8 [h,w][, "normal": int32 [h,w,3]]} of a bake (disp, hit:
    scanbake.bake_displacement's maps of `face_obj` with `vertices` under the reach `dist`).  In this order: quantize; with `fill`,
    texfinish.fill16_islands over projtex.island_labels with the texels that have a value as the valid ones, after which the filled
    texels have a value too (has = has | filled); `smooth` rounds of smoothing; with `normals`, the normal map over
    projtex.surface_maps' points with unit = dist / 32767."""
    from . import projtex, texfinish
    h, w = _map(disp, "disp", (torch.float32,))                # argument errors first, with or without a device
    _args.mask(hit, "hit", h, w)
    check_options(dist, smooth)
    dev = _lib.hip_device(device, "the displacement map", ValueError)
    with torch.cuda.device(dev):
        code, has = quantize(disp.to(dev), hit.to(dev), dist)
        filled = torch.zeros(h, w, dtype=torch.uint8, device=dev)
        labels = projtex.island_labels(face_obj, h, w, device=dev) if (fill or smooth or normals) else None
        if fill:
            code, filled = texfinish.fill16_islands(code, has, labels)
            has = has | filled
        if smooth:
            code = _smooth(code, has, labels, int(smooth))
        out = {"code": code, "has": has, "filled": filled}
        if normals:
            v = vertices if isinstance(vertices, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vertices, np.float64))
            pos = projtex.surface_maps(face_obj, v.detach().to(dev), (h, w), device=dev)[0]
            out["normal"] = _normals(code, has, labels, pos, code_unit(dist))
    return out


def write_frame(frame_dir: str, result: dict) -> list:
    """finish's result as files in `frame_dir`: face_disp.png (16-bit grey, the codes) and, if the result holds a normal map,
    face_disp_normal.png (16-bit RGB); returns the paths."""
    from .png import write_png16
    paths = [os.path.join(frame_dir, PNG_NAME)]
    write_png16(paths[0], result["code"])
    if "normal" in result:
        paths.append(os.path.join(frame_dir, NORMAL_NAME))
        write_png16(paths[1], result["normal"])
    return paths


def png_info(dist: float, fill: bool, smooth: int, normals: bool) -> dict:
    """What eval.json's "bake" says about the PNG: how to read a code back and the steps taken."""
    return {"zero": ZERO, "unit": code_unit(dist), "fill": bool(fill), "smooth": int(smooth), "normals": bool(normals)}


# ---- command line ----------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.dispmap",
                                description="Finish every frame's baked displacement map: 16-bit PNG, hole fill, smoothing, normal map.")
    _run.add_run_flags(p, "exp", "seq", "output_dir", frames_help="Frames to finish: '1-10', '1,5,9' (default: every frame directory).")
    p.add_argument("--dist", type=float, required=True, metavar="DIST", help="The reach the maps were baked with (evaluate --bake_disp).")
    p.add_argument("--fill", action="store_true", help="Fill the texels the bake's rays missed, per UV island (push-pull).")
    p.add_argument("--smooth", type=int, default=0, metavar="K", help=f"Rounds of smoothing within the islands, 0..{MAX_ROUNDS} (default 0).")
    p.add_argument("--normals", action="store_true", help="Also write face_disp_normal.png, the tangent-space normal map.")
    return p


def finish_tree(args, device=None) -> list:
    """The files written for the run <od>/<exp>/<seq>; frames without face.obj, face_disp.npy or face_disp_hit.png are left alone."""
    from . import scanbake
    try:
        check_options(args.dist, args.smooth)
    except ValueError as e:
        raise SystemExit(f"--dist / --smooth: {e}") from None
    dev = torch.device(device if device is not None else "cuda")
    run_dir = _run.run_dir_of(args)
    written = []
    with torch.cuda.device(dev):
        for t in _run.frames_of(args, run_dir):
            paths = _run.frame_files(run_dir, t, "face.obj", scanbake.DISP_NAME, scanbake.HIT_NAME)
            if paths is None:
                continue
            frame_dir = _run.frame_dir(run_dir, t)
            obj = _run.read_frame_obj(frame_dir)
            disp = np.load(paths[1])
            hit = _run.read_hit_mask(paths[2])
            if disp.dtype != np.float32 or disp.ndim != 2 or hit.shape != disp.shape:
                raise SystemExit(f"{frame_dir}: {scanbake.DISP_NAME} must be float32 [h,w] and {scanbake.HIT_NAME} of the same size")
            result = finish(obj, obj.vertices, torch.from_numpy(disp).to(dev), torch.from_numpy(hit).to(dev), args.dist,
                            fill=args.fill, smooth=args.smooth, normals=args.normals, device=dev)
            written += write_frame(frame_dir, result)
    return written


def main(argv=None) -> None:
    _run.print_written(finish_tree(build_parser().parse_args(argv)))


if __name__ == "__main__":
    main()
