"""
Finishing a baked UV texture on the GPU, over csrc/t4d_texfinish.hip (include/topo4d_raster.h states the exact rules):

    coverage_from_depth(depth)                 uint8 [h,w]: depth > -999999, the texels a bake wrote
    quantize(image_f32)                        float32 [h,w,c] -> uint8, the PNG encoder's rule: numpy's (x*255).astype(np.uint8)
    erode(coverage, rounds)                    rounds (0..4) of 4-neighbour erosion; image edges do not erode
    pad(image, coverage, radius)               -> (image, coverage): every uncovered texel within `radius` (0..64, a disc) of a
                                               covered one takes the nearest covered texel, ties to the smallest (y', x')
    halve(image, coverage)                     -> (image, coverage): 2x2 means over the covered texels only, round half up
    finish(image_u8, coverage, pad, erode, sizes)  -> {res: image}: level 0 and the smaller levels, each with its own gutter
    coverage_from_obj(face_obj, h, w)          the coverage of a face.obj's UV faces, for a tree whose bake is gone
    fill(image, valid, domain=None)            -> (image, filled): every texel of `domain` that is not valid takes a smooth
                                               interpolation of the valid texels: push-pull over a pyramid, csrc/t4d_texfill.hip
    fill_islands(image, valid, labels)         -> (image, filled): fill per UV island, from that island's valid texels alone
    fill16(image_i32, valid, domain=None)      fill for 16-bit samples held in int32 (0..65535): a quantised displacement map
    fill16_islands(image_i32, valid, labels)   fill_islands for them, by the same per-island rule

pad is right for a gutter and wrong for a hole: the nearest texel makes blocky streaks with a crease where two fronts meet.  fill is
for the holes of a projected texture (projtex: the texels no camera sees): the valid texels are averaged down a pyramid over valid
texels alone (halve's rule, in units of 1/256), and every hole takes the bilinear enlargement of the first level that has a colour
for it, so a small hole is filled from its rim and a large one from further away.  Known limit: within one island the fill is an
interpolation in UV space that knows nothing of the surface, so a large hole comes out smooth, not plausible.

Why: face.png is black outside the UV islands and the mesh vertices on a UV seam sit on an island's border, so every bilinear
tap there (meshrender's default, and every viewer's) and every mip level a viewer builds mixes black in.  A gutter of the
island's own border colour removes the seams; levels averaged over covered texels alone keep them out of smaller textures.
Inherited as it is: the reference bake writes the texels of the image's outermost two-texel ring that fall into a triangle's
bounding box by extrapolation, inside the triangle or not (mesh_core.cpp:211); they have a depth and count as covered.

Everything is integer arithmetic on device images; nothing here synchronises or copies to the host.  There is no CPU path.

`python -m topo4d_amd.texfinish -e EXP -s SEQ -od DIR [--frames 1-10] --pad R [--erode 1] [--sizes 2048,1024] [--in_place]`
finishes an output tree that already exists (the reference's too): beside every %06d/face.png it writes face_pad.png and
face_pad_<res>.png for the sizes, from the coverage of the frame's face.obj (accurate to about a texel at the island borders,
hence the default --erode 1); --in_place writes face.png and face_<res>.png instead.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, Sequence, Tuple

import torch

from . import _args, _lib, _run
from ._lib import on_device, ptr

MAX_PAD, MAX_ERODE = 64, 4
_NOTE = {torch.uint8: "", torch.int32: " holding 0..65535"}    # what _args.image says of an image of 8-bit / of 16-bit samples


def _image_and_coverage(image, coverage) -> Tuple[torch.Tensor, torch.Tensor, int, int, int]:
    h, w, c = _args.image(image, "image")
    img = on_device(image, "image")
    _args.mask(coverage, "coverage", h, w)
    return img, on_device(coverage, "coverage", img.device, "the image's"), h, w, c


def coverage_from_depth(depth: torch.Tensor) -> torch.Tensor:
    """uint8 [h,w], 1 where the bake whose depth buffer this is (render_colors(..., return_depth=True)) wrote a texel."""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.dim() != 2:
        raise ValueError("coverage_from_depth expects the float32 [h,w] depth buffer of a bake")
    d = on_device(depth, "the depth buffer")
    h, w = int(d.shape[0]), int(d.shape[1])
    out = torch.empty(h, w, dtype=torch.uint8, device=d.device)
    _lib.call("t4d_texture_coverage", ptr(d), h, w, ptr(out), _lib.stream(d.device))
    return out


def quantize(image_f32: torch.Tensor) -> torch.Tensor:
    """float32 [h,w] / [h,w,c] -> uint8 of the same shape, exactly as png.encode_png quantises a float32 image."""
    if not isinstance(image_f32, torch.Tensor) or image_f32.dtype != torch.float32 or image_f32.dim() not in (2, 3):
        raise ValueError("quantize expects a float32 [h,w] or [h,w,c] tensor")
    img = on_device(image_f32, "the image")
    h, w = int(img.shape[0]), int(img.shape[1])
    c = 1 if img.dim() == 2 else int(img.shape[2])
    if h < 1 or w < 1 or c not in (1, 3, 4):
        raise ValueError(f"quantize: need h, w >= 1 and c in (1, 3, 4); got {tuple(img.shape)}")
    out = torch.empty(img.shape, dtype=torch.uint8, device=img.device)
    _lib.call("t4d_texture_quantize", ptr(img), h, w, c, ptr(out), _lib.stream(img.device))
    return out


def erode(coverage: torch.Tensor, rounds: int) -> torch.Tensor:
    """`rounds` rounds of: a texel stays covered only if it and its 4-neighbours inside the image are covered."""
    rounds = int(rounds)
    if not 0 <= rounds <= MAX_ERODE:
        raise ValueError(f"erode: rounds must be in [0, {MAX_ERODE}], got {rounds}")
    h, w = _args.mask(coverage, "coverage")
    cov = on_device(coverage, "coverage")
    out = torch.empty_like(cov)
    _lib.call("t4d_texture_erode", ptr(cov), h, w, rounds, ptr(out), _lib.stream(cov.device))
    return out


def pad(image: torch.Tensor, coverage: torch.Tensor, radius: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(image, coverage) with every uncovered texel within `radius` of a covered one filled from the nearest (see the module)."""
    radius = int(radius)
    if not 0 <= radius <= MAX_PAD:
        raise ValueError(f"pad: radius must be in [0, {MAX_PAD}], got {radius}")
    img, cov, h, w, c = _image_and_coverage(image, coverage)
    scratch, nbytes = _lib.scratch("t4d_texture_pad_scratch_bytes", img.device, h, w)
    out, out_cov = torch.empty_like(img), torch.empty_like(cov)
    _lib.call("t4d_texture_pad", ptr(img), ptr(cov), h, w, c, radius, ptr(out), ptr(out_cov), ptr(scratch), nbytes,
              _lib.stream(img.device))
    return out, out_cov


def halve(image: torch.Tensor, coverage: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(image [h/2,w/2(,c)], coverage [h/2,w/2]): per 2x2 block the mean of its covered texels, rounded half up; 0 without any."""
    img, cov, h, w, c = _image_and_coverage(image, coverage)
    if h % 2 or w % 2:
        raise ValueError(f"halve: h and w must be even, got {h} x {w}")
    out = torch.empty((h // 2, w // 2) + tuple(img.shape[2:]), dtype=torch.uint8, device=img.device)
    out_cov = torch.empty(h // 2, w // 2, dtype=torch.uint8, device=img.device)
    _lib.call("t4d_texture_halve", ptr(img), ptr(cov), h, w, c, ptr(out), ptr(out_cov), _lib.stream(img.device))
    return out, out_cov


def _fill(image, valid, domain, dtype, entry: str) -> Tuple[torch.Tensor, torch.Tensor]:
    h, w, c = _args.image(image, "image", (dtype,), _NOTE[dtype])  # argument errors first, with or without a device
    _args.mask(valid, "valid", h, w)
    if domain is not None:
        _args.mask(domain, "domain", h, w)
    img = on_device(image, "image")
    val = on_device(valid, "valid", img.device, "the image's")
    dom = None if domain is None else on_device(domain, "domain", img.device, "the image's")
    scratch, nbytes = _lib.scratch(entry + "_scratch_bytes", img.device, h, w, c)
    out = torch.empty_like(img)
    filled = torch.empty(h, w, dtype=torch.uint8, device=img.device)
    _lib.call(entry, ptr(img), ptr(val), ptr(dom), h, w, c, ptr(out), ptr(filled), ptr(scratch), nbytes, _lib.stream(img.device))
    return out, filled


def fill(image: torch.Tensor, valid: torch.Tensor, domain: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(image, filled uint8 [h,w]): every texel of `domain` (None: every texel) that is not `valid` takes the push-pull
    interpolation of the valid texels (include/topo4d_raster.h states the rule, tests/texfill_ref.py restates it); every other
    texel is copied through.  filled is 1 at the texels written.  Without any valid texel the image comes back as it is."""
    return _fill(image, valid, domain, torch.uint8, "t4d_texture_fill")


def fill16(image_i32: torch.Tensor, valid: torch.Tensor, domain: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fill for an int32 image of 16-bit samples (0..65535; the low 16 bits of every word count), over t4d_texture_fill16: the
    same rule in units of 1/256 of a 16-bit step (tests/dispmap_ref.py restates it)."""
    return _fill(image_i32, valid, domain, torch.int32, "t4d_texture_fill16")


def fill_islands(image: torch.Tensor, valid: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(image, filled): fill per UV island.  labels uint8 [h,w] (projtex.island_labels; 0: no island).  For every label i that holds
    both a valid texel and a texel to fill, fill(image, valid & (labels == i), labels == i), and the filled texels are merged: an
    island's colours never enter another island's holes, and an island without any valid texel stays as it is.  Every pass runs on
    the whole image (a crop would shift the pyramid and change the bits).  The labels that need a pass are found by one read of
    two flags per label from the device."""
    return _fill_islands(image, valid, labels, torch.uint8, fill)


def fill16_islands(image_i32: torch.Tensor, valid: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fill_islands for an int32 image of 16-bit samples: exactly its per-island rule, with fill16 for every pass."""
    return _fill_islands(image_i32, valid, labels, torch.int32, fill16)


def _fill_islands(image, valid, labels, dtype, fill) -> Tuple[torch.Tensor, torch.Tensor]:
    h, w, _ = _args.image(image, "image", (dtype,), _NOTE[dtype])
    _args.mask(valid, "valid", h, w)
    _args.mask(labels, "labels", h, w, (torch.uint8,))
    img = on_device(image, "image")
    val = on_device(valid, "valid", img.device, "the image's") != 0
    lab = on_device(labels, "labels", img.device, "the image's")
    flat = lab.reshape(-1).to(torch.int64)
    flags = torch.stack([torch.bincount(flat, weights=val.reshape(-1).to(torch.float64), minlength=256),
                         torch.bincount(flat, weights=(~val).reshape(-1).to(torch.float64), minlength=256)]).cpu().numpy()
    out, filled = img.clone(), torch.zeros(h, w, dtype=torch.uint8, device=img.device)
    for i in range(1, 256):
        if not (flags[0, i] > 0 and flags[1, i] > 0):
            continue
        island = lab == i
        o, f = fill(img, val & island, island)
        out = torch.where((f != 0).reshape((h, w) + (1,) * (img.dim() - 2)), o, out)
        filled |= f
    return out, filled


_pad, _erode = pad, erode                                     # finish's keyword arguments carry the same names


def _levels(res: int, w: int, sizes: Sequence[int]) -> Dict[int, int]:
    """{size: k} with size = res / 2^k for every entry of `sizes`; ValueError for anything else."""
    out = {}
    for s in sizes:
        s = int(s)
        k = 0
        while s > 0 and (s << k) < res:
            k += 1
        if s < 1 or (s << k) != res or res % (1 << k) or w % (1 << k):
            raise ValueError(f"finish: size {s} is not {res} / 2^k (with {res} x {w} divisible by 2^k)")
        out[s] = k
    return out


def check_options(pad: int, erode: int, sizes: Sequence[int], res: int) -> None:
    """ValueError for a radius, a round count or a size that finish would refuse (callable without a device)."""
    if not 0 <= int(pad) <= MAX_PAD:
        raise ValueError(f"pad must be in [0, {MAX_PAD}], got {pad}")
    if not 0 <= int(erode) <= MAX_ERODE:
        raise ValueError(f"erode must be in [0, {MAX_ERODE}], got {erode}")
    _levels(int(res), int(res), sizes)


def finish(image_u8: torch.Tensor, coverage: torch.Tensor, pad: int = 0, erode: int = 0, sizes: Sequence[int] = ()) -> Dict[int, torch.Tensor]:
    """{res: image} for res = the image's height and every entry of `sizes` (each res / 2^k).  The coverage is eroded `erode`
    rounds once; level 0 is the image padded by `pad` under that coverage; every further level halves the UNPADDED image and the
    eroded coverage repeatedly and is then padded by the same `pad`, in its own texels."""
    h, w, _ = _args.image(image_u8, "image")                   # argument errors first, with or without a device
    levels = _levels(h, w, sizes)
    pad_r, rounds = int(pad), int(erode)
    if not 0 <= pad_r <= MAX_PAD or not 0 <= rounds <= MAX_ERODE:
        raise ValueError(f"finish: pad must be in [0, {MAX_PAD}] and erode in [0, {MAX_ERODE}], got {pad_r}, {rounds}")
    img, cov = _image_and_coverage(image_u8, coverage)[:2]
    cov0 = _erode(cov, rounds)
    out = {}
    cur, cur_cov = img, cov0
    for k in range(max(levels.values(), default=0) + 1):
        if k:
            cur, cur_cov = halve(cur, cur_cov)
        size = h >> k
        if k == 0 or size in levels:
            out[size] = _pad(cur, cur_cov, pad_r)[0] if pad_r else cur
    return out


def coverage_from_obj(face_obj, h: int, w: int, device="cuda") -> torch.Tensor:
    """The coverage of an [h,w] texture baked for `face_obj` (meshrender.read_face_obj): its triangulated UV faces rasterised by
    the bake itself.  A bake of the dense mesh covers the same islands to about a texel at their borders."""
    from . import meshrender, texture
    _, uv_tris = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
    verts = texture.process_uv(face_obj.uvs, h, w)
    zeros = torch.zeros(len(face_obj.uvs), 3, dtype=torch.float32, device=device)
    _, depth = texture.render_colors(verts, uv_tris, zeros, h, w, device=device, return_depth=True)
    return coverage_from_depth(depth)


def level_path(path, size: int) -> str:
    """face.png -> face_<size>.png: the file of a smaller level beside `path`."""
    root, ext = os.path.splitext(os.fspath(path))
    return f"{root}_{int(size)}{ext}"


def write_levels(path, levels: Dict[int, torch.Tensor]) -> list:
    """finish's levels as PNG files through png.write_png: the largest at `path`, the others at level_path(path, size)."""
    from .png import write_png
    top = max(levels)
    written = []
    for size in sorted(levels, reverse=True):
        p = os.fspath(path) if size == top else level_path(path, size)
        write_png(p, levels[size])
        written.append(p)
    return written


# ---- command line ----------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.texfinish",
                                description="Pad the UV islands of every frame's face.png and write smaller levels.")
    _run.add_run_flags(p, "exp", "seq", "output_dir", frames_help="Frames to finish: '1-10', '1,5,9' (default: every frame directory).")
    p.add_argument("--pad", type=int, required=True, metavar="R", help=f"Gutter radius in texels, 0..{MAX_PAD}.")
    p.add_argument("--erode", type=int, default=1, metavar="E",
                   help=f"Rounds of erosion of the face.obj coverage before padding, 0..{MAX_ERODE} (default 1).")
    p.add_argument("--sizes", type=_run.size_list, default=[], help="Smaller levels to write too, comma-separated: res / 2^k each.")
    p.add_argument("--in_place", action="store_true", help="Overwrite face.png (and write face_<res>.png) instead of face_pad*.png.")
    return p


def finish_tree(args, device=None) -> list:
    """The files written for the run <od>/<exp>/<seq>; frames without face.obj or face.png are left alone."""
    dev = torch.device(device if device is not None else "cuda")
    run_dir = _run.run_dir_of(args)
    written = []
    with torch.cuda.device(dev):
        for t in _run.frames_of(args, run_dir):
            frame_dir = _run.frame_dir(run_dir, t)
            obj, tex = _run.read_textured_frame(frame_dir, "face.png")
            if obj is None or tex is None:
                continue
            png_path = os.path.join(frame_dir, "face.png")
            try:
                check_options(args.pad, args.erode, args.sizes, tex.shape[0])
            except ValueError as e:
                raise SystemExit(f"{png_path}: {e}") from None
            image = torch.from_numpy(tex).to(dev)
            cov = coverage_from_obj(obj, tex.shape[0], tex.shape[1], device=dev)
            levels = finish(image, cov, pad=args.pad, erode=args.erode, sizes=args.sizes)
            written += write_levels(png_path if args.in_place else os.path.join(frame_dir, "face_pad.png"), levels)
    return written


def main(argv=None) -> None:
    _run.print_written(finish_tree(build_parser().parse_args(argv)))


if __name__ == "__main__":
    main()
