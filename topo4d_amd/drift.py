"""
Tracking drift between two frames, measured by matching their UV textures on the GPU (csrc/t4d_drift.hip).

    luma(image)                                               uint8 [h,w]: (77 R + 150 G + 29 B + 128) >> 8
    match(image_a, valid_a, image_b, valid_b, labels, ...)    -> int32 [nby,nbx,16]: per block the best displacement and its costs
    flow(table, radius, ratio)                                -> (d float64 [nby,nbx,2], kept bool [nby,nbx]): sub-texel (dy, dx)
    metric(d, kept, pos, labels, block, stride)               -> (drift float64 [nby,nbx] in surface units, kept)
    drift_stats(texels, units, kept, unit)                    blocks, kept, kept_fraction and mean, median, p90, max
    frame_pair(obj_a, tex_a, valid_a, tex_b, valid_b, level)  the steps above for two frames' textures
    dense_flow(d, kept, labels, block, stride, level, reach)  -> (flow int32 [H,W,2] in 1/256 texel, support uint8 [H,W])
    warp(image, valid, labels, flow)                          -> (image, valid): frame b's texture on frame a's texels
    correct_vertices(face_obj, vertices, flow, support, labels)  -> (vertices float64 [N,3], moved bool [N])
    stabilise_pair(obj_a, tex_a, valid_a, obj_b, tex_b, valid_b, ...)  frame_pair and the three above

One topology is tracked through a sequence, so with perfect tracking a pore or a mole stays on the same texel of every frame's
projected texture (projtex: face_proj.png).  The displacement between two frames' textures, taken through the surface's metric, is
therefore how far the mesh slid along the skin: the number that neither the photometric score (each frame's own texture on its own
mesh) nor the scan score (distances along the normal) can see.

match compares census words (7 x 7, 48 bits: which neighbours are darker than the texel), so a change of exposure or shading
between the frames does not matter; a texel takes part only if its whole census window is valid and inside a UV island, and a pair
only if both texels carry one island label.  include/topo4d_raster.h states the rule and the layout of the table exactly; it is
integer arithmetic, and tests/drift_ref.py restates it, flow and metric in numpy bit for bit.

flow keeps a block when it has a best and a second candidate, the second's c > 0 (a flat block, whose costs are all zero, is
never kept), q_best <= ratio q_second with q = c / n (the best stands out), and max(|dy|, |dx|) < radius (a best on the rim of
the search range is a clipped match).  Per axis the sub-texel offset is (q- - q+) / (2 ((q- - 2 q0) + q+)), clamped to +-0.5,
from the costs q-, q+ of the best's two neighbours on that axis; it applies when both are admissible and the denominator is
positive, and is 0 otherwise.  All of it is float64 torch arithmetic in that order.

metric takes the central differences Jx, Jy of surface_maps' pos over +-1 texel at the block's centre texel
(y0 + B/2, x0 + B/2), in float64: the drift is |Jx dx + Jy dy|, with |v| = sqrt((v0 v0 + v1 v1) + v2 v2).  A block whose five
texels do not share one non-zero label is dropped from kept.

Known limits: an expression that stretches the skin changes the texture itself, not only its place; census tolerates shading
changes but not wrinkles.  A drift beyond `radius` texels at the chosen level is dropped, not measured.  The defaults (block 32,
stride 16, radius 8, ratio 0.8, level 2) are conventional, not tuned on a capture.  There is no CPU path.

Stabilisation uses the measurement (csrc/t4d_stabilise.hip; include/topo4d_raster.h states the rule, tests/stabilise_ref.py restates
it).  Every kept block is a node at its centre in the full-resolution texture, holding d in 1/256 texel.  dense_flow gives every
texel of an island the mean of the nodes of that island within `reach` block spacings, weighted by the product of two tents (reach
1: bilinear between the four nodes round the texel, renormalised over those that take part); warp resamples frame b's texture at
x + f(x) with four taps in 1/256 texel, restricted to the texel's island and to valid texels, so a pore sits on the texel it has in
frame a.  Both are integer arithmetic and equal the restatement bit for bit.  To first order the stabilised texture is the texture
of the corrected mesh: correct_vertices moves every vertex of frame b along frame b's own surface (surface_maps at full
resolution, sampled in float64 in a fixed order) to the point at p + f.  Matching frame a against the stabilised texture measures
what the correction left behind.  Known limits: a texel without support is copied, which may leave a tear at the rim of the
support; where x + f leaves the island the stabilised texture is not valid, so after a large shift the blocks on that rim can
fall below min_count; a border vertex whose nearest texel is outside the coverage is not moved; drift beyond `radius` is never
measured and therefore never corrected; the correction is one step, not iterated, and flows against the previous frame are not
composed (--stabilise needs --ref first); reach 1 is conventional, not tuned on a capture.

`python -m topo4d_amd.drift -e EXP -s SEQ -od DIR [--frames 1-10] [--texture face_proj.png] [--ref first|previous] [--level 2]
[--block 32] [--stride S] [--radius 8] [--ratio 0.8] [--unit 1000] [--save_fields] [--stabilise [--reach 1] [--correct_obj]]`
works over an output tree that exists (the reference's too) and writes <od>/<exp>/<seq>/drift.json: the options, per frame the pair and its statistics, and a summary.  A
frame's validity is face_proj_weight.png > 0 where that file exists and texfinish.coverage_from_obj of its face.obj otherwise
("valid_from").  --ref first measures the drift accumulated since the first selected frame, --ref previous the slip from frame to
frame; --save_fields also writes %06d/face_drift.npz (table, d, kept, drift).  `evaluate --drift` puts the same dictionary under
"drift" in eval.json.  --stabilise (this command only, with --ref first) also writes per measured frame %06d/<texture>_stab.png
and <texture>_stab_weight.png (the warp's validity) through the GPU PNG encoder and, with --correct_obj, %06d/face_stab.obj; the
frame's row gains "stabilised" (drift_stats of reference against stabilised texture, "support_fraction" over labelled texels,
"moved_vertices"), "options" gains "stabilise" and "reach", and --save_fields adds flow and support to face_drift.npz.  Without
--stabilise every file and every key is what it was.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Tuple

import numpy as np
import torch

from . import _args, _lib, _run
from ._lib import on_device, ptr

MIN_BLOCK, MAX_BLOCK, MAX_RADIUS = 8, 64, 16
MAX_LEVEL, MAX_REACH, MAX_NODE, MAX_TENT = 8, 4, 1 << 22, 46340
TABLE_WIDTH = 16
TEXTURE_FILE = "face_proj.png"
WEIGHT_FILE = "face_proj_weight.png"
FIELDS_NAME = "face_drift.npz"
STAB_OBJ = "face_stab.obj"
DEFAULTS = dict(texture=TEXTURE_FILE, ref="first", level=2, block=32, stride=None, radius=8, ratio=0.8, unit=1000.0)


def check_options(block=32, stride=None, radius=8, min_count=None) -> Tuple[int, int, int, int]:
    """(block, stride, radius, min_count) with the defaults filled in (stride = block // 2, min_count = block^2 // 2); ValueError
    for what t4d_drift_match would refuse (callable without a device)."""
    block, radius = int(block), int(radius)
    if not MIN_BLOCK <= block <= MAX_BLOCK or block % 2:
        raise ValueError(f"block must be even and in [{MIN_BLOCK}, {MAX_BLOCK}], got {block}")
    stride = block // 2 if stride is None else int(stride)
    if not 1 <= stride <= block:
        raise ValueError(f"stride must be in [1, block = {block}], got {stride}")
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be in [0, {MAX_RADIUS}], got {radius}")
    min_count = block * block // 2 if min_count is None else int(min_count)
    if not 1 <= min_count <= block * block:
        raise ValueError(f"min_count must be in [1, block^2 = {block * block}], got {min_count}")
    return block, stride, radius, min_count


def blocks(h: int, w: int, block: int, stride: int) -> Tuple[int, int]:
    """(nby, nbx): the blocks that lie wholly inside an [h,w] image."""
    return ((h - block) // stride + 1 if h >= block else 0), ((w - block) // stride + 1 if w >= block else 0)


def luma(image: torch.Tensor) -> torch.Tensor:
    """uint8 [h,w]: (77 R + 150 G + 29 B + 128) >> 8 of a uint8 [h,w,3] image (RGBA: its first three channels), in integer torch
    ops; a one-channel image is its own luma."""
    h, w = _args.image(image, "image")[:2]
    if image.dim() == 2 or image.shape[2] == 1:
        return image.reshape(h, w).contiguous()
    rgb = image[..., :3].to(torch.int32)
    return ((77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + 128) >> 8).to(torch.uint8).contiguous()


def match(image_a: torch.Tensor, valid_a: torch.Tensor, image_b: torch.Tensor, valid_b: torch.Tensor, labels: torch.Tensor,
          block: int = 32, stride: int = None, radius: int = 8, min_count: int = None) -> torch.Tensor:
    """int32 [nby,nbx,16] on the device: per block of `block`^2 texels of frame a, every `stride` texels, the displacement
    (dy, dx) in [-radius, radius]^2 at which frame b's census words differ least, with the costs flow needs
    (include/topo4d_raster.h states the rule and the table, tests/drift_ref.py restates it).  images uint8 [h,w] or [h,w,c];
    valid_a, valid_b uint8 or bool [h,w], non-zero = the texel holds a photograph; labels uint8 [h,w] (projtex.island_labels;
    0: no island).  A shape without a whole block gives an empty table."""
    h, w = _args.image(image_a, "image_a")[:2]                 # argument errors first, with or without a device
    if _args.image(image_b, "image_b")[:2] != (h, w):
        raise ValueError(f"image_b {tuple(image_b.shape)} does not match image_a's [{h},{w}]")
    _args.mask(valid_a, "valid_a", h, w)
    _args.mask(valid_b, "valid_b", h, w)
    _args.mask(labels, "labels", h, w, dtypes=(torch.uint8,))
    block, stride, radius, min_count = check_options(block, stride, radius, min_count)
    img_a = on_device(image_a, "image_a")
    dev = img_a.device
    img_b, val_a, val_b = on_device(image_b, "image_b", dev), on_device(valid_a, "valid_a", dev), on_device(valid_b, "valid_b", dev)
    lab = on_device(labels, "labels", dev)
    nby, nbx = blocks(h, w, block, stride)
    if nby == 0 or nbx == 0:
        return torch.zeros(nby, nbx, TABLE_WIDTH, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        scratch, nbytes = _lib.scratch("t4d_drift_scratch_bytes", dev, h, w, block, stride, radius)
        la, lb = luma(img_a), luma(img_b)
        out = torch.empty(nby, nbx, TABLE_WIDTH, dtype=torch.int32, device=dev)
        _lib.call("t4d_drift_match", ptr(la), ptr(val_a), ptr(lb), ptr(val_b), ptr(lab), h, w, block, stride, radius, min_count,
                  ptr(out), ptr(scratch), nbytes, _lib.stream(dev))
    return out


def flow(table: torch.Tensor, radius: int, ratio: float = 0.8) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d float64 [nby,nbx,2] = (dy, dx) with its sub-texel offset, kept bool [nby,nbx]) of match's table, by the module's rule:
    float64 torch operations in the order the docstring states."""
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 3 or table.shape[2] != TABLE_WIDTH:
        raise ValueError(f"table must be match's int32 [nby,nbx,{TABLE_WIDTH}] tensor")
    radius, ratio = int(radius), float(ratio)
    if not 0 <= radius <= MAX_RADIUS or not 0.0 < ratio <= 1.0:
        raise ValueError(f"flow: radius must be in [0, {MAX_RADIUS}] and ratio in (0, 1], got {radius}, {ratio}")
    t = table.to(torch.float64)
    one = torch.ones((), dtype=torch.float64, device=table.device)
    q = lambda k: t[..., k] / torch.maximum(t[..., k + 1], one)          # c / n, 0 where there is none
    has = lambda k: table[..., k + 1] > 0
    q0, q2 = q(2), q(12)
    kept = has(2) & has(12) & (table[..., 12] > 0) & (q0 <= ratio * q2)
    kept &= torch.maximum(table[..., 0].abs(), table[..., 1].abs()) < radius
    d = []
    for axis, k in ((0, 4), (1, 8)):
        qm, qp = q(k), q(k + 2)
        den = (qm - 2.0 * q0) + qp
        ok = has(2) & has(k) & has(k + 2) & (den > 0.0)
        off = ((qm - qp) / (2.0 * torch.where(ok, den, one))).clamp(-0.5, 0.5)
        d.append(t[..., axis] + torch.where(ok, off, torch.zeros_like(off)))
    return torch.stack(d, dim=-1), kept


def length(d: torch.Tensor) -> torch.Tensor:
    """float64 [nby,nbx]: sqrt(dy dy + dx dx) of flow's d, the drift in texels."""
    return torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def metric(d: torch.Tensor, kept: torch.Tensor, pos: torch.Tensor, labels: torch.Tensor, block: int, stride: int = None):
    """(drift float64 [nby,nbx], kept bool [nby,nbx]): flow's displacement in the units of pos (projtex.surface_maps' map of the
    same size as the matched textures) by the module's rule; a block whose centre texel and its four neighbours do not share one
    non-zero label is dropped from kept."""
    block, stride, _, _ = check_options(block, stride)
    if not isinstance(pos, torch.Tensor) or pos.dim() != 3 or pos.shape[2] != 3 or not pos.is_floating_point():
        raise ValueError("pos must be a float [h,w,3] tensor")
    h, w = int(pos.shape[0]), int(pos.shape[1])
    _args.mask(labels, "labels", h, w, dtypes=(torch.uint8,))
    nby, nbx = blocks(h, w, block, stride)
    if not isinstance(d, torch.Tensor) or tuple(d.shape) != (nby, nbx, 2) or tuple(kept.shape) != (nby, nbx):
        raise ValueError(f"d and kept must be flow's [{nby},{nbx},2] and [{nby},{nbx}] for this size, block and stride")
    dev = d.device
    cy = (torch.arange(nby, device=dev) * stride + block // 2)[:, None].expand(nby, nbx)
    cx = (torch.arange(nbx, device=dev) * stride + block // 2)[None, :].expand(nby, nbx)
    p = pos.to(torch.float64)
    jx = (p[cy, cx + 1] - p[cy, cx - 1]) * 0.5
    jy = (p[cy + 1, cx] - p[cy - 1, cx]) * 0.5
    v = jx * d[..., 1:2] + jy * d[..., 0:1]
    drift = torch.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    lab = labels[cy, cx]
    same = (lab != 0) & (labels[cy, cx + 1] == lab) & (labels[cy, cx - 1] == lab) & (labels[cy + 1, cx] == lab) & (labels[cy - 1, cx] == lab)
    return drift, kept & same


def drift_stats(texels: torch.Tensor, units: torch.Tensor, kept: torch.Tensor, unit: float = 1.0) -> dict:
    """blocks, kept, kept_fraction and, over the kept blocks, mean, median (the lower one), p90 and max of `units` x unit and, as
    *_texels, of `texels`; a field without a kept block has the first three only (scanbake.displacement_stats' conventions)."""
    m = kept.reshape(-1)
    total, n = int(m.numel()), int(m.sum())
    out = {"blocks": total, "kept": n, "kept_fraction": n / total if total else 0.0}
    if n == 0:
        return out
    for values, suffix in ((units.reshape(-1)[m].to(torch.float64) * unit, ""), (texels.reshape(-1)[m].to(torch.float64), "_texels")):
        srt = torch.sort(values).values
        picks = torch.stack([srt[(n - 1) // 2], srt[min(n - 1, -(-9 * n // 10) - 1)], srt[-1], values.sum()]).cpu().tolist()
        out["mean" + suffix] = picks[3] / n
        out["median" + suffix], out["p90" + suffix], out["max" + suffix] = picks[0], picks[1], picks[2]
    return out


def frame_pair(obj_a, tex_a: torch.Tensor, valid_a: torch.Tensor, tex_b: torch.Tensor, valid_b: torch.Tensor, level: int = 2,
               block: int = 32, stride: int = None, radius: int = 8, min_count: int = None, ratio: float = 0.8, device=None) -> dict:
    """table, d, kept, texels (the drift in texels of the level) and drift (in the units of obj_a's vertices) for two frames'
    textures of one size on the device.  Textures and validities are halved `level` times (texfinish.halve: means over the valid
    texels alone); island_labels and surface_maps of that size come from frame a's face.obj (meshrender.FaceObj)."""
    from . import projtex, texfinish
    level = int(level)
    h, w = _args.image(tex_a, "tex_a")[:2]
    block, stride, radius, min_count = check_options(block, stride, radius, min_count)
    if not 0 <= level <= 8 or h % (1 << level) or w % (1 << level):
        raise ValueError(f"level must be in [0, 8] with {h} x {w} divisible by 2^level, got {level}")
    dev = tex_a.device if device is None else torch.device(device)
    with torch.cuda.device(dev):
        a, va, b, vb = tex_a, valid_a, tex_b, valid_b
        for _ in range(level):
            a, va = texfinish.halve(a, va)
            b, vb = texfinish.halve(b, vb)
        h, w = h >> level, w >> level
        labels = projtex.island_labels(obj_a, h, w, device=dev)
        verts = torch.from_numpy(np.ascontiguousarray(obj_a.vertices, np.float64)).to(dev)
        pos = projtex.surface_maps(obj_a, verts, (h, w), device=dev)[0]
        table = match(a, va, b, vb, labels, block, stride, radius, min_count)
        d, kept = flow(table, radius, ratio)
        drift, kept = metric(d, kept, pos, labels, block, stride)
    return {"table": table, "d": d, "kept": kept, "texels": length(d), "drift": drift}


# ---- stabilisation -----------------------------------------------------------------------------------------------------------
def _level_size(labels, level: int) -> Tuple[int, int, int]:
    """(H, W, level) of a full-resolution label map whose size is divisible by 2^level"""
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 2 or labels.numel() == 0:
        raise ValueError("labels must be a uint8 [H,W] tensor")
    H, W, level = int(labels.shape[0]), int(labels.shape[1]), int(level)
    if not 0 <= level <= MAX_LEVEL or H % (1 << level) or W % (1 << level):
        raise ValueError(f"level must be in [0, {MAX_LEVEL}] with {H} x {W} divisible by 2^level, got {level}")
    return H, W, level


def check_reach(reach=1, stride: int = None, level: int = None) -> int:
    """reach as an int; ValueError outside 1..4 and, given stride and level, for a tent of reach 2 stride 2^level > 46340 doubled
    texels, which t4d_drift_dense refuses (its weights are 32-bit products)."""
    reach = int(reach)
    if not 1 <= reach <= MAX_REACH:
        raise ValueError(f"reach must be in [1, {MAX_REACH}], got {reach}")
    if stride is not None and reach * 2 * int(stride) * (1 << int(level)) > MAX_TENT:
        raise ValueError(f"reach 2 stride 2^level must be at most {MAX_TENT}, got reach {reach}, stride {stride}, level {level}")
    return reach


def node_values(d: torch.Tensor, level: int, check: bool = True) -> torch.Tensor:
    """int32 [nby,nbx,2]: q = rint(d 2^level 256), flow's displacement in 1/256 of a full-resolution texel; with check, ValueError
    for a d that is not finite or beyond t4d_drift_dense's |q| <= 2^22 (the test reads the tensor back: a host synchronisation)."""
    q = torch.round(d * float((1 << int(level)) * 256))
    if check and q.numel() and not bool((torch.isfinite(q) & (q.abs() <= float(MAX_NODE))).all()):
        raise ValueError(f"d must be finite with |d| 2^level 256 <= {MAX_NODE}")
    return q.to(torch.int32).contiguous()


def dense_flow(d: torch.Tensor, kept: torch.Tensor, labels: torch.Tensor, block: int, stride: int = None, level: int = 0,
               reach: int = 1, check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(flow int32 [H,W,2] = (f_y, f_x) in 1/256 of a texel, support uint8 [H,W]) on the device: flow's / metric's d and kept of
    the blocks at `level`, spread over every texel of the full-resolution island map `labels` by the rule of t4d_drift_dense
    (include/topo4d_raster.h; tests/stabilise_ref.py restates it).  A texel of frame a's texture at x shows what frame b's shows at
    x + f / 256.  A shape without a block gives an all-zero flow and support.  check: node_values' test that d is finite and
    within |q| <= 2^22 reads d back, which waits for the device; a caller whose d is flow's own (|d| <= radius + 0.5, always within
    the bound) passes check=False and the call stays asynchronous."""
    H, W, level = _level_size(labels, level)                   # argument errors first, with or without a device
    block, stride, _, _ = check_options(block, stride)
    reach = check_reach(reach, stride, level)
    nby, nbx = blocks(H >> level, W >> level, block, stride)
    if not isinstance(d, torch.Tensor) or d.dtype != torch.float64 or tuple(d.shape) != (nby, nbx, 2):
        raise ValueError(f"d must be flow's float64 [{nby},{nbx},2] for this size, level, block and stride")
    _args.mask(kept, "kept", nby, nbx)
    q = node_values(d, level, check)
    lab = on_device(labels, "labels")
    dev = lab.device
    q, keep = on_device(q, "d", dev), on_device(kept, "kept", dev)
    with torch.cuda.device(dev):
        out = torch.empty(H, W, 2, dtype=torch.int32, device=dev)
        support = torch.empty(H, W, dtype=torch.uint8, device=dev)
        _lib.call("t4d_drift_dense", ptr(q), ptr(keep), ptr(lab), H, W, block, stride, level, reach, ptr(out), ptr(support),
                  _lib.stream(dev))
    return out, support


def _flow_field(flow, h: int, w: int) -> None:
    if not isinstance(flow, torch.Tensor) or flow.dtype != torch.int32 or tuple(flow.shape) != (h, w, 2):
        raise ValueError(f"flow must be dense_flow's int32 [{h},{w},2] tensor, got {getattr(flow, 'dtype', type(flow))} "
                         f"{list(getattr(flow, 'shape', ()))}")


def warp(image: torch.Tensor, valid: torch.Tensor, labels: torch.Tensor, flow: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(image uint8 of the given shape, valid uint8 [H,W]) on the device: frame b's texture resampled through dense_flow's field
    by the rule of t4d_drift_warp (four taps in 1/256 texel, restricted to the texel's island and to valid texels), so that a
    feature sits on the texel it has in frame a.  The inputs are left as they are."""
    h, w, c = _args.image(image, "image")                      # argument errors first, with or without a device
    _args.mask(valid, "valid", h, w)
    _args.mask(labels, "labels", h, w, dtypes=(torch.uint8,))
    _flow_field(flow, h, w)
    img = on_device(image, "image")
    dev = img.device
    val, lab, fl = on_device(valid, "valid", dev), on_device(labels, "labels", dev), on_device(flow, "flow", dev)
    with torch.cuda.device(dev):
        out, out_valid = torch.empty_like(img), torch.empty(h, w, dtype=torch.uint8, device=dev)
        _lib.call("t4d_drift_warp", ptr(img), ptr(val), ptr(lab), ptr(fl), h, w, c, ptr(out), ptr(out_valid), _lib.stream(dev))
    return out, out_valid


def sample_positions(pos: torch.Tensor, labels: torch.Tensor, py: torch.Tensor, px: torch.Tensor, label: torch.Tensor):
    """(values float64 [n,3], ok bool [n]): pos (float [H,W,3]) at the float64 texel positions (py, px), by the warp's four taps
    restricted to the island `label` [n], in float64: y0 = floor(py), t = py - y0 and likewise in x; the taps weigh (1 - ty)(1 - tx),
    (1 - ty) tx, ty (1 - tx), ty tx, and 0 where the tap is outside the map, its label differs or label is 0; Wt = ((w00 + w01) +
    w10) + w11, the value is (((w00 v00 + w01 v01) + w10 v10) + w11 v11) / Wt and ok = Wt > 0 (the value is 0 where it is not)."""
    H, W = int(labels.shape[0]), int(labels.shape[1])
    y0, x0 = torch.floor(py), torch.floor(px)
    ty, tx = py - y0, px - x0
    y0, x0 = y0.to(torch.int64), x0.to(torch.int64)
    weights, values = [], []
    for a, wy in ((0, 1.0 - ty), (1, ty)):
        for b, wx in ((0, 1.0 - tx), (1, tx)):
            yy, xx = y0 + a, x0 + b
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            yc, xc = yy.clamp(0, H - 1), xx.clamp(0, W - 1)
            ok = inside & (labels[yc, xc] == label) & (label != 0)
            weights.append(torch.where(ok, wy * wx, torch.zeros_like(wy)))
            values.append(pos[yc, xc].to(torch.float64))
    total = ((weights[0] + weights[1]) + weights[2]) + weights[3]
    s = ((weights[0][:, None] * values[0] + weights[1][:, None] * values[1]) + weights[2][:, None] * values[2]) + weights[3][:, None] * values[3]
    ok = total > 0.0
    return torch.where(ok[:, None], s / torch.where(ok, total, torch.ones_like(total))[:, None], torch.zeros_like(s)), ok


def correct_vertices(face_obj, vertices, flow: torch.Tensor, support: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(vertices float64 [N,3], moved bool [N]) on the device: every mesh vertex of frame b (face_obj: meshrender.FaceObj,
    vertices [N,3]) moved along frame b's own surface to the point that shows what the vertex showed in frame a.  A UV vertex at
    the texel position p (texture.process_uv at the size of `labels`) takes the flow f of the texel rint(p); it is skipped when
    that texel lies outside the map or has support 0.  projtex.surface_maps' position map of the mesh at full resolution is
    sampled at p + f / 256 by sample_positions with the texel's label, and skipped when no tap is admissible.  A mesh vertex
    (projtex.uv_vertex_owner: the one surface_maps puts at the UV vertex) becomes the mean of the samples of its UV vertices that
    were not skipped, summed in ascending UV index; one whose UV vertices were all skipped stays where it is.  Float64 torch
    operations in that order."""
    from . import meshrender, projtex, texture
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.uint8 or labels.dim() != 2:
        raise ValueError("labels must be a uint8 [H,W] tensor")
    H, W = int(labels.shape[0]), int(labels.shape[1])
    _flow_field(flow, H, W)
    _args.mask(support, "support", H, W)
    verts = torch.as_tensor(vertices) if isinstance(vertices, np.ndarray) else vertices
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3 or not verts.is_floating_point():
        raise ValueError("vertices must be a float [N,3] tensor or array")
    n_vert = int(verts.shape[0])
    faces, uv_faces = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
    if faces.size and (faces.min() < 0 or faces.max() >= n_vert):
        raise ValueError(f"faces name vertex {int(faces.max())} but only {n_vert} vertices were given")
    lab = on_device(labels, "labels")
    dev = lab.device
    fl, sup = on_device(flow, "flow", dev), on_device(support, "support", dev)
    owner = projtex.uv_vertex_owner(faces, uv_faces, len(face_obj.uvs))
    used = np.nonzero(owner >= 0)[0]                            # ascending UV index
    own = owner[used]
    order = np.argsort(own, kind="stable")
    rank = np.empty(len(used), np.int64)                        # the place of a UV vertex among those of its mesh vertex
    starts = np.concatenate([[0], np.nonzero(np.diff(own[order]))[0] + 1]) if len(used) else np.zeros(0, np.int64)
    rank[order] = np.arange(len(used)) - np.repeat(starts, np.diff(np.concatenate([starts, [len(used)]])))
    p = texture.process_uv(face_obj.uvs, H, W)[used]
    with torch.cuda.device(dev):
        verts = verts.to(device=dev, dtype=torch.float64)
        pos = projtex.surface_maps(face_obj, verts, (H, W), device=dev)[0]
        py, px = torch.from_numpy(np.ascontiguousarray(p[:, 1])).to(dev), torch.from_numpy(np.ascontiguousarray(p[:, 0])).to(dev)
        ry, rx = torch.round(py).to(torch.int64), torch.round(px).to(torch.int64)
        inside = (ry >= 0) & (ry < H) & (rx >= 0) & (rx < W)
        ryc, rxc = ry.clamp(0, H - 1), rx.clamp(0, W - 1)
        f = fl[ryc, rxc].to(torch.float64)
        value, ok = sample_positions(pos, lab, py + f[:, 0] / 256.0, px + f[:, 1] / 256.0, lab[ryc, rxc])
        ok &= inside & (sup[ryc, rxc] != 0)
        own_t, rank_t = torch.from_numpy(own).to(dev), torch.from_numpy(rank).to(dev)
        total = torch.zeros(n_vert, 3, dtype=torch.float64, device=dev)
        count = torch.zeros(n_vert, dtype=torch.float64, device=dev)
        for k in range(int(rank.max()) + 1 if len(used) else 0):   # one UV vertex per mesh vertex and pass: a fixed order of additions
            sel = (rank_t == k) & ok
            total[own_t[sel]] += value[sel]
            count[own_t[sel]] += 1.0
        moved = count > 0.0
        out = torch.where(moved[:, None], total / torch.where(moved, count, torch.ones_like(count))[:, None], verts)
    return out, moved


def stabilise_pair(obj_a, tex_a: torch.Tensor, valid_a: torch.Tensor, obj_b, tex_b: torch.Tensor, valid_b: torch.Tensor, level: int = 2,
                   block: int = 32, stride: int = None, radius: int = 8, min_count: int = None, ratio: float = 0.8, reach: int = 1,
                   vertices_b=None, device=None) -> dict:
    """frame_pair's dictionary for the two frames, and with it labels (frame a's full-resolution island map), flow and support
    (dense_flow of d and kept), image and valid (frame b's texture through warp) and vertices and moved (correct_vertices of
    obj_b, with vertices_b or obj_b's own vertices).  One step: the residual is what a second frame_pair of tex_a against the
    stabilised image measures."""
    from . import projtex
    reach = check_reach(reach)
    h, w = _args.image(tex_a, "tex_a")[:2]
    if _args.image(tex_b, "tex_b")[:2] != (h, w):
        raise ValueError(f"tex_b {tuple(tex_b.shape)} does not match tex_a's [{h},{w}]")
    _args.mask(valid_b, "valid_b", h, w)
    r = frame_pair(obj_a, tex_a, valid_a, tex_b, valid_b, level, block, stride, radius, min_count, ratio, device=device)
    dev = r["table"].device
    block, stride, _, _ = check_options(block, stride, radius, min_count)
    with torch.cuda.device(dev):
        labels = projtex.island_labels(obj_a, h, w, device=dev)
        r["labels"] = labels
        r["flow"], r["support"] = dense_flow(r["d"], r["kept"], labels, block, stride, level, reach, check=False)   # flow's own d
        r["image"], r["valid"] = warp(tex_b, valid_b, labels, r["flow"])
        verts = obj_b.vertices if vertices_b is None else vertices_b
        r["vertices"], r["moved"] = correct_vertices(obj_b, verts, r["flow"], r["support"], labels)
    return r


# ---- command line ----------------------------------------------------------------------------------------------------------
def add_options(p: argparse.ArgumentParser, prefix: str = "") -> None:
    """The matcher's flags, as `python -m topo4d_amd.drift` has them (prefix "": --level ...) and evaluate (prefix "drift_")."""
    flag = lambda name: f"--{prefix}{name}"
    p.add_argument(flag("texture"), default=DEFAULTS["texture"], metavar="NAME",
                   help="Drift: the file of every frame directory that is matched (default face_proj.png).")
    p.add_argument(flag("ref"), choices=("first", "previous"), default=DEFAULTS["ref"],
                   help="Drift: match every frame against the first selected frame (accumulated drift) or the one before (slip).")
    p.add_argument(flag("level"), type=int, default=DEFAULTS["level"], metavar="K", help="Drift: halve the textures K times first (default 2).")
    p.add_argument(flag("block"), type=int, default=DEFAULTS["block"], metavar="B", help="Drift: block side in texels, even, 8..64 (default 32).")
    p.add_argument(flag("stride"), type=int, default=DEFAULTS["stride"], metavar="S", help="Drift: block spacing, 1..B (default B / 2).")
    p.add_argument(flag("radius"), type=int, default=DEFAULTS["radius"], metavar="R", help="Drift: search radius in texels, 0..16 (default 8).")
    p.add_argument(flag("ratio"), type=float, default=DEFAULTS["ratio"],
                   help="Drift: keep a block whose best cost is at most this fraction of its second's (default 0.8).")
    p.add_argument(flag("unit"), type=float, default=DEFAULTS["unit"],
                   help="Drift: reported unit per face.obj unit (default 1000: metres -> mm).")


def options_of(args, prefix: str = "") -> dict:
    return {k: getattr(args, prefix + k, v) for k, v in DEFAULTS.items()}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.drift",
                                description="Measure tracking drift between the frames of a run by matching their UV textures.")
    _run.add_run_flags(p, "exp", "seq", "output_dir", frames_help="Frames to measure: '1-10', '1,5,9' (default: every frame directory).",
                       png_decoder=True)
    add_options(p)
    p.add_argument("--save_fields", action="store_true", help=f"Also write %%06d/{FIELDS_NAME} (table, d, kept, drift).")
    p.add_argument("--stabilise", action="store_true",
                   help="Also resample every measured frame's texture onto the reference frame's texels (%%06d/<texture>_stab.png and "
                        "_stab_weight.png) and report the residual drift; needs --ref first.")
    p.add_argument("--reach", type=int, default=1, metavar="K",
                   help="Stabilise: a texel's flow comes from the nodes within K block spacings, 1..4 (default 1: bilinear).")
    p.add_argument("--correct_obj", action="store_true", help=f"Stabilise: also write %%06d/{STAB_OBJ}, the frame's mesh with its vertices corrected.")
    return p


def stab_names(texture: str) -> Tuple[str, str]:
    """the stabilised texture's and its validity's file names: face_proj.png -> face_proj_stab.png, face_proj_stab_weight.png"""
    stem, ext = os.path.splitext(texture)
    return f"{stem}_stab{ext}", f"{stem}_stab_weight{ext}"


def _stabilise_frame(args, o: dict, frame_dir: str, ref, cur, r: dict, options: tuple, dev) -> Tuple[dict, dict]:
    """what --stabilise adds for one measured frame: its files, and (the "stabilised" entry of its row, the fields --save_fields adds)"""
    from . import objexport, png, projtex
    (obj_a, tex_a, val_a, _), (obj_b, tex_b, val_b, _) = ref, cur
    block, stride, radius, min_count = options
    h, w = int(tex_b.shape[0]), int(tex_b.shape[1])
    labels = projtex.island_labels(obj_a, h, w, device=dev)
    flow_, support = dense_flow(r["d"], r["kept"], labels, block, stride, o["level"], o["reach"], check=False)      # flow's own d
    image, valid = warp(tex_b, val_b, labels, flow_)
    vertices, moved = correct_vertices(obj_b, obj_b.vertices, flow_, support, labels)
    res = frame_pair(obj_a, tex_a, val_a, image, valid, o["level"], block, stride, radius, min_count, o["ratio"], device=dev)
    name, weight_name = stab_names(o["texture"])
    png.write_png(os.path.join(frame_dir, name), image)
    png.write_png(os.path.join(frame_dir, weight_name), valid * 255)
    if getattr(args, "correct_obj", False):
        objexport.write_obj_with_uv(os.path.join(frame_dir, STAB_OBJ), vertices, obj_b.faces_ori, obj_b.uvs, obj_b.uv_faces_ori)
    labelled = int((labels != 0).sum())
    entry = drift_stats(res["texels"], res["drift"], res["kept"], unit=float(o["unit"]))
    entry["support_fraction"] = int((support != 0).sum()) / labelled if labelled else 0.0
    entry["moved_vertices"] = int(moved.sum())
    return entry, {"flow": flow_, "support": support}


def read_frame(frame_dir: str, texture: str, dev, decode_on=None):
    """(FaceObj, texture uint8 [h,w,3], valid uint8 [h,w], "weight" | "obj") of one frame directory, the arrays on the device;
    None without its files.  valid: where the directory's weight image is above 0, else the coverage of its face.obj.
    decode_on: the device that decodes the PNGs (_run.reader_device), None: PIL on the host."""
    from . import texfinish
    obj, tex = _run.read_textured_frame(frame_dir, texture, decode_on)
    if obj is None or tex is None:
        return None
    h, w = int(tex.shape[0]), int(tex.shape[1])
    on_dev = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(dev)
    weight_path = os.path.join(frame_dir, WEIGHT_FILE)
    if os.path.exists(weight_path):
        valid = _run.read_validity(weight_path, (h, w), texture, decode_on)
        return obj, on_dev(tex), on_dev(valid), "weight"
    return obj, on_dev(tex), texfinish.coverage_from_obj(obj, h, w, device=dev), "obj"


def tree_options(args, options: dict = None) -> Tuple[dict, Tuple[int, int, int, int]]:
    """(the "options" of drift.json, (block, stride, radius, min_count)) of a run, checked without a device; SystemExit for what
    cannot run.  options: options_of(args) by default.  "stabilise" and "reach" are there only with --stabilise, so that without
    the flag drift.json is what it was before the flag existed."""
    o = dict(options if options is not None else options_of(args))
    try:
        block, stride, radius, min_count = check_options(o["block"], o["stride"], o["radius"])
        if not 0.0 < float(o["ratio"]) <= 1.0 or not 0 <= int(o["level"]) <= 8:
            raise ValueError(f"ratio must be in (0, 1] and level in [0, 8], got {o['ratio']}, {o['level']}")
    except ValueError as e:
        raise SystemExit(f"drift: {e}") from None
    o["stride"] = stride
    reach = o.pop("reach", getattr(args, "reach", 1))         # read with --stabilise alone: without it the flag says nothing
    if o.pop("stabilise", getattr(args, "stabilise", False)):
        if o["ref"] != "first":
            raise SystemExit("drift: --stabilise needs --ref first (flows against the previous frame would have to be composed)")
        try:
            o["stabilise"], o["reach"] = True, check_reach(reach, stride, o["level"])
        except ValueError as e:
            raise SystemExit(f"drift: {e}") from None
    return {**o, "min_count": min_count}, (block, stride, radius, min_count)


def drift_tree(args, device=None, options: dict = None) -> dict:
    """The dictionary of drift.json for the run <od>/<exp>/<seq>: the options, per measured frame its pair and drift_stats (with
    --stabilise also "stabilised": the residual's drift_stats, support_fraction and moved_vertices), and a summary.  options:
    options_of(args) by default.  Frames without face.obj or the texture are left out."""
    o, (block, stride, radius, min_count) = tree_options(args, options)
    stabilise = "stabilise" in o
    dev = torch.device(device if device is not None else "cuda")
    run_dir = _run.run_dir_of(args)
    out = {"options": o, "frames": {}}
    ref = None                                                # (key, files) of the frame matched against
    with torch.cuda.device(dev):
        for t in _run.frames_of(args, run_dir):
            key = _run.frame_key(t)
            cur = read_frame(os.path.join(run_dir, key), o["texture"], dev, _run.reader_device(args, dev))
            if cur is None:
                continue
            if ref is not None:
                (ref_key, (obj_a, tex_a, val_a, from_a)), (_, tex_b, val_b, from_b) = ref, cur
                if tex_a.shape != tex_b.shape:
                    raise SystemExit(f"{key}/{o['texture']}: {tuple(tex_b.shape)} does not match frame {ref_key}'s {tuple(tex_a.shape)}")
                try:
                    r = frame_pair(obj_a, tex_a, val_a, tex_b, val_b, o["level"], block, stride, radius, min_count, o["ratio"], device=dev)
                except ValueError as e:
                    raise SystemExit(f"{key}/{o['texture']}: {e}") from None
                row = {"pair": [ref_key, key], "valid_from": {ref_key: from_a, key: from_b}}
                row.update(drift_stats(r["texels"], r["drift"], r["kept"], unit=float(o["unit"])))
                out["frames"][key] = row
                fields = {k: r[k] for k in ("table", "d", "kept", "drift")}
                if stabilise:
                    try:
                        row["stabilised"], more = _stabilise_frame(args, o, os.path.join(run_dir, key), ref[1], cur, r,
                                                                   (block, stride, radius, min_count), dev)
                    except ValueError as e:
                        raise SystemExit(f"{key}/{o['texture']}: {e}") from None
                    fields.update(more)
                if getattr(args, "save_fields", False):
                    np.savez(os.path.join(run_dir, key, FIELDS_NAME), **{k: v.cpu().numpy() for k, v in fields.items()})
            if ref is None or o["ref"] == "previous":
                ref = (key, cur)
    rows = out["frames"]
    scored = {k: r for k, r in rows.items() if "mean" in r}
    summary = {"frames": len(rows), "kept_fraction": sum(r["kept_fraction"] for r in rows.values()) / len(rows) if rows else 0.0}
    if scored:
        summary["mean"] = sum(r["mean"] for r in scored.values()) / len(scored)
        worst = max(sorted(scored), key=lambda k: scored[k]["mean"])
        summary["worst_frame"], summary["worst_mean"] = worst, scored[worst]["mean"]
    out["summary"] = summary
    return out


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    out = drift_tree(args)
    with open(os.path.join(args.output_dir, args.exp, args.seq, "drift.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("drift", json.dumps(out["summary"]))
    if args.png_decoder == "gpu":
        from . import png
        print("drift", png.schedule_report())


if __name__ == "__main__":
    main()
