"""
The capture photographs projected into a frame's UV texture on the GPU, over csrc/t4d_projtex.hip (include/topo4d_raster.h
states the per-texel rule; tests/projtex_ref.py restates it in numpy bit for bit):

    project(pos, nrm, coverage, cams, photos, depth, ...)   -> (color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8)
    view_flows(renders, photos, depth, ...)                 -> (flows int16 [V,H,W,2], support uint8 [V,H,W], report): each view against the consensus
    low_band(photos, depth, radius)                         -> low [V,3,H,W] float32: each photograph's box mean over its mesh pixels
    project_bands(pos, nrm, coverage, cams, photos, low, depth, ...) -> (low_color, weight, count, high, best_weight): mode "twoband"
    surface_maps(face_obj, vertices, res, device)           -> (pos [h,w,3], nrm [h,w,3], coverage [h,w]) of a face.obj's UV layout
    project_frame(face_obj, vertices, dataset, res, ...)    -> (texture [h,w,3] uint8, weight, count): one frame from its views
    pair_stats(pos, nrm, coverage, groups, ...)             -> (count [V,V], sums [V,V,3]) int64: what the cameras share, per pair
    solve_gains(count, sums, ...)                           -> float64 [V,3]: one gain per camera and channel, on the host
    estimate_gains(face_obj, vertices, dataset, res, ...)   -> (gains, report) of one frame; write_gains / read_gains: proj_gains.json
    consistency(pos, nrm, coverage, groups, ...)            -> (skip int32 [h,w], votes uint8 [h,w]): the views to leave out, per texel
    frame_consistency(face_obj, vertices, dataset, res, ...) -> (skip, votes) of one frame, the bits in dataset order; rejected_count(skip)
    uv_islands(face_obj)                                    -> int [n_uv]: the UV island of every UV vertex, numbered from 1 (host)
    island_labels(face_obj, h, w, device)                   -> uint8 [h,w]: the island of every texel, 0 outside the coverage

Every texel is coloured from the cameras that see it: a view counts when the texel's point projects inside its photograph,
in front of the near plane, is not hidden (the depth map of meshrender.MeshRenderer.render, within depth_tol) and faces the
camera (cos of the angle between normal and viewing direction >= cos_min).  mode="weighted" blends the views by cos^power,
faded over fade_px pixels towards the image edge; mode="best" keeps the single view of largest weight.  The four defaults are
conventional choices, not tuned on a capture.  Unlike face.png (the texture loop's Gaussian-filtered
colour field) this is the photographs themselves.  There is no CPU path.

Calibration, the tracked mesh and the lens model are never exact to the pixel, so the views disagree by a pixel or two: "weighted"
then smears the detail the photographs carry, and "best" shows a step wherever the best view changes, since what equalisation
leaves (shading, vignetting) is no gain per camera.  mode="twoband" (project_frame, both command lines) takes the next step of
stitchers and photogrammetry texturing (Brown & Lowe's multi-band blending, Baumberg's two-band texture blending): low_band
low-passes every photograph with a box of band_radius pixels over its mesh pixels, project_bands blends these low bands over all
views as "weighted" does and takes the detail above them, photograph minus low band, from the best view alone; the texture is the
sum.  The low-pass runs on the photographs, since a blur in UV space would run across island borders.  Known limit: across a
self-occlusion edge (nose over cheek) the box mixes the two surfaces.  band_radius = 8 is a conventional choice, not tuned on a
capture, and is in pixels of the photograph.

The cameras of a rig never agree exactly in exposure and white balance, and a blend of unequal cameras shows a step wherever the
set of contributing views changes.  pair_stats counts, for every pair of cameras, the texels both see and sums each camera's
samples there (integers, so the result is the same bits in any order); solve_gains finds the gain per camera and channel that
makes the pairs agree in the least-squares sense (the gain compensation of panorama stitchers, in the log domain), and project /
project_frame take these gains.  Exposure belongs to the rig, not to a frame: one set of gains serves a whole run.

Specular highlights (skin, eyes and lips are glossy, and a highlight sits elsewhere in every camera), leaks of the occlusion test
(hair, lashes, a nose rim the tracked mesh does not model) and transient content in one camera (a blink) are no gain per camera
and no registration error: one view disagrees with a consensus of the others.  consistency is the per-texel photo-consistency check
of MVS texturing (Waechter et al., "Let There Be Color!"): at a texel the views that face it (cos >= vote_cos_min) vote, the lower
median of their samples per channel is the consensus, and a view further than reject_tol from it in some channel is rejected: its
bit is set in skip, which project, project_bands and project_frame(reject=...) take.  With fewer than min_votes voters, or when
every view would go, nothing is rejected, so a texel never loses its last view.  The samples are integers of 2^-16, so the mask is
the same bits in any order.  The stages run in the order equalise, reject, blend, fill.  The defaults (0.1, 0.5, 3) are conventional
choices, not tuned on a capture.  Known limits: with fewer than min_votes facing views nothing is rejected, so the rim of the
coverage keeps its highlights; a defect most voters share survives; the threshold is absolute, so it is looser in the shadows than
a relative one would be.  --reject (train: --tex_reject) switches it on; --save_rejected also writes face_proj_rejected.png, the
number of rejected views per texel.

None of the stages above registers the views of one frame against each other: the gains equalise exposure, the consistency check
drops outliers, two bands keep only the best view's detail.  The standard cure in photogrammetry texturing is a small 2D flow per
view against the consensus, through which the photograph is sampled (Eisemann et al., "Floating Textures"); it lets "weighted" and
the low band of "twoband" blend many views without blurring them.  project_frame(register=...) projects the frame once in mode
"weighted" (with the gains and the mask), fills that texture's holes per island, renders it into every camera
(meshrender.MeshRenderer.render) and calls view_flows, which matches every photograph against its render with the pieces of drift
(match: the census block matcher; flow: sub-pixel offsets; dense_flow: a per-pixel field in 1/256 px) and returns the fields as
int16.  project and project_bands take them as flows=: a view is accepted and weighed at its unshifted pixel exactly as without
flows (geometry decides visibility and weight), the flow read at the nearest pixel moves only the colour sample, and a view whose
moved taps leave the image is left out (include/topo4d_raster.h, F.1..F.5; tests/projtex_flow_ref.py restates it bit for bit).
The stages run in the order equalise, reject, register, blend, fill.  --register (train: --tex_register) switches it on, with
--reg_block, --reg_stride, --reg_radius, --reg_ratio, --reg_reach and --reg_rounds; every frame then also gets
face_proj_register.json (the options and view_flows' report) and with --save_flows face_proj_flows.npz (flows, support, camera
names).  Known limits: a block straddling a self-occlusion edge (nose over cheek) matches two surfaces; the census needs texture,
so smooth skin at low resolution keeps few blocks and falls back to zero flow there; a misregistration beyond the radius is
dropped, not corrected; consistency and pair_stats still sample unregistered, so rejection and gain statistics are taken on
unregistered samples; the defaults (block 32, stride 16, radius 4, ratio 0.8, reach 1, one round) are conventional, not tuned on a
capture.

`python -m topo4d_amd.projtex -e EXP -s SEQ [-id ... -did ... -od ... -dr N] [--frames 1-10] [--views A,B] [--set low|dense]
[--undistort] [--tex_res R] [--mode weighted|best|twoband [--band_radius R]] [--power P --cos_min C --fade_px F --depth_tol T] [--tex_pad R]
[--tex_sizes 2048,1024] [--save_weight] [--tex_fill] [--equalize [--equalize_frames 1-10] | --gains FILE] [--stat_cos_min C --stat_lo L
--stat_hi H --eq_prior P --eq_min_overlap N] [--reject [--reject_tol T --vote_cos_min C --min_votes N] [--save_rejected]]
[--register [--reg_block B --reg_stride S --reg_radius R --reg_ratio Q --reg_reach K --reg_rounds N] [--save_flows]]` works on an output tree that already exists (the reference's too): it writes
%06d/face_proj.png (and face_proj_<size>.png) beside every frame's face.obj, with --save_weight also face_proj_weight.png (the
8-bit count of contributing views).  By default it projects the full-size photographs of the cameras training uses.
--equalize gathers the pair statistics over --equalize_frames (default: the first frame projected), solves once, writes
proj_gains.json into the run directory and projects every frame with these gains; --gains FILE takes a saved file instead.
`python -m topo4d_amd.train --tex_project` writes the same file while the run is made; with --tex_equalize it estimates the gains on the first frame it writes.

project and project_bands write zeros where no view counts: under the chin, in the nostrils, behind the ears.  --tex_fill (both
command lines; write_frame(fill=True)) fills these texels island by island with texfinish.fill_islands over island_labels, the
push-pull interpolation of the island's projected texels, before the gutter and the smaller levels are made; an island no view
sees at all stays black, and face_proj_weight.png still holds the count, so its zeros inside an island mark what was filled.
Known limit: the fill interpolates in UV space and knows nothing of the surface, so a large hole comes out smooth, not plausible.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
from typing import Tuple

import numpy as np
import torch

from . import _lib, _run
from ._lib import ptr

T4D_PROJTEX_WEIGHTED, T4D_PROJTEX_BEST = 0, 1
_MODES = {"weighted": T4D_PROJTEX_WEIGHTED, "best": T4D_PROJTEX_BEST}
MODES = (*_MODES, "twoband")                                   # "twoband" is project_bands', not a mode of the one kernel
MAX_POWER, MAX_VIEWS, MAX_BAND_RADIUS = 8, 255, 32
DEFAULTS = dict(power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002, mode="weighted")
BAND_DEFAULTS = dict(band_radius=8)
FILE_NAME, WEIGHT_NAME = "face_proj.png", "face_proj_weight.png"
MAX_STAT_VIEWS, MAX_STAT = 32, 1024.0                          # pair_stats: a 32-bit mask of views per texel; |stat_lo|, |stat_hi|
STAT_DEFAULTS = dict(stat_cos_min=0.5, stat_lo=0.02, stat_hi=0.98)
SOLVE_DEFAULTS = dict(prior=0.01, min_overlap=64)
GAINS_NAME = "proj_gains.json"
MAX_REJECT_TOL = 4.0                                           # consistency: samples are clamped to [0, 4] before they are rounded
CONSIST_DEFAULTS = dict(reject_tol=0.1, vote_cos_min=0.5, min_votes=3)
REJECTED_NAME = "face_proj_rejected.png"
MAX_REG_ROUNDS = 3
REG_DEFAULTS = dict(block=32, stride=None, radius=4, ratio=0.8, reach=1)      # view_flows'; stride None: block // 2
REGISTER_DEFAULTS = dict(**REG_DEFAULTS, rounds=1)                            # project_frame's `register`
REGISTER_NAME, FLOWS_NAME = "face_proj_register.json", "face_proj_flows.npz"


def _filled(defaults: dict, **given) -> dict:
    """`given`, every None replaced by its default"""
    return {k: defaults[k] if v is None else v for k, v in given.items()}


def check_options(power=None, cos_min=None, fade_px=None, depth_tol=None, mode=None) -> dict:
    """ValueError for a parameter project would refuse (callable without a device); the five options, None: DEFAULTS'."""
    o = _filled(DEFAULTS, power=power, cos_min=cos_min, fade_px=fade_px, depth_tol=depth_tol, mode=mode)
    if o["mode"] not in MODES:
        raise ValueError(f"mode must be 'weighted', 'best' or 'twoband', got {o['mode']!r}")
    if isinstance(o["power"], bool) or int(o["power"]) != o["power"] or not 0 <= int(o["power"]) <= MAX_POWER:
        raise ValueError(f"power must be an integer in [0, {MAX_POWER}], got {o['power']!r}")
    for k, lo, hi in (("cos_min", -1.0, 1.0), ("fade_px", 0.0, 65536.0), ("depth_tol", 0.0, 1.0)):
        if not lo <= float(o[k]) <= hi:
            raise ValueError(f"{k} must be in [{lo:g}, {hi:g}], got {o[k]!r}")
    return o


def _rule(o: dict) -> tuple:
    """the four parameters of the per-view rule as the C entry points take them"""
    return int(o["power"]), float(o["cos_min"]), float(o["fade_px"]), float(o["depth_tol"])


def check_band_options(band_radius=8) -> None:
    """ValueError for a radius low_band would refuse (callable without a device)."""
    if isinstance(band_radius, bool) or not isinstance(band_radius, (int, float, np.integer, np.floating)) \
            or int(band_radius) != band_radius or not 0 <= int(band_radius) <= MAX_BAND_RADIUS:
        raise ValueError(f"band_radius must be an integer in [0, {MAX_BAND_RADIUS}], got {band_radius!r}")


def check_stat_options(stat_cos_min=None, stat_lo=None, stat_hi=None) -> dict:
    """ValueError for a parameter pair_stats would refuse (callable without a device)."""
    o = _filled(STAT_DEFAULTS, stat_cos_min=stat_cos_min, stat_lo=stat_lo, stat_hi=stat_hi)
    if not -1.0 <= float(o["stat_cos_min"]) <= 1.0:
        raise ValueError(f"stat_cos_min must be in [-1, 1], got {o['stat_cos_min']!r}")
    if not -MAX_STAT <= float(o["stat_lo"]) <= float(o["stat_hi"]) <= MAX_STAT:
        raise ValueError(f"need -{MAX_STAT:g} <= stat_lo <= stat_hi <= {MAX_STAT:g}, got {o['stat_lo']!r} and {o['stat_hi']!r}")
    return o


def check_consist_options(reject_tol=None, vote_cos_min=None, min_votes=None) -> dict:
    """ValueError for a parameter consistency would refuse (callable without a device); the three options, None: CONSIST_DEFAULTS'."""
    o = _filled(CONSIST_DEFAULTS, reject_tol=reject_tol, vote_cos_min=vote_cos_min, min_votes=min_votes)
    for k, lo, hi in (("reject_tol", 0.0, MAX_REJECT_TOL), ("vote_cos_min", -1.0, 1.0)):
        if isinstance(o[k], bool) or not isinstance(o[k], (int, float, np.integer, np.floating)) or not lo <= float(o[k]) <= hi:
            raise ValueError(f"{k} must be in [{lo:g}, {hi:g}], got {o[k]!r}")
    n = o["min_votes"]
    if isinstance(n, bool) or not isinstance(n, (int, float, np.integer, np.floating)) or not np.isfinite(n) or int(n) != n \
            or not 2 <= int(n) <= MAX_STAT_VIEWS:
        raise ValueError(f"min_votes must be an integer in [2, {MAX_STAT_VIEWS}], got {n!r}")
    return o


def _whole(x, what: str, lo: int, hi: int) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x) or int(x) != x \
            or not lo <= int(x) <= hi:
        raise ValueError(f"{what} must be an integer in [{lo}, {hi}], got {x!r}")
    return int(x)


def check_reg_options(block=None, stride=None, radius=None, ratio=None, reach=None) -> dict:
    """ValueError for a parameter view_flows would refuse (callable without a device); the five options, None: REG_DEFAULTS'
    (stride: block // 2).  block, stride and radius are drift.match's, ratio is drift.flow's, reach is drift.dense_flow's."""
    from . import drift
    o = _filled(REG_DEFAULTS, block=block, stride=None, radius=radius, ratio=ratio, reach=reach)
    o["block"] = _whole(o["block"], "block", drift.MIN_BLOCK, drift.MAX_BLOCK)
    o["radius"] = _whole(o["radius"], "radius", 0, drift.MAX_RADIUS)
    o["reach"] = _whole(o["reach"], "reach", 1, drift.MAX_REACH)
    o["stride"] = None if stride is None else _whole(stride, "stride", 1, o["block"])
    o["block"], o["stride"], o["radius"], _ = drift.check_options(o["block"], o["stride"], o["radius"])
    if isinstance(o["ratio"], bool) or not isinstance(o["ratio"], (int, float, np.integer, np.floating)) or not 0.0 < float(o["ratio"]) <= 1.0:
        raise ValueError(f"ratio must be in (0, 1], got {o['ratio']!r}")
    o["ratio"] = float(o["ratio"])
    drift.check_reach(o["reach"], o["stride"], 0)
    return o


def check_register_options(register) -> dict:
    """None, or the checked options of project_frame's `register`: a dict of view_flows' options and rounds (1..3), {} for
    REGISTER_DEFAULTS; ValueError for anything else (callable without a device)."""
    if register is None:
        return None
    if not isinstance(register, dict) or set(register) - set(REGISTER_DEFAULTS):
        raise ValueError(f"register must be a dict of {', '.join(REGISTER_DEFAULTS)}, got {register!r}")
    rounds = register.get("rounds")
    o = check_reg_options(**{k: v for k, v in register.items() if k != "rounds"})
    o["rounds"] = _whole(REGISTER_DEFAULTS["rounds"] if rounds is None else rounds, "rounds", 1, MAX_REG_ROUNDS)
    return o


def check_solve_options(prior=None, min_overlap=None) -> dict:
    """ValueError for a parameter solve_gains would refuse."""
    o = _filled(SOLVE_DEFAULTS, prior=prior, min_overlap=min_overlap)
    if not 0.0 <= float(o["prior"]) < float("inf"):
        raise ValueError(f"prior must be finite and >= 0, got {o['prior']!r}")
    if isinstance(o["min_overlap"], bool) or int(o["min_overlap"]) != o["min_overlap"] or int(o["min_overlap"]) < 1:
        raise ValueError(f"min_overlap must be a positive integer, got {o['min_overlap']!r}")
    return o


def _gains(gains, V: int):
    """None, or gains as a float64 [V,3] host array; ValueError for anything else"""
    if gains is None:
        return None
    g = np.asarray(gains.detach().cpu() if isinstance(gains, torch.Tensor) else gains)
    if g.shape != (V, 3) or g.dtype.kind not in "fiu":
        raise ValueError(f"gains must be a real [{V},3] array (one per view and channel), got {g.dtype} {list(g.shape)}")
    g = np.ascontiguousarray(g, dtype=np.float64)
    if not np.isfinite(g).all():
        raise ValueError("gains must be finite")
    return g


def _map(t, what: str, shape, dtype) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be a {str(dtype).split('.')[-1]} tensor of shape {list(shape)}, got "
                         f"{getattr(t, 'dtype', type(t))} {list(getattr(t, 'shape', ()))}")
    return t


def _texel_maps(pos, nrm, coverage) -> tuple:
    """(h, w, device) of the texel maps as project, project_bands and pair_stats take them; ValueError for anything else"""
    if not isinstance(pos, torch.Tensor) or pos.dim() != 3 or pos.shape[2] != 3 or pos.shape[0] < 1 or pos.shape[1] < 1:
        raise ValueError(f"pos must be a float32 [h,w,3] tensor, got {list(getattr(pos, 'shape', ()))}")
    h, w = int(pos.shape[0]), int(pos.shape[1])
    _map(pos, "pos", (h, w, 3), torch.float32)
    _map(nrm, "nrm", (h, w, 3), torch.float32)
    if not isinstance(coverage, torch.Tensor) or coverage.dtype not in (torch.uint8, torch.bool) or tuple(coverage.shape) != (h, w):
        raise ValueError(f"coverage must be a uint8 or bool [{h},{w}] tensor")
    return h, w, pos.device


def _view_group(dev, cams, depth, **images) -> tuple:
    """(packed views, V, H, W) of the views of one image size, with their depth maps and `images` (photos=..., project_bands: low=...)"""
    from .meshrender import _views
    views, H, W = _views(cams, dev)
    V = int(views.shape[0])
    if V > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views per call, got {V}")
    for name, t in images.items():
        _map(t, name, (V, 3, H, W), torch.float32)
    _map(depth, "depth", (V, 1, H, W), torch.float32)
    return views, V, H, W


def _skip(skip, skip_base, h: int, w: int, V: int) -> list:
    """[] for no mask, or [("skip", skip)] for _placed: skip an int32 [h,w] tensor (consistency's), skip_base an integer with
    skip_base >= 0 and skip_base + V <= 32; ValueError for anything else"""
    if isinstance(skip_base, bool) or not isinstance(skip_base, (int, np.integer)):
        raise ValueError(f"skip_base must be an integer, got {skip_base!r}")
    if skip is None:
        if skip_base != 0:
            raise ValueError(f"skip_base {skip_base} without skip")
        return []
    _map(skip, "skip", (h, w), torch.int32)
    if skip_base < 0 or skip_base + V > MAX_STAT_VIEWS:
        raise ValueError(f"skip holds {MAX_STAT_VIEWS} views: need skip_base >= 0 and skip_base + {V} views <= {MAX_STAT_VIEWS}, got "
                         f"skip_base {skip_base}")
    return [("skip", skip)]


def _flows(flows, V: int, H: int, W: int) -> list:
    """[] for no flows, or [("flows", flows)] for _placed: view_flows' int16 [V,H,W,2] tensor; ValueError for anything else"""
    return [] if flows is None else [("flows", _map(flows, "flows", (V, H, W, 2), torch.int16))]


def _placed(dev, pos, nrm, coverage, others, g) -> tuple:
    """The last step before a launch, after every argument error: the named tensors `others` live where pos does (ValueError), and
    that is a HIP device (RuntimeError).  (pos, nrm, coverage as uint8, others' tensors), all contiguous, and the gains uploaded."""
    for name, t in [("nrm", nrm), ("coverage", coverage), *others]:
        if t.device != dev:
            raise ValueError(f"{name} must live on pos's device {dev}, got {t.device}")
    if dev.type != "cuda":
        raise RuntimeError("topo4d_amd has no CPU path: the maps, the photographs and the depth must live on a HIP device")
    cov = coverage.to(torch.uint8) if coverage.dtype == torch.bool else coverage
    return pos.contiguous(), nrm.contiguous(), cov.contiguous(), [t.contiguous() for _, t in others], None if g is None else torch.from_numpy(g).to(dev)


def project(pos: torch.Tensor, nrm: torch.Tensor, coverage: torch.Tensor, cams, photos: torch.Tensor, depth: torch.Tensor, *,
            power=None, cos_min=None, fade_px=None, depth_tol=None, mode=None, gains=None, skip=None,
            skip_base=0, flows=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8).  pos / nrm [h,w,3] float32: each texel's point in the
    training world frame and its normal (any length; a zero normal switches the texel off); coverage [h,w] uint8 or bool;
    cams: a sequence of GaussianRasterizationSettings of one size, or (packed view records, H, W), as MeshRenderer.render takes
    them; photos [V,3,H,W] float32; depth [V,1,H,W] float32, MeshRenderer.render's (0: empty).  Everything on one HIP device.
    power, cos_min, fade_px, depth_tol, mode: None is DEFAULTS'.  gains [V,3] (None: none): view v's sample is multiplied by
    gains[v] in the kernel, in float64; no scaled copy of the photographs is made.  skip (None: no mask): consistency's int32
    [h,w] mask on the same device; view v of this call is left out at a texel, exactly as a view the rule does not accept there,
    when bit skip_base + v of skip is set (skip_base an integer, skip_base + V <= 32): it enters no blend, cannot be the best
    view and does not count.  flows (None: none): view_flows' int16 [V,H,W,2] tensor on the same device, (f_y, f_x) in 1/256 px:
    a view is accepted and weighed at its pixel (px, py) as without flows, and its photograph is then sampled at (px + f_x / 256,
    py + f_y / 256), the flow read at the pixel nearest to (px, py); a view whose moved taps leave the image is left out as a
    masked one is.  An all-zero flows gives the bits of None."""
    o = check_options(power, cos_min, fade_px, depth_tol, mode)
    if o["mode"] not in _MODES:
        raise ValueError(f"mode {o['mode']!r} has five outputs and takes the low bands: it is project_bands'")
    h, w, dev = _texel_maps(pos, nrm, coverage)
    views, V, H, W = _view_group(dev, cams, depth, photos=photos)
    g = _gains(gains, V)
    mask, flow = _skip(skip, skip_base, h, w, V), _flows(flows, V, H, W)
    pos, nrm, cov, (photos, depth, *held), g = _placed(dev, pos, nrm, coverage, [("photos", photos), ("depth", depth), *mask, *flow], g)
    color = torch.empty(h, w, 3, dtype=torch.float32, device=dev)
    weight = torch.empty(h, w, dtype=torch.float32, device=dev)
    count = torch.empty(h, w, dtype=torch.uint8, device=dev)
    name, more = ("t4d_project_texture_flow", (ptr(held[-1]),)) if flow else ("t4d_project_texture_skip", ())
    _lib.call(name, ptr(pos), ptr(nrm), ptr(cov), h, w, ptr(views), V, H, W, ptr(photos), ptr(depth), ptr(g),
              *_rule(o), _MODES[o["mode"]], ptr(color), ptr(weight), ptr(count), ptr(held[0]) if mask else None, int(skip_base),
              _lib.stream(dev), *more)
    return color, weight, count


def low_band(photos: torch.Tensor, depth: torch.Tensor, radius: int = 8) -> torch.Tensor:
    """low [V,3,H,W] float32: every photograph's mean over the (2 radius + 1)^2 box, counted over the mesh pixels alone (depth >
    0), so that the background never bleeds into the face at its silhouette; 0 where the box holds no mesh pixel.  photos [V,3,H,W]
    float32, depth [V,1,H,W] float32 (MeshRenderer.render's), on one HIP device; radius an integer in [0, 32], in pixels.  A pixel
    off the mesh is never read (a NaN there stays out); with radius 0 the result is the photographs on the mesh and 0 elsewhere.
    The box is separable, rows first, in float64 (csrc/t4d_projtex.hip states the order; tests/projtex_bands_ref.py restates it
    bit for bit).  Known limit: across a self-occlusion edge the box mixes the two surfaces."""
    check_band_options(radius)
    if not isinstance(photos, torch.Tensor) or photos.dim() != 4 or photos.shape[1] != 3 or min(photos.shape) < 1:
        raise ValueError(f"photos must be a float32 [V,3,H,W] tensor, got {list(getattr(photos, 'shape', ()))}")
    V, _, H, W = (int(x) for x in photos.shape)
    if V > MAX_VIEWS or H > 65536 or W > 65536:
        raise ValueError(f"at most {MAX_VIEWS} views of sides up to 65536 per call, got {V} of {H} x {W}")
    _map(photos, "photos", (V, 3, H, W), torch.float32)
    _map(depth, "depth", (V, 1, H, W), torch.float32)
    if depth.device != photos.device:
        raise ValueError(f"depth must live on photos' device {photos.device}, got {depth.device}")
    if not photos.is_cuda:                                     # argument errors first, with or without a device
        raise RuntimeError("topo4d_amd has no CPU path: the photographs and the depth must live on a HIP device")
    photos, depth = photos.contiguous(), depth.contiguous()
    low = torch.empty_like(photos)
    _lib.call("t4d_projtex_low_band", ptr(photos), ptr(depth), V, H, W, int(radius), ptr(low), _lib.stream(photos.device))
    return low


def project_bands(pos: torch.Tensor, nrm: torch.Tensor, coverage: torch.Tensor, cams, photos: torch.Tensor, low: torch.Tensor,
                  depth: torch.Tensor, *, power=None, cos_min=None, fade_px=None, depth_tol=None, gains=None, skip=None,
                  skip_base=0, flows=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(low_color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8, high [h,w,3] float32, best_weight [h,w] float32): the
    two bands of mode "twoband".  The arguments of project and low [V,3,H,W] float32, low_band's.  Every view that project would
    accept at a texel gives its sample s and, by the same bilinear mix over the same taps of low, its low band l (both times
    gains[v] when given).  low_color, weight, count: the blend of the l as mode "weighted" blends the s.  high = s - l and
    best_weight = the weight of the view mode "best" would keep.  The texture is low_color + high; zeros where no view counts.
    skip, skip_base: as project takes them; a masked view enters neither band.  flows: as project takes them; s and l are both
    sampled at the moved position, and a view whose moved taps leave the image enters neither band."""
    o = check_options(power, cos_min, fade_px, depth_tol)
    h, w, dev = _texel_maps(pos, nrm, coverage)
    views, V, H, W = _view_group(dev, cams, depth, photos=photos, low=low)
    g = _gains(gains, V)
    mask, flow = _skip(skip, skip_base, h, w, V), _flows(flows, V, H, W)
    pos, nrm, cov, (photos, low, depth, *held), g = _placed(dev, pos, nrm, coverage,
                                                              [("photos", photos), ("low", low), ("depth", depth), *mask, *flow], g)
    low_color, high = (torch.empty(h, w, 3, dtype=torch.float32, device=dev) for _ in range(2))
    weight, best_weight = (torch.empty(h, w, dtype=torch.float32, device=dev) for _ in range(2))
    count = torch.empty(h, w, dtype=torch.uint8, device=dev)
    name, more = ("t4d_project_texture_bands_flow", (ptr(held[-1]),)) if flow else ("t4d_project_texture_bands_skip", ())
    _lib.call(name, ptr(pos), ptr(nrm), ptr(cov), h, w, ptr(views), V, H, W, ptr(photos), ptr(low), ptr(depth),
              ptr(g), *_rule(o), ptr(low_color), ptr(weight), ptr(count), ptr(high), ptr(best_weight), ptr(held[0]) if mask else None,
              int(skip_base), _lib.stream(dev), *more)
    return low_color, weight, count, high, best_weight


def flow_report(d, kept) -> dict:
    """One view's entry of view_flows' report, on the host in float64: "blocks" and "kept", and over the kept blocks of drift.flow's
    d [nby,nbx,2] the mean (the exactly rounded sum over their number), the lower median, p90 (the value of rank ceil(0.9 n)) and the
    max of |d| = sqrt(dy dy + dx dx), in pixels; a view without a kept block has the first two only."""
    import math
    d, kept = np.asarray(d, np.float64).reshape(-1, 2), np.asarray(kept).reshape(-1) != 0
    n = int(kept.sum())
    out = {"blocks": int(kept.size), "kept": n}
    if n:
        srt = np.sort(np.sqrt(d[kept, 0] * d[kept, 0] + d[kept, 1] * d[kept, 1]))
        out.update(mean=math.fsum(srt.tolist()) / n, median=float(srt[(n - 1) // 2]), p90=float(srt[min(n - 1, -(-9 * n // 10) - 1)]),
                   max=float(srt[-1]))
    return out


def view_flows(renders: torch.Tensor, photos: torch.Tensor, depth: torch.Tensor, *, block=32, stride=None, radius=4, ratio=0.8,
               reach=1) -> Tuple[torch.Tensor, torch.Tensor, list]:
    """(flows int16 [V,H,W,2], support uint8 [V,H,W], report): every view registered against the consensus.  renders [V,3,H,W] float32:
    the consensus texture in every camera (meshrender.MeshRenderer.render); photos [V,3,H,W] float32; depth [V,1,H,W] float32, the
    render's; on one HIP device.  Per view: image A is texfinish.quantize of the render and B of the photograph; a pixel is valid in
    both when depth > 0 and A's pixel is not zero in all three channels, and its label is then 1; drift.match(A, valid, B, valid,
    labels, block, stride, radius), drift.flow(table, radius, ratio) and drift.dense_flow(d, kept, labels, block, stride, 0, reach)
    give the field, which is cast to int16 (|f| <= (radius + 0.5) 256).  A at x shows what B shows at x + f / 256: what project's
    flows are.  support: 1 where a kept block reaches the pixel; the flow is 0 elsewhere.  report: flow_report per view.  The options
    (REG_DEFAULTS; stride None: block // 2) are conventional choices, not tuned on a capture.  The views go one after
    the other: the peak memory is one view's intermediates and the int16 stack.  Known limits: a block straddling a self-occlusion
    edge (nose over cheek) matches two surfaces; the census needs texture, so smooth skin at low resolution keeps few blocks and
    falls back to zero flow there; a misregistration beyond `radius` is dropped, not corrected."""
    from . import drift, texfinish
    o = check_reg_options(block, stride, radius, ratio, reach)
    if not isinstance(renders, torch.Tensor) or renders.dim() != 4 or renders.shape[1] != 3 or min(renders.shape) < 1:
        raise ValueError(f"renders must be a float32 [V,3,H,W] tensor, got {list(getattr(renders, 'shape', ()))}")
    V, _, H, W = (int(x) for x in renders.shape)
    if V > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views per call, got {V}")
    _map(renders, "renders", (V, 3, H, W), torch.float32)
    _map(photos, "photos", (V, 3, H, W), torch.float32)
    _map(depth, "depth", (V, 1, H, W), torch.float32)
    for name, t in (("photos", photos), ("depth", depth)):
        if t.device != renders.device:
            raise ValueError(f"{name} must live on renders' device {renders.device}, got {t.device}")
    if not renders.is_cuda:                                    # argument errors first, with or without a device
        raise RuntimeError("topo4d_amd has no CPU path: the renders, the photographs and the depth must live on a HIP device")
    dev = renders.device
    flows = torch.empty(V, H, W, 2, dtype=torch.int16, device=dev)
    support = torch.empty(V, H, W, dtype=torch.uint8, device=dev)
    report = []
    with torch.cuda.device(dev):
        for v in range(V):
            a = texfinish.quantize(renders[v].permute(1, 2, 0).contiguous())
            b = texfinish.quantize(photos[v].permute(1, 2, 0).contiguous())
            valid = ((depth[v, 0] > 0) & (a != 0).any(dim=2)).to(torch.uint8)      # the labels too: 1 on valid pixels
            table = drift.match(a, valid, b, valid, valid, o["block"], o["stride"], o["radius"])
            d, kept = drift.flow(table, o["radius"], o["ratio"])
            f, s = drift.dense_flow(d, kept, valid, o["block"], o["stride"], 0, o["reach"], check=False)
            flows[v], support[v] = f.to(torch.int16), s
            report.append(flow_report(d.cpu().numpy(), kept.cpu().numpy()))
    return flows, support, report


def _mixed_views(dev, groups: list, name: str, what: str) -> tuple:
    """(packed records per group, (H, W) per view, [(what, photos), (what, depth)] per group for _placed) of the groups pair_stats
    and consistency take: (cams, photos, depth) per image size, at most 32 views in all; ValueError for anything else"""
    if not groups:
        raise ValueError(f"{name}: no views")
    records, sizes, held = [], [], []
    for cams, photos, depth in groups:
        views, v, H, W = _view_group(dev, cams, depth, photos=photos)
        if not 1 <= H <= 65536 or not 1 <= W <= 65536:
            raise ValueError(f"image sides must be in [1, 65536], got {H} x {W}")
        records.append(views)
        sizes += [(H, W)] * v
        held += [(what, photos), (what, depth)]
    if len(sizes) > MAX_STAT_VIEWS:
        raise ValueError(f"at most {MAX_STAT_VIEWS} views per call, got {len(sizes)}")
    return records, sizes, held


def _view_tables(dev, records, sizes, held) -> tuple:
    """(views [V,40], sizes [V,2] int32, tables [2,V] int64: the views' photograph and depth pointers) on the device.  held: the
    contiguous photographs and depth maps of _placed, group after group; the caller keeps them alive until the launch is queued
    on their stream."""
    photo_ptrs = [p[k].data_ptr() for p in held[0::2] for k in range(p.shape[0])]
    depth_ptrs = [d[k].data_ptr() for d in held[1::2] for k in range(d.shape[0])]
    tables = torch.tensor([photo_ptrs, depth_ptrs], dtype=torch.int64).to(dev)
    return torch.cat(records).contiguous(), torch.tensor(sizes, dtype=torch.int32).to(dev), tables


def pair_stats(pos: torch.Tensor, nrm: torch.Tensor, coverage: torch.Tensor, groups, *, gains=None, out=None, stat_cos_min=None,
               stat_lo=None, stat_hi=None, power=None, cos_min=None, fade_px=None, depth_tol=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(count [V,V], sums [V,V,3]), int64 on the device.  pos, nrm, coverage as project takes them; groups: a list of (cams, photos
    [v,3,H,W], depth [v,1,H,W]) as project takes them, one per image size, V <= 32 views in all, numbered in the order given.  View v
    takes part at a texel when project would accept it there (power, cos_min, fade_px, depth_tol), its cosine is >= stat_cos_min
    and every channel of its sample (times gains[v], [V,3], when given) lies in [stat_lo, stat_hi]: a clipped or black sample follows
    no gain model.  count[i][j]: the texels where i and j both take part; sums[i][j]: the sum of view i's samples there, as integers
    in units of 2^-16 (count[i][i], sums[i][i]: over all of view i's texels).  out = (count, sums) of an earlier call is added to and
    returned: the statistics of several frames.  The three stat_* defaults (None: STAT_DEFAULTS') are conventional choices (a facing
    limit of 60 degrees, 2 % off either end of the range), not tuned on a capture."""
    o = check_options(power, cos_min, fade_px, depth_tol)
    stat = check_stat_options(stat_cos_min, stat_lo, stat_hi)
    h, w, dev = _texel_maps(pos, nrm, coverage)
    groups = list(groups)
    records, sizes, held = _mixed_views(dev, groups, "pair_stats", "photos, depth and out")
    V = len(sizes)
    g = _gains(gains, V)
    if out is not None:
        count, sums = out
        _map(count, "out[0]", (V, V), torch.int64)
        _map(sums, "out[1]", (V, V, 3), torch.int64)
    pos, nrm, cov, held, g = _placed(dev, pos, nrm, coverage, held + [("photos, depth and out", t) for t in out or ()], g)
    if out is None:
        count, sums = torch.zeros(V, V, dtype=torch.int64, device=dev), torch.zeros(V, V, 3, dtype=torch.int64, device=dev)
    elif not (count.is_contiguous() and sums.is_contiguous()):
        raise ValueError("out must be contiguous")
    views, sizes_t, tables = _view_tables(dev, records, sizes, held[:2 * len(groups)])
    _lib.call("t4d_projtex_pair_stats", ptr(pos), ptr(nrm), ptr(cov), h, w, ptr(views), V, ptr(sizes_t), ptr(tables[0]), ptr(tables[1]),
              *_rule(o), float(stat["stat_cos_min"]), float(stat["stat_lo"]), float(stat["stat_hi"]), ptr(g), ptr(count), ptr(sums),
              _lib.stream(dev))
    return count, sums


def consistency(pos: torch.Tensor, nrm: torch.Tensor, coverage: torch.Tensor, groups, *, gains=None, reject_tol=None, vote_cos_min=None,
                min_votes=None, power=None, cos_min=None, fade_px=None, depth_tol=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(skip int32 [h,w], votes uint8 [h,w]) on the device: the per-texel photo-consistency check (Waechter et al., "Let There Be
    Color!").  pos, nrm, coverage, groups and gains as pair_stats takes them: V <= 32 views of any mix of sizes, numbered in the
    order given.  At a texel the views project would accept (power, cos_min, fade_px, depth_tol) give their samples (times gains[v]),
    clamped to [0, 4] and rounded to integers of 2^-16; those with a cosine >= vote_cos_min are the voters, votes their number.
    With at least min_votes voters, a view (voter or not) whose sample is further than reject_tol from the voters' lower median in
    some channel is an outlier, and bit v of skip (bit 31: the sign) is set for every outlier v, unless every accepted view is one:
    then, as with fewer voters, nothing is rejected, so a texel never loses its last view.  Integers throughout: the result is the
    same bits in any order (include/topo4d_raster.h states the rule, tests/projtex_consist_ref.py restates it).  project and
    project_bands take skip.  The three defaults (None: CONSIST_DEFAULTS': a tenth of the range, a facing limit of 60 degrees, three
    voters) are conventional choices, not tuned on a capture.  Known limits: where fewer than min_votes views face a texel (the
    rim of the coverage) nothing is rejected; a defect most voters share survives; the threshold is absolute, so it is looser in the
    shadows than a relative one would be."""
    o = check_options(power, cos_min, fade_px, depth_tol)
    c = check_consist_options(reject_tol, vote_cos_min, min_votes)
    h, w, dev = _texel_maps(pos, nrm, coverage)
    groups = list(groups)
    records, sizes, held = _mixed_views(dev, groups, "consistency", "photos and depth")
    V = len(sizes)
    g = _gains(gains, V)
    pos, nrm, cov, held, g = _placed(dev, pos, nrm, coverage, held, g)
    views, sizes_t, tables = _view_tables(dev, records, sizes, held)
    skip = torch.empty(h, w, dtype=torch.int32, device=dev)
    votes = torch.empty(h, w, dtype=torch.uint8, device=dev)
    _lib.call("t4d_projtex_consistency", ptr(pos), ptr(nrm), ptr(cov), h, w, ptr(views), V, ptr(sizes_t), ptr(tables[0]), ptr(tables[1]),
              *_rule(o), ptr(g), float(c["reject_tol"]), float(c["vote_cos_min"]), int(c["min_votes"]), ptr(skip), ptr(votes),
              _lib.stream(dev))
    return skip, votes


def _solve(count, sums, prior=None, min_overlap=None):
    prior, min_overlap = check_solve_options(prior, min_overlap).values()
    count = np.asarray(count.detach().cpu() if isinstance(count, torch.Tensor) else count)
    sums = np.asarray(sums.detach().cpu() if isinstance(sums, torch.Tensor) else sums)
    if count.ndim != 2 or count.shape[0] != count.shape[1] or count.shape[0] < 1 or sums.shape != (*count.shape, 3):
        raise ValueError(f"count must be [V,V] and sums [V,V,3], got {list(count.shape)} and {list(sums.shape)}")
    V = count.shape[0]
    count, sums = count.astype(np.float64), sums.astype(np.float64)
    gains = np.ones((V, 3))
    report = dict(pairs=[], rms_before=[], rms_after=[])
    off = ~np.eye(V, dtype=bool)
    for c in range(3):
        s = sums[..., c]
        use = off & (count >= min_overlap) & (s > 0) & (s.T > 0)
        N = np.where(use, count, 0.0)
        with np.errstate(all="ignore"):
            d = np.where(N > 0, np.log(np.where(use, s, 1.0)) - np.log(np.where(use, s.T, 1.0)), 0.0)
        n = N.sum(1)
        A = -N + np.diag((1.0 + prior) * n)
        b = -(N * d).sum(1)
        lone = n == 0
        A[lone, lone] = 1.0
        l = np.linalg.solve(A, b)
        l[lone] = 0.0
        gains[:, c] = np.exp(l)
        total = N.sum()
        r = l[:, None] - l[None, :] + d
        report["pairs"].append(int((N > 0).sum() // 2))
        report["rms_before"].append(float(np.sqrt((N * d * d).sum() / total)) if total else 0.0)
        report["rms_after"].append(float(np.sqrt((N * r * r).sum() / total)) if total else 0.0)
    return gains, report


def solve_gains(count, sums, *, prior=None, min_overlap=None) -> np.ndarray:
    """float64 [V,3]: the gain of every camera and channel that makes the pairs of pair_stats agree, on the host in numpy float64.
    Per channel c, in the log domain: N_ij = count[i][j] for i != j, 0 where it is below min_overlap or where sums[i][j][c] or
    sums[j][i][c] is not positive; d_ij = log(sums[i][j][c]) - log(sums[j][i][c]), the log ratio of the two cameras' means over the
    texels they share; l minimises E(l) = sum_{i<j} N_ij (l_i - l_j + d_ij)^2 + prior sum_i n_i l_i^2 with n_i = sum_j N_ij, that
    is A l = b with A_ii = (1 + prior) n_i, A_ij = -N_ij, b_i = -sum_j N_ij d_ij; a camera with n_i = 0 keeps l_i = 0.  The gain is
    exp(l).  The prior only fixes the common factor every connected group of cameras is free in, at about 1.  SOLVE_DEFAULTS (None)
    are conventional choices, not tuned on a capture."""
    return _solve(count, sums, prior, min_overlap)[0]


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
    dev = _lib.hip_device(device if device is not None else (vertices.device if vertices.is_cuda else None), "the mesh renderer", ValueError)
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


def uv_islands(face_obj) -> np.ndarray:
    """int64 [n_uv]: the UV island of every UV vertex (host).  The islands are the connected components of the triangulated
    uv_faces over shared UV-vertex indices, numbered from 1 in the order of each component's lowest face index; 0 for a UV vertex
    no face names.  More than 255 islands (a label is a uint8) is a ValueError."""
    from . import meshrender
    _, uv_tris = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
    n_uv = len(face_obj.uvs)
    if uv_tris.size and (uv_tris.min() < 0 or uv_tris.max() >= n_uv):
        raise ValueError(f"uv_faces name UV vertex {int(uv_tris.max())} but the mesh has {n_uv}")
    parent = list(range(n_uv))

    def root(a: int) -> int:
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b, c in uv_tris.tolist():
        ra = root(a)
        for other in (b, c):
            ro = root(other)
            if ro != ra:
                parent[ro] = ra
    number, ids = {}, np.zeros(n_uv, np.int64)
    for a, _, _ in uv_tris.tolist():                           # in face order: a component is numbered when its first face comes
        r = root(a)
        if r not in number:
            number[r] = len(number) + 1
    if len(number) > 255:
        raise ValueError(f"the UV layout has {len(number)} islands; island_labels holds at most 255")
    for v in np.unique(uv_tris).tolist():
        ids[v] = number[root(v)]
    return ids


def island_labels(face_obj, h: int, w: int, device=None) -> torch.Tensor:
    """uint8 [h,w]: the uv_islands number of the island every texel belongs to, 0 where texfinish.coverage_from_obj is 0.  The
    numbers are rasterised by texture.render_colors as a vertex attribute: one constant per island, which the interpolation gives
    back to within rounding, so the nearest integer is exact."""
    from . import meshrender, texfinish, texture
    h, w = _size((h, w))
    ids = uv_islands(face_obj)                                 # argument errors first, with or without a device
    dev = _lib.hip_device(device, "the mesh renderer", ValueError)
    _, uv_tris = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
    uv_verts = texture.process_uv(face_obj.uvs, h, w)
    img = texture.render_colors(uv_verts, uv_tris, ids.astype(np.float32)[:, None], h, w, c=1, device=dev)
    labels = torch.round(img[..., 0]).clamp_(0, 255).to(torch.uint8)
    return torch.where(texfinish.coverage_from_obj(face_obj, h, w, device=dev) != 0, labels, torch.zeros_like(labels))


def _size_groups(dataset) -> dict:
    groups = {}
    for k, e in enumerate(dataset):
        groups.setdefault((int(e["cam"].image_height), int(e["cam"].image_width)), []).append(k)
    return groups


def _frame_inputs(face_obj, vertices: torch.Tensor, dataset, res, device):
    """(pos, nrm, coverage, groups) of one frame: surface_maps' texel maps and, one image size after the other, (the entries' indices
    in `dataset`, their cams, their photographs [v,3,H,W] float32, their depth maps): the mesh is rendered once per size for the
    depth (meshrender.MeshRenderer over a 1x1 dummy texture)."""
    from . import meshrender
    faces, uv_faces = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
    dev = _lib.hip_device(device if device is not None else (vertices.device if vertices.is_cuda else None), "the mesh renderer", ValueError)
    renderer = meshrender.MeshRenderer(faces, uv_faces, face_obj.uvs, np.zeros((1, 1, 3), np.uint8), device=dev)

    def groups():
        for ks in _size_groups(dataset).values():
            cams = [dataset[k]["cam"] for k in ks]
            yield ks, cams, torch.stack([dataset[k]["im"] for k in ks]).to(torch.float32), renderer.render(vertices, cams)[1]

    return (*surface_maps(face_obj, vertices, res, device=dev), groups())


def _blend(a, b):
    """(color, weight) of two weighted blends as one: the weighted sums add up"""
    ws = a[1] + b[1]
    mixed = (a[0] * a[1][..., None] + b[0] * b[1][..., None]) / ws.clamp_min(torch.finfo(torch.float32).tiny)[..., None]
    return torch.where((ws > 0)[..., None], mixed, torch.zeros_like(mixed)), ws


def _keep_larger(a, b):
    """(value, weight) per texel of the one with the larger weight: a, the earlier size, on ties"""
    take = b[1] > a[1]
    return torch.where(take[..., None], b[0], a[0]), torch.where(take, b[1], a[1])


def _reject_options(reject, n_views: int):
    """None, or the checked consist options of project_frame's `reject`; ValueError for anything else"""
    if reject is None:
        return None
    if not isinstance(reject, dict) or set(reject) - set(CONSIST_DEFAULTS):
        raise ValueError(f"reject must be a dict of {', '.join(CONSIST_DEFAULTS)}, got {reject!r}")
    if n_views > MAX_STAT_VIEWS:
        raise ValueError(f"at most {MAX_STAT_VIEWS} views can be checked for consistency, got {n_views}")
    return check_consist_options(**reject)


def rejected_count(skip: torch.Tensor) -> torch.Tensor:
    """uint8 [h,w]: the number of views consistency rejects at each texel, the set bits of skip"""
    bits = skip.to(torch.int64) & 0xFFFFFFFF
    n = torch.zeros_like(skip, dtype=torch.uint8)
    for i in range(MAX_STAT_VIEWS):
        n += ((bits >> i) & 1).to(torch.uint8)
    return n


def frame_consistency(face_obj, vertices: torch.Tensor, dataset, res, *, gains=None, device=None, **options):
    """consistency of one frame over _frame_inputs' maps and depth renders: (skip, votes), bit v of skip for entry v of `dataset`
    whatever the image sizes are (the views go in size group after size group, and the bits are put back).  gains
    [len(dataset),3] in the order of `dataset`.  options: consistency's (reject_tol, vote_cos_min, min_votes, power, cos_min,
    fade_px, depth_tol)."""
    check_options(**{k: v for k, v in options.items() if k not in CONSIST_DEFAULTS})
    _reject_options({k: v for k, v in options.items() if k in CONSIST_DEFAULTS}, len(dataset))
    if not dataset:
        raise ValueError("frame_consistency: no views")
    gains = _gains(gains, len(dataset))
    pos, nrm, cov, groups = _frame_inputs(face_obj, vertices, dataset, res, device)
    groups = list(groups)
    order = [k for ks, *_ in groups for k in ks]
    skip, votes = consistency(pos, nrm, cov, [g[1:] for g in groups], gains=None if gains is None else gains[order], **options)
    if order != sorted(order):                                 # several sizes: back from group order to dataset order
        bits, back = skip.to(torch.int64) & 0xFFFFFFFF, torch.zeros_like(skip, dtype=torch.int64)
        for i, k in enumerate(order):
            back |= ((bits >> i) & 1) << k
        skip = torch.where(back >= 2 ** 31, back - 2 ** 32, back).to(torch.int32)
    return skip, votes


def project_frame(face_obj, vertices: torch.Tensor, dataset, res, *, power=None, cos_min=None, fade_px=None, depth_tol=None, mode=None,
                  gains=None, device=None, band_radius: int = 8, reject=None, register=None):
    """(texture [h,w,3] uint8, weight [h,w] float32, count [h,w] uint8) of one frame: `dataset` holds ingest.get_dataset's entries
    ("cam", "im"), vertices [N,3] the mesh in the training world frame.  _frame_inputs gives the texel maps and the depth maps,
    project gathers, texfinish.quantize rounds as the PNG encoder does.  Views of one size go in one launch; a rig with several
    sizes (turned cameras) is merged per size: weighted sums add up, "best" keeps the larger weight, the earlier size on ties.
    gains [len(dataset),3] (None: none): one row per entry of `dataset`, in its order.  mode "twoband": per size low_band
    (band_radius) and project_bands; the low bands merge as "weighted" does, the detail by the larger best weight (the earlier size
    on ties), and the texture is their sum, one float32 addition, clamped to [0, 1] (where the views disagree the sum overshoots,
    and the quantisation wraps).  reject (None: no check): a dict of consistency's options (reject_tol, vote_cos_min, min_votes; {}
    for CONSIST_DEFAULTS), at most 32 views: consistency runs first over all sizes at once, with the gains, and every size's
    projection takes its part of the mask, in every mode.  The order is equalise, reject, blend, fill.  With "twoband" the low bands
    are still made from every photograph; the mask decides which views enter the two blends and which may be the best view.
    count is then the number of views that contributed.  register (None: no registration): a dict of view_flows' options (block,
    stride, radius, ratio, reach) and rounds (1..3, default 1), {} for REGISTER_DEFAULTS: the views of the frame are registered
    against their consensus before they are blended (Eisemann et al., "Floating Textures").  The frame is projected once in mode
    "weighted", with the gains and the mask; that texture's holes are filled island by island (texfinish.fill_islands over
    island_labels: a black hole would be an edge to match against); MeshRenderer.render puts it into every camera (mapping
    "bilinear"); view_flows registers every size's photographs against these renders; and the requested mode is projected with the
    flows.  With rounds > 1 the registered "weighted" projection is the next round's consensus.  The order is equalise, reject,
    register, blend, fill.  Known limits: view_flows'; consistency and pair_stats still sample unregistered, so the mask and the
    gains come from unregistered samples; the defaults are conventional, not tuned on a capture."""
    return _project_frame(face_obj, vertices, dataset, res, dict(power=power, cos_min=cos_min, fade_px=fade_px, depth_tol=depth_tol, mode=mode),
                          gains, device, band_radius, reject, register)[:3]


def _project_frame(face_obj, vertices, dataset, res, options: dict, gains, device, band_radius, reject, register=None) -> tuple:
    """project_frame, as a fourth result the mask of consistency (group order; None without `reject`) and as a fifth what the
    registration found (None without `register`): dict(order: the entries of `dataset` in group order, flows and support: view_flows'
    per size group, report: view_flows' entries in the order of `dataset`)"""
    from . import meshrender, texfinish
    o = check_options(**options)
    mode, rule = o["mode"], {k: v for k, v in o.items() if k != "mode"}
    check_band_options(band_radius)
    if not dataset:
        raise ValueError("project_frame: no views")
    gains = _gains(gains, len(dataset))
    reject = _reject_options(reject, len(dataset))
    register = check_register_options(register)
    pos, nrm, cov, groups = _frame_inputs(face_obj, vertices, dataset, res, device)
    skip = None
    if reject is not None or register is not None:
        groups = list(groups)
        order = [k for ks, *_ in groups for k in ks]
    if reject is not None:                                     # every size at once: a texel's voters come from all of them
        skip, _ = consistency(pos, nrm, cov, [g[1:] for g in groups], gains=None if gains is None else gains[order], **reject, **rule)

    def blend(mode, flows):
        """(texture uint8, weight, count) of the groups in `mode`, group i sampled through flows[i] (flows None: none)"""
        total = detail = count = None
        base = 0
        for i, (ks, cams, photos, depth) in enumerate(groups):
            g = None if gains is None else gains[ks]
            mask = {} if skip is None else dict(skip=skip, skip_base=base)      # the group's views are bits base .. base + len(ks) - 1
            base += len(ks)
            moved = {} if flows is None else dict(flows=flows[i])
            if mode == "twoband":
                color, weight, n, high, best = project_bands(pos, nrm, cov, cams, photos, low_band(photos, depth, band_radius), depth, gains=g,
                                                             **mask, **moved, **rule)
                detail = (high, best) if detail is None else _keep_larger(detail, (high, best))
            else:
                color, weight, n = project(pos, nrm, cov, cams, photos, depth, mode=mode, gains=g, **mask, **moved, **rule)
            if total is None:
                total, count = (color, weight), n
            else:
                total, count = (_keep_larger if mode == "best" else _blend)(total, (color, weight)), count + n
        color, weight = total
        if detail is not None:                                 # the sum of two bands can leave [0, 1], and quantize wraps as numpy's cast does
            color = (color + detail[0]).clamp_(0.0, 1.0)
        return texfinish.quantize(color), weight, count

    if register is None:
        return (*blend(mode, None), skip, None)
    vf = {k: v for k, v in register.items() if k != "rounds"}
    h, w = int(pos.shape[0]), int(pos.shape[1])
    labels = island_labels(face_obj, h, w, device=pos.device)
    faces, uv_faces = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
    flows = None
    for _ in range(register["rounds"]):
        tex, _, n = blend("weighted", flows)                   # the consensus: at first unregistered, then the registered one
        tex, _ = texfinish.fill_islands(tex, (n > 0).to(torch.uint8), labels)
        renderer = meshrender.MeshRenderer(faces, uv_faces, face_obj.uvs, tex, device=pos.device)
        found = [view_flows(renderer.render(vertices, cams, mapping="bilinear")[0], photos, depth, **vf) for _, cams, photos, depth in groups]
        flows = [f for f, _, _ in found]
    by_view = dict(zip(order, (r for _, _, rep in found for r in rep)))
    found = dict(order=order, flows=flows, support=[s for _, s, _ in found], report=[by_view[k] for k in range(len(dataset))])
    return (*blend(mode, flows), skip, found)


def frame_stats(face_obj, vertices: torch.Tensor, dataset, res, *, out=None, device=None, **options):
    """pair_stats of one frame, its views numbered as in `dataset`, over _frame_inputs' maps and depth renders.  out: the statistics
    of earlier frames of the same cameras, added to.  options: pair_stats' (stat_cos_min, stat_lo, stat_hi, power, cos_min, fade_px,
    depth_tol)."""
    check_options(**{k: v for k, v in options.items() if k not in STAT_DEFAULTS})
    check_stat_options(**{k: v for k, v in options.items() if k in STAT_DEFAULTS})
    if not dataset:
        raise ValueError("frame_stats: no views")
    if len(dataset) > MAX_STAT_VIEWS:
        raise ValueError(f"at most {MAX_STAT_VIEWS} views can be equalised, got {len(dataset)}")
    pos, nrm, cov, groups = _frame_inputs(face_obj, vertices, dataset, res, device)
    groups = list(groups)
    order = [k for ks, *_ in groups for k in ks]
    count, sums = pair_stats(pos, nrm, cov, [g[1:] for g in groups], **options)
    if order != sorted(order):                                 # several sizes: back from group order to dataset order
        back = torch.tensor(np.argsort(order), device=pos.device)
        count, sums = count[back][:, back], sums[back][:, back]
    if out is not None:
        out[0].add_(count)
        out[1].add_(sums)
        return out
    return count.contiguous(), sums.contiguous()


def estimate_gains(face_obj, vertices: torch.Tensor, dataset, res, *, prior=None, min_overlap=None, device=None, **options):
    """(gains float64 [len(dataset),3], report) of one frame: frame_stats, then solve_gains.  options: frame_stats's.  report:
    per channel the number of camera pairs used ("pairs"), the count-weighted rms of the pairs' log ratios d_ij as the cameras come
    ("rms_before") and of l_i - l_j + d_ij with the gains applied ("rms_after")."""
    check_solve_options(prior, min_overlap)
    count, sums = frame_stats(face_obj, vertices, dataset, res, device=device, **options)
    return _solve(count, sums, prior, min_overlap)


def write_gains(path: str, names, gains, report: dict = None, options: dict = None) -> None:
    """proj_gains.json: {"cameras": names, "gains": [[r, g, b] per camera], "report", "options"}"""
    names = [str(n) for n in names]
    g = _gains(gains, len(names))
    if len(set(names)) != len(names):
        raise ValueError("write_gains: camera names must be distinct")
    with open(path, "w") as f:
        json.dump({"cameras": names, "gains": [[float(x) for x in row] for row in g], "report": report or {}, "options": options or {}},
                  f, indent=1)
        f.write("\n")


def read_gains(path: str, names=None):
    """float64 [len(names),3]: the gains of proj_gains.json for the cameras `names`, matched by name; a camera the file does not
    hold is a ValueError.  names None: (the file's names, its gains)."""
    with open(path) as f:
        doc = json.load(f)
    try:
        held = [str(n) for n in doc["cameras"]]
        g = _gains(np.asarray(doc["gains"], dtype=np.float64).reshape(len(held), 3), len(held))
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f"{path}: not a gains file ({e})") from None
    if names is None:
        return held, g
    row = {n: k for k, n in enumerate(held)}
    missing = [str(n) for n in names if str(n) not in row]
    if missing:
        raise ValueError(f"{path}: no gains for camera(s) {', '.join(missing)}")
    return g[[row[str(n)] for n in names]]


def _names(dataset) -> list:
    return [e["cam_name"] for e in dataset]


def write_frame(frame_dir, face_obj, trans_g, dataset, res, options: dict, pad: int = 0, sizes=(), save_weight: bool = False,
                device=None, gains=None, fill: bool = False, save_rejected: bool = False, register=None, save_flows: bool = False) -> list:
    """One frame's face_proj.png (and face_proj_<size>.png, face_proj_weight.png) in `frame_dir`, from the face.obj read there:
    what the command line and train --tex_project both call.  Returns the files written.  The gutter of `pad` texels is filled
    from the texels some view contributed to (count > 0), through texfinish.finish.  gains: None, or
    {camera name: [r, g, b]} holding every camera of `dataset`.  fill: the texels of an island that no view contributed to take the
    push-pull interpolation of that island's projected texels (texfinish.fill_islands over island_labels) and count as projected
    for the gutter and the smaller levels; face_proj_weight.png is unchanged, so its zeros inside an island mark what was filled.
    Consistency options among `options` (reject_tol, vote_cos_min, min_votes: what _check_args merges under --reject) switch the
    photo-consistency check on (project_frame's reject); save_rejected then also writes face_proj_rejected.png, the 8-bit number
    of rejected views per texel.  register (None: no registration): project_frame's; the frame then also gets
    face_proj_register.json, {"options", "cameras", "report": view_flows' entry per camera}, and with save_flows face_proj_flows.npz:
    per image size "cameras_<H>x<W>", "flows_<H>x<W>" int16 [v,H,W,2] and "support_<H>x<W>" uint8 [v,H,W].  Without register every
    file is what it was."""
    from . import texfinish
    from .evaluate import training_vertices
    from .png import write_png
    reject = {k: v for k, v in options.items() if k in CONSIST_DEFAULTS} or None
    options = {k: v for k, v in options.items() if k not in CONSIST_DEFAULTS}
    if save_rejected and reject is None:
        raise ValueError("save_rejected needs the consistency options: nothing is rejected without them")
    register = check_register_options(register)
    if save_flows and register is None:
        raise ValueError("save_flows needs register: there are no flows without it")
    dev = torch.device(device if device is not None else "cuda")
    verts = torch.from_numpy(training_vertices(face_obj.vertices, trans_g)).to(dev)
    if gains is not None:
        missing = [n for n in _names(dataset) if n not in gains]
        if missing:
            raise ValueError(f"no gains for camera(s) {', '.join(missing)}")
        gains = np.asarray([gains[n] for n in _names(dataset)], dtype=np.float64)
    band_radius = options.pop("band_radius", BAND_DEFAULTS["band_radius"])
    tex, _, count, skip, found = _project_frame(face_obj, verts, dataset, res, options, gains, dev, band_radius, reject, register)
    seen = (count > 0).to(torch.uint8)
    if fill:
        tex, filled = texfinish.fill_islands(tex, seen, island_labels(face_obj, tex.shape[0], tex.shape[1], device=dev))
        seen |= filled
    levels = texfinish.finish(tex, seen, pad=pad, erode=0, sizes=sizes)
    written = texfinish.write_levels(os.path.join(frame_dir, FILE_NAME), levels)
    if save_weight:
        path = os.path.join(frame_dir, WEIGHT_NAME)
        write_png(path, count)
        written.append(path)
    if save_rejected:
        path = os.path.join(frame_dir, REJECTED_NAME)
        write_png(path, rejected_count(skip))
        written.append(path)
    if register is not None:
        names = _names(dataset)
        path = os.path.join(frame_dir, REGISTER_NAME)
        with open(path, "w") as f:
            json.dump({"options": register, "cameras": [str(n) for n in names], "report": found["report"]}, f, indent=1)
            f.write("\n")
        written.append(path)
        if save_flows:
            arrays, at = {}, 0
            for flows, support in zip(found["flows"], found["support"]):
                v, size = int(flows.shape[0]), f"{int(flows.shape[1])}x{int(flows.shape[2])}"
                arrays["cameras_" + size] = np.asarray([str(names[k]) for k in found["order"][at:at + v]])
                arrays["flows_" + size], arrays["support_" + size] = flows.cpu().numpy(), support.cpu().numpy()
                at += v
            path = os.path.join(frame_dir, FLOWS_NAME)
            np.savez_compressed(path, **arrays)
            written.append(path)
    return written


# ---- command line ----------------------------------------------------------------------------------------------------------
def _add_flags(p: argparse.ArgumentParser, suppress: bool, defaults: dict, helps, prefix: str = "", **more) -> None:
    """One flag --<prefix><key> per entry of `defaults`, of the default's type, with its help text; `more`: further add_argument
    arguments per key.  suppress (train's parser): absent from the parse unless given."""
    for (k, v), text in zip(defaults.items(), helps):
        p.add_argument(f"--{prefix}{k}", type=type(v), default=argparse.SUPPRESS if suppress else v, help=text, **more.get(k, {}))


def _flags_of(args, defaults: dict, prefix: str = "") -> dict:
    return {k: getattr(args, prefix + k, v) for k, v in defaults.items()}


def add_options(p: argparse.ArgumentParser, suppress: bool = False) -> None:
    """The four parameters and --mode, on the parser of this module and (suppress=True) of train."""
    _add_flags(p, suppress, DEFAULTS, (
        f"Projection: weight = cos^power, 0..{MAX_POWER} (default 2).",
        "Projection: drop a view whose viewing direction makes a cosine below this with the normal (default 0.1).",
        "Projection: fade a view's weight over this many pixels towards the image edge; 0: no fade (default 16).",
        "Projection: relative slack of the occlusion test against the mesh's depth map (default 0.002).",
        "Projection: blend the views that see a texel by their weights, keep the best one, or blend the photographs' "
        "low band and take the detail from the best view (default weighted)."), mode=dict(choices=MODES))


def options_of(args) -> dict:
    return _flags_of(args, DEFAULTS)


def add_band_options(p: argparse.ArgumentParser, suppress: bool = False) -> None:
    """The parameter of --mode twoband, beside add_options' on both parsers."""
    _add_flags(p, suppress, BAND_DEFAULTS, (
        f"With --mode twoband: the low band is the photograph's mean over a box of 2R+1 pixels, 0..{MAX_BAND_RADIUS} (default 8).",),
        band_radius=dict(metavar="R"))


def band_options_of(args) -> dict:
    return _flags_of(args, BAND_DEFAULTS)


def add_eq_options(p: argparse.ArgumentParser, suppress: bool = False) -> None:
    """The parameters of the equalisation, beside add_options' on both parsers."""
    _add_flags(p, suppress, STAT_DEFAULTS, (
        "Equalisation: a view's texel counts when the cosine between normal and viewing direction is at least this (default 0.5).",
        "Equalisation: leave out samples with a channel below this: black follows no gain (default 0.02).",
        "Equalisation: leave out samples with a channel above this: clipped (default 0.98)."))
    _add_flags(p, suppress, SOLVE_DEFAULTS, (
        "Equalisation: weight of the pull of every gain towards 1, which fixes the common factor (default 0.01).",
        "Equalisation: ignore a pair of cameras that shares fewer texels than this (default 64)."), prefix="eq_")


def eq_options_of(args) -> Tuple[dict, dict]:
    """(the stat_* options of pair_stats, the options of solve_gains) of a parse, checked"""
    stat, solve = _flags_of(args, STAT_DEFAULTS), _flags_of(args, SOLVE_DEFAULTS, "eq_")
    try:
        check_stat_options(**stat)
        check_solve_options(**solve)
    except ValueError as e:
        raise SystemExit(f"equalisation options: {e}") from None
    return stat, solve


def add_consist_options(p: argparse.ArgumentParser, suppress: bool = False) -> None:
    """The parameters of the photo-consistency check (--reject here, --tex_reject on train's parser), beside add_options' on both."""
    _add_flags(p, suppress, CONSIST_DEFAULTS, (
        f"Consistency: reject a view whose sample differs from the median of the facing views by more than this in some channel, "
        f"0..{MAX_REJECT_TOL:g} in colour units (default 0.1, a conventional choice).",
        "Consistency: a view votes for the median when the cosine between normal and viewing direction is at least this (default 0.5).",
        f"Consistency: reject nothing at a texel with fewer voters than this, 2..{MAX_STAT_VIEWS} (default 3)."),
        reject_tol=dict(metavar="T"), vote_cos_min=dict(metavar="C"), min_votes=dict(metavar="N"))


def consist_options_of(args) -> dict:
    return _flags_of(args, CONSIST_DEFAULTS)


def add_register_options(p: argparse.ArgumentParser, suppress: bool = False) -> None:
    """The parameters of the registration (--register here, --tex_register on train's parser), beside add_options' on both."""
    helps = dict(
        block="Registration: side of the matched blocks in pixels of the photograph, even, 8..64 (default 32).",
        stride="Registration: distance between blocks, 1..block (default block / 2).",
        radius="Registration: the largest misregistration searched for, in pixels, 0..16 (default 4); a larger one is dropped, not corrected.",
        ratio="Registration: keep a block whose best cost is at most this times the second best, in (0, 1] (default 0.8).",
        reach="Registration: a kept block's flow reaches this many strides, 1..4 (default 1).",
        rounds=f"Registration: rounds, each against the consensus the one before registered, 1..{MAX_REG_ROUNDS} (default 1).")
    metavar = dict(block="B", stride="S", radius="R", ratio="Q", reach="K", rounds="N")
    for k, v in REGISTER_DEFAULTS.items():
        p.add_argument(f"--reg_{k}", type=float if k == "ratio" else int, default=argparse.SUPPRESS if suppress else v, metavar=metavar[k],
                       help=helps[k])


def register_options_of(args):
    """None without --register (train: --tex_register), else project_frame's `register` of a parse, checked: SystemExit for what
    it would refuse"""
    if not (getattr(args, "register", False) or getattr(args, "tex_register", False)):     # (this module's flag, train's flag)
        return None
    try:
        return check_register_options(_flags_of(args, REGISTER_DEFAULTS, "reg_"))
    except ValueError as e:
        raise SystemExit(f"registration options: {e}") from None


def check_frame_views(dataset, options: dict) -> None:
    """SystemExit when `options` (of _check_args) ask for the consistency check and the frame holds more views than its mask"""
    if any(k in options for k in CONSIST_DEFAULTS) and len(dataset) > MAX_STAT_VIEWS:
        raise SystemExit(f"consistency: at most {MAX_STAT_VIEWS} views can be checked, the frame has {len(dataset)}")


class GainEstimator:
    """The gains of a run: add(face_obj, trans_g, dataset) gathers one frame's statistics, finish(path) solves, writes
    proj_gains.json and returns {camera name: gain}.  Every frame must hold the same cameras in the same order."""

    def __init__(self, res, options: dict, stat: dict, solve: dict, device=None):
        self.res, self.options, self.stat, self.solve, self.dev = res, dict(options), dict(stat), dict(solve), device
        self.names, self.out, self.frames = None, None, 0

    def add(self, face_obj, trans_g, dataset) -> None:
        from .evaluate import training_vertices
        dev = torch.device(self.dev if self.dev is not None else "cuda")
        if self.names is None:
            self.names = _names(dataset)
        elif self.names != _names(dataset):
            raise ValueError(f"the frames to equalise over hold different cameras: {self.names} and {_names(dataset)}")
        verts = torch.from_numpy(training_vertices(face_obj.vertices, trans_g)).to(dev)
        rule = {k: v for k, v in self.options.items() if k in DEFAULTS and k != "mode"}     # (mode and band_radius are project_frame's)
        self.out = frame_stats(face_obj, verts, dataset, self.res, out=self.out, device=dev, **rule, **self.stat)
        self.frames += 1

    def finish(self, path: str) -> dict:
        if self.out is None:
            raise ValueError("no frame to estimate the gains from")
        gains, report = _solve(self.out[0], self.out[1], **self.solve)
        report["frames"] = self.frames
        write_gains(path, self.names, gains, report, {**self.options, **self.stat, **self.solve})
        return dict(zip(self.names, gains.tolist()))


def load_gains(path: str) -> dict:
    """{camera name: gain} of a proj_gains.json"""
    names, g = read_gains(path)
    return dict(zip(names, g.tolist()))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.projtex",
                                description="Project the capture photographs into every frame's UV texture: face_proj.png.")
    _run.add_run_flags(p, "exp", "seq", "input_dir", "dense_input_dir", "output_dir", "down_ratio", "tex_res",
                       frames_help="Frames to project: '1-10', '1,5,9' (default: every frame directory).")
    p.add_argument("--views", type=_run.view_list, default=None,
                   help="Cameras to project, comma-separated (default: the cameras training uses).")
    p.add_argument("--set", choices=("low", "dense"), default="dense",
                   help="Photographs to project: the texture inputs (-did, the default) or the geometry inputs (-id).")
    p.add_argument("--undistort", action="store_true",
                   help="Undistort the photographs by the lens calibration of cameras.xml, as topo4d_amd.train --undistort does.")
    add_options(p)
    add_band_options(p)
    p.add_argument("--equalize", action="store_true",
                   help="Equalise the cameras' exposure and white balance: estimate one gain per camera and channel, write "
                        "proj_gains.json into the run directory and project every frame with these gains.")
    p.add_argument("--equalize_frames", type=_run.frame_list, default=None,
                   help="With --equalize: the frames the statistics are gathered over (default: the first frame projected).")
    p.add_argument("--gains", default=None, metavar="FILE", help="Project with the gains of a saved proj_gains.json instead of estimating.")
    add_eq_options(p)
    p.add_argument("--tex_pad", type=int, default=0, metavar="R",
                   help="Fill a gutter of R texels (0..64) round the projected texels (texfinish.finish).")
    p.add_argument("--tex_sizes", type=_run.size_list, default=[],
                   help="Smaller levels to write too, comma-separated, each tex_res / 2^k: face_proj_<size>.png.")
    p.add_argument("--save_weight", action="store_true", help="Also write %%06d/face_proj_weight.png: the number of views per texel.")
    p.add_argument("--tex_fill", action="store_true",
                   help="Fill the texels of every UV island that no view sees by push-pull from the island's projected texels "
                        "(texfinish.fill_islands); the gutter and the smaller levels are then built from the filled texture.")
    p.add_argument("--reject", action="store_true",
                   help="Leave a view out of a texel where it disagrees with the median of the views that face it: specular "
                        "highlights, occlusion leaks, content only one camera holds (at most 32 views; after the equalisation, before the blend).")
    add_consist_options(p)
    p.add_argument("--save_rejected", action="store_true",
                   help="With --reject: also write %%06d/face_proj_rejected.png, the number of rejected views per texel.")
    p.add_argument("--register", action="store_true",
                   help="Register every view to the blend of all views before it is projected: a small 2D flow per view, found by "
                        "block matching against the weighted texture rendered into the camera (after --reject, before the blend); "
                        "also writes %%06d/face_proj_register.json.")
    add_register_options(p)
    p.add_argument("--save_flows", action="store_true",
                   help="With --register: also write %%06d/face_proj_flows.npz, every view's flow (1/256 px) and its support.")
    return p


def _check_args(args, res: int) -> dict:
    from . import texfinish
    opts, band, consist = options_of(args), band_options_of(args), consist_options_of(args)
    reject = getattr(args, "reject", False) or getattr(args, "tex_reject", False)     # (this module's flag, train's flag)
    try:
        check_options(**opts)
        check_band_options(**band)
        if reject:
            check_consist_options(**consist)
        texfinish.check_options(getattr(args, "tex_pad", 0), 0, getattr(args, "tex_sizes", ()), res)
    except ValueError as e:
        raise SystemExit(f"projection options: {e}") from None
    # (the band radius and the consistency options only when they act: the options are recorded in proj_gains.json, and
    # write_frame takes the presence of the latter for the switch)
    return {**opts, **(band if opts["mode"] == "twoband" else {}), **(consist if reject else {})}


def project_tree(args, device=None) -> list:
    """The files written for the run <od>/<exp>/<seq>; frames without face.obj or without views are left alone."""
    from . import cameras as C, ingest
    dev = torch.device(device if device is not None else "cuda")
    run_dir = _run.run_dir_of(args)
    opts = _check_args(args, args.tex_res)
    save_rejected = getattr(args, "save_rejected", False)
    if save_rejected and not getattr(args, "reject", False):
        raise SystemExit("--save_rejected writes what the consistency check rejects: it needs --reject")
    register, save_flows = register_options_of(args), getattr(args, "save_flows", False)
    if save_flows and register is None:
        raise SystemExit("--save_flows writes what the registration finds: it needs --register")
    equalize, gains_file = getattr(args, "equalize", False), getattr(args, "gains", None)
    if equalize and gains_file:
        raise SystemExit("--equalize estimates the gains and --gains reads them: give one of the two")
    stat, solve = eq_options_of(args)
    cameras, trans_g, lenses, data_dir, _, skip = _run.select_cameras(args, args.set, absent="trained")    # the cameras training uses
    frames = _run.frames_of(args, run_dir)
    written = []

    def read_obj(t):
        return _run.read_frame_obj(_run.frame_dir(run_dir, t))

    with torch.cuda.device(dev):
        pf = ingest.FramePrefetcher(data_dir, args.seq, cameras, use_mask=False, blacklist=skip, rotate_mask=C.ROTATE_MASK,
                                    setup_camera=functools.partial(C.setup_camera, device=dev), device=dev, lenses=lenses)
        try:
            gains = None
            try:
                if gains_file:
                    gains = load_gains(gains_file)
                elif equalize:
                    est = GainEstimator(args.tex_res, opts, stat, solve, device=dev)
                    for t in getattr(args, "equalize_frames", None) or frames:
                        obj, dataset = read_obj(t), pf.get(t)
                        if obj is None or not dataset:
                            continue
                        est.add(obj, trans_g, dataset)
                        if not getattr(args, "equalize_frames", None):
                            break                                  # the first frame that can be projected
                    gains = est.finish(os.path.join(run_dir, GAINS_NAME))
                    written.append(os.path.join(run_dir, GAINS_NAME))
            except (OSError, ValueError) as e:
                raise SystemExit(f"equalisation: {e}") from None
            with _run.prefetched(frames, read_obj, ahead=pf.prefetch, thread_name="t4d-projtex") as walk:
                for t, obj in walk:
                    dataset = pf.get(t)
                    if obj is None or not dataset:
                        continue
                    if gains is not None and any(n not in gains for n in _names(dataset)):
                        raise SystemExit(f"equalisation: no gains for camera(s) {', '.join(n for n in _names(dataset) if n not in gains)}")
                    check_frame_views(dataset, opts)
                    written += write_frame(_run.frame_dir(run_dir, t), obj, trans_g, dataset, args.tex_res, opts,
                                           pad=args.tex_pad, sizes=args.tex_sizes, save_weight=args.save_weight, device=dev, gains=gains,
                                           fill=getattr(args, "tex_fill", False), save_rejected=save_rejected, register=register,
                                           save_flows=save_flows)
        finally:
            pf.close()
    return written


def main(argv=None) -> None:
    _run.print_written(project_tree(build_parser().parse_args(argv)))


if __name__ == "__main__":
    main()
