"""
A whole Topo4D capture sequence from one entry point - train.py:590-755 on the fused MI355X pieces:

    python -m topo4d_amd.train -s seq_01 -id <low-res views> -did <full-res views> -od <results> -t

writes the same output tree as the reference's `python train.py ...`: <output_dir>/<exp>/<seq>/%06d/face.obj (+ face.png with
--gen_tex), the progress renders vis<cam>_<i>.png / dense_<cam>_<i>.png, params.npz and loss.json.

    cameras            cameras.get_cameras (Metashape cameras.xml)                           train.py:595-596
    setup              coarse.initialize_params / initialize_losses, densify, TopologyPriors  train.py:597-601
    views              ingest.FramePrefetcher (GPU JPEG decode + rotation)                   train.py:653, :722
    geometry loop      loop.optimise_views: hand-chained render, loss, backward, fused priors,
                       Adam + region pins in one launch (FusedAdamPins)                       train.py:661-711
    texture loop       loop.optimise_dense_views                                             train.py:715-743
    progress           progress.report_progress[_dense] (PNG on the GPU)                     train.py:702, :742
    outputs            params2cpu / save_params / write_loss_json, objexport.save_mesh        train.py:744-755

The one deliberate difference: --log_views takes a comma-separated list of camera names (the reference's `type=list` splits
its argument into characters).  Flags the reference does not have: --undistort undistorts every photograph and mask by the
lens calibration of cameras.xml while it is loaded (cameras.get_lenses, ingest.undistort_views; the reference needs photographs
exported undistorted), and --low_from_full makes the geometry inputs from the full-size photographs as down_ratio x down_ratio
means, so that -id holds cameras.xml, the mesh and the masks only; with --gen_tex, --tex_pad R fills a gutter of R texels round
the UV islands of face.png and --tex_sizes 4096,2048 also writes face_<size>.png (texfinish.finish); --tex_project writes
face_proj.png beside every face.obj, the frame's full-size photographs projected into the UV layout (projtex, with or without
--gen_tex; --mode, --band_radius, --power, --cos_min, --fade_px and --depth_tol as python -m topo4d_amd.projtex takes them; --tex_equalize
estimates one gain per camera and channel on the first frame written, stores proj_gains.json in the run directory and projects
every frame with it; --tex_fill fills the texels of every UV island that no view sees by push-pull from the island's projected
texels, texfinish.fill_islands; --tex_reject leaves a view out of a texel where it disagrees with the median of the views that
face it, projtex.consistency, with --reject_tol, --vote_cos_min and --min_votes; --tex_register registers every view to the
blend of all views before it is projected, projtex.view_flows, with --reg_block, --reg_stride, --reg_radius, --reg_ratio, --reg_reach
and --reg_rounds).  Without them nothing changes.

The region "freezes" of train.py:676-700 are FusedAdamPins pins, written by the step kernel itself; the pin set changes at
most twice per frame (the dynamic-eye pins end at iteration int(0.7 n) of frame 0) and the learning rates once (the colour
phase of a later frame's last 99 iterations).  Both switches run between two steps of one optimise_views call, from the table
`geometry_schedule` builds, so the camera sequence is get_batch's over the whole frame.  One random.Random serves every
get_batch of the run, as the module-level `random` of the reference does.
"""
from __future__ import annotations

import argparse
import contextlib
import functools
import json
import os
import time
from random import Random
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import cameras as C
from ._run import size_list, view_list

# train.py:272-289 (initialize_optimizer)
LRS = {
    'means3D': 0.0, 'rgb_colors': 0.0025, 'unnorm_rotations': 0.001, 'logit_opacities': 0.0, 'log_scales': 0.001,
    'dense_means3D': 0.0, 'dense_unnorm_rotations': 0.001, 'dense_logit_opacities': 0.0, 'dense_log_scales': 0.0,
    'dense_rgb_colors': 0.0025,
    'cam_m': 1e-4, 'cam_c': 1e-4,
}
# train.py:606-616, :648-650: the rates of every later frame
NEW_LR = {
    'logit_opacities': 0.0, 'log_scales': 0.0, 'unnorm_rotations': 0.001, 'rgb_colors': 0.0, 'means3D': 0.000016,
    'dense_log_scales': 0.0, 'cam_m': 0.0, 'cam_c': 0.0,
}
# train.py:705-710: the colour phase of a later frame, set after the step of every iteration i >= opt_num - 100
COLOR_LR = {'rgb_colors': 0.00025, 'means3D': 0.0}
EYE_PIN_FRACTION = 0.7                        # train.py:683
USE_MASK, USE_MASK_DENSE = True, False        # train.py:631-632
_COARSE = ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales')


# ---- schedule --------------------------------------------------------------------------------------------------------------
def pin_phase(i: int, n_iters: int, is_initial_timestep: bool) -> str:
    """The pin set in force after the step of iteration i (train.py:682-700): "eye" (frame 0 with the dynamic-eye scale and
    opacity pins, i < int(0.7 n)), "first" (frame 0 without them) or "later"."""
    if not is_initial_timestep:
        return "later"
    return "eye" if i < int(n_iters * EYE_PIN_FRACTION) else "first"


def geometry_lrs(i: int, n_iters: int, is_initial_timestep: bool) -> Dict[str, float]:
    """Every group's learning rate in the step of iteration i.  Frame 0 keeps initialize_optimizer's; a later frame starts
    from NEW_LR (train.py:648-650) and takes COLOR_LR from the step AFTER iteration n_iters - 100 on (train.py:705-710)."""
    if is_initial_timestep:
        return dict(LRS)
    lrs = {**LRS, **NEW_LR}
    if i >= 1 and i - 1 >= n_iters - 100:
        lrs.update(COLOR_LR)
    return lrs


def geometry_schedule(n_iters: int, is_initial_timestep: bool) -> List[tuple]:
    """[(pin phase, learning rates)] of every iteration of one frame's geometry loop."""
    out, prev = [], None
    for i in range(n_iters):
        cur = (pin_phase(i, n_iters, is_initial_timestep), geometry_lrs(i, n_iters, is_initial_timestep))
        if prev is not None and cur == prev:
            cur = prev                                              # (one object per segment)
        out.append(cur)
        prev = cur
    return out


# ---- optimiser -------------------------------------------------------------------------------------------------------------
def initialize_optimizer(params: dict, capturable: bool = False):
    """train.py:270-297 on FusedAdamPins: one group per parameter, in the params dict's order."""
    from .optim import FusedAdamPins
    groups = [{'params': [v], 'name': k, 'lr': LRS[k]} for k, v in params.items()]
    return FusedAdamPins(groups, lr=0.0, eps=1e-15, capturable=capturable)


def update_optimizer(update_list: dict, optimizer) -> None:
    """helpers.py:801-804, pushed to the device copy of a capturable optimiser."""
    for g in optimizer.param_groups:
        if g["name"] in update_list:
            g['lr'] = update_list[g["name"]]
    optimizer.sync_hyper()


def _rows(index) -> np.ndarray:
    """Sorted distinct rows of a facial_regions index array (some hold a row twice; the reference writes equal values there)."""
    return np.unique(np.asarray(index, dtype=np.int64).reshape(-1))


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))                                  # helpers.py:22-23


class RegionPins:
    """The fixed values of train.py:619-629 and initialize_post_first_timestep (train.py:441-451), and the assignments of
    train.py:676-700 as FusedAdamPins pins, in the reference's order (a later assignment wins on the rows it shares)."""

    def __init__(self, params: dict, facial_regions: dict):
        fr = self.fr = facial_regions
        r = lambda k: _rows(fr[k])
        with torch.no_grad():
            dev = params['means3D'].device
            self.static_verts = params['means3D'][r("static_masks")].clone().detach()                  # train.py:620
            self.static_face_colors = params['rgb_colors'][r("face_masks")].clone().detach()           # :621, BEFORE :622-623
            params["rgb_colors"][r("dynamic_mouth_masks")] = 0.0                                          # train.py:622
            params["rgb_colors"][r("dynamic_eye_masks")] = 1.0                                            # train.py:623
            n = lambda k: len(r(k))
            self.dynamic_mouth_opacity = inverse_sigmoid(0.99999 * torch.ones((n("dynamic_mouth_masks"), 1))).to(dev)   # :624
            self.dynamic_mouth_scales = torch.log(torch.ones((n("dynamic_mouth_masks"), 3), device=dev) * 0.01)        # :625
            self.eye_inner_opacity = inverse_sigmoid(0.000001 * torch.ones((n("eye_inner_masks"), 1))).to(dev)         # :626
            self.mouth_inner_scales = torch.log(torch.ones((n("mouth_inner_masks"), 3), device=dev) * 0.002)          # :627
            self.dynamic_eye_scales = torch.log(torch.ones((n("dynamic_eye_masks"), 3), device=dev) * 0.0025)         # :628
            self.dynamic_eye_opacity = inverse_sigmoid(0.99999 * torch.ones((n("dynamic_eye_masks"), 1))).to(dev)      # :629
        self.first_frame = None

    def capture_first_frame(self, params: dict) -> None:
        """initialize_post_first_timestep (train.py:441-451, called at :749 after frame 0's texture loop and params2cpu)."""
        fr, rgb = self.fr, params['rgb_colors'].detach()
        self.first_frame = {
            "dynamic_eye_colors": rgb[_rows(fr["dynamic_eye_masks"])].clone(),
            "eye_around_colors": rgb[_rows(fr["eye_around_masks"])].clone(),
            "eye_bottom_colors": rgb[_rows(fr["region_masks"]["EyeLidBottom"])].clone(),
            "mouth_around_colors": rgb[_rows(fr["mouth_around_masks"])].clone(),
            "face_bottom_colors": rgb[_rows(fr["face_bottom_masks"])].clone(),
        }

    def assignments(self, phase: str) -> List[tuple]:
        """[(parameter, rows, values)] of one pin phase (pin_phase), in the order of train.py:676-700."""
        fr, r = self.fr, lambda k: _rows(self.fr[k])
        out = [('means3D', r("static_masks"), self.static_verts),                                        # train.py:676
               ('logit_opacities', r("eye_inner_masks"), self.eye_inner_opacity),                        # :677
               ('rgb_colors', r("dynamic_mouth_masks"), 0.0),                                            # :678
               ('logit_opacities', r("dynamic_mouth_masks"), self.dynamic_mouth_opacity),                # :679
               ('log_scales', r("dynamic_mouth_masks"), self.dynamic_mouth_scales),                      # :680
               ('log_scales', r("mouth_inner_masks"), self.mouth_inner_scales)]                          # :681
        if phase in ("eye", "first"):
            if phase == "eye":                                                                           # :683-686
                out += [('log_scales', r("dynamic_eye_masks"), self.dynamic_eye_scales),
                        ('logit_opacities', r("dynamic_eye_masks"), self.dynamic_eye_opacity)]
            out += [('rgb_colors', r("face_masks"), self.static_face_colors),                            # :688
                    ('rgb_colors', r("mouth_inner_masks"), 0.0)]                                         # :689
        elif phase == "later":
            if self.first_frame is None:
                raise RuntimeError("RegionPins: the later-frame pins need capture_first_frame after frame 0 (train.py:749)")
            ff = self.first_frame
            out += [('rgb_colors', r("dynamic_eye_masks"), ff["dynamic_eye_colors"]),                    # :693
                    ('rgb_colors', r("dynamic_mouth_masks"), 0.0),                                       # :694
                    ('rgb_colors', r("eye_del_masks"), 0.0),                                             # :695
                    ('rgb_colors', r("eye_around_masks"), ff["eye_around_colors"]),                      # :696
                    ('rgb_colors', _rows(fr["region_masks"]["EyeLidBottom"]), ff["eye_bottom_colors"]),  # :697
                    ('rgb_colors', r("mouth_around_masks"), ff["mouth_around_colors"]),                  # :698
                    ('rgb_colors', r("face_bottom_masks"), ff["face_bottom_colors"]),                    # :699
                    ('rgb_colors', r("mouth_inner_masks"), 0.0)]                                         # :700
        else:
            raise ValueError(f"unknown pin phase {phase!r}")
        return out

    def install(self, optimizer, phase: str) -> None:
        """Replace the geometry pins of `optimizer` by those of `phase` (rows an ended pin held fall back to the earlier ones)."""
        for name in _COARSE:
            optimizer.clear_pin(name)
        for name, rows, values in self.assignments(phase):
            optimizer.set_pin(name, rows, values)

    def dense_assignments(self) -> List[tuple]:
        """train.py:732-734: rows of dense_rgb_colors zeroed before every texture-loop render."""
        return [('dense_rgb_colors', _rows(self.fr[k]), 0.0) for k in ("static_masks", "dynamic_masks", "mouth_inner_masks")]


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def params2cpu(params: dict, is_initial_timestep: bool) -> Dict[str, np.ndarray]:
    """helpers.py:160-166: frame 0 keeps every non-dense parameter, later frames means3D, rgb_colors and unnorm_rotations."""
    if is_initial_timestep:
        keep = [k for k in params if not k.startswith("dense")]
    else:
        keep = [k for k in params if k in ('means3D', 'rgb_colors', 'unnorm_rotations')]
    return {k: params[k].detach().cpu().contiguous().numpy() for k in keep}


def save_params(output_params: List[dict], args) -> None:
    """helpers.py:169-178: <output_dir>/<exp>/<seq>/params.npz; a key every frame has is stacked over the frames, the others
    are frame 0's."""
    to_save = {}
    for k in output_params[0]:
        to_save[k] = np.stack([p[k] for p in output_params]) if k in output_params[1] else output_params[0][k]
    out = os.path.join(args.output_dir, args.exp, args.seq)
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "params"), **to_save)


def write_loss_json(dir, loss_list: dict, loss_w: dict) -> None:
    """helpers.py:826-833: <dir>/loss.json = [{term: configured}, losses_weights], written once."""
    path = os.path.join(dir, "loss.json")
    if os.path.exists(path):
        return
    with open(path, 'w') as f:
        json.dump([{k: v is not None for k, v in loss_list.items()}, loss_w], f, indent=4)


# ---- the run ---------------------------------------------------------------------------------------------------------------
class _Clock:
    """Seconds per phase when `timings` is a dict (synchronising at both ends of every span; a span's time excludes the spans
    nested in it), nothing otherwise."""

    def __init__(self, timings: Optional[dict], dev):
        self.t, self.dev, self.stack = timings, dev, []

    def _now(self) -> float:
        torch.cuda.synchronize(self.dev)
        return time.perf_counter()

    @contextlib.contextmanager
    def __call__(self, phase: str):
        if self.t is None:
            yield
            return
        self.stack.append(0.0)                                  # time spent in nested spans
        t0 = self._now()
        try:
            yield
        finally:
            total = self._now() - t0
            nested = self.stack.pop()
            self.t[phase] = self.t.get(phase, 0.0) + total - nested
            if self.stack:
                self.stack[-1] += total


def _bar(n: int, desc: str):
    from tqdm import tqdm
    return tqdm(range(n), desc=desc)


def initialize_per_timestep(params: dict, optimizer, priors) -> None:
    """train.py:420-438 in place (recorded graphs keep their addresses): the prior state of the frame from normalize(q)
    (priors.begin_frame), unnorm_rotations <- normalize(normalize(q)), and update_params_and_optimizer's reset of the Adam
    moments of means3D and unnorm_rotations, whose step counts stay (external.py:126-138)."""
    with torch.no_grad():
        priors.begin_frame(params)                                                  # train.py:421-432, from the old q
        q = params['unnorm_rotations']
        q.copy_(F.normalize(F.normalize(q)))                                        # train.py:422, :425, :434-435
        for k in ('means3D', 'unnorm_rotations'):
            st = optimizer.state.get(params[k])
            if st is None or "exp_avg" not in st:
                raise RuntimeError(f"initialize_per_timestep: {k} has no Adam state (the reference's optimizer.state.get fails too)")
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()


def update_dense_states(params: dict, variables: dict, is_init: bool) -> None:
    """train.py:498-507 in place: a later frame's soft-colour anchor is the last frame's dense colours, and its dense centres
    the interpolated coarse ones (texture.compute_vertex_attribute_by_weight on the GPU)."""
    if is_init:
        return
    from .texture import compute_vertex_attribute_by_weight
    with torch.no_grad():
        variables["dense_init_colors"].copy_(params['dense_rgb_colors'].detach())
        params["dense_means3D"].copy_(compute_vertex_attribute_by_weight(variables, params["means3D"].detach()))


def train(args, facial_regions: Optional[dict] = None, device=None, seed: int = 0,
          on_frame: Optional[Callable[[int, dict], None]] = None, timings: Optional[dict] = None):
    """train.py:590-755.  `facial_regions`: default ./assets/facial_regions.pkl (as the reference).  `seed`: of the one
    random.Random every get_batch draws from.  `on_frame(t, state)`: called at the end of every frame with state = {params,
    variables, optimizer, priors, pins, frames}.  `timings`: a dict that receives seconds per phase (setup, ingest, geometry,
    transition, texture, progress, export; synchronising at every phase boundary).  Returns that state, or None when the output directory already exists."""
    from . import _lib, coarse, ingest, loop, objexport, progress
    from .priors import TopologyPriors
    out_dir = os.path.join(args.output_dir, args.exp, args.seq)
    if os.path.exists(out_dir):                                                             # train.py:591-593
        print(f"Experiment '{args.exp}' for sequence '{args.seq}' already exists. Exiting.")
        return None
    tex_pad, tex_sizes = getattr(args, "tex_pad", 0), getattr(args, "tex_sizes", ())
    if tex_pad or len(tex_sizes):                              # a bad radius or size stops the run here, not at its first export
        from . import texfinish
        try:
            texfinish.check_options(tex_pad, 0, tex_sizes, args.tex_res)
        except ValueError as e:
            raise SystemExit(f"--tex_pad / --tex_sizes: {e}") from None
    tex_project = getattr(args, "tex_project", False)
    if tex_project:
        from . import meshrender, projtex
        proj_opts = projtex._check_args(args, args.tex_res)
    tex_equalize, proj_gains = getattr(args, "tex_equalize", False), None
    if tex_equalize:
        if not tex_project:
            raise SystemExit("--tex_equalize equalises the projected texture: it needs --tex_project")
        eq_stat, eq_solve = projtex.eq_options_of(args)
    tex_fill = getattr(args, "tex_fill", False)
    if tex_fill and not tex_project:
        raise SystemExit("--tex_fill fills the holes of the projected texture: it needs --tex_project")
    if getattr(args, "tex_reject", False) and not tex_project:
        raise SystemExit("--tex_reject rejects inconsistent views of the projected texture: it needs --tex_project")
    if getattr(args, "tex_register", False) and not tex_project:
        raise SystemExit("--tex_register registers the views of the projected texture: it needs --tex_project")
    proj_register = projtex.register_options_of(args) if tex_project else None
    dev = _lib.hip_device(device, "the coarse setup")
    clock = _Clock(timings, dev)
    with torch.cuda.device(dev), clock("setup"):
        undistort, low_from_full = getattr(args, "undistort", False), getattr(args, "low_from_full", False)
        views_dir = args.dense_input_dir if low_from_full else None          # the calibration of input_dir, the view list of this
        cameras, _, trans_g = C.get_cameras(args.input_dir, args.seq, resize_factor=args.down_ratio, views_dir=views_dir)   # train.py:595
        cameras_dense, _, trans_g = C.get_cameras(args.input_dir, args.seq, resize_factor=1, views_dir=views_dir)          # train.py:596
        lenses, lenses_dense = (None, None) if not undistort else C.get_lenses(
            args.input_dir, args.seq, args.down_ratio, views_dir=views_dir)
        params, variables = coarse.initialize_params(args, trans_g, facial_regions=facial_regions, device=dev)  # :597
        optimizer = initialize_optimizer(params)                                                           # :600
        variables, losses, loss_weights, _ = coarse.initialize_losses(variables)                           # :601
        priors = TopologyPriors.from_topo4d(variables, losses, loss_weights)
        pins = RegionPins(params, variables["facial_regions"])                                             # :619-629
        inner_mouth = C.parsing_colormap_bgr(14)[[C.CMAP_INDEX["inner_mouth"]]]                           # :633, helpers.py:806
        cam_fn = functools.partial(C.setup_camera, device=dev)
        png_decoder = "gpu" if getattr(args, "gpu_png", False) else "pil"
        if low_from_full:                  # the geometry targets are down_ratio x down_ratio means of the full-size photographs
            pf = ingest.FramePrefetcher(args.dense_input_dir, args.seq, cameras, use_mask=USE_MASK, blacklist=C.BLACKLIST,
                                        rotate_mask=C.ROTATE_MASK, setup_camera=cam_fn, device=dev, lenses=lenses_dense,
                                        supersample=args.down_ratio, mask_dir=args.input_dir, png_decoder=png_decoder)
        else:
            pf = ingest.FramePrefetcher(args.input_dir, args.seq, cameras, use_mask=USE_MASK, blacklist=C.BLACKLIST,
                                        rotate_mask=C.ROTATE_MASK, setup_camera=cam_fn, device=dev, lenses=lenses,
                                        png_decoder=png_decoder)
        pf_dense = ingest.FramePrefetcher(args.dense_input_dir, args.seq, cameras_dense, use_mask=USE_MASK_DENSE,
                                          blacklist=C.BLACKLIST, rotate_mask=C.ROTATE_MASK, setup_camera=cam_fn, device=dev,
                                          lenses=lenses_dense, png_decoder=png_decoder)
    rng = Random(seed)
    output_params = []
    state = {"params": params, "variables": variables, "optimizer": optimizer, "priors": priors, "pins": pins, "frames": 0}
    with torch.cuda.device(dev):
        try:
            for t in range(args.frame_num):                                                                # train.py:640
                first = t == 0
                n = args.init_opt_num if first else args.opt_num
                if not first:
                    with clock("transition"):
                        initialize_per_timestep(params, optimizer, priors)                               # train.py:646
                        update_optimizer(NEW_LR, optimizer)                                               # :647-650
                with clock("ingest"):
                    dataset = pf.get(t + 1)                                                               # train.py:653
                    if args.gen_tex or tex_project:
                        pf_dense.prefetch(t + 1)
                    pf.prefetch(t + 2)
                if len(dataset) == 0:                                                                     # :654-655
                    break

                # ---- geometry (train.py:658-712) ----
                schedule = geometry_schedule(n, first)
                with clock("transition"):
                    if n:
                        pins.install(optimizer, schedule[0][0])
                        update_optimizer(schedule[0][1], optimizer)
                bar = _bar(n, f"timestep geometry {t}")

                def after_step(i, dataset=dataset, schedule=schedule, bar=bar, t=t, n=n):
                    if i % args.log_freq == 0:
                        with clock("progress"):
                            progress.report_progress(params, dataset, t + 1, i, bar, every_i=args.log_freq,
                                                     idx=args.log_views, path=out_dir)              # train.py:702
                    if i + 1 < n:
                        (ph0, lr0), (ph1, lr1) = schedule[i], schedule[i + 1]
                        if ph1 != ph0:
                            pins.install(optimizer, ph1)                                          # train.py:683 ends
                        if lr1 != lr0:
                            update_optimizer(lr1, optimizer)                                      # train.py:705-710

                with clock("geometry"):
                    loop.optimise_views(params, dataset, optimizer, n, use_mask=USE_MASK, is_initial_timestep=first,
                                        label_colors=inner_mouth, max_2D_radius=variables['max_2D_radius'], priors=priors,
                                        report=after_step, rng=rng)
                if not first and n:
                    update_optimizer(geometry_lrs(n, n, False), optimizer)            # train.py:705-710 after the last step too
                bar.close()
                for name in _COARSE:
                    optimizer.clear_pin(name)

                # ---- texture (train.py:714-743) ----
                sav_tex, dense = True, None
                if args.gen_tex:
                    with clock("transition"):
                        update_dense_states(params, variables, first)                                     # train.py:720
                    with clock("ingest"):
                        dense = pf_dense.get(t + 1)                                                       # train.py:722
                        pf_dense.prefetch(t + 2)
                    n_tex = args.dense_opt_num
                    if len(dense) == 0:                                                                   # :723-725
                        n_tex, sav_tex = 0, False
                    bar = _bar(n_tex, f"timestep texture {t}")

                    def after_dense(i, dense=dense, bar=bar, t=t):
                        if i % args.dense_log_freq == 0:
                            with clock("progress"):
                                progress.report_progress_dense(variables, params, dense, t + 1, i, bar,
                                                               every_i=args.dense_log_freq, idx=args.log_views,
                                                               path=out_dir)                          # train.py:742
                    for name, rows, values in pins.dense_assignments():
                        optimizer.set_pin(name, rows, values)                                            # :732-734, before each render
                    try:
                        with clock("texture"):
                            loop.optimise_dense_views(params, variables, dense, optimizer, n_tex,
                                                      max_2D_radius=variables['dense_max_2D_radius'],
                                                      report=after_dense, rng=rng)
                    finally:
                        optimizer.clear_pin('dense_rgb_colors')       # the next frame's geometry steps must leave them alone
                    bar.close()

                with clock("export"):
                    output_params.append(params2cpu(params, first))                                      # train.py:744
                    if first:
                        pins.capture_first_frame(params)                                                 # :747-749
                    if t % args.ckp_freq == 0 and t != 0:                                                 # :751-753
                        save_params(output_params, args)
                        write_loss_json(out_dir, losses, loss_weights)
                    objexport.save_mesh(os.path.join(out_dir, "%06d" % (t + 1)), params, variables, t + 1,
                                        res=args.tex_res, gen_texture=args.gen_tex and sav_tex,          # train.py:755
                                        pad=tex_pad, sizes=tex_sizes)
                if tex_project:
                    if dense is None:
                        with clock("ingest"):
                            dense = pf_dense.get(t + 1)
                            pf_dense.prefetch(t + 2)
                    if len(dense):
                        with clock("export"):                    # from the face.obj just written: the file the command line reads
                            frame_dir = os.path.join(out_dir, "%06d" % (t + 1))
                            face_obj = meshrender.read_face_obj(os.path.join(frame_dir, "face.obj"))
                            if tex_equalize and proj_gains is None:          # the rig's gains, from the first frame written
                                est = projtex.GainEstimator(args.tex_res, proj_opts, eq_stat, eq_solve, device=dev)
                                est.add(face_obj, trans_g, dense)
                                proj_gains = est.finish(os.path.join(out_dir, projtex.GAINS_NAME))
                            projtex.check_frame_views(dense, proj_opts)
                            projtex.write_frame(frame_dir, face_obj, trans_g, dense, args.tex_res, proj_opts, pad=tex_pad,
                                                sizes=tex_sizes, device=dev, gains=proj_gains, fill=tex_fill, register=proj_register)
                state["frames"] = t + 1
                if on_frame is not None:
                    on_frame(t, state)
        finally:
            pf.close()
            pf_dense.close()
    return state


# ---- command line ----------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    """train.py:759-780: the same flags, names and defaults (--log_views: comma-separated)."""
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.train")
    p.add_argument('-e', '--exp', type=str, default='exp_op1', help="Experiment name.")
    p.add_argument('-s', '--seq', type=str, default="seq_01", help="Input sequence name.")
    p.add_argument('-id', '--input_dir', type=str, default='/data/Topo4D/videos_low',
                   help="Root of inputs, the input sequence should be '$input_dir/$seq'")
    p.add_argument('-od', '--output_dir', type=str, default='/data/Topo4D/Topo4D_results',
                   help="Root of outputs, results will be saved in '$output_dir/$exp/$seq'")
    p.add_argument('-did', '--dense_input_dir', type=str, default='/data/Topo4D/videos',
                   help="Root of high resolution inputs, the input sequence should be '$dense_input_dir/$seq'")
    p.add_argument('-fn', '--frame_num', type=int, default=800, help="Frame number.")
    p.add_argument('-t', '--gen_tex', action='store_true', help="Whether generate texture.")
    p.add_argument('-tr', '--tex_res', type=int, default=8192, help="Texture resolution.")
    p.add_argument('-dn', '--density', type=int, default=30, help="Density for uv-space densification.")
    p.add_argument('-dr', '--down_ratio', type=int, default=8,
                   help="Downsample ratio of geometry optimization inputs compared with raw captures.")
    p.add_argument('-ddr', '--dense_down_ratio', type=int, default=1,
                   help="Downsample ratio of texture optimization inputs compared with raw captures.")
    p.add_argument('-ion', '--init_opt_num', type=int, default=7000, help="Iteration number for optimizing the first frame.")
    p.add_argument('-on', '--opt_num', type=int, default=1100, help="Iteration number for geometry generation.")
    p.add_argument('-don', '--dense_opt_num', type=int, default=301, help="Iteration number for texture generation.")
    p.add_argument('-lf', '--log_freq', type=int, default=500, help="Frequence of saving gaussian rendering results per frame.")
    p.add_argument('-dlf', '--dense_log_freq', type=int, default=300,
                   help="Frequence of saving dense gaussian rendering results per frame.")
    p.add_argument('-lv', '--log_views', type=view_list, default=["K98707293"],
                   help="Views of the saved renderings, comma-separated.")
    p.add_argument('-cf', '--ckp_freq', type=int, default=5, help="Frequence of saving gaussian attributes.")
    # the flags the reference does not have stay out of the namespace unless given (read with getattr)
    p.add_argument('--undistort', action='store_true', default=argparse.SUPPRESS,
                   help="Undistort every photograph (and its mask) by the lens calibration of cameras.xml while it is loaded; "
                        "without it the photographs must have been exported undistorted.")
    p.add_argument('--low_from_full', action='store_true', default=argparse.SUPPRESS,
                   help="Make the geometry inputs from $dense_input_dir's photographs (down_ratio x down_ratio means) instead "
                        "of reading $input_dir's; $input_dir then holds cameras.xml, the mesh and the masks only.")
    p.add_argument('--gpu_png', action='store_true', default=argparse.SUPPRESS,
                   help="Decode the masks and the *.png views of $input_dir and $dense_input_dir on the GPU (topo4d_amd.png); the "
                        "kinds its decoder does not take (palette, under 8 bits, 16-bit colour, interlaced) still come from PIL.")
    p.add_argument('--tex_pad', type=int, default=argparse.SUPPRESS, metavar='R',
                   help="With --gen_tex: fill a gutter of R texels (0..64) round the UV islands of face.png from the nearest "
                        "baked texel, so that bilinear taps on the seams no longer mix in the black background.")
    p.add_argument('--tex_sizes', type=size_list, default=argparse.SUPPRESS,
                   help="With --gen_tex: texture sizes to write, comma-separated, each tex_res / 2^k: face.png holds tex_res, "
                        "face_<size>.png the others, averaged over baked texels only.")
    p.add_argument('--tex_project', action='store_true', default=argparse.SUPPRESS,
                   help="Also write face_proj.png beside every face.obj: the frame's full-size photographs projected into the UV "
                        "layout (topo4d_amd.projtex), with or without --gen_tex; --tex_pad and --tex_sizes apply to it too.")
    p.add_argument('--tex_equalize', action='store_true', default=argparse.SUPPRESS,
                   help="With --tex_project: equalise the cameras' exposure and white balance. The gains are estimated on the first "
                        "frame written, stored as proj_gains.json in the run directory and used for every frame (topo4d_amd.projtex "
                        "--equalize; --stat_cos_min, --stat_lo, --stat_hi, --eq_prior and --eq_min_overlap as it takes them).")
    p.add_argument('--tex_fill', action='store_true', default=argparse.SUPPRESS,
                   help="With --tex_project: fill the texels of every UV island that no view sees by push-pull from the island's "
                        "projected texels (topo4d_amd.projtex --tex_fill).")
    p.add_argument('--tex_reject', action='store_true', default=argparse.SUPPRESS,
                   help="With --tex_project: leave a view out of a texel where it disagrees with the median of the views that face "
                        "it (topo4d_amd.projtex --reject; --reject_tol, --vote_cos_min and --min_votes as it takes them).")
    p.add_argument('--tex_register', action='store_true', default=argparse.SUPPRESS,
                   help="With --tex_project: register every view to the blend of all views before it is projected "
                        "(topo4d_amd.projtex --register; --reg_block, --reg_stride, --reg_radius, --reg_ratio, --reg_reach and "
                        "--reg_rounds as it takes them).")
    from .projtex import add_band_options, add_consist_options, add_eq_options, add_options, add_register_options
    add_options(p, suppress=True)
    add_band_options(p, suppress=True)
    add_eq_options(p, suppress=True)
    add_consist_options(p, suppress=True)
    add_register_options(p, suppress=True)
    return p


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    train(args)
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
