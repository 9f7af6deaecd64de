"""
Camera cases for the rasterizer parity tests (tests/test_views_host.py on the CPU, tests/test_gpu_views.py on the GPU).

Every other parity test renders the scaffold head through scaffold/scene.camera_rig: principal point at the image centre,
fx == fy, no roll, every camera 0.9 m from the origin and aimed at it.  View depth stays in [0.79, 1.0] m there, so the near
cull, the EWA frustum clamp (T4D_FRUSTUM_CLAMP) and the difference between what `projmatrix` and what `tanfov` say about the
camera are never reached by the per-Gaussian arithmetic of k_preprocess and its backward.  The cases here reach them:

  family       what the views do
  offcentre    cx, cy at 20 % / 75 % of the image, the +-2 px offsets a Metashape calibration gives, and a centred view
  focal        fx / fy = 0.6 / 1.5 and the reverse
  roll         90, 180 and 37 degrees about the optical axis
  lateral      camera at 0.9 m aimed 0.2-0.3 m beside, above, below and diagonally off the head: Gaussians past the clamp on
               each side in x, in y and in both, carrying a large share of the gradient
  close        camera 0.26-0.30 m from the centre: Gaussians near-culled, others just past 0.2 m with radii of ~200 px
  inside       camera inside the head: one view with exactly one visible Gaussian, one with none
  depth        Gaussians from 0.21 m to 90 m (depth keys span float exponents) and exact duplicates of a mean, with different
               colour and opacity, in one tile (order by index)
  calibrated   the 24 cameras of tests/golden/g16_cameras.npz, intrinsics and image size divided by 32, the head translated to
               camera_center + 0.9 * view_direction of each camera in turn
  random<k>    24 seeded draws mixing all of the above (kept apart from test_gpu_configs._randomised_trial, whose seeds are
               named regressions)

A Case is ONE view.  Cases of a family share their Gaussians and image size and run in one launch (`batches`); a calibrated
case runs with the other cameras of the capture that have its image size (17 landscape, 5 portrait).  Every case DECLARES what it covers (`Coverage`); the tests measure the
same quantities from the oracles (`measure`) and assert the declaration (`check_coverage`), so that a later edit of a case
cannot quietly empty it.

Scenes use anisotropic scales (x3, per-axis factors 0.4-2.5) and random unit quaternions: with isotropic scales the rotation
gradient is round-off.  Images are at most 160 px on a side and not multiples of 16.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from oracle import torch_oracle as TO
from scaffold import reference_boundary as boundary, scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAD_KEYS = ("means3D", "means2D", "opacities", "scales", "rotations", "colors_precomp")
SUBSETS = ("clamp_x", "clamp_y", "clamp_xy", "edge", "near")
NEAR_BAND = 1.1                      # "near" subset: view depth within 10 % of the near plane


class Coverage(NamedTuple):
    """What a case declares about itself; lower bounds unless said otherwise."""
    culled: Tuple[int, int] = (0, 0)                         # near-culled Gaussians (z <= T4D_NEAR_CULL_Z): inclusive range
    visible: Tuple[int, Optional[int]] = (1, None)           # visible Gaussians (radius > 0): inclusive range
    clamp: Tuple[float, float, float, float] = (0, 0, 0, 0)  # share of the visible past the clamp at x-, x+, y-, y+
    both: float = 0.0                                        # share of the visible past it in x AND y
    clamp_grad: float = 0.0    # the clamped subset's largest float64 gradient entry / the tensor's, least over the tensors
    radius: int = 0                                          # largest radius, pixels


class Case(NamedTuple):
    name: str
    family: str
    rv: Dict[str, torch.Tensor]
    cam: object                      # GaussianRasterizationSettings (CPU tensors)
    cot_seed: int
    depth_alpha: bool
    cover: Coverage
    companions: tuple = ()           # cameras that run in the same launch besides the family's cases (calibrated)


def look_at(H, W, position, target=(0.0, 0.0, 0.0), roll=0.0, fx=1.0, fy=1.0, cx=None, cy=None, f=None, bg=None, place=None):
    """A camera at `position` whose optical axis passes through `target`, rolled by `roll` degrees about that axis, through
    the G1-pinned setup_camera.  f defaults to camera_rig's focal length (the 0.24 m head spans 70 % of the image height from
    0.9 m) whatever the distance, fx / fy are factors on it, cx / cy default to the image centre.  place = (u, v): turn the
    camera so that `target` projects to that pixel instead of the principal point."""
    c, t = np.asarray(position, np.float64), np.asarray(target, np.float64)
    fwd = (t - c) / np.linalg.norm(t - c)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.99 else np.array([0.0, 0.0, 1.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    a = math.radians(roll)
    right, down = math.cos(a) * right + math.sin(a) * down, -math.sin(a) * right + math.cos(a) * down
    R = np.stack([right, down, fwd], axis=0)
    if f is None:
        f = 0.7 * H * 0.9 / (2 * scene.SEMI_AXES[1])
    K = np.array([[f * fx, 0, W / 2.0 if cx is None else cx], [0, f * fy, H / 2.0 if cy is None else cy], [0, 0, 1.0]])
    if place is not None:
        d = np.array([(place[0] - K[0, 2]) / K[0, 0], (place[1] - K[1, 2]) / K[1, 1], 1.0])
        d /= np.linalg.norm(d)
        axis = np.cross([0.0, 0.0, 1.0], d)                 # rotation taking the optical axis onto the ray of that pixel
        s_, c_ = np.linalg.norm(axis), d[2]
        if s_ > 1e-12:
            k = axis / s_
            Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            R = (np.eye(3) + s_ * Kx + (1 - c_) * Kx @ Kx) @ R
    w2c = np.eye(4)
    w2c[:3, :3] = R
    w2c[:3, 3] = -R @ c
    cam = boundary.setup_camera(W, H, K, w2c.astype(np.float32), near=0.01, far=100)
    if bg is not None:
        cam = cam._replace(bg=torch.tensor(bg, dtype=torch.float32))
    return cam


def rig_position(azim, elev, distance=0.9):
    a, e = math.radians(azim), math.radians(elev)
    return distance * np.array([math.sin(a) * math.cos(e), math.sin(e), math.cos(a) * math.cos(e)])


def head(n_lat=16, n_lon=24, opacity="B", seed=0, scale=3.0):
    """The scaffold head with anisotropic scales and random unit quaternions."""
    p = scene.make_gaussians(n_lat, n_lon, opacity=opacity, seed=seed)
    rv = {k: v.detach() for k, v in boundary.params2rendervar(p).items() if k != "means2D"}
    rng = np.random.default_rng(7000 + seed)
    P = rv["means3D"].shape[0]
    rv["scales"] = (rv["scales"] * scale * torch.tensor(rng.uniform(0.4, 2.5, size=(P, 3)), dtype=torch.float32)).contiguous()
    rv["rotations"] = torch.nn.functional.normalize(torch.tensor(rng.normal(size=(P, 4)), dtype=torch.float32))
    return rv


def cotangents(case: Case):
    dc, dd, da = scene.output_cotangents(1, case.cam.image_height, case.cam.image_width, seed=case.cot_seed, depth_alpha=True)
    return (dc[0], dd[0], da[0]) if case.depth_alpha else (dc[0], None, None)


# ----------------------------------------------------------------------------------------------------------------------
# seeds and declarations
# ----------------------------------------------------------------------------------------------------------------------
# One scene seed per family (per camera for the calibrated cases, per draw for the randomised ones), chosen so that on every
# view the two oracles take each discrete per-pixel decision the same way (n_contrib identical, no alpha >= 1/255 decision
# split between fp32 and float64) and agree within tests/test_views_host.py's bounds on every subset.
SEEDS = {"offcentre": 12, "focal": 12, "roll": 14, "lateral": 15, "close": 15, "inside": 16, "depth": 20}
CALIBRATED_SEEDS = (500, 506, 503, 504, 504, 507, 506, 507, 508, 509, 511, 511, 513, 513, 514, 519, 516, 518, 519, 519, 520,
                    524, 523, 524)
RANDOM_SEEDS = (0, 101, 302, 3, 4, 5, 306, 7, 8, 109, 10, 11, 212, 13, 14, 415, 16, 17, 318, 119, 20, 21, 22, 123)

# name -> Coverage: what each case declares (lower bounds; `culled` and `visible` are ranges).  Written from the measured
# figures of the cases as committed, rounded down; tests/test_views_host.py prints the measured table.
DECLARED: Dict[str, Coverage] = {
    "offcentre/cx20_cy75": Coverage(culled=(0, 0), visible=(315, None), clamp=(0.0, 0.33, 0.33, 0.0), both=0.12, clamp_grad=0.6, radius=80),
    "offcentre/cx75_cy20": Coverage(culled=(0, 0), visible=(331, None), clamp=(0.25, 0.0, 0.0, 0.42), both=0.11, clamp_grad=0.2, radius=79),
    "offcentre/metashape_a": Coverage(culled=(0, 0), visible=(345, None), radius=69),
    "offcentre/metashape_b": Coverage(culled=(0, 0), visible=(345, None), radius=70),
    "offcentre/centred": Coverage(culled=(0, 0), visible=(345, None), radius=72),
    "focal/fx0.6_fy1.5": Coverage(culled=(0, 0), visible=(270, None), clamp=(0.45, 0.0, 0.13, 0.0), both=0.06, clamp_grad=0.1, radius=105),
    "focal/fx1.5_fy0.6": Coverage(culled=(0, 0), visible=(304, None), clamp=(0.0, 0.0, 0.0, 0.37), clamp_grad=0.1, radius=92),
    "roll/90": Coverage(culled=(0, 0), visible=(344, None), clamp=(0.0, 0.0, 0.11, 0.0), radius=84),
    "roll/180": Coverage(culled=(0, 0), visible=(345, None), clamp=(0.0, 0.17, 0.0, 0.0), radius=85),
    "roll/37": Coverage(culled=(0, 0), visible=(277, None), clamp=(0.21, 0.0, 0.0, 0.24), clamp_grad=0.1, radius=81),
    "lateral/right": Coverage(culled=(0, 0), visible=(189, None), clamp=(0.63, 0.0, 0.0, 0.0), clamp_grad=0.1, radius=74),
    "lateral/left": Coverage(culled=(0, 0), visible=(328, None), clamp=(0.0, 0.59, 0.0, 0.0), clamp_grad=0.1, radius=71),
    "lateral/above": Coverage(culled=(0, 0), visible=(276, None), clamp=(0.0, 0.0, 0.0, 0.28), clamp_grad=0.1, radius=70),
    "lateral/below": Coverage(culled=(0, 0), visible=(239, None), clamp=(0.0, 0.0, 0.35, 0.0), clamp_grad=0.1, radius=72),
    "lateral/diag_a": Coverage(culled=(0, 0), visible=(233, None), clamp=(0.42, 0.0, 0.0, 0.33), both=0.16, clamp_grad=0.1, radius=74),
    "lateral/diag_b": Coverage(culled=(0, 0), visible=(232, None), clamp=(0.0, 0.67, 0.35, 0.0), both=0.23, clamp_grad=0.1, radius=77),
    "close/0.30": Coverage(culled=(2, 2), visible=(279, None), clamp=(0.02, 0.0, 0.21, 0.24), radius=182),
    "close/0.26": Coverage(culled=(58, 58), visible=(221, None), clamp=(0.07, 0.07, 0.24, 0.24), both=0.01, clamp_grad=0.95, radius=181),
    "inside/one_visible": Coverage(culled=(383, 383), visible=(1, 1), radius=40),
    "inside/none_visible": Coverage(culled=(384, 384), visible=(0, 0), radius=0),
    "inside/outside": Coverage(culled=(0, 0), visible=(384, 384), radius=48),
    "depth/range_and_ties": Coverage(culled=(0, 0), visible=(284, None), radius=18),
    "depth/rolled": Coverage(culled=(0, 0), visible=(284, None), radius=18),
    "calibrated/J87351627": Coverage(culled=(0, 0), visible=(345, None), radius=90),
    "calibrated/K19210959": Coverage(culled=(0, 0), visible=(345, None), radius=93),
    "calibrated/K98707288": Coverage(culled=(0, 0), visible=(345, None), radius=94),
    "calibrated/K98707289": Coverage(culled=(0, 0), visible=(345, None), radius=80),
    "calibrated/K98707290": Coverage(culled=(0, 0), visible=(345, None), radius=98),
    "calibrated/K98707291": Coverage(culled=(0, 0), visible=(345, None), radius=92),
    "calibrated/K98707292": Coverage(culled=(0, 0), visible=(345, None), radius=94),
    "calibrated/K98707293": Coverage(culled=(0, 0), visible=(345, None), radius=82),
    "calibrated/K98707294": Coverage(culled=(0, 0), visible=(345, None), radius=94),
    "calibrated/K98707295": Coverage(culled=(0, 0), visible=(345, None), radius=96),
    "calibrated/K98707296": Coverage(culled=(0, 0), visible=(345, None), radius=94),
    "calibrated/K98707297": Coverage(culled=(0, 0), visible=(345, None), radius=84),
    "calibrated/K99216880": Coverage(culled=(0, 0), visible=(345, None), radius=90),
    "calibrated/K99216881": Coverage(culled=(0, 0), visible=(345, None), radius=90),
    "calibrated/K99216882": Coverage(culled=(0, 0), visible=(345, None), radius=88),
    "calibrated/K99216883": Coverage(culled=(0, 0), visible=(345, None), radius=81),
    "calibrated/K99216885": Coverage(culled=(0, 0), visible=(345, None), radius=84),
    "calibrated/K99216886": Coverage(culled=(0, 0), visible=(345, None), radius=87),
    "calibrated/K99216887": Coverage(culled=(0, 0), visible=(345, None), radius=89),
    "calibrated/K99216888": Coverage(culled=(0, 0), visible=(345, None), radius=81),
    "calibrated/K99216890": Coverage(culled=(0, 0), visible=(345, None), radius=97),
    "calibrated/K99216891": Coverage(culled=(0, 0), visible=(345, None), radius=93),
    "calibrated/K99216892": Coverage(culled=(0, 0), visible=(345, None), radius=90),
    "calibrated/K99216893": Coverage(culled=(0, 0), visible=(345, None), radius=83),
    "random0/0": Coverage(culled=(0, 0), visible=(135, None), clamp=(0.0, 0.0, 0.03, 0.05), radius=110),
    "random0/1": Coverage(culled=(0, 0), visible=(135, None), clamp=(0.0, 0.0, 0.0, 0.26), clamp_grad=0.1, radius=38),
    "random1/0": Coverage(culled=(0, 0), visible=(257, None), radius=90),
    "random1/1": Coverage(culled=(0, 0), visible=(240, None), radius=95),
    "random2/0": Coverage(culled=(0, 0), visible=(82, None), clamp=(0.05, 0.02, 0.2, 0.13), radius=423),
    "random2/1": Coverage(culled=(0, 0), visible=(90, None), clamp=(0.03, 0.0, 0.0, 0.0), radius=165),
    "random3/0": Coverage(culled=(0, 0), visible=(138, None), clamp=(0.0, 0.0, 0.3, 0.3), radius=303),
    "random3/1": Coverage(culled=(0, 0), visible=(175, None), radius=71),
    "random4/0": Coverage(culled=(0, 0), visible=(194, None), radius=43),
    "random4/1": Coverage(culled=(0, 0), visible=(194, None), radius=31),
    "random5/0": Coverage(culled=(0, 0), visible=(324, None), radius=77),
    "random5/1": Coverage(culled=(0, 0), visible=(240, None), clamp=(0.11, 0.0, 0.0, 0.0), radius=95),
    "random6/0": Coverage(culled=(0, 0), visible=(126, None), clamp=(0.36, 0.39, 0.07, 0.08), both=0.06, radius=325),
    "random6/1": Coverage(culled=(2, 2), visible=(154, None), clamp=(0.25, 0.26, 0.22, 0.14), both=0.15, radius=354),
    "random7/0": Coverage(culled=(0, 0), visible=(88, None), clamp=(0.31, 0.35, 0.03, 0.05), clamp_grad=0.4, radius=657),
    "random7/1": Coverage(culled=(0, 0), visible=(89, None), radius=313),
    "random8/0": Coverage(culled=(0, 0), visible=(158, None), radius=54),
    "random8/1": Coverage(culled=(0, 0), visible=(141, None), clamp=(0.34, 0.36, 0.09, 0.09), both=0.07, clamp_grad=0.75, radius=234),
    "random9/0": Coverage(culled=(0, 0), visible=(125, None), clamp=(0.0, 0.11, 0.01, 0.0), radius=61),
    "random9/1": Coverage(culled=(1, 1), visible=(111, None), clamp=(0.21, 0.27, 0.0, 0.0), clamp_grad=0.15, radius=183),
    "random10/0": Coverage(culled=(0, 0), visible=(316, None), radius=18),
    "random10/1": Coverage(culled=(0, 0), visible=(283, None), clamp=(0.0, 0.0, 0.11, 0.1), radius=80),
    "random11/0": Coverage(culled=(0, 0), visible=(135, None), clamp=(0.2, 0.18, 0.0, 0.0), radius=144),
    "random11/1": Coverage(culled=(11, 11), visible=(125, None), clamp=(0.32, 0.29, 0.29, 0.3), both=0.33, clamp_grad=0.95, radius=629),
    "random12/0": Coverage(culled=(0, 0), visible=(180, None), radius=122),
    "random12/1": Coverage(culled=(0, 0), visible=(179, None), clamp=(0.11, 0.09, 0.02, 0.11), radius=346),
    "random13/0": Coverage(culled=(0, 0), visible=(148, None), radius=37),
    "random13/1": Coverage(culled=(0, 0), visible=(148, None), radius=34),
    "random14/0": Coverage(culled=(0, 0), visible=(93, None), radius=99),
    "random14/1": Coverage(culled=(0, 0), visible=(79, None), clamp=(0.0, 0.39, 0.09, 0.0), both=0.04, clamp_grad=0.35, radius=97),
    "random15/0": Coverage(culled=(0, 0), visible=(138, None), radius=41),
    "random15/1": Coverage(culled=(0, 0), visible=(108, None), clamp=(0.0, 0.0, 0.08, 0.24), radius=127),
    "random16/0": Coverage(culled=(0, 0), visible=(118, None), radius=39),
    "random16/1": Coverage(culled=(0, 0), visible=(110, None), clamp=(0.0, 0.23, 0.24, 0.0), both=0.05, clamp_grad=0.05, radius=68),
    "random17/0": Coverage(culled=(0, 0), visible=(149, None), clamp=(0.03, 0.03, 0.14, 0.18), radius=124),
    "random17/1": Coverage(culled=(0, 0), visible=(170, None), clamp=(0.12, 0.0, 0.0, 0.0), radius=57),
    "random18/0": Coverage(culled=(0, 0), visible=(164, None), clamp=(0.0, 0.0, 0.0, 0.24), clamp_grad=0.3, radius=62),
    "random18/1": Coverage(culled=(0, 0), visible=(198, None), radius=44),
    "random19/0": Coverage(culled=(0, 0), visible=(155, None), clamp=(0.0, 0.93, 0.0, 0.0), clamp_grad=0.95, radius=234),
    "random19/1": Coverage(culled=(0, 0), visible=(168, None), radius=195),
    "random20/0": Coverage(culled=(0, 0), visible=(162, None), radius=23),
    "random20/1": Coverage(culled=(0, 0), visible=(155, None), clamp=(0.0, 0.0, 0.08, 0.16), clamp_grad=0.1, radius=81),
    "random21/0": Coverage(culled=(0, 0), visible=(229, None), radius=80),
    "random21/1": Coverage(culled=(0, 0), visible=(229, None), radius=65),
    "random22/0": Coverage(culled=(0, 0), visible=(99, None), radius=139),
    "random22/1": Coverage(culled=(0, 0), visible=(88, None), clamp=(0.28, 0.0, 0.0, 0.62), both=0.23, clamp_grad=0.85, radius=211),
    "random23/0": Coverage(culled=(0, 0), visible=(162, None), radius=74),
    "random23/1": Coverage(culled=(0, 0), visible=(162, None), radius=65),
}


def _case(name, family, rv, cam, cot_seed, depth_alpha=True, companions=()):
    return Case(name, family, rv, cam, cot_seed, depth_alpha, DECLARED.get(name, Coverage()), tuple(companions))


# ----------------------------------------------------------------------------------------------------------------------
# the named families
# ----------------------------------------------------------------------------------------------------------------------
def _offcentre(seed):
    """The head sits on the far side of the image from the principal point: Gaussians past the clamp (1.3 half-widths from the
    optical axis) are INSIDE the picture there, which a centred principal point never shows."""
    H, W = 104, 138
    rv = head(seed=seed)
    mk = lambda n, az, el, **kw: _case(f"offcentre/{n}", "offcentre", rv, look_at(H, W, rig_position(az, el), **kw), 201)
    return [mk("cx20_cy75", -35, 10, cx=0.20 * W, cy=0.75 * H, place=(0.80 * W, 0.22 * H)),
            mk("cx75_cy20", 40, -15, cx=0.75 * W, cy=0.20 * H, place=(0.18 * W, 0.80 * H)),
            mk("metashape_a", 20, 20, cx=W / 2 + 2.0, cy=H / 2 - 1.6),
            mk("metashape_b", -60, 0, cx=W / 2 - 2.0, cy=H / 2 + 1.3),
            mk("centred", 0, 0)]


def _focal(seed):
    H, W = 90, 122
    rv = head(seed=seed)
    return [_case("focal/fx0.6_fy1.5", "focal", rv, look_at(H, W, rig_position(25, 10), fx=0.6, fy=1.5, place=(-0.15 * W, 0.30 * H)), 202),
            _case("focal/fx1.5_fy0.6", "focal", rv, look_at(H, W, rig_position(-50, -10), fx=1.5, fy=0.6, place=(0.60 * W, 1.12 * H)), 203)]


def _roll(seed):
    H, W = 118, 86
    rv = head(seed=seed)
    views = ((90, 30, 10, (0.5 * W, 0.03 * H)), (180, -20, -20, (0.97 * W, 0.6 * H)), (37, 60, 15, (0.05 * W, 0.95 * H)))
    return [_case(f"roll/{r}", "roll", rv, look_at(H, W, rig_position(az, el), roll=r, place=pl), 204 + i)
            for i, (r, az, el, pl) in enumerate(views)]


def _lateral(seed):
    H, W = 106, 98
    rv = head(seed=seed)
    pos = rig_position(0, 0)
    aims = (("right", (0.25, 0, 0)), ("left", (-0.22, 0, 0)), ("above", (0, 0.20, 0)), ("below", (0, -0.25, 0)),
            ("diag_a", (0.20, 0.20, 0)), ("diag_b", (-0.24, -0.22, 0)))
    return [_case(f"lateral/{n}", "lateral", rv, look_at(H, W, pos, target=t), 210 + i) for i, (n, t) in enumerate(aims)]


def _close(seed):
    H, W = 72, 88
    rv = head(seed=seed)
    return [_case("close/0.30", "close", rv, look_at(H, W, rig_position(20, 10, 0.30)), 220),
            _case("close/0.26", "close", rv, look_at(H, W, rig_position(-40, -15, 0.26)), 221)]


def _inside(seed):
    H, W = 70, 90
    rv = head(seed=seed)
    # looking along +y from inside: place the camera so that the near plane passes between the two Gaussians that are
    # furthest along the axis - exactly one survives the cull
    y = np.sort(rv["means3D"][:, 1].double().numpy())
    near = TO.C["T4D_NEAR_CULL_Z"]
    bg = (0.3, 0.6, 0.1)
    one = look_at(H, W, (0.0, 0.5 * (y[-1] + y[-2]) - near, 0.0), target=(0.0, 1.0, 0.0), bg=bg)
    none = look_at(H, W, (0.0, 0.0, 0.0), target=(0.0, 0.0, 1.0), bg=bg)
    out = look_at(H, W, rig_position(10, 5), bg=bg)
    return [_case("inside/one_visible", "inside", rv, one, 230), _case("inside/none_visible", "inside", rv, none, 231),
            _case("inside/outside", "inside", rv, out, 232)]


DUPLICATES = 8          # of _depth: Gaussians 300 + j and 308 + j repeat the mean (and shape) of one of the first 300


def _depth(seed):
    """Gaussians along the rays of one camera at depths 0.21 m .. 90 m (geometric), sized in proportion to their depth, and
    eight of them three times over with different colours and opacities.  Opacity falls off as 1 / depth beyond 0.5 m, so that
    the DEPTH image stays of order one and the absolute output tolerance means what it means elsewhere."""
    H, W = 84, 108
    rng = np.random.default_rng(seed)
    cam = look_at(H, W, (0.0, 0.0, 0.0), target=(0.0, 0.0, 1.0))
    n = 300
    z = np.geomspace(0.21, 90.0, n)
    rng.shuffle(z)
    u, v = rng.uniform(-0.9, 0.9, n) * cam.tanfovx, rng.uniform(-0.9, 0.9, n) * cam.tanfovy
    means = np.stack([u * z, v * z, z], 1)
    scales = z[:, None] * 0.012 * rng.uniform(0.4, 2.5, size=(n, 3))
    q = rng.normal(size=(n, 4))
    dup = rng.choice(n, DUPLICATES, replace=False)
    means, scales, q, z = (np.concatenate([a, a[dup], a[dup]]) for a in (means, scales, q, z))
    P = means.shape[0]
    op = rng.uniform(0.3, 0.95, size=P) * np.minimum(1.0, 0.5 / z)
    rv = dict(means3D=torch.tensor(means, dtype=torch.float32), scales=torch.tensor(scales, dtype=torch.float32),
              rotations=torch.nn.functional.normalize(torch.tensor(q, dtype=torch.float32)),
              opacities=torch.tensor(op[:, None], dtype=torch.float32),
              colors_precomp=torch.tensor(rng.uniform(0, 1, size=(P, 3)), dtype=torch.float32))
    cam_b = look_at(H, W, (0.0, 0.0, 0.0), target=(0.0, 0.0, 1.0), roll=180, cx=W / 2 + 2.0, cy=H / 2 - 1.6)
    return [_case("depth/range_and_ties", "depth", rv, cam, 240), _case("depth/rolled", "depth", rv, cam_b, 241)]


def _calibrated(seeds):
    g = np.load(os.path.join(GOLDEN, "g16_cameras.npz"))
    cams, centres = [], []
    for i in range(len(g["labels"])):
        K = g[f"intrinsics_1_{i}"].copy()
        K[:2] /= 32.0
        H, W = (int(s) // 32 for s in g[f"image_size_1_{i}"])
        w2c = np.eye(4)
        w2c[:3] = g[f"extrinsics_1_{i}"]
        cams.append(boundary.setup_camera(W, H, K, w2c.astype(np.float32), near=0.01, far=100))
        centres.append(g[f"camera_center_1_{i}"] + 0.9 * g[f"view_direction_1_{i}"])
    size = lambda c: (c.image_height, c.image_width)
    out = []
    for i, cam in enumerate(cams):
        rv = head(seed=seeds[i])
        rv["means3D"] = (rv["means3D"].double() + torch.tensor(centres[i])).float().contiguous()
        others = tuple(c for j, c in enumerate(cams) if j != i and size(c) == size(cam))     # a launch has one image size
        assert others
        out.append(_case(f"calibrated/{g['labels'][i]}", "calibrated", rv, cam, 250 + i, i % 3 != 0, companions=others))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# randomised draws
# ----------------------------------------------------------------------------------------------------------------------
def _random(k, seed):
    rng = np.random.default_rng(52000 + seed)
    H, W = (int(s) + (3 if s % 16 == 0 else 0) for s in rng.integers(40, 157, size=2))
    rv = head(int(rng.integers(8, 17)), int(rng.integers(10, 25)), opacity="AB"[k % 2], seed=300 + seed,
              scale=float(rng.choice([1.0, 2.0, 3.0, 5.0])))
    cases = []
    for v in range(2):
        kind = str(rng.choice(["rig", "lateral", "close", "far"], p=[0.3, 0.3, 0.25, 0.15]))
        dist = {"rig": 0.9, "lateral": 0.9, "close": rng.uniform(0.26, 0.4), "far": rng.uniform(0.5, 1.6)}[kind]
        pos = rig_position(rng.uniform(-180, 180), rng.uniform(-60, 60), dist)
        target = np.zeros(3)
        if kind == "lateral":
            d = rng.normal(size=3)
            target = d / np.linalg.norm(d) * rng.uniform(0.15, 0.3)
        roll = float(rng.choice([0.0, 90.0, 180.0, rng.uniform(0, 360)]))
        fx, fy = (rng.uniform(0.6, 1.5), rng.uniform(0.6, 1.5)) if rng.random() < 0.5 else (1.0, 1.0)
        cx, cy = W / 2.0, H / 2.0
        off = rng.random()
        if off < 0.4:
            cx, cy = rng.uniform(0.2, 0.8) * W, rng.uniform(0.2, 0.8) * H
        elif off < 0.7:
            cx, cy = cx + rng.uniform(-2, 2), cy + rng.uniform(-2, 2)
        bg = rng.uniform(0, 1, 3) if k % 4 == 1 else None
        cam = look_at(H, W, pos, target=target, roll=roll, fx=fx, fy=fy, cx=cx, cy=cy, bg=bg)
        cases.append(_case(f"random{k}/{v}", f"random{k}", rv, cam, 400 + 2 * k + v, k % 3 != 0))
    return cases


FAMILY_BUILDERS = dict(offcentre=_offcentre, focal=_focal, roll=_roll, lateral=_lateral, close=_close, inside=_inside,
                       depth=_depth)
_CASES: Optional[List[Case]] = None


def cases() -> List[Case]:
    global _CASES
    if _CASES is None:
        out = []
        for fam, make in FAMILY_BUILDERS.items():
            out += make(SEEDS[fam])
        out += _calibrated(CALIBRATED_SEEDS)
        for k, s in enumerate(RANDOM_SEEDS):
            out += _random(k, s)
        assert len({c.name for c in out}) == len(out)
        for c in out:
            assert max(c.cam.image_height, c.cam.image_width) <= 160
            assert c.cam.image_height % 16 or c.cam.image_width % 16
        _CASES = out
    return _CASES


def families() -> Dict[str, List[Case]]:
    out: Dict[str, List[Case]] = {}
    for c in cases():
        out.setdefault(c.family, []).append(c)
    return out


def batches():
    """The multi-view launches: (label, rv, cams, [(view index, case), ...]).  One launch per family with shared Gaussians; a
    calibrated case runs among the other cameras of the capture with its image size, which see its head off-axis or not at all."""
    out = []
    for fam, cs in families().items():
        if cs[0].companions:
            for c in cs:
                out.append((c.name, c.rv, [c.cam] + list(c.companions), [(0, c)]))
        else:
            out.append((fam, cs[0].rv, [c.cam for c in cs], list(enumerate(cs))))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# subsets and coverage, measured from oracle results
# ----------------------------------------------------------------------------------------------------------------------
def view_space(case: Case):
    """(tx/tz, ty/tz, tz, limx, limy) of every Gaussian in the case's view, float64."""
    VT = case.cam.viewmatrix.reshape(4, 4).double().numpy()
    m = case.rv["means3D"].double().numpy()
    t = np.concatenate([m, np.ones((m.shape[0], 1))], 1) @ VT[:, :3]
    tz = np.where(t[:, 2] != 0, t[:, 2], 1.0)
    lim = TO.C["T4D_FRUSTUM_CLAMP"]
    return t[:, 0] / tz, t[:, 1] / tz, t[:, 2], lim * case.cam.tanfovx, lim * case.cam.tanfovy


def subsets(case: Case, radii, xy) -> Dict[str, np.ndarray]:
    """Boolean masks [P] over the VISIBLE Gaussians (radii > 0; radii and xy from an oracle): past the frustum clamp in x only,
    in y only, in both; 3-sigma rectangle clipped by an image edge; view depth within 10 % of the near plane."""
    H, W = case.cam.image_height, case.cam.image_width
    gx, gy = (W + 15) // 16, (H + 15) // 16
    vis = np.asarray(radii) > 0
    x, y, z, limx, limy = view_space(case)
    px, py = np.abs(x) > limx, np.abs(y) > limy
    r = np.asarray(radii, np.float64)
    xy = np.asarray(xy, np.float64)
    lo = lambda c: np.trunc((c - r) / 16)
    hi = lambda c: np.trunc((c + r + 15) / 16)
    clipped = (lo(xy[:, 0]) < 0) | (lo(xy[:, 1]) < 0) | (hi(xy[:, 0]) > gx) | (hi(xy[:, 1]) > gy)
    return dict(clamp_x=vis & px & ~py, clamp_y=vis & py & ~px, clamp_xy=vis & px & py, edge=vis & clipped,
                near=vis & (z <= NEAR_BAND * TO.C["T4D_NEAR_CULL_Z"]))


def measure(case: Case, radii, truth_grads) -> dict:
    """The quantities a Coverage declares, from an oracle's radii and the float64 oracle's gradients (dict of arrays)."""
    x, y, z, limx, limy = view_space(case)
    vis = np.asarray(radii) > 0
    n = max(int(vis.sum()), 1)
    share = lambda m: float((vis & m).sum()) / n
    clamped = vis & ((np.abs(x) > limx) | (np.abs(y) > limy))
    grad = 0.0
    if clamped.any():
        grad = min(float(np.abs(np.asarray(truth_grads[k], np.float64)[clamped]).max() /
                         max(np.abs(np.asarray(truth_grads[k], np.float64)).max(), 1e-300)) for k in GRAD_KEYS)
    return dict(culled=int((z <= TO.C["T4D_NEAR_CULL_Z"]).sum()), visible=int(vis.sum()),
                clamp=(share(x < -limx), share(x > limx), share(y < -limy), share(y > limy)),
                both=share((np.abs(x) > limx) & (np.abs(y) > limy)), n_clamped=int(clamped.sum()), clamp_grad=grad,
                radius=int(np.asarray(radii).max()) if len(radii) else 0)


def check_coverage(case: Case, got: dict):
    c = case.cover
    assert c.culled[0] <= got["culled"] <= c.culled[1], f"{case.name}: {got['culled']} near-culled, declared {c.culled}"
    assert c.visible[0] <= got["visible"] and (c.visible[1] is None or got["visible"] <= c.visible[1]), \
        f"{case.name}: {got['visible']} visible, declared {c.visible}"
    for side, want, have in zip(("x-", "x+", "y-", "y+"), c.clamp, got["clamp"]):
        assert have >= want, f"{case.name}: {have:.3f} of the visible past the clamp at {side}, declared {want}"
    assert got["both"] >= c.both, f"{case.name}: {got['both']:.3f} past the clamp in x and y, declared {c.both}"
    assert got["clamp_grad"] >= c.clamp_grad, \
        f"{case.name}: clamped subset carries {got['clamp_grad']:.3f} of the largest gradient, declared {c.clamp_grad}"
    assert got["radius"] >= c.radius, f"{case.name}: largest radius {got['radius']}, declared {c.radius}"


def coverage_row(case: Case, got: dict) -> str:
    return (f"{case.name:28s} {case.cam.image_width:3d}x{case.cam.image_height:<3d} vis {got['visible']:4d} culled {got['culled']:4d} "
            f"clamp x- {got['clamp'][0]:.2f} x+ {got['clamp'][1]:.2f} y- {got['clamp'][2]:.2f} y+ {got['clamp'][3]:.2f} "
            f"xy {got['both']:.2f} grad {got['clamp_grad']:.2f} rmax {got['radius']:4d}")


def subset_errors(mine, truth, masks, exclude=None) -> Dict[Tuple[str, str], Tuple[float, float, float]]:
    """(subset, tensor) -> (largest |mine - truth| over the subset, the subset's largest |truth| entry, the tensor's largest
    |truth| entry).  `exclude`: Gaussians left out (those with a threshold pixel in reach, held to the flip bounds instead)."""
    out = {}
    for s, m in masks.items():
        if exclude is not None:
            m = m & ~exclude
        if not m.any():
            continue
        for k in GRAD_KEYS:
            a = np.asarray(mine[k], np.float64).reshape(len(m), -1)
            b = np.asarray(truth[k], np.float64).reshape(len(m), -1)
            out[(s, k)] = (float(np.abs(a[m] - b[m]).max()), float(np.abs(b[m]).max()), float(np.abs(b).max()))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# both oracles on a case, computed once per process (the GPU tests run every case under three builds and two launch sizes)
# ----------------------------------------------------------------------------------------------------------------------
class Oracles(NamedTuple):
    r: object                # oracle.c_oracle.OracleRender (fp32)
    state: dict              # its state()
    grads: dict              # its gradients
    outs64: dict             # float64 restatement: outputs ...
    grads64: dict            # ... and autograd gradients, numpy


_ORACLES: Dict[str, Oracles] = {}


@contextlib.contextmanager
def one_oracle_thread():
    """oracle/raster_oracle.c sums its per-pixel backward into the per-Gaussian gradients with `omp atomic` from dynamically
    scheduled threads: the fp32 rounding of a gradient depends on the run (seen here: 1.9e-6 of a subset's scale on one
    thread, 2.0e-5 on eight).  The cases run it on ONE thread - pixels in scan order - so that what the tests measure and
    bound is reproducible; the caller's setting is put back afterwards."""
    try:
        gomp = ctypes.CDLL("libgomp.so.1")
        before = gomp.omp_get_max_threads()
    except (OSError, AttributeError):
        yield
        return
    gomp.omp_set_num_threads(1)
    try:
        yield
    finally:
        gomp.omp_set_num_threads(before)


def oracles(case: Case) -> Oracles:
    if case.name not in _ORACLES:
        from tests import util
        dc, dd, da = cotangents(case)
        with one_oracle_thread():
            r, g = util.c_oracle_render(case.cam, case.rv, dc, dd, da)
        outs, grads = util.torch_oracle_render(case.cam, case.rv, dc, dd, da)
        _ORACLES[case.name] = Oracles(r, r.state(), g, outs, {k: v.numpy() for k, v in grads.items()})
    return _ORACLES[case.name]
