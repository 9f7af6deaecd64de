"""
A per-Gaussian yardstick for the rasterizer's gradients, from the float64 oracle alone (no product code, no GPU).

tests/test_gpu_parity.check_grads holds a whole tensor to GRAD_REL of its LARGEST entry, so most rows - two thirds to four
fifths of them lie below a tenth of that entry - may be off by a percent of their own size and pass.  Here every row answers to
its own scale:

    t      the float64 autograd gradient (util.torch_oracle_render) - the truth
    g_j    the same backward, K = 4 times, every non-zero cotangent multiplied elementwise by independent seeded random signs
           (the gradient is linear in the cotangents; the K passes and the truth share one forward graph)
    n      sqrt(mean_j g_j^2), elementwise: the size the row's pixel sum has when nothing cancels by luck
    S_i    max over the components of row i of max(|t|, n)

so that a row whose true gradient happens to cancel answers to the size of its terms, not to zero.  `rotations` cancels later,
in the per-Gaussian chain rule behind the pixel sums, where n cannot see it: its scale is raised to
4 max_k(scales[i,k])^2 S_cov[i], S_cov the row scale of the float64 oracle's `cov3D_precomp` gradient for the covariance built
from the same scales and quaternions (|dSigma/dq| <= 2 |s|^2 |dR/dq|, |dR/dq| <= 2 for a unit quaternion).

check_grads_rowwise: max|g - t| over row i <= GRAD_REL * S_i for every visible Gaussian; exactly zero where radii == 0 or
S_i == 0.  GRAD_REL is tests/test_gpu_parity's, imported.

The module also names the CASES the row check runs on (tests/test_grad_rows_host.py on the two oracles,
tests/test_gpu_grad_rows.py on the kernels) and their cotangent KINDS.  A case is only a row-check case if the fp32 C oracle
and the float64 oracle take every discrete decision the same way (radii and n_contrib equal at every pixel): its seeds were
picked on the CPU, from the references alone, until that held, and the host test asserts it.  There are no "allowed flips".
"""
from __future__ import annotations

import contextlib
import math
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, NamedTuple, Tuple

import numpy as np
import torch

from oracle import torch_oracle as TO
from scaffold import scene
from tests import util
from tests.adversarial_views import one_oracle_thread
from tests.test_gpu_parity import GRAD_REL

K_SIGNS = 4
SIGN_SEED = 9100
KINDS = ("mixed", "colour", "depth", "alpha", "l1")
COV_KEYS = ("means3D", "means2D", "opacities", "colors_precomp", "cov3D_precomp")
SH_KEYS = ("means3D", "means2D", "opacities", "scales", "rotations", "shs")


# ----------------------------------------------------------------------------------------------------------------------
# the yardstick
# ----------------------------------------------------------------------------------------------------------------------
def sign_flipped(cot, j):
    """The cotangent triple `cot` with every non-zero tensor multiplied elementwise by seeded random signs (draw j)."""
    g = torch.Generator().manual_seed(SIGN_SEED + j)
    out = []
    for t in cot:
        if t is None:
            out.append(None)
            continue
        s = torch.randint(0, 2, t.shape, generator=g).to(t.dtype) * 2 - 1
        out.append(t * s if bool(t.any()) else t)
    return tuple(out)


def covariance_of(rv, scale_modifier=1.0):
    """[P, 6] float64 upper triangle of R diag(s)^2 R^T, as tests/test_gpu_parity.test_cov3d_precomp_path builds it."""
    R = TO.quat_to_rot(rv["rotations"].double())
    RS = R * (scale_modifier * rv["scales"].double())[:, None, :]
    S = RS @ RS.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def _rows(a):
    a = np.asarray(a, np.float64)
    return a.reshape(a.shape[0], -1)


def _scales_of(t, flipped):
    """{tensor: S[P]} from the truth `t` and the sign-flipped gradients (dicts of float64 tensors)."""
    out = {}
    for k in t:
        n = np.sqrt(np.mean([_rows(g[k].numpy()) ** 2 for g in flipped], axis=0))
        out[k] = np.maximum(np.abs(_rows(t[k].numpy())), n).max(axis=1) if n.shape[1] else np.zeros(n.shape[0])
    return out


@contextlib.contextmanager
def one_torch_thread():
    """The float64 oracle is thousands of small tensor operations: torch's intra-op thread pool only slows it down (x2 here).  One
    intra-op thread while it runs - independent passes run side by side instead - and the caller's setting back afterwards."""
    before = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(before)


def _oracle_passes(cam, rv, cot, flips):
    with one_torch_thread():
        return util.torch_oracle_render(cam, rv, *cot, extra_cotangents=flips)


def yardstick(cam, rv, cot):
    """(outs, truth, S) of one view, one scene and one cotangent triple (dc, dd, da): the float64 oracle's outputs, its gradients
    {tensor: float64 array} and the row scales {tensor: [P]}."""
    flips = [sign_flipped(cot, j) for j in range(K_SIGNS)]
    with ThreadPoolExecutor(max_workers=1) as side:
        cov = None
        if rv.get("rotations") is not None:
            rv_cov = {k: v for k, v in rv.items() if k not in ("scales", "rotations")}
            rv_cov["cov3D_precomp"] = covariance_of(rv, cam.scale_modifier)
            cov = side.submit(_oracle_passes, cam, rv_cov, cot, flips)
        outs, t, flipped = _oracle_passes(cam, rv, cot, flips)
        S = _scales_of(t, flipped)
        if cov is not None:
            _, tc, fc = cov.result()
    if cov is not None:
        S_cov = _scales_of({"cov3D_precomp": tc["cov3D_precomp"]}, fc)["cov3D_precomp"]
        smax = rv["scales"].double().numpy().max(axis=1)
        S["rotations"] = np.maximum(S["rotations"], 4.0 * smax ** 2 * S_cov)
    return outs, {k: g.numpy() for k, g in t.items()}, S


def row_ratios(g, truth, S, radii, v, keys):
    """{tensor: (err[P], ratio[P])} of view v of `g` ([V, P, ...] arrays): err = max|g - t| over the row, ratio = err / S_i where the
    row is held to its scale (radii > 0 and S_i > 0), 0 elsewhere (those rows must be exactly zero)."""
    out = {}
    live = np.asarray(radii) > 0
    for k in keys:
        a = _rows(np.asarray(g[k])[v])
        err = np.abs(a - _rows(truth[k])).max(axis=1) if a.shape[1] else np.zeros(a.shape[0])
        held = live & (S[k] > 0)
        out[k] = (err, np.where(held, err / np.where(held, S[k], 1.0), 0.0))
    return out


def check_grads_rowwise(hip_g, truth, S, radii, v, keys=util.GRAD_KEYS, xy=None):
    """Every Gaussian of view v of `hip_g` against the float64 truth, relative to its own row scale (module docstring).  `xy`
    (optional, [P, 2] pixel centres) adds the failing Gaussian's position and tile to the message.  Returns {tensor: worst ratio}."""
    radii = np.asarray(radii)
    worst = {}
    for k, (err, ratio) in row_ratios(hip_g, truth, S, radii, v, keys).items():
        a = _rows(np.asarray(hip_g[k])[v])
        worst[k] = float(ratio.max()) if len(ratio) else 0.0
        where = lambda i: "" if xy is None else (f" at ({xy[i, 0]:.2f}, {xy[i, 1]:.2f}), tile ({int(xy[i, 0]) // 16}, "
                                                 f"{int(xy[i, 1]) // 16})")
        dead = np.nonzero((radii == 0) & (np.abs(a).max(axis=1, initial=0.0) != 0))[0]
        assert len(dead) == 0, f"grad {k}[view {v}], Gaussian {dead[0]}: radius 0 but gradient {a[dead[0]]}"
        null = np.nonzero((radii > 0) & (S[k] == 0) & (np.abs(a).max(axis=1, initial=0.0) != 0))[0]
        assert len(null) == 0, f"grad {k}[view {v}], Gaussian {null[0]}{where(null[0])}: row scale 0 but gradient {a[null[0]]}"
        i = int(ratio.argmax()) if len(ratio) else 0
        assert worst[k] <= GRAD_REL, (f"grad {k}[view {v}], Gaussian {i} (radius {int(radii[i])}){where(i)}: err {err[i]:.3e} vs its "
                                      f"row scale S_i {S[k][i]:.3e}; worst err / S_i of the tensor {worst[k]:.3e} > {GRAD_REL:g} "
                                      f"({int((ratio > GRAD_REL).sum())} rows over)")
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# cotangents
# ----------------------------------------------------------------------------------------------------------------------
def cotangents(kind, V, H, W, seed):
    """(dc, dd, da), each [V, C, H, W] or None.  "mixed", "colour", "depth" and "alpha" are cuts of ONE draw of
    scene.output_cotangents(depth_alpha=True) - the dense white noise of the parity tests; "depth" and "alpha" carry an all-zero
    colour cotangent.  "l1": sign(low-frequency pattern) / (3HW) on colour, the coherent signs a masked L1 loss hands the backward."""
    dc, dd, da = scene.output_cotangents(V, H, W, seed=seed, depth_alpha=True)
    if kind == "mixed":
        return dc, dd, da
    if kind == "colour":
        return dc, None, None
    if kind == "depth":
        return torch.zeros_like(dc), dd, None
    if kind == "alpha":
        return torch.zeros_like(dc), None, da
    if kind == "l1":
        rng = np.random.default_rng(seed)
        y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
        fx, fy, ph = rng.uniform(0.5, 2.5, (V, 3, 1, 1)), rng.uniform(0.5, 2.5, (V, 3, 1, 1)), rng.uniform(0, 2 * math.pi, (V, 3, 1, 1))
        pattern = np.sin(2 * math.pi * (fx * x + fy * y) + ph)
        return torch.tensor(np.where(pattern >= 0, 1.0, -1.0) / (3 * H * W), dtype=torch.float32), None, None
    raise ValueError(kind)


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
def anisotropic(rv, seed):
    """scene.make_gaussians makes isotropic splats, whose rotation gradient is only its radial part: per-axis scale factors
    0.4-2.5 and random unit quaternions, as tests/adversarial_views.head."""
    rng = np.random.default_rng(7100 + seed)
    P = rv["means3D"].shape[0]
    rv = dict(rv)
    rv["scales"] = (rv["scales"] * torch.tensor(rng.uniform(0.4, 2.5, size=(P, 3)), dtype=torch.float32)).contiguous()
    rv["rotations"] = torch.nn.functional.normalize(torch.tensor(rng.normal(size=(P, 4)), dtype=torch.float32))
    return rv


class Case(NamedTuple):
    name: str
    make: Callable[[], Tuple[dict, list]]        # -> (rv, cams)
    cot_seed: int
    kinds: Tuple[str, ...]
    keys: Tuple[str, ...] = util.GRAD_KEYS
    builds: bool = True                          # run under every render_build (False: the launch picks its own)


def _head(n_lat, n_lon, H, W, V, opacity, seed, **kw):
    def make():
        rv, cams = util.make_scene(n_lat, n_lon, H, W, V, opacity=opacity, seed=seed, **kw)
        return anisotropic(rv, seed), cams
    return make


def _negative_sh(make):
    def build():
        rv, cams = make()
        rv["shs"] = rv["shs"].clone()
        rv["shs"][::7, 0, :] = -3.0     # negative colours: clamped, their `shs` rows have no gradient at all (S_i == 0)
        return rv, cams
    return build


def _corners(seed):
    def make():
        from tests.test_gpu_bwd_moments import corner_scene
        rv, cams, _, _, _ = corner_scene(96, 96, 2, seed=seed)
        return rv, cams
    return make


def _cov(make):
    def build():
        rv, cams = make()
        rv["cov3D_precomp"] = covariance_of(rv).float().contiguous()
        del rv["scales"], rv["rotations"]
        return rv, cams
    return build


# corner_scene draws its cotangents from scene.output_cotangents(seed + 1): kinds "colour" and "mixed" with cot_seed = seed + 1
# ARE its depth_alpha = False and True variants
CORNER_SEED = 31
CASES: Dict[str, Case] = {c.name: c for c in (
    Case("head96_B", _head(20, 32, 96, 96, 2, "B", seed=5), 6, KINDS),
    Case("head96_A", _head(20, 32, 96, 96, 2, "A", seed=5), 6, ("mixed", "l1")),
    Case("ragged75x100_bg", _head(16, 24, 75, 100, 3, "B", seed=11, bg=[0.2, 0.5, 0.9]), 12, ("mixed", "alpha")),
    Case("corners96", _corners(CORNER_SEED), CORNER_SEED + 1, ("colour", "mixed", "depth")),
    Case("sh3_80", _negative_sh(_head(16, 24, 80, 80, 2, "B", seed=7, sh_degree=3)), 8, ("mixed", "l1"), SH_KEYS, builds=False),
    Case("cov3d_80", _cov(_head(16, 24, 80, 80, 2, "B", seed=9)), 10, ("mixed", "colour"), COV_KEYS, builds=False),
    Case("one_view128", _head(30, 50, 128, 128, 1, "B", seed=36), 37, ("mixed", "depth"), builds=False),
)}
PAIRS = [(c.name, kind) for c in CASES.values() for kind in c.kinds]


class Prepared(NamedTuple):
    rv: dict
    cams: list
    cot: tuple                 # (dc, dd, da), [V, ...] or None
    views: list                # per view: View


class View(NamedTuple):
    outs: dict                 # float64 oracle: radii, n_contrib, color, depth, alpha (numpy)
    truth: dict                # float64 gradients
    S: dict                    # row scales
    r: object                  # fp32 C oracle render (radii, state())
    state: dict
    grads_c: dict              # its gradients


_SCENES: Dict[str, tuple] = {}
_PREPARED: Dict[Tuple[str, str], Prepared] = {}


def prepared(name, kind) -> Prepared:
    """Scene, cotangents and both oracles' results of a (case, kind), computed once per process and left unchanged."""
    if (name, kind) not in _PREPARED:
        case = CASES[name]
        if name not in _SCENES:
            _SCENES[name] = case.make()
        rv, cams = _SCENES[name]
        V, H, W = len(cams), cams[0].image_height, cams[0].image_width
        cot = cotangents(kind, V, H, W, case.cot_seed)
        views = []
        cvs = [tuple(None if t is None else t[v] for t in cot) for v in range(V)]
        with ThreadPoolExecutor(max_workers=V) as pool:                       # torch releases the GIL inside its operations
            sticks = list(pool.map(lambda v: yardstick(cams[v], rv, cvs[v]), range(V)))
        for v, cv in enumerate(cvs):
            outs, truth, S = sticks[v]
            with one_oracle_thread():
                r, g = util.c_oracle_render(cams[v], rv, *cv)
            outs = {k: outs[k].numpy() for k in ("radii", "n_contrib", "color", "depth", "alpha")}
            views.append(View(outs, truth, S, r, r.state(), g))
        _PREPARED[(name, kind)] = Prepared(rv, cams, cot, views)
    return _PREPARED[(name, kind)]
