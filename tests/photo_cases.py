"""
A per-pixel yardstick for the fused photometric loss (t4d_photometric_loss), from a float64 restatement of the reference loss
alone: no product code, no GPU.

tests/test_gpu_photometric.py feeds the kernel uniform noise and holds dL/dim to 5e-5 of the tensor's largest entry.  Noise has
variance 1/12: the SSIM constants do not matter there and nothing in E[x^2 + y^2] - mu1^2 - mu2^2, A2 - A1 or B2 - B1 cancels.
Captures are the opposite - smooth skin, a black background that render and target share exactly, a render that converges to the
photograph, a masked target with x0.1 steps - and on such images the reference's own float32 gradient is off by up to 5e-4 of
the tensor's maximum (noise: 1.4e-6), so that form of tolerance cannot be applied to them.  Here every pixel answers to its own scale.

TRUTH.  train.py:310,315 with helpers.py:115-116 and external.py:73-116, per view of N = 3 H W values and weight w = dL/dloss[v]:

    x' = e^m im + c,  y = gt,  G = the 11 x 11 window (zero padding),  mu1 = G*x', mu2 = G*y, e11 = G*x'^2, e22 = G*y^2, e12 = G*x'y
    A1 = 2 mu1 mu2 + C1,  A2 = 2 (e12 - mu1 mu2) + C2,  B1 = mu1^2 + mu2^2 + C1,  B2 = e11 + e22 - mu1^2 - mu2^2 + C2,  S = A1 A2 / (B1 B2)
    loss = 0.8 mean|x' - y| + 0.2 (1 - mean S)                                                       g = dL/dS = -0.2 w / N
    D1 = dL/dmu1 = 2 g (mu2 (A2 - A1) - S mu1 (B2 - B1)) / (B1 B2),   D2 = dL/de11 = -g S / B2,   D3 = dL/de12 = 2 g A1 / (B1 B2)
    dL/dx' = G*D1 + 2 x' (G*D2) + y (G*D3) + (0.8 w / N) sign(x' - y)                                 (G is symmetric: its own adjoint)
    dL/dim = e^m dL/dx',   dL/dcam_c = sum dL/dx',   dL/dcam_m = sum dL/dx' e^m im

all in float64, on the float32 inputs.  The window and the constants are the reference's own float32 values promoted to double:
the 11 taps are built and normalised in float32 (external.py:73-76) and C1, C2 are what float32 arithmetic makes of 0.01^2 and
0.03^2.  With the float64 window instead, the gradient of `bright_flat` moves by 1e-4 of its maximum: that is a difference of
operation, not of rounding, and the float32 window is what the reference computes with.  (The window and constants are
parameters of `forward`: with the float64 ones it equals oracle/loss_oracle.photometric_loss_torch in float64 to 1e-12, which ties
this module to the G3-pinned restatement; tests/test_photo_cases_host.py.)

SCALE.  s(p) is the same expression with every term replaced by its magnitude one level down,

    s' = G*T1 + 2 |x'| G*|D2| + |y| G*|D3| + (0.8 |w| / N) [x' != y],    T1 = 2 |g / (B1 B2)| (|mu2| (|A2| + |A1|) + |S mu1| (|B2| + |B1|))

(T1 so that the cancellation inside D1 counts), s = e^m s'; the camera gradients answer to the sums of the same magnitudes,
sum s' and sum s' |e^m im|.  A pixel of the shared black background further than the window from the face has s == 0 and must
receive exactly 0.

CASES (V = 2, seeded; `build`).  noise: the control.  flat_pair: two constants per plane, variance exactly 0 away from the
border.  bright_flat: gt = 1, im = 0.98 + 1e-3 noise, the worst cancellation of e11 + e22 - mu^2.  smooth: low-contrast shading
+ 0.004 noise, variance far below C2.  black_bg: a smooth face blob on exact zeros in both images, no affine - thousands of exact
ties x' == y and of pixels with s == 0.  converged: the same with the render within 0.002 of the target.  identity_affine:
black_bg with cam_m = cam_c = 0 exactly, so x' == im and the affine path and the camera gradients run with ties.  masked_step:
black_bg whose target has a rectangle x0.1 (train.py:324-326).  out_of_range: render in [-0.2, 1.5].  anti: im = 1 - gt, negative
sigma12 and negative S.  The cases without ties carry an affine with |cam_m| <= 0.1, |cam_c| <= 0.05.  Weights: (1, 1); the variant
"scaled" of every case has (0.5, 2.0); "zero_neg" of identity_affine has (0, -1.5).

SHAPES, the smallest at which each kernel's structure is exercised: (75, 100) - tiles of 64 x 44 and 32 x 44 in both
directions with ragged last tiles, three 64-thread strips, row segments of 16 and of 37 with a short last one; (7, 130) - shorter
than the window, three strips; (140, 47) - one column past a 44-wide tile and strip, three tile rows.

DECISIONS.  sign(x' - y) is the one discrete decision.  There are no allowed flips: the builder nudges im until every pixel that
is not an intended tie has |x' - y| >= 64 ulp32(max(|x'|, |y|)) in float64, so the sign is the same in float32 and float64; ties
exist only where x' == im exactly (no affine, or the identity affine) on the shared background.  No pixel is left out of any
check.

YARDSTICK.  Q32[(case, shape)] = (max_p |g32 - t| / s over s > 0, the same ratio for dL/dcam_m and for dL/dcam_c, max_v |l32 -
l64|) of oracle/loss_oracle.photometric_loss_torch in float32 on the CPU with one torch thread: the reference's numbers, never a
kernel's.  `python -m tests.photo_cases --measure` prints the table below.

CHECK.  |d_im - t| <= MARGIN Q32 s at every pixel with s > 0 and d_im == 0 where s == 0; camera gradients |err| <= max(MARGIN
Q32_cam, ceil(log2 n) 2^-24) scale with n = H W summed terms (the bound of a pairwise float32 sum: one realised scalar error can
be small by luck); loss |l - l64| <= max(MARGIN |l32 - l64|, 3e-6), 3e-6 being the suite's loss tolerance.  MARGIN = 4: the
kernel sums the same 121 products in another order (separable, fused multiply-adds, one reciprocal), so its error is another
draw of the same size; a factor of 4 covers the spread of a maximum over ~2e4 such draws and the order, and still fails an
implementation that loses a further digit.  It is not to be raised to make a case pass.
"""
from __future__ import annotations

import math
import sys
from typing import Callable, Dict, NamedTuple, Optional

import numpy as np
import torch

R = 5                                     # window radius
MARGIN = 4.0
SIGN_ULPS = 64                            # every decided pixel: |x' - y| at least this many float32 ulps
LOSS_TOL = 3e-6                           # tests/test_gpu_photometric.py's loss tolerance
V = 2
SHAPES = ((75, 100), (7, 130), (140, 47))
NAMES = ("noise", "flat_pair", "bright_flat", "smooth", "black_bg", "converged", "identity_affine", "masked_step", "out_of_range",
         "anti")
TIE_CASES = ("black_bg", "converged", "identity_affine", "masked_step")
NO_AFFINE = ("black_bg", "converged", "masked_step")
WEIGHTS = {"unit": (1.0, 1.0), "scaled": (0.5, 2.0), "zero_neg": (0.0, -1.5)}
VARIANTS = [(n, "unit") for n in NAMES] + [(n, "scaled") for n in NAMES] + [("identity_affine", "zero_neg")]

C1_32 = float(np.float32(0.01 ** 2))      # what `2 * mu1_mu2 + c1` adds in float32 (external.py:108-111)
C2_32 = float(np.float32(0.03 ** 2))


def window32() -> torch.Tensor:
    """external.py:73-76: torch.Tensor([...]) is float32, and so is the normalisation.  Returned as float64."""
    g = torch.tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return (g / g.sum()).double()


def window64() -> torch.Tensor:
    g = torch.tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float64)
    return g / g.sum()


# ----------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# ----------------------------------------------------------------------------------------------------------------------
def _band(n, win):
    """[n, n]: the 11 taps along one axis with zero padding (external.py:97 padding = 5)."""
    i = torch.arange(n)
    d = i[None, :] - i[:, None] + R
    return torch.where((d >= 0) & (d <= 2 * R), win[d.clamp(0, 2 * R)], torch.zeros((), dtype=win.dtype))


def _conv(shape, win):
    bh, bw = _band(shape[0], win), _band(shape[1], win)
    return lambda a: bh @ a @ bw


def _affine(im, cam_m, cam_c):
    if cam_m is None:
        return im, torch.ones(im.shape[0], 3, 1, 1, dtype=im.dtype)
    em = torch.exp(cam_m)[:, :, None, None]
    return em * im + cam_c[:, :, None, None], em


def _maps(x, y, conv, c1, c2):
    mu1, mu2 = conv(x), conv(y)
    e11, e22, e12 = conv(x * x), conv(y * y), conv(x * y)
    mu12 = mu1 * mu2
    A1, A2 = 2 * mu12 + c1, 2 * (e12 - mu12) + c2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + c1, (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + c2
    return mu1, mu2, A1, A2, B1, B2, A1 * A2 / (B1 * B2)


def forward(im, gt, cam_m=None, cam_c=None, win=None, c1=C1_32, c2=C2_32):
    """loss [V] of float64 tensors im, gt [V,3,H,W] (cam_m, cam_c [V,3] or None); differentiable."""
    H, W = im.shape[-2:]
    x, _ = _affine(im, cam_m, cam_c)
    S = _maps(x, gt, _conv((H, W), window32() if win is None else win), c1, c2)[-1]
    n = 3 * H * W
    return 0.8 * (x - gt).abs().sum((1, 2, 3)) / n + 0.2 * (1.0 - S.sum((1, 2, 3)) / n)


class Truth(NamedTuple):
    loss: np.ndarray             # [V]
    d_im: np.ndarray             # [V,3,H,W]
    d_m: np.ndarray              # [V,3] (also without an affine: what cam_m = 0 would receive)
    d_c: np.ndarray
    s: np.ndarray                # [V,3,H,W] per-pixel scale
    s_m: np.ndarray              # [V,3]
    s_c: np.ndarray
    ties: np.ndarray             # [V,3,H,W] bool: x' == y


def adjoint(im, gt, cam_m, cam_c, weight, mutate_d1: Optional[Callable] = None) -> Truth:
    """The explicit float64 adjoint (module docstring) of float32 (or float64) tensors.  `mutate_d1`: a map D1 -> D1' applied before
    the second filter (the host test's mutation)."""
    with torch.no_grad():
        im, gt = im.double(), gt.double()
        cam_m = None if cam_m is None else cam_m.double()
        cam_c = None if cam_c is None else cam_c.double()
        H, W = im.shape[-2:]
        n = 3 * H * W
        conv = _conv((H, W), window32())
        x, em = _affine(im, cam_m, cam_c)
        y = gt
        mu1, mu2, A1, A2, B1, B2, S = _maps(x, y, conv, C1_32, C2_32)
        w = weight.double()[:, None, None, None]
        g = -0.2 * w / n
        inv = 1.0 / (B1 * B2)
        D1 = 2 * g * inv * (mu2 * (A2 - A1) - S * mu1 * (B2 - B1))
        D2 = -g * S * B1 * inv
        D3 = 2 * g * A1 * inv
        if mutate_d1 is not None:
            D1 = mutate_d1(D1)
        dx = conv(D1) + 2 * x * conv(D2) + y * conv(D3) + (0.8 * w / n) * torch.sign(x - y)
        T1 = 2 * (g * inv).abs() * (mu2.abs() * (A2.abs() + A1.abs()) + (S * mu1).abs() * (B2.abs() + B1.abs()))
        sp = conv(T1) + 2 * x.abs() * conv(D2.abs()) + y.abs() * conv(D3.abs()) + (0.8 * w.abs() / n) * (x != y).double()
        loss = 0.8 * (x - y).abs().sum((1, 2, 3)) / n + 0.2 * (1.0 - S.sum((1, 2, 3)) / n)
        xi = em * im
        return Truth(loss.numpy(), (em * dx).numpy(), (dx * xi).sum((2, 3)).numpy(), dx.sum((2, 3)).numpy(),
                     (em * sp).numpy(), (sp * xi.abs()).sum((2, 3)).numpy(), sp.sum((2, 3)).numpy(), (x == y).numpy())


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    shape: tuple                          # (H, W)
    variant: str
    im: torch.Tensor                      # [V,3,H,W] float32
    gt: torch.Tensor
    cam_m: Optional[torch.Tensor]         # [V,3] float32 or None
    cam_c: Optional[torch.Tensor]
    weight: torch.Tensor                  # [V] float32
    tie_ok: torch.Tensor                  # [V,3,H,W] bool: the shared background, where x' == y is intended

    @property
    def key(self):
        return (self.name, self.shape)


def _smooth(g, H, W, waves=4):
    """[V,3,H,W] in about [-1, 1]: a few long waves (40 .. 150 pixels) of random direction and phase per plane."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    out = torch.zeros(V, 3, H, W)
    for _ in range(waves):
        lam = 40 + 110 * torch.rand(V, 3, 1, 1, generator=g)
        th = 2 * math.pi * torch.rand(V, 3, 1, 1, generator=g)
        ph = 2 * math.pi * torch.rand(V, 3, 1, 1, generator=g)
        out += torch.cos(2 * math.pi * (xx * torch.cos(th) + yy * torch.sin(th)) / lam + ph)
    return out / waves


def _blob(H, W):
    """[H, W] bool: the face, an ellipse that leaves more than a window of background on both sides of the longer axis."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ry, rx = max(0.3 * H, 4.0), 0.25 * W
    return ((yy - (H - 1) / 2) / ry) ** 2 + ((xx - (W - 1) / 2) / rx) ** 2 < 1.0


def _ulp32(a64):
    return np.spacing(np.abs(a64).astype(np.float32)).astype(np.float64)


def sign_margin(c: Case):
    """(min over the pixels that are not exact ties of |x' - y| / ulp32(max(|x'|, |y|)), ties [V,3,H,W]), from float64."""
    x, _ = _affine(c.im.double(), None if c.cam_m is None else c.cam_m.double(), None if c.cam_c is None else c.cam_c.double())
    x, y = x.numpy(), c.gt.double().numpy()
    tie = x == y
    rel = np.abs(x - y) / _ulp32(np.maximum(np.abs(x), np.abs(y)))
    return (float(rel[~tie].min()) if (~tie).any() else np.inf), tie


def _nudged(im, gt, cam_m, cam_c, tie_ok):
    """im moved, pixel by pixel, until every pixel outside `tie_ok` has |x' - y| >= 2 SIGN_ULPS ulp32 (float64 arithmetic on the
    float32 values): by 4 SIGN_ULPS ulps of x', away from y."""
    im = im.clone()
    m64 = None if cam_m is None else cam_m.double()
    c64 = None if cam_c is None else cam_c.double()
    for _ in range(20):
        x, em = _affine(im.double(), m64, c64)
        d = x - gt.double()
        ulp = torch.from_numpy(_ulp32(torch.maximum(x.abs(), gt.double().abs()).numpy()))
        bad = (d.abs() < 2 * SIGN_ULPS * ulp) & ~tie_ok
        if not bad.any():
            return im
        step = torch.where(d >= 0, 1.0, -1.0) * 4 * SIGN_ULPS * ulp / em
        im = torch.where(bad, (im.double() + step).float(), im)
    raise AssertionError("the nudge did not settle")


def build(name: str, shape, variant: str = "unit") -> Case:
    H, W = shape
    like = "black_bg" if name in ("identity_affine", "masked_step") else name          # those two ARE black_bg's images
    g = torch.Generator().manual_seed(7000 + 100 * NAMES.index(like) + SHAPES.index(tuple(shape)))
    rand = lambda *s: torch.rand(*s, generator=g)
    randn = lambda *s: torch.randn(*s, generator=g)
    full = (V, 3, H, W)
    tie_ok = torch.zeros(full, dtype=torch.bool)
    if name == "noise":
        im = rand(*full)
        gt = (im + randn(*full) * 0.1).clamp(0, 1)
    elif name == "flat_pair":
        im = (0.3 + 0.5 * rand(V, 3, 1, 1)).expand(full).contiguous()
        gt = (0.3 + 0.5 * rand(V, 3, 1, 1)).expand(full).contiguous()
    elif name == "bright_flat":
        gt = torch.ones(full)
        im = 0.98 + 1e-3 * randn(*full)
    elif name == "smooth":
        base = 0.5 + 0.1 * _smooth(g, H, W)
        gt = base + 0.004 * randn(*full)
        im = base + 0.02 * _smooth(g, H, W) + 0.004 * randn(*full)
    elif name in TIE_CASES:
        face = _blob(H, W).expand(full)
        skin = (0.45 + 0.25 * _smooth(g, H, W)) * (0.6 + 0.4 * rand(V, 3, 1, 1))
        zero = torch.zeros(full)
        gt = torch.where(face, skin, zero)
        if name == "converged":
            im = torch.where(face, skin + 0.002 * (2 * rand(*full) - 1), zero)
        else:
            im = torch.where(face, skin + 0.05 * _smooth(g, H, W) + 0.01 * randn(*full), zero)
        if name == "masked_step":                 # train.py:324-326: masked_gt[filtered_mask == 1] *= 0.1
            r0, r1, c0, c1 = H // 3, (2 * H + 2) // 3, W // 2 - 3, W // 2 + max(W // 8, 6)
            gt[:, :, r0:r1, c0:c1] *= 0.1
        tie_ok = ~face.clone()
    elif name == "out_of_range":
        im = -0.2 + 1.7 * rand(*full)
        gt = rand(*full)
    elif name == "anti":
        gt = (0.5 + 0.35 * _smooth(g, H, W) + 0.02 * randn(*full)).clamp(0, 1)
        im = 1.0 - gt + 0.02 * randn(*full)
    else:
        raise KeyError(name)
    if name in NO_AFFINE:
        cam_m = cam_c = None
    elif name == "identity_affine":
        cam_m, cam_c = torch.zeros(V, 3), torch.zeros(V, 3)
    else:
        cam_m, cam_c = 0.2 * rand(V, 3) - 0.1, 0.1 * rand(V, 3) - 0.05
    im, gt = im.float().contiguous(), gt.float().contiguous()
    im = _nudged(im, gt, cam_m, cam_c, tie_ok).contiguous()
    return Case(name, tuple(shape), variant, im, gt, cam_m, cam_c, torch.tensor(WEIGHTS[variant], dtype=torch.float32), tie_ok)


_PREPARED: Dict[tuple, tuple] = {}


def prepared(name, shape, variant="unit"):
    """(case, float64 truth), computed once per process and left unchanged."""
    k = (name, tuple(shape), variant)
    if k not in _PREPARED:
        c = build(name, shape, variant)
        _PREPARED[k] = (c, adjoint(c.im, c.gt, c.cam_m, c.cam_c, c.weight))
    return _PREPARED[k]


# ----------------------------------------------------------------------------------------------------------------------
# the reference's own float32 arithmetic, and the yardstick recorded from it
# ----------------------------------------------------------------------------------------------------------------------
def restatement32(c: Case):
    """(loss [V], dL/dim, dL/dcam_m, dL/dcam_c) of oracle/loss_oracle.photometric_loss_torch in float32 on the CPU, one torch
    thread, autograd with the case's view weights.  Camera gradients are None without an affine."""
    from oracle import loss_oracle
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        im = c.im.clone().requires_grad_(True)
        cam = None if c.cam_m is None else [c.cam_m.clone().requires_grad_(True), c.cam_c.clone().requires_grad_(True)]
        l = torch.stack([loss_oracle.photometric_loss_torch(im[v], c.gt[v], *(() if cam is None else (cam[0][v], cam[1][v])))
                         for v in range(V)])
        (l * c.weight).sum().backward()
    finally:
        torch.set_num_threads(threads)
    return (l.detach().numpy(), im.grad.numpy(), None if cam is None else cam[0].grad.numpy(),
            None if cam is None else cam[1].grad.numpy())


def ratios(t: Truth, loss, d_im, d_m=None, d_c=None) -> dict:
    """{"im": max_p |d_im - t| / s over s > 0, "m", "c": the same for the camera gradients over scale > 0 (None without them),
    "loss": max_v |loss - l64|, "stray": the number of non-zero values where the scale is 0}."""
    def one(got, want, scale):
        got = np.asarray(got, np.float64)
        held = scale > 0
        r = np.where(held, np.abs(got - want) / np.where(held, scale, 1.0), 0.0)
        return float(r.max()), int(((got != 0) & ~held).sum())
    out = {"loss": float(np.abs(np.asarray(loss, np.float64) - t.loss).max())}
    out["im"], stray = one(d_im, t.d_im, t.s)
    out["m"] = out["c"] = None
    if d_m is not None:
        out["m"], a = one(d_m, t.d_m, t.s_m)
        out["c"], b = one(d_c, t.d_c, t.s_c)
        stray += a + b
    out["stray"] = stray
    return out


def cam_floor(shape) -> float:
    """ceil(log2 n) 2^-24, n = H W: the bound of a pairwise float32 sum of n terms, relative to the sum of their magnitudes."""
    return math.ceil(math.log2(shape[0] * shape[1])) * 2.0 ** -24


def check(c: Case, loss, d_im, d_m=None, d_c=None, q32=None, margin=MARGIN, what="") -> dict:
    """A result (arrays of the case's shapes, any float type) against the float64 truth of the case (module docstring, CHECK).
    `q32`: the yardstick row, Q32[c.key] when None.  Returns ratios(...)."""
    _, t = prepared(c.name, c.shape, c.variant)
    q_im, q_m, q_c, q_loss = Q32[c.key] if q32 is None else q32
    what = what or f"{c.name} {c.shape[0]}x{c.shape[1]} {c.variant}"
    d_im = np.asarray(d_im, np.float64)
    assert np.isfinite(d_im).all() and np.isfinite(np.asarray(loss, np.float64)).all(), f"{what}: not finite"
    null = np.argwhere((t.s == 0) & (d_im != 0))
    assert len(null) == 0, (f"{what}: dL/dim{tuple(null[0])} = {d_im[tuple(null[0])]:.3e} where the pixel's scale is 0 "
                            f"({len(null)} such pixels)")
    r = ratios(t, loss, d_im, d_m, d_c)
    err = np.abs(d_im - t.d_im)
    over = err - margin * q_im * t.s
    i = np.unravel_index(int(over.argmax()), over.shape)
    assert over[i] <= 0, (f"{what}: dL/dim{i} = {d_im[i]:.6e}, truth {t.d_im[i]:.6e}: err {err[i]:.3e} is {err[i] / t.s[i]:.3e} of the "
                          f"pixel's scale {t.s[i]:.3e}, allowed {margin:g} x {q_im:.2e} ({int((over > 0).sum())} pixels over; worst "
                          f"ratio {r['im']:.3e})")
    if c.cam_m is not None:
        assert d_m is not None and d_c is not None, f"{what}: the case has an affine and the result no camera gradients"
        for nm, got, want, scale, q in (("cam_m", d_m, t.d_m, t.s_m, q_m), ("cam_c", d_c, t.d_c, t.s_c, q_c)):
            got = np.asarray(got, np.float64)
            assert np.isfinite(got).all(), f"{what}: dL/d{nm} not finite"
            assert not ((scale == 0) & (got != 0)).any(), f"{what}: dL/d{nm} = {got} where its scale is 0"
            bound = max(margin * q, cam_floor(c.shape)) * scale
            bad = np.abs(got - want) > bound
            assert not bad.any(), (f"{what}: dL/d{nm} {got[bad]} vs {want[bad]}: err / scale {r[nm[-1]]:.3e}, allowed "
                                   f"{max(margin * q, cam_floor(c.shape)):.3e}")
    tol = max(margin * q_loss, LOSS_TOL)
    assert r["loss"] <= tol, f"{what}: loss {np.asarray(loss)} vs {t.loss}: off by {r['loss']:.3e}, allowed {tol:.3e}"
    return r


def measure(name, shape):
    """The yardstick row of one case and shape from the float32 restatement: (q_im, q_m, q_c, |l32 - l64|); 0.0 where the case has
    no affine."""
    c, t = prepared(name, shape)
    r = ratios(t, *restatement32(c))
    return (r["im"], r["m"] or 0.0, r["c"] or 0.0, r["loss"])


# (max_p |g32 - t| / s,  the same for dL/dcam_m,  for dL/dcam_c,  max_v |l32 - l64|) - `python -m tests.photo_cases --measure`
Q32: Dict[tuple, tuple] = {
    ('noise', (75, 100)): (2.62e-07, 7.82e-09, 5.84e-09, 9.7e-09),
    ('noise', (7, 130)): (1.91e-07, 9.25e-09, 9.81e-09, 1.4e-08),
    ('noise', (140, 47)): (2.82e-07, 5.50e-09, 9.06e-09, 3.2e-08),
    ('flat_pair', (75, 100)): (4.12e-07, 1.83e-07, 1.82e-07, 6.7e-05),
    ('flat_pair', (7, 130)): (2.57e-07, 9.41e-08, 1.00e-07, 3.6e-07),
    ('flat_pair', (140, 47)): (4.49e-07, 3.53e-07, 3.53e-07, 1.2e-05),
    ('bright_flat', (75, 100)): (6.95e-07, 3.70e-08, 3.70e-08, 2.0e-05),
    ('bright_flat', (7, 130)): (2.05e-07, 7.75e-09, 1.28e-08, 9.1e-08),
    ('bright_flat', (140, 47)): (8.85e-07, 6.86e-08, 6.87e-08, 1.6e-05),
    ('smooth', (75, 100)): (1.87e-06, 1.51e-08, 1.52e-08, 2.3e-07),
    ('smooth', (7, 130)): (2.05e-07, 8.62e-09, 7.17e-09, 2.6e-08),
    ('smooth', (140, 47)): (1.27e-06, 8.97e-09, 8.82e-09, 4.7e-07),
    ('black_bg', (75, 100)): (2.59e-06, 0.00e+00, 0.00e+00, 2.6e-08),
    ('black_bg', (7, 130)): (3.87e-07, 0.00e+00, 0.00e+00, 1.4e-08),
    ('black_bg', (140, 47)): (1.55e-06, 0.00e+00, 0.00e+00, 5.2e-08),
    ('converged', (75, 100)): (2.53e-06, 0.00e+00, 0.00e+00, 3.0e-08),
    ('converged', (7, 130)): (3.42e-07, 0.00e+00, 0.00e+00, 1.8e-08),
    ('converged', (140, 47)): (2.40e-06, 0.00e+00, 0.00e+00, 8.2e-08),
    ('identity_affine', (75, 100)): (2.59e-06, 9.01e-09, 9.98e-09, 2.6e-08),
    ('identity_affine', (7, 130)): (3.87e-07, 1.12e-08, 1.11e-08, 1.4e-08),
    ('identity_affine', (140, 47)): (1.55e-06, 7.01e-09, 4.97e-09, 5.2e-08),
    ('masked_step', (75, 100)): (4.26e-06, 0.00e+00, 0.00e+00, 5.6e-09),
    ('masked_step', (7, 130)): (5.10e-07, 0.00e+00, 0.00e+00, 1.8e-08),
    ('masked_step', (140, 47)): (4.40e-06, 0.00e+00, 0.00e+00, 2.6e-08),
    ('out_of_range', (75, 100)): (4.47e-07, 1.81e-08, 4.95e-09, 5.0e-08),
    ('out_of_range', (7, 130)): (2.42e-07, 2.81e-08, 1.08e-08, 9.3e-08),
    ('out_of_range', (140, 47)): (5.55e-07, 3.25e-08, 7.13e-09, 5.9e-08),
    ('anti', (75, 100)): (6.03e-06, 6.22e-09, 5.56e-09, 2.9e-07),
    ('anti', (7, 130)): (3.86e-07, 9.68e-09, 7.45e-09, 3.3e-08),
    ('anti', (140, 47)): (4.00e-06, 5.08e-09, 5.87e-09, 1.9e-07),
}


if __name__ == "__main__":
    if "--measure" in sys.argv:
        print("Q32: Dict[tuple, tuple] = {")
        for name in NAMES:
            for shape in SHAPES:
                q = measure(name, shape)
                print(f"    ({name!r}, {shape!r}): ({q[0]:.2e}, {q[1]:.2e}, {q[2]:.2e}, {q[3]:.1e}),")
        print("}")
