"""
Per-element yardsticks for the kernels of csrc/t4d_optim.hip that run in every iteration of every loop: the fused Adam step with
region pins (k_adam_pin, host- and device-counted), the parameter activations and their vector-Jacobian products (k_activate_fwd /
k_activate_bwd, csrc/t4d_activations.h), the view sums (k_sum_views) and the dense-attribute interpolation (k_dense_interp).
numpy only: no product code, no GPU, no torch device.  Three pieces per operation, written next to each other:

REFERENCE.  The operation in float64 on the float32 inputs, from the formulas of the kernel headers (torch.optim.Adam without
weight decay or amsgrad, reference train.py:272-297 and :672-700; F.normalize / sigmoid / exp, helpers.py:95-97; the four-corner
weighted sum of helpers.py:237-253).  The hyper-parameters are the float32 values the C ABI receives, widened to double; the
bias corrections 1 - beta^t are evaluated in double on the host, as the library and torch do.

EMULATION.  The kernel's documented operation order with every float32 operation a numpy float32 operation (IEEE, round to
nearest even, denormals kept).  The two fmaf of the Adam step and the fmaf chains of the normalisation are exact: the product of
two float32 is exact in float64, the float64 sum s = fl(ab + c) leaves the remainder e of the two-sum, and rounding s to float32
differs from rounding ab + c only when s lies exactly half way between two float32 values and e != 0 - then e decides (`fmaf`).
`sqrtf(v) * inv_bc2_sqrt + eps` and `p - step_size * (m / denom)` are unfused, as `#pragma clang fp contract(off)` leaves them.
The emulation takes a `mutant` name: one-line deviations that tests/test_elementwise_host.py must see violate the bounds.

BOUND.  A running first-order error analysis through the reference's OWN intermediate values (class `E`): every quantity carries
its float64 value and a bound e on |float32 kernel value - float64 value|.  Exact inputs have e = 0.  The operations propagate

    a +- b : ea + eb          a b : |a| eb + |b| ea + ea eb          a / b : (ea + |a / b| eb) / (|b| - eb)
    sqrt a : min(ea / (sqrt a + sqrt max(a - ea, 0)), sqrt ea)                       c a, c exact : |c| ea

and every operation the kernel rounds adds ONE float32 rounding of its result: half the spacing of float32 at |value| + e (a
relative 2^-24 at most; 2^-150, half the DENORMAL spacing, below the normal range - so a v' under 1.2e-38 answers to the
denormal grid and a flushed denormal is a violation).  A host constant cast to float32 (step_size, inv_bc2_sqrt) carries its
actual cast error.  For the Adam step (c1 = 1 - beta1, c2 = 1 - beta2, both exact in float32):

    d  = rnd(g - m)                      m' = rnd(c1 d + m)                 -> e(m') = c1 e(d) + rnd:  |c1 (g - m)| and |m'| <= |m| + |c1 (g - m)|
    gg = rnd(g g),  bv = rnd(beta2 v)    v' = rnd(c2 gg + bv)               -> e(v') = c2 e(gg) + e(bv) + rnd:  |c2 g^2|, |beta2 v| and |v'|
    s  = rnd(sqrt v')                    denom = rnd(rnd(s inv) + eps)      -> e(v') enters through the square root
    q  = rnd(m' / denom)                 p' = rnd(p - rnd(step_size q))     -> e(m') and e(denom) enter the update, plus 1/2 ulp of p'

m' = m + c1 (g - m) cancels, which is why a bound relative to the update is unsound and the error is carried per operation.
The activations follow the same scheme (`activations_fwd_ref`, `activations_bwd_ref`); their backward takes the forward's float32 OUTPUTS as inputs, as the
kernel does, so g s (1 - s) is three roundings even where 1 - s cancels, and the normalisation's backward comes out relative to
|g| / |q| (every term of the propagated error carries the factor 1 / |q| and a factor |g_i| or |y . g| <= |g|), not to the result.
`wild` marks the elements where float32 leaves the reference's range - a non-finite input, or an intermediate beyond FLT_MAX
(g g for g = 1e20, the squared norm of a quaternion near 1e19): there no float64 statement holds and the kernel answers to the
emulation, bit for bit (NaN == NaN).

The view sums and the interpolation need no bound: a sequential float32 sum, v ascending, and a float64 left-to-right sum of
four products cast once to float32 are exact statements (`sum_views_ref`, `dense_interp_ref`); the check is bit equality.

CASES.  `adam_cases()`, `adam_trajectory()`, `activation_case(P)`, `SUM_VIEWS`, `sum_case`, `dense_cases()` build the inputs of
tests/test_gpu_elementwise.py; tests/test_elementwise_host.py proves on every one of them that the emulation stays inside the
bounds (soundness), anchors the references to torch in float64, and shows that each mutant leaves the bounds (sensitivity).
"""
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

F32, F64 = np.float32, np.float64
FMAX = float(np.finfo(F32).max)
FMIN = float(np.finfo(F32).tiny)                # smallest normal float32
DENORM = 2.0 ** -149                            # float32 denormal spacing
BETAS, EPS = (0.9, 0.999), 1e-15                # Topo4D's optimiser (train.py:296)
NORM_EPS = float(F32(1e-12))                    # kT4DNormEps
MAX_TENSORS, SUM_MAX_TENSORS, BLOCK = 12, 8, 256


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).reshape(np.shape(x))      # (ascontiguousarray makes a 0-dim array 1-dim)


def bits(x):
    return _f32(x).view(np.uint32)


def same_bits(a, b):
    """Element-wise: the same float32 bit pattern, or both NaN (the payload of a NaN is not part of any statement here)."""
    a, b = _f32(a), _f32(b)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulp32(x):
    """Spacing of float32 at |x| (float64 array); 2^-149 below the normal range."""
    with np.errstate(all="ignore"):
        return np.spacing(np.minimum(np.abs(np.asarray(x, F64)), FMAX).astype(F32)).astype(F64)


# ---------------------------------------------------------------------------------------------------------------------------
# value + error bound
# ---------------------------------------------------------------------------------------------------------------------------
class E:
    """float64 value `v` of a quantity and a bound `e` on |its float32 value in the kernel - v|."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=F64)
        self.e = np.broadcast_to(np.asarray(e, dtype=F64), self.v.shape)

    @staticmethod
    def const(x):
        """A host double handed to the kernel as float32: the actual cast error."""
        with np.errstate(all="ignore"):
            return E(x, abs(float(F32(x)) - float(x)))

    def rnd(self):
        return E(self.v, self.e + 0.5 * ulp32(np.abs(self.v) + self.e))

    def __add__(self, o):
        return E(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return E(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return E(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        q = self.v / o.v
        room = np.abs(o.v) - o.e
        return E(q, np.where(room > 0, (self.e + np.abs(q) * o.e) / np.where(room > 0, room, 1.0), np.inf))

    def scale(self, c):
        return E(self.v * c, self.e * abs(c))

    def sqrt(self):
        r = np.sqrt(self.v)
        den = r + np.sqrt(np.maximum(self.v - self.e, 0.0))
        return E(r, np.minimum(np.where(den > 0, self.e / np.where(den > 0, den, 1.0), np.inf), np.sqrt(self.e)))

    def out_of_range(self):
        """Not a statement about finite float32 arithmetic: NaN / inf, or beyond FLT_MAX."""
        return ~np.isfinite(self.v) | ~np.isfinite(self.e) | (np.abs(self.v) + self.e > FMAX)


def fmaf(a, b, c):
    """fmaf(a, b, c) of float32 arrays, exactly (one rounding of a b + c)."""
    a, b, c = (np.asarray(x, dtype=F32) for x in (a, b, c))
    with np.errstate(all="ignore"):
        ab = a.astype(F64) * b.astype(F64)                      # exact: 48 significant bits, exponent far inside float64's
        c64 = np.broadcast_to(c.astype(F64), ab.shape)
        s = ab + c64
        bb = s - ab
        e = (ab - (s - bb)) + (c64 - bb)                        # two-sum: ab + c == s + e exactly
        r = s.astype(F32)
        r64 = r.astype(F64)
        diff = s - r64
        nb = np.nextafter(r, np.where(diff > 0, np.inf, -np.inf).astype(F32))
        tie = np.isfinite(s) & np.isfinite(r64) & (diff != 0) & (e != 0) & (2.0 * s == r64 + nb.astype(F64))
        return np.where(tie & (np.sign(e) == np.sign(diff)), nb, r).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------------
# Adam + pins
# ---------------------------------------------------------------------------------------------------------------------------
def adam_hyper(lr, t, betas=BETAS, eps=EPS):
    """(beta1, beta2, eps, step_size, inv_bc2_sqrt) in double from the float32 hyper-parameters and the 1-based step t."""
    b1, b2, e, l = float(F32(betas[0])), float(F32(betas[1])), float(F32(eps)), float(F32(lr))
    bc1, bc2 = 1.0 - math.pow(b1, float(t)), 1.0 - math.pow(b2, float(t))
    return b1, b2, e, l / bc1, 1.0 / math.sqrt(bc2)


def _pin_rows(shape):
    rows = shape[0] if len(shape) > 0 else 1
    n = int(np.prod(shape, dtype=np.int64))
    return rows, (n // rows if rows else int(np.prod(shape[1:], dtype=np.int64)) or 1)


@dataclass
class AdamTensor:
    name: str
    p: np.ndarray                                   # float32, any shape ([rows, ...]; 0-dim: one row of one)
    g: Optional[np.ndarray] = None                  # None: no gradient this step (pins only, state untouched)
    m: Optional[np.ndarray] = None
    v: Optional[np.ndarray] = None
    lr: float = 0.0
    t: int = 1                                      # the step this call takes (state["step"] is t - 1 before it)
    pin_mask: Optional[np.ndarray] = None           # [rows] bool
    pin_values: Optional[np.ndarray] = None         # p's shape, read where the row is pinned
    clear_grad: bool = False


def _pinned(T, mutant=None):
    n = T.p.size
    if T.pin_mask is None:
        return np.zeros(n, dtype=bool)
    rows, width = _pin_rows(T.p.shape)
    i = np.arange(n)
    row = i % rows if mutant == "pin_mod_rows" else i // width
    return np.asarray(T.pin_mask, dtype=bool)[row]


def adam_ref(T, betas=BETAS, eps=EPS):
    """One Adam + pin step of tensor T in float64.  dict: p, m, v (class E, flat: value and bound), wild_p / wild_m / wild_v
    (where the float32 arithmetic leaves the reference's range), grad_after (None without a gradient), pinned."""
    p = E(np.asarray(T.p, F64).ravel())
    pinned = _pinned(T)
    none = np.zeros(p.v.shape, dtype=bool)
    with np.errstate(all="ignore"):
        if T.g is None:
            m = None if T.m is None else E(np.asarray(T.m, F64).ravel())
            v = None if T.v is None else E(np.asarray(T.v, F64).ravel())
            p2, wm, wv, wp, ga = p, none, none, ~np.isfinite(p.v), None
        else:
            b1, b2, ep, ss, inv = adam_hyper(T.lr, T.t, betas, eps)
            c1, c2 = 1.0 - b1, 1.0 - b2
            g, m, v = (E(np.asarray(x, F64).ravel()) for x in (T.g, T.m, T.v))
            d = (g - m).rnd()
            m2 = (d.scale(c1) + m).rnd()
            gg = (g * g).rnd()
            bv = v.scale(b2).rnd()
            v2 = (gg.scale(c2) + bv).rnd()
            s = v2.sqrt().rnd()
            den = ((s * E.const(inv)).rnd() + E(ep)).rnd()
            q = (m2 / den).rnd()
            r = (E.const(ss) * q).rnd()
            p2 = (p - r).rnd()
            wm = d.out_of_range() | m2.out_of_range()
            wv = gg.out_of_range() | bv.out_of_range() | v2.out_of_range() | (v.v < 0)
            wp = wm | wv | s.out_of_range() | den.out_of_range() | q.out_of_range() | r.out_of_range() | p2.out_of_range()
            m, v = m2, v2
            ga = np.zeros(p.v.shape, F32) if T.clear_grad else _f32(T.g).ravel()
        if T.pin_mask is not None:
            pv = np.asarray(T.pin_values, F64).ravel()
            p2 = E(np.where(pinned, pv, p2.v), np.where(pinned, 0.0, p2.e))
            wp = wp & ~pinned
    return {"p": p2, "m": m, "v": v, "wild_p": wp, "wild_m": wm, "wild_v": wv, "grad_after": ga, "pinned": pinned}


MUTANTS_ADAM = ("step_minus_1", "eps_1e-8", "flush_denormal_g", "pin_mod_rows", "fused_beta2_v", "neighbour_inv_bc2")


def adam_emu(T, betas=BETAS, eps=EPS, mutant=None, inv_from=None):
    """The kernel's float32 arithmetic on tensor T: dict p, m, v (float32, flat; m / v None without state), grad_after.
    inv_from: another tensor whose inv_bc2_sqrt this one uses (the `neighbour_inv_bc2` mutant, see adam_emu_case)."""
    p = _f32(T.p).ravel().copy()
    with np.errstate(all="ignore"):
        if T.g is None:
            m = None if T.m is None else _f32(T.m).ravel().copy()
            v = None if T.v is None else _f32(T.v).ravel().copy()
            ga = None
        else:
            t = T.t - 1 if mutant == "step_minus_1" else T.t
            b1, b2, ep, ss, inv = adam_hyper(T.lr, t, betas, 1e-8 if mutant == "eps_1e-8" else eps)
            if inv_from is not None and inv_from.g is not None:
                inv = adam_hyper(inv_from.lr, inv_from.t, betas, eps)[4]
            b1, b2, ep, ss, inv = F32(b1), F32(b2), F32(ep), F32(ss), F32(inv)
            g, m, v = (_f32(x).ravel() for x in (T.g, T.m, T.v))
            if mutant == "flush_denormal_g":
                g = np.where(np.abs(g) < F32(FMIN), F32(0) * g, g)
            c1, c2 = F32(1) - b1, F32(1) - b2
            m = fmaf(c1, g - m, m)
            if mutant == "fused_beta2_v":
                v = fmaf(b2, v, c2 * (g * g))
            else:
                v = fmaf(c2, g * g, b2 * v)
            denom = np.sqrt(v) * inv + ep
            p = p - ss * (m / denom)
            ga = np.zeros(p.shape, F32) if T.clear_grad else _f32(T.g).ravel().copy()
        pinned = _pinned(T, mutant)
        if T.pin_mask is not None:
            p = np.where(pinned, _f32(T.pin_values).ravel(), p)
    return {"p": _f32(p), "m": m, "v": v, "grad_after": ga}


def adam_emu_case(tensors, mutant=None, **kw):
    """adam_emu of every tensor of one launch; `neighbour_inv_bc2`: tensor k reads the next tensor's inv_bc2_sqrt."""
    out = []
    for k, T in enumerate(tensors):
        nb = tensors[(k + 1) % len(tensors)] if mutant == "neighbour_inv_bc2" else None
        out.append(adam_emu(T, mutant=mutant, inv_from=nb, **kw))
    return out


def excess(got, ref: E, wild, emu):
    """How far `got` (float32) is outside its statement, per element (<= 0: inside).  Where the reference holds: |got - ref| -
    bound.  Where float32 left its range (`wild`): 0 when got has the emulation's bits, +inf otherwise."""
    got = _f32(got).ravel()
    with np.errstate(all="ignore"):
        inside = np.abs(got.astype(F64) - ref.v) - ref.e
        inside = np.where(np.isfinite(got), inside, np.inf)
    return np.where(wild, np.where(same_bits(got, emu), 0.0, np.inf), inside)


# ---- Adam cases -----------------------------------------------------------------------------------------------------------
ADAM_STEPS = (1, 2, 10, 1100, 100000)
ADAM_LRS = (0.0, 1.6e-5, 0.0025, 0.05)
# 12 tensors (T4D_ADAM_MAX_TENSORS): element counts 256, 1, 255, 257, 0, 768, 512, 769, 256, 768, 3, 255 - below, at and one
# past a workgroup of 256, exact multiples (a tensor that exactly fills its workgroups), three workgroups + 1; widths 1, 3, 4, 48;
# tensors without gradient first, in the middle and last; an empty tensor in the middle; pins on the first row only, the last
# row only, every row, no row (an all-zero mask), random rows of a 48-wide tensor, and on a tensor without gradient.
ADAM_LAYOUT = (
    # name          shape      grad   pins      clear_grad
    ("nograd_first", (64, 4), False, "random", False),
    ("scalar", (), True, None, False),
    ("w3_255", (85, 3), True, "first", False),
    ("w1_257", (257,), True, "last", False),
    ("empty", (0, 3), True, None, False),
    ("w48_768", (16, 48), True, "every", False),
    ("nograd_mid", (128, 4), False, None, False),
    ("w1_769", (769, 1), True, "none", True),
    ("w4_256", (64, 4), True, "every", False),
    ("w48_pins", (16, 48), True, "random", False),
    ("w3_3", (1, 3), True, None, False),
    ("nograd_last", (85, 3), False, None, False),
)


def _pins(rng, shape, kind):
    if kind is None:
        return None, None
    rows = shape[0]
    mask = np.zeros(rows, dtype=bool)
    if kind == "first":
        mask[0] = True
    elif kind == "last":
        mask[-1] = True
    elif kind == "every":
        mask[:] = True
    elif kind == "random":
        mask[:] = rng.random(rows) < 0.4
        mask[1], mask[2] = True, False
    return mask, _f32(rng.standard_normal(shape) * 3.0)


def _gradients(rng, n):
    """Normal, log-uniform over 1e-12 .. 1e8, float32 denormals and exact zeros, interleaved element by element."""
    kind = rng.integers(0, 4, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = np.where(kind == 0, rng.standard_normal(n), 0.0)
    g = np.where(kind == 1, sign * 10.0 ** rng.uniform(-12, 8, n), g)
    g = np.where(kind == 2, sign * rng.integers(1, 1 << 23, n) * DENORM, g)
    return _f32(g)


def _consistent_state(rng, g, t, steps=40):
    """The float64 reference trajectory's (m, v) after min(t - 1, steps) steps from zero under gradients of g's own scale."""
    b1, b2 = float(F32(BETAS[0])), float(F32(BETAS[1]))
    m, v = np.zeros(g.shape, F64), np.zeros(g.shape, F64)
    for _ in range(min(t - 1, steps)):
        gk = g.astype(F64) * (1.0 + 0.3 * rng.standard_normal(g.shape))
        m = m + (1.0 - b1) * (gk - m)
        v = b2 * v + (1.0 - b2) * gk * gk
    return _f32(m), _f32(v)


def _inconsistent_state(rng, n):
    """Moments unrelated to the gradient: v over 60 decades, exactly zero and denormal under a non-zero m; m of either sign."""
    m = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2, n)
    v = 10.0 ** rng.uniform(-44, 16, n)
    kind = rng.integers(0, 6, n)
    v = np.where(kind == 0, 0.0, v)
    v = np.where(kind == 1, rng.integers(1, 1 << 20, n) * DENORM, v)
    return _f32(m), _f32(v)


def _fusion_probes(rng, n):
    """(g, m, v) whose v' tells `fmaf(c2, g g, beta2 v)` from the other fusion `fmaf(beta2, v, c2 (g g))`: v far below g^2,
    so that the second form's extra rounding of c2 g^2 is not covered by the (small) rounding of beta2 v.  The two forms differ
    by less than the bound on most inputs; the generator keeps the candidates on which the reference's own bound rejects the
    other form and fills up with the rest - a property of the arithmetic and the bound, no kernel involved."""
    N = 400000
    g = _f32(rng.standard_normal(N) * 10.0 ** rng.uniform(-6, 3, N))
    v = _f32(g.astype(F64) ** 2 * 10.0 ** rng.uniform(-8, -3, N))
    m = _f32(g * F32(0.5))
    T = AdamTensor("probe", g, g, m, v, lr=0.0025, t=10)
    bad = excess(adam_emu(T, mutant="fused_beta2_v")["v"], adam_ref(T)["v"], np.zeros(N, bool), g) > 0
    idx = np.concatenate([np.flatnonzero(bad)[:n // 4], np.flatnonzero(~bad)])[:n]
    return g[idx], m[idx], v[idx]


def adam_case(t, lr, seed=0, mixed=False):
    """The 12 tensors of one launch at step t and learning rate lr; mixed: t and lr rotate through ADAM_STEPS / ADAM_LRS from
    tensor to tensor (neighbours never share a step count) and tensor w48_768 carries the fusion probes."""
    rng = np.random.default_rng([seed, int(t), int(round(lr * 1e7)), int(mixed)])
    out: List[AdamTensor] = []
    for k, (name, shape, has_grad, pin_kind, clear) in enumerate(ADAM_LAYOUT):
        n = int(np.prod(shape, dtype=np.int64))
        tk = ADAM_STEPS[k % len(ADAM_STEPS)] if mixed else t
        lk = ADAM_LRS[(k + 1) % len(ADAM_LRS)] if mixed else lr
        p = rng.standard_normal(n) * np.where(rng.random(n) < 0.1, 1e3, 1.0)
        p = _f32(np.where(rng.random(n) < 0.05, 0.0, p))
        mask, vals = _pins(rng, shape, pin_kind)
        T = AdamTensor(name, p.reshape(shape), lr=lk, t=tk, pin_mask=mask, pin_values=vals, clear_grad=clear)
        m, v = _inconsistent_state(rng, n)
        if has_grad:
            g = _gradients(rng, n)
            mc, vc = _consistent_state(rng, g, tk)
            use = rng.random(n) < (0.7 if tk > 1 else 0.3)              # mostly the trajectory's own state, the rest unrelated
            m, v = np.where(use, mc, m), np.where(use, vc, v)
            if mixed and name == "w48_768":
                g, m, v = _fusion_probes(rng, n)
            if n >= 255:                                                # a handful of rows outside float32's range
                w = rng.choice(n, 10, replace=False)
                g[w[:8]] = _f32([np.inf, -np.inf, np.nan, 1e20, -1e20, 3e19, 1e20, -np.inf])
                m[w[6]], v[w[7]] = np.inf, np.nan
                p[w[8]], p[w[9]] = np.nan, -np.inf
                T.p = p.reshape(shape)
            T.g, T.m, T.v = g.reshape(shape), _f32(m).reshape(shape), _f32(v).reshape(shape)
        elif name != "nograd_last":                                     # state that a pins-only launch must leave alone
            T.m, T.v = _f32(m).reshape(shape), _f32(v).reshape(shape)
        out.append(T)
    return out


def adam_cases():
    """{name: tensors}: every step count with every learning rate, and the mixed launch."""
    cases = {f"t{t}_lr{lr:g}": adam_case(t, lr) for t in ADAM_STEPS for lr in ADAM_LRS}
    cases["mixed"] = adam_case(0, 0.0, mixed=True)
    return cases


TRAJ_STEPS = 40


def adam_trajectory(seed=7):
    """40 steps over the 12-tensor layout: (initial tensors with zero state, per-step {name: gradient or None}, per-step
    {name: lr}).  `w1_257` has a gradient on even steps only (20 steps at the end), the tensors without gradient never;
    learning rates change at steps 10 and 25."""
    rng = np.random.default_rng(seed)
    init = adam_case(1, 0.0025, seed=seed)
    for T in init:
        T.g, T.clear_grad = None, False
        T.m = T.v = None
        T.p = _f32(np.where(np.isfinite(T.p), T.p, 1.0))
    base = {T.name: 10.0 ** rng.uniform(-3, 1) for T in init}
    grads, lrs = [], []
    for it in range(TRAJ_STEPS):
        step_g = {}
        for (name, shape, has_grad, _, _) in ADAM_LAYOUT:
            on = has_grad and not (name == "w1_257" and it % 2 == 1)
            step_g[name] = _f32(rng.standard_normal(shape) * base[name]) if on else None
        grads.append(step_g)
        lr0 = 0.0025 if it < 10 else (0.00025 if it < 25 else 0.05)
        lrs.append({T.name: (lr0 if k % 2 == 0 else 1.6e-5 * (1 + (it >= 10))) for k, T in enumerate(init)})
    return init, grads, lrs


# ---------------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------------
LOGITS = (0.0, -0.0, 1e-8, -1e-8, 1.0, -1.0, 10.0, -10.0, 20.0, -20.0, 87.0, -87.0, 88.8, -88.8, 104.0, -104.0, -88.5, 88.5)
LOG_SCALES = (-104.0, -87.4, -10.0, 0.0, 10.0, 88.7, 89.0, -100.0, -88.5, 1e-8, -1e-8)
EXP_OVERFLOW = math.log(FMAX)                   # 88.7228: expf overflows above it


def _chain4(a, b):
    """fmaf(a3, b3, fmaf(a2, b2, fmaf(a1, b1, a0 b0))) of [P, 4] float32 arrays (x, y, z, w order)."""
    s = a[:, 0] * b[:, 0]
    for k in (1, 2, 3):
        s = fmaf(a[:, k], b[:, k], s)
    return s


def _chain4_E(a: List[E], b: List[E]) -> E:
    s = (a[0] * b[0]).rnd()
    for k in (1, 2, 3):
        s = (a[k] * b[k] + s).rnd()
    return s


def activations_fwd_ref(q, logit, log_scale):
    """float64 forward.  rot: list of 4 E (the normalisation's derived bound), wild_rot; sigmoid / exp: float64 values only (their
    float32 error rests on the device expf and is MEASURED in ulps, see ulp_error)."""
    q = np.asarray(q, F64)
    with np.errstate(all="ignore"):
        qe = [E(q[:, k]) for k in range(4)]
        n = _chain4_E(qe, qe).sqrt().rnd()
        clamped = n.v <= NORM_EPS
        undecided = np.abs(n.v - NORM_EPS) <= n.e                   # float32 may take the other branch: no case has such a row
        n = E(np.where(clamped, NORM_EPS, n.v), np.where(clamped, 0.0, n.e))
        rot = [(c / n).rnd() for c in qe]
        wild = ~np.isfinite(q).all(1) | ((q * q).sum(1) * (1 + 2.0 ** -20) > FMAX) | n.out_of_range() | undecided
        x, ls = np.asarray(logit, F64), np.asarray(log_scale, F64)
        return {"rot": rot, "wild_rot": wild, "op": 1.0 / (1.0 + np.exp(-x)), "scale": np.exp(ls)}


def activations_fwd_emu(q, logit, log_scale):
    """float32 forward in the kernel's order; expf is the correctly rounded float32 exponential here (the device's is not
    required to be: the GPU test measures it)."""
    q, x, ls = _f32(q), _f32(logit), _f32(log_scale)
    with np.errstate(all="ignore"):
        n = np.maximum(np.sqrt(_chain4(q, q)), F32(NORM_EPS))
        rot = q / n[:, None]
        e = np.exp(-x.astype(F64)).astype(F32)
        return {"rot": _f32(rot), "op": _f32(F32(1) / (F32(1) + e)), "scale": np.exp(ls.astype(F64)).astype(F32)}


def ulp_error(got, ref64):
    """|got - ref| in float32 ulps at the reference (denormal spacing below the normal range); a reference beyond FLT_MAX asks
    for +inf exactly, a NaN anywhere is an infinite error."""
    got = _f32(got).astype(F64)
    ref64 = np.asarray(ref64, F64)
    with np.errstate(all="ignore"):
        over = np.abs(ref64) > FMAX
        err = np.abs(got - ref64) / ulp32(ref64)
        err = np.where(over, np.where(got == np.sign(ref64) * np.inf, 0.0, np.inf), err)
        return np.where(np.isnan(got) | np.isnan(ref64), np.inf, err)


MUTANTS_ACT = ("sigmoid_bwd_gss", "normalize_bwd_clamped_at_2e-12")


def activations_bwd_ref(q, op, scale, g_rot, g_op, g_scale):
    """float64 vector-Jacobian products on the float32 forward OUTPUTS op / scale.  d_rot: list of 4 E, d_logit, d_log_scale: E;
    wild_rot / wild_logit / wild_scale."""
    q, g = np.asarray(q, F64), np.asarray(g_rot, F64)
    with np.errstate(all="ignore"):
        qe, ge = [E(q[:, k]) for k in range(4)], [E(g[:, k]) for k in range(4)]
        nn = _chain4_E(qe, qe).sqrt().rnd()
        clamped = nn.v <= NORM_EPS
        undecided = np.abs(nn.v - NORM_EPS) <= nn.e
        one = E(np.ones(q.shape[0]))
        inv = (one / E(np.where(clamped, 1.0, nn.v), np.where(clamped, 0.0, nn.e))).rnd()
        y = [(c * inv).rnd() for c in qe]
        yg = _chain4_E(y, ge)
        free = [(((gk - (yk * yg).rnd()).rnd()) * inv).rnd() for gk, yk in zip(ge, y)]
        held = [(gk / E(np.full(q.shape[0], NORM_EPS))).rnd() for gk in ge]
        d_rot = [E(np.where(clamped, h.v, f.v), np.where(clamped, h.e, f.e)) for f, h in zip(free, held)]
        wild_rot = ~np.isfinite(q).all(1) | ~np.isfinite(g).all(1) | ((q * q).sum(1) * (1 + 2.0 ** -20) > FMAX) | undecided
        for d in d_rot:
            wild_rot = wild_rot | d.out_of_range()
        s, go = E(np.asarray(op, F64).ravel()), E(np.asarray(g_op, F64).ravel())
        d_logit = ((go * s).rnd() * (E(np.ones(s.v.shape)) - s).rnd()).rnd()
        e, gs = E(np.asarray(scale, F64).ravel()), E(np.asarray(g_scale, F64).ravel())
        d_ls = (gs * e).rnd()
        return {"d_rot": d_rot, "d_logit": d_logit, "d_log_scale": d_ls, "wild_rot": wild_rot,
                "wild_logit": d_logit.out_of_range(), "wild_scale": d_ls.out_of_range()}


def activations_bwd_emu(q, op, scale, g_rot, g_op, g_scale, mutant=None):
    q, s, e, g, go, gs = (_f32(x) for x in (q, op, scale, g_rot, g_op, g_scale))
    with np.errstate(all="ignore"):
        nn = np.sqrt(_chain4(q, q))
        free = nn > F32(4e-12 if mutant == "normalize_bwd_clamped_at_2e-12" else NORM_EPS)
        inv = F32(1) / nn
        y = q * inv[:, None]
        yg = _chain4(y, g)
        d_free = (g - y * yg[:, None]) * inv[:, None]
        d_held = g / F32(NORM_EPS)
        d_rot = np.where(free[:, None], d_free, d_held)
        d_logit = go * s * s if mutant == "sigmoid_bwd_gss" else go * s * (F32(1) - s)
        return {"d_rot": _f32(d_rot), "d_logit": _f32(d_logit), "d_log_scale": _f32(gs * e)}


ACT_SIZES = (1, 255, 256, 257)
_ACT_ROWS = 257


def _activation_rows():
    rng = np.random.default_rng(11)
    N = _ACT_ROWS
    i = np.arange(N)
    unit = rng.standard_normal((N, 4))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    q = unit * (0.2 + 3.0 * rng.random((N, 1)))                       # ordinary non-unit rows
    kind = i % 8                                                    # the last row (P = 1) is kind 0 of 257 % 8 == 1 -> see below
    q[kind == 0] = 0.0
    q[kind == 1] = unit[kind == 1] * 5e-13                          # below kT4DNormEps: the clamped branch
    q[kind == 2] = unit[kind == 2] * 2e-12                          # just above it
    q[kind == 3] = rng.integers(-(1 << 22), 1 << 22, ((kind == 3).sum(), 4)) * DENORM
    q[kind == 4] = np.sign(unit[kind == 4]) * 10.0 ** rng.uniform(19.1, 19.4,((kind == 4).sum(), 4))   # |q|^2 overflows
    q = _f32(q)
    q64 = q.astype(F64)
    nrm = np.linalg.norm(q64, axis=1, keepdims=True)
    direction = np.where(nrm > 0, q64 / np.where(nrm > 0, nrm, 1.0), unit)
    rand = rng.standard_normal((N, 4))
    gk = (i // 8) % 4
    g = rand.copy()
    g[gk == 0] = direction[gk == 0] * rng.uniform(0.5, 4.0, ((gk == 0).sum(), 1))                   # parallel to q: d cancels
    g[gk == 1] = (rand - direction * (rand * direction).sum(1, keepdims=True))[gk == 1]             # orthogonal to q
    g[gk == 2] = 0.0
    g = _f32(g)
    nL, nS = len(LOGITS), len(LOG_SCALES)
    logit = np.where((i // nL) % 2 == 0, np.asarray(LOGITS)[i % nL], rng.standard_normal(N) * 4.0)
    j = np.arange(3 * N)
    ls = np.where((j // nS) % 2 == 0, np.asarray(LOG_SCALES)[j % nS], rng.standard_normal(3 * N) * 2.0 - 3.0)
    mag = lambda n: rng.standard_normal(n) * np.where(rng.random(n) < 0.1, 1e10, 1.0) * np.where(rng.random(n) < 0.1, 1e-30, 1.0)
    g_op = np.where(rng.random(N) < 0.1, 0.0, mag(N))
    g_sc = np.where(rng.random(3 * N) < 0.1, 0.0, mag(3 * N))
    return q, _f32(logit).reshape(N, 1), _f32(ls).reshape(N, 3), g, _f32(g_op).reshape(N, 1), _f32(g_sc).reshape(N, 3)


_ROWS_CACHE = []


def activation_case(P):
    """(unnorm_rotations [P,4], logit_opacities [P,1], log_scales [P,3], g_rot, g_op, g_scale): the LAST P rows of one table of
    257, so every size ends on the same rows and starts elsewhere; P = 1 is an ordinary quaternion with a parallel cotangent."""
    if not _ROWS_CACHE:
        _ROWS_CACHE.append(_activation_rows())
    rows = [a[_ACT_ROWS - P:].copy() for a in _ROWS_CACHE[0]]
    if P == 1:
        rows[0][:] = _f32([[0.3, -1.2, 0.8, 2.0]])
        rows[3][:] = rows[0] * F32(0.75)
    return tuple(rows)


# ---------------------------------------------------------------------------------------------------------------------------
# view sums and dense interpolation: exact statements
# ---------------------------------------------------------------------------------------------------------------------------
SUM_VIEWS = (1, 2, 7, 24)
SUM_N = (1, 3, 4, 5, 1023, 1024, 1025, 4096, 4100)


def sum_case(V, n, seed=0):
    """[V, n] float32 of mixed magnitudes (the order of a float32 sum matters on them)."""
    rng = np.random.default_rng([seed, V, n])
    return _f32(rng.standard_normal((V, n)) * 10.0 ** rng.integers(-3, 4, (V, n)))


def sum_views_ref(x):
    """Sequential float32 sum over the views, v ascending, one rounding per addition."""
    acc = _f32(x[0]).copy()
    for v in range(1, x.shape[0]):
        acc = acc + _f32(x[v])
    return acc


def dense_interp_ref(attr, quads, father, weight):
    """[n_coarse + n_dense, width]: the coarse rows copied, dense row d = the float64 left-to-right sum of its father quad's four
    corners times weight[d], cast to float32 once."""
    attr = _f32(attr)
    out = [attr]
    if len(father):
        c = attr[np.asarray(quads)[np.asarray(father)]].astype(F64)          # [n_dense, 4, width]
        w = np.asarray(weight, F64)
        s = c[:, 0] * w[:, 0, None]
        for k in (1, 2, 3):
            s = s + c[:, k] * w[:, k, None]
        out.append(s.astype(F32))
    return np.concatenate(out, 0)


def dense_cases(seed=3):
    """{name: (attr [n_coarse, width], quads [n_quads, 4] int32, father [n_dense] int32, weight [n_dense, 4] float64)}: widths 1,
    3, 4; quads that repeat a corner; weights that do not sum to 1 (negative, zero, large); no dense rows; nothing at all."""
    rng = np.random.default_rng(seed)
    cases = {}
    for width, nc, nq, nd in ((1, 300, 77, 555), (3, 97, 40, 260), (4, 64, 30, 449)):
        attr = _f32(rng.standard_normal((nc, width)) * 10.0 ** rng.integers(-2, 3, (nc, 1)))
        quads = rng.integers(0, nc, (nq, 4)).astype(np.int32)
        quads[::5, 3] = quads[::5, 0]                                         # a degenerate quad: one corner twice
        quads[1::7, 1] = quads[1::7, 2] = quads[1::7, 0]
        father = rng.integers(0, nq, nd).astype(np.int32)
        w = rng.random((nd, 4))
        w /= w.sum(1, keepdims=True)
        w[::3] = rng.standard_normal((len(w[::3]), 4)) * 3.0                  # no partition of unity
        w[1::11] = 0.0
        cases[f"w{width}"] = (attr, quads, father, np.ascontiguousarray(w, F64))
    a, qd, _, _ = cases["w3"]
    cases["no_dense"] = (a, qd, np.zeros(0, np.int32), np.zeros((0, 4), F64))
    cases["nothing"] = (np.zeros((0, 3), F32), qd, np.zeros(0, np.int32), np.zeros((0, 4), F64))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# verdicts shared by the host and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def adam_verdict(T, got, betas=BETAS, eps=EPS):
    """`got` = {p, m, v, grad_after} (flat float32; m / v / grad_after None where T has none) after one step of tensor T, held to
    the float64 reference under its bound.  Returns (violations, not_bit_equal): messages naming output and element, and the number
    of elements of p, m, v whose bits differ from the emulation's."""
    ref, emu = adam_ref(T, betas, eps), adam_emu(T, betas, eps)
    bad, off = [], 0
    for key, wild in (("p", ref["wild_p"]), ("m", ref["wild_m"]), ("v", ref["wild_v"])):
        if ref[key] is None:
            if got.get(key) is not None:
                bad.append(f"{T.name}.{key}: state appeared")
            continue
        x = excess(got[key], ref[key], wild, emu[key])
        if ref[key].v.size and not np.all(np.isfinite(ref[key].e[~wild])):
            bad.append(f"{T.name}.{key}: no finite bound")
        for i in np.flatnonzero(~(x <= 0))[:3]:
            bad.append(f"{T.name}.{key}[{i}]: got {_f32(got[key]).ravel()[i]!r}, reference {ref[key].v[i]!r} +- {ref[key].e[i]:.3g}"
                       f"{' (float32 out of range: emulation ' + repr(emu[key][i]) + ')' if wild[i] else ''}")
        off += int((~same_bits(got[key], emu[key])).sum())
    if ref["grad_after"] is not None and not np.all(same_bits(got["grad_after"], ref["grad_after"])):
        bad.append(f"{T.name}.grad: {'not zeroed' if T.clear_grad else 'changed'}")
    return bad, off


def bound_verdict(name, got, ref: E, wild, emu):
    """Messages for the elements of `got` outside `ref`'s bound (outside the emulation's bits where `wild`)."""
    x = excess(got, ref, wild, _f32(emu).ravel())
    bad = [] if np.all(np.isfinite(ref.e[~wild])) else [f"{name}: no finite bound"]
    for i in np.flatnonzero(~(x <= 0))[:3]:
        bad.append(f"{name}[{i}]: got {_f32(got).ravel()[i]!r}, reference {ref.v[i]!r} +- {ref.e[i]:.3g}, emulation {_f32(emu).ravel()[i]!r}")
    return bad


def activations_bwd_verdict(inputs, got, mutant_of=None):
    """inputs = (q, op, scale, g_rot, g_op, g_scale) with op / scale the forward's float32 outputs; got = {d_rot [P,4], d_logit,
    d_log_scale}: every element under the derived bound of activations_bwd_ref."""
    ref, emu = activations_bwd_ref(*inputs), activations_bwd_emu(*inputs)
    bad = []
    for k in range(4):
        bad += bound_verdict(f"d_rot[:, {k}]", _f32(got["d_rot"])[:, k], ref["d_rot"][k], ref["wild_rot"], emu["d_rot"][:, k])
    bad += bound_verdict("d_logit", got["d_logit"], ref["d_logit"], ref["wild_logit"], emu["d_logit"])
    bad += bound_verdict("d_log_scale", got["d_log_scale"], ref["d_log_scale"], ref["wild_scale"], emu["d_log_scale"])
    off = sum(int((~same_bits(_f32(got[k]).ravel(), emu[k].ravel())).sum()) for k in ("d_rot", "d_logit", "d_log_scale"))
    return bad, off


def rot_fwd_verdict(q, got_rot):
    ref = activations_fwd_ref(q, np.zeros((len(q), 1)), np.zeros((len(q), 3)))
    emu = activations_fwd_emu(q, np.zeros((len(q), 1), F32), np.zeros((len(q), 3), F32))["rot"]
    bad = []
    for k in range(4):
        bad += bound_verdict(f"rot[:, {k}]", _f32(got_rot)[:, k], ref["rot"][k], ref["wild_rot"], emu[:, k])
    return bad, int((~same_bits(got_rot, emu)).sum())
