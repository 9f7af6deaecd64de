"""
tests/elementwise_ref.py on the CPU: what makes its bounds a yardstick for tests/test_gpu_elementwise.py.

  * the exact fmaf emulation against rational arithmetic, ties and denormals included;
  * SOUNDNESS: on every Adam and activation case of the GPU tests the float32 emulation of the kernel's operation order stays
    inside the float64 reference's bound, with zero exceptions, every bound finite where it is applied, and the elements handed to
    the emulation instead (float32 out of range) are the handful of rows built for that;
  * ANCHOR: the float64 Adam reference iterated over 12 steps (a tensor skipping alternate steps, a learning-rate change at step
    4, pins left out) equals torch.optim.Adam on float64 CPU tensors to 1e-12 per element, step counts included; the float64
    activation reference equals F.normalize / sigmoid / exp and their autograd in float64 to 1e-12;
  * SENSITIVITY: each one-line mutant of the EMULATION leaves the bound on a committed case, named in the assertion.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import elementwise_ref as R

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def adam_cases():
    return R.adam_cases()


def test_fmaf_emulation_is_exact():
    rng = np.random.default_rng(1)
    n = 4000
    a = R._f32(rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n))
    b = R._f32(rng.standard_normal(n) * 10.0 ** rng.integers(-20, 18, n))
    c = R._f32(-(a.astype(F64) * b.astype(F64)) * (1 + rng.standard_normal(n) * 10.0 ** rng.integers(-9, 1, n)))   # cancelling
    # half-way cases: a b + c exactly between two float32 values up to a remainder far below float64's last bit of the sum
    a[:200] = F32(1 + 2.0 ** -23); b[:200] = F32(1 + 2.0 ** -23)          # a b = 1 + 2^-22 + 2^-46
    c[:100] = F32(2.0 ** -24); c[100:200] = F32(-2.0 ** -24)
    a[200:300] = F32(1 - 2.0 ** -24); b[200:300] = F32(1 + 2.0 ** -23); c[200:300] = F32(2.0 ** -24) * rng.integers(1, 9, 100)
    a[300:400] = R._f32(rng.integers(1, 1 << 12, 100) * R.DENORM); b[300:400] = R._f32(rng.random(100)); c[300:400] = R._f32(rng.integers(-9, 9, 100) * R.DENORM)
    got = R.fmaf(a, b, c)
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = hi = F32(float(exact))                                         # Python rounds a Fraction to double correctly; then bracket
        cand = {float(lo), float(np.nextafter(lo, F32(np.inf))), float(np.nextafter(lo, F32(-np.inf)))}
        best = min(cand, key=lambda x: (abs(Fraction(x) - exact), int(F32(x).view(np.uint32)) & 1))
        assert float(got[i]) == best, (i, a[i], b[i], c[i], got[i], best)


def test_adam_emulation_stays_inside_the_bounds(adam_cases):
    total = wild = 0
    for name, tensors in adam_cases.items():
        assert len(tensors) == R.MAX_TENSORS
        for T, emu in zip(tensors, R.adam_emu_case(tensors)):
            bad, off = R.adam_verdict(T, emu)
            assert not bad and off == 0, (name, bad)
            ref = R.adam_ref(T)
            total += T.p.size
            wild += int(ref["wild_p"].sum())
            if T.g is not None and T.lr == 0.0:                            # lr = 0: the reference is p itself and the bound leaves no room for another float
                keep = ~ref["wild_p"] & ~ref["pinned"]
                assert np.all(ref["p"].v[keep] == T.p.ravel()[keep]) and np.all(ref["p"].e[keep] <= R.ulp32(T.p.ravel()[keep]))
    assert total == 21 * 4100 and 0 < wild <= 21 * 6 * 10, (total, wild)    # 6 tensors with a gradient and >= 255 elements, 10 such rows each


def test_adam_trajectory_emulation_stays_inside_the_bounds():
    init, grads, lrs = R.adam_trajectory()
    state = {T.name: T for T in init}
    steps = {T.name: 0 for T in init}
    for it in range(R.TRAJ_STEPS):
        for name, T in state.items():
            g = grads[it][name]
            if g is not None:
                steps[name] += 1
                if T.m is None:
                    T.m, T.v = np.zeros(T.p.shape, F32), np.zeros(T.p.shape, F32)
            T.g, T.lr, T.t = g, lrs[it][name], steps[name]
            emu = R.adam_emu(T)
            bad, off = R.adam_verdict(T, emu)
            assert not bad and off == 0, (it, bad)
            T.p = emu["p"].reshape(T.p.shape)                              # teacher-forced: the float32 state goes on
            if g is not None:
                T.m, T.v = emu["m"].reshape(T.p.shape), emu["v"].reshape(T.p.shape)
    assert steps["w1_257"] == 20 and steps["w1_769"] == 40 and steps["nograd_mid"] == 0


@pytest.mark.parametrize("P", R.ACT_SIZES)
def test_activation_emulation_stays_inside_the_bounds(P):
    q, lo, ls, g_rot, g_op, g_sc = R.activation_case(P)
    assert q.shape == (P, 4) and lo.shape == (P, 1) and ls.shape == (P, 3)
    fwd = R.activations_fwd_emu(q, lo, ls)
    bad, off = R.rot_fwd_verdict(q, fwd["rot"])
    assert not bad and off == 0, bad
    inputs = (q, fwd["op"], fwd["scale"], g_rot, g_op, g_sc)
    bad, off = R.activations_bwd_verdict(inputs, R.activations_bwd_emu(*inputs))
    assert not bad and off == 0, bad
    ref = R.activations_bwd_ref(*inputs)
    if P >= 255:                                                           # the rows built to leave float32's range, and no others
        kind = (np.arange(257) % 8)[257 - P:]
        assert np.array_equal(ref["wild_rot"], kind == 4) and np.array_equal(R.activations_fwd_ref(q, lo, ls)["wild_rot"], kind == 4)
        assert ref["wild_logit"].sum() == 0 and 0 < ref["wild_scale"].sum() <= 3 * P // 10     # exp(89) = inf times a cotangent


def test_adam_reference_is_torch_adam_in_float64():
    rng = np.random.default_rng(4)
    shapes = {"a": (37, 3), "b": (50,), "c": (5, 4)}
    lr = {"a": 1.6e-5, "b": 0.0025, "c": 0.05}
    p0 = {k: rng.standard_normal(s) for k, s in shapes.items()}
    tp = {k: torch.nn.Parameter(torch.tensor(v, dtype=torch.float64)) for k, v in p0.items()}
    w = lambda x: float(F32(x))
    opt = torch.optim.Adam([{"params": [tp[k]], "lr": w(lr[k]), "name": k} for k in shapes], betas=(w(0.9), w(0.999)), eps=w(1e-15),
                           foreach=False)
    mine = {k: R.AdamTensor(k, p0[k].copy(), m=np.zeros(s), v=np.zeros(s)) for k, s in shapes.items()}
    steps = {k: 0 for k in shapes}
    close = lambda a, b: np.all(np.abs(a - b) <= 1e-12 * np.maximum(np.abs(a), np.abs(b)))
    for it in range(12):
        if it == 4:
            lr["b"] = 0.00025
            opt.param_groups[1]["lr"] = w(lr["b"])
        for k, s in shapes.items():
            g = None if (k == "c" and it % 2 == 1) else rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 2)
            tp[k].grad = None if g is None else torch.tensor(g, dtype=torch.float64)
            T = mine[k]
            steps[k] += g is not None
            T.g, T.lr, T.t = g, lr[k], steps[k]
            ref = R.adam_ref(T)
            T.p = ref["p"].v.reshape(s)
            if g is not None:
                T.m, T.v = ref["m"].v.reshape(s), ref["v"].v.reshape(s)
        opt.step()
        for k in shapes:
            st = opt.state[tp[k]]
            assert int(st["step"]) == steps[k], (it, k)
            assert close(mine[k].p, tp[k].detach().numpy()), (it, k)
            assert close(mine[k].m, st["exp_avg"].numpy()) and close(mine[k].v, st["exp_avg_sq"].numpy()), (it, k)
    assert steps == {"a": 12, "b": 12, "c": 6}


def test_activation_reference_is_torch_in_float64():
    q, lo, ls, g_rot, g_op, g_sc = R.activation_case(257)
    ref = R.activations_fwd_ref(q, lo, ls)
    t = lambda x: torch.tensor(np.asarray(x, F64), requires_grad=True)
    tq, tlo, tls = t(q), t(lo), t(ls)
    rot = torch.nn.functional.normalize(tq, p=2, dim=1, eps=R.NORM_EPS)
    op, sc = torch.sigmoid(tlo), torch.exp(tls)
    close = lambda a, b: bool(np.all((np.abs(a - b) <= 1e-12 * np.maximum(np.abs(a), np.abs(b))) | (a == b)))
    assert close(np.stack([e.v for e in ref["rot"]], 1), rot.detach().numpy())
    assert close(ref["op"], op.detach().numpy()) and close(ref["scale"], sc.detach().numpy())
    # backward on the forward's float32 outputs: torch's autograd of sigmoid / exp is g s (1 - s) / g e on ITS outputs, so feed
    # the reference torch's float64 outputs here
    (rot * t(g_rot).detach()).sum().backward()
    (op * t(g_op).detach()).sum().backward()
    (sc * t(g_sc).detach()).sum().backward()
    with np.errstate(all="ignore"):
        b = R.activations_bwd_ref(q, op.detach().numpy(), sc.detach().numpy(), g_rot, g_op, g_sc)
    ok = np.isfinite(tq.grad.numpy()).all(1)
    got = np.stack([e.v for e in b["d_rot"]], 1)
    # d = (g - y (y.g)) / n cancels for a cotangent parallel to q: torch's own float64 rounding is relative to |g| / |q| there
    scale = np.linalg.norm(g_rot.astype(F64), axis=1, keepdims=True) / np.maximum(np.linalg.norm(q.astype(F64), axis=1, keepdims=True), R.NORM_EPS)
    assert np.all(np.abs(got - tq.grad.numpy())[ok] <= 1e-12 * np.broadcast_to(scale, got.shape)[ok])
    fin = np.isfinite(tls.grad.numpy().ravel())
    assert close(b["d_logit"].v, tlo.grad.numpy().ravel()) and close(b["d_log_scale"].v[fin], tls.grad.numpy().ravel()[fin])


def _first_violation(cases, mutant):
    for name, tensors in cases.items():
        for T, emu in zip(tensors, R.adam_emu_case(tensors, mutant=mutant)):
            bad, _ = R.adam_verdict(T, emu)
            if bad:
                return name, bad[0]
    return None


@pytest.mark.parametrize("mutant, where", [
    ("step_minus_1", "t1100_"),                 # the step count off by one at t = 1100
    ("eps_1e-8", None),
    ("flush_denormal_g", None),
    ("pin_mod_rows", None),
    ("fused_beta2_v", "mixed"),
    ("neighbour_inv_bc2", "mixed"),
])
def test_adam_mutants_leave_the_bounds(adam_cases, mutant, where):
    cases = {k: v for k, v in adam_cases.items() if where is None or k.startswith(where)}
    hit = _first_violation(cases, mutant)
    assert hit is not None, f"mutant {mutant} passes every case {list(cases)}"
    print(mutant, "caught by case", *hit)


@pytest.mark.parametrize("mutant", R.MUTANTS_ACT)
def test_activation_mutants_leave_the_bounds(mutant):
    hits = []
    for P in R.ACT_SIZES:
        q, lo, ls, g_rot, g_op, g_sc = R.activation_case(P)
        fwd = R.activations_fwd_emu(q, lo, ls)
        inputs = (q, fwd["op"], fwd["scale"], g_rot, g_op, g_sc)
        bad, _ = R.activations_bwd_verdict(inputs, R.activations_bwd_emu(*inputs, mutant=mutant))
        if bad:
            hits.append((P, bad[0]))
    assert hits, f"mutant {mutant} passes every activation case"
    print(mutant, "caught by case P =", *hits[0])


def test_exact_references_of_the_sums():
    x = R.sum_case(7, 1025)
    assert R.sum_views_ref(x).dtype == F32 and not np.array_equal(R.sum_views_ref(x), x.astype(F64).sum(0).astype(F32))   # order matters
    assert np.array_equal(R.sum_views_ref(x[:1]), x[0])
    for name, (attr, quads, father, weight) in R.dense_cases().items():
        out = R.dense_interp_ref(attr, quads, father, weight)
        assert out.dtype == F32 and out.shape == (len(attr) + len(father), attr.shape[1]), name
        for d in range(0, len(father), 37):                                # the statement, spelled out row by row
            s = np.zeros(attr.shape[1], F64)
            for k in range(4):
                s = s + attr[quads[father[d], k]].astype(F64) * weight[d, k]
            assert np.array_equal(out[len(attr) + d], s.astype(F32)), (name, d)
