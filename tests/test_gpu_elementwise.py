"""
The per-iteration kernels of csrc/t4d_optim.hip element by element on an MI355X, against tests/elementwise_ref.py (float64
references, derived bounds, the exact float32 emulation of the documented operation order, the case lists; its soundness,
anchor and sensitivity are proved on the CPU in tests/test_elementwise_host.py):

  * k_adam_pin<false>: teacher-forced single steps through FusedAdamPins (the test sets exp_avg, exp_avg_sq and step = t - 1) of 12
    tensors - 1 .. 769 elements, widths 1 / 3 / 4 / 48, an empty (0, 3) tensor in the middle, tensors without gradient first, in
    the middle and last, pins on the first / last / every / no row and on a tensor without gradient, one clear_grad tensor - at
    t in {1, 2, 10, 1100, 100000} x lr in {0, 1.6e-5, 0.0025, 0.05} and one launch that mixes them; gradients normal, log-uniform
    1e-12 .. 1e8, denormal, zero, +-inf / NaN / 1e20; consistent and inconsistent moments.  EVERY element of p, m, v under the
    float64 bound and bit-equal to the emulation; lr = 0 leaves p's bits; gradients zeroed exactly where clear_grad says;
  * a 40-step trajectory (learning-rate changes, a tensor on alternate steps), each step held to the reference from the kernel's
    own previous float32 state; k_adam_pin<true> (capturable) over the same 40 steps bit-equal to it, every workgroup's counter
    equal to its tensor's step count, then one step from counters filled with 1099; apply_pins() alone;
  * k_activate_fwd / k_activate_bwd at P in {1, 255, 256, 257} on saturating, denormal and overflowing inputs, clamped and
    cancelling quaternion rows, and every NULL cotangent / NULL output combination;
  * k_sum_views bit-equal to the sequential float32 sum at V in {1, 2, 7, 24}, n in {1 .. 4100}, misaligned views, NULL slots,
    canaries; k_dense_interp bit-equal to the float64 left-to-right sum.

MEASURED on an MI355X (the figures the tests print):

  * Adam: elements of p, m, v not bit-equal to the emulation: 0 of the 86100 of the 21 single-step cases and 0 over the 41
    trajectory steps, host- and device-counted (division and square root are correctly rounded, nothing is contracted; the
    device's double pow gives the host's bias corrections at every step count tried).  The normalisation forward and all three
    backwards are bit-equal to the emulation as well (0 elements differ);
  * device expf against float64, in float32 ulps over the case list: exp 0.688, sigmoid 1.407; asserted at the next whole ulp
    plus one (EXP_ULP = 2, SIGMOID_ULP = 3 below), the margin because the list samples the float range and does not exhaust it;
  * FINDING, explained and not adopted as a tolerance: for a logit below -88.7228 (= -log FLT_MAX) expf(-x) is +inf and
    1 / (1 + expf(-x)) returns 0 where the exact sigmoid is a float32 denormal (2.7e-39 at -88.8): about 2e6 denormal ulps, an
    absolute error below 2^-126.  torch's float32 sigmoid computes the same expression and returns the same 0, so the kernel
    stands as the reference has it; those logits are held to exactly 0 (`flushed`) and every other logit to SIGMOID_ULP.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import elementwise_ref as R
from topo4d_amd import _lib, boundary
from topo4d_amd._lib import ptr
from topo4d_amd.optim import FusedAdamPins

pytestmark = pytest.mark.gpu

F32 = np.float32
EXP_ULP = 2.0          # measured 0.688 against float64 (module docstring): next whole ulp + 1
SIGMOID_ULP = 3.0      # measured 1.407


def dev(x, dtype=None):
    x = np.asarray(x, dtype)
    return torch.from_numpy(np.ascontiguousarray(x)).reshape(x.shape).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy().ravel()


@pytest.fixture(scope="module")
def adam_cases():
    return R.adam_cases()


def make_optimiser(tensors, capturable=False):
    """FusedAdamPins over the case's tensors in layout order, pins set; returns (optimiser, {name: Parameter})."""
    params = {T.name: torch.nn.Parameter(dev(T.p)) for T in tensors}
    opt = FusedAdamPins([{"params": [params[T.name]], "name": T.name, "lr": T.lr} for T in tensors], eps=R.EPS, betas=R.BETAS,
                        capturable=capturable)
    for T in tensors:
        if T.pin_mask is not None:
            opt.set_pin(T.name, dev(T.pin_mask), dev(T.pin_values[T.pin_mask]))
    return opt, params


def force(opt, params, tensors):
    """Teacher-forcing: the optimiser's state, gradients and learning rates as the case has them (step = t - 1 before the call)."""
    opt.clear_grad = {T.name for T in tensors if T.clear_grad}
    for T, grp in zip(tensors, opt.param_groups):
        p = params[T.name]
        grp["lr"] = T.lr
        p.grad = None if T.g is None else dev(T.g)
        if T.m is not None:
            opt.state[p] = {"exp_avg": dev(T.m), "exp_avg_sq": dev(T.v), "step": (T.t - 1) if T.g is not None else 5}


def read(opt, params, T):
    st = opt.state.get(params[T.name], {})
    return {"p": host(params[T.name]), "m": host(st.get("exp_avg")), "v": host(st.get("exp_avg_sq")), "grad_after": host(params[T.name].grad)}


# ------------------------------------------------------------------------------------------------------------------------------
# Adam + pins
# ------------------------------------------------------------------------------------------------------------------------------
CASE_NAMES = [f"t{t}_lr{lr:g}" for t in R.ADAM_STEPS for lr in R.ADAM_LRS] + ["mixed"]


@pytest.mark.parametrize("case", CASE_NAMES)
def test_adam_single_step_per_element(adam_cases, case):
    tensors = adam_cases[case]
    opt, params = make_optimiser(tensors)
    force(opt, params, tensors)
    opt.step()
    torch.cuda.synchronize()
    bad, off, steps = [], 0, opt.steps()
    for k, T in enumerate(tensors):
        got = read(opt, params, T)
        b, o = R.adam_verdict(T, got)
        bad += b
        off += o
        if T.g is not None:
            assert steps[k] == T.t, (T.name, steps[k])
            if T.lr == 0.0:                                  # lr = 0: every element whose reference update is finite keeps its bits
                ref = R.adam_ref(T)
                keep = ~ref["wild_p"] & ~ref["pinned"]
                assert np.all(R.same_bits(got["p"], T.p.ravel())[keep]), T.name
        else:
            assert steps[k] == (5 if T.m is not None else 0), (T.name, steps[k])
    print(f"{case}: {off} elements not bit-equal to the emulation, {len(bad)} outside the float64 bound")
    assert not bad, bad[:6]
    assert off == 0


def test_clear_grad_needs_a_gradient_it_can_zero_in_place():
    """T4D_ADAM_CLEAR_GRAD promises zeros in p.grad.  A non-contiguous p.grad would be copied for the launch and the COPY zeroed:
    FusedAdamPins refuses it with a ValueError (zeroing it in place afterwards would cost the launch the flag exists to save).
    Without the flag a non-contiguous gradient is taken as before and left as it is."""
    g = np.random.default_rng(2)
    p0, g0 = R._f32(g.standard_normal((40, 3))), R._f32(g.standard_normal((3, 40)))
    res = []
    for contiguous in (True, False):
        p = torch.nn.Parameter(dev(p0))
        opt = FusedAdamPins([{"params": [p], "name": "a", "lr": 0.01}], eps=R.EPS)
        p.grad = dev(g0.T.copy()) if contiguous else dev(g0).t()
        assert p.grad.is_contiguous() == contiguous
        opt.step()
        assert torch.equal(p.grad, dev(g0.T.copy()))
        res.append(p.detach().clone())
    assert torch.equal(res[0], res[1])
    T = R.AdamTensor("a", p0, g0.T.copy(), np.zeros_like(p0), np.zeros_like(p0), lr=0.01, t=1)
    bad, off = R.adam_verdict(T, {"p": host(res[1]), "m": host(opt.state[p]["exp_avg"]), "v": host(opt.state[p]["exp_avg_sq"]),
                                  "grad_after": host(p.grad.contiguous())})
    assert not bad and off == 0, bad
    p = torch.nn.Parameter(dev(p0))
    opt = FusedAdamPins([{"params": [p], "name": "a", "lr": 0.01}], eps=R.EPS)
    opt.clear_grad = {"a"}
    p.grad = dev(g0).t()
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    assert torch.equal(p.detach(), dev(p0)) and torch.equal(p.grad, dev(g0).t())      # refused before anything ran
    p.grad = dev(g0.T.copy())
    opt.step()
    assert not p.grad.any() and torch.equal(p.detach(), res[0])


def _counters(opt):
    first, n = opt._counter_layout()
    flat = opt._step_dev.cpu().numpy()
    return [flat[f:(first[k + 1] if k + 1 < len(first) else n)] for k, f in enumerate(first)]


def test_adam_trajectory_host_and_device_counted():
    init, grads, lrs = R.adam_trajectory()
    opt_h, ph = make_optimiser(init)
    opt_c, pc = make_optimiser(init, capturable=True)
    state = {T.name: T for T in init}                       # the kernel's own float32 state, read back after every step
    steps = {T.name: 0 for T in init}
    bad, off = [], 0

    def one_step(it, step_g, step_lr, t_of):
        nonlocal bad, off
        for opt, params in ((opt_h, ph), (opt_c, pc)):
            for T, grp in zip(init, opt.param_groups):
                grp["lr"] = step_lr[T.name]
                params[T.name].grad = None if step_g[T.name] is None else dev(step_g[T.name])
            opt.step()
        for T in init:
            g = step_g[T.name]
            if g is not None and T.m is None:
                T.m, T.v = np.zeros(T.p.shape, F32), np.zeros(T.p.shape, F32)
            T.g, T.lr, T.t = g, step_lr[T.name], t_of(T.name)
            got = read(opt_h, ph, T)
            b, o = R.adam_verdict(T, got)
            bad += [f"step {it}: {x}" for x in b]
            off += o
            sc = opt_c.state.get(pc[T.name], {})
            assert torch.equal(pc[T.name], ph[T.name]), (it, T.name)
            if g is not None:
                sh = opt_h.state[ph[T.name]]
                assert torch.equal(sc["exp_avg"], sh["exp_avg"]) and torch.equal(sc["exp_avg_sq"], sh["exp_avg_sq"]), (it, T.name)
                T.m, T.v = got["m"].reshape(T.p.shape), got["v"].reshape(T.p.shape)
            T.p = got["p"].reshape(T.p.shape)

    for it in range(R.TRAJ_STEPS):
        for name, g in grads[it].items():
            steps[name] += g is not None
        one_step(it, grads[it], lrs[it], lambda name: steps[name])
    # every workgroup's own counter equals its tensor's step count; a tensor without gradient never advanced
    assert steps["w1_257"] == 20 and steps["w1_769"] == 40 and steps["nograd_first"] == 0
    want = [steps[T.name] if T.p.size else 0 for T in init]
    assert opt_h.steps() == [steps[T.name] for T in init] and opt_c.steps() == want
    for T, cnt in zip(init, _counters(opt_c)):
        assert len(cnt) == (T.p.size + 255) // 256 and np.all(cnt == steps[T.name]), (T.name, cnt)
    assert len(_counters(opt_c)[7]) == 4 and len(_counters(opt_c)[5]) == 3          # 769 and 768 elements: 4 and 3 workgroups
    # from step count 1099 on both sides: one more step, bit-equal and inside the float64 bound at t = 1100
    opt_c._step_dev.fill_(1099)
    for p in ph.values():
        if p in opt_h.state:
            opt_h.state[p]["step"] = 1099
    one_step("1100", grads[0], lrs[0], lambda name: 1100)
    for T, cnt in zip(init, _counters(opt_c)):
        assert np.all(cnt == (1100 if grads[0][T.name] is not None else 1099)), (T.name, cnt)
    print(f"trajectory: {off} elements not bit-equal to the emulation, {len(bad)} outside the float64 bound")
    assert not bad, bad[:6]
    assert off == 0
    # apply_pins() alone: pinned rows written, every other element and all optimiser state bit-unchanged, no counter advanced
    with torch.no_grad():
        for p in pc.values():
            p.add_(1.0)
    before = {T.name: read(opt_c, pc, T) for T in init}
    cnt_before = opt_c._step_dev.clone()
    opt_c.apply_pins()
    torch.cuda.synchronize()
    assert torch.equal(opt_c._step_dev, cnt_before)
    for T in init:
        after, pinned = read(opt_c, pc, T), R._pinned(T)
        want_p = np.where(pinned, T.pin_values.ravel(), before[T.name]["p"]) if T.pin_mask is not None else before[T.name]["p"]
        assert np.all(R.same_bits(after["p"], want_p)), T.name
        for key in ("m", "v"):
            assert (after[key] is None) == (before[T.name][key] is None)
            assert after[key] is None or np.all(R.same_bits(after[key], before[T.name][key])), (T.name, key)


# ------------------------------------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", R.ACT_SIZES)
def test_activations_per_element(P):
    q, lo, ls, g_rot, g_op, g_sc = R.activation_case(P)
    rot, op, sc = boundary.activate_forward(dev(q), dev(lo), dev(ls))
    ref = R.activations_fwd_ref(q, lo, ls)
    bad, off = R.rot_fwd_verdict(q, host(rot).reshape(P, 4))
    flushed = lo.ravel() < -R.EXP_OVERFLOW                  # expf(-x) = +inf: 1 / (1 + inf) = 0 (module docstring, FINDING)
    assert np.all(host(op)[flushed] == 0.0)
    sig_ulp = R.ulp_error(host(op), ref["op"].ravel())[~flushed].max(initial=0.0)
    exp_ulp = R.ulp_error(host(sc), ref["scale"].ravel()).max()
    print(f"P={P}: device sigmoid {sig_ulp:.3f} ulp, exp {exp_ulp:.3f} ulp against float64; normalize: {off} elements not bit-equal "
          f"to the emulation, {len(bad)} outside the bound")
    assert not bad, bad[:6]
    assert sig_ulp <= SIGMOID_ULP and exp_ulp <= EXP_ULP
    d_ur, d_lo, d_ls = boundary.activate_backward(dev(q), op, sc, dev(g_rot), dev(g_op), dev(g_sc))
    inputs = (q, host(op).reshape(P, 1), host(sc).reshape(P, 3), g_rot, g_op, g_sc)      # the forward's OWN float32 outputs
    got = {"d_rot": host(d_ur).reshape(P, 4), "d_logit": host(d_lo), "d_log_scale": host(d_ls)}
    bad, off = R.activations_bwd_verdict(inputs, got)
    print(f"P={P}: backward: {off} elements not bit-equal to the emulation, {len(bad)} outside the bound")
    assert not bad, bad[:6]


def test_activation_backward_null_combinations():
    """Every NULL cotangent / NULL output combination activate_backward(need=...) allows: a missing cotangent counts as zeros, an
    output that is not needed is not written (None), and what IS computed has the bits of the full call."""
    P = 257
    q, lo, ls, g_rot, g_op, g_sc = R.activation_case(P)
    dq = dev(q)
    rot, op, sc = boundary.activate_forward(dq, dev(lo), dev(ls))
    cot = (dev(g_rot), dev(g_op), dev(g_sc))
    full = boundary.activate_backward(dq, op, sc, *cot)
    same = lambda a, b: bool(np.all(R.same_bits(host(a), host(b))))
    for have in range(8):
        c = [cot[k] if have >> k & 1 else None for k in range(3)]
        for need_bits in range(8):
            need = tuple(bool(need_bits >> k & 1) for k in range(3))
            out = boundary.activate_backward(dq, op, sc, *c, need=need)
            for k in range(3):
                if not need[k]:
                    assert out[k] is None
                elif c[k] is None:
                    assert out[k].shape == full[k].shape and not out[k].any(), (have, need, k)
                else:
                    assert same(out[k], full[k]), (have, need, k)


# ------------------------------------------------------------------------------------------------------------------------------
# view sums
# ------------------------------------------------------------------------------------------------------------------------------
CANARY = 12345.0


def _sum_call(V, slots):
    """slots: list of (src pointer or None, dst pointer or None, n) in T4D_SUM_MAX_TENSORS entries."""
    n = len(slots)
    src = (C.c_void_p * n)(*[s for s, _, _ in slots])
    dst = (C.c_void_p * n)(*[d for _, d, _ in slots])
    cnt = (C.c_int64 * n)(*[c for _, _, c in slots])
    _lib.call("t4d_sum_views", V, n, src, dst, cnt, _lib.stream(torch.device("cuda", torch.cuda.current_device())))


@pytest.mark.parametrize("V", R.SUM_VIEWS)
def test_sum_views_bit_equal_to_the_sequential_sum(V):
    items = []                                              # (name, src view, dst buffer, dst view, expected)
    for n in R.SUM_N:
        x = R.sum_case(V, n)
        buf = torch.full((n + 1,), CANARY, device="cuda")
        items.append((f"n{n}", dev(x), buf, buf[:n], R.sum_views_ref(x)))
    x = R.sum_case(V, 1024)
    sbuf = torch.zeros(V * 1024 + 1, device="cuda")
    sbuf[1:] = dev(x).ravel()
    buf = torch.full((1025,), CANARY, device="cuda")
    items.append(("src_off_by_one_float", sbuf[1:], buf, buf[:1024], R.sum_views_ref(x)))
    x = R.sum_case(V, 4096)
    buf = torch.full((4098,), CANARY, device="cuda")
    items.append(("dst_off_by_one_float", dev(x), buf, buf[1:4097], R.sum_views_ref(x)))
    for name, s, _, d, _ in items:
        assert (s.data_ptr() % 16 != 0) == (name == "src_off_by_one_float") and (d.data_ptr() % 16 != 0) == (name == "dst_off_by_one_float")
    slot = lambda i: (items[i][1].data_ptr(), items[i][3].data_ptr(), items[i][3].numel())
    dummy = torch.full((8,), CANARY, device="cuda")
    assert R.SUM_MAX_TENSORS == 8
    _sum_call(V, [slot(0), (None, None, 7), slot(1), slot(2), (None, dummy.data_ptr(), 4), slot(3), slot(4), slot(5)])
    _sum_call(V, [slot(6), slot(7), (dummy.data_ptr(), None, 4), slot(8), slot(9), (dummy.data_ptr(), dummy.data_ptr(), 0), slot(10),
                  (None, None, 0)])
    torch.cuda.synchronize()
    assert torch.all(dummy == CANARY)
    for name, _, buf, d, want in items:
        assert np.all(R.same_bits(host(d), want)), (V, name)
        rest = torch.ones_like(buf, dtype=torch.bool)
        off = (d.data_ptr() - buf.data_ptr()) // 4
        rest[off:off + d.numel()] = False
        assert torch.all(buf[rest] == CANARY), (V, name)
    assert np.array_equal(host(items[5][3]), host(items[9][3]))         # the misaligned source: the aligned call's bits


# ------------------------------------------------------------------------------------------------------------------------------
# dense interpolation
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["w1", "w3", "w4", "no_dense", "nothing"])
def test_dense_interpolation_bit_equal_to_the_float64_sum(case):
    attr, quads, father, weight = R.dense_cases()[case]
    want = R.dense_interp_ref(attr, quads, father, weight)
    width = attr.shape[1]
    n = want.size
    out = torch.full((n + 1,), CANARY, device="cuda")
    a = dev(attr) if attr.size else torch.full((4,), CANARY, device="cuda")      # an empty tensor has no storage to point at
    dq, df, dw = dev(quads), dev(father), dev(weight)
    _lib.call("t4d_dense_interpolate", ptr(a), ptr(dq), ptr(df) if len(father) else None,
              ptr(dw) if len(father) else None, attr.shape[0], len(father), width, ptr(out),
              _lib.stream(torch.device("cuda", torch.cuda.current_device())))
    torch.cuda.synchronize()
    assert np.all(R.same_bits(host(out[:n]), want.ravel())) and float(out[n]) == CANARY, case
