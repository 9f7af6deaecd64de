"""CPU: the per-pixel yardstick of the photometric loss (tests/photo_cases.py) - its explicit float64 adjoint against float64
autograd through its own forward, its tie to the G3-pinned restatement (oracle/loss_oracle.py) and to golden G3 itself, the
conditions the cases were built under (decision margin, ties, pixels of scale 0), the recorded float32 yardstick against a live
measurement, the float32 restatement under the checker and under the suite's earlier 5e-5-of-the-maximum form, and two mutations
the checker has to reject."""
import os

import numpy as np
import pytest
import torch

from oracle import loss_oracle
from tests import photo_cases as PC

CASES = [(n, s) for n in PC.NAMES for s in PC.SHAPES]
IDS = [f"{n}-{s[0]}x{s[1]}" for n, s in CASES]
_R32 = {}


def restatement32(name, shape, variant="unit"):
    k = (name, shape, variant)
    if k not in _R32:
        _R32[k] = PC.restatement32(PC.prepared(name, shape, variant)[0])
    return _R32[k]


def _f64(t):
    return None if t is None else t.double()


@pytest.mark.parametrize("variant", ["unit", "scaled"])
@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_explicit_adjoint_equals_float64_autograd(name, shape, variant):
    """To 1e-11 of max|t|, per tensor; the loss to 1e-14."""
    c, t = PC.prepared(name, shape, variant)
    im = c.im.double().requires_grad_(True)
    zeros = torch.zeros(PC.V, 3, dtype=torch.float64)          # without an affine: the gradient an identity affine would receive
    cm = (zeros if c.cam_m is None else c.cam_m.double()).clone().requires_grad_(True)
    cc = (zeros if c.cam_c is None else c.cam_c.double()).clone().requires_grad_(True)
    l = PC.forward(im, c.gt.double(), cm, cc)
    (l * c.weight.double()).sum().backward()
    assert np.abs(l.detach().numpy() - t.loss).max() <= 1e-14
    for got, want in ((im.grad, t.d_im), (cm.grad, t.d_m), (cc.grad, t.d_c)):
        assert np.abs(got.numpy() - want).max() <= 1e-11 * np.abs(want).max()
    assert (t.s >= 0).all() and (np.abs(t.d_im) <= t.s * (1 + 1e-12)).all()       # the scale bounds the truth: magnitudes of its terms
    assert (np.abs(t.d_c) <= t.s_c * (1 + 1e-12)).all() and (np.abs(t.d_m) <= t.s_m * (1 + 1e-12)).all()


@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_forward_with_the_float64_window_is_the_pinned_restatement(name, shape):
    c, _ = PC.prepared(name, shape)
    l = PC.forward(c.im.double(), c.gt.double(), _f64(c.cam_m), _f64(c.cam_c), win=PC.window64(), c1=loss_oracle.C1, c2=loss_oracle.C2)
    for v in range(PC.V):
        cam = () if c.cam_m is None else (c.cam_m[v].double(), c.cam_c[v].double())
        ref = loss_oracle.photometric_loss_torch(c.im[v].double(), c.gt[v].double(), *cam)
        assert abs(float(l[v]) - float(ref)) <= 1e-12


def test_truth_reproduces_golden_g3():
    """G3's own tolerances (tests/test_golden_boundary.py): loss 1e-6, gradient rtol 1e-4 + atol 1e-9 per element."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g3_photometric.npz"))
    for i in range(3):
        t = PC.adjoint(torch.tensor(g[f"im{i}"])[None], torch.tensor(g[f"gt{i}"])[None], None, None, torch.ones(1))
        assert abs(t.loss[0] - float(g[f"loss_{i}"])) < 1e-6
        np.testing.assert_allclose(t.d_im[0], g[f"grad{i}"], rtol=1e-4, atol=1e-9)


def test_window_and_constants_are_the_float32_ones():
    w = PC.window32()
    assert torch.equal(w, loss_oracle.gaussian_window_1d(torch.float32).double())
    assert torch.equal(w.float().double(), w) and not torch.equal(w, PC.window64())
    assert PC.C1_32 == float(torch.tensor(0.0, dtype=torch.float32) + 0.01 ** 2) != 0.01 ** 2
    assert PC.C2_32 == float(torch.tensor(0.0, dtype=torch.float32) + 0.03 ** 2) != 0.03 ** 2


@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_decision_margin_and_tie_counts(name, shape):
    c, t = PC.prepared(name, shape)
    margin, tie = PC.sign_margin(c)
    assert margin >= PC.SIGN_ULPS, margin
    assert np.array_equal(tie, t.ties)
    for cam in (c.cam_m, c.cam_c):
        assert cam is None or (float(cam.abs().max()) <= (0.1 if cam is c.cam_m else 0.05))
    if name in PC.TIE_CASES:
        assert np.array_equal(tie, c.tie_ok.numpy())                     # ties: the shared background and nothing else
        assert not c.im[c.tie_ok].any() and not c.gt[c.tie_ok].any()
        assert tie.sum() >= 1000 and (t.s == 0).sum() >= 1000, (int(tie.sum()), int((t.s == 0).sum()))
        assert not (t.s == 0)[~tie].any()
        assert c.cam_m is None or not (c.cam_m.any() or c.cam_c.any())
        if name == "converged":
            assert float((c.im - c.gt).abs().max()) <= 0.002 + 1e-5
        if name == "masked_step":
            b, _ = PC.prepared("black_bg", shape)
            assert torch.equal(c.im, b.im) and torch.equal(c.tie_ok, b.tie_ok)
            stepped = c.gt != b.gt
            assert torch.equal(c.gt[stepped], b.gt[stepped] * 0.1) and 0.05 < float(stepped[~c.tie_ok].float().mean()) < 0.8
        if name == "identity_affine":
            b, _ = PC.prepared("black_bg", shape)
            assert torch.equal(c.im, b.im) and torch.equal(c.gt, b.gt)
    else:
        assert not tie.any() and (t.s > 0).all()
        assert c.cam_m is not None and c.cam_m.abs().min() > 0 and c.cam_c.abs().min() > 0
    if name == "out_of_range":
        assert c.im.min() < -0.15 and c.im.max() > 1.45
    if name == "anti" and shape[0] > 2 * PC.R + 1:       # (on 7 rows every window holds the zero padding of both images: s12 > 0)
        conv = PC._conv(shape, PC.window32())
        x, _ = PC._affine(c.im.double(), c.cam_m.double(), c.cam_c.double())
        mu1, mu2, A1, A2, B1, B2, S = PC._maps(x, c.gt.double(), conv, PC.C1_32, PC.C2_32)
        assert float((A2 < 0).double().mean()) > 0.5 and float((S < 0).double().mean()) > 0.5


def test_weight_variants():
    assert PC.WEIGHTS == {"unit": (1.0, 1.0), "scaled": (0.5, 2.0), "zero_neg": (0.0, -1.5)}
    c, t = PC.prepared("identity_affine", PC.SHAPES[0], "zero_neg")
    assert not t.s[0].any() and not t.d_im[0].any() and not t.s_m[0].any() and not t.s_c[0].any()
    u = PC.prepared("identity_affine", PC.SHAPES[0])[1]
    assert (np.abs(t.d_im[1] + 1.5 * u.d_im[1]) <= 1e-13 * t.s[1]).all() and (np.abs(t.s[1] - 1.5 * u.s[1]) <= 1e-13 * t.s[1]).all()
    assert np.array_equal(t.loss, u.loss)                                # the weight is dL/dloss[v]: the loss does not carry it


@pytest.mark.parametrize("name,shape", CASES, ids=IDS)
def test_recorded_yardstick_is_the_live_float32_restatement(name, shape, capsys):
    """Within a factor 2, either way, of the recorded table; the restatement passes the checker with a ratio of at most 1 of its
    own yardstick (margin 2 for that factor)."""
    c, t = PC.prepared(name, shape)
    live = PC.ratios(t, *restatement32(name, shape))
    q_im, q_m, q_c, q_loss = PC.Q32[(name, shape)]
    with capsys.disabled():
        print(f"\n{name} {shape[0]}x{shape[1]}: fp32 restatement err / s  im {live['im']:.2e} (recorded {q_im:.2e})  cam_m "
              f"{live['m'] or 0:.2e} ({q_m:.2e})  cam_c {live['c'] or 0:.2e} ({q_c:.2e})  loss {live['loss']:.1e} ({q_loss:.1e})")
    assert q_im / 2 <= live["im"] <= q_im * 2
    if c.cam_m is not None:
        assert q_m / 2 <= live["m"] <= q_m * 2 and q_c / 2 <= live["c"] <= q_c * 2
    else:
        assert q_m == 0 and q_c == 0
    assert live["stray"] == 0
    r = PC.check(c, *restatement32(name, shape), margin=2.0)
    assert r["im"] <= 2 * q_im


def test_float32_restatement_fails_the_earlier_form_on_bright_flat():
    """5e-5 of the tensor's largest entry (tests/test_gpu_photometric.py) cannot be asked of such inputs: the reference's own
    float32 arithmetic misses it, while it is within its recorded yardstick of every pixel's scale."""
    shape = PC.SHAPES[0]
    c, t = PC.prepared("bright_flat", shape)
    _, g, _, _ = restatement32("bright_flat", shape)
    assert np.abs(g - t.d_im).max() > 5e-5 * np.abs(t.d_im).max()
    n, tn = PC.prepared("noise", shape)
    assert np.abs(restatement32("noise", shape)[1] - tn.d_im).max() <= 5e-5 * np.abs(tn.d_im).max()
    # what the per-tensor form hides: a pixel's own scale against the largest gradient of the tensor, inside the face
    b, tb = PC.prepared("black_bg", shape)
    inside = ~b.tie_ok.numpy()
    assert np.mean(np.abs(tb.d_im[inside]) < 0.05 * np.abs(tb.d_im).max()) > 0.1


# ---- mutations: the checker can fail ------------------------------------------------------------------------------------
def _sign_of_zero_is_plus(name, shape):
    """The float32 restatement with sign(0) = +1: every tie receives +0.8 w / N."""
    c, t = PC.prepared(name, shape)
    l, g, gm, gc = restatement32(name, shape)
    n = 3 * shape[0] * shape[1]
    g = g + (np.float32(0.8) * c.weight.numpy()[:, None, None, None] / np.float32(n)) * t.ties
    return c, (l, g, gm, gc)


def _d1_shifted_in_the_border_band(name, shape):
    """The float32 restatement plus the effect, in float64, of a D1 map read one column off inside the outer 5-pixel band."""
    c, t = PC.prepared(name, shape)
    H, W = shape
    band = torch.ones(H, W, dtype=torch.bool)
    band[PC.R:H - PC.R, PC.R:W - PC.R] = False
    m = PC.adjoint(c.im, c.gt, c.cam_m, c.cam_c, c.weight, mutate_d1=lambda d: torch.where(band, torch.roll(d, 1, -1), d))
    l, g, gm, gc = restatement32(name, shape)
    cam = (None, None) if gm is None else ((gm + (m.d_m - t.d_m)).astype(np.float32), (gc + (m.d_c - t.d_c)).astype(np.float32))
    return c, (l, (g + (m.d_im - t.d_im)).astype(np.float32), *cam)


@pytest.mark.parametrize("mutation", [_sign_of_zero_is_plus, _d1_shifted_in_the_border_band], ids=["sign0", "d1_shift"])
def test_checker_rejects_the_mutation(mutation, capsys):
    rejected = []
    for name in PC.NAMES:
        c, result = mutation(name, PC.SHAPES[0])
        try:
            PC.check(c, *result)
        except AssertionError:
            rejected.append(name)
    with capsys.disabled():
        print(f"\nmutation {mutation.__name__}: rejected on {rejected}")
    assert rejected
    if mutation is _sign_of_zero_is_plus:
        assert sorted(rejected) == sorted(PC.TIE_CASES)                  # exactly the cases that have ties
    else:
        # (the tie cases' border band is background: D1 == 0 there and the shift moves nothing)
        assert sorted(rejected) == sorted(n for n in PC.NAMES if n not in PC.TIE_CASES)
