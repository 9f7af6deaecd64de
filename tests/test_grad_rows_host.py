"""CPU: the per-Gaussian gradient yardstick of tests/grad_rows.py, validated on the two oracles.

  * the sign-flipped backward passes that share one forward graph (oracle/torch_oracle.rasterize_with_grads, extra_cotangents)
    return bit for bit what separate calls return;
  * every (case, cotangent kind) the kernels are held to in tests/test_gpu_grad_rows.py meets the SELECTION CONDITION - the fp32
    C oracle and the float64 oracle agree on radii and on n_contrib at every pixel - and on it the fp32 C oracle, which shares
    every formula with the kernels, passes the row check; each test prints the reference's worst err / S_i per tensor and view;
  * three corruptions of the C oracle's gradients that tests/test_gpu_parity.check_grads accepts and the row check rejects.

Measured on the committed cases (36 views; C oracle built -O3 -march=native -ffp-contract=off, run on one OpenMP thread): the
reference's worst err / S_i is 8.8e-5 (one_view128/depth, scales), so GRAD_REL = 2e-4 leaves the kernels 2.3 x the fp32
reference's own worst row; per tensor in RESULTS in the docstring of tests/test_gpu_grad_rows.py.
"""
import numpy as np
import pytest
import torch

from tests import grad_rows as GR, util
from tests.test_gpu_parity import check_grads


def as_views(g):
    """A per-view gradient dict (the C oracle's) in the [V, P, ...] layout check_grads and check_grads_rowwise index."""
    return {k: np.asarray(a)[None] for k, a in g.items()}


def test_backward_passes_over_one_forward_equal_separate_calls():
    rv, cams = util.make_scene(6, 8, 40, 56, 1, opacity="B", seed=3)
    rv = GR.anisotropic(rv, 3)
    cot = tuple(t[0] for t in GR.cotangents("mixed", 1, 40, 56, 4))
    extra = [GR.sign_flipped(cot, 0), (cot[0], None, None), (torch.zeros_like(cot[0]), None, cot[2])]
    outs, g, more = util.torch_oracle_render(cams[0], rv, *cot, extra_cotangents=extra)
    assert len(more) == len(extra)
    for c, got in zip([cot] + extra, [g] + more):
        _, want = util.torch_oracle_render(cams[0], rv, *c)
        assert set(want) == set(got)
        for k in want:
            assert torch.equal(want[k], got[k]), k
    assert any(bool((more[0][k] != g[k]).any()) for k in g)                       # the flipped signs do reach the backward
    _, _, none = util.torch_oracle_render(cams[0], rv, *cot, extra_cotangents=[])
    assert none == []


def test_the_cases_are_what_the_row_check_needs():
    assert set(GR.CASES["head96_B"].kinds) == set(GR.KINDS)
    for c in GR.CASES.values():
        assert "mixed" in c.kinds and len(c.kinds) >= 2, c.name
        rv, cams = c.make()
        if c.name.startswith("corners") or "scales" not in rv:
            continue
        s = rv["scales"].numpy()
        assert (s.max(axis=1) / s.min(axis=1)).max() > 3.0, c.name                # anisotropic
        np.testing.assert_allclose(np.linalg.norm(rv["rotations"].numpy(), axis=1), 1.0, atol=1e-6)
    # the cuts of the dense noise, and the loss-shaped cotangent
    dc, dd, da = GR.cotangents("mixed", 2, 20, 24, 1)
    assert not GR.cotangents("depth", 2, 20, 24, 1)[0].any() and torch.equal(GR.cotangents("depth", 2, 20, 24, 1)[1], dd)
    assert not GR.cotangents("alpha", 2, 20, 24, 1)[0].any() and torch.equal(GR.cotangents("alpha", 2, 20, 24, 1)[2], da)
    l1 = GR.cotangents("l1", 2, 64, 64, 1)[0]
    assert torch.equal(l1.abs(), torch.full_like(l1, 1.0 / (3 * 64 * 64)))
    same = (torch.sign(l1[..., 1:]) == torch.sign(l1[..., :-1])).float().mean()
    assert 0.85 < float(same) < 1.0                                               # coherent signs, and both of them
    # corner_scene's own cotangents are the "colour" and "mixed" kinds of the corner case
    from tests.test_gpu_bwd_moments import corner_scene
    c = GR.CASES["corners96"]
    for kind, depth_alpha in (("colour", False), ("mixed", True)):
        want = corner_scene(96, 96, 2, seed=GR.CORNER_SEED, depth_alpha=depth_alpha)[2:]
        for a, b in zip(want, GR.cotangents(kind, 2, 96, 96, c.cot_seed)):
            assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("name,kind", GR.PAIRS)
def test_c_oracle_passes_the_row_check_on_every_case(name, kind):
    case, p = GR.CASES[name], GR.prepared(name, kind)
    print()
    for v, w in enumerate(p.views):
        # the selection condition: no discrete decision differs between the references
        np.testing.assert_array_equal(w.outs["radii"], w.r.radii, err_msg=f"{name}/{kind} view {v}: radii")
        flips = int((w.outs["n_contrib"] != w.state["n_contrib"]).sum())
        assert flips == 0, f"{name}/{kind} view {v}: the oracles differ on n_contrib at {flips} pixels - not a row-check case"
        assert (w.r.radii > 0).any()
        for k in case.keys:
            assert (w.S[k] >= np.abs(w.truth[k]).reshape(len(w.S[k]), -1).max(axis=1)).all()
            assert not w.S[k][w.r.radii == 0].any(), k
        if kind in ("depth", "alpha"):                                            # a zero colour cotangent: no colour gradient
            ck = "shs" if "shs" in case.keys else "colors_precomp"
            assert not w.S[ck].any() and not w.truth[ck].any()
        worst = GR.check_grads_rowwise(as_views(w.grads_c), w.truth, w.S, w.r.radii, 0, case.keys, xy=w.state["xy"])
        print(f"{name}/{kind} view {v}: fp32 C oracle, worst err / S_i  " + "  ".join(f"{k} {x:.2e}" for k, x in worst.items()))
        check_grads(as_views(w.grads_c), w.truth, 0, keys=case.keys)             # (and the per-tensor check, as ever)


def _low_rows(t, frac):
    """Rows of the float64 gradient `t` whose largest entry is below `frac` of the tensor's largest entry."""
    rows = np.abs(t).reshape(t.shape[0], -1).max(axis=1)
    return rows < frac * rows.max()


def _corrupt_a(g, truth, radii):
    """every row below 1 % of its tensor's maximum is 1 % too large"""
    for k in g:
        g[k][_low_rows(truth[k], 0.01)] *= 1.01


def _corrupt_a5(g, truth, radii):
    """every row below 5 % of its tensor's maximum is 0.3 % too large"""
    for k in g:
        g[k][_low_rows(truth[k], 0.05)] *= 1.003


def _corrupt_b(g, truth, radii):
    """the means2D rows below 10 % of the maximum are off by 1e-3 of their own size"""
    m = _low_rows(truth["means2D"], 0.10)
    g["means2D"][m] += 1e-3 * np.abs(g["means2D"][m])


def _corrupt_c(g, truth, radii):
    """every opacity row below 1e-4 of the maximum is lost"""
    g["opacities"][_low_rows(truth["opacities"], 1e-4)] = 0.0


@pytest.mark.parametrize("corrupt,tensor", [(_corrupt_a, "means3D"), (_corrupt_a5, "means3D"), (_corrupt_b, "means2D"),
                                            (_corrupt_c, "opacities")], ids=["a", "a5", "b", "c"])
def test_row_check_rejects_what_the_tensor_check_accepts(corrupt, tensor):
    """(a): a 1 % error on the rows below 5 % of the maximum is 5e-4 of the maximum, which check_grads (2e-4) does see on the rows
    between 2 % and 5 %; the two halves of that corruption it cannot see are run instead - the 1 % error on the rows below 1 %, and
    the rows below 5 % with an error of 0.3 %."""
    w = GR.prepared("head96_B", "mixed").views[0]
    keys = util.GRAD_KEYS
    g = {k: np.array(w.grads_c[k], np.float32) for k in keys}
    GR.check_grads_rowwise(as_views(g), w.truth, w.S, w.r.radii, 0, keys)         # intact: passes
    corrupt(g, w.truth, w.r.radii)
    assert any((g[k] != w.grads_c[k]).any() for k in keys), "the corruption touched no row"
    check_grads(as_views(g), w.truth, 0, keys=keys)                               # one number per tensor: cannot see it
    with pytest.raises(AssertionError, match=rf"grad {tensor}\[view 0\], Gaussian \d+ .* worst err / S_i of the tensor"):
        GR.check_grads_rowwise(as_views(g), w.truth, w.S, w.r.radii, 0, keys)
    if corrupt is _corrupt_a:                                                     # ... in every tensor, not only the first
        for k in keys:
            with pytest.raises(AssertionError, match=f"grad {k}"):
                GR.check_grads_rowwise(as_views(g), w.truth, w.S, w.r.radii, 0, (k,))


def test_row_check_wants_exact_zeros_where_nothing_contributes():
    w = GR.prepared("head96_B", "depth").views[0]
    g = {k: np.array(w.grads_c[k], np.float32) for k in util.GRAD_KEYS}
    i = int(np.nonzero(w.r.radii > 0)[0][0])
    g["colors_precomp"][i, 1] = 1e-30
    with pytest.raises(AssertionError, match="row scale 0"):
        GR.check_grads_rowwise(as_views(g), w.truth, w.S, w.r.radii, 0)
    # a Gaussian the view does not see (radius 0) has no gradient at all, whatever its row scale says
    g = {k: np.array(w.grads_c[k], np.float32) for k in util.GRAD_KEYS}
    radii = w.r.radii.copy()
    radii[i] = 0
    with pytest.raises(AssertionError, match=f"Gaussian {i}: radius 0"):
        GR.check_grads_rowwise(as_views(g), w.truth, w.S, radii, 0)
    for k in util.GRAD_KEYS:
        g[k][i] = 0
    GR.check_grads_rowwise(as_views(g), w.truth, w.S, radii, 0)
