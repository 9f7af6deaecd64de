"""CPU: the per-term, per-vertex yardstick of the topology priors' gradients (tests/priors_rows.py) - its tie to the G12-pinned
evaluate_torch, the fp32 plain-torch evaluation against it at PRIORS_REL / 4 on every case (the kernels get PRIORS_REL in
tests/test_gpu_priors_rows.py: a factor of four over a reference of the same precision, for their summation order and the
device's sqrtf / acosf / expf), the conditions the cases were chosen under, and four mutations that today's per-tensor rule
lets through and the row check does not.

Mutation classes met so far by the kernels (tests/test_gpu_priors_rows.py): none - no row of t4d_priors_eval has failed."""
import numpy as np
import pytest
import torch

from tests import priors_rows as PR
from tests.test_priors_host import KEYS
from topo4d_amd import priors as T

CASES = [(n, f) for n in PR.NAMES for f in PR.FRAMES]
_TORCH = {}


def torch_term_grads(name, frame):
    """{term: {tensor: [P, w] float32 array}}: the fp32 plain-torch evaluation's gradient of every term alone."""
    if (name, frame) not in _TORCH:
        c = PR.case(name, frame)
        pr = c.build()
        p = {k: c.params[k].clone().requires_grad_(True) for k in KEYS}
        _, detail = pr.evaluate_torch(p, c.is_initial)
        out = {}
        for term in PR.terms_of(c.is_initial):
            g = torch.autograd.grad(detail[term], [p[k] for k in KEYS], retain_graph=True, allow_unused=True) \
                if detail[term].requires_grad else (None,) * 3
            out[term] = {k: np.zeros(tuple(p[k].shape), np.float32) if a is None else a.numpy() for k, a in zip(KEYS, g)}
        _TORCH[(name, frame)] = out
    return _TORCH[(name, frame)]


@pytest.mark.parametrize("name,frame", CASES)
def test_elements_sum_to_the_pinned_evaluation(name, frame):
    """weight * elements.sum() == evaluate_torch's detail[term] on float64 parameters, to 1e-12 relative, every term.  The cached
    cos_init is handed to evaluate_torch as float64 too (the same values): it takes arccos in the buffer's own precision."""
    c = PR.case(name, frame)
    pr = c.build()
    pr.cos_init = {k: v.double() for k, v in pr.cos_init.items()}
    p64 = {k: v.double() for k, v in c.params.items()}
    L = PR.elements(pr, p64, c.is_initial)
    _, detail = pr.evaluate_torch(p64, c.is_initial)
    assert sorted(L) == sorted(detail) == sorted(PR.terms_of(c.is_initial))
    nbr_shape = (pr.P, pr.K)
    for term, e in L.items():
        assert e.dtype == torch.float64
        want = nbr_shape if term in PR.NBR_TERMS else ((pr.edges_np[term].shape[1],) if term in T.EDGE_TERMS else
                                                       ((pr.regions_np[term].size,) if term in T.REGION_TERMS else (pr.P,)))
        assert tuple(e.shape) == want, (term, tuple(e.shape), want)
        got, ref = pr.weights[term] * float(e.sum()), float(detail[term])
        assert detail[term].dtype == torch.float64 and abs(got - ref) <= 1e-12 * abs(ref), (term, got, ref)


@pytest.mark.parametrize("name,frame", CASES)
def test_fp32_torch_meets_a_quarter_of_the_bound_on_every_row(name, frame, capsys):
    c, pr, yard = PR.prepared(name, frame)
    grads = torch_term_grads(name, frame)
    lines = []
    for term in PR.terms_of(c.is_initial):
        for k in KEYS:
            _, ratio = PR.row_ratios(grads[term][k], yard.truth[term][k], yard.S[term][k], PR.extra_of(yard, term, k))
            if (yard.S[term][k] > 0).any():
                lines.append(f"{name}/{frame} {term:17s} {k:17s} fp32 torch, worst err / S_i {ratio.max():.2e}")
    # fp32 torch under the rule tests/test_gpu_priors_rows.py holds the kernels' all-terms gradient to: the total's gradient
    # against the sum of the per-term gradients, relative to sum_terms |g_term| (allowed there: 8 * 2^-24 = 4.8e-7).  Printed only.
    p = {k: c.params[k].clone().requires_grad_(True) for k in KEYS}
    c.build().evaluate_torch(p, c.is_initial)[0].backward()
    for k in KEYS:
        if p[k].grad is not None:
            parts = [grads[term][k].astype(np.float64) for term in PR.terms_of(c.is_initial)]
            size = sum(np.abs(a) for a in parts)
            diff = np.abs(p[k].grad.numpy() - sum(parts))
            lines.append(f"{name}/{frame} all terms vs the sum of the terms alone, {k}: fp32 torch, worst diff / sum |g_term| "
                         f"{np.where(size > 0, diff / np.where(size > 0, size, 1.0), 0.0).max():.2e}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    for term in PR.terms_of(c.is_initial):
        for k in KEYS:
            PR.check_rows(grads[term][k], yard.truth[term][k], yard.S[term][k], PR.PRIORS_REL / 4, PR.extra_of(yard, term, k),
                          what=f"{name}/{frame} {term} grad {k} (fp32 torch)", names=lambda i, term=term: PR.named_by(pr, term, i))


@pytest.mark.parametrize("name", PR.NAMES)
def test_the_kinks_lie_where_the_cases_say(name):
    """From the float64 inputs alone: iso's ties touch at most 0.5 % of its live rows on G12 (17 ties, 18 of 5,166 rows) and none on
    the grids, whose live elements all keep 2^-10 |off| from the kink; no live rigid or rot element sits at d = 0; on the grids at
    least a fifth of each soft term's elements lie on either side of cos_init."""
    c, pr, yard = PR.prepared(name, "later")
    info = yard.info
    assert info["iso_tie_rows"] <= PR.TIE_ROWS * info["iso_live_rows"], info
    assert info["rigid_at_kink"] == 0 and info["rot_at_kink"] == 0, info
    if name == "g12":
        assert (info["iso_ties"], info["iso_live"], info["iso_tie_rows"], info["iso_live_rows"]) == (17, 20529, 18, 5166), info
        live, rel, _ = PR.iso_state(pr, c.params)
        for e in range(-22, -15):                                 # the count does not depend on the threshold
            assert int((live & (rel < 2.0 ** e)).sum()) == 17, e
    else:
        assert info["iso_ties"] == 0 and info["iso_min_rel"] >= PR.CLEAR, info
        assert not yard.extra.any()
        for k, (pos, neg) in info["soft_sign_share"].items():
            assert pos >= 0.2 and neg >= 0.2, (k, pos, neg)
        assert sorted(info["soft_sign_share"]) == sorted(k for k in T.SOFT_TERMS if pr.edges_np[k].shape[1])


@pytest.mark.parametrize("name", PR.NAMES[1:])
def test_the_grids_exercise_what_g12_leaves_idle(name):
    c, pr, _ = PR.prepared(name, "later")
    n_lat, n_lon, _ = PR.GRID_SHAPES[name]
    assert pr.P == n_lat * n_lon and pr.P % 256 in (240, 1) and (pr.P * pr.K) % 256 != 0
    assert pr.edges_np["flat_lid_top"].shape[1] == 0 and pr.edges_np["flat_lip"].shape[1] == 256
    assert pr.regions_np["flat_face_bottom"].size == 0 and pr.regions_np["flat_eye"].size > 0
    dropped = np.arange(0, pr.P, 7)
    slot = (pr.nnum_np[dropped] + 1) // 2                       # neighbor_num is already one less: the middle of the ring as it was
    assert (pr.mask_np[dropped, slot] == 0).all() and slot.min() >= 1 and (slot < pr.nnum_np[dropped]).all()
    assert (pr.mask_np.sum(1) == pr.nnum_np).all()
    q, prev = c.params["unnorm_rotations"], pr.prev_inv_rot_fg
    norm = q.norm(dim=1)
    assert norm.min() < 0.7 and norm.max() > 1.6 and norm.min() >= 0.5 and norm.max() <= 2.0
    rel = PR._rel_rot(pr, q.double())
    assert float((rel[:, 1:].norm(dim=1) > 0.5).double().mean()) > 0.5           # relative angles over 60 degrees on most vertices
    assert torch.allclose(prev.norm(dim=1), torch.ones(pr.P), atol=1e-6)
    # the conditions the mesh was drawn under (priors_rows._grid), from the float64 inputs: no edge element close to flat or folded,
    # no sliver triangle, every soft element GRID_TURN_MIN away from its cos_init (the fp32 evaluation's: 1e-5 rad covers its
    # rounding at |cos| <= 0.95)
    x = c.params["means3D"].double()
    for k in T.EDGE_TERMS:
        cos, s1, s2 = PR._dihedral(x, pr.edges[k].long())
        assert (cos.abs() <= PR.GRID_COS_MAX).all() and (torch.minimum(s1, s2) >= PR.GRID_SIN_MIN).all(), k
        if k in T.SOFT_TERMS:
            assert (pr.cos_init[k].abs() <= PR.GRID_COS_MAX + 1e-6).all(), k
            assert ((torch.arccos(cos) - torch.arccos(pr.cos_init[k].double())).abs() >= PR.GRID_TURN_MIN - 1e-5).all(), k
    ls = c.params["log_scales"]
    tie = (ls[:, 0] == ls[:, 1]) & (ls[:, 1] == ls[:, 2])
    over = ls.exp().max(dim=1).values - 1.5 * pr.init_scale
    assert tie.sum() >= pr.P // 5 and (~tie).sum() > pr.P // 2
    for rows in (tie, ~tie):
        assert (over[rows] > 0).any() and (over[rows] < 0).any()


def test_grid_priors_without_the_new_arguments_is_unchanged_by_them():
    """The optional arguments act after every random draw: what they do not touch is the same with and without them."""
    from scaffold import scene
    from tests.test_gpu_priors import grid_priors
    x0 = scene.make_gaussians(12, 20, seed=3)["means3D"]
    a = grid_priors(12, 20, x0, device="cpu")
    b = grid_priors(12, 20, x0, device="cpu", **PR.GRID_TOPOLOGY)
    for k in ("nbr", "neighbor_dist", "rig_w", "rot_w", "iso_w", "init_scale"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.edges["flat"], b.edges["flat"]) and torch.equal(a.edges["flat_lip"][:, :256], b.edges["flat_lip"])
    assert torch.equal(a.regions["flat_eye"], b.regions["flat_eye"])
    assert (a.nbr_mask.sum(1) == a.neighbor_num).all() and a.weights == b.weights == T.DEFAULT_WEIGHTS


# ---- what today's rule lets through -----------------------------------------------------------------------------------
def _passes_the_tensor_rule(total, ref):
    """tests/test_gpu_priors._check_against_torch: 1e-4 of the summed tensor's largest entry."""
    return all(float(np.abs(total[k] - ref[k]).max()) <= 1e-4 * max(float(np.abs(ref[k]).max()), 1e-30) for k in KEYS)


MUTATIONS = {   # name -> (term, tensor, factor applied to that term's gradient of that tensor)
    "a: rigid's means3D gradient set to zero": ("rigid", "means3D", 0.0),
    "b: rigid's unnorm_rotations gradient x 0.5": ("rigid", "unnorm_rotations", 0.5),
    # as stated, (c) iso x 1.5 changes the summed means3D by 1.01e-4 of its largest entry and (d) flat_face_bottom with the wrong
    # sign by 2.2e-4: the tensor rule (1e-4) catches both.  Halved until it does not: x 1.25, and a change of half the gradient
    # instead of twice it (-1 -> 0 -> 0.5)
    "c: iso x 1.25 (x 1.5 halved once)": ("iso", "means3D", 1.25),
    "d: flat_face_bottom x 0.5 (the wrong sign halved twice)": ("flat_face_bottom", "means3D", 0.5),
}


@pytest.mark.parametrize("which", list(MUTATIONS))
def test_mutation_passes_the_tensor_rule_and_fails_the_row_check(which, capsys):
    """Applied to the fp32 torch per-term gradients of G12's later frame, then summed as the kernel sums them.  Every one passes
    today's rule - (c) and (d) only after halving, see MUTATIONS - and fails check_rows on its term."""
    term, key, factor = MUTATIONS[which]
    c, pr, yard = PR.prepared("g12", "later")
    grads = torch_term_grads("g12", "later")
    terms = PR.terms_of(False)
    ref = {k: sum(grads[t][k].astype(np.float32) for t in terms) for k in KEYS}
    mutated = {k: sum((np.float32(factor) * grads[t][k] if (t, k) == (term, key) else grads[t][k]) for t in terms) for k in KEYS}
    assert _passes_the_tensor_rule(ref, ref)
    share = float(np.abs(mutated[key] - ref[key]).max()) / float(np.abs(ref[key]).max())
    with capsys.disabled():
        print(f"\nmutation {which}: changes the summed {key} by {share:.2e} of its largest entry (the tensor rule allows 1e-4)")
    assert _passes_the_tensor_rule(mutated, ref), (which, share)
    with pytest.raises(AssertionError, match=f"{term} grad {key}"):
        PR.check_rows(np.float32(factor) * grads[term][key], yard.truth[term][key], yard.S[term][key], PR.PRIORS_REL,
                      PR.extra_of(yard, term, key), what=f"g12/later {term} grad {key}")
    # and in the sum of all terms, row by row
    S_all = sum(yard.S[t][key] for t in terms)
    t_all = sum(yard.truth[t][key] for t in terms)
    PR.check_rows(ref[key], t_all, S_all, PR.PRIORS_REL, PR.extra_of(yard, "iso", key), what=f"g12/later all terms grad {key}")
    with pytest.raises(AssertionError, match="all terms"):
        PR.check_rows(mutated[key], t_all, S_all, PR.PRIORS_REL, PR.extra_of(yard, "iso", key), what=f"g12/later all terms grad {key}")
