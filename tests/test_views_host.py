"""CPU: the camera cases of tests/adversarial_views.py on the two oracles.

oracle/raster_oracle.c (fp32, explicit backward formulas) against torch.autograd over oracle/torch_oracle.py (float64) under
off-centre principal points, fx != fy, roll, laterally aimed and close cameras, a camera inside the head, a 0.21-90 m depth
range with duplicated means, the 24 calibrated cameras of golden G16 and 24 randomised draws: outputs, radii, n_contrib
(exactly: the cases' seeds are chosen for it) and gradients, per tensor and per SUBSET - the Gaussians past the frustum
clamp in x, in y, in both, those whose rectangle an image edge clips, those within 10 % of the near plane - each relative to
the subset's own largest float64 entry.  tests/test_gpu_views.py holds the kernels to GRAD_REL = 2e-4 on the same subsets; the
oracles, which share every formula with the kernels, must agree far more tightly for that to mean anything.

Measured on the committed cases (95 views; C oracle built -O3 -march=native -ffp-contract=off, run on ONE OpenMP thread,
see adversarial_views.one_oracle_thread: with several its atomics sum in a run-dependent order and the same figure moves
between 2e-6 and 2e-5):
  outputs          largest |C - float64| = 1.1e-6                               bound OUT_BOUND    = 5e-6
  tensor gradients largest error / tensor's largest entry = 8.7e-6              bound (test_oracle) 1e-4
  subset gradients largest error / SUBSET's largest entry, per family:          bound SUBSET_BOUND = 4e-5
                   offcentre 8.6e-6, focal 6.0e-6, roll 7.0e-6, lateral 9.5e-6 (diag_a, clamp_y, rotations), close 3.0e-6,
                   inside 2.1e-6, depth 3.9e-6, calibrated 8.2e-6, random 1.0e-5 (random7/0, clamp_y, opacities)
SUBSET_BOUND is 4 x the measured worst: how the C oracle rounds depends on the host it is built on (-march=native; soak seed
2635 of tests/test_gpu_configs.py documents the effect).  It stays at or below 5e-5, a quarter of GRAD_REL; a case that
cannot meet it is to be changed (another scene seed), not the bound.
"""
import numpy as np
import pytest

from tests import adversarial_views as AV

OUT_BOUND = 5e-6
TENSOR_BOUND = 1e-4
SUBSET_BOUND = 4e-5
assert SUBSET_BOUND <= 5e-5

FAMILIES = AV.families()
GROUPS = ["offcentre", "focal", "roll", "lateral", "close", "inside", "depth", "calibrated", "random"]


def group(name):
    """The cases of a named family; "random" = the 24 randomised draws together."""
    return [c for f, cs in FAMILIES.items() if f == name or (name == "random" and f.startswith("random")) for c in cs]


def test_the_families_the_cases_are_made_of():
    assert set(GROUPS[:-1]) | {f"random{k}" for k in range(24)} == set(FAMILIES)
    n = {g: len(group(g)) for g in GROUPS}
    assert n["offcentre"] >= 5 and n["focal"] == 2 and n["roll"] == 3 and n["lateral"] >= 4 and n["close"] == 2
    assert n["calibrated"] == 24 and n["random"] == 48
    for c in AV.cases():
        assert c.name in AV.DECLARED, f"{c.name} declares no coverage"
        assert max(c.cam.image_height, c.cam.image_width) <= 160 and (c.cam.image_height % 16 or c.cam.image_width % 16)
        s = c.rv["scales"].numpy()
        assert (s.max(axis=1) / s.min(axis=1)).max() > 3.0                       # anisotropic
        np.testing.assert_allclose(np.linalg.norm(c.rv["rotations"].numpy(), axis=1), 1.0, atol=1e-6)
    for c in group("lateral"):
        assert c.cover.clamp_grad >= 0.1 and max(c.cover.clamp) >= 0.1
    lat = [c.cover for c in group("lateral")]
    for side in range(4):                                                        # each side in x and in y, and both at once
        assert any(cv.clamp[side] >= 0.1 for cv in lat)
    assert any(cv.both >= 0.1 for cv in lat)
    assert all(c.cover.culled[0] > 0 and c.cover.radius >= 150 for c in group("close"))
    # every launch of a family has one image size and one set of Gaussians
    for label, rv, cams, checked in AV.batches():
        assert len({(c.image_height, c.image_width) for c in cams}) == 1, label
        assert len(cams) >= 2 and all(case.rv is rv for _, case in checked), label


@pytest.mark.parametrize("name", GROUPS)
def test_c_oracle_against_float64_autograd_per_subset(name):
    worst = (0.0, None)
    print()
    for c in group(name):
        o = AV.oracles(c)
        r, st, outs = o.r, o.state, o.outs64
        got = AV.measure(c, r.radii, o.grads64)
        print(AV.coverage_row(c, got))
        AV.check_coverage(c, got)
        np.testing.assert_array_equal(outs["radii"].numpy(), r.radii, err_msg=c.name)
        np.testing.assert_array_equal(outs["n_contrib"].numpy(), st["n_contrib"], err_msg=c.name)
        for k in ("color", "depth", "alpha"):
            err = np.abs(outs[k].numpy() - getattr(r, k)).max()
            assert err <= OUT_BOUND, f"{c.name}: {k} differs by {err:.2e}"
        for k in AV.GRAD_KEYS:
            a, b = np.asarray(o.grads[k], np.float64).reshape(o.grads64[k].shape), o.grads64[k]
            assert np.abs(a - b).max() <= TENSOR_BOUND * np.abs(b).max() + 1e-10, (c.name, k)
        masks = AV.subsets(c, r.radii, st["xy"])
        for (s, k), (err, scale, _) in AV.subset_errors(o.grads, o.grads64, masks).items():
            print(f"    {s:9s} {k:15s} {int(masks[s].sum()):4d} Gaussians: err {err:.2e} / subset max {scale:.2e} = {err / max(scale, 1e-300):.2e}")
            worst = max(worst, (err / max(scale, 1e-300), (c.name, s, k)))
            assert err <= SUBSET_BOUND * scale, f"{c.name}: {k} on subset {s}: {err:.3e} vs the subset's largest {scale:.3e}"
    print(f"{name}: worst subset-relative error between the oracles {worst[0]:.2e} {worst[1]}")


def test_near_culled_and_empty_views_have_zero_gradients():
    one, none, _ = group("inside")
    for c, n_vis in ((one, 1), (none, 0)):
        o = AV.oracles(c)
        assert int((o.r.radii > 0).sum()) == n_vis == int((o.outs64["radii"] > 0).sum())
        dead = o.r.radii == 0
        for k in AV.GRAD_KEYS:
            assert not np.asarray(o.grads[k])[dead].any() and not o.grads64[k][dead].any(), (c.name, k)
    o = AV.oracles(none)
    bg = none.cam.bg.numpy()
    for color, depth, alpha in ((o.r.color, o.r.depth, o.r.alpha), tuple(o.outs64[k].numpy() for k in ("color", "depth", "alpha"))):
        assert (color == bg[:, None, None]).all() and not depth.any() and not alpha.any()
    assert o.r.num_rendered == 0
    # Gaussians behind the near plane of a view that does see others: no radius, no gradient
    for c in group("close"):
        o = AV.oracles(c)
        culled = AV.view_space(c)[2] <= AV.TO.C["T4D_NEAR_CULL_Z"]
        assert culled.sum() == c.cover.culled[0] and not o.r.radii[culled].any()
        for k in AV.GRAD_KEYS:
            assert not np.asarray(o.grads[k])[culled].any() and not o.grads64[k][culled].any(), (c.name, k)


def test_depth_keys_span_exponents_and_duplicates_sort_by_index():
    c = group("depth")[0]
    o = AV.oracles(c)
    st = o.state
    d = st["depth"][o.r.radii > 0]
    assert d.min() < 0.22 and d.max() > 80.0
    assert len(np.unique(np.frexp(d)[1])) >= 9                      # binary exponents -2 .. 7
    n = c.rv["means3D"].shape[0] - 2 * AV.DUPLICATES
    m = c.rv["means3D"].numpy()
    lists = [st["point_list"][a:b] for a, b in st["ranges"] if b > a]
    for j in range(AV.DUPLICATES):
        twins = [i for i in range(n) if (m[i] == m[n + j]).all()] + [n + j, n + AV.DUPLICATES + j]
        assert len(twins) == 3 and len({st["depth"][i].tobytes() for i in twins}) == 1
        assert len({tuple(c.rv["colors_precomp"][i].tolist()) for i in twins}) == 3
        assert len({float(c.rv["opacities"][i]) for i in twins}) == 3
        seen = 0
        for l in lists:
            pos = [int(np.nonzero(l == i)[0][0]) for i in twins if (l == i).any()]
            if len(pos) == 3:
                seen += 1
                assert pos[1] == pos[0] + 1 and pos[2] == pos[1] + 1, f"duplicates {twins} not adjacent in index order: {pos}"
        assert seen >= 1, f"duplicates {twins} share no tile"
