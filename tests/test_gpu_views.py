"""
GPU parity under off-axis, close, rolled and calibrated cameras: the cases of tests/adversarial_views.py through the C ABI.

Every other parity test sees the head through scaffold/scene.camera_rig, where view depth stays in [0.79, 1.0] m, no Gaussian
is near-culled, almost none is past the EWA frustum clamp and `projmatrix` and `tanfov` describe the same centred pinhole.
Here every case runs under the three render builds, once as a one-view launch (k_front_small) and once in a launch with the
other views of its family, and per view:

  * integer state bit-exact against the C oracle: radii, tile counts, per-tile key order, view_total, and xy, depth and
    conic_opacity of the visible Gaussians (as test_gpu_parity.test_forward_backward_vs_c_oracle);
  * outputs within OUT_TOL; at most 2 threshold pixels (flipped_pixels), gradients through check_grads_modulo_flips with the
    float64 autograd values as `truth`, as the randomised trials of test_gpu_configs do;
  * the SUBSET check: for the Gaussians past the clamp in x, in y, in both, those whose rectangle an image edge clips and
    those within 10 % of the near plane, every gradient tensor against float64 autograd to GRAD_REL = 2e-4 of the SUBSET's own
    largest entry.  The tensor-relative tolerance cannot see an error confined to such a subset when the subset's gradients
    are small beside the tensor's largest (in the close view random12/1 a 5 % error on all 78 clamped Gaussians is 1.4e-5 to
    3.2e-5 of the tensors' largest entries); this one can.  Gaussians with a threshold pixel in reach keep the flip allowance
    and are left out;
  * near-culled Gaussians and empty views: gradients exactly zero, radii zero, pixels exactly the background.

The tests print the kernels' worst subset error per family (DESIGN.md section 2 records the measured figures).
"""
import numpy as np
import pytest
import torch

from tests import adversarial_views as AV, util
from tests.test_gpu_parity import GRAD_REL, check_grads_modulo_flips, check_n_contrib, check_outputs, flipped_pixels
from tests.test_views_host import GROUPS, group

pytestmark = pytest.mark.gpu

MAX_FLIPS = 2


def in_reach_of(flips, xy, radii):
    """[P] bool: Gaussians with one of the threshold pixels `flips` in a tile of their 3-sigma rectangle (the rule of
    test_gpu_parity.check_grads_modulo_flips)."""
    out = np.zeros(len(radii), bool)
    if len(flips) == 0:
        return out
    r = np.asarray(radii, np.float64)
    x0, x1 = np.maximum(0, np.trunc((xy[:, 0] - r) / 16)), np.trunc((xy[:, 0] + r + 15) / 16)
    y0, y1 = np.maximum(0, np.trunc((xy[:, 1] - r) / 16)), np.trunc((xy[:, 1] + r + 15) / 16)
    for fy, fx in flips // 16:
        out |= (fx >= x0) & (fx < x1) & (fy >= y0) & (fy < y1)
    return out & (r > 0)


def check_subset_grads(name, mine, truth, masks, exclude=None, rel=GRAD_REL):
    """Every gradient tensor on every non-empty subset: max-abs-err <= rel * the SUBSET's largest |float64 entry|.  Returns
    the worst error / scale met, with where."""
    worst = (0.0, None)
    for (s, k), (err, scale, _) in AV.subset_errors(mine, truth, masks, exclude).items():
        print(f"    {name} {s:9s} {k:15s}: err {err:.2e} / subset max {scale:.2e} = {err / max(scale, 1e-300):.2e}")
        worst = max(worst, (err / max(scale, 1e-300), (name, s, k)))
        assert err <= rel * scale, f"{name}: grad {k} on subset {s}: err {err:.3e} vs the subset's largest entry {scale:.3e}"
    return worst


def check_view(case, hip, hg, st, v):
    """One view of a launch against both oracles.  Returns (threshold pixels, worst subset error)."""
    o = AV.oracles(case)
    r, os_ = o.r, o.state
    # integer state: bit exact
    np.testing.assert_array_equal(hip["radii"][v], r.radii, err_msg=case.name)
    counts = os_["ranges"][:, 1] - os_["ranges"][:, 0]
    np.testing.assert_array_equal(st["tile_count"][v], counts, err_msg=case.name)
    assert int(st["view_total"][v]) == r.num_rendered, case.name
    for t in np.nonzero(counts)[0]:
        off = int(st["tile_off"][v, t])
        mine = (st["keys"][v, off: off + counts[t]] & np.uint64(0xffffffff)).astype(np.uint32)
        np.testing.assert_array_equal(mine, os_["point_list"][os_["ranges"][t, 0]: os_["ranges"][t, 1]], err_msg=f"{case.name} tile {t}")
    vis = r.radii > 0
    np.testing.assert_array_equal(st["xy"][v][vis], os_["xy"][vis], err_msg=case.name)
    np.testing.assert_array_equal(st["depth"][v][vis], os_["depth"][vis], err_msg=case.name)
    np.testing.assert_array_equal(st["conic_opacity"][v][vis], os_["conic_opacity"][vis], err_msg=case.name)
    # outputs, threshold pixels, gradients per tensor
    flips = flipped_pixels(hip, v, r, st["n_contrib"][v])
    assert len(flips) <= MAX_FLIPS, f"{case.name}: {len(flips)} pixels took a discrete decision the other way"
    check_n_contrib(st["n_contrib"][v], os_["n_contrib"], max_flips=len(flips))
    check_outputs(hip, r.color, r.depth, r.alpha, v, max_flips=len(flips))
    check_grads_modulo_flips(hg, o.grads, v, flips, os_["xy"], r.radii, truth=lambda: o.grads64)
    # gradients per subset, against float64
    mine = {k: hg[k][v] for k in AV.GRAD_KEYS}
    masks = AV.subsets(case, r.radii, os_["xy"])
    worst = check_subset_grads(case.name, mine, o.grads64, masks, exclude=in_reach_of(flips, os_["xy"], r.radii))
    # what the view does not see: no radius, no gradient at all
    dead = ~vis
    assert not hip["radii"][v][dead].any()
    for k in AV.GRAD_KEYS:
        assert not mine[k][dead].any(), f"{case.name}: grad {k} of an invisible Gaussian is not zero"
    if not vis.any():
        bg = case.cam.bg.numpy()
        assert (hip["color"][v] == bg[:, None, None]).all() and not hip["depth"][v].any() and not hip["alpha"][v].any(), case.name
        assert int(st["view_total"][v]) == 0 and not st["tile_count"][v].any()
    return len(flips), worst


def _launch(rv, cams, cots):
    """cots: per view (dc, dd, da), dd and da None for all views or for none."""
    dc = torch.stack([c[0] for c in cots])
    with_da = cots[0][1] is not None
    assert all((c[1] is not None) == with_da for c in cots)
    dd = torch.stack([c[1] for c in cots]) if with_da else None
    da = torch.stack([c[2] for c in cots]) if with_da else None
    hip, hg, batch = util.hip_render(cams, rv, dc, dd, da)
    st = util.decode_state(batch)
    assert st["status"][0] == 0
    return hip, hg, st


def _companion_cotangents(case, n):
    from scaffold import scene
    dc, dd, da = scene.output_cotangents(n, case.cam.image_height, case.cam.image_width, seed=1000 + case.cot_seed, depth_alpha=True)
    return [(dc[i], dd[i], da[i]) if case.depth_alpha else (dc[i], None, None) for i in range(n)]


def _report(name, mode, build, flips, worst):
    print(f"views: {name} ({mode}, {build}): {flips} threshold pixels, worst subset error {worst[0]:.2e} of the subset's scale {worst[1]}")


@pytest.mark.parametrize("name", GROUPS)
def test_one_view_launches(name, render_build):
    """Each case alone: a one-view launch takes the k_front_small front end."""
    flips, worst = 0, (0.0, None)
    for case in group(name):
        hip, hg, st = _launch(case.rv, [case.cam], [AV.cotangents(case)])
        f, w = check_view(case, hip, hg, st, 0)
        flips, worst = flips + f, max(worst, w)
    _report(name, "one view per launch", render_build, flips, worst)


@pytest.mark.parametrize("name", GROUPS)
def test_family_launches(name, render_build):
    """Each case in one launch with the other views of its family (off-centre principal points next to a centred one, an empty
    view next to full ones, a calibrated camera among the others of the capture)."""
    members = {c.name for c in group(name)}
    flips, worst, seen = 0, (0.0, None), set()
    for label, rv, cams, checked in AV.batches():
        if checked[0][1].name not in members:
            continue
        cots = _companion_cotangents(checked[0][1], len(cams))
        for v, case in checked:
            cots[v] = AV.cotangents(case)
        hip, hg, st = _launch(rv, cams, cots)
        assert hip["color"].shape[0] == len(cams) >= 2
        for v, case in checked:
            f, w = check_view(case, hip, hg, st, v)
            flips, worst = flips + f, max(worst, w)
            seen.add(case.name)
    assert seen == members
    _report(name, "family launch", render_build, flips, worst)
