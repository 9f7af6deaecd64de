"""
The rasterizer's gradients, Gaussian by Gaussian: every row of every gradient tensor within GRAD_REL of ITS OWN scale, against
the float64 autograd oracle (tests/grad_rows.py: the yardstick, the cases and the cotangent kinds).

The other gradient checks (test_gpu_parity.check_grads) hold a tensor to GRAD_REL of its largest entry, which leaves two thirds
of the rows free to be wrong by a percent of their own size; an error that scales with the individual splat - the moment shift
of the backward render cancels most where a splat is small and far from the wave's origin - is invisible to them.  Here:

  * scenes with anisotropic scales and random unit quaternions (the rotation gradient of an isotropic splat is round-off), the
    smallest splats on tile corners, a ragged image with a background, SH degree 3, the cov3D_precomp path, and a one-view launch
    that takes the segmented backward on its own; the multi-view ones under every render_build;
  * cotangents: the parity tests' dense noise on colour + depth + alpha ("mixed") and on colour alone, depth alone and alpha alone
    with an all-zero colour cotangent, and the coherent signs of an L1 loss ("l1");
  * before the row check, radii and n_contrib equal the C oracle's exactly: the cases are those on which both references take
    every discrete decision the same way (tests/test_grad_rows_host.py asserts it), so there are no "allowed flips".

RESULTS - worst err / S_i over all cases, kinds and views (bound: GRAD_REL = 2e-4), measured on an MI355X; the C oracle's
column is printed by tests/test_grad_rows_host.py:

    tensor           kernels, whole-tile backward   kernels, segmented backward   fp32 C oracle
                     ("throughput")                 ("latency", "segments", and
                                                    the launches left to themselves)
    means3D          3.9e-5                         6.3e-4                        4.3e-5
    means2D          4.0e-5                         6.3e-4                        4.3e-5
    opacities        5.3e-5                         7.6e-4                        6.5e-5
    scales           5.4e-5                         3.7e-4                        8.8e-5
    rotations        2.2e-5                         2.8e-4                        7.3e-5
    colors_precomp   3.1e-5                         3.1e-5                        3.1e-5
    shs              -                              2.5e-5                        2.5e-5
    cov3D_precomp    -                              2.7e-5                        1.4e-5

The whole-tile backward is as good as the fp32 reference on every row.  The SEGMENTED backward is not, and the cases on which it
misses the bound are marked xfail(strict) below (KNOWN): a segment that does not end at the list's end starts its replay from the
forward's snapshots, with "the colour behind position p" taken as (C_final - C_prefix(p)) . dL/dC (csrc/t4d_raster_render_bwd.h).
Both are fp32 running sums of the whole pixel, so the difference carries a few ulp OF THE PIXEL'S COLOUR (~1e-7), whatever is
left behind p; it enters dL/dalpha_i T_i of every splat of the segment as that absolute amount, while the splat's own terms
scale with its transmittance T_i.  Splats deep in a list (position 45-199 of 186-318 on the failing rows, T_i down to the 1e-4
stop threshold) are therefore off by 2e-4 .. 8e-4 of their own scale in means, opacities, scales and rotations - never in the
colours, which do not read the suffix - and the per-tensor check cannot see it (3e-8 of the tensor's largest entry).  The
whole-tile replay builds the suffix by recursion and has no such term.  A fix has to give the backward a suffix that was summed
on its own (per-segment partial sums kept by the forward beside its running sums, four more accumulations per step and another
snapshot layout for all three forward kernels); it is not part of this change.
"""
import numpy as np
import pytest

from tests import grad_rows as GR, util

pytestmark = pytest.mark.gpu


def rows_against_truth(name, kind, label):
    case, p = GR.CASES[name], GR.prepared(name, kind)
    hip, hg, batch = util.hip_render(p.cams, p.rv, *p.cot)
    st = util.decode_state(batch)
    assert st["status"][0] == 0
    print()
    for v, w in enumerate(p.views):
        np.testing.assert_array_equal(hip["radii"][v], w.r.radii, err_msg=f"{name}/{kind} view {v}")
        np.testing.assert_array_equal(st["n_contrib"][v], w.state["n_contrib"], err_msg=f"{name}/{kind} view {v}")
        ratios = GR.row_ratios(hg, w.truth, w.S, w.r.radii, v, case.keys)
        print(f"{name}/{kind} view {v} [{label}]: kernels, worst err / S_i  " +
              "  ".join(f"{k} {r.max():.2e}" for k, (_, r) in ratios.items()))
        GR.check_grads_rowwise(hg, w.truth, w.S, w.r.radii, v, case.keys, xy=st["xy"][v])


CAUSE = ("segmented backward: the suffix behind a segment is the difference of two fp32 running sums of the whole pixel "
         "(C_final - C_prefix(p), t4d_raster_render_bwd.h), an absolute error of a few ulp of the pixel's colour that splats of "
         "transmittance ~1e-3 .. 1e-4 see at this share of their own scale")
# (case, kind) -> (tensor with the worst row, its err / S_i): the same in the "latency" and the "segments" build, which share
# the segmented backward's arithmetic per pixel; the whole-tile ("throughput") build passes all of them
KNOWN = {
    ("head96_B", "colour"): ("opacities", 2.35e-4),
    ("head96_B", "depth"): ("means2D", 3.39e-4),
    ("head96_A", "mixed"): ("opacities", 4.31e-4),
    ("head96_A", "l1"): ("scales", 2.96e-4),
    ("one_view128", "mixed"): ("opacities", 3.86e-4),
    ("one_view128", "depth"): ("opacities", 7.61e-4),
}


def _param(name, kind, *build):
    marks = ()
    if (name, kind) in KNOWN and build != ("throughput",):
        tensor, ratio = KNOWN[(name, kind)]
        marks = pytest.mark.xfail(strict=True, raises=AssertionError, reason=f"{tensor}: worst err / S_i {ratio:.2e} > GRAD_REL; {CAUSE}")
    return pytest.param(name, kind, *build, marks=marks, id="-".join((name, kind) + build))


@pytest.mark.parametrize("name,kind,render_build", [_param(n, k, b) for n, k in GR.PAIRS if GR.CASES[n].builds
                                                    for b in ("throughput", "latency", "segments")], indirect=["render_build"])
def test_every_row_under_every_build(name, kind, render_build):
    rows_against_truth(name, kind, render_build)


@pytest.mark.parametrize("name,kind", [_param(n, k) for n, k in GR.PAIRS if not GR.CASES[n].builds])
def test_every_row_of_the_launch_as_it_runs(name, kind):
    """No build forced: the SH and cov3D_precomp launches (two views) and the one-view launch take the segmented backward on
    their own, the one-view launch in the latency build."""
    rows_against_truth(name, kind, "default")
