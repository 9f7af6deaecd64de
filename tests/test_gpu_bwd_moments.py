"""
The backward render accumulates the moments of e = G dL/dalpha about a fixed origin per wave and shifts them to the splat centre
when a (Gaussian, tile) record is written (csrc/t4d_raster_render_bwd.h).  The shift cancels, most where a splat is small and
far from the origin, and the backward has a pixel-to-lane map of its own; these tests pin RESULTS where either could show:

  * the smallest splats the 0.3 px^2 dilation allows, centred on tile corners and just outside tile edges, against the float64
    oracle and the C oracle;
  * the same launch twice: bit-identical gradients;
  * a one-view and a three-view launch (the segmented builds read the forward's snapshots by thread), an image whose size is not
    a multiple of 16, and a launch with depth and alpha cotangents, each against the oracles.

Tolerances are those of tests/test_gpu_parity.py.
"""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_parity import check_grads, check_outputs

pytestmark = pytest.mark.gpu


def corner_scene(H, W, V, seed, depth_alpha=False):
    """Isotropic splats of vanishing 3D size (their 2D covariance is the dilation alone: cut-off radius <= 1.8 px) whose centres, in
    view 0, sit ON the corners of the 16x16 tiles (pixel coordinates 16 k - 0.5), just outside and just inside tile edges, and on
    the corners of the 8x8 blocks; the other views see the same splats from elsewhere."""
    from scaffold import scene
    rng = np.random.default_rng(seed)
    cams = scene.camera_rig(H, W, n_views=V)
    cam = cams[0]
    pts = []
    edges_x, edges_y = np.arange(16, W, 16) - 0.5, np.arange(16, H, 16) - 0.5
    for ex, ey in [(ex, ey) for _ in range(3) for ex in edges_x for ey in edges_y]:      # three layers: the splats overlap and occlude
        pts.append((ex, ey))                                         # a tile corner: four tiles, sixteen sub-blocks in reach
        pts.append((ex + rng.choice([-0.75, 0.75]), ey + rng.uniform(1.0, 14.0)))            # beside a vertical tile edge
        pts.append((ex + rng.uniform(1.0, 14.0), ey + rng.choice([-0.75, 0.75])))            # beside a horizontal one
        pts.append((ex + rng.choice([-1.7, 1.7]), ey + rng.choice([-1.7, 1.7])))             # a corner at the cut-off's reach
        pts.append((ex + rng.choice([-8.0, 8.0]), ey + rng.choice([-8.0, 8.0])))             # a corner of the waves' 8x8 blocks
    uv = np.array(pts)
    uv = uv[(uv[:, 0] > 0) & (uv[:, 0] < W - 1) & (uv[:, 1] > 0) & (uv[:, 1] < H - 1)]
    P = len(uv)
    z = 0.9 + rng.permutation(P) * 1e-3                              # distinct depths: one order for every oracle
    xc = ((uv[:, 0] + 0.5) * 2.0 / W - 1.0) * z * cam.tanfovx
    yc = ((uv[:, 1] + 0.5) * 2.0 / H - 1.0) * z * cam.tanfovy
    pc = np.stack([xc, yc, z, np.ones(P)], 1)
    world = pc @ np.linalg.inv(cam.viewmatrix.double().numpy().reshape(4, 4))      # row vectors: p_cam = p_world @ viewmatrix
    rv = {
        "means3D": torch.tensor(world[:, :3]).float().contiguous(),
        "opacities": torch.tensor(rng.uniform(0.3, 0.95, (P, 1))).float(),
        "scales": torch.full((P, 3), 1e-6),
        "rotations": torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1),
        "colors_precomp": torch.tensor(rng.uniform(0.0, 1.0, (P, 3))).float(),
    }
    dc, dd, da = scene.output_cotangents(V, H, W, seed=seed + 1, depth_alpha=depth_alpha)
    return rv, cams, dc, dd, da


def check_against_both_oracles(cams, rv, dc, dd, da, hip, hg):
    for v in range(len(cams)):
        r, g = util.c_oracle_render(cams[v], rv, dc[v], None if dd is None else dd[v], None if da is None else da[v])
        np.testing.assert_array_equal(hip["radii"][v], r.radii)
        check_outputs(hip, r.color, r.depth, r.alpha, v)
        check_grads(hg, g, v)
        outs, grads = util.torch_oracle_render(cams[v], rv, dc[v], None if dd is None else dd[v], None if da is None else da[v])
        check_outputs(hip, outs["color"].numpy(), outs["depth"].numpy(), outs["alpha"].numpy(), v)
        check_grads(hg, {k: x.numpy() for k, x in grads.items()}, v)


@pytest.mark.parametrize("depth_alpha", [False, True])
def test_smallest_splats_on_tile_corners_and_edges(depth_alpha, render_build):
    H = W = 96
    V = 2
    rv, cams, dc, dd, da = corner_scene(H, W, V, seed=31, depth_alpha=depth_alpha)
    hip, hg, _ = util.hip_render(cams, rv, dc, dd, da)
    assert (hip["radii"][0] > 0).all()                      # view 0 sees every splat where it was put
    check_against_both_oracles(cams, rv, dc, dd, da, hip, hg)


def test_same_launch_twice_is_bit_identical(render_build):
    H = W = 96
    rv, cams, dc, dd, da = corner_scene(H, W, 2, seed=33, depth_alpha=True)
    _, g1, _ = util.hip_render(cams, rv, dc, dd, da)
    _, g2, _ = util.hip_render(cams, rv, dc, dd, da)
    for k in util.GRAD_KEYS:
        np.testing.assert_array_equal(g1[k], g2[k])
    rv2, cams2 = util.make_scene(30, 50, 128, 128, 3, opacity="B", seed=34)
    from scaffold import scene
    dc2, _, _ = scene.output_cotangents(3, 128, 128, seed=35)
    _, g1, _ = util.hip_render(cams2, rv2, dc2)
    _, g2, _ = util.hip_render(cams2, rv2, dc2)
    for k in util.GRAD_KEYS:
        np.testing.assert_array_equal(g1[k], g2[k])


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("depth_alpha", [False, True])
def test_one_and_three_view_launches(V, depth_alpha):
    """No build is forced: a one-view and a three-view launch take the segmented backward on their own, the latency build included."""
    H = W = 128
    rv, cams = util.make_scene(30, 50, H, W, V, opacity="B", seed=36)
    from scaffold import scene
    dc, dd, da = scene.output_cotangents(V, H, W, seed=37, depth_alpha=depth_alpha)
    hip, hg, _ = util.hip_render(cams, rv, dc, dd, da)
    check_against_both_oracles(cams, rv, dc, dd, da, hip, hg)


@pytest.mark.parametrize("V", [1, 3])
def test_image_size_not_a_multiple_of_16(V, render_build):
    H, W = 75, 100
    rv, cams = util.make_scene(16, 24, H, W, V, opacity="B", seed=38, bg=[0.2, 0.5, 0.9])
    from scaffold import scene
    dc, dd, da = scene.output_cotangents(V, H, W, seed=39, depth_alpha=True)
    hip, hg, _ = util.hip_render(cams, rv, dc, dd, da)
    check_against_both_oracles(cams, rv, dc, dd, da, hip, hg)
    rv, cams, dc, dd, da = corner_scene(H, W, V, seed=40)
    hip, hg, _ = util.hip_render(cams, rv, dc, dd, da)
    check_against_both_oracles(cams, rv, dc, dd, da, hip, hg)
