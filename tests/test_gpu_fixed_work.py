"""
The fixed work of the render kernels - what a workgroup does before its first work item and once per tile - through the C ABI
against the oracles, with the tolerances of tests/test_gpu_parity.py:
  * tile coordinates from the launch's multiplier instead of a division (csrc/t4d_tile_div.h): grids that are no power of two,
    with partial tiles at the right and bottom edges;
  * tile workgroups whose first work item is empty leave at once, while the spare workgroups behind them still sum the empty
    views' share of <outputs, cotangents>;
  * a launch of 9,216 tiles, nearly all of them empty, in the throughput build;
  * a tile of 129 .. 140 pairs whose far batch no pixel reads (the backward writes its records as zeros);
  * depth and alpha cotangents (the DA instantiation of the backward).
"""
import math

import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_parity import GRAD_REL, check_grads, check_n_contrib, check_outputs

pytestmark = pytest.mark.gpu


def _build(monkeypatch, build):
    """"throughput": the whole-tile throughput builds of both render kernels, whatever the launch size would have picked;
    "default": what the launch size picks (small launches: the latency forward and the segmented backward)."""
    if build == "throughput":
        monkeypatch.setenv("T4D_LATENCY_TILES", "0")
        monkeypatch.setenv("T4D_NO_SEGMENTS", "1")
    else:
        monkeypatch.delenv("T4D_LATENCY_TILES", raising=False)
        monkeypatch.delenv("T4D_NO_SEGMENTS", raising=False)


@pytest.mark.parametrize("W,H,depth_alpha,build", [(200, 72, False, "throughput"), (1000, 24, False, "throughput"),
                                                   (200, 72, True, "throughput"), (1000, 24, False, "default")])
def test_grids_that_are_no_power_of_two(W, H, depth_alpha, build, monkeypatch):
    """One view of 200 x 72 (13 x 5 tiles) and one of 1000 x 24 (63 x 2 tiles), 300 Gaussians, a background: every pixel of
    every tile - full, partial or empty - and every gradient against the C oracle."""
    from scaffold import scene
    _build(monkeypatch, build)
    rv, cams = util.make_scene(15, 20, H, W, 1, opacity="B", seed=91, bg=(0.3, 0.1, 0.6))
    assert rv["means3D"].shape[0] == 300
    dc, dd, da = scene.output_cotangents(1, H, W, seed=92, depth_alpha=True)
    if not depth_alpha:
        dd = da = None
    hip, hg, batch = util.hip_render(cams, rv, dc, dd, da)
    st = util.decode_state(batch)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    assert (gx, gy) in ((13, 5), (63, 2))
    filled = st["tile_count"][0].reshape(gy, gx) > 0
    assert filled.any() and not filled.all()
    r, g = util.c_oracle_render(cams[0], rv, dc[0], None if dd is None else dd[0], None if da is None else da[0])
    np.testing.assert_array_equal(hip["radii"][0], r.radii)
    os_ = r.state()
    np.testing.assert_array_equal(st["tile_count"][0], os_["ranges"][:, 1] - os_["ranges"][:, 0])
    check_n_contrib(st["n_contrib"][0], os_["n_contrib"])
    check_outputs(hip, r.color, r.depth, r.alpha, 0)
    check_grads(hg, g, 0)


def _rig_with_views_turned_away(H, W, away, bg):
    """scene.camera_rig's first elevation (four azimuths); the views listed in `away` look the other way (nothing in sight)."""
    from scaffold import reference_boundary as boundary, scene
    distance = 0.9
    f = 0.7 * H * distance / (2 * scene.SEMI_AXES[1])
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    cams = []
    for i, az in enumerate(np.linspace(-70.0, 70.0, 4)):
        e, a = math.radians(-20.0), math.radians(az)
        c = distance * np.array([math.sin(a) * math.cos(e), math.sin(e), math.cos(a) * math.cos(e)])
        fwd = -c / np.linalg.norm(c)
        if i in away:
            fwd = -fwd
        right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd], axis=0)
        w2c = np.eye(4)
        w2c[:3, :3] = R
        w2c[:3, 3] = -R @ c
        cam = boundary.setup_camera(W, H, K, w2c.astype(np.float32), near=0.01, far=100)
        cams.append(cam._replace(bg=torch.tensor(bg, dtype=torch.float32)))
    return cams


@pytest.mark.parametrize("build", ["default", "throughput"])
def test_views_that_see_nothing_keep_their_cotangent_dot(build, monkeypatch):
    """Four views of 64 x 64, two of them turned away from the 200 Gaussians, a non-black background: the tile workgroups of
    the empty views find no tile and leave at once; the spare workgroups must still deliver those views' <outputs, cotangents>
    = sum over the view of bg . dL/dC."""
    from topo4d_amd import ViewBatch, pack_views
    from scaffold import scene
    _build(monkeypatch, build)
    H = W = 64
    V = 4
    bg = (0.3, 0.6, 0.1)
    rv, _ = util.make_scene(10, 20, H, W, V, opacity="B", seed=93)
    assert rv["means3D"].shape[0] == 200
    cams = _rig_with_views_turned_away(H, W, away=(1, 3), bg=bg)
    dc, _, _ = scene.output_cotangents(V, H, W, seed=94)
    dev = torch.device("cuda")
    batch = ViewBatch(pack_views(util.to_device(cams, dev), dev), H, W, 1.0, 0)
    d = lambda k: rv[k].to(dev)
    color, radii, depth, alpha = batch.forward(d("means3D"), d("opacities"), d("scales"), d("rotations"), d("colors_precomp"))
    dot = torch.full((V,), float("nan"), device=dev)
    g = batch.backward(dc.to(dev), None, None, cotangent_dot=dot)
    st = util.decode_state(batch)
    assert (st["tile_count"][[1, 3]] == 0).all() and (st["tile_count"][[0, 2]] > 0).any()
    assert (radii[[1, 3]] == 0).all()
    dcd = dc.double()
    want = (color.double().cpu() * dcd).sum(dim=(1, 2, 3))
    scale = (color.double().cpu() * dcd).abs().sum(dim=(1, 2, 3))
    got = dot.double().cpu()
    assert torch.all((got - want).abs() <= 2e-6 * scale), (got, want, scale)
    bgd = torch.tensor(bg, dtype=torch.float64)[None, :, None, None]
    want_bg = (bgd * dcd).sum(dim=(1, 2, 3))
    scale_bg = (bgd * dcd).abs().sum(dim=(1, 2, 3))
    for v in (1, 3):
        assert abs(float(got[v] - want_bg[v])) <= 2e-6 * float(scale_bg[v]), (v, got[v], want_bg[v])
    hip = dict(color=color.cpu().numpy(), depth=depth.cpu().numpy(), alpha=alpha.cpu().numpy())
    hg = {k: (t.cpu().numpy() if t is not None else None) for k, t in g.items()}
    for v in range(V):
        r, go = util.c_oracle_render(cams[v], rv, dc[v])
        check_outputs(hip, r.color, r.depth, r.alpha, v)
        check_grads(hg, go, v)


def test_a_launch_of_mostly_idle_workgroups():
    """Nine views of 512 x 512 = 9,216 tiles (more than the segmented backward takes: the throughput builds, 4,608 tile
    workgroups) of 64 small Gaussians in one corner of the image: all but a few workgroups find an empty first item."""
    from scaffold import scene
    H = W = 512
    V = 9
    rv, cams = util.make_scene(8, 8, H, W, V, opacity="B", seed=95, bg=(0.2, 0.4, 0.1))
    assert rv["means3D"].shape[0] == 64
    rv["means3D"] = (rv["means3D"] * 0.15 + torch.tensor([-0.10, 0.10, 0.0])).contiguous()
    rv["scales"] = (rv["scales"] * 0.15).contiguous()
    dc, _, _ = scene.output_cotangents(V, H, W, seed=96)
    hip, hg, batch = util.hip_render(cams, rv, dc)
    st = util.decode_state(batch)
    filled = (st["tile_count"] > 0).sum(axis=1)
    assert (filled > 0).all() and filled.sum() < 500, filled
    for v, (r, g) in enumerate(util.c_oracle_render_many(cams, rv, dc)):
        np.testing.assert_array_equal(hip["radii"][v], r.radii)
        check_outputs(hip, r.color, r.depth, r.alpha, v)
        check_grads(hg, g, v)


def test_a_far_batch_nobody_reads(monkeypatch):
    """140 splats of opacity 0.95 stacked behind one another over ONE 16 x 16 tile: every pixel is saturated within the first
    twenty, so the tile's second batch of the whole-tile backward (list positions 128 .. 139) is not live: its twelve records
    are written as zeros.  Gradients against the float64 oracle."""
    from scaffold import reference_boundary as boundary
    from scaffold import scene
    _build(monkeypatch, "throughput")
    P, H, W = 140, 16, 16
    g = torch.Generator().manual_seed(97)
    z = 0.5 + 1e-3 * torch.arange(P, dtype=torch.float32)
    perm = torch.randperm(P, generator=g)                        # index order != depth order
    means = torch.stack([(torch.rand(P, generator=g) - 0.5) * 0.01, (torch.rand(P, generator=g) - 0.5) * 0.01, z], 1)[perm]
    rv = dict(means3D=means.contiguous(), opacities=torch.full((P, 1), 0.95), scales=torch.full((P, 3), 0.1),
              rotations=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1), colors_precomp=torch.rand(P, 3, generator=g))
    K = np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]])
    cams = [boundary.setup_camera(W, H, K, np.eye(4, dtype=np.float32))._replace(bg=torch.tensor([0.5, 0.2, 0.7]))]
    dc, _, _ = scene.output_cotangents(1, H, W, seed=98)
    hip, hg, batch = util.hip_render(cams, rv, dc)
    st = util.decode_state(batch)
    assert 129 <= int(st["tile_count"][0, 0]) <= 140
    assert int(st["n_contrib"].max()) < 128                       # nobody reads the far batch
    outs, grads = util.torch_oracle_render(cams[0], rv, dc[0])
    check_outputs(hip, outs["color"].numpy(), outs["depth"].numpy(), outs["alpha"].numpy(), 0)
    check_grads(hg, {k: t.numpy() for k, t in grads.items()}, 0, rel=GRAD_REL)
    far = np.argsort(means[:, 2].numpy())[128:]                   # the splats of the far batch: no gradient at all
    for k in ("means3D", "opacities", "scales", "rotations", "colors_precomp"):
        assert not hg[k][0][far].any(), k
