"""
GPU: the one-wave bin sort of big launches (k_sort_tiles<256>'s small-bin units: one bin per wave, 1, 2, 4 or 8 keys per lane in
registers) against the path it replaces (T4D_NO_WAVE_SORT: bins of 64 keys and more through LDS, one per workgroup) and against
the C oracle.

24 views of 64 x 64 pixels, forced into the throughput regime (the render_build fixture's switches) and onto the 256-thread
sorter (T4D_SORT_256: a launch of 384 tiles would take the 1024-thread one).  One tile of every view holds exactly n stacked
Gaussians, another a handful; n walks every class edge of the network (64 K for K = 1, 2, 4, 8) and the hand-over to the
whole-workgroup sort at 512.  The sorted arena is a unique permutation, so every output and every gradient of the two paths must
be BIT-equal; the forward is held to the parity tolerance of tests/test_gpu_parity.py against the C oracle.
"""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_parity import check_outputs

pytestmark = pytest.mark.gpu

H = W = 64
V = 24
F = 40.0
C0 = 24.5                    # principal point: the stack projects into tile (1, 1), pixels 16..31
EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)


def _regime(monkeypatch, wave):
    monkeypatch.setenv("T4D_LATENCY_TILES", "0")
    monkeypatch.setenv("T4D_NO_SEGMENTS", "1")
    monkeypatch.setenv("T4D_SORT_256", "1")
    if wave:
        monkeypatch.delenv("T4D_NO_WAVE_SORT", raising=False)
    else:
        monkeypatch.setenv("T4D_NO_WAVE_SORT", "1")


def _cameras():
    from scaffold import reference_boundary as boundary
    K = np.array([[F, 0, C0], [0, F, C0], [0, 0, 1.0]])
    cams = []
    for v in range(V):
        w2c = np.eye(4, dtype=np.float32)
        w2c[2, 3] = 1e-3 * v                                    # every view sees all of the stack, at its own depths
        cams.append(boundary.setup_camera(W, H, K, w2c))
    return cams


def _stack(n, equal_depths, seed):
    """n sub-pixel Gaussians in front of pixel (24.5, 24.5), index order shuffled against depth order, and five more in front of
    pixel (52, 52).  equal_depths: groups of seven share one z bit for bit, so their keys differ in the index word only."""
    g = torch.Generator().manual_seed(seed)
    rank = torch.arange(n, dtype=torch.float32)
    z = 0.5 + 4e-4 * (torch.floor(rank / 7.0) * 7.0 if equal_depths else rank)
    xy = (torch.rand(n, 2, generator=g) - 0.5) * 0.004
    stack = torch.cat([xy, z[:, None]], 1)[torch.randperm(n, generator=g)]
    zf = 0.55 + 0.01 * torch.arange(5, dtype=torch.float32)
    far = torch.stack([(52.0 - C0) / F * zf, (52.0 - C0) / F * zf, zf], 1)
    means = torch.cat([stack, far])
    P = n + 5
    return dict(means3D=means, opacities=torch.rand(P, 1, generator=g) * 0.03 + 0.01, scales=torch.full((P, 3), 1e-3),
                rotations=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1), colors_precomp=torch.rand(P, 3, generator=g))


@pytest.fixture(scope="module")
def cotangents():
    from scaffold import scene
    return scene.output_cotangents(V, H, W, seed=41, depth_alpha=True)


@pytest.mark.parametrize("equal_depths", [False, True], ids=["distinct", "equal-depth-groups"])
@pytest.mark.parametrize("n", EDGES)
def test_wave_sort_equals_the_block_sort_bit_for_bit(n, equal_depths, cotangents, monkeypatch):
    cams = _cameras()
    rv = _stack(n, equal_depths, seed=100 + n)
    dc, dd, da = cotangents
    _regime(monkeypatch, wave=False)
    old, old_g, _ = util.hip_render(cams, rv, dc, dd, da)
    _regime(monkeypatch, wave=True)
    new, new_g, batch = util.hip_render(cams, rv, dc, dd, da)

    # the scene is what the docstring says, and the bins are sorted by (depth bits, index)
    st = util.decode_state(batch)
    assert st["status"][0] == 0
    tile = 1 * (W // 16) + 1
    np.testing.assert_array_equal(st["tile_count"][:, tile], np.full(V, n, np.uint32))
    for v in range(V):
        for t in np.nonzero(st["tile_count"][v])[0]:
            off, cnt = int(st["tile_off"][v, t]), int(st["tile_count"][v, t])
            keys = st["keys"][v, off: off + cnt]
            idx = (keys & np.uint64(0xffffffff)).astype(np.int64)
            expect = np.sort((st["depth"][v][idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64))
            assert len(np.unique(idx)) == cnt, f"view {v} tile {t}: the bin is not a permutation of its Gaussians"
            np.testing.assert_array_equal(keys, expect, err_msg=f"view {v} tile {t}: bin of {cnt} keys not sorted")

    for k in ("color", "depth", "alpha", "radii"):
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)
    assert set(new_g) == set(old_g)
    for k in new_g:
        if old_g[k] is None:
            assert new_g[k] is None, k
        else:
            np.testing.assert_array_equal(new_g[k], old_g[k], err_msg=f"gradient {k}")

    for v, (r, _) in enumerate(util.c_oracle_render_many(cams, rv)):
        np.testing.assert_array_equal(new["radii"][v], r.radii)
        check_outputs(new, r.color, r.depth, r.alpha, v)


def test_truncated_arena_in_lazy_mode_returns_zero_gradients(monkeypatch):
    """A pair arena of 512 for 640 Gaussians in lazy mode: the lists are truncated and key slots of dropped pairs hold stale,
    possibly duplicate keys.  The network sorts them like any others; outputs are finite and every gradient is exactly zero."""
    import topo4d_amd
    from scaffold import scene
    from topo4d_amd import rasterizer
    _regime(monkeypatch, wave=True)
    rv, cams = util.make_scene(20, 32, H, W, V, opacity="B", seed=4)
    P = rv["means3D"].shape[0]
    dc, _, _ = scene.output_cotangents(V, H, W, seed=5)
    dev_index = torch.device("cuda").index or 0
    rasterizer._forget_scenes()
    rasterizer._scene(0, P, H, W).capacity = 512
    rasterizer._scene(dev_index, P, H, W).capacity = 512
    topo4d_amd.set_sync_mode("lazy")
    try:
        out, g, batch = util.hip_render(cams, rv, dc)
        stt = batch.fetch_status()
        assert stt.overflow == 1 and stt.max_pairs_per_view > 512
        for k in ("color", "depth", "alpha"):
            assert np.isfinite(out[k]).all(), k
        for k, v in g.items():
            if v is not None:
                assert not v.any(), k
    finally:
        topo4d_amd.set_sync_mode("checked")
        rasterizer._forget_scenes()
