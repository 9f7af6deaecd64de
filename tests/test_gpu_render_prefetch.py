"""
The backward render kernel's throughput build stages a batch on the waves that write no records: the next batch is requested
while the current one is written out, and a tile's first batch under the tile's pixel-state loads (csrc/t4d_raster_render_bwd.h,
PF).  These cases put batch and tile boundaries where that hand-over happens, through the C ABI against the C oracle with the
tolerances of tests/test_gpu_parity.py and the per-row check of tests/grad_rows.py, and bit for bit between calls:
  * one and three views of 128 x 96 whose chosen tiles hold exactly 1, 127, 128, 129, 192, 193, 256, 257 and 385 pairs, every
    other tile none: a last batch of one splat, full batches, a tile of three (four) backward batches, two forward batches;
  * forty views of the same size with 42 of 48 tiles in use: more non-empty tiles than either kernel launches tile workgroups
    (the grid is min(tiles, 6 or 4 per CU of 256 CUs) = 1,536 / 1,024 - no handle shrinks it below that, so the launch is made
    larger than it), so a workgroup meets a tile behind a tile, two batches behind one, and an empty item that ends its loop;
  * lazy mode with a pair arena one pair too small: stale key slots (g >= P) go through the same staging.
A big one-view launch (the LONG builds, a skipped long tile between two short ones) needs millions of pairs and is left to
tests/test_gpu_parity.py::test_long_tiles_of_a_big_one_view_launch_are_segmented and tests/test_gpu_fullsize.py.
Scenes are built in PIXELS, as in tests/test_gpu_batch_fixed_work.py: small faint isotropic splats (scale 0.3 px, opacity 0.1,
3-sigma radius 2 px) at least 4 px inside their tile, nearly coplanar (depth 1 + 1e-5 i), seen down the z axis by a long lens;
the further views are the same camera moved by one tile to either side.  The exact-count scene needs as many Gaussians as its
tiles hold pairs (1,668).
"""
import functools

import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_parity import check_grads, check_n_contrib, check_outputs

pytestmark = pytest.mark.gpu

F = 640.0
H, W = 96, 128
GX, GY = W // 16, H // 16
LAYOUT = {(1, 0): 1, (3, 0): 127, (5, 0): 128, (1, 2): 129, (3, 2): 192, (5, 2): 193, (1, 4): 256, (3, 4): 257, (5, 4): 385}
DZ = 1e-5


def _throughput(monkeypatch):
    """The whole-tile throughput builds of both render kernels, whatever the launch size would have picked (the switch of the
    render_build fixture)."""
    monkeypatch.setenv("T4D_LATENCY_TILES", "0")
    monkeypatch.setenv("T4D_NO_SEGMENTS", "1")


def _camera(shift_tiles=0, bg=(0.3, 0.1, 0.6)):
    """The camera moved so that the image moves by shift_tiles tiles in x (to within 16 DZ P px: depths are 1 .. 1 + DZ P)"""
    from scaffold import reference_boundary as boundary
    K = np.array([[F, 0, W / 2.0], [0, F, H / 2.0], [0, 0, 1.0]])
    w2c = np.eye(4, dtype=np.float32)
    w2c[0, 3] = 16.0 * shift_tiles / F
    return boundary.setup_camera(W, H, K, w2c)._replace(bg=torch.tensor(bg, dtype=torch.float32))


def _splats(cx, cy, seed, s_px=0.3, opacity=0.1):
    cx, cy = np.asarray(cx, np.float64), np.asarray(cy, np.float64)
    P = cx.size
    g = torch.Generator().manual_seed(seed)
    z = 1.0 + DZ * np.arange(P)
    means = np.stack([(cx + 0.5 - W / 2.0) * z / F, (cy + 0.5 - H / 2.0) * z / F, z], 1)
    perm = torch.randperm(P, generator=g).numpy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[perm], dtype=np.float32))
    return dict(means3D=t(means), opacities=t(np.full((P, 1), opacity)), scales=t(np.repeat((s_px * z / F)[:, None], 3, 1)),
                rotations=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1), colors_precomp=torch.rand(P, 3, generator=g))


def _in_tiles(counts, seed):
    """counts[(tx, ty)] splats in the middle 8 x 8 pixels of tile (tx, ty), depth order shuffled across the tiles"""
    rng = np.random.default_rng(seed)
    cx, cy = [], []
    for (tx, ty), n in counts.items():
        cx.append(16.0 * tx + rng.uniform(4.0, 11.0, n))
        cy.append(16.0 * ty + rng.uniform(4.0, 11.0, n))
    order = rng.permutation(sum(counts.values()))
    return np.concatenate(cx)[order], np.concatenate(cy)[order]


def _tile_counts(counts, shift=0):
    t = np.zeros((GY, GX), np.uint32)
    for (tx, ty), n in counts.items():
        t[ty, tx + shift] = n
    return t.reshape(-1)


@functools.lru_cache(maxsize=None)
def _edge_scene(V):
    """(rv, cams, (dc, dd, da), [(oracle render, colour-only grads, all-cotangent grads) per view]) - computed once, left unchanged"""
    from scaffold import scene
    rv = _splats(*_in_tiles(LAYOUT, seed=5), seed=6)
    shifts = [0] if V == 1 else [-1, 0, 1]
    cams = [_camera(s) for s in shifts]
    cot = scene.output_cotangents(V, H, W, seed=7, depth_alpha=True)
    ref = []
    for v, (r, g) in enumerate(util.c_oracle_render_many(cams, rv, cot[0])):
        ref.append((r, g, r.backward(cot[0][v], cot[1][v], cot[2][v])))
    return rv, cams, cot, shifts, ref


def _check_edge_scene(V, depth_alpha, out, grads, batch):
    rv, cams, cot, shifts, ref = _edge_scene(V)
    total = sum(LAYOUT.values())
    stt = batch.fetch_status()
    assert stt.overflow == 0 and stt.max_pairs_per_view == total
    st = util.decode_state(batch)
    for v in range(V):
        r, g_c, g_da = ref[v]
        want = _tile_counts(LAYOUT, shifts[v])
        np.testing.assert_array_equal(st["tile_count"][v], want)
        ranges = r.state()["ranges"]
        np.testing.assert_array_equal(ranges[:, 1] - ranges[:, 0], want)
        np.testing.assert_array_equal(out["radii"][v], r.radii)
        check_n_contrib(st["n_contrib"][v], r.state()["n_contrib"])
        check_outputs(out, r.color, r.depth, r.alpha, v)
        check_grads(grads, g_da if depth_alpha else g_c, v)
        # every batch of every tile is read by the backward: some pixel's last contributor lies in the tile's last batch
        for (tx, ty), n in LAYOUT.items():
            x0, y0 = 16 * (tx + shifts[v]), 16 * ty
            assert int(st["n_contrib"][v, y0:y0 + 16, x0:x0 + 16].max()) > (n - 1) // 128 * 128, (tx, ty, n)


@pytest.mark.parametrize("depth_alpha", [False, True])
@pytest.mark.parametrize("V", [1, 3])
def test_tiles_of_exact_pair_counts(V, depth_alpha, monkeypatch):
    """Outputs, state and gradients against the C oracle, and a second call bit for bit."""
    _throughput(monkeypatch)
    rv, cams, (dc, dd, da), _, _ = _edge_scene(V)
    if not depth_alpha:
        dd = da = None
    out, grads, batch = util.hip_render(cams, rv, dc, dd, da)
    _check_edge_scene(V, depth_alpha, out, grads, batch)
    again, grads2, _ = util.hip_render(cams, rv, dc, dd, da)
    for k in out:
        np.testing.assert_array_equal(out[k], again[k])
    for k in grads:
        if grads[k] is not None:
            np.testing.assert_array_equal(grads[k], grads2[k])


def test_gradients_row_by_row(monkeypatch):
    """Every Gaussian of the one-view scene against the float64 oracle, relative to its own row scale (tests/grad_rows.py).  The
    scene qualifies as a row-check case: the C oracle and the float64 oracle take every discrete decision the same way."""
    from tests import grad_rows
    _throughput(monkeypatch)
    rv, cams, (dc, _, _), _, ref = _edge_scene(1)
    outs, truth, S = grad_rows.yardstick(cams[0], rv, (dc[0], None, None))
    np.testing.assert_array_equal(np.asarray(outs["radii"]), ref[0][0].radii)
    np.testing.assert_array_equal(np.asarray(outs["n_contrib"]), ref[0][0].state()["n_contrib"])
    out, grads, batch = util.hip_render(cams, rv, dc)
    grad_rows.check_grads_rowwise(grads, truth, S, out["radii"][0], 0, xy=util.decode_state(batch)["xy"][0])


def test_one_frame_at_a_time_equals_two_batches_on_two_streams(monkeypatch):
    """The three views through one ViewBatch, and then through two ViewBatches (views 0-1 and view 2) whose forwards and backwards
    are queued on two streams side by side: bit for bit."""
    from topo4d_amd import ViewBatch, pack_views
    _throughput(monkeypatch)
    rv, cams, (dc, _, _), _, _ = _edge_scene(3)
    out, grads, _ = util.hip_render(cams, rv, dc)
    dev = torch.device("cuda")
    d = lambda k: rv[k].to(dev)
    parts = [(slice(0, 2), torch.cuda.Stream()), (slice(2, 3), torch.cuda.Stream())]
    batches, fwd, bwd = [], [], []
    torch.cuda.synchronize()
    for sl, s in parts:
        with torch.cuda.stream(s):
            b = ViewBatch(pack_views(util.to_device(cams[sl], dev), dev), H, W, 1.0, 0)
            fwd.append(b.forward(d("means3D"), d("opacities"), d("scales"), d("rotations"), d("colors_precomp")))
            batches.append(b)
    for (sl, s), b in zip(parts, batches):
        with torch.cuda.stream(s):
            bwd.append(b.backward(dc[sl].to(dev), None, None))
    torch.cuda.synchronize()
    for (sl, _), (color, radii, depth, alpha), g in zip(parts, fwd, bwd):
        for k, t in (("color", color), ("radii", radii), ("depth", depth), ("alpha", alpha)):
            np.testing.assert_array_equal(out[k][sl], t.cpu().numpy())
        for k, t in g.items():
            if t is not None:
                np.testing.assert_array_equal(grads[k][sl], t.cpu().numpy())


def test_more_tiles_than_tile_workgroups(monkeypatch):
    """Forty identical views, 42 of 48 tiles in use (1,680 non-empty tiles of 1,920; 1 .. 5 pairs each, one of 130 and one of 257 per
    view): the forward launches 1,536 tile workgroups and the backward 1,024, so workgroups take a second tile behind their
    first - a long one first, the items are ordered by length - or find an empty item there.  Every view against the one oracle
    render."""
    from scaffold import scene
    _throughput(monkeypatch)
    V = 40
    counts = {(tx, ty): 1 + (tx + GX * ty) % 5 for ty in range(GY) for tx in range(GX) if (tx + GX * ty) % 8 != 7}
    counts[(2, 1)], counts[(4, 3)] = 130, 257
    assert len(counts) == 42 and V * len(counts) > 6 * 256 and V * GX * GY > V * len(counts)
    rv = _splats(*_in_tiles(counts, seed=11), seed=12)
    cams = [_camera()] * V
    dc1, _, _ = scene.output_cotangents(1, H, W, seed=13)
    out, grads, batch = util.hip_render(cams, rv, dc1.repeat(V, 1, 1, 1))
    st = util.decode_state(batch)
    r, g = util.c_oracle_render(cams[0], rv, dc1[0])
    for v in range(V):
        np.testing.assert_array_equal(st["tile_count"][v], _tile_counts(counts))
        np.testing.assert_array_equal(out["radii"][v], r.radii)
        check_n_contrib(st["n_contrib"][v], r.state()["n_contrib"])
        check_outputs(out, r.color, r.depth, r.alpha, v)
        check_grads(grads, g, v)
    for k in out:                                            # a view does not know which workgroup round rendered it
        assert (out[k] == out[k][:1]).all(), k
    for k in grads:
        if grads[k] is not None:
            assert (grads[k] == grads[k][:1]).all(), k


def test_stale_keys_of_a_truncated_arena(monkeypatch):
    """Lazy mode with an arena ONE pair too small for the one-view scene: a pair is dropped and its key slot holds stale bytes.
    The forward outputs of every tile whose list is whole - inside the arena, no stale key in it, read from the decoded state -
    are those of the full render, bit for bit; nothing is read out of range (outputs finite), and the gradients of an
    overflowed render are zero."""
    import topo4d_amd
    from topo4d_amd import rasterizer
    _throughput(monkeypatch)
    rv, cams, (dc, _, _), _, _ = _edge_scene(1)
    full, _, _ = util.hip_render(cams, rv, dc)
    P, total = rv["means3D"].shape[0], sum(LAYOUT.values())
    dev_index = torch.device("cuda").index or 0
    rasterizer._forget_scenes()
    rasterizer._scene(0, P, H, W).capacity = total - 1
    rasterizer._scene(dev_index, P, H, W).capacity = total - 1
    topo4d_amd.set_sync_mode("lazy")
    try:
        out, g, batch = util.hip_render(cams, rv, dc)
        stt = batch.fetch_status()
        assert stt.overflow == 1 and stt.max_pairs_per_view == total
        # the truncated tiles, from the state: a list that runs past the arena, or holds a stale key
        st = util.decode_state(batch)
        off, cnt, keys = st["tile_off"][0].astype(np.int64), st["tile_count"][0].astype(np.int64), st["keys"][0]
        np.testing.assert_array_equal(cnt, _tile_counts(LAYOUT))
        stale = lambda t: bool(((keys[off[t]:min(off[t] + cnt[t], total - 1)] & 0xffffffff) >= P).any())
        truncated = np.array([cnt[t] > 0 and (off[t] + cnt[t] > total - 1 or stale(t)) for t in range(GX * GY)])
        assert truncated.any()
        differs = np.zeros((GY, GX), bool)
        for k in ("color", "depth", "alpha"):
            assert np.isfinite(out[k]).all(), k
            ne = (out[k][0] != full[k][0]).reshape(-1, GY, 16, GX, 16)
            differs |= ne.any(axis=(0, 2, 4))
        assert not differs.reshape(-1)[~truncated].any(), (np.flatnonzero(differs.reshape(-1)), np.flatnonzero(truncated))
        for k, v in g.items():
            if v is not None:
                assert not v.any(), k
    finally:
        topo4d_amd.set_sync_mode("checked")
        rasterizer._forget_scenes()
