"""
The work the render kernels do once per STAGED BATCH - staging, touch masks, the four row lists of every wave with their padding,
the backward's same-splat step masks and its write-out - through the C ABI against the C oracle, with the tolerances of
tests/test_gpu_parity.py, in the throughput builds (whole tiles, 192 splats per forward batch, 128 per backward batch):
  * tiles of 127 .. 257 pairs: the last splat of a batch, a full batch, a second batch of one splat, a full second batch;
  * rows of very unequal list lengths (one long list beside three empty ones; 1, 2, 3 and 5 entries), where the padding is most of
    what a row walks;
  * a short-list render behind a long-list render through the same ViewBatch: no entry of the first may survive;
  * rows of one wave that hold the same splat in the same step (two, three and four of them), and a control with none;
  * depth and alpha cotangents (the DA instantiation);
  * a truncated pair arena in lazy mode (stale key slots).
Scenes are built in PIXELS: isotropic splats at given centres over one 16 x 16 tile, seen by a long lens down the z axis, and
every case first checks, with the kernels' own conservative test restated in numpy on the decoded state, that the lists it
means to produce are the lists it gets.
"""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_parity import check_grads, check_n_contrib, check_outputs

pytestmark = pytest.mark.gpu

F = 640.0                    # focal length in pixels: 16 px off axis tilt a splat's footprint by 6e-4 of its variance
H = W = 16


def _throughput(monkeypatch, on=True):
    """The whole-tile throughput builds of both render kernels, whatever the launch size would have picked (a one-tile launch:
    the latency forward and the segmented backward)."""
    if on:
        monkeypatch.setenv("T4D_LATENCY_TILES", "0")
        monkeypatch.setenv("T4D_NO_SEGMENTS", "1")
    else:
        monkeypatch.delenv("T4D_LATENCY_TILES", raising=False)
        monkeypatch.delenv("T4D_NO_SEGMENTS", raising=False)


def _camera(bg=(0.3, 0.1, 0.6)):
    from scaffold import reference_boundary as boundary
    K = np.array([[F, 0, W / 2.0], [0, F, H / 2.0], [0, 0, 1.0]])
    return [boundary.setup_camera(W, H, K, np.eye(4, dtype=np.float32))._replace(bg=torch.tensor(bg, dtype=torch.float32))]


def _splats(cx, cy, s_px, opacity, seed):
    """Isotropic splats whose centres project to pixel (cx[i], cy[i]) (pixel centres are integers), of scale s_px pixels (the
    rasterizer adds 0.3 to the variance) - nearest first in the order given, index order shuffled."""
    cx, cy, s_px, opacity = (np.asarray(a, np.float64) for a in np.broadcast_arrays(cx, cy, s_px, opacity))
    P = cx.size
    g = torch.Generator().manual_seed(seed)
    z = 1.0 + 1e-3 * np.arange(P)
    means = np.stack([(cx + 0.5 - W / 2.0) * z / F, (cy + 0.5 - H / 2.0) * z / F, z], 1)
    perm = torch.randperm(P, generator=g).numpy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[perm], dtype=np.float32))
    return dict(means3D=t(means), opacities=t(opacity[:, None]), scales=t(np.repeat((s_px * z / F)[:, None], 3, 1)),
                rotations=torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1), colors_precomp=torch.rand(P, 3, generator=g)), perm


def _touch(st):
    """(P, 4, 4) bool: does the kernels' conservative test put Gaussian g on the list of the 4 x 4 sub-block (sy, sx) of tile 0?
    (wave_touch_masks and cutoff_radius2 restated; the margins of the designs below are far wider than float64 against float32)"""
    xy, co = st["xy"][0].astype(np.float64), st["conic_opacity"][0].astype(np.float64)
    lnarg = np.log(np.maximum(255.0 * co[:, 3], 1e-30))
    mid, det = 0.5 * (co[:, 0] + co[:, 2]), co[:, 0] * co[:, 2] - co[:, 1] ** 2
    lmin = det / (mid + np.sqrt(np.maximum(mid * mid - det, 0.0)))
    r2 = np.where(lnarg > -1e-3, 2.0 * (lnarg + 2e-3) / lmin * 1.001, -1.0)
    x0 = 4.0 * np.arange(4)
    d = lambda p: np.maximum(np.maximum(x0[None, :] - p[:, None], p[:, None] - (x0[None, :] + 3.0)), 0.0)
    return d(xy[:, 1])[:, :, None] ** 2 + d(xy[:, 0])[:, None, :] ** 2 <= r2[:, None, None]


def _rows_of_wave(touch, w):
    """(P, 4) bool: the four row lists of wave w (its 8 x 8 block is (w & 1, w >> 1), row r the sub-block (r & 1, r >> 1) in it)"""
    return np.stack([touch[:, 2 * (w >> 1) + (r >> 1), 2 * (w & 1) + (r & 1)] for r in range(4)], 1)


def _against_the_oracle(rv, cams, dc, dd=None, da=None, n_pairs=None):
    hip, hg, batch = util.hip_render(cams, rv, dc, dd, da)
    st = util.decode_state(batch)
    if n_pairs is not None:
        assert int(st["tile_count"][0, 0]) == n_pairs
    r, g = util.c_oracle_render(cams[0], rv, dc[0], None if dd is None else dd[0], None if da is None else da[0])
    np.testing.assert_array_equal(hip["radii"][0], r.radii)
    check_n_contrib(st["n_contrib"][0], r.state()["n_contrib"])
    check_outputs(hip, r.color, r.depth, r.alpha, 0)
    check_grads(hg, g, 0)
    return hip, hg, st


def _sub_block_centres(n, rng, jitter=0.3):
    """n centres dealt to the sixteen sub-blocks in turn, near each one's middle"""
    i = np.arange(n)
    return 4.0 * (i % 4) + 1.5 + rng.uniform(-jitter, jitter, n), 4.0 * ((i // 4) % 4) + 1.5 + rng.uniform(-jitter, jitter, n)


@pytest.mark.parametrize("n", [127, 128, 129, 191, 192, 193, 256, 257])
def test_batch_edges(n, monkeypatch):
    """One tile of n pairs dealt over all sixteen sub-blocks - small faint splats (opacity 0.1: sixteen and more behind one
    another leave every pixel unsaturated, so the last batch is live), every fifth one wide enough to reach its neighbours."""
    from scaffold import scene
    _throughput(monkeypatch)
    rng = np.random.default_rng(100 + n)
    cx, cy = _sub_block_centres(n, rng)
    s = np.where(np.arange(n) % 5 == 4, 1.5, 0.3)
    rv, _ = _splats(cx, cy, s, 0.1, seed=n)
    dc, _, _ = scene.output_cotangents(1, H, W, seed=n + 1)
    _, _, st = _against_the_oracle(rv, _camera(), dc, n_pairs=n)
    touch = _touch(st)
    assert touch.reshape(n, 16).any(axis=0).all() and (touch.reshape(n, 16).sum(axis=1) > 1).any()
    assert int(st["n_contrib"].max()) > (n - 1) // 128 * 128                 # the backward's last batch is read


@pytest.mark.parametrize("lengths", [(0, 0, 40, 0), (1, 2, 3, 5)])
def test_unequal_rows(lengths, monkeypatch):
    """All splats inside the four sub-blocks of wave 1, lengths[r] of them in row r and none reaching another sub-block: the
    other rows walk padding for most of - or all of - the longest row's steps; 40 is a list ten groups long beside three empty
    ones, (1, 2, 3, 5) the padding to a group of four and the three entries a walk may fetch beyond it."""
    from scaffold import scene
    _throughput(monkeypatch)
    rng = np.random.default_rng(7)
    w = 1
    cx = np.concatenate([8.0 * (w & 1) + 4.0 * (r & 1) + 1.5 + rng.uniform(-0.2, 0.2, k) for r, k in enumerate(lengths)])
    cy = np.concatenate([8.0 * (w >> 1) + 4.0 * (r >> 1) + 1.5 + rng.uniform(-0.2, 0.2, k) for r, k in enumerate(lengths)])
    rv, _ = _splats(cx, cy, 0.4, 0.3, seed=sum(lengths))
    dc, _, _ = scene.output_cotangents(1, H, W, seed=12)
    _, _, st = _against_the_oracle(rv, _camera(), dc, n_pairs=sum(lengths))
    touch = _touch(st)
    assert tuple(_rows_of_wave(touch, w).sum(axis=0)) == lengths
    assert int(touch.sum()) == sum(lengths)                                  # nothing on any other wave's lists


def _render_through(batch, rv, dc, dev="cuda"):
    d = lambda k: rv[k].to(dev)
    color, radii, depth, alpha = batch.forward(d("means3D"), d("opacities"), d("scales"), d("rotations"), d("colors_precomp"))
    out = dict(color=color.cpu().numpy(), radii=radii.cpu().numpy(), depth=depth.cpu().numpy(), alpha=alpha.cpu().numpy())
    g = batch.backward(dc.to(dev), None, None)
    return out, {k: (v.cpu().numpy() if v is not None else None) for k, v in g.items()}


def test_no_stale_entries_behind_a_longer_render(monkeypatch):
    """200 splats as wide as the tile (every row list longer than a backward batch), then - through the SAME ViewBatch - 200 splats of
    which 189 sit behind the camera and eleven make lists of 1, 2, 3 and 5 entries in one wave: whatever the first render left in
    the lists must be gone.  The second render equals a fresh batch's byte for byte."""
    from scaffold import scene
    from topo4d_amd import ViewBatch, pack_views
    _throughput(monkeypatch)
    rng = np.random.default_rng(21)
    P = 200
    cams = _camera()
    dev = torch.device("cuda")
    dc, _, _ = scene.output_cotangents(1, H, W, seed=22)
    long_rv, _ = _splats(rng.uniform(0, 15, P), rng.uniform(0, 15, P), 6.0, 0.05, seed=23)
    lengths = (1, 2, 3, 5)
    cx = np.concatenate([4.0 * (r & 1) + 1.5 + rng.uniform(-0.2, 0.2, k) for r, k in enumerate(lengths)] + [np.full(P - 11, 8.0)])
    cy = np.concatenate([4.0 * (r >> 1) + 1.5 + rng.uniform(-0.2, 0.2, k) for r, k in enumerate(lengths)] + [np.full(P - 11, 8.0)])
    short_rv, perm = _splats(cx, cy, 0.4, 0.3, seed=24)
    behind = torch.from_numpy(perm >= 11)                                    # (_splats shuffles: row i holds splat perm[i])
    short_rv["means3D"][behind, 2] = -1.0
    batch = ViewBatch(pack_views(util.to_device(cams, dev), dev), H, W, 1.0, 0)
    out_long, _ = _render_through(batch, long_rv, dc)
    st = util.decode_state(batch)
    assert int(st["tile_count"][0, 0]) == P and _touch(st).reshape(P, 16).sum(axis=0).min() > 128
    out, g = _render_through(batch, short_rv, dc)
    assert int(util.decode_state(batch)["tile_count"][0, 0]) == 11
    fresh = ViewBatch(pack_views(util.to_device(cams, dev), dev), H, W, 1.0, 0)
    out_f, g_f = _render_through(fresh, short_rv, dc)
    for k in out:
        np.testing.assert_array_equal(out[k], out_f[k])
    for k in g:
        if g[k] is not None:
            np.testing.assert_array_equal(g[k], g_f[k])
    r, go = util.c_oracle_render(cams[0], short_rv, dc[0])
    check_outputs(out, r.color, r.depth, r.alpha, 0)
    check_grads(g, go, 0)


def _conflict_scene(kind, seed):
    """Twelve splats per wave, all of one footprint, so that the rows they reach hold IDENTICAL lists - the same splat in the same
    step of two, three or four rows:
      wave 0: centred on the wave's middle (3.5, 3.5), reach 1.4: all four sub-blocks;
      wave 1: on the edge between rows 0 and 1 at (3.5, 1.5), reach 1.4: those two;
      wave 2: at (3, 3) - inside row 0, one pixel from rows 1 and 2, 1.41 from row 3 - reach 1.2: three;
      wave 3: in the middle of row 2, reach 1.4: one sub-block, as has every splat of the control ("none": all four waves)."""
    rng = np.random.default_rng(seed)
    k = 12
    jit = lambda: rng.uniform(-0.02, 0.02, k)
    if kind == "none":
        cx, cy = _sub_block_centres(4 * k, rng, jitter=0.2)
        return cx, cy, np.full(4 * k, 0.1), np.full(4 * k, 0.08)
    at = [(3.5, 3.5, 0.08), (8 + 3.5, 1.5, 0.08), (3.0, 8 + 3.0, 0.04), (8 + 1.5, 8 + 5.5, 0.08)]
    cx = np.concatenate([x + jit() for x, _, _ in at])
    cy = np.concatenate([y + jit() for _, y, _ in at])
    # reach = sigma sqrt(2 ln(255 opacity)), sigma^2 = 0.3 + 0.01: 1.37 at opacity 0.08, 1.19 at 0.04
    return cx, cy, np.full(4 * k, 0.1), np.concatenate([np.full(k, o) for _, _, o in at])


@pytest.mark.parametrize("kind,depth_alpha", [("same", False), ("none", False), ("same", True)])
def test_rows_that_hold_the_same_splat_in_the_same_step(kind, depth_alpha, monkeypatch):
    """Gradients against the oracle where two, three and four rows of a wave add to one slab entry in one step (and where none
    does), without and with depth and alpha cotangents; and the throughput build against the default one - one slab per row, no
    turns to take: the forward byte for byte, the gradients to the summation-order bound of
    test_latency_and_throughput_builds_agree."""
    from scaffold import scene
    cx, cy, s, op = _conflict_scene(kind, seed=31)
    rv, _ = _splats(cx, cy, s, op, seed=32)
    cams = _camera()
    dc, dd, da = scene.output_cotangents(1, H, W, seed=33, depth_alpha=True)
    if not depth_alpha:
        dd = da = None
    _throughput(monkeypatch)
    hip, hg, st = _against_the_oracle(rv, cams, dc, dd, da, n_pairs=48)
    touch = _touch(st)
    per_splat = np.stack([_rows_of_wave(touch, w).sum(axis=1) for w in range(4)], 1)          # (P, wave): rows that hold it
    if kind == "none":
        assert (touch.reshape(48, 16).sum(axis=1) == 1).all()
    else:
        assert sorted(per_splat.max(axis=1).tolist()) == [1] * 12 + [2] * 12 + [3] * 12 + [4] * 12
        assert (touch.reshape(48, 16).sum(axis=1) == per_splat.max(axis=1)).all()             # ... and no other wave's
        # every reached row SEES its twelve splats (the backward trims a row's list at its last contributor)
        for w, rows in ((0, 4), (1, 2), (2, 3), (3, 1)):
            reached = np.flatnonzero(_rows_of_wave(touch, w).any(axis=0))
            assert len(reached) == rows
            for r in reached:
                y0, x0 = 8 * (w >> 1) + 4 * (r >> 1), 8 * (w & 1) + 4 * (r & 1)
                assert int(st["n_contrib"][0, y0:y0 + 4, x0:x0 + 4].max()) == 12 * w + 12, (w, r)      # wave w's are 12 w .. 12 w + 11
    _throughput(monkeypatch, on=False)
    dflt, dg, _ = util.hip_render(cams, rv, dc, dd, da)
    for k in hip:
        np.testing.assert_array_equal(hip[k], dflt[k])
    for k in hg:
        if hg[k] is not None:
            scale = np.abs(hg[k]).max()
            assert np.abs(hg[k].astype(np.float64) - dg[k]).max() <= 2e-6 * scale + 1e-12, k


def test_truncated_arena_in_lazy_mode(monkeypatch):
    """Two views of 64 x 64, 640 Gaussians, a pair arena of 512 in lazy mode: the lists are truncated and key slots of dropped
    pairs hold stale bytes (g >= P).  The throughput builds stage such a batch without reading out of range; outputs are finite
    and every gradient is exactly zero."""
    import topo4d_amd
    from scaffold import scene
    from topo4d_amd import rasterizer
    _throughput(monkeypatch)
    Hh = Ww = 64
    rv, cams = util.make_scene(20, 32, Hh, Ww, 2, opacity="B", seed=4)
    assert rv["means3D"].shape[0] == 640
    dc, _, _ = scene.output_cotangents(2, Hh, Ww, seed=5)
    dev_index = torch.device("cuda").index or 0
    rasterizer._forget_scenes()
    rasterizer._scene(0, 640, Hh, Ww).capacity = 512
    rasterizer._scene(dev_index, 640, Hh, Ww).capacity = 512
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
