"""CPU: the float64 yardsticks of the two-band projection (tests/projtex_bands_ref.py) on hand-worked low bands, their agreement
with the yardsticks of "weighted" and "best" where the rule says so, what two bands buy on misregistered views, the argument
checks of the wrappers and of the two C entry points, and the command-line parsers.  No GPU.

What two bands buy (test_two_bands_keep_the_detail_of_best_and_the_seams_of_weighted): the patch of tests/projtex_scenes.py at
128 x 128 texels under three 192 x 160 views of focal lengths 210 / 200 / 200; views 1 and 2 are photographed aiming at
(0.02, 0, 0) and (0, 0.02, 0) but projected with cameras aiming at the origin, about 1.4 px off.  Compared are the texels all
three views see, six texels inside the island.  "Detail energy kept", on smooth_texture + 0.12 x 5x5-box-filtered unit Gaussian
noise: with E(T) the sum of (T_a - T_b)^2 over the pairs a, b of compared texels that are horizontal or vertical neighbours and
over the three channels, E(result - smooth_texture) / E(detail): what is left of the texel-to-texel variation.  (The issue states
no formula; this one gives figures within 0.01 of its table, whose noise had another seed.)  "Largest neighbour step", on
smooth_texture under exposures 1.0 / 0.85 / 1.15 without gains: the largest |difference| of two compared texels that are
horizontal or vertical neighbours, over the channels.  The figures of the float64 restatements, as measured, are the constants
below; the asserted conditions are the four ratios."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import meshrender_ref, projtex_bands_ref as bands, projtex_eq_ref as eq, projtex_ref as ref, projtex_scenes as S
from tests.test_meshrender_host import look_at_view

# the figures of test_two_bands_keep_the_detail_of_best_and_the_seams_of_weighted, as measured (radius 3, radius 6 for two bands)
COMPARED_TEXELS = 3853
DETAIL_KEPT = dict(weighted=0.35284, best=0.57352, twoband=(0.53777, 0.55370))
LARGEST_STEP = dict(truth=0.011810, weighted=0.012373, best=0.123220, twoband=(0.012784, 0.013655))


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- hand-worked low bands -------------------------------------------------------------------------------------------------------
def _three_by_four():
    """values 1 .. 12 row by row, the pixel (1, 1) off the mesh and holding a NaN; the other channels are 2 x and 0.5 + the first"""
    base = np.arange(1.0, 13.0).reshape(3, 4)
    photo = np.stack([base, 2.0 * base, base + 0.5]).astype(np.float32)
    depth = np.full((1, 1, 3, 4), 2.5, np.float32)
    depth[0, 0, 1, 1] = 0.0
    photo[:, 1, 1] = np.nan
    return photo[None], depth


def test_low_band_of_a_three_by_four_image_with_a_hole():
    photos, depth = _three_by_four()
    # per pixel (sum, number) of the values of the 3x3 box that lie in the image and are not the hole (which holds 6)
    want = [[(1 + 2 + 5, 3), (1 + 2 + 3 + 5 + 7, 5), (2 + 3 + 4 + 7 + 8, 5), (3 + 4 + 7 + 8, 4)],
            [(1 + 2 + 5 + 9 + 10, 5), (1 + 2 + 3 + 5 + 7 + 9 + 10 + 11, 8), (2 + 3 + 4 + 7 + 8 + 10 + 11 + 12, 8), (3 + 4 + 7 + 8 + 11 + 12, 6)],
            [(5 + 9 + 10, 3), (5 + 7 + 9 + 10 + 11, 5), (7 + 8 + 10 + 11 + 12, 5), (7 + 8 + 11 + 12, 4)]]
    low = bands.low_band(photos, depth, 1)
    assert low.shape == (1, 3, 3, 4) and low.dtype == np.float32 and np.isfinite(low).all()     # the NaN off the mesh stays out
    for r in range(3):
        for c in range(4):
            s, n = want[r][c]
            assert low[0, 0, r, c] == np.float32(s / n), (r, c)
            assert low[0, 1, r, c] == np.float32(2 * s / n) and low[0, 2, r, c] == np.float32((s + 0.5 * n) / n)
    assert low[0, 0, 1, 1] == 6.0                                # the hole itself takes the mean of its neighbours
    # radius 0: the photograph on the mesh, 0 off it
    on = depth[0, 0] > 0
    same = bands.low_band(photos, depth, 0)
    assert np.array_equal(bits(same[0][:, on]), bits(photos[0][:, on])) and not same[0][:, ~on].any()
    # a radius larger than the image: every box holds the whole mesh
    wide = bands.low_band(photos, depth, 5)
    assert (wide[0, 0] == np.float32((78 - 6) / 11)).all() and (wide[0, 1] == np.float32(2 * (78 - 6) / 11)).all()
    # no mesh in the view: zeros, whatever the photograph holds
    assert not bands.low_band(photos, np.zeros_like(depth), 1).any() and not bands.low_band(photos, np.zeros_like(depth), 0).any()
    # a box that holds no mesh pixel: only the corner (0, 0) is on the mesh, radius 1 reaches columns 0 .. 1 and rows 0 .. 1
    corner = np.zeros_like(depth)
    corner[0, 0, 0, 0] = 1.0
    got = bands.low_band(photos, corner, 1)[0, 0]
    assert (got[:2, :2] == 1.0).all() and not got[2].any() and not got[:, 2:].any()


def test_a_nan_only_spreads_from_the_mesh():
    rng = np.random.default_rng(3)
    photos = rng.uniform(0, 1, size=(2, 3, 9, 11)).astype(np.float32)
    depth = (rng.uniform(0, 1, size=(2, 1, 9, 11)) > 0.4).astype(np.float32)
    clean = bands.low_band(photos, depth, 2)
    off = np.argwhere(depth[1, 0] == 0)[0]
    dirty = photos.copy()
    dirty[1, :, off[0], off[1]] = np.nan
    assert np.array_equal(bits(bands.low_band(dirty, depth, 2)), bits(clean))
    on = np.argwhere(depth[1, 0] > 0)[0]
    dirty = photos.copy()
    dirty[1, 0, on[0], on[1]] = np.nan
    got = bands.low_band(dirty, depth, 2)
    y, x = np.mgrid[0:9, 0:11]
    near = (np.abs(y - on[0]) <= 2) & (np.abs(x - on[1]) <= 2)
    assert np.isnan(got[1, 0][near]).all() and np.isfinite(got[1, 0][~near]).all() and np.isfinite(got[0]).all() and np.isfinite(got[1, 1:]).all()


# ---- against the yardsticks of "weighted" and "best" -----------------------------------------------------------------------------
def _quads(res, seed=0, n_views=3):
    from topo4d_amd.meshrender import triangulate
    obj, views = S.three_quads(), S.three_views()[:n_views]
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    depth = np.stack([meshrender_ref.render(obj.vertices, tris, uv_tris, obj.uvs, np.zeros((1, 1, 3), np.uint8), v, S.H, S.W)[1] for v in views])
    photos = np.random.default_rng(seed).uniform(0, 1, size=(n_views, 3, S.H, S.W)).astype(np.float32)
    return S.quad_maps64(obj, *res), views, photos, depth


GAINS = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])


def test_radius_zero_is_the_weighted_projection_with_no_detail():
    (pos, nrm, cov), views, photos, depth = _quads((40, 56))
    low = bands.low_band(photos, depth, 0)
    for kw in (dict(depth_tol=0.02), dict(depth_tol=0.02, power=0, fade_px=0.0, cos_min=0.3)):
        for gains in (None, GAINS):
            lc, weight, count, high, bw = bands.project_bands(pos, nrm, cov, views, S.H, S.W, photos, low, depth, gains=gains, **kw)
            if gains is None:
                want = ref.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth, mode="weighted", **kw)
                best = ref.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth, mode="best", **kw)
            else:
                want = eq.project_texture_gains(pos, nrm, cov, views, S.H, S.W, photos, depth, mode="weighted", gains=gains, **kw)
                best = eq.project_texture_gains(pos, nrm, cov, views, S.H, S.W, photos, depth, mode="best", gains=gains, **kw)
            assert count.max() == 3 and (count == 2).any()
            assert not bits(high).any()                          # exactly +0: the low band under an accepted view's taps is the photograph
            for g, w, name in zip((lc, weight, count), want, ("low_color", "weight", "count")):
                assert np.array_equal(bits(g), bits(w)), name
            assert np.array_equal(bits(bw), bits(best[1]))
            assert lc.dtype == weight.dtype == high.dtype == bw.dtype == np.float32 and count.dtype == np.uint8


def test_one_view_gives_the_best_view_whatever_the_radius():
    (pos, nrm, cov), views, photos, depth = _quads((40, 56), seed=2, n_views=1)
    want = ref.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth, mode="best", depth_tol=0.02)
    assert (want[2] == 1).sum() > 300
    for radius in (1, 4, 32):
        low = bands.low_band(photos, depth, radius)
        lc, weight, count, high, bw = bands.project_bands(pos, nrm, cov, views, S.H, S.W, photos, low, depth, depth_tol=0.02)
        err = np.abs((lc + high).astype(np.float64) - want[0]).max()
        print("radius", radius, "max |low + high - best|", err)
        assert err <= 1e-6
        assert np.array_equal(bits(bw), bits(want[1])) and np.array_equal(bits(weight), bits(want[1])) and np.array_equal(count, want[2])
        assert np.abs(high).max() > 0.1                          # random photographs: the detail is most of the picture
        assert not lc[count == 0].any() and not high[count == 0].any()


def test_ties_keep_the_lower_view_and_the_best_view_alone_gives_the_detail():
    view = look_at_view([0, 0, -2], [0, 0, 0], 24, 32, f=40.0)
    side = look_at_view([1.5, 0, -2], [0, 0, 0], 24, 32, f=40.0)
    photos = np.random.default_rng(1).uniform(0, 1, size=(3, 3, 24, 32)).astype(np.float32)
    depth = np.full((3, 1, 24, 32), 1e3, np.float32)
    low = bands.low_band(photos, depth, 2)
    pos, nrm, cov = np.zeros((1, 1, 3), np.float32), np.array([[[0, 0, -1]]], np.float32), np.ones((1, 1), np.uint8)
    one = lambda vs, k: [a[0, 0] for a in bands.project_bands(pos, nrm, cov, np.stack(vs), 24, 32, photos[k], low[k], depth[k], fade_px=0.0)]
    alone = [one([view], [0]), one([view], [1]), one([side], [2])]
    lc, w, n, high, bw = one([view, view, side], [0, 1, 2])
    assert n == 3 and bw == 1.0 and np.array_equal(high, alone[0][3])                    # the tie goes to the lower view
    w2 = float(alone[2][1])
    assert 0.5 < w2 < 0.7 and abs(float(w) - (2.0 + w2)) < 1e-6
    mix = (alone[0][0].astype(np.float64) + alone[1][0] + w2 * alone[2][0]) / (2.0 + w2)
    assert np.abs(lc - mix).max() < 1e-6
    lc, w, n, high, bw = one([side, view, view], [2, 1, 0])
    assert n == 3 and bw == 1.0 and np.array_equal(high, alone[1][3])


# ---- what two bands buy ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def misregistered():
    """the patch under three views; views 1 and 2 are photographed with a camera that aims a little off the one they are projected with"""
    from topo4d_amd.meshrender import triangulate
    obj, verts = S.patch_scene()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    h, w = 160, 192
    eyes = ([0.0, 0.0, -3.0], 210.0, 0.0), ([1.2, 0.3, -2.8], 200.0, 0.0), ([-1.0, -0.5, -2.9], 200.0, 0.3)
    aims = ([0.0, 0.0, 0.0], [0.02, 0.0, 0.0], [0.0, 0.02, 0.0])
    views = np.stack([S.view(eye, [0, 0, 0], h, w, f=f, roll=roll) for eye, f, roll in eyes])
    shot_with = np.stack([S.view(eye, aim, h, w, f=f, roll=roll) for (eye, f, roll), aim in zip(eyes, aims)])
    smooth = S.smooth_texture(128, 128)
    noise = np.random.default_rng(0).standard_normal((128 + 4, 128 + 4, 3))
    box = sum(noise[dy:dy + 128, dx:dx + 128] for dy in range(5) for dx in range(5)) / 25.0
    detail = (0.12 * box).astype(np.float32)

    def shoot(tex):
        shots = [meshrender_ref.render(verts, tris, uv_tris, obj.uvs, tex, v, h, w) for v in shot_with]
        return np.stack([s[0] for s in shots])

    depth = np.stack([meshrender_ref.render(verts, tris, uv_tris, obj.uvs, smooth, v, h, w)[1] for v in views])
    pos, nrm, cov = S.patch_maps64(128)
    return dict(views=views, h=h, w=w, depth=depth, pos=pos, nrm=nrm, cov=cov, smooth=smooth, detail=detail,
                photos_detail=shoot(smooth + detail), photos_smooth=shoot(smooth))


def _three_ways(m, photos, radii=(3, 6)):
    a = (m["pos"], m["nrm"], m["cov"], m["views"], m["h"], m["w"], photos, m["depth"])
    out = {mode: ref.project_texture(*a, mode=mode) for mode in ("weighted", "best")}
    for r in radii:
        out[r] = bands.twoband(*a, r)
    seen = S.erode(m["cov"], 6) & (out["weighted"][2] == 3)
    assert all(np.array_equal(o[2], out["weighted"][2]) for o in out.values())
    return {k: o[0].astype(np.float64) for k, o in out.items()}, seen


def _neighbour_steps(t, seen):
    """the differences of the pairs of compared texels that are horizontal or vertical neighbours, all channels"""
    across = (t[:, 1:] - t[:, :-1])[seen[:, 1:] & seen[:, :-1]]
    down = (t[1:] - t[:-1])[seen[1:] & seen[:-1]]
    return np.concatenate([across.reshape(-1), down.reshape(-1)])


def _largest_step(t, seen):
    return np.abs(_neighbour_steps(t, seen)).max()


def _detail_energy(t, seen):
    return (_neighbour_steps(t, seen) ** 2).sum()


def test_two_bands_keep_the_detail_of_best_and_the_seams_of_weighted(misregistered):
    m = misregistered
    out, seen = _three_ways(m, m["photos_detail"])
    n = int(seen.sum())
    truth = _detail_energy(m["detail"].astype(np.float64), seen)
    kept = {k: _detail_energy(o - m["smooth"].astype(np.float64), seen) / truth for k, o in out.items()}
    print("compared texels", n)
    print("detail energy kept", {k: round(float(v), 5) for k, v in kept.items()})
    assert n >= 3000 and n == COMPARED_TEXELS
    for r, rec in zip((3, 6), DETAIL_KEPT["twoband"]):
        print("radius", r, "kept / best", kept[r] / kept["best"], "kept / weighted", kept[r] / kept["weighted"])
        assert kept[r] >= 0.9 * kept["best"]
        assert kept[r] >= 1.3 * kept["weighted"]
        assert abs(kept[r] - rec) <= 1e-4
    assert abs(kept["weighted"] - DETAIL_KEPT["weighted"]) <= 1e-4 and abs(kept["best"] - DETAIL_KEPT["best"]) <= 1e-4
    # exposure: the cameras differ by 15 % either way and nobody equalises them
    exposed = m["photos_smooth"] * np.array([1.0, 0.85, 1.15], np.float32)[:, None, None, None]
    out, seen2 = _three_ways(m, exposed)
    assert np.array_equal(seen, seen2)
    step = {k: float(_largest_step(o, seen)) for k, o in out.items()}
    step["truth"] = float(_largest_step(m["smooth"].astype(np.float64), seen))
    print("largest neighbour step", {k: round(v, 6) for k, v in step.items()})
    for r, rec in zip((3, 6), LARGEST_STEP["twoband"]):
        print("radius", r, "step / weighted", step[r] / step["weighted"], "step / best", step[r] / step["best"])
        assert step[r] <= 1.25 * step["weighted"]
        assert step[r] <= 0.25 * step["best"]
        assert abs(step[r] - rec) <= 1e-5
    for k in ("truth", "weighted", "best"):
        assert abs(step[k] - LARGEST_STEP[k]) <= 1e-5


# ---- arguments, parsers ------------------------------------------------------------------------------------------------------------
H, W = 24, 32


def test_argument_errors_are_raised_without_a_device():
    from topo4d_amd import projtex
    view = torch.from_numpy(look_at_view([0, 0, -2], [0, 0, 0], H, W, f=40.0))[None]
    photos, depth = torch.zeros(1, 3, H, W), torch.zeros(1, 1, H, W)
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.low_band(photos, depth, 8)
    for radius in (0, 32, np.int64(5), 4.0):
        projtex.check_band_options(radius)
    for radius in (-1, 33, 1.5, True, "8", None, float("nan")):
        with pytest.raises(ValueError):
            projtex.low_band(photos, depth, radius)
        with pytest.raises(ValueError):
            projtex.check_band_options(radius)
    for p, d in ((photos.double(), depth), (photos[0], depth), (photos, depth[:, 0]), (photos, torch.zeros(1, 1, H, W + 1)),
                 (torch.zeros(1, 4, H, W), depth), (photos, depth.double()), (photos.numpy(), depth)):
        with pytest.raises(ValueError):
            projtex.low_band(p, d, 8)
    good = dict(pos=torch.zeros(4, 5, 3), nrm=torch.zeros(4, 5, 3), coverage=torch.ones(4, 5, dtype=torch.uint8), cams=(view, H, W),
                photos=photos, low=torch.zeros(1, 3, H, W), depth=depth)
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.project_bands(**good)
    bad = [dict(low=torch.zeros(1, 3, H, W + 1)), dict(low=torch.zeros(2, 3, H, W)), dict(low=torch.zeros(1, 3, H, W, dtype=torch.float64)),
           dict(low=torch.zeros(1, 1, H, W)), dict(low=None), dict(photos=torch.zeros(2, 3, H, W)), dict(depth=torch.zeros(1, H, W)),
           dict(nrm=torch.zeros(4, 6, 3)), dict(coverage=torch.ones(4, 5)), dict(power=9), dict(cos_min=1.5), dict(fade_px=-1.0),
           dict(depth_tol=float("nan")), dict(gains=np.ones((2, 3))), dict(gains=np.array([[1.0, np.inf, 1.0]]))]
    for change in bad:
        with pytest.raises(ValueError):
            projtex.project_bands(**{**good, **change})
    with pytest.raises(TypeError):
        projtex.project_bands(**good, mode="weighted")           # it has no modes
    del good["low"]
    with pytest.raises(ValueError, match="project_bands"):
        projtex.project(**good, mode="twoband")
    projtex.check_options(mode="twoband")
    with pytest.raises(ValueError):
        projtex.check_options(mode="threeband")
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.project(**good)                                  # as before


def test_the_entry_points_reject_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    one, other, none = C.c_void_p(64), C.c_void_p(128), None
    ok = [one, one, 3, 40, 48, 8, other, none]
    for k, v in ((0, none), (1, none), (6, none), (2, 0), (2, 256), (3, 0), (4, 0), (3, 65537), (4, -1), (5, -1), (5, 33), (6, one)):
        args = list(ok)
        args[k] = v
        assert lib.t4d_projtex_low_band(*args) == _lib.T4D_ERR_ARG, (k, v)
        assert b"t4d_projtex_low_band" in lib.t4d_last_error()
    ok = [one, one, one, 64, 64, one, 3, 40, 48, one, one, one, none, 2, 0.1, 16.0, 0.002, one, one, one, one, one, none]
    changes = [(k, none) for k in (0, 1, 2, 5, 9, 10, 11, 17, 18, 19, 20, 21)]
    changes += [(3, 0), (4, 0), (4, 65537), (6, 0), (6, 256), (7, 0), (8, 0), (8, -1), (13, 9), (13, -1), (14, 2.0), (14, float("nan")),
                (15, -1.0), (16, -0.5), (16, 2.0)]
    for k, v in changes:
        args = list(ok)
        args[k] = v
        assert lib.t4d_project_texture_bands(*args) == _lib.T4D_ERR_ARG, (k, v)
        assert b"t4d_project_texture_bands" in lib.t4d_last_error()


def test_command_lines():
    from topo4d_amd import projtex, train
    assert projtex.DEFAULTS == dict(power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002, mode="weighted")
    assert projtex.BAND_DEFAULTS == dict(band_radius=8) and projtex._MODES == {"weighted": 0, "best": 1}
    a = projtex.build_parser().parse_args(["-e", "x"])
    assert a.band_radius == 8 and a.mode == "weighted"
    assert projtex.options_of(a) == projtex.DEFAULTS and projtex.band_options_of(a) == projtex.BAND_DEFAULTS
    assert projtex._check_args(a, 8192) == projtex.DEFAULTS     # without the flag nothing new reaches a frame or proj_gains.json
    a = projtex.build_parser().parse_args(["--mode", "twoband", "--band_radius", "3", "--power", "4", "--equalize", "--tex_pad", "2",
                                           "--tex_sizes", "4096", "--save_weight"])
    assert projtex.options_of(a) == {**projtex.DEFAULTS, "mode": "twoband", "power": 4} and projtex.band_options_of(a) == dict(band_radius=3)
    assert projtex._check_args(a, 8192) == {**projtex.DEFAULTS, "mode": "twoband", "power": 4, "band_radius": 3}
    assert (a.equalize, a.tex_pad, a.tex_sizes, a.save_weight) == (True, 2, [4096], True)
    a = projtex.build_parser().parse_args(["--mode", "twoband"])
    assert projtex._check_args(a, 8192) == {**projtex.DEFAULTS, "mode": "twoband", "band_radius": 8}
    a = projtex.build_parser().parse_args(["--mode", "best", "--band_radius", "3"])
    assert projtex._check_args(a, 8192) == {**projtex.DEFAULTS, "mode": "best"}
    for argv in (["--mode", "twoband", "--band_radius", "33"], ["--band_radius", "-1"]):
        with pytest.raises(SystemExit):
            projtex._check_args(projtex.build_parser().parse_args(argv), 8192)
    for argv in (["--mode", "threeband"], ["--band_radius", "1.5"]):
        with pytest.raises(SystemExit):
            projtex.build_parser().parse_args(argv)
    plain = train.build_parser().parse_args([])
    assert not hasattr(plain, "band_radius") and not hasattr(plain, "mode")        # absent unless given, like the other added flags
    assert projtex.band_options_of(plain) == projtex.BAND_DEFAULTS and projtex._check_args(plain, 8192) == projtex.DEFAULTS
    t = train.build_parser().parse_args(["--tex_project", "--tex_equalize", "--mode", "twoband", "--band_radius", "5", "--tex_pad", "2"])
    assert t.tex_project is True and t.tex_equalize is True
    assert projtex._check_args(t, 8192) == {**projtex.DEFAULTS, "mode": "twoband", "band_radius": 5}
    t = train.build_parser().parse_args(["--tex_project", "--mode", "twoband"])
    assert projtex._check_args(t, 8192) == {**projtex.DEFAULTS, "mode": "twoband", "band_radius": 8}
