"""CPU: the camera equalisation of topo4d_amd.projtex without a device: solve_gains against the energy it is stated to minimise,
the numpy restatement tests/projtex_eq_ref.py against tests/projtex_ref.py and against its own texel-by-texel form, the argument
checks, proj_gains.json and the command-line parsers.  No GPU."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import meshrender_ref, projtex_eq_ref as eq, projtex_ref as ref, projtex_scenes as S
from tests.test_meshrender_host import look_at_view
from topo4d_amd import projtex

# max |gain - 1| of the float64 restatement on rendered, mutually consistent photographs of one texture, as measured by
# test_consistent_photographs_give_gains_of_one below (48 x 48 texels, the defaults but depth_tol = 0.02)
CONSISTENT_DEVIATION = 3.217e-5


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- solve_gains -----------------------------------------------------------------------------------------------------------------
def _stats(V, seed, gains=None, density=1.0):
    """a consistent set of pair statistics: every pair shares N_ij texels of mean brightness m_ij, seen by camera i as m_ij / g_i"""
    rng = np.random.default_rng(seed)
    N = np.triu(rng.integers(100, 5000, size=(V, V)), 1)
    N = N * (rng.uniform(size=(V, V)) < density)
    N = N + N.T
    m = rng.uniform(0.3, 0.6, size=(V, V, 3))
    m = (m + m.transpose(1, 0, 2)) / 2
    g = np.ones((V, 3)) if gains is None else np.asarray(gains)
    sums = np.rint(N[..., None] * m / g[:, None, :] * 65536.0).astype(np.int64)
    count = N.astype(np.int64)
    count[np.arange(V), np.arange(V)] = N.sum(1)
    return count, sums


def _energy_gradient(count, sums, l, c, prior, min_overlap):
    """(dE/dl, |b|) of E(l) = sum_{i<j} N_ij (l_i - l_j + d_ij)^2 + prior sum_i n_i l_i^2, halved, written as loops"""
    V = len(count)
    grad, b = np.zeros(V), np.zeros(V)
    for i in range(V):
        for j in range(V):
            if i == j or count[i, j] < min_overlap or sums[i, j, c] == 0 or sums[j, i, c] == 0:
                continue
            d = np.log(float(sums[i, j, c])) - np.log(float(sums[j, i, c]))
            grad[i] += count[i, j] * (l[i] - l[j] + d) + prior * count[i, j] * l[i]
            b[i] -= count[i, j] * d
    return grad, np.abs(b).max()


def test_the_gradient_of_the_stated_energy_vanishes_at_the_solution():
    true = np.random.default_rng(1).uniform(0.8, 1.25, size=(7, 3))
    count, sums = _stats(7, seed=2, gains=true, density=0.7)
    sums[1, 4] = sums[4, 1] // 3                                  # an inconsistent pair: no exact solution
    for prior, min_overlap in ((0.01, 64), (1e-6, 1000), (0.5, 1)):
        g = projtex.solve_gains(count, sums, prior=prior, min_overlap=min_overlap)
        assert g.shape == (7, 3) and g.dtype == np.float64
        for c in range(3):
            grad, scale = _energy_gradient(count, sums, np.log(g[:, c]), c, prior, min_overlap)
            assert scale > 0 and np.abs(grad).max() <= 1e-9 * scale, (prior, c, np.abs(grad).max() / scale)
    # consistent statistics and a weak prior: the true gains up to the common factor
    count, sums = _stats(7, seed=2, gains=true)
    g = projtex.solve_gains(count, sums, prior=1e-9)
    ratio = g / true
    assert np.abs(ratio / ratio.mean(0) - 1).max() < 1e-4


def test_disconnected_groups_lonely_cameras_and_small_overlaps():
    ga, gb = np.array([[1.0, 1.1, 0.9], [1.2, 1.0, 0.8], [0.9, 1.0, 1.1]]), np.array([[1.0, 0.9, 1.2], [0.8, 1.1, 1.0]])
    ca, sa = _stats(3, seed=3, gains=ga)
    cb, sb = _stats(2, seed=4, gains=gb)
    count, sums = np.zeros((6, 6), np.int64), np.zeros((6, 6, 3), np.int64)
    count[:3, :3], sums[:3, :3] = ca, sa
    count[3:5, 3:5], sums[3:5, 3:5] = cb, sb
    count[5, 5], sums[5, 5] = 900, 900 * 30000                     # a camera that shares nothing with the others
    g = projtex.solve_gains(count, sums)
    assert np.array_equal(g[:3], projtex.solve_gains(ca, sa)) and np.array_equal(g[3:5], projtex.solve_gains(cb, sb))
    assert (g[5] == 1.0).all()
    # a pair below min_overlap is ignored: joining the groups through 63 texels of wild brightness changes nothing
    count[2, 3] = count[3, 2] = 63
    sums[2, 3], sums[3, 2] = 63 * 60000, 63 * 2000
    assert np.array_equal(projtex.solve_gains(count, sums), g)
    assert not np.array_equal(projtex.solve_gains(count, sums, min_overlap=63), g)
    # a pair with an empty sum is ignored too
    count[2, 3] = count[3, 2] = 500
    sums[2, 3], sums[3, 2] = 0, 500 * 2000
    assert np.array_equal(projtex.solve_gains(count, sums), g)
    assert (projtex.solve_gains(np.array([[5]]), np.array([[[7, 7, 7]]])) == 1.0).all()


def test_permuting_and_scaling_the_cameras():
    true = np.random.default_rng(5).uniform(0.8, 1.25, size=(6, 3))
    count, sums = _stats(6, seed=6, gains=true, density=0.8)
    g = projtex.solve_gains(count, sums)
    perm = np.array([3, 0, 5, 1, 4, 2])
    gp = projtex.solve_gains(count[perm][:, perm], sums[perm][:, perm])
    assert np.abs(gp / g[perm] - 1).max() < 1e-12
    # camera 2 twice as bright: its gain halves, up to the factor common to all cameras
    scaled = sums.copy()
    scaled[2] = sums[2] * 2
    g2 = projtex.solve_gains(count, scaled, prior=1e-9)
    ratio = g2 / projtex.solve_gains(count, sums, prior=1e-9)
    ratio[2] *= 2.0
    assert np.abs(ratio / ratio.mean(0) - 1).max() < 1e-6


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _quads(res, seed=0):
    from topo4d_amd.meshrender import triangulate
    obj, views = S.three_quads(), S.three_views()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    depth = np.stack([meshrender_ref.render(obj.vertices, tris, uv_tris, obj.uvs, np.zeros((1, 1, 3), np.uint8), v, S.H, S.W)[1] for v in views])
    photos = np.random.default_rng(seed).uniform(0, 1, size=(3, 3, S.H, S.W)).astype(np.float32)
    return S.quad_maps64(obj, *res), views, photos, depth


def test_the_restatement_without_gains_is_the_yardstick_of_the_projection():
    (pos, nrm, cov), views, photos, depth = _quads((40, 56))
    for mode in ("weighted", "best"):
        want = ref.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth.reshape(3, 1, S.H, S.W), mode=mode, depth_tol=0.02)
        for gains in (None, np.ones((3, 3))):
            got = eq.project_texture_gains(pos, nrm, cov, views, S.H, S.W, photos, depth, mode=mode, depth_tol=0.02, gains=gains)
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))
        assert want[2].max() == 3
        g = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])
        got = eq.project_texture_gains(pos, nrm, cov, views, S.H, S.W, photos, depth, mode=mode, depth_tol=0.02, gains=g)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and not np.array_equal(got[0], want[0])


def test_pair_stats_slow_equals_the_vectorised_restatement():
    (pos, nrm, cov), views, photos, depth = _quads((13, 17), seed=1)
    kw = dict(depth_tol=0.05, stat_cos_min=0.3, stat_lo=0.1, stat_hi=0.9, fade_px=4.0)
    for gains in (None, np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])):
        a = eq.pair_stats(pos, nrm, cov, views, [(S.H, S.W)] * 3, photos, depth, gains=gains, **kw)
        b = eq.pair_stats_slow(pos, nrm, cov, views, [(S.H, S.W)] * 3, photos, depth, gains=gains, **kw)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        count, sums = a
        assert np.array_equal(count, count.T) and count.diagonal().min() > 0 and count[~np.eye(3, dtype=bool)].max() > 0
        assert (count <= np.minimum.outer(count.diagonal(), count.diagonal())).all()
        assert (sums >= np.rint(0.1 * 65536) * count[..., None]).all() and (sums <= np.rint(0.9 * 65536) * count[..., None]).all()


def test_consistent_photographs_give_gains_of_one():
    """rendered photographs of one texture agree with one another, so their gains are 1 up to what the bilinear resampling of the
    render and of the projection leaves: the measured deviation is recorded above and in DESIGN.md, and held at twice its value"""
    from topo4d_amd.meshrender import triangulate
    obj, verts = S.patch_scene()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    tex = S.smooth_texture(128, 128).astype(np.float64)
    tex = (0.3 + 0.3 * (tex - tex.min()) / (tex.max() - tex.min())).astype(np.float32)
    views, h, w = S.patch_views(), 80, 96
    shots = [meshrender_ref.render(verts, tris, uv_tris, obj.uvs, tex, v, h, w) for v in views]
    photos, depth = np.stack([s[0] for s in shots]), np.stack([s[1] for s in shots])
    pos, nrm, cov = S.patch_maps64(48)
    count, sums = eq.pair_stats(pos, nrm, cov, views, [(h, w)] * 3, photos, depth, depth_tol=0.02)
    assert count[~np.eye(3, dtype=bool)].min() > 500
    g = projtex.solve_gains(count, sums)
    dev = np.abs(g - 1).max()
    print("pair counts", count.tolist(), "max |gain - 1|", dev)
    assert dev <= 2 * CONSISTENT_DEVIATION


# ---- arguments, files, parsers ---------------------------------------------------------------------------------------------------
H, W = 24, 32


def test_argument_errors_are_raised_without_a_device():
    view = torch.from_numpy(look_at_view([0, 0, -2], [0, 0, 0], H, W, f=40.0))[None]
    maps = dict(pos=torch.zeros(4, 5, 3), nrm=torch.zeros(4, 5, 3), coverage=torch.ones(4, 5, dtype=torch.uint8))
    group = lambda v: ((view.repeat(v, 1), H, W), torch.zeros(v, 3, H, W), torch.zeros(v, 1, H, W))
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.pair_stats(**maps, groups=[group(2), group(1)])
    bad = [dict(groups=[group(33)]), dict(groups=[group(20), group(13)]), dict(groups=[]), dict(stat_lo=0.9, stat_hi=0.1),
           dict(stat_cos_min=1.5), dict(stat_hi=float("nan")), dict(stat_hi=1e6), dict(gains=np.ones((3, 3))), dict(gains=np.ones(6)),
           dict(gains=np.full((2, 3), np.nan)), dict(power=9), dict(cos_min=-2.0),
           dict(out=(torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 2, 3, dtype=torch.int32))),
           dict(out=(torch.zeros(3, 3, dtype=torch.int64), torch.zeros(3, 3, 3, dtype=torch.int64))),
           dict(groups=[((view, H, W), torch.zeros(1, 3, H, W), torch.zeros(1, 1, H, W + 1))]), dict(nrm=torch.zeros(4, 6, 3))]
    for change in bad:
        with pytest.raises(ValueError):
            projtex.pair_stats(**{**maps, "groups": [group(2)], **change})
    good = dict(**maps, cams=(view, H, W), photos=torch.zeros(1, 3, H, W), depth=torch.zeros(1, 1, H, W))
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.project(**good, gains=np.ones((1, 3)))
    for g in (np.ones((2, 3)), np.ones(3), np.array([[1.0, np.inf, 1.0]]), [["a", "b", "c"]]):
        with pytest.raises(ValueError):
            projtex.project(**good, gains=g)
    count, sums = _stats(3, seed=0)
    for kw in (dict(prior=-0.1), dict(prior=float("nan")), dict(min_overlap=0), dict(min_overlap=2.5)):
        with pytest.raises(ValueError):
            projtex.solve_gains(count, sums, **kw)
    with pytest.raises(ValueError):
        projtex.solve_gains(count, sums[:, :, :2])
    with pytest.raises(ValueError):
        projtex.solve_gains(count[:2], sums)


def test_the_entry_points_reject_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    one, none = C.c_void_p(64), None
    ok = [one, one, one, 64, 64, one, 3, one, one, one, 2, 0.1, 16.0, 0.002, 0.5, 0.02, 0.98, none, one, one, none]

    def rejected(**at):
        args = list(ok)
        for k, v in at.items():
            args[int(k[1:])] = v
        assert lib.t4d_projtex_pair_stats(*args) == _lib.T4D_ERR_ARG
        assert b"t4d_projtex_pair_stats" in lib.t4d_last_error()

    for k in (0, 1, 2, 5, 7, 8, 9, 18, 19):
        rejected(**{f"a{k}": none})
    for change in (dict(a3=0), dict(a4=65537), dict(a6=0), dict(a6=33), dict(a10=9), dict(a11=2.0), dict(a12=-1.0), dict(a13=-0.5),
                   dict(a14=1.5), dict(a14=float("nan")), dict(a15=0.99), dict(a16=float("nan")), dict(a15=-2000.0), dict(a16=2000.0)):
        rejected(**change)
    gains = [one, one, one, 64, 64, one, 3, 40, 48, one, one, none, 2, 0.1, 16.0, 0.002, 0, one, one, one, none]
    for k, v in ((0, none), (9, none), (6, 256), (12, 9), (16, 2), (7, 0)):
        args = list(gains)
        args[k] = v
        assert lib.t4d_project_texture_gains(*args) == _lib.T4D_ERR_ARG


def test_proj_gains_json_round_trip(tmp_path):
    names = ["A01", "B02", "C03"]
    g = np.random.default_rng(0).uniform(0.8, 1.25, size=(3, 3))
    path = str(tmp_path / projtex.GAINS_NAME)
    report = dict(pairs=[3, 3, 2], rms_before=[0.1, 0.2, 0.3], rms_after=[0.01, 0.02, 0.03])
    projtex.write_gains(path, names, g, report, dict(prior=0.01, stat_lo=0.02))
    doc = json.load(open(path))
    assert doc["cameras"] == names and doc["report"] == report and doc["options"] == dict(prior=0.01, stat_lo=0.02)
    held, back = projtex.read_gains(path)
    assert held == names and np.array_equal(back, g)                         # repr of a double survives json
    assert np.array_equal(projtex.read_gains(path, ["C03", "A01"]), g[[2, 0]])
    assert projtex.load_gains(path) == {n: list(r) for n, r in zip(names, g)}
    with pytest.raises(ValueError, match="D04"):
        projtex.read_gains(path, ["A01", "D04"])
    with pytest.raises(ValueError):
        projtex.write_gains(path, ["A", "A"], g[:2])
    with pytest.raises(ValueError):
        projtex.write_gains(path, names, g[:2])
    open(path, "w").write('{"cameras": ["A"], "gains": [[1, 2]]}')
    with pytest.raises(ValueError):
        projtex.read_gains(path)


def test_command_lines():
    from topo4d_amd import train
    a = projtex.build_parser().parse_args(["-e", "x"])
    assert (a.equalize, a.equalize_frames, a.gains) == (False, None, None)
    assert projtex.eq_options_of(a) == (projtex.STAT_DEFAULTS, projtex.SOLVE_DEFAULTS)
    assert projtex.STAT_DEFAULTS == dict(stat_cos_min=0.5, stat_lo=0.02, stat_hi=0.98) and projtex.SOLVE_DEFAULTS == dict(prior=0.01, min_overlap=64)
    assert projtex.options_of(a) == projtex.DEFAULTS == dict(power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002, mode="weighted")
    a = projtex.build_parser().parse_args(["--equalize", "--equalize_frames", "1-3", "--stat_cos_min", "0.7", "--stat_lo", "0.05",
                                           "--stat_hi", "0.9", "--eq_prior", "0.1", "--eq_min_overlap", "10"])
    assert a.equalize is True and a.equalize_frames == [1, 2, 3]
    assert projtex.eq_options_of(a) == (dict(stat_cos_min=0.7, stat_lo=0.05, stat_hi=0.9), dict(prior=0.1, min_overlap=10))
    assert projtex.options_of(a) == projtex.DEFAULTS
    assert projtex.build_parser().parse_args(["--gains", "g.json"]).gains == "g.json"
    for argv in (["--stat_lo", "0.9", "--stat_hi", "0.1"], ["--eq_prior", "-1"], ["--eq_min_overlap", "0"]):
        with pytest.raises(SystemExit):
            projtex.eq_options_of(projtex.build_parser().parse_args(argv))
    plain = train.build_parser().parse_args([])
    for name in ("tex_equalize", "stat_cos_min", "stat_lo", "stat_hi", "eq_prior", "eq_min_overlap"):
        assert not hasattr(plain, name)                                      # absent unless given, like the other added flags
    assert projtex.options_of(plain) == projtex.DEFAULTS
    assert projtex.eq_options_of(plain) == (projtex.STAT_DEFAULTS, projtex.SOLVE_DEFAULTS)
    t = train.build_parser().parse_args(["--tex_project", "--tex_equalize", "--stat_hi", "0.95", "--eq_min_overlap", "32"])
    assert t.tex_project is True and t.tex_equalize is True
    assert projtex.eq_options_of(t) == ({**projtex.STAT_DEFAULTS, "stat_hi": 0.95}, dict(prior=0.01, min_overlap=32))
