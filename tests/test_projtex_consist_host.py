"""CPU: the photo-consistency check of topo4d_amd.projtex without a device: the option checks, the command-line parsers, the
argument checks of the wrappers and of the three C entry points, the numpy restatement tests/projtex_consist_ref.py on hand-worked
texels and its invariants, and what the check buys on a specular highlight.  No GPU.

What it buys (the tests over the `highlight` fixture): the patch of tests/projtex_scenes.py at 48 x 48 texels under five 80 x 96
views, all within 25 degrees of the patch's axis with the whole patch in every image, photographed by tests/meshrender_ref.render
from smooth_texture(128, 128) and projected with depth_tol = 0.02 (the default 0.2 % suits 4096-pixel photographs; at these sizes
it rejects oblique views outright) and CONSIST_DEFAULTS.  One set is clean; in the other a Gaussian highlight of amplitude 0.6 and
sigma 6 px sits in view 0, the frontal one and the best view of most texels.  Over the texels with at least three voters, as measured
on the float64 restatement (the constants below): the largest error of the masked "weighted" result against the clean blend is
MASKED_ERROR, that of the unmasked one UNMASKED_ERROR, and CLEAN_SPREAD is the largest difference between two clean views' samples
of one texel.  With the highlight in view 1, an oblique one, the two errors are 0.0214 and 0.1002, and "best" is the clean result
bit for bit wherever the highlight's excess is above reject_tol."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import meshrender_ref, projtex_consist_ref as cons, projtex_ref as ref, projtex_scenes as S
from tests.test_meshrender_host import look_at_view
from topo4d_amd import projtex

# the figures of the highlight tests, as measured
VOTER_SHARE = 0.91551
CLEAN_SPREAD = 0.0013885
MASKED_ERROR = 0.022104
UNMASKED_ERROR = 0.133749


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- options, parsers --------------------------------------------------------------------------------------------------------------
def test_option_checks_and_their_messages():
    assert projtex.CONSIST_DEFAULTS == dict(reject_tol=0.1, vote_cos_min=0.5, min_votes=3)
    assert projtex.check_consist_options() == projtex.CONSIST_DEFAULTS
    assert projtex.check_consist_options(0.0, -1.0, 2) == dict(reject_tol=0.0, vote_cos_min=-1.0, min_votes=2)
    assert projtex.check_consist_options(4.0, 1.0, 32) == dict(reject_tol=4.0, vote_cos_min=1.0, min_votes=32)
    assert projtex.check_consist_options(min_votes=np.int64(5))["min_votes"] == 5 and projtex.check_consist_options(min_votes=4.0)["min_votes"] == 4
    for kw, text in ((dict(reject_tol=-0.01), r"reject_tol must be in \[0, 4\]"), (dict(reject_tol=4.5), "reject_tol"),
                     (dict(reject_tol=float("nan")), "reject_tol"), (dict(reject_tol="0.1"), "reject_tol"), (dict(reject_tol=True), "reject_tol"),
                     (dict(vote_cos_min=1.5), r"vote_cos_min must be in \[-1, 1\]"), (dict(vote_cos_min=-2), "vote_cos_min"),
                     (dict(vote_cos_min=float("nan")), "vote_cos_min"),
                     (dict(min_votes=1), r"min_votes must be an integer in \[2, 32\]"), (dict(min_votes=33), "min_votes"),
                     (dict(min_votes=2.5), "min_votes"), (dict(min_votes=True), "min_votes"), (dict(min_votes="3"), "min_votes"),
                     (dict(min_votes=float("inf")), "min_votes"), (dict(min_votes=float("nan")), "min_votes")):
        with pytest.raises(ValueError, match=text):
            projtex.check_consist_options(**kw)


def test_command_lines():
    from topo4d_amd import train
    # a plain parse and _check_args give exactly what they gave before the check existed
    a = projtex.build_parser().parse_args(["-e", "x"])
    assert (a.reject, a.save_rejected) == (False, False)
    assert projtex.consist_options_of(a) == projtex.CONSIST_DEFAULTS
    assert projtex.options_of(a) == projtex.DEFAULTS == dict(power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002, mode="weighted")
    assert projtex.BAND_DEFAULTS == dict(band_radius=8) and projtex._MODES == {"weighted": 0, "best": 1}
    assert projtex._check_args(a, 8192) == projtex.DEFAULTS
    a = projtex.build_parser().parse_args(["--mode", "twoband"])
    assert projtex._check_args(a, 8192) == {**projtex.DEFAULTS, "mode": "twoband", "band_radius": 8}
    a = projtex.build_parser().parse_args(["--reject_tol", "0.3", "--min_votes", "4"])             # the parameters without the switch
    assert projtex._check_args(a, 8192) == projtex.DEFAULTS
    # with the flag the three options are merged, as the band radius is under twoband
    a = projtex.build_parser().parse_args(["--reject"])
    assert a.reject is True and projtex._check_args(a, 8192) == {**projtex.DEFAULTS, **projtex.CONSIST_DEFAULTS}
    a = projtex.build_parser().parse_args(["--reject", "--reject_tol", "0.05", "--vote_cos_min", "0.7", "--min_votes", "4", "--save_rejected",
                                           "--mode", "twoband", "--band_radius", "3"])
    assert a.save_rejected is True and projtex.consist_options_of(a) == dict(reject_tol=0.05, vote_cos_min=0.7, min_votes=4)
    assert projtex._check_args(a, 8192) == {**projtex.DEFAULTS, "mode": "twoband", "band_radius": 3, "reject_tol": 0.05, "vote_cos_min": 0.7,
                                            "min_votes": 4}
    for argv in (["--reject", "--reject_tol", "5"], ["--reject", "--vote_cos_min", "2"], ["--reject", "--min_votes", "1"],
                 ["--reject", "--min_votes", "33"]):
        with pytest.raises(SystemExit, match="projection options"):
            projtex._check_args(projtex.build_parser().parse_args(argv), 8192)
    with pytest.raises(SystemExit):
        projtex.build_parser().parse_args(["--min_votes", "2.5"])
    # train: absent unless given, like the other added flags
    plain = train.build_parser().parse_args([])
    for name in ("tex_reject", "reject_tol", "vote_cos_min", "min_votes"):
        assert not hasattr(plain, name)
    assert projtex.consist_options_of(plain) == projtex.CONSIST_DEFAULTS and projtex._check_args(plain, 8192) == projtex.DEFAULTS
    t = train.build_parser().parse_args(["--tex_project", "--tex_reject", "--reject_tol", "0.2"])
    assert t.tex_project is True and t.tex_reject is True
    assert projtex._check_args(t, 8192) == {**projtex.DEFAULTS, **projtex.CONSIST_DEFAULTS, "reject_tol": 0.2}
    t = train.build_parser().parse_args(["--tex_project", "--min_votes", "5"])
    assert projtex._check_args(t, 8192) == projtex.DEFAULTS
    # more views than the mask holds: a message, not a traceback
    projtex.check_frame_views([None] * 40, projtex.DEFAULTS)
    projtex.check_frame_views([None] * 32, {**projtex.DEFAULTS, **projtex.CONSIST_DEFAULTS})
    with pytest.raises(SystemExit, match="32"):
        projtex.check_frame_views([None] * 33, {**projtex.DEFAULTS, **projtex.CONSIST_DEFAULTS})


def test_train_with_the_flag_needs_the_projection(tmp_path):
    from topo4d_amd import train
    argv = ["-e", "exp", "-s", "seq", "-id", str(tmp_path / "in"), "-did", str(tmp_path / "dense"), "-od", str(tmp_path / "out"),
            "--tex_reject"]
    with pytest.raises(SystemExit, match="--tex_project"):
        train.train(train.build_parser().parse_args(argv))
    assert not (tmp_path / "out").exists() or not any((tmp_path / "out").rglob("*.npz"))


def test_save_rejected_needs_the_check(tmp_path):
    (tmp_path / "exp" / "seq").mkdir(parents=True)
    args = projtex.build_parser().parse_args(["-e", "exp", "-s", "seq", "-od", str(tmp_path), "--save_rejected"])
    with pytest.raises(SystemExit, match="--reject"):
        projtex.project_tree(args)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
H, W = 24, 32


def test_argument_errors_are_raised_without_a_device():
    view = torch.from_numpy(look_at_view([0, 0, -2], [0, 0, 0], H, W, f=40.0))[None]
    maps = dict(pos=torch.zeros(4, 5, 3), nrm=torch.zeros(4, 5, 3), coverage=torch.ones(4, 5, dtype=torch.uint8))
    group = lambda v: ((view.repeat(v, 1), H, W), torch.zeros(v, 3, H, W), torch.zeros(v, 1, H, W))
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.consistency(**maps, groups=[group(2), group(1)])
    bad = [dict(groups=[group(33)]), dict(groups=[group(20), group(13)]), dict(groups=[]), dict(reject_tol=-1.0), dict(reject_tol=4.5),
           dict(vote_cos_min=1.5), dict(min_votes=1), dict(min_votes=33), dict(min_votes=2.5), dict(gains=np.ones((3, 3))),
           dict(gains=np.full((2, 3), np.nan)), dict(power=9), dict(cos_min=-2.0), dict(depth_tol=float("nan")),
           dict(groups=[((view, H, W), torch.zeros(1, 3, H, W), torch.zeros(1, 1, H, W + 1))]), dict(nrm=torch.zeros(4, 6, 3))]
    for change in bad:
        with pytest.raises(ValueError):
            projtex.consistency(**{**maps, "groups": [group(2)], **change})
    with pytest.raises(ValueError, match="32"):
        projtex.consistency(**maps, groups=[group(33)])
    # skip / skip_base of the two blends: before any device check
    good = dict(**maps, cams=(view.repeat(3, 1), H, W), photos=torch.zeros(3, 3, H, W), depth=torch.zeros(3, 1, H, W))
    skip = torch.zeros(4, 5, dtype=torch.int32)
    wrong = [dict(skip=skip.to(torch.int64)), dict(skip=skip.to(torch.uint8)), dict(skip=torch.zeros(4, 6, dtype=torch.int32)),
             dict(skip=torch.zeros(4, 5, 1, dtype=torch.int32)), dict(skip=skip.numpy()), dict(skip=skip, skip_base=-1),
             dict(skip=skip, skip_base=30), dict(skip=skip, skip_base=1.0), dict(skip=skip, skip_base=True), dict(skip=skip, skip_base=None),
             dict(skip_base=2)]
    for call, more in ((projtex.project, {}), (projtex.project_bands, dict(low=torch.zeros(3, 3, H, W)))):
        for change in wrong:
            with pytest.raises(ValueError, match="skip"):
                call(**good, **more, **change)
        for fine in (dict(skip=skip), dict(skip=skip, skip_base=29), dict(skip=None, skip_base=0), dict(skip=skip, skip_base=np.int64(4))):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(**good, **more, **fine)
    # project_frame's reject: before anything touches a device
    obj, verts = S.patch_scene()
    entry = {"cam": None, "im": None}
    for reject in (dict(reject_tol=9.0), dict(min_votes=1), dict(tol=0.1), [0.1, 0.5, 3], 0.1):
        with pytest.raises(ValueError):
            projtex.project_frame(obj, torch.zeros(49, 3), [entry] * 3, 48, reject=reject)
    with pytest.raises(ValueError, match="32"):
        projtex.project_frame(obj, torch.zeros(49, 3), [entry] * 33, 48, reject={})
    with pytest.raises(ValueError, match="save_rejected"):
        projtex.write_frame("nowhere", obj, None, [entry], 48, dict(projtex.DEFAULTS), save_rejected=True)


def test_the_entry_points_reject_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    one, none = C.c_void_p(64), None
    ok = [one, one, one, 64, 64, one, 3, one, one, one, 2, 0.1, 16.0, 0.002, none, 0.1, 0.5, 3, one, one, none]
    changes = [(k, none) for k in (0, 1, 2, 5, 7, 8, 9, 18, 19)]
    changes += [(3, 0), (4, 65537), (6, 0), (6, 33), (10, 9), (11, 2.0), (12, -1.0), (13, -0.5), (15, -0.1), (15, 4.5), (15, float("nan")),
                (16, 1.5), (16, float("nan")), (17, 1), (17, 33), (17, -3)]
    for k, v in changes:
        args = list(ok)
        args[k] = v
        assert lib.t4d_projtex_consistency(*args) == _lib.T4D_ERR_ARG, (k, v)
        assert b"t4d_projtex_consistency" in lib.t4d_last_error()
    ok = [one, one, one, 64, 64, one, 3, 40, 48, one, one, none, 2, 0.1, 16.0, 0.002, 0, one, one, one, one, 0, none]
    for k, v in ((0, none), (9, none), (6, 256), (12, 9), (16, 2), (7, 0), (21, -1), (21, 30), (21, 33), (6, 33)):
        args = list(ok)
        args[k] = v
        assert lib.t4d_project_texture_skip(*args) == _lib.T4D_ERR_ARG, (k, v)
        assert b"t4d_project_texture" in lib.t4d_last_error()
    ok = [one, one, one, 64, 64, one, 3, 40, 48, one, one, one, none, 2, 0.1, 16.0, 0.002, one, one, one, one, one, one, 0, none]
    for k, v in ((0, none), (10, none), (21, none), (6, 256), (13, 9), (23, -1), (23, 30), (6, 33)):
        args = list(ok)
        args[k] = v
        assert lib.t4d_project_texture_bands_skip(*args) == _lib.T4D_ERR_ARG, (k, v)
        assert b"t4d_project_texture_bands" in lib.t4d_last_error()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_worked_texels():
    q = lambda *rows: {v: r for v, r in enumerate(rows) if r is not None}
    rule = cons.texel_rule
    # three voters in agreement, one far off: rejected, whichever view it is
    assert rule([0, 1, 2], [0, 1, 2], q((100, 100, 100), (105, 95, 100), (900, 100, 100)), 50, 3) == (0b100, 3)
    assert rule([0, 1, 2], [0, 1, 2], q((900, 100, 100), (105, 95, 100), (100, 100, 100)), 50, 3) == (0b001, 3)
    # one channel is enough, and the distance is to the median of that channel
    assert rule([0, 1, 2], [0, 1, 2], q((100, 100, 100), (100, 100, 100), (100, 100, 151)), 50, 3) == (0b100, 3)
    assert rule([0, 1, 2], [0, 1, 2], q((100, 100, 100), (100, 100, 100), (100, 100, 150)), 50, 3) == (0, 3)         # |q - m| = qt stays
    # the lower median: of four voters the second in order; ties in q go by the view index, which does not change the value
    assert rule([0, 1, 2, 3], [0, 1, 2, 3], q((10, 0, 0), (20, 0, 0), (80, 0, 0), (90, 0, 0)), 15, 3) == (0b1100, 4)     # m = 20
    assert rule([0, 1, 2, 3], [0, 1, 2, 3], q((90, 0, 0), (80, 0, 0), (20, 0, 0), (10, 0, 0)), 15, 3) == (0b0011, 4)
    assert rule([0, 1, 2], [0, 1, 2], q((7, 7, 7), (7, 7, 7), (7, 7, 7)), 0, 2) == (0, 3)
    # too few voters: nothing, though the views disagree; a view that does not vote can still be rejected
    assert rule([0, 1, 2], [0, 1], q((100, 0, 0), (100, 0, 0), (900, 0, 0)), 50, 3) == (0, 2)
    assert rule([0, 1, 2], [0, 1], q((100, 0, 0), (100, 0, 0), (900, 0, 0)), 50, 2) == (0b100, 2)
    assert rule([1, 4, 31], [1, 4], q(None, (100, 0, 0), None, None, (100, 0, 0), *[None] * 26, (900, 0, 0)), 50, 2) == (1 << 31, 2)
    # no consensus: every accepted view is an outlier (the median mixes channels of different views), so all are kept
    assert rule([0, 1, 2], [0, 1, 2], q((0, 500, 900), (500, 900, 0), (900, 0, 500)), 50, 3) == (0, 3)
    # at least one view is kept otherwise: the median's own view in a channel need not be kept, but then another is
    word, n = rule([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], q((0, 0, 0), (10, 10, 10), (20, 500, 20), (30, 30, 30), (40, 40, 900)), 25, 3)
    assert n == 5 and word == 0b10101


def _quads(res, seed=0):
    from topo4d_amd.meshrender import triangulate
    obj, views = S.three_quads(), S.three_views()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    depth = np.stack([meshrender_ref.render(obj.vertices, tris, uv_tris, obj.uvs, np.zeros((1, 1, 3), np.uint8), v, S.H, S.W)[1] for v in views])
    photos = np.random.default_rng(seed).uniform(0, 1, size=(3, 3, S.H, S.W)).astype(np.float32)
    return S.quad_maps64(obj, *res), views, photos, depth


def test_invariants_of_the_restatement():
    (pos, nrm, cov), views, photos, depth = _quads((37, 41))
    photos[1, 0, 10, 12] = np.nan
    photos[2, :, 20:24, 20:24] = 7.0                              # beyond the clamp
    sizes = [(S.H, S.W)] * 3
    seen_any = False
    for kw in (dict(min_votes=2, reject_tol=0.3), dict(min_votes=3, reject_tol=0.2, vote_cos_min=0.3), dict(min_votes=2, reject_tol=0.0),
               dict(min_votes=2, vote_cos_min=1.0)):
        skip, votes = cons.consistency(pos, nrm, cov, views, sizes, photos, depth, depth_tol=0.02, **kw)
        acc, vot, q = cons.samples(pos, nrm, cov, views, sizes, photos, depth, depth_tol=0.02, vote_cos_min=kw.get("vote_cos_min", 0.5))
        assert skip.dtype == np.uint32 and votes.dtype == np.uint8 and skip.shape == votes.shape == (37, 41)
        assert q.min() >= 0 and q.max() == 4 * 65536
        accepted = sum(acc[v].astype(np.uint32) << v for v in range(3))
        assert not (skip & ~accepted).any()                       # a bit is set only for an accepted view
        assert not (accepted[skip != 0] == skip[skip != 0]).any()  # no texel loses all of its accepted views
        assert np.array_equal(votes, vot.sum(0)) and not skip[votes < kw["min_votes"]].any()
        assert not skip[~cov].any() and not votes[~cov].any()
        count = ref.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth.reshape(3, 1, S.H, S.W), depth_tol=0.02)[2]
        masked = cons.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth.reshape(3, 1, S.H, S.W), depth_tol=0.02, skip=skip)[2]
        assert np.array_equal(masked, count - cons.popcount(skip)) and ((masked > 0) == (count > 0)).all()
        if kw.get("vote_cos_min") == 1.0:
            assert not votes.any() and not skip.any()
        else:
            seen_any |= bool(skip.any())
            assert votes.max() == 3
    assert seen_any


def test_the_masked_restatements_without_a_mask_are_the_yardsticks():
    from tests import projtex_bands_ref as bands
    (pos, nrm, cov), views, photos, depth = _quads((40, 56), seed=1)
    depth = depth.reshape(3, 1, S.H, S.W)
    low = bands.low_band(photos, depth, 2)
    g = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])
    zero = np.zeros((40, 56), np.uint32)
    for gains in (None, g):
        for skip in (None, zero):
            for mode in ("weighted", "best"):
                want = ref.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth, depth_tol=0.02, mode=mode, gains=gains)
                got = cons.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth, depth_tol=0.02, mode=mode, gains=gains, skip=skip)
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
            want = bands.project_bands(pos, nrm, cov, views, S.H, S.W, photos, low, depth, depth_tol=0.02, gains=gains)
            got = cons.project_bands(pos, nrm, cov, views, S.H, S.W, photos, low, depth, depth_tol=0.02, gains=gains, skip=skip)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
    # a mask that drops view 1 everywhere is the projection of views 0 and 2; with skip_base the same bits sit higher
    only = np.full((40, 56), 0b010, np.uint32)
    want = ref.project_texture(pos, nrm, cov, views[[0, 2]], S.H, S.W, photos[[0, 2]], depth[[0, 2]], depth_tol=0.02)
    for skip, base in ((only, 0), (only << 29, 29)):
        got = cons.project_texture(pos, nrm, cov, views, S.H, S.W, photos, depth, depth_tol=0.02, skip=skip, skip_base=base)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))


# ---- what the check buys -------------------------------------------------------------------------------------------------------------
EYES = ([0.0, 0.0, -3.0], [1.2, 0.3, -2.8], [-1.0, -0.5, -2.9], [0.4, -1.1, -2.8], [-0.5, 1.0, -2.85])
PATCH_KW = dict(depth_tol=0.02)


def highlight_views(h=80, w=96):
    return np.stack([S.view(eye, [0, 0, 0], h, w, f=78.0) for eye in EYES])


def highlight_photos(h=80, w=96, view=0):
    """(views, clean photos [5,3,h,w], photos with the highlight in `view`, depth [5,h,w]) of the patch, rendered on the host"""
    from topo4d_amd.meshrender import triangulate
    obj, verts = S.patch_scene()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    views = highlight_views(h, w)
    shots = [meshrender_ref.render(verts, tris, uv_tris, obj.uvs, S.smooth_texture(128, 128), v, h, w) for v in views]
    clean, depth = np.stack([s[0] for s in shots]).astype(np.float32), np.stack([s[1] for s in shots])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    spot = 0.6 * np.exp(-((x - 54.0) ** 2 + (y - 34.0) ** 2) / (2 * 6.0 ** 2))
    marked = clean.copy()
    marked[view] += spot.astype(np.float32)
    return views, clean, marked, depth


@pytest.fixture(scope="module")
def highlight():
    h, w = 80, 96
    views, clean, marked, depth = highlight_photos(h, w)
    obj, verts = S.patch_scene()
    for v, eye in zip(views, EYES):                                # the conditions of the scene: within 25 degrees, the whole patch in the image
        assert np.degrees(np.arccos(-np.asarray(eye)[2] / np.linalg.norm(eye))) <= 25.0
        px, py, _ = meshrender_ref.project(verts, v, h, w)
        assert px.min() >= 1 and px.max() <= w - 2 and py.min() >= 1 and py.max() <= h - 2
    pos, nrm, cov = S.patch_maps64(48)
    a = (pos, nrm, cov, views, [(h, w)] * 5)
    out = dict(views=views, h=h, w=w, clean=clean, marked=marked, depth=depth, maps=(pos, nrm, cov))
    out["clean_mask"] = cons.consistency(*a, clean, depth, **PATCH_KW)
    out["mask"] = cons.consistency(*a, marked, depth, **PATCH_KW)
    out["acc"], _, out["q_clean"] = cons.samples(*a, clean, depth, **PATCH_KW)
    _, _, out["q_marked"] = cons.samples(*a, marked, depth, **PATCH_KW)
    return out


def _blend(hl, photos, mode, skip=None):
    pos, nrm, cov = hl["maps"]
    return cons.project_texture(pos, nrm, cov, hl["views"], hl["h"], hl["w"], photos, hl["depth"][:, None], mode=mode, skip=skip, **PATCH_KW)


def test_the_scene_has_voters_and_the_clean_set_rejects_nothing(highlight):
    hl = highlight
    cov = hl["maps"][2]
    skip, votes = hl["clean_mask"]
    share = (votes[cov] >= 3).mean()
    q = np.where(hl["acc"][..., None], hl["q_clean"], -1)
    lo = np.where(hl["acc"][..., None], hl["q_clean"], 1 << 30).min(0)
    spread = ((q.max(0) - lo)[votes >= 3].max()) / 65536.0
    print("covered", int(cov.sum()), "share with >= 3 voters", share, "clean spread", spread)
    assert share >= 0.85
    assert not skip.any()
    assert abs(share - VOTER_SHARE) <= 1e-4 and abs(spread - CLEAN_SPREAD) <= 1e-5


def test_the_masked_blend_is_within_the_tolerance_and_three_times_nearer(highlight):
    """|masked - clean| <= reject_tol + spread follows from the rule: with n >= 3 voters of which one is off, the lower median (rank
    (n - 1) / 2, neither the first nor the last for n >= 3) lies among the clean values; every kept sample is within reject_tol of it,
    so their blend is, and the clean blend lies among the clean values too."""
    hl = highlight
    skip, votes = hl["mask"]
    sel = votes >= 3
    clean = _blend(hl, hl["clean"], "weighted")[0].astype(np.float64)
    plain = _blend(hl, hl["marked"], "weighted")[0].astype(np.float64)
    masked, _, count = _blend(hl, hl["marked"], "weighted", skip)
    err_masked = np.abs(masked - clean)[sel].max()
    err_plain = np.abs(plain - clean)[sel].max()
    print("texels", int(sel.sum()), "rejected somewhere", int((skip != 0).sum()), "masked error", err_masked, "unmasked error", err_plain)
    assert (skip != 0).sum() > 20 and not (skip & ~np.uint32(1)).any()          # only the highlighted view is ever rejected
    assert np.array_equal(count, _blend(hl, hl["clean"], "weighted")[2] - cons.popcount(skip))
    assert err_masked <= projtex.CONSIST_DEFAULTS["reject_tol"] + CLEAN_SPREAD
    assert err_masked <= err_plain / 3.0
    assert abs(err_masked - MASKED_ERROR) <= 1e-5 and abs(err_plain - UNMASKED_ERROR) <= 1e-5


def test_best_takes_no_highlight_where_it_exceeds_the_tolerance(highlight):
    """Where the highlighted view's excess over its own clean sample is above reject_tol it is rejected, and "best" shows a clean
    photograph: where the highlighted view was not the best one the result is the clean "best" result bit for bit; where it was,
    the next best view takes its place, whose clean sample agrees with it within the clean spread."""
    hl = highlight
    tol = projtex.CONSIST_DEFAULTS["reject_tol"]
    skip, votes = hl["mask"]
    excess = (hl["q_marked"][0] - hl["q_clean"][0]).max(-1) / 65536.0
    sel = (votes >= 3) & hl["acc"][0] & (excess > tol)
    assert sel.sum() > 20
    assert (skip[sel] & 1).all()
    clean = _blend(hl, hl["clean"], "best")
    plain = _blend(hl, hl["marked"], "best")
    masked = _blend(hl, hl["marked"], "best", skip)
    same_mask = _blend(hl, hl["clean"], "best", skip)
    assert np.array_equal(bits(masked[0][sel]), bits(same_mask[0][sel]))          # nothing of the highlight is left
    front = bits(clean[1]) == bits(ref.project_texture(*hl["maps"], hl["views"][:1], hl["h"], hl["w"], hl["clean"][:1], hl["depth"][:1, None],
                                                        mode="best", **PATCH_KW)[1])
    assert (sel & front).sum() > 10                               # the highlight sits where view 0 is the best view
    other = sel & ~front
    assert np.array_equal(bits(masked[0][other]), bits(clean[0][other]))
    assert np.abs(masked[0].astype(np.float64) - clean[0])[sel].max() <= CLEAN_SPREAD
    assert np.abs(plain[0].astype(np.float64) - clean[0])[sel & front].min() > tol


def test_best_equals_the_clean_result_when_the_highlight_sits_in_a_view_that_is_not_the_best():
    """the highlight in view 1, an oblique one: wherever its excess is above reject_tol the view is rejected, and since the frontal
    view is the best one there the masked "best" result is the clean one, bit for bit"""
    tol = projtex.CONSIST_DEFAULTS["reject_tol"]
    views, clean, marked, depth = highlight_photos(view=1)
    pos, nrm, cov = S.patch_maps64(48)
    a = (pos, nrm, cov, views, [(80, 96)] * 5)
    skip, votes = cons.consistency(*a, marked, depth, **PATCH_KW)
    acc, _, q_clean = cons.samples(*a, clean, depth, **PATCH_KW)
    _, _, q_marked = cons.samples(*a, marked, depth, **PATCH_KW)
    excess = (q_marked[1] - q_clean[1]).max(-1) / 65536.0
    sel = (votes >= 3) & acc[1] & (excess > tol)
    assert sel.sum() > 20 and (skip[sel] == 0b10).all() and not (skip & ~np.uint32(0b10)).any()
    b = (pos, nrm, cov, views, 80, 96)
    want = cons.project_texture(*b, clean, depth[:, None], mode="best", **PATCH_KW)
    got = cons.project_texture(*b, marked, depth[:, None], mode="best", skip=skip, **PATCH_KW)
    assert np.array_equal(bits(got[0][sel]), bits(want[0][sel])) and np.array_equal(bits(got[1][sel]), bits(want[1][sel]))
    # and "weighted" there is within the bound of the rule
    clean_w = cons.project_texture(*b, clean, depth[:, None], **PATCH_KW)[0].astype(np.float64)
    plain_w = cons.project_texture(*b, marked, depth[:, None], **PATCH_KW)[0].astype(np.float64)
    masked_w = cons.project_texture(*b, marked, depth[:, None], skip=skip, **PATCH_KW)[0].astype(np.float64)
    err_masked, err_plain = np.abs(masked_w - clean_w)[votes >= 3].max(), np.abs(plain_w - clean_w)[votes >= 3].max()
    print("highlight in view 1: masked error", err_masked, "unmasked error", err_plain)
    assert err_masked <= tol + CLEAN_SPREAD and err_masked <= err_plain / 3.0
