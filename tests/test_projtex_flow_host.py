"""CPU: the registration of the projected texture (projtex.view_flows, project / project_bands(flows=), project_frame(register=)):
the argument checks of the wrappers and of the two C entry points, the command-line parsers, the float64 restatement
tests/projtex_flow_ref.py against the restatements without flows and against a photograph moved by hand, and what registration
buys on misregistered views.  No GPU.

What registration buys (test_registration_keeps_the_detail_of_best_and_the_seams_of_weighted), through the numpy chain of
tests/projtex_register_scene.three_ways with block 16, stride 8, radius 4.  On the scene of tests/test_projtex_bands_host.py as it
stands (192 x 160 views, about 1.3 px off, AS_ISSUED below) registered "weighted" keeps 0.473 of the detail energy against 0.353
unregistered, but only 0.825 of what "best" keeps (0.574), short of the 0.9 asked for; three rounds give 0.854, and no admissible
option set (block 8..16, radius 2..4, reach 1..2, rounds 1..3) gives more than 0.856.  The limit is the sampling, not the matcher
alone: at this size a texel spans 0.85 px, and "weighted" from photographs taken with the very cameras they are projected with,
no misregistration at all, keeps 0.523 = 0.912 of "best", so the bilinear mix of three samplings costs nearly the whole margin and
the sub-pixel error of a census match (about a quarter of a pixel) takes the rest.  A stronger detail amplitude changes nothing
(0.3 instead of 0.12: 0.830).  So, as the issue provides for, the scene is strengthened in resolution, the conditions stay: the
same cameras at twice the sampling (384 x 320 views, focal lengths 420 / 400 / 400, about 2.6 px off; a texel spans 1.7 px), and
rounds = 3.  There the perfectly registered blend keeps 0.971 of "best" and the registered one 0.9047 (one round: 0.797, two:
0.866).  The figures of the chain, as measured, are the constants below; the asserted conditions are the four of
projtex_register_scene.check.  The pos / nrm maps are rounded to float32, what a device takes, so tests/test_gpu_projtex_flow.py
holds the device to the same constants."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import projtex_bands_ref as bands, projtex_consist_ref as cons, projtex_flow_ref as flow, projtex_ref as ref
from tests import meshrender_ref, projtex_register_scene as R, projtex_scenes as S
from tests.test_meshrender_host import look_at_view

# the figures of projtex_register_scene.measure, as measured: the strengthened scene (scale 2) with rounds = 3, and the scene as
# the issue states it (scale 1) with one round, which misses kept["registered"] >= 0.9 kept["best"] and is recorded, not asserted
REGISTER = dict(R.REGISTER, rounds=3)
MEASURED = dict(texels=7582, kept=dict(weighted=0.420521, best=0.741945, registered=0.671218),
                step=dict(weighted=0.012377, best=0.123505, registered=0.015462), kept_blocks=[960, 765, 768], kept_blocks_exposed=[5, 0, 0])
AS_ISSUED = dict(texels=3853, kept=dict(weighted=0.352836, best=0.573521, registered=0.473187),
                 step=dict(weighted=0.012373, best=0.123220, registered=0.012373), kept_blocks=[224, 204, 194], kept_blocks_exposed=[0, 0, 0])


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_figures(fig: dict, rec: dict) -> None:
    assert fig["texels"] == rec["texels"] and fig["kept_blocks"] == rec["kept_blocks"] and fig["kept_blocks_exposed"] == rec["kept_blocks_exposed"]
    for what in ("kept", "step"):
        for k, v in rec[what].items():
            assert abs(fig[what][k] - v) <= 1e-6, (what, k, fig[what][k], v)


# ---- arguments -------------------------------------------------------------------------------------------------------------------
H, W = 24, 32


def test_flows_are_checked_without_a_device():
    from topo4d_amd import projtex
    view = torch.from_numpy(look_at_view([0, 0, -2], [0, 0, 0], H, W, f=40.0))[None]
    good = dict(pos=torch.zeros(4, 5, 3), nrm=torch.zeros(4, 5, 3), coverage=torch.ones(4, 5, dtype=torch.uint8), cams=(view.repeat(3, 1), H, W),
                photos=torch.zeros(3, 3, H, W), depth=torch.zeros(3, 1, H, W))
    flows = torch.zeros(3, H, W, 2, dtype=torch.int16)
    wrong = [flows.to(torch.int32), flows.float(), flows[:2], flows[..., :1], torch.zeros(3, W, H, 2, dtype=torch.int16), flows[0], flows.numpy(),
             torch.zeros(3, 2, H, W, dtype=torch.int16), 0]
    for call, more in ((projtex.project, {}), (projtex.project_bands, dict(low=torch.zeros(3, 3, H, W)))):
        for f in wrong:
            with pytest.raises(ValueError, match="flows"):
                call(**good, **more, flows=f)
        for fine in (dict(flows=flows), dict(flows=None), dict(flows=flows, skip=torch.zeros(4, 5, dtype=torch.int32), skip_base=2, gains=np.ones((3, 3)))):
            with pytest.raises(RuntimeError, match="no CPU path"):
                call(**good, **more, **fine)
        with pytest.raises(ValueError, match="device"):
            call(**good, **more, flows=flows.to("meta"))


def test_view_flows_and_register_are_checked_without_a_device():
    from topo4d_amd import projtex
    a = dict(renders=torch.zeros(2, 3, H, W), photos=torch.zeros(2, 3, H, W), depth=torch.zeros(2, 1, H, W))
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.view_flows(**a)
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.view_flows(**a, block=16, stride=8, radius=2, ratio=1.0, reach=4)
    bad_options = [dict(block=6), dict(block=66), dict(block=15), dict(block=16.5), dict(block=True), dict(block="16"), dict(stride=0),
                   dict(block=16, stride=17), dict(stride=1.5), dict(radius=-1), dict(radius=17), dict(radius=2.5), dict(radius=float("nan")),
                   dict(ratio=0.0), dict(ratio=1.5), dict(ratio=float("nan")), dict(ratio="0.8"), dict(ratio=True), dict(reach=0), dict(reach=5),
                   dict(reach=1.5)]
    for o in bad_options:
        with pytest.raises(ValueError):
            projtex.view_flows(**a, **o)
        with pytest.raises(ValueError):
            projtex.check_reg_options(**o)
        with pytest.raises(ValueError):
            projtex.check_register_options(o)
    bad_tensors = [dict(renders=a["renders"].double()), dict(renders=a["renders"][0]), dict(renders=torch.zeros(2, 1, H, W)), dict(renders=None),
                   dict(photos=torch.zeros(3, 3, H, W)), dict(photos=torch.zeros(2, 3, H, W + 1)), dict(photos=a["photos"].numpy()),
                   dict(depth=torch.zeros(2, H, W)), dict(depth=a["depth"].double()), dict(depth=a["depth"].to("meta"))]
    for change in bad_tensors:
        with pytest.raises(ValueError):
            projtex.view_flows(**{**a, **change})
    assert projtex.check_reg_options() == dict(block=32, stride=16, radius=4, ratio=0.8, reach=1)
    assert projtex.check_register_options(None) is None
    assert projtex.check_register_options({}) == dict(block=32, stride=16, radius=4, ratio=0.8, reach=1, rounds=1)
    assert projtex.check_register_options(dict(block=16, rounds=3, reach=np.int64(2))) == dict(block=16, stride=8, radius=4, ratio=0.8, reach=2, rounds=3)
    for register in (dict(rounds=0), dict(rounds=4), dict(rounds=1.5), dict(rounds=True), dict(level=0), dict(band_radius=3), [16, 8, 4], 3, "yes"):
        with pytest.raises(ValueError):
            projtex.check_register_options(register)
    # project_frame's and write_frame's register: before anything touches a device
    obj, _ = S.patch_scene()
    entry = {"cam": None, "im": None, "cam_name": "a"}
    for register in (dict(block=15), dict(rounds=4), dict(tol=0.1), [16, 8, 4], 0.1):
        with pytest.raises(ValueError):
            projtex.project_frame(obj, torch.zeros(49, 3), [entry] * 3, 48, register=register)
        with pytest.raises(ValueError):
            projtex.write_frame("nowhere", obj, None, [entry], 48, dict(projtex.DEFAULTS), register=register)
    with pytest.raises(ValueError, match="save_flows"):
        projtex.write_frame("nowhere", obj, None, [entry], 48, dict(projtex.DEFAULTS), save_flows=True)


def test_the_entry_points_reject_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    one, odd, none = C.c_void_p(64), C.c_void_p(66), None
    ok = [one, one, one, 64, 64, one, 3, 40, 48, one, one, none, 2, 0.1, 16.0, 0.002, 0, one, one, one, one, 0, none, one]
    for k, v in ((0, none), (9, none), (6, 256), (12, 9), (16, 2), (7, 0), (21, -1), (21, 30), (23, odd)):
        args = list(ok)
        args[k] = v
        assert lib.t4d_project_texture_flow(*args) == _lib.T4D_ERR_ARG, (k, v)
        assert b"t4d_project_texture" in lib.t4d_last_error()
    ok = [one, one, one, 64, 64, one, 3, 40, 48, one, one, one, none, 2, 0.1, 16.0, 0.002, one, one, one, one, one, one, 0, none, one]
    for k, v in ((0, none), (10, none), (21, none), (6, 256), (13, 9), (23, -1), (23, 30), (25, odd)):
        args = list(ok)
        args[k] = v
        assert lib.t4d_project_texture_bands_flow(*args) == _lib.T4D_ERR_ARG, (k, v)
        assert b"t4d_project_texture_bands" in lib.t4d_last_error()


def test_command_lines():
    from topo4d_amd import projtex, train
    defaults = dict(block=32, stride=None, radius=4, ratio=0.8, reach=1, rounds=1)
    assert projtex.REGISTER_DEFAULTS == defaults and projtex.REG_DEFAULTS == {k: v for k, v in defaults.items() if k != "rounds"}
    a = projtex.build_parser().parse_args(["-e", "x"])
    assert a.register is False and a.save_flows is False and (a.reg_block, a.reg_stride, a.reg_radius, a.reg_ratio, a.reg_reach, a.reg_rounds) == (32, None, 4, 0.8, 1, 1)
    assert projtex.register_options_of(a) is None
    assert projtex._check_args(a, 8192) == projtex.DEFAULTS     # without the flag nothing new reaches a frame or proj_gains.json
    a = projtex.build_parser().parse_args(["--reg_block", "16"])
    assert projtex.register_options_of(a) is None               # the options alone switch nothing on
    a = projtex.build_parser().parse_args(["--register"])
    assert projtex.register_options_of(a) == dict(block=32, stride=16, radius=4, ratio=0.8, reach=1, rounds=1)
    assert projtex._check_args(a, 8192) == projtex.DEFAULTS     # the registration options travel beside the projection's, not among them
    a = projtex.build_parser().parse_args(["--register", "--reg_block", "16", "--reg_stride", "4", "--reg_radius", "3", "--reg_ratio", "0.7",
                                           "--reg_reach", "2", "--reg_rounds", "3", "--save_flows", "--mode", "twoband", "--reject"])
    assert projtex.register_options_of(a) == dict(block=16, stride=4, radius=3, ratio=0.7, reach=2, rounds=3) and a.save_flows is True
    for argv in (["--register", "--reg_block", "15"], ["--register", "--reg_block", "66"], ["--register", "--reg_stride", "33"],
                 ["--register", "--reg_radius", "17"], ["--register", "--reg_ratio", "0"], ["--register", "--reg_reach", "5"],
                 ["--register", "--reg_rounds", "4"], ["--register", "--reg_rounds", "0"]):
        with pytest.raises(SystemExit):
            projtex.register_options_of(projtex.build_parser().parse_args(argv))
    for argv in (["--reg_block", "16.5"], ["--reg_rounds", "two"], ["--register", "yes"]):
        with pytest.raises(SystemExit):
            projtex.build_parser().parse_args(argv)
    plain = train.build_parser().parse_args([])
    assert not hasattr(plain, "tex_register") and not hasattr(plain, "reg_block")   # absent unless given, like the other added flags
    assert projtex.register_options_of(plain) is None
    t = train.build_parser().parse_args(["--tex_project", "--tex_register", "--reg_block", "16", "--reg_rounds", "2"])
    assert t.tex_register is True and projtex.register_options_of(t) == dict(block=16, stride=8, radius=4, ratio=0.8, reach=1, rounds=2)
    assert projtex._check_args(t, 8192) == projtex.DEFAULTS
    with pytest.raises(SystemExit):
        projtex.register_options_of(train.build_parser().parse_args(["--tex_project", "--tex_register", "--reg_radius", "20"]))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _quads(res, seed=0):
    from topo4d_amd.meshrender import triangulate
    obj, views = S.three_quads(), S.three_views()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    depth = np.stack([meshrender_ref.render(obj.vertices, tris, uv_tris, obj.uvs, np.zeros((1, 1, 3), np.uint8), v, S.H, S.W)[1] for v in views])
    photos = np.random.default_rng(seed).uniform(0, 1, size=(3, 3, S.H, S.W)).astype(np.float32)
    return S.quad_maps64(obj, *res), views, photos, depth


GAINS = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])


def test_zero_flows_are_no_flows():
    (pos, nrm, cov), views, photos, depth = _quads((40, 56))
    zero = np.zeros((3, S.H, S.W, 2), np.int16)
    skip = np.random.default_rng(1).integers(0, 1 << 5, size=(40, 56)).astype(np.int32)
    low = bands.low_band(photos, depth, 2)
    a = (pos, nrm, cov, views, S.H, S.W, photos, depth)
    for kw in (dict(depth_tol=0.02), dict(depth_tol=0.02, power=0, fade_px=0.0, cos_min=0.3)):
        for mode in ("weighted", "best"):
            want = ref.project_texture(*a, mode=mode, **kw)
            assert want[2].max() == 3 and (want[2] == 1).any()
            for got in (flow.project_texture(*a, mode=mode, flows=zero, **kw), flow.project_texture(*a, mode=mode, **kw)):
                assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want)), (mode, kw)
            want = cons.project_texture(*a, mode=mode, gains=GAINS, skip=skip, skip_base=1, **kw)
            got = flow.project_texture(*a, mode=mode, gains=GAINS, skip=skip, skip_base=1, flows=zero, **kw)
            assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want)), (mode, kw)
        b = (pos, nrm, cov, views, S.H, S.W, photos, low, depth)
        want = bands.project_bands(*b, **kw)
        assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(flow.project_bands(*b, flows=zero, **kw), want))
        want = cons.project_bands(*b, gains=GAINS, skip=skip, skip_base=1, **kw)
        got = flow.project_bands(*b, gains=GAINS, skip=skip, skip_base=1, flows=zero, **kw)
        assert all(np.array_equal(bits(g), bits(w)) for g, w in zip(got, want))


def test_a_whole_pixel_flow_samples_the_moved_photograph_and_changes_no_weight():
    """f = (f_y, f_x) = (-5, 8) px everywhere: the sample of the photograph at (px + 8, py - 5) is the sample at (px, py) of the
    photograph moved by (-8, +5), to rounding, wherever the moved taps stay inside; where they leave, the view is rejected"""
    (pos, nrm, cov), views, photos, depth = _quads((40, 56), seed=3)
    flows = np.zeros((3, S.H, S.W, 2), np.int16)
    flows[..., 0], flows[..., 1] = -5 * 256, 8 * 256
    moved = np.roll(photos, (5, -8), axis=(2, 3))                # moved[y, x] = photos[y - 5, x + 8]
    left = 0
    a = (pos, nrm, cov, views, S.H, S.W)
    kw = dict(depth_tol=0.02, fade_px=4.0)
    for v in range(3):
        ok, cs, w, s = flow.view_samples(*a[:3], views[v], S.H, S.W, photos[v], depth[v], flow=flows[v], **kw)
        ok0, cs0, w0, s0 = ref.view_samples(*a[:3], views[v], S.H, S.W, moved[v], depth[v], **kw)
        px, py = flow.pixels(pos, views[v], S.H, S.W)
        inside = (np.floor(px) + 8 + 1 <= S.W - 1) & (np.floor(py) - 5 >= 0)
        assert np.array_equal(ok, ok0 & inside) and ok.sum() > 100
        left += int((ok0 & ~inside).sum())
        assert np.array_equal(cs[ok], cs0[ok]) and np.array_equal(w[ok], w0[ok])              # geometry decides visibility and weight
        assert np.abs(s[ok] - s0[ok]).max() <= 1e-13             # (px + 8 rounds, so the fractions differ in their last bits)
    assert left > 50
    got = flow.project_texture(*a, photos, depth, mode="weighted", flows=flows, **kw)
    plain = ref.project_texture(*a, photos, depth, mode="weighted", **kw)
    assert (got[2] <= plain[2]).all() and (got[2] < plain[2]).any() and (got[0] != plain[0]).any()
    # the components are (f_y, f_x): swapped, the result differs
    swapped = flow.project_texture(*a, photos, depth, mode="weighted", flows=flows[..., ::-1].copy(), **kw)
    assert (swapped[0] != got[0]).any()
    # the flow is read at the pixel nearest to (px, py): a flow that is non-zero only there moves exactly that texel's sample
    ok, _, _, s = ref.view_samples(*a[:3], views[0], S.H, S.W, photos[0], depth[0], **kw)
    px, py = flow.pixels(pos, views[0], S.H, S.W)
    ty, tx = np.argwhere(ok & (px > 5) & (px < S.W - 6) & (py > 5) & (py < S.H - 6))[7]
    one = np.zeros((S.H, S.W, 2), np.int16)
    one[int(np.floor(py[ty, tx] + 0.5)), int(np.floor(px[ty, tx] + 0.5))] = (300, -200)
    ok1, _, _, s1 = flow.view_samples(*a[:3], views[0], S.H, S.W, photos[0], depth[0], flow=one, **kw)
    assert ok1[ty, tx] and (s1[ty, tx] != s[ty, tx]).any()
    x, y = px[ty, tx] - 200 / 256.0, py[ty, tx] + 300 / 256.0
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    q = photos[0].astype(np.float64)
    by_hand = (1 - (y - y0)) * ((1 - (x - x0)) * q[:, y0, x0] + (x - x0) * q[:, y0, x0 + 1]) + (y - y0) * ((1 - (x - x0)) * q[:, y0 + 1, x0] + (x - x0) * q[:, y0 + 1, x0 + 1])
    assert np.array_equal(s1[ty, tx], by_hand)


def test_the_report_of_a_hand_made_field():
    d = np.array([[[3.0, 4.0], [0.0, 0.0]], [[0.0, -1.0], [6.0, 8.0]]])
    assert flow.flow_report(d, np.zeros((2, 2), bool)) == dict(blocks=4, kept=0)
    assert flow.flow_report(d, np.array([[1, 0], [1, 1]])) == dict(blocks=4, kept=3, mean=16.0 / 3, median=5.0, p90=10.0, max=10.0)
    from topo4d_amd import projtex
    for kept in (np.zeros((2, 2), bool), np.array([[1, 0], [1, 1]]), np.ones((2, 2), bool)):
        assert projtex.flow_report(d, kept) == flow.flow_report(d, kept)


# ---- what registration buys --------------------------------------------------------------------------------------------------------
def test_registration_keeps_the_detail_of_best_and_the_seams_of_weighted():
    fig = R.measure(R.misregistered(R.SCALE), REGISTER)
    print("strengthened scene", json.dumps(fig))
    print("registered / best", fig["kept"]["registered"] / fig["kept"]["best"], "registered / weighted", fig["kept"]["registered"] / fig["kept"]["weighted"],
          "step / weighted", fig["step"]["registered"] / fig["step"]["weighted"])
    R.check(fig)
    same_figures(fig, MEASURED)


def test_the_scene_as_issued_is_recorded():
    """the 192 x 160 scene with one round: registration helps, but the sampling leaves too little room for 0.9 of "best" (the module
    docstring has the figures); recorded so that a change of the chain shows here too"""
    fig = R.measure(R.misregistered(1), dict(R.REGISTER, rounds=1))
    print("scene as issued", json.dumps(fig), "registered / best", fig["kept"]["registered"] / fig["kept"]["best"])
    same_figures(fig, AS_ISSUED)
    assert fig["kept"]["registered"] > fig["kept"]["weighted"] and fig["step"]["registered"] <= 1.25 * fig["step"]["weighted"]
