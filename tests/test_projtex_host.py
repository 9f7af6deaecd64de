"""CPU: the float64 yardstick of topo4d_amd.projtex (tests/projtex_ref.py) on hand-worked cases, its rejections, the argument
checks of the wrapper and of the C entry point, and the command-line parsers.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import meshrender_ref, projtex_ref as ref
from tests.test_meshrender_host import look_at_view

H, W = 24, 32
F = 40.0


def _one(point, normal, views, photos, depth=None, **kw):
    """the yardstick on a 1x1 texture: (color [3], weight, count)"""
    views = np.stack(views)
    V = len(views)
    if depth is None:
        depth = np.full((V, 1, H, W), 1e3, np.float32)          # a far wall everywhere: nothing hides the point
    pos = np.asarray(point, np.float32).reshape(1, 1, 3)
    nrm = np.asarray(normal, np.float32).reshape(1, 1, 3)
    kw.setdefault("fade_px", 0.0)
    c, w, n = ref.project_texture(pos, nrm, np.ones((1, 1), np.uint8), views, H, W, photos, depth, **kw)
    return c[0, 0].astype(np.float64), float(w[0, 0]), int(n[0, 0])


def _photos(V, seed=0):
    return np.random.default_rng(seed).uniform(0, 1, size=(V, 3, H, W)).astype(np.float32)


def _pixel(point, view):
    px, py, z = meshrender_ref.project(np.asarray(point, np.float32).reshape(1, 3), view, H, W)
    return float(px[0]), float(py[0]), float(z[0])


def _mix(photo, px, py):
    x0, y0 = int(np.floor(px)), int(np.floor(py))
    fx, fy = px - x0, py - y0
    p = photo.astype(np.float64)
    return (1 - fy) * ((1 - fx) * p[:, y0, x0] + fx * p[:, y0, x0 + 1]) + fy * ((1 - fx) * p[:, y0 + 1, x0] + fx * p[:, y0 + 1, x0 + 1])


def test_a_texel_straight_in_front_of_one_camera():
    view = look_at_view([0, 0, -2], [0, 0, 0], H, W, f=F)
    photos = _photos(1)
    px, py, z = _pixel([0, 0, 0], view)
    assert abs(px - (W - 1) / 2) < 1e-5 and abs(py - (H - 1) / 2) < 1e-5 and abs(z - 2) < 1e-6
    c, w, n = _one([0, 0, 0], [0, 0, -3.0], [view], photos)        # the normal's length does not matter
    assert n == 1 and abs(w - 1.0) < 1e-7
    centre = photos[0][:, H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].astype(np.float64).mean(axis=(1, 2))
    assert np.abs(c - centre).max() < 1e-5
    assert np.abs(c - _mix(photos[0], px, py)).max() < 1e-7


@pytest.mark.parametrize("power,want", [(0, 1.0), (1, 0.5), (2, 0.25), (3, 0.125), (8, 0.5 ** 8)])
def test_a_texel_at_sixty_degrees(power, want):
    view = look_at_view([0, 0, -2], [0, 0, 0], H, W, f=F)
    n60 = [np.sin(np.pi / 3), 0.0, -np.cos(np.pi / 3)]
    _, w, n = _one([0, 0, 0], n60, [view], _photos(1), power=power)
    assert n == 1 and abs(w - want) < 1e-6


def test_the_angle_comes_from_the_view_matrix_not_from_campos():
    eye = np.array([1.0, 0.5, -2.0])
    view = look_at_view(eye, [0, 0, 0], H, W, f=F)
    assert not view[32:].any()                                     # setup_camera's campos quirk: (0, 0, 0)
    assert np.abs(ref.camera_centre(view) - eye).max() < 1e-6
    _, w, n = _one([0, 0, 0], eye, [view], _photos(1), power=2)    # the normal points at the camera: cos = 1
    assert n == 1 and abs(w - 1.0) < 1e-6
    other = view.copy()
    other[32:] = 7.0                                               # whatever the record carries there changes nothing
    a, b = _one([0, 0, 0], eye, [other], _photos(1), power=2), _one([0, 0, 0], eye, [view], _photos(1), power=2)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def _point_at(view, px_want, py_want, z=2.0):
    """a world point on the plane Z = 0 of the camera at (0, 0, -2) that projects to the given pixel"""
    p0 = np.array(_pixel([0, 0, 0], view)[:2])
    dx = np.array(_pixel([1, 0, 0], view)[:2]) - p0
    dy = np.array(_pixel([0, 1, 0], view)[:2]) - p0
    a = np.linalg.solve(np.stack([dx, dy], 1), np.array([px_want, py_want]) - p0)
    return [a[0], a[1], 0.0]


def test_the_weight_fades_towards_the_image_edge():
    view = look_at_view([0, 0, -2], [0, 0, 0], H, W, f=F)
    p = _point_at(view, 4.0, (H - 1) / 2)
    px, py, _ = _pixel(p, view)
    assert abs(px - 4.0) < 1e-4
    _, w, n = _one(p, [0, 0, -1], [view], _photos(1), power=0, fade_px=16.0)
    assert n == 1 and abs(w - 0.25) < 1e-5
    _, w, n = _one(p, [0, 0, -1], [view], _photos(1), power=0, fade_px=0.0)
    assert n == 1 and w == 1.0
    _, w, _ = _one(p, [0, 0, -1], [view], _photos(1), power=0, fade_px=2.0)
    assert w == 1.0                                                # 4 px inside a 2 px fade: full weight
    q = _point_at(view, (W - 1) / 2, H - 1 - 2.0)                  # 2 px from the bottom edge
    _, w, _ = _one(q, [0, 0, -1], [view], _photos(1), power=0, fade_px=16.0)
    assert abs(w - 0.125) < 1e-5


def test_rejections():
    view = look_at_view([0, 0, -2], [0, 0, 0], H, W, f=F)
    photos = _photos(1)
    zero = lambda r: r[2] == 0 and r[1] == 0.0 and not r[0].any()
    assert zero(_one([0, 0, -2.005], [0, 0, -1], [view], photos))            # 5 mm in front of the camera: behind the near plane
    assert zero(_one([0, 0, -3.0], [0, 0, -1], [view], photos))              # behind the camera
    assert not zero(_one([0, 0, -1.9], [0, 0, -1], [view], photos))
    assert zero(_one(_point_at(view, -0.5, 5.0), [0, 0, -1], [view], photos))          # a tap left of the image
    assert zero(_one(_point_at(view, W - 1 + 1e-3, 5.0), [0, 0, -1], [view], photos))  # x0 + 1 = W
    assert zero(_one(_point_at(view, 5.0, H - 0.5), [0, 0, -1], [view], photos))
    assert not zero(_one(_point_at(view, W - 1 - 1e-3, 5.0), [0, 0, -1], [view], photos))
    px, py, z = _pixel([0, 0, 0], view)
    x0, y0 = int(px), int(py)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        depth = np.full((1, 1, H, W), 2.0, np.float32)
        assert not zero(_one([0, 0, 0], [0, 0, -1], [view], photos, depth))
        depth[0, 0, y0 + dy, x0 + dx] = 0.0                                   # one tap on the background
        assert zero(_one([0, 0, 0], [0, 0, -1], [view], photos, depth))
        depth[0, 0, y0 + dy, x0 + dx] = 1.9                                   # one tap on a nearer surface
        assert zero(_one([0, 0, 0], [0, 0, -1], [view], photos, depth))
        depth[0, 0, y0 + dy, x0 + dx] = 2.0 / 1.001                           # nearer, within depth_tol = 0.002
        assert not zero(_one([0, 0, 0], [0, 0, -1], [view], photos, depth))
        assert zero(_one([0, 0, 0], [0, 0, -1], [view], photos, depth, depth_tol=0.0005))
    grazing = [np.sin(np.radians(85)), 0.0, -np.cos(np.radians(85))]         # cos 85 deg = 0.087 < 0.1
    assert zero(_one([0, 0, 0], grazing, [view], photos))
    assert not zero(_one([0, 0, 0], grazing, [view], photos, cos_min=0.05))
    assert zero(_one([0, 0, 0], [0, 0, 1], [view], photos, cos_min=-1.0, power=1))   # back-facing: a weight <= 0 contributes nothing
    assert zero(_one([0, 0, 0], [0, 0, 0], [view], photos))                  # no normal
    pos = np.zeros((1, 1, 3), np.float32)
    nrm = np.array([[[0, 0, -1]]], np.float32)
    c, w, n = ref.project_texture(pos, nrm, np.zeros((1, 1), np.uint8), view[None], H, W, photos, np.full((1, 1, H, W), 9.0, np.float32))
    assert not c.any() and not w.any() and not n.any()                       # uncovered


def test_modes_and_ties():
    view = look_at_view([0, 0, -2], [0, 0, 0], H, W, f=F)
    side = look_at_view([1.5, 0, -2], [0, 0, 0], H, W, f=F)
    photos = _photos(3, seed=1)
    c0, w0, _ = _one([0, 0, 0], [0, 0, -1], [view], photos[:1])
    c1, w1, _ = _one([0, 0, 0], [0, 0, -1], [view], photos[1:2])
    c2, w2, _ = _one([0, 0, 0], [0, 0, -1], [side], photos[2:3])
    assert w0 == w1 == 1.0 and 0.5 < w2 < 0.7
    c, w, n = _one([0, 0, 0], [0, 0, -1], [view, view, side], photos, mode="best")
    assert n == 3 and w == 1.0 and np.array_equal(c, c0)                     # the tie goes to the lowest view
    c, w, n = _one([0, 0, 0], [0, 0, -1], [side, view, view], photos[[2, 1, 0]], mode="best")
    assert n == 3 and w == 1.0 and np.array_equal(c, c1)
    c, w, n = _one([0, 0, 0], [0, 0, -1], [view, view, side], photos, mode="weighted")
    assert n == 3 and abs(w - (2.0 + w2)) < 1e-6
    assert np.abs(c - (c0 + c1 + w2 * c2) / (2.0 + w2)).max() < 1e-6


def test_brute_force_visibility():
    view = look_at_view([0, 0, -2], [0, 0, 0], H, W, f=F)
    verts = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0],
                      [-0.2, -0.2, -0.5], [0.2, -0.2, -0.5], [0.2, 0.2, -0.5], [-0.2, 0.2, -0.5]], np.float64)
    tris = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    pts = np.array([[0, 0, 0], [0.1, 0.1, 0], [0.5, 0.5, 0], [0, 0, -0.5], [0.28, 0, 0]])
    # the front quad's shadow on the plane Z = 0 is the square |x|, |y| < 0.2 * 2 / 1.5
    assert ref.visible_brute_force(pts, view, verts, tris).tolist() == [False, False, True, True, True]


def test_the_wrapper_refuses_bad_arguments_without_a_device():
    from topo4d_amd import projtex
    view = torch.from_numpy(look_at_view([0, 0, -2], [0, 0, 0], H, W, f=F))[None]
    good = dict(pos=torch.zeros(4, 5, 3), nrm=torch.zeros(4, 5, 3), coverage=torch.ones(4, 5, dtype=torch.uint8), cams=(view, H, W),
                photos=torch.zeros(1, 3, H, W), depth=torch.zeros(1, 1, H, W))
    with pytest.raises(RuntimeError, match="no CPU path"):
        projtex.project(**good)
    bad = [dict(pos=torch.zeros(4, 5, 3, dtype=torch.float64)), dict(pos=torch.zeros(4, 5)), dict(nrm=torch.zeros(4, 6, 3)),
           dict(coverage=torch.ones(4, 5)), dict(coverage=torch.ones(5, 4, dtype=torch.uint8)), dict(photos=torch.zeros(2, 3, H, W)),
           dict(photos=torch.zeros(1, 3, H, W, dtype=torch.float64)), dict(depth=torch.zeros(1, H, W)), dict(depth=torch.zeros(1, 1, H, W + 1)),
           dict(cams=(view[:, :39], H, W)), dict(power=9), dict(power=-1), dict(power=1.5), dict(mode="median"), dict(cos_min=1.5),
           dict(fade_px=-1.0), dict(depth_tol=-0.1), dict(depth_tol=float("nan"))]
    for change in bad:
        with pytest.raises(ValueError):
            projtex.project(**{**good, **change})
    for p in range(9):
        projtex.check_options(power=p)
    assert projtex.uv_vertex_owner(np.array([[0, 1, 2], [3, 1, 2]]), np.array([[4, 0, 1], [4, 0, 2]]), 6).tolist() == [1, 2, 2, -1, 0, -1]


def test_the_entry_point_rejects_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    one, none = C.c_void_p(64), None
    call = lambda *a: lib.t4d_project_texture(*a)
    ok = [one, one, one, 64, 64, one, 3, 40, 48, one, one, 2, 0.1, 16.0, 0.002, 0, one, one, one, none]

    def rejected(**at):
        args = list(ok)
        for k, v in at.items():
            args[int(k[1:])] = v
        assert call(*args) == _lib.T4D_ERR_ARG
        assert b"t4d_project_texture" in lib.t4d_last_error()

    for k in (0, 1, 2, 5, 9, 10, 16, 17, 18):
        rejected(**{f"a{k}": none})
    rejected(a3=0)
    rejected(a4=65537)
    rejected(a6=0)
    rejected(a6=256)
    rejected(a7=0)
    rejected(a8=-1)
    rejected(a11=9)
    rejected(a11=-1)
    rejected(a12=2.0)
    rejected(a12=float("nan"))
    rejected(a13=-1.0)
    rejected(a14=-0.5)
    rejected(a15=2)


def test_command_lines():
    from topo4d_amd import evaluate, projtex, train
    a = projtex.build_parser().parse_args(["-e", "x"])
    assert (a.power, a.cos_min, a.fade_px, a.depth_tol, a.mode) == (2, 0.1, 16.0, 0.002, "weighted")
    assert (a.tex_res, a.tex_pad, a.tex_sizes, a.save_weight, a.undistort, a.set, a.frames, a.views) == (8192, 0, [], False, False, "dense", None, None)
    a = projtex.build_parser().parse_args(["--mode", "best", "--power", "4", "--cos_min", "0.3", "--fade_px", "0", "--depth_tol", "0.01",
                                           "--tex_res", "1024", "--tex_pad", "4", "--tex_sizes", "512,256", "--save_weight", "--undistort",
                                           "--frames", "2-3", "--views", "A,B", "--set", "low"])
    assert projtex.options_of(a) == dict(power=4, cos_min=0.3, fade_px=0.0, depth_tol=0.01, mode="best")
    assert (a.tex_res, a.tex_pad, a.tex_sizes, a.save_weight, a.undistort, a.set, a.frames, a.views) == (
        1024, 4, [512, 256], True, True, "low", [2, 3], ["A", "B"])
    with pytest.raises(SystemExit):
        projtex._check_args(projtex.build_parser().parse_args(["--power", "9"]), 8192)
    with pytest.raises(SystemExit):
        projtex._check_args(projtex.build_parser().parse_args(["--tex_sizes", "1000"]), 8192)
    plain = train.build_parser().parse_args([])
    for name in ("tex_project", "mode", "power", "cos_min", "fade_px", "depth_tol"):
        assert not hasattr(plain, name)                            # absent unless given, like the other added flags
    assert projtex.options_of(plain) == projtex.DEFAULTS
    t = train.build_parser().parse_args(["--tex_project", "--mode", "best", "--power", "3"])
    assert t.tex_project is True and projtex.options_of(t) == {**projtex.DEFAULTS, "mode": "best", "power": 3}
    assert t.gen_tex is False
    e = evaluate.build_parser().parse_args([])
    assert e.texture == "face.png" == evaluate.TEXTURE_FILE
    assert evaluate.build_parser().parse_args(["--texture", "face_proj.png"]).texture == "face_proj.png"


# ---- the CPU halves of tests/test_gpu_projtex.py ---------------------------------------------------------------------------------
ROUND_TRIP_F64 = 3.14534e-4   # the float64 pipeline's maximum error of the round trip below, as measured, in both modes


@pytest.mark.parametrize("res", [(64, 64), (40, 56)])
def test_occlusion_scene_on_the_host(res):
    """the geometry of the GPU occlusion test, with the yardsticks alone: outside the excluded band the count map is the ray
    cast, the band holds at most 10 % of the covered texels, nearly every covered texel projects into the image, and more than
    100 compared texels are hidden behind the front quad"""
    from tests import projtex_scenes as S
    from topo4d_amd.meshrender import triangulate
    obj, vw = S.occlusion_scene()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    _, depth, index = meshrender_ref.render(obj.vertices, tris, uv_tris, obj.uvs, np.zeros((1, 1, 3), np.uint8), vw, S.H, S.W)
    assert ((index // 2) == 1).sum() > 150 and ((index // 2) == 0).sum() > 800 and (depth > 0).all()
    pos, nrm, cov = S.quad_maps64(obj, *res)
    _, _, count = ref.project_texture(pos, nrm, cov, vw[None], S.H, S.W, np.zeros((1, 3, S.H, S.W), np.float32), depth[None],
                                      power=0, cos_min=-1.0, fade_px=0.0)
    seen, in_image, excluded = S.occlusion_truth(pos[cov], obj, vw)
    keep = ~excluded
    hidden = in_image & ~seen & keep
    print("covered", cov.sum(), "in the image", in_image.sum(), "excluded", excluded.sum(), "share", excluded.mean(),
          "hidden and compared", hidden.sum(), "seen and compared", (in_image & seen & keep).sum())
    assert excluded.mean() <= 0.10
    assert in_image.mean() > 0.99
    assert np.array_equal(count[cov][keep] > 0, (seen & in_image)[keep])
    assert hidden.sum() > 100 and (in_image & seen & keep).sum() > 1000


def test_round_trip_figure_of_the_float64_pipeline():
    """the figure tests/test_gpu_projtex.py's round trip is held to: meshrender_ref photographs the patch, projtex_ref projects
    them back through float64 texel maps"""
    from tests import projtex_scenes as S
    from topo4d_amd.meshrender import triangulate
    obj, verts = S.patch_scene()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    tex, views = S.smooth_texture(128, 128), S.patch_views()
    h, w = 80, 96
    shots = [meshrender_ref.render(verts, tris, uv_tris, obj.uvs, tex, v, h, w) for v in views]
    photos, depth = np.stack([s[0] for s in shots]), np.stack([s[1] for s in shots])
    pos, nrm, cov = S.patch_maps64(128)
    for mode in ("weighted", "best"):
        color, _, count = ref.project_texture(pos, nrm, cov, views, h, w, photos, depth, mode=mode)
        inner = S.erode(cov, 2) & (count >= 1)
        err = np.abs(color.astype(np.float64) - tex.astype(np.float64))[inner].max()
        print(mode, "texels", inner.sum(), "max error", err)
        assert inner.sum() > 8000 and err <= ROUND_TRIP_F64
