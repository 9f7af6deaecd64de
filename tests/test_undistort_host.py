"""CPU: the host half of the undistortion - cameras.load_lens / get_lenses on calibration files written here, the host C++ build
of csrc/t4d_lens.h (tests/native/lens_host.cpp) against the numpy restatement of tests/undistort_ref.py bit for bit, the model
itself against an analytically known image, T4DLensView's layout and the refusals of t4d_undistort_views."""
import ctypes as C
import os
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import ingest_ref
from tests import undistort_ref as ref
from topo4d_amd import _lib, cameras, ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. calibration ---------------------------------------------------------------------------------------------------------------
FULL = dict(f=3500.25, cx=12.5, cy=-7.25, k1=-0.08, k2=0.05, k3=-0.01, k4=0.002, p1=3e-4, p2=-2e-4, b1=1.5, b2=-0.7)
IDENT = "1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1"


def lens_xml(sensors, cams):
    """A cameras.xml with the calibration tags given per sensor: {id, width, height, type, tags {name: value}}."""
    out = ['<?xml version="1.0" encoding="UTF-8"?>', '<document version="1.4.0">', '  <chunk label="Chunk 1" enabled="true">',
           '    <sensors next_id="%d">' % len(sensors)]
    for s in sensors:
        kind = s.get("type", "frame")
        out.append('      <sensor id="%d" label="s" type="%s">' % (s["id"], kind))
        out.append('        <resolution width="%d" height="%d"/>' % (s["width"], s["height"]))
        out.append('        <calibration type="%s" class="adjusted">' % kind)
        out += ['          <%s>%r</%s>' % (k, float(v), k) for k, v in s["tags"].items()]
        out += ['        </calibration>', '      </sensor>']
    out += ['    </sensors>', '    <cameras next_id="%d" next_group_id="0">' % len(cams)]
    for i, (label, sid) in enumerate(cams):
        out += ['      <camera id="%d" sensor_id="%d" label="%s">' % (i, sid, label), '        <transform>%s</transform>' % IDENT,
                '      </camera>']
    out += ['    </cameras>', '  </chunk>', '</document>', '']
    return "\n".join(out).encode()


@pytest.fixture()
def calib(tmp_path):
    sensors = [dict(id=0, width=4096, height=3008, tags=FULL),
               dict(id=1, width=4097, height=3011, tags=dict(f=11021.0, k1=-0.0312, p2=1e-4, b1=0.25)),
               dict(id=2, width=640, height=480, tags=dict(f=500.0)),
               dict(id=3, width=640, height=480, type="fisheye", tags=dict(f=300.0, k1=0.01))]
    path = tmp_path / "cameras.xml"
    path.write_bytes(lens_xml(sensors, [("all", 0), ("some", 1), ("none", 2), ("fish", 3)]))
    return str(path)


def test_load_lens_reads_every_coefficient(calib):
    lens = cameras.load_lens(calib, "all")
    assert (lens.width, lens.height) == (4096, 3008)
    assert lens.f == FULL["f"] and lens.cxa == 4096 / 2.0 + FULL["cx"] and lens.cya == 3008 / 2.0 + FULL["cy"]
    for k in cameras.LENS_COEFFICIENTS:
        assert getattr(lens, k) == FULL[k], k
    assert lens.numbers() == (lens.f, lens.cxa, lens.cya) + tuple(FULL[k] for k in ("k1", "k2", "k3", "k4", "p1", "p2", "b1", "b2"))
    assert not lens.is_pinhole


def test_load_lens_missing_tags_are_zero(calib):
    some = cameras.load_lens(calib, "some")
    assert (some.k1, some.p2, some.b1) == (-0.0312, 1e-4, 0.25)
    assert (some.k2, some.k3, some.k4, some.p1, some.b2) == (0.0,) * 5
    assert (some.cxa, some.cya) == (4097 / 2.0, 3011 / 2.0)          # no cx / cy: the image centre
    none = cameras.load_lens(calib, "none")
    assert none.is_pinhole and none.numbers()[3:] == (0.0,) * 8


@pytest.mark.parametrize("name", ["all", "some"])
def test_load_lens_scales_with_the_image(calib, name):
    one, low = cameras.load_lens(calib, name, 1), cameras.load_lens(calib, name, 8)
    for k in ("f", "cxa", "cya", "b1", "b2"):
        assert getattr(low, k) == getattr(one, k) / 8, k
    for k in ("k1", "k2", "k3", "k4", "p1", "p2"):
        assert getattr(low, k) == getattr(one, k), k
    assert (low.width, low.height) == (one.width // 8, one.height // 8)      # 4097 x 3011 floors to 512 x 376
    cam, _ = cameras.load_camera(calib, name, resize_factor=8, rt=0)
    assert tuple(cam["image_size"]) == (low.height, low.width)
    assert cam["intrinsics"][0, 0] == low.f and cam["intrinsics"][0, 2] == low.cxa and cam["intrinsics"][1, 2] == low.cya
    assert one.scaled(8) == low and one.scaled(1) is one


def test_load_lens_errors(calib):
    with pytest.raises(ValueError, match="'nobody'"):
        cameras.load_lens(calib, "nobody")
    with pytest.raises(ValueError, match="fisheye"):
        cameras.load_lens(calib, "fish")
    cam, _ = cameras.load_camera(calib, "fish")                      # load_camera itself never looked at the type
    assert cam["intrinsics"][0, 0] == 300.0


def test_get_lenses_is_keyed_like_get_cameras(tmp_path):
    seq = tmp_path / "seq"
    (seq / "000001").mkdir(parents=True)
    for n in ("b.jpg", "a.jpg", "c.png"):
        (seq / "000001" / n).write_bytes(b"")
    (seq / "cameras.xml").write_bytes(lens_xml([dict(id=0, width=4096, height=3008, tags=FULL)], [("a", 0), ("b", 0), ("c", 0)]))
    low, full = cameras.get_lenses(str(tmp_path), "seq", 8)
    cams, cams_full, _ = cameras.get_cameras(str(tmp_path), "seq", 8, rotate_mask={"a": 1, "b": -1, "c": 0})
    assert list(low) == list(full) == list(cams) == ["a.jpg", "b.jpg", "c.png"]
    assert full["a.jpg"] == cameras.load_lens(str(seq / "cameras.xml"), "a") and low["c.png"] == full["c.png"].scaled(8)
    other = tmp_path / "views" / "seq" / "000001"
    other.mkdir(parents=True)
    (other / "b.jpg").write_bytes(b"")
    assert list(cameras.get_lenses(str(tmp_path), "seq", 8, views_dir=str(tmp_path / "views"))[0]) == ["b.jpg"]
    of, of_full, _ = cameras.get_cameras(str(tmp_path), "seq", 8, rotate_mask={"b": -1}, views_dir=str(tmp_path / "views"))
    assert list(of) == ["b.jpg"]
    for got, want in ((of["b.jpg"], cams["b.jpg"]), (of_full["b.jpg"], cams_full["b.jpg"])):
        assert all(np.array_equal(got[k], v) for k, v in want.items())


# ---- 2. the host build of csrc/t4d_lens.h against the restatement -------------------------------------------------------------------
def image(rows, cols, channels, seed):
    """A random uint8 image that holds 0 and 255 in every channel where it has two pixels."""
    img = np.random.default_rng(seed).integers(0, 256, (rows, cols, channels), dtype=np.uint8)
    img[0, 0], img[-1, -1] = 0, 255
    return img


def blend(lens, weight):
    """The lens with its eight coefficients scaled by `weight` (0: a pinhole)."""
    return {k: v * (weight if k in cameras.LENS_COEFFICIENTS else 1.0) for k, v in lens.items()}


def cases():
    """[dict(img, crop, angle, lens, s, nearest)]: sizes from 1x1 to 375x512, angles 0, +-90, 180, channels 1 and 3, crops,
    supersample 1, 2 and 8, nearest, lenses from a pinhole to the wide one."""
    out = []
    k = 0
    for (rows, cols) in [(1, 1), (7, 9), (17, 33), (61, 93), (375, 512)]:
        for angle in (0, 90, -90, 180):
            for s in (1, 2, 8):
                if min(rows, cols) < s:
                    continue
                channels = (1, 3)[k % 2]
                weight = (0.0, 0.25, 1.0)[k % 3]
                crop = (rows, cols) if k % 4 == 1 else None
                pad = (5, 3) if crop else (0, 0)
                out.append(dict(img=image(rows + pad[0], cols + pad[1], channels, k), crop=crop, angle=angle, s=s,
                                lens=blend(ref.wide_lens(cols, rows), weight), nearest=k % 5 == 2))
                k += 1
    return out


def geometry(case):
    """(rows, cols, matrix, out_shape) of a case: the sensor is the cropped image, U is its turned shape."""
    rows, cols = case["crop"] or case["img"].shape[:2]
    m, shape = ingest.rotate_matrix(rows, cols, float(case["angle"]))
    return rows, cols, m, (shape[0] // case["s"], shape[1] // case["s"])


def expected(case):
    rows, cols, m, shape = geometry(case)
    return ref.undistort_target(case["img"][:rows, :cols], m, shape, case["lens"], case["s"], case["nearest"])


def describe(case):
    return dict(shape=case["img"].shape, crop=case["crop"], angle=case["angle"], s=case["s"], nearest=case["nearest"],
                k1=case["lens"]["k1"])


@pytest.fixture(scope="module")
def lens_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs a host C++ compiler")
    exe = tmp_path_factory.mktemp("native") / "lens_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "lens_host.cpp")])
    return str(exe)


def host_undistort(exe, img, matrix, out_shape, lens, s=1, nearest=False, crop=None, cval=0.0):
    img = img if img.ndim == 3 else img[..., None]
    rows, cols = crop or img.shape[:2]
    v = _lib.T4DLensView()
    v.rows, v.cols, v.channels, v.src_pitch = rows, cols, img.shape[2], img.shape[1] * img.shape[2]
    v.out_rows, v.out_cols, v.supersample, v.nearest = out_shape[0], out_shape[1], s, int(nearest)
    for k in range(6):
        v.matrix[k] = float(np.asarray(matrix)[k // 3, k % 3])
    for k, x in enumerate(ref.lens_numbers(lens)):
        v.lens[k] = float(x)
    v.cval = cval
    r = subprocess.run([exe], input=bytes(v) + struct.pack("<i", img.shape[0]) + np.ascontiguousarray(img).tobytes(),
                       capture_output=True)
    assert r.returncode == 0, r.returncode
    return torch.from_numpy(np.frombuffer(r.stdout, np.float32).reshape(img.shape[2], *out_shape).copy())


def test_host_build_matches_restatement(lens_host):
    bad = []
    for case in cases():
        rows, cols, m, shape = geometry(case)
        got = host_undistort(lens_host, case["img"], m, shape, case["lens"], case["s"], case["nearest"], case["crop"])
        if not torch.equal(got, expected(case)):
            bad.append(describe(case))
    assert not bad, bad[:5]


def test_pinhole_lens_returns_the_coordinates_exactly():
    r, c = np.meshgrid(np.arange(-3.0, 3011.0, 7.0), np.arange(-3.0, 4099.0, 7.0), indexing="ij")
    rs, cs = ref.source_coords(blend(ref.wide_lens(4096, 3008), 0.0), r, c)
    assert np.array_equal(rs, r) and np.array_equal(cs, c)


@pytest.mark.parametrize("angle", [0, 90, -90, 180])
@pytest.mark.parametrize("size", [(7, 9), (61, 93), (375, 512)])
@pytest.mark.parametrize("channels", [1, 3])
def test_pinhole_lens_is_the_restated_rotate(lens_host, angle, size, channels):
    """Supersample 1 and no distortion: skimage's rotate, bit for bit.  The model has no clip step, so this is stated for images
    that hold 0 and 255 (skimage then clips to [0, 1], which no convex combination with cval 0 leaves); a 1x1 image cannot."""
    img = image(size[0], size[1], channels, abs(angle) + channels + (angle < 0))
    m, shape = ingest.rotate_matrix(size[0], size[1], float(angle))
    lens = blend(ref.wide_lens(size[1], size[0]), 0.0)
    want = ingest_ref.rotate_target(img, angle)
    assert torch.equal(ref.undistort_target(img, m, shape, lens), want)
    assert torch.equal(host_undistort(lens_host, img, m, shape, lens), want)


# ---- 3. the model against Metashape's formulas written a second time ------------------------------------------------------------------
# (undistorted point from the image's corner, lens tags) -> its displacement in the photograph, in pixels: worked by hand from
# the manual's absolute form u = w/2 + cx + x'f + x'B1 + y'B2, v = h/2 + cy + y'f for a 4096 x 3008 sensor and checked in exact
# rational arithmetic.  E.g. the golden rig's top-left corner: x = -2048/11021, y = -1504/11021, r^2 = 0.0531573,
# K1 r^2 + K2 r^4 = -0.00129961, so the photograph shows the corner 2.66 px to the right and 1.95 px down: a barrel lens
# (K1 < 0) pulls it towards the centre.  Tangential terms at the top-right corner of the f = 3,500 lens: x = 0.585143,
# y = -0.429714, r^2 = 0.527046, P1 (r^2 + 2x^2) + 2 P2 x y = 4.6413e-4 -> +1.6244 px; P2 (r^2 + 2y^2) + 2 P1 x y =
# -3.3014e-4 -> -1.1555 px.  Affinity and skew at the bottom-right corner: x B1 + y B2 = 0.877714 - 0.300800 = +0.576914 px.
DISPLACEMENTS = [
    ("golden rig, top-left corner", dict(f=11021.0, k1=-0.0312, k2=0.127), (0.0, 0.0), (2.66158284786732, 1.9545999039025632)),
    ("f 3,500 with k1 alone, top-left corner", dict(f=3500.0, k1=-0.08), (0.0, 0.0), (86.3513035755102, 63.41423856326531)),
    ("f 3,500 with k1, k2, k3, top-left corner", dict(f=3500.0, k1=-0.08, k2=0.05, k3=-0.01), (0.0, 0.0),
     (60.90514376438342, 44.727214951969074)),
    ("the wide lens, top-left corner", dict(f=3500.0, cx=6.0, cy=-4.0, k1=-0.08, k2=0.05, k3=-0.01, p1=3e-4, p2=-2e-4, b1=1.5, b2=-0.7),
     (0.0, 0.0), (61.521766835876775, 44.56453414260453)),
    ("the wide lens, bottom-right corner", dict(f=3500.0, cx=6.0, cy=-4.0, k1=-0.08, k2=0.05, k3=-0.01, p1=3e-4, p2=-2e-4, b1=1.5, b2=-0.7),
     (4096.0, 3008.0), (-59.18030688078942, -44.891552816046946)),
    ("p1 and p2 alone, top-right corner", dict(f=3500.0, p1=3e-4, p2=-2e-4), (4096.0, 0.0), (1.624444342857143, -1.1554816)),
    ("b1 and b2 alone, bottom-right corner", dict(f=3500.0, b1=1.5, b2=-0.7), (4096.0, 3008.0), (0.5769142857142857, 0.0)),
]


def lens_from_tags(tags, cols, rows, resize_factor=1):
    """cameras.load_lens of a cameras.xml that holds these tags: the path the calibration takes in a run."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "cameras.xml")
        open(path, "wb").write(lens_xml([dict(id=0, width=cols, height=rows, tags=tags)], [("cam", 0)]))
        return cameras.load_lens(path, "cam", resize_factor)


@pytest.mark.parametrize("name,tags,point,shift", DISPLACEMENTS)
def test_displacements_worked_by_hand(name, tags, point, shift):
    """Sign, size and axis of the displacement at image corners, for the radial, tangential and affinity terms apart and
    together: the undistorted point (u0, v0) from the corner is index (u0 - 0.5, v0 - 0.5)."""
    lens = lens_from_tags(tags, 4096, 3008)
    rs, cs = ref.source_coords(lens, point[1] - 0.5, point[0] - 0.5)
    assert abs((cs - (point[0] - 0.5)) - shift[0]) < 1e-9 and abs((rs - (point[1] - 0.5)) - shift[1]) < 1e-9, name
    u, v = ref.manual_project(tags, 4096, 3008, (point[0] - 2048.0 - tags.get("cx", 0.0)) / tags["f"],
                              (point[1] - 1504.0 - tags.get("cy", 0.0)) / tags["f"])
    assert abs(u - point[0] - shift[0]) < 1e-9 and abs(v - point[1] - shift[1]) < 1e-9, name
    low = lens_from_tags(tags, 4096, 3008, 8)                     # the same photograph at 1/8 size: an eighth of the shift
    rs, cs = ref.source_coords(low, point[1] / 8 - 0.5, point[0] / 8 - 0.5)
    assert abs((cs - (point[0] / 8 - 0.5)) * 8 - shift[0]) < 1e-9 and abs((rs - (point[1] / 8 - 0.5)) * 8 - shift[1]) < 1e-9, name


ANALYTIC = [("wide lens / 4", 752, 1024, 1.0), ("wide lens / 4, half the coefficients", 752, 1024, 0.5),
            ("wide lens / 8", 376, 512, 1.0)]


def analytic_case(rows, cols, weight):
    """(photograph, lens, ideal image at the pixel centres, the pixels whose taps lie inside, the bound).  The photograph is
    synthesised from the raw tags by ref.manual_project's inverse; the lens is what cameras.load_lens makes of the same tags."""
    tags = ref.wide_tags(cols, rows, weight)
    lens = lens_from_tags(tags, cols, rows)
    photo = ref.synthesise_photograph(rows, cols, tags)
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    return photo, lens, ref.ideal(c + 0.5, r + 0.5), ref.inside_mask(lens, rows, cols), ref.analytic_bound(ref.magnification(lens, rows, cols))


def check_analytic(name, got, want, inside, bound):
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name}: inside {inside.mean():.4f}, largest error {err[inside].max():.5f}, bound {bound:.5f}")
    assert inside.mean() >= 0.95, name
    assert err[inside].max() <= bound, (name, err[inside].max(), bound)


@pytest.mark.parametrize("name,rows,cols,weight", ANALYTIC)
def test_undistorted_photograph_is_the_ideal_image(lens_host, name, rows, cols, weight):
    """Direction, signs, the P1 / P2 order and the half-pixel convention against a second statement of the model: the
    photograph a lens takes of I(u, v) is synthesised by inverting Metashape's formulas in the manual's absolute form
    (ref.manual_project, from the raw tags, sharing nothing with source_coords or t4d_lens.h), undistorted by the host build, and
    compared with I at the pixel centres, within the error of order-1 interpolation at the map's largest magnification plus
    half a uint8 level.  test_wrong_models_miss_the_ideal_image shows what the check catches."""
    photo, lens, want, inside, bound = analytic_case(rows, cols, weight)
    got = host_undistort(lens_host, photo, np.eye(3), (rows, cols), lens)[0].numpy()
    check_analytic(name, got, want, inside, bound)
    assert np.abs(photo[..., 0] / 255.0 - want).max() > 10 * bound            # the photograph itself is far from I


def wrong_source_coords(kind):
    """ref.source_coords with one mistake in it."""
    def coords(lens, R, C):
        f, cxa, cya, k1, k2, k3, k4, p1, p2, b1, b2 = (np.float64(x) for x in ref.lens_numbers(lens))
        if kind == "P1 and P2 swapped":
            p1, p2 = p2, p1
        if kind == "signs of K flipped":
            k1, k2, k3, k4 = -k1, -k2, -k3, -k4
        if kind == "direction reversed":
            k1, k2, k3, k4, p1, p2 = -k1, -k2, -k3, -k4, -p1, -p2
        half = 0.0 if kind == "half pixel dropped" else 0.5
        R, C = np.asarray(R, np.float64), np.asarray(C, np.float64)
        x, y = ((C + half) - cxa) / f, ((R + half) - cya) / f
        r2 = x * x + y * y
        rad = r2 * (k1 + r2 * (k2 + r2 * (k3 + r2 * k4)))
        dx = x * rad + p1 * (r2 + 2 * x * x) + 2 * p2 * x * y
        dy = y * rad + p2 * (r2 + 2 * y * y) + 2 * p1 * x * y
        if kind == "B2 on the rows":
            return R + f * dy + b2 * (y + dy), C + f * dx + b1 * (x + dx)
        return R + f * dy, C + f * dx + b1 * (x + dx) + b2 * (y + dy)
    return coords


@pytest.mark.parametrize("kind", ["none", "P1 and P2 swapped", "signs of K flipped", "direction reversed", "half pixel dropped",
                                  "B2 on the rows"])
def test_wrong_models_miss_the_ideal_image(monkeypatch, kind):
    """The analytic check on the numpy restatement with one mistake planted in its map: every one of them must miss the bound
    (and the unmodified copy must meet it, so that the copy itself is not the mistake)."""
    photo, lens, want, inside, bound = analytic_case(376, 512, 1.0)
    monkeypatch.setattr(ref, "source_coords", wrong_source_coords(kind))
    got = ref.undistort_target(photo, np.eye(3), (376, 512), lens)[0].numpy()
    if kind == "none":
        check_analytic(kind, got, want, inside, bound)
    else:
        with pytest.raises(AssertionError):
            check_analytic(kind, got, want, inside, bound)


# ---- 4. the C ABI -------------------------------------------------------------------------------------------------------------------
def test_lens_view_layout_matches_ctypes():
    fields = [n for n, _ in _lib.T4DLensView._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "topo4d_raster.h"\nint main(void) {\n' \
          '  printf("%zu %d", sizeof(T4DLensView), T4D_LENS_MAX_SUPERSAMPLE);\n' + \
          "".join('  printf(" %%zu", offsetof(T4DLensView, %s));\n' % f for f in fields) + "  return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        nums = [int(x) for x in subprocess.check_output([os.path.join(d, "s")], text=True).split()]
    assert nums[:2] == [C.sizeof(_lib.T4DLensView), _lib.T4D_LENS_MAX_SUPERSAMPLE]
    assert nums[2:] == [getattr(_lib.T4DLensView, f).offset for f in fields]


def good_view():
    v = _lib.T4DLensView()
    v.src, v.dst = 64, 64                                  # "some address": never dereferenced by a call that is rejected
    v.rows, v.cols, v.channels, v.src_pitch, v.out_rows, v.out_cols, v.supersample, v.nearest = 8, 8, 3, 24, 8, 8, 1, 0
    v.matrix[0] = v.matrix[4] = 1.0
    v.lens[0], v.lens[1], v.lens[2] = 10.0, 4.0, 4.0
    return v


BAD_VIEWS = {"no source": dict(src=None), "no destination": dict(dst=None), "no rows": dict(rows=0), "no columns": dict(cols=-1),
             "no channels": dict(channels=0), "five channels": dict(channels=5), "pitch below a row": dict(src_pitch=23),
             "empty output": dict(out_rows=0), "negative output": dict(out_cols=-4), "supersample 0": dict(supersample=0),
             "supersample past the limit": dict(supersample=_lib.T4D_LENS_MAX_SUPERSAMPLE + 1), "nearest 2": dict(nearest=2),
             "virtual image past int32": dict(out_rows=1 << 26, supersample=64)}


def test_undistort_views_rejects_bad_arguments_before_touching_a_device():
    from topo4d_amd import build
    build.build(verbose=False)
    lib = _lib.load()

    def rejected(rc):
        assert rc == _lib.T4D_ERR_ARG, (rc, lib.t4d_last_error())
        assert b"t4d_undistort_views" in lib.t4d_last_error()

    one = C.c_void_p(64)
    arr = (_lib.T4DLensView * 2)(good_view(), good_view())
    rejected(lib.t4d_undistort_views(None, one, 2, None))
    rejected(lib.t4d_undistort_views(arr, None, 2, None))
    rejected(lib.t4d_undistort_views(arr, one, 0, None))
    for why, fields in BAD_VIEWS.items():
        arr = (_lib.T4DLensView * 2)(good_view(), good_view())
        for k, x in fields.items():
            setattr(arr[1], k, x)
        rejected(lib.t4d_undistort_views(arr, one, 2, None))
        assert b"view 1" in lib.t4d_last_error(), why
    for where, k in (("matrix", 2), ("lens", 3), ("lens", 0)):
        for x in (float("nan"), float("inf")):
            arr = (_lib.T4DLensView * 2)(good_view(), good_view())
            getattr(arr[0], where)[k] = x
            rejected(lib.t4d_undistort_views(arr, one, 2, None))
    for f in (0.0, -3.0):
        arr = (_lib.T4DLensView * 1)(good_view())
        arr[0].lens[0] = f
        rejected(lib.t4d_undistort_views(arr, one, 1, None))
    arr = (_lib.T4DLensView * 1)(good_view())
    arr[0].cval = float("nan")
    rejected(lib.t4d_undistort_views(arr, one, 1, None))
