"""GPU: topo4d_amd.dispmap and texfinish.fill16 - bit for bit against the numpy restatements of tests/dispmap_ref.py, the normal map
of an analytic scene (a flat square under a tilted plane) under two UV layouts, the fill of a knocked-out disc on the height field
of tests/test_gpu_scanbake.py, and `evaluate --bake_disp ... --disp_*` and `python -m topo4d_amd.dispmap` end to end on the
two-frame run of tests/test_gpu_scanscore.py."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import dispmap_ref as ref
from tests import png16_check
from tests.test_gpu_scanbake import height_field, square
from tests.test_gpu_scanscore import _eval, run                              # noqa: F401  (run: the module's fixture)
from topo4d_amd import dispmap, meshrender, projtex, scanbake, scanscore
from topo4d_amd import texfinish as TF

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = 64
FLAT = [32768, 32768, 65535]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


# ---- the 16-bit push-pull fill ------------------------------------------------------------------------------------------------
def valid_sets(h, w, rng):
    """{name: (valid, domain or None)}"""
    single = np.zeros((h, w), np.uint8)
    single[h // 2, w // 3] = 1
    return {"sparse": ((rng.random((h, w)) < 0.08).astype(np.uint8), None),
            "dense": ((rng.random((h, w)) < 0.7).astype(np.uint8), None),
            "single": (single, None),
            "none": (np.zeros((h, w), np.uint8), None),
            "domain": ((rng.random((h, w)) < 0.3).astype(np.uint8), (rng.random((h, w)) < 0.5).astype(np.uint8))}


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (65, 130), (128, 128)])
def test_fill16_equals_the_reference(shape):
    """1x1 has no level above it, 5x7 has odd ceil-halving levels, 65x130 crosses the 64-texel tile both ways"""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(0, 65536, (h, w)).astype(np.int32)
    for name, (valid, domain) in valid_sets(h, w, rng).items():
        out, filled = TF.fill16(dev(img), dev(valid), None if domain is None else dev(domain))
        assert out.dtype == torch.int32 and filled.dtype == torch.uint8 and out.shape == (h, w)
        want, want_filled = ref.fill16(img, valid, domain)
        assert np.array_equal(host(filled), want_filled), name
        assert np.array_equal(host(out), want), name
        if name == "none":
            assert np.array_equal(host(out), img) and int(filled.sum()) == 0
        if name == "single" and (h, w) != (1, 1):
            assert (host(out)[valid == 0] == img[valid != 0][0]).all() and int(filled.sum()) == h * w - 1
    # bool masks are taken as well
    valid, _ = valid_sets(h, w, rng)["dense"]
    a = TF.fill16(dev(img), dev(valid != 0))
    b = TF.fill16(dev(img), dev(valid))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("c", [3, 4])
def test_fill16_with_channels(c):
    rng = np.random.default_rng(c)
    img = rng.integers(0, 65536, (65, 130, c)).astype(np.int32)
    valid = (rng.random((65, 130)) < 0.1).astype(np.uint8)
    domain = (rng.random((65, 130)) < 0.8).astype(np.uint8)
    out, filled = TF.fill16(dev(img), dev(valid), dev(domain))
    want, want_filled = ref.fill16(img, valid, domain)
    assert np.array_equal(host(out), want) and np.array_equal(host(filled), want_filled)


@pytest.mark.parametrize("shape", [(5, 7), (65, 130), (128, 128)])
def test_fill16_keeps_a_white_image_white(shape):
    """every sample 65535: the push sum is 16 * 65535 * 256 + 8 > 2^31, which a signed 32-bit sum would turn negative"""
    h, w = shape
    rng = np.random.default_rng(9)
    valid = (rng.random((h, w)) < 0.05).astype(np.uint8)
    valid[0, 0] = 1
    img = np.where(valid != 0, 65535, 0).astype(np.int32)
    out, filled = TF.fill16(dev(img), dev(valid))
    assert int(filled.sum()) == int((valid == 0).sum()) > 0
    assert bool((out == 65535).all())


def test_fill16_islands_do_not_mix():
    h, w = 65, 130
    rng = np.random.default_rng(11)
    labels = np.zeros((h, w), np.uint8)
    labels[:, :60] = 1
    labels[:, 60:] = 2                                           # the islands touch along a line inside a tile
    labels[:3] = 0
    labels[20:30, 100:110] = 3                                   # an island without any valid texel: stays as it is
    consts = {1: 1000, 2: 64000}
    valid = (rng.random((h, w)) < 0.2).astype(np.uint8)
    valid[labels == 3] = 0
    img = rng.integers(0, 65536, (h, w)).astype(np.int32)
    for i, v in consts.items():
        img[(labels == i) & (valid != 0)] = v
    out, filled = TF.fill16_islands(dev(img), dev(valid), dev(labels))
    want, want_filled = ref.fill16_islands(img, valid, labels)
    assert np.array_equal(host(out), want) and np.array_equal(host(filled), want_filled)
    o = host(out)
    for i, v in consts.items():
        assert (o[labels == i] == v).all()
    untouched = (labels == 0) | (labels == 3)
    assert np.array_equal(o[untouched], img[untouched]) and not host(filled)[untouched].any()
    # random values per island: still the reference, bit for bit
    img2 = rng.integers(0, 65536, (h, w)).astype(np.int32)
    out2, filled2 = TF.fill16_islands(dev(img2), dev(valid), dev(labels))
    want2, want_filled2 = ref.fill16_islands(img2, valid, labels)
    assert np.array_equal(host(out2), want2) and np.array_equal(host(filled2), want_filled2)


# ---- quantise, smooth, normals against the reference -------------------------------------------------------------------------
def random_maps(h, w, seed):
    """codes over the full range, random `has`, three labelled islands that touch and a strip of label 0, and surface points with
    repeats (neighbours at the same point: a == 0)"""
    rng = np.random.default_rng(seed)
    code = rng.integers(0, 65536, (h, w)).astype(np.int32)
    code[0, :4] = [0, 65535, 0, 65535]
    has = (rng.random((h, w)) < 0.8).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    labels = np.where(x + y < (h + w) // 3, 1, np.where(x > w // 2, 2, 3)).astype(np.uint8)
    labels[h // 2, :] = np.where(rng.random(w) < 0.5, 0, labels[h // 2, :])
    labels[:, -1] = 0
    pos = rng.random((h, w, 3)).astype(np.float32)
    pos[:, 10:14] = pos[:, 10:11]                                # runs of equal points along x
    pos[20:23] = pos[20:21]                                      # and along y
    return code, has, labels, pos


@pytest.fixture(scope="module", params=[(64, 64), (65, 130)], ids=lambda s: "%dx%d" % s)
def maps(request):
    h, w = request.param
    return random_maps(h, w, seed=h + w)


def test_quantize_equals_the_reference(maps):
    h, w = maps[0].shape
    rng = np.random.default_rng(3)
    dist = 0.0123
    disp = (rng.uniform(-1.2, 1.2, (h, w)) * dist).astype(np.float32)
    steps = rng.integers(-32767, 32767, w)
    disp[0] = ((steps + 0.5) * (dist / 32767.0)).astype(np.float32)      # close to ties
    disp[1, :8] = [dist, -dist, 2 * dist, -2 * dist, np.inf, -np.inf, np.nan, 0.0]
    hit = (rng.random((h, w)) < 0.7).astype(np.uint8)
    hit[1, :8] = 1
    code, has = dispmap.quantize(dev(disp), dev(hit), dist)
    want, want_has = ref.quantize(disp, hit, dist)
    assert code.dtype == torch.int32 and has.dtype == torch.uint8
    assert np.array_equal(host(code), want) and np.array_equal(host(has), want_has)
    assert host(code)[1, :8].tolist() == [65535, 1, 65535, 1, 32768, 32768, 32768, 32768] and host(has)[1, :8].tolist() == [1] * 4 + [0] * 3 + [1]
    # exact ties in float64: a reach of 32767 makes disp the step count
    ties = (np.arange(h * w).reshape(h, w) % 200 - 100 + 0.5).astype(np.float32)
    code, _ = dispmap.quantize(dev(ties), dev(np.ones((h, w), np.uint8)), 32767.0)
    assert np.array_equal(host(code), ref.quantize(ties, np.ones((h, w)), 32767.0)[0]) and bool((code % 2 == 0).all())


@pytest.mark.parametrize("rounds", [0, 1, 2, 8])
def test_smooth_equals_the_reference(maps, rounds):
    code, has, labels, _ = maps
    out = dispmap.smooth(dev(code), dev(has), dev(labels), rounds)
    want = ref.smooth(code, has, labels, rounds)
    assert out.dtype == torch.int32 and np.array_equal(host(out), want)
    keep = (has == 0) | (labels == 0)
    assert np.array_equal(host(out)[keep], code[keep])
    if rounds == 0:
        assert np.array_equal(host(out), code)
    else:
        assert not np.array_equal(host(out), code)


def test_normals_equal_the_reference(maps):
    code, has, labels, pos = maps
    for unit in (1.0 / 32767, 3e-6):
        out = dispmap.normals(dev(code), dev(has), dev(labels), dev(pos), unit)
        want = ref.normals(code, has, labels, pos, unit)
        assert out.dtype == torch.int32 and out.shape == code.shape + (3,)
        assert np.array_equal(host(out), want)
    none = (has == 0) | (labels == 0)
    assert (host(out)[none] == np.array(FLAT)).all() and not (host(out)[~none] == np.array(FLAT)).all()
    # smooth codes: the slopes are small and the normals near +z, where the rounding of the encoding is the finest test
    y, x = np.mgrid[0:code.shape[0], 0:code.shape[1]]
    wave = (32768 + 3000 * np.sin(x / 5.0) * np.cos(y / 7.0)).astype(np.int32)
    out = dispmap.normals(dev(wave), dev(has), dev(labels), dev(pos), 1e-5)
    assert np.array_equal(host(out), ref.normals(wave, has, labels, pos, 1e-5))


# ---- analytic: a flat square under a tilted plane ----------------------------------------------------------------------------
ALPHA, BETA = 0.02, -0.03
REACH = 0.0625


def plane_scan():
    """z = 0.01 + ALPHA x + BETA y over [-0.2, 1.2]^2, two triangles, normals towards +z"""
    c = np.array([[-0.2, -0.2], [1.2, -0.2], [1.2, 1.2], [-0.2, 1.2]])
    v = np.concatenate([c, (0.01 + ALPHA * c[:, :1] + BETA * c[:, 1:])], 1)
    return scanscore.Scan(v, np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def interior(has):
    """texels whose four neighbours have a value too"""
    m = has != 0
    out = np.zeros_like(m)
    out[1:-1, 1:-1] = m[1:-1, 1:-1] & m[:-2, 1:-1] & m[2:, 1:-1] & m[1:-1, :-2] & m[1:-1, 2:]
    return out


def plane_normals(v_scale):
    obj = square()
    obj = meshrender.FaceObj(obj.vertices, obj.uvs * np.array([1.0, v_scale]), obj.faces_ori, obj.uv_faces_ori)
    verts = dev(obj.vertices)
    disp, hit, _ = scanbake.bake_displacement(obj, verts, plane_scan(), RES, REACH, device=DEV)
    result = dispmap.finish(obj, verts, disp, hit, REACH, normals=True, device=DEV)
    assert sorted(result) == ["code", "filled", "has", "normal"] and int(result["filled"].sum()) == 0
    assert torch.equal(result["has"], hit)
    return ref.decode_normals(host(result["normal"])), interior(host(result["has"])), host(result["normal"]), host(result["has"])


def test_the_normal_map_of_a_tilted_plane():
    """Every interior covered texel decodes to normalize(-ALPHA, -BETA, 1), under UV = (x, y) and under UV = (x, y / 2): the
    surface's own texel lengths set the slope, not the texel counts.
    Tolerance: a code is the displacement rounded to a step, so the difference of two codes is off by at most one step, `unit`, and
    the slope over the shortest span `a` (two texels of the unit square at RES: 2 / RES) by at most unit / a; a component of the unit
    normal moves by at most the slope's error (|d n_i / d s_i| <= 1; the cross terms carry a factor |s| <= 0.03); the 16-bit
    encoding adds half a step of 2 / 65535."""
    unit = REACH / 32767.0
    a = 2.0 / RES
    tol = unit / a + 1.0 / 65535.0
    want = np.array([-ALPHA, -BETA, 1.0]) / np.sqrt(ALPHA * ALPHA + BETA * BETA + 1.0)
    full, inner_full, raw_full, has_full = plane_normals(1.0)
    half, inner_half, raw_half, has_half = plane_normals(0.5)
    assert inner_full.sum() > 0.8 * RES * RES and 0.35 * RES * RES < inner_half.sum() < 0.5 * RES * RES
    for got, inner in ((full, inner_full), (half, inner_half)):
        err = np.abs(got[inner] - want).max()
        print("largest component error", err, "tolerance", tol, "texels", int(inner.sum()))
        assert err <= tol
    # the two layouts state the same normal: both lie within the bound of it, texel by texel (above), and so do their means
    assert np.abs(full[inner_full].mean(0) - half[inner_half].mean(0)).max() <= tol
    assert (raw_full[has_full == 0] == np.array(FLAT)).all() and (raw_half[has_half == 0] == np.array(FLAT)).all()
    assert (has_half == 0).sum() > 0.4 * RES * RES
    # had texel counts set the slope, the half-height layout would state a v-slope twice as large
    wrong = np.array([-ALPHA, -2 * BETA, 1.0]) / np.sqrt(ALPHA * ALPHA + 4 * BETA * BETA + 1.0)
    assert np.abs(half[inner_half] - wrong).max() > 10 * tol


@pytest.fixture(scope="module")
def field():
    obj = square()
    v, f, _, _ = height_field()
    verts = dev(obj.vertices)
    disp, hit, _ = scanbake.bake_displacement(obj, verts, scanscore.Scan(v, f), RES, REACH, device=DEV)
    pos = projtex.surface_maps(obj, verts, RES, device=DEV)[0]
    labels = projtex.island_labels(obj, RES, RES, device=DEV)
    return dict(obj=obj, verts=verts, disp=disp, hit=hit, pos=host(pos), labels=host(labels))


def test_a_knocked_out_disc_is_filled_from_its_island(field):
    y, x = np.mgrid[0:RES, 0:RES]
    disc = (x - 30) ** 2 + (y - 35) ** 2 <= 8 ** 2
    hit = host(field["hit"]).copy()
    assert hit[disc].all()
    hit[disc] = 0
    result = dispmap.finish(field["obj"], field["verts"], field["disp"], dev(hit), REACH, fill=True, device=DEV)
    code, has, filled = host(result["code"]), host(result["has"]), host(result["filled"])
    isl = field["labels"] != 0
    assert np.array_equal(filled != 0, isl & (hit == 0)) and filled[disc].all()
    assert np.array_equal(has, hit | filled)
    plain, _ = ref.quantize(host(field["disp"]), hit, REACH)
    lo, hi = plain[hit != 0].min(), plain[hit != 0].max()
    assert lo > 32768 and hi < 65535                             # heights 8/1024 .. 0.05 under a reach of 1/16
    print("valid codes", lo, hi, "filled codes", code[filled != 0].min(), code[filled != 0].max(), "texels", int(filled.sum()))
    assert (code[filled != 0] >= lo).all() and (code[filled != 0] <= hi).all()
    assert np.array_equal(code[hit != 0], plain[hit != 0])
    assert (code[~isl] == 32768).all() and not has[~isl].any()


@pytest.mark.parametrize("fill,rounds,normals", [(False, 0, False), (True, 0, False), (False, 3, True), (True, 2, True)])
def test_finish_equals_the_reference_steps(field, fill, rounds, normals):
    y, x = np.mgrid[0:RES, 0:RES]
    hit = host(field["hit"]).copy()
    hit[(x - 20) ** 2 + (y - 40) ** 2 <= 36] = 0
    hit[::7, ::5] = 0
    result = dispmap.finish(field["obj"], field["verts"], field["disp"], dev(hit), REACH, fill=fill, smooth=rounds, normals=normals,
                            device=DEV)
    want = ref.finish(field["labels"], field["pos"], host(field["disp"]), hit, REACH, fill, rounds, normals)
    assert sorted(result) == sorted(want)
    for k in want:
        assert np.array_equal(host(result[k]), want[k]), k
    assert (int(result["filled"].sum()) > 0) == fill


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli_finishes_the_displacement_map_end_to_end(run, tmp_path):          # noqa: F811
    out = str(tmp_path / "out")
    shutil.copytree(run["out"], out)
    run_dir = os.path.join(out, "exp", "seq")
    frame = os.path.join(run_dir, "000001")
    dist = 2.0 * run["delta"]
    base = ["--scans", run["scans"], "--set", "none", "--scan_unit", "1000", "--bake_disp", repr(dist), "--bake_res", "256",
            "--bake_both_sides"]
    before = _tree(out)
    plain_text = _eval(run, *base, out=out)
    plain = json.loads(plain_text)
    plain_files = {n: open(os.path.join(frame, n), "rb").read() for n in ("face_disp.npy", "face_disp_hit.png")}
    new = sorted(set(_tree(out)) - set(before) - {os.path.join("exp", "seq", "eval.json")})
    assert new == [os.path.join("exp", "seq", "000001", n) for n in ("face_disp.npy", "face_disp_hit.png")]     # no PNG without a flag
    assert "png" not in plain["scan"]["bake"] and "filled" not in plain["scan"]["frames"]["000001"]["displacement"]

    full = json.loads(_eval(run, *base, "--disp_fill", "--disp_smooth", "2", "--disp_normals", out=out))
    new = sorted(set(_tree(out)) - set(before) - {os.path.join("exp", "seq", "eval.json")})
    assert new == [os.path.join("exp", "seq", "000001", n) for n in ("face_disp.npy", "face_disp.png", "face_disp_hit.png",
                                                                      "face_disp_normal.png")]
    for n, data in plain_files.items():
        assert open(os.path.join(frame, n), "rb").read() == data
    # the PNGs decode to dispmap.finish's arrays
    sv, sf, _, _ = run["made"][1]
    obj = meshrender.read_face_obj(os.path.join(frame, "face.obj"))
    disp, hit, _ = scanbake.bake_displacement(obj, obj.vertices, scanscore.Scan(sv, sf.astype(np.int32)), 256, dist, same_side=False,
                                              device=DEV)
    want = dispmap.finish(obj, obj.vertices, disp, hit, dist, fill=True, smooth=2, normals=True, device=DEV)
    pngs = {n: open(os.path.join(frame, n), "rb").read() for n in ("face_disp.png", "face_disp_normal.png")}
    code, _ = png16_check.decode_png16(pngs["face_disp.png"])
    normal, _ = png16_check.decode_png16(pngs["face_disp_normal.png"])
    assert code.shape == (256, 256, 1) and np.array_equal(code[..., 0], host(want["code"]))
    assert normal.shape == (256, 256, 3) and np.array_equal(normal, host(want["normal"]))
    assert 0 < int(want["filled"].sum()) and len(np.unique(code)) > 16
    # eval.json carries the new keys, and nothing else changed
    assert full["scan"]["bake"]["png"] == {"zero": 32768, "unit": dist / 32767, "fill": True, "smooth": 2, "normals": True}
    assert full["scan"]["frames"]["000001"]["displacement"]["filled"] == int(want["filled"].sum())
    assert "filled" not in full["scan"]["frames"]["000002"]["displacement"]      # a cloud: nothing baked, nothing finished
    strip = json.loads(json.dumps(full))
    del strip["scan"]["bake"]["png"]
    del strip["scan"]["frames"]["000001"]["displacement"]["filled"]
    assert strip == plain
    # --disp_png alone: the quantised map, no normal map, nothing filled
    os.remove(os.path.join(frame, "face_disp_normal.png"))
    only = json.loads(_eval(run, *base, "--disp_png", out=out))
    assert not os.path.exists(os.path.join(frame, "face_disp_normal.png"))
    assert only["scan"]["bake"]["png"] == {"zero": 32768, "unit": dist / 32767, "fill": False, "smooth": 0, "normals": False}
    assert only["scan"]["frames"]["000001"]["displacement"]["filled"] == 0
    code, _ = png16_check.decode_png16(open(os.path.join(frame, "face_disp.png"), "rb").read())
    assert np.array_equal(code[..., 0], host(dispmap.quantize(disp, hit, dist)[0]))
    # the same flags again without the new ones: the parent's files and JSON, byte for byte
    assert _eval(run, *base, out=out) == plain_text
    # python -m topo4d_amd.dispmap on that tree reproduces the PNGs byte for byte
    os.remove(os.path.join(frame, "face_disp.png"))
    argv = ["-e", "exp", "-s", "seq", "-od", out, "--dist", repr(dist), "--fill", "--smooth", "2", "--normals"]
    written = dispmap.finish_tree(dispmap.build_parser().parse_args(argv), device=DEV)
    assert written == [os.path.join(frame, n) for n in ("face_disp.png", "face_disp_normal.png")]      # frame 2 holds no bake
    for n, data in pngs.items():
        assert open(os.path.join(frame, n), "rb").read() == data
    assert dispmap.finish_tree(dispmap.build_parser().parse_args(argv + ["--frames", "2"]), device=DEV) == []
