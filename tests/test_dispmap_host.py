"""CPU: the numpy restatements of the displacement-map rules (tests/dispmap_ref.py) on hand-worked cases, the strict 16-bit PNG
decoder (tests/png16_check.py) against files PIL wrote, and the argument errors of every new Python entry point, which are raised
before anything needs a device."""
import io

import numpy as np
import pytest
import torch

from tests import dispmap_ref as ref
from tests import png16_check


# ---- the references on hand-worked cases -------------------------------------------------------------------------------------
def test_quantize_ties_go_to_even_and_the_reach_maps_to_the_ends():
    dist = 32767.0                                              # one code step is one unit: disp is the step count
    disp = np.array([[0.5, 1.5, 2.5, -0.5, -1.5, 0.0, dist, -dist, 2 * dist, -2 * dist, np.inf, np.nan, 3.0]], np.float32)
    hit = np.ones(disp.shape, np.uint8)
    hit[0, -1] = 0
    code, has = ref.quantize(disp, hit, dist)
    assert code.dtype == np.int32 and has.dtype == np.uint8
    assert code.tolist() == [[32768, 32770, 32770, 32768, 32766, 32768, 65535, 1, 65535, 1, 32768, 32768, 32768]]
    assert has.tolist() == [[1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0]]
    # a reach in scan units: +-dist are the ends whatever the reach
    code, _ = ref.quantize(np.array([[0.004, -0.004, 0.002]], np.float32), np.ones((1, 3)), np.float32(0.004))
    assert code.tolist() == [[65535, 1, 32768 + 16384]]        # 0.5 * 32767 = 16383.5 -> 16384 (even)


def test_smoothing_stays_inside_the_island_and_skips_texels_without_a_value():
    code = np.full((1, 7), 100, np.int32)
    code[0, 3:] = 60000
    has = np.ones((1, 7), np.uint8)
    labels = np.array([[1, 1, 1, 2, 2, 2, 2]], np.uint8)
    out = ref.smooth(code, has, labels, 1)
    assert out.tolist() == code.tolist()                        # constant islands: no tap crosses the border
    # a tap onto a texel without a value does not count: its code never enters
    code2 = code.copy()
    code2[0, 1] = 40000
    has2 = has.copy()
    has2[0, 1] = 0
    out2 = ref.smooth(code2, has2, labels, 3)
    assert out2[0, 0] == 100 and out2[0, 2] == 100 and out2[0, 1] == 40000      # copied through, and nobody read it
    # with a value it does: texel 0 takes (36*100 + 24*40000 + 6*100 + 33) / 66
    out3 = ref.smooth(code2, has, labels, 1)
    assert out3[0, 0] == (2 * (36 * 100 + 24 * 40000 + 6 * 100) + 66) // 132
    assert out3[0, 3] == 60000
    assert ref.smooth(code2, has, labels, 0).tolist() == code2.tolist()
    # a texel of label 0 is copied through even with a value
    lab0 = labels.copy()
    lab0[0, 0] = 0
    assert ref.smooth(code2, has, lab0, 2)[0, 0] == 100


def test_a_one_texel_island_keeps_its_code_and_gets_the_flat_normal():
    code = np.array([[1000, 50000, 2000], [3000, 4000, 5000], [6000, 7000, 8000]], np.int32)
    has = np.ones((3, 3), np.uint8)
    labels = np.full((3, 3), 1, np.uint8)
    labels[1, 1] = 2
    pos = np.random.default_rng(0).random((3, 3, 3)).astype(np.float32)
    assert ref.smooth(code, has, labels, 8)[1, 1] == 4000
    n = ref.normals(code, has, labels, pos, 0.01)
    assert n.shape == (3, 3, 3) and n.dtype == np.int32
    assert n[1, 1].tolist() == [32768, 32768, 65535]
    assert n[0, 0].tolist() != [32768, 32768, 65535]
    none = ref.normals(code, np.zeros((3, 3), np.uint8), labels, pos, 0.01)
    assert (none == np.array([32768, 32768, 65535])).all()


def test_normals_follow_the_surface_metric_and_the_sign_convention():
    # a plane of codes rising 10 steps per texel to the right and 20 per texel downwards, over texels 0.5 apart in x and 0.25 in y
    y, x = np.mgrid[0:5, 0:6]
    code = (32768 + 10 * x + 20 * y).astype(np.int32)
    has, labels = np.ones((5, 6), np.uint8), np.ones((5, 6), np.uint8)
    pos = np.stack([0.5 * x, -0.25 * y, 0 * x], -1).astype(np.float32)
    unit = 0.001
    n = ref.decode_normals(ref.normals(code, has, labels, pos, unit))
    sx, sy = 10 * unit / 0.5, 20 * unit / 0.25                  # one-sided at the borders: the same slope on a plane
    want = np.array([-sx, sy, 1.0]) / np.sqrt(sx * sx + sy * sy + 1.0)
    assert np.abs(n - want).max() <= 1.0 / 65535.0
    # two texels at the same point: a == 0 gives slope 0 along that axis
    flat = ref.normals(code, has, labels, np.zeros((5, 6, 3), np.float32), unit)
    assert (flat == np.array([32768, 32768, 65535])).all()


def test_fill16_reference_on_small_cases():
    img = np.full((4, 4), 65535, np.int32)
    valid = np.ones((4, 4), np.uint8)
    valid[1:3, 1:3] = 0
    img[valid == 0] = 7
    out, filled = ref.fill16(img, valid)
    assert (out == 65535).all() and filled.sum() == 4
    out, filled = ref.fill16(img, np.zeros((4, 4), np.uint8))
    assert np.array_equal(out, img) and filled.sum() == 0
    two = np.array([[10, 0, 0, 50010]], np.int32)
    out, _ = ref.fill16(two, np.array([[1, 0, 0, 1]]))
    assert out[0, 0] == 10 and out[0, 3] == 50010 and 10 < out[0, 1] <= out[0, 2] < 50010
    lab = np.array([[1, 1, 2, 2]], np.uint8)
    out, filled = ref.fill16_islands(two, np.array([[1, 0, 0, 1]]), lab)
    assert out.tolist() == [[10, 10, 50010, 50010]] and filled.tolist() == [[0, 1, 1, 0]]


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (9, 40)])
def test_the_16_bit_decoder_reads_what_pil_writes(shape):
    from PIL import Image
    img = np.random.default_rng(3).integers(0, 65536, shape).astype(np.uint16)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    got, filters = png16_check.decode_png16(buf.getvalue())
    assert got.shape == shape + (1,) and np.array_equal(got[..., 0], img.astype(np.int32)) and filters.shape == (shape[0],)
    with pytest.raises(png16_check.PngError):
        buf8 = io.BytesIO()
        Image.fromarray((img >> 8).astype(np.uint8)).save(buf8, format="PNG")
        png16_check.decode_png16(buf8.getvalue())              # depth 8 is refused
    assert png16_check.best_filters(np.zeros((3, 4, 1), np.int32)).tolist() == [0, 0, 0]
    ramp = (np.arange(12).reshape(1, 12, 1) * 257).astype(np.int32)
    assert png16_check.best_filters(ramp).tolist() == [1]       # a ramp: Sub leaves 1, 1 per sample; Up on row 0 is None


# ---- argument errors, without a device ---------------------------------------------------------------------------------------
def test_png16_argument_errors():
    from topo4d_amd import png
    ok = torch.zeros(4, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="tensor"):
        png.encode_png16(np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError, match="int32"):
        png.encode_png16(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="int32"):
        png.encode_png16(torch.zeros(4, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        png.encode_png16(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="C in"):
        png.encode_png16(torch.zeros(4, 4, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match=">= 1"):
        png.encode_png16(torch.zeros(0, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.encode_png16(ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.write_png16("/nonexistent/x.png", ok)
    with pytest.raises(ValueError):
        png.max_encoded_bytes16(4, 4, 2)
    with pytest.raises(ValueError):
        png.max_encoded_bytes16(0, 4, 1)
    # the bound: every segment stored, plus the framing; 16-bit rows are 1 + 2 w c bytes
    n = 40 * (1 + 2 * 300)
    segs = -(-n // 16384)
    assert png.max_encoded_bytes16(40, 300, 1) == 47 + 28 + n + segs * 17 == png.max_encoded_bytes(40, 600, 1)


def test_fill16_argument_errors():
    from topo4d_amd import texfinish as TF
    img = torch.zeros(4, 5, dtype=torch.int32)
    valid = torch.ones(4, 5, dtype=torch.uint8)
    labels = torch.ones(4, 5, dtype=torch.uint8)
    for fn, third in ((TF.fill16, None), (TF.fill16_islands, labels)):
        with pytest.raises(ValueError, match="int32"):
            fn(torch.zeros(4, 5, dtype=torch.uint8), valid, third)
        with pytest.raises(ValueError, match="int32"):
            fn(np.zeros((4, 5), np.int32), valid, third)
        with pytest.raises(ValueError, match="c in"):
            fn(torch.zeros(4, 5, 2, dtype=torch.int32), valid, third)
        with pytest.raises(ValueError, match="valid"):
            fn(img, torch.ones(5, 4, dtype=torch.uint8), third)
        with pytest.raises(ValueError, match="valid"):
            fn(img, valid.to(torch.float32), third)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(img, valid, third)
    with pytest.raises(ValueError, match="domain"):
        TF.fill16(img, valid, torch.ones(4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="labels"):
        TF.fill16_islands(img, valid, labels.to(torch.int32))
    with pytest.raises(ValueError, match="labels"):
        TF.fill16_islands(img, valid, torch.ones(5, 4, dtype=torch.uint8))


def test_dispmap_argument_errors(tmp_path):
    from topo4d_amd import dispmap as D
    disp = torch.zeros(4, 5, dtype=torch.float32)
    hit = torch.ones(4, 5, dtype=torch.uint8)
    code = torch.zeros(4, 5, dtype=torch.int32)
    labels = torch.ones(4, 5, dtype=torch.uint8)
    pos = torch.zeros(4, 5, 3, dtype=torch.float32)
    with pytest.raises(ValueError, match="disp"):
        D.quantize(disp.to(torch.float64), hit, 1.0)
    with pytest.raises(ValueError, match="disp"):
        D.quantize(torch.zeros(4, dtype=torch.float32), hit, 1.0)
    with pytest.raises(ValueError, match="hit"):
        D.quantize(disp, torch.ones(5, 4, dtype=torch.uint8), 1.0)
    with pytest.raises(ValueError, match="hit"):
        D.quantize(disp, hit.to(torch.int32), 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="dist"):
            D.quantize(disp, hit, bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.quantize(disp, hit, 1.0)
    with pytest.raises(ValueError, match="code"):
        D.smooth(code.to(torch.int64), hit, labels, 1)
    with pytest.raises(ValueError, match="has"):
        D.smooth(code, torch.ones(4, 4, dtype=torch.uint8), labels, 1)
    with pytest.raises(ValueError, match="labels"):
        D.smooth(code, hit, labels.to(torch.bool), 1)
    for bad in (-1, 9, 1.5):
        with pytest.raises(ValueError, match="smooth"):
            D.smooth(code, hit, labels, bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.smooth(code, hit, labels, 1)
    with pytest.raises(ValueError, match="pos"):
        D.normals(code, hit, labels, torch.zeros(4, 5, 2), 0.1)
    with pytest.raises(ValueError, match="pos"):
        D.normals(code, hit, labels, torch.zeros(5, 4, 3), 0.1)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="unit"):
            D.normals(code, hit, labels, pos, bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.normals(code, hit, labels, pos, 0.1)
    # finish: the maps, the reach and the round count before a device is looked for
    with pytest.raises(ValueError, match="disp"):
        D.finish(None, None, code, hit, 1.0)
    with pytest.raises(ValueError, match="hit"):
        D.finish(None, None, disp, torch.ones(4, 4, dtype=torch.uint8), 1.0)
    with pytest.raises(ValueError, match="dist"):
        D.finish(None, None, disp, hit, 0.0)
    with pytest.raises(ValueError, match="smooth"):
        D.finish(None, None, disp, hit, 1.0, smooth=9)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.write_frame(str(tmp_path), {"code": code})
    assert not list(tmp_path.iterdir())
    assert D.png_info(32767.0, True, 2, False) == {"zero": 32768, "unit": 1.0, "fill": True, "smooth": 2, "normals": False}
    assert D.code_unit(0.5) == 0.5 / 32767


def test_command_lines_refuse_bad_options(tmp_path):
    from topo4d_amd import dispmap as D
    from topo4d_amd import evaluate as E
    (tmp_path / "exp" / "seq").mkdir(parents=True)
    (tmp_path / "scans").mkdir()
    base = ["-e", "exp", "-s", "seq", "-od", str(tmp_path), "--set", "none", "--scans", str(tmp_path / "scans")]
    for extra in (["--disp_png"], ["--disp_fill"], ["--disp_smooth", "2"], ["--disp_normals"],         # no --bake_disp
                  ["--bake_disp", "0", "--disp_png"], ["--bake_disp", "0", "--disp_normals"],        # DIST must be > 0
                  ["--bake_disp", "0.01", "--disp_smooth", "9"], ["--bake_disp", "0.01", "--disp_smooth", "-1"]):
        with pytest.raises(SystemExit) as e:
            E.evaluate(E.build_parser().parse_args(base + extra))
        assert "disp" in str(e.value), extra
    args = E.build_parser().parse_args(base)
    assert (args.disp_png, args.disp_fill, args.disp_smooth, args.disp_normals) == (False, False, 0, False)
    assert E.disp_png_options(args) is None
    args = E.build_parser().parse_args(base + ["--bake_disp", "32767", "--disp_smooth", "3"])
    assert E.disp_png_options(args) == {"zero": 32768, "unit": 1.0, "fill": False, "smooth": 3, "normals": False}
    own = ["-e", "exp", "-s", "seq", "-od", str(tmp_path)]
    for extra in (["--dist", "0"], ["--dist", "nan"], ["--dist", "0.01", "--smooth", "9"]):
        with pytest.raises(SystemExit) as e:
            D.finish_tree(D.build_parser().parse_args(own + extra))
        assert "dist" in str(e.value) or "smooth" in str(e.value)
    with pytest.raises(SystemExit):
        D.build_parser().parse_args(own)                        # --dist is required
    with pytest.raises(SystemExit, match="no run"):
        D.finish_tree(D.build_parser().parse_args(["-e", "exp", "-s", "other", "-od", str(tmp_path), "--dist", "0.01"]))


def test_every_new_export_rejects_bad_arguments_before_touching_a_device():
    import ctypes as C
    from topo4d_amd import _lib
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, two = C.c_void_p(64), C.c_void_p(4096)             # "some address": never dereferenced by a call that is rejected

    def rejected(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    cap, ns = lib.t4d_png_max_bytes16(4, 4, 1), lib.t4d_png_scratch_bytes16(4, 4, 1)
    assert cap > 0 and ns > 0 and lib.t4d_png_max_bytes16(4, 4, 2) == 0 and lib.t4d_png_scratch_bytes16(0, 4, 1) == 0
    rejected(lib.t4d_png_encode16(None, 4, 4, 1, one, cap, one, one, ns, None))
    rejected(lib.t4d_png_encode16(one, 4, 4, 2, one, cap, one, one, ns, None))
    rejected(lib.t4d_png_encode16(one, 4, 4, 1, one, cap - 1, one, one, ns, None))
    rejected(lib.t4d_png_encode16(one, 4, 4, 1, one, cap, one, one, ns - 1, None), SIZE)
    nf = lib.t4d_texture_fill16_scratch_bytes(5, 7, 1)
    assert nf > 0 and lib.t4d_texture_fill16_scratch_bytes(5, 7, 2) == 0 and lib.t4d_texture_fill16_scratch_bytes(0, 7, 1) == 0
    assert lib.t4d_texture_fill16_scratch_bytes(64, 64, 3) > lib.t4d_texture_fill_scratch_bytes(64, 64, 3)
    rejected(lib.t4d_texture_fill16(None, one, None, 5, 7, 1, two, two, two, nf, None))
    rejected(lib.t4d_texture_fill16(one, one, None, 5, 7, 1, one, two, two, nf, None))      # in place
    rejected(lib.t4d_texture_fill16(one, one, None, 5, 7, 2, two, two, two, nf, None))
    rejected(lib.t4d_texture_fill16(one, one, None, 70000, 7, 1, two, two, two, nf, None))
    rejected(lib.t4d_texture_fill16(one, one, None, 5, 7, 1, two, two, two, nf - 1, None), SIZE)
    rejected(lib.t4d_texture_fill16(one, one, None, 5, 7, 1, two, two, C.c_void_p(4098), nf, None))   # scratch not aligned
    rejected(lib.t4d_disp_quantize(None, one, 4, 4, 1.0, two, two, None))
    rejected(lib.t4d_disp_quantize(one, one, 0, 4, 1.0, two, two, None))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rejected(lib.t4d_disp_quantize(one, one, 4, 4, bad, two, two, None))
    nsm = lib.t4d_disp_smooth_scratch_bytes(4, 4)
    assert nsm >= 64 and lib.t4d_disp_smooth_scratch_bytes(4, 0) == 0
    rejected(lib.t4d_disp_smooth(one, one, one, 4, 4, 1, None, two, nsm, None))
    rejected(lib.t4d_disp_smooth(one, one, one, 4, 4, 1, one, two, nsm, None))             # in place
    rejected(lib.t4d_disp_smooth(one, one, one, 4, 4, 9, two, two, nsm, None))
    rejected(lib.t4d_disp_smooth(one, one, one, 4, 4, -1, two, two, nsm, None))
    rejected(lib.t4d_disp_smooth(one, one, one, 4, 4, 1, two, two, nsm - 1, None), SIZE)
    rejected(lib.t4d_disp_normals(one, one, one, None, 4, 4, 0.1, two, None))
    rejected(lib.t4d_disp_normals(one, one, one, one, 4, 4, 0.0, two, None))
    rejected(lib.t4d_disp_normals(one, one, one, one, 4, 70000, 0.1, two, None))
