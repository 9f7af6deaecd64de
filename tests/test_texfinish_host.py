"""CPU: the brute force of tests/texfinish_ref.py reproduces hand-worked cases of the finishing rules; every new export rejects
bad arguments with a code and a message before anything touches a device; the argument errors and the command-line defaults of
topo4d_amd/texfinish.py, and train's namespace without the new flags."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import texfinish_ref as ref


# ---- the yardstick on cases worked by hand ---------------------------------------------------------------------------------
def test_pad_takes_the_upper_of_four_equidistant_neighbours():
    up, left, right, down = (10, 20, 30), (40, 50, 60), (70, 80, 90), (100, 110, 120)
    img = np.zeros((3, 3, 3), np.uint8)
    img[0, 1], img[1, 0], img[1, 2], img[2, 1] = up, left, right, down
    cov = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], np.uint8)
    out, out_cov = ref.pad(img, cov, 1)
    want = np.array([[up, up, up],                       # the corners: (d^2 = 1) the smaller y' wins, left / right lose to up
                     [left, up, right],                  # the centre: four candidates at d^2 = 1, the smallest y' is the upper one
                     [left, down, right]], np.uint8)     # the lower corners: y' = 1 (left / right) before y' = 2 (down)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(out_cov, np.ones((3, 3), np.uint8))


def test_pad_prefers_the_left_texel_within_a_row_and_the_nearer_over_the_upper():
    img = np.zeros((3, 5), np.uint8)
    img[1, 0], img[1, 4], img[0, 3] = 7, 9, 5
    cov = (img != 0).astype(np.uint8)
    out, _ = ref.pad(img, cov, 2)
    assert out[1, 2] == 5                                 # (3,0) at d^2 = 2 beats both row neighbours at d^2 = 4
    assert out[2, 2] == 0                                 # d^2 = 5 to either row neighbour: outside the disc of radius 2
    img[0, 3] = 0
    out, _ = ref.pad(img, (img != 0).astype(np.uint8), 2)
    assert out[1, 2] == 7                                 # equal d^2 and y': the smaller x' wins


def test_pad_is_a_disc_not_a_square():
    R = 3
    img = np.zeros((12, 12), np.uint8)
    img[5, 5] = 200
    cov = (img != 0).astype(np.uint8)
    out, out_cov = ref.pad(img, cov, R)
    assert out[5, 5 + R] == 200 and out_cov[5, 5 + R] == 1      # offset (R, 0): d^2 = R^2, inside
    assert out[6, 5 + R] == 0 and out_cov[6, 5 + R] == 0        # offset (R, 1): d^2 = R^2 + 1, stays unfilled
    assert out[5 + R, 6] == 0 and out_cov[5 + R, 6] == 0
    assert int(out_cov.sum()) == 29                             # the lattice points of the disc of radius 3
    out0, cov0 = ref.pad(img, cov, 0)
    np.testing.assert_array_equal(out0, img)
    np.testing.assert_array_equal(cov0, cov)


def test_halve_rounds_half_up_over_the_covered_texels_only():
    #         cnt = 1        cnt = 2        cnt = 3        cnt = 4        cnt = 0       cnt = 4
    img = np.array([[7, 99, 1, 2, 1, 1, 1, 2, 50, 60, 0, 0],
                    [99, 99, 99, 99, 2, 99, 3, 4, 70, 80, 0, 1]], np.uint8)
    cov = np.array([[1, 0, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1],
                    [0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 1, 1]], np.uint8)
    out, out_cov = ref.halve(img, cov)
    # 7/1 = 7; 3/2 = 1.5 -> 2; 4/3 = 1.33 -> 1; 10/4 = 2.5 -> 3; nothing covered -> 0; 1/4 = 0.25 -> 0
    np.testing.assert_array_equal(out, np.array([[7, 2, 1, 3, 0, 0]], np.uint8))
    np.testing.assert_array_equal(out_cov, np.array([[1, 1, 1, 1, 0, 1]], np.uint8))
    rgb = np.stack([img, img // 2, 255 - img], -1)
    out3, _ = ref.halve(rgb, cov)
    assert out3.shape == (1, 6, 3)
    np.testing.assert_array_equal(out3[..., 0], out)
    assert tuple(out3[0, 2]) == (1, 0, 254)               # (0+0+1)/3 = 0.33 -> 0; (254+254+253)/3 = 253.67 -> 254


def test_erode_keeps_the_image_edges():
    cov = np.ones((5, 6), np.uint8)
    np.testing.assert_array_equal(ref.erode(cov, 4), cov)        # neighbours outside the image count as covered
    cov[2, 3] = 0
    want1 = np.ones((5, 6), np.uint8)
    want1[2, 2:5] = 0
    want1[1, 3] = want1[3, 3] = 0
    np.testing.assert_array_equal(ref.erode(cov, 1), want1)
    np.testing.assert_array_equal(ref.erode(cov, 0), cov)
    np.testing.assert_array_equal(ref.erode(cov * 200, 0), cov)  # any non-zero value is "covered"; the output holds 0 / 1


def test_finish_levels_halve_the_unpadded_image():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    cov = (rng.uniform(size=(8, 8)) < 0.4).astype(np.uint8)
    out = ref.finish(img, cov, pad_radius=1, erode_rounds=0, sizes=(4, 2))
    assert sorted(out) == [2, 4, 8]
    h4, c4 = ref.halve(img, cov)
    h2, c2 = ref.halve(h4, c4)
    np.testing.assert_array_equal(out[8], ref.pad(img, cov, 1)[0])
    np.testing.assert_array_equal(out[4], ref.pad(h4, c4, 1)[0])
    np.testing.assert_array_equal(out[2], ref.pad(h2, c2, 1)[0])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_every_new_export_rejects_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, two, three, four = (C.c_void_p(64 * k) for k in (1, 2, 3, 4))    # never dereferenced by a call that is rejected

    def rejected(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    cov = lib.t4d_texture_coverage
    rejected(cov(None, 8, 8, two, None))
    rejected(cov(one, 8, 8, None, None))
    rejected(cov(one, 0, 8, two, None))
    rejected(cov(one, 8, -1, two, None))
    q = lib.t4d_texture_quantize
    rejected(q(None, 8, 8, 3, two, None))
    rejected(q(one, 8, 8, 3, None, None))
    rejected(q(one, 0, 8, 3, two, None))
    rejected(q(one, 8, 0, 3, two, None))
    rejected(q(one, 8, 8, 2, two, None))
    er = lib.t4d_texture_erode
    rejected(er(None, 8, 8, 1, two, None))
    rejected(er(one, 8, 8, 1, None, None))
    rejected(er(one, 8, 8, 1, one, None))                 # in place
    rejected(er(one, -3, 8, 1, two, None))
    rejected(er(one, 8, 0, 1, two, None))
    rejected(er(one, 8, 8, 5, two, None))
    rejected(er(one, 8, 8, -1, two, None))
    assert lib.t4d_texture_pad_scratch_bytes(0, 8) == 0 and lib.t4d_last_error()
    assert lib.t4d_texture_pad_scratch_bytes(8, -2) == 0
    sb = lib.t4d_texture_pad_scratch_bytes(67, 93)
    assert sb >= 67 * 93
    pad = lib.t4d_texture_pad
    scratch = C.c_void_p(64 * 5)
    for k in range(5):                                    # each of the five buffers NULL in turn
        bufs = [one, two, three, four, scratch]
        bufs[k] = None
        rejected(pad(bufs[0], bufs[1], 67, 93, 3, 4, bufs[2], bufs[3], bufs[4], sb, None))
    rejected(pad(one, two, 67, 93, 3, 4, one, four, scratch, sb, None))      # image in place
    rejected(pad(one, two, 67, 93, 3, 4, three, two, scratch, sb, None))     # coverage in place
    rejected(pad(one, two, 0, 93, 3, 4, three, four, scratch, sb, None))
    rejected(pad(one, two, 67, 0, 3, 4, three, four, scratch, sb, None))
    rejected(pad(one, two, 67, 93, 2, 4, three, four, scratch, sb, None))
    rejected(pad(one, two, 67, 93, 3, 65, three, four, scratch, sb, None))
    rejected(pad(one, two, 67, 93, 3, -1, three, four, scratch, sb, None))
    rejected(pad(one, two, 67, 93, 3, 4, three, four, scratch, sb - 1, None), SIZE)
    hv = lib.t4d_texture_halve
    for k in range(4):
        bufs = [one, two, three, four]
        bufs[k] = None
        rejected(hv(bufs[0], bufs[1], 8, 8, 3, bufs[2], bufs[3], None))
    rejected(hv(one, two, 0, 8, 3, three, four, None))
    rejected(hv(one, two, 8, -8, 3, three, four, None))
    rejected(hv(one, two, 8, 8, 2, three, four, None))
    rejected(hv(one, two, 7, 8, 3, three, four, None))
    rejected(hv(one, two, 8, 9, 3, three, four, None))


# ---- the Python surface ----------------------------------------------------------------------------------------------------
def test_finish_refuses_a_size_that_is_not_a_power_of_two_fraction():
    from topo4d_amd import texfinish
    img, cov = torch.zeros(64, 64, 3, dtype=torch.uint8), torch.ones(64, 64, dtype=torch.uint8)
    for sizes in ((48,), (32, 20), (128,), (0,), (-32,), (3,)):
        with pytest.raises(ValueError, match="2\\^k"):
            texfinish.finish(img, cov, pad=2, sizes=sizes)
    with pytest.raises(ValueError, match="2\\^k"):                       # 16 = 64 / 4, but 66 columns do not divide by 4
        texfinish.finish(torch.zeros(64, 66, 3, dtype=torch.uint8), torch.ones(64, 66, dtype=torch.uint8), sizes=(16,))
    with pytest.raises(ValueError):
        texfinish.finish(img, cov, pad=65)
    with pytest.raises(ValueError):
        texfinish.finish(img, cov, erode=5)
    with pytest.raises(RuntimeError, match="no CPU path"):               # good arguments: only then is the device missed
        texfinish.finish(img, cov, pad=2, sizes=(32, 16))
    texfinish.check_options(2, 1, (32, 64, 1), 64)
    with pytest.raises(ValueError):
        texfinish.check_options(2, 1, (48,), 64)


def test_wrapper_argument_errors_without_a_device():
    from topo4d_amd import texfinish, texture
    u8, cov = torch.zeros(4, 4, 3, dtype=torch.uint8), torch.ones(4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError):
        texfinish.pad(u8, cov, 65)
    with pytest.raises(ValueError):
        texfinish.pad(u8, cov, -1)
    with pytest.raises(ValueError):
        texfinish.erode(cov, 5)
    with pytest.raises(ValueError):
        texfinish.pad(torch.zeros(4, 4, 2, dtype=torch.uint8), cov, 1)
    with pytest.raises(ValueError):
        texfinish.pad(u8.float(), cov, 1)
    with pytest.raises(ValueError):
        texfinish.quantize(u8)
    with pytest.raises(ValueError):
        texfinish.coverage_from_depth(torch.zeros(4, 4, 1))
    for call in (lambda: texfinish.pad(u8, cov, 1), lambda: texfinish.halve(u8, cov), lambda: texfinish.erode(cov, 1),
                 lambda: texfinish.quantize(u8.float()), lambda: texfinish.coverage_from_depth(torch.zeros(4, 4))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    uvs, colors, faces = np.zeros((3, 2)), np.zeros((3, 3), np.float32), np.array([[0, 1, 2]])
    with pytest.raises(ValueError, match="2\\^k"):                       # write_texture checks the options before it bakes
        texture.write_texture("unused.png", uvs, colors, faces, res=64, encoder="gpu", pad=2, sizes=(48,))
    with pytest.raises(ValueError):
        texture.write_texture("unused.png", uvs, colors, faces, res=64, encoder="gpu", pad=65)
    assert texfinish.level_path("a/b/face.png", 2048) == "a/b/face_2048.png"


def test_texfinish_parser_defaults():
    from topo4d_amd import texfinish
    p = texfinish.build_parser()
    a = p.parse_args(["-e", "exp", "-s", "seq", "--pad", "8"])
    assert (a.exp, a.seq, a.pad, a.erode, a.sizes, a.in_place, a.frames) == ("exp", "seq", 8, 1, [], False, None)
    assert a.output_dir == '/data/Topo4D/Topo4D_results'
    b = p.parse_args(["--pad", "4", "--erode", "0", "--sizes", "2048,1024", "--in_place", "--frames", "2-4"])
    assert (b.pad, b.erode, b.sizes, b.in_place, b.frames) == (4, 0, [2048, 1024], True, [2, 3, 4])
    with pytest.raises(SystemExit):
        p.parse_args(["-e", "exp"])                                      # --pad is required
    with pytest.raises(SystemExit):
        p.parse_args(["--pad", "4", "--sizes", "2048,x"])


def test_train_and_evaluate_namespaces_without_the_new_flags():
    from topo4d_amd import evaluate, train
    a = train.build_parser().parse_args([])
    assert not hasattr(a, "tex_pad") and not hasattr(a, "tex_sizes")
    b = train.build_parser().parse_args(["--tex_pad", "16", "--tex_sizes", "4096,2048"])
    assert b.tex_pad == 16 and b.tex_sizes == [4096, 2048]
    e = evaluate.build_parser().parse_args([])
    assert e.tex_pad is None and e.tex_erode == 1
    e = evaluate.build_parser().parse_args(["--tex_pad", "2", "--tex_erode", "0"])
    assert (e.tex_pad, e.tex_erode) == (2, 0)
