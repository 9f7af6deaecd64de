"""CPU: the push-pull hole fill's rule (tests/texfill_ref.py, the yardstick of tests/test_gpu_texfill.py) checked against what the
rule promises, the UV islands of a face.obj, and every refusal of texfinish.fill / fill_islands, projtex.uv_islands, the two exports
and the command lines that needs no device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import projtex_scenes as S, texfill_ref as ref


def test_one_row_worked_by_hand():
    """[10, _, _, 200], 1x4, in units of 1/256: level 0 = [2560, _, _, 51200]; level 1 (1x2) = [2560, 51200], each the mean of its
    one valid child; level 2 (1x1) = (2 * 53760 + 2) / 4 = 26880.  Push to level 1: both valid, kept.  Push to level 0: texel 1 is
    odd, px = 0, nx = 1, and the level has one row, so ny = py = 0: (9 * 2560 + 3 * 51200 + 3 * 2560 + 51200 + 8) >> 4 = 14720,
    and (14720 + 128) >> 8 = 58.  Texel 2 is even, px = 1, nx = 0: (12 * 51200 + 4 * 2560 + 8) >> 4 = 39040 -> 153."""
    out, filled = ref.fill(np.array([[10, 0, 0, 200]], np.uint8), np.array([[1, 0, 0, 1]], np.uint8))
    assert out.tolist() == [[10, 58, 153, 200]] and filled.tolist() == [[0, 1, 1, 0]]
    assert (9 * 2560 + 3 * 51200 + 3 * 2560 + 51200 + 8) >> 4 == 14720 and (14720 + 128) >> 8 == 58
    assert (12 * 51200 + 4 * 2560 + 8) >> 4 == 39040 and (39040 + 128) >> 8 == 153


def test_four_by_four_worked_by_hand():
    """40 at (0,0) and 200 at (3,3).  Level 1 (2x2) = [[10240, _], [_, 51200]]; level 2 = (2 * 61440 + 2) / 4 = 30720 (120).  Push to
    level 1: the two holes take 30720 (every tap is the one texel).  Level 1 complete: [[40, 120], [120, 200]] * 256.  Push to
    level 0 weighs parent 9, the two neighbours 3 each, the diagonal 1; at (0,1): px = 0, nx = 1, py = 0, ny = clamp(-1) = 0:
    (12 * 40 + 4 * 120) / 16 = 60; at (1,1): (9 * 40 + 3 * 120 + 3 * 120 + 200) / 16 = 80; at (1,2): parent (0,1) = 120,
    nx = 0, ny = 1: (9 * 120 + 3 * 40 + 3 * 200 + 120) / 16 = 120; and so on by symmetry."""
    img, valid = np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8)
    img[0, 0], img[3, 3] = 40, 200
    valid[0, 0] = valid[3, 3] = 1
    out, filled = ref.fill(img, valid)
    assert out.tolist() == [[40, 60, 100, 120], [60, 80, 120, 140], [100, 120, 160, 180], [120, 140, 180, 200]]
    assert np.array_equal(filled, 1 - valid)


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (5, 3), (37, 53), (64, 64), (70, 130)])
def test_what_the_rule_promises(shape):
    rng = np.random.default_rng(sum(shape))
    for c in (1, 3, 4):
        for share in (0.02, 0.5, 0.97):
            img = rng.integers(0, 256, size=shape + (c,), dtype=np.uint8)
            valid = (rng.random(shape) < share).astype(np.uint8) * rng.integers(1, 256, size=shape).astype(np.uint8)
            domain = (rng.random(shape) < 0.6).astype(np.uint8)
            for dom in (None, domain):
                out, filled = ref.fill(img, valid, dom)
                assert out.shape == img.shape and out.dtype == np.uint8 and filled.shape == shape and filled.dtype == np.uint8
                take = (valid == 0) & (True if dom is None else dom != 0)
                if not valid.any():                                  # no valid texel: the input back, nothing filled
                    assert np.array_equal(out, img) and not filled.any()
                    continue
                assert np.array_equal(filled, take.astype(np.uint8))
                assert np.array_equal(out[~take], img[~take])        # valid texels and texels outside the domain never change
                lo, hi = img[valid != 0].min(0), img[valid != 0].max(0)
                assert (out[take] >= lo).all() and (out[take] <= hi).all()
            # a constant image stays constant exactly, whatever is valid
            flat = np.broadcast_to(rng.integers(0, 256, size=c, dtype=np.uint8), shape + (c,)).copy()
            out, _ = ref.fill(flat, valid)
            assert np.array_equal(out, flat) or not valid.any()
    out, filled = ref.fill(np.full(shape, 7, np.uint8), np.zeros(shape, np.uint8))
    assert (out == 7).all() and not filled.any() and out.shape == shape


@pytest.mark.parametrize("w", [33, 64, 97, 200])
@pytest.mark.parametrize("a,b", [(10, 200), (0, 255), (100, 101)])
def test_a_two_sided_ramp_fills_without_a_dip(w, a, b):
    img, valid = np.zeros((40, w), np.uint8), np.zeros((40, w), np.uint8)
    img[:, :5], img[:, -7:], valid[:, :5], valid[:, -7:] = a, b, 1, 1
    out, filled = ref.fill(img, valid)
    assert (np.diff(out.astype(np.int64), axis=1) >= 0).all()
    assert out.min() == a and out.max() == b and filled.sum() == 40 * (w - 12)


def _disc(r):
    y, x = np.mgrid[0:256, 0:256]
    return (x - 128) ** 2 + (y - 128) ** 2 <= r * r


@pytest.mark.parametrize("r,fill_err,nearest_err", [(8, 2, 10), (20, 8, 30)])
def test_a_hole_in_a_smooth_texture_fills_better_than_from_the_nearest_texel(r, fill_err, nearest_err):
    tex = (S.smooth_texture(256, 256) * 255).astype(np.uint8)
    hole = _disc(r)
    out, filled = ref.fill(np.where(hole[..., None], 0, tex).astype(np.uint8), ~hole)
    near = ref.nearest_fill(tex, ~hole)
    err = np.abs(out.astype(np.int64) - tex)[hole].max()
    err_near = np.abs(near.astype(np.int64) - tex)[hole].max()
    print("radius", r, "push-pull", err, "nearest texel", err_near)
    assert np.array_equal(filled != 0, hole)
    assert err < err_near
    assert (err, err_near) == (fill_err, nearest_err)                # the figures this rule gives on the CPU


def test_fill_islands_keeps_the_islands_apart():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(40, 60, 3), dtype=np.uint8)
    labels = np.zeros((40, 60), np.uint8)
    labels[2:20, 3:30], labels[22:38, 5:25], labels[5:35, 35:55] = 1, 2, 3
    img[labels == 1], img[labels == 3] = 50, 220
    valid = np.ones((40, 60), np.uint8)
    valid[8:12, 10:20] = 0                                           # a hole in island 1
    valid[labels == 2] = 0                                           # island 2: never seen
    valid[10:30, 40:42] = 0                                          # a hole in island 3
    valid[0, 0] = 0                                                  # outside every island
    out, filled = ref.fill_islands(img, valid, labels)
    assert np.array_equal(filled != 0, (valid == 0) & ((labels == 1) | (labels == 3)))
    assert (out[(filled != 0) & (labels == 1)] == 50).all() and (out[(filled != 0) & (labels == 3)] == 220).all()
    assert np.array_equal(out[filled == 0], img[filled == 0])


# ---- the islands of a face.obj -------------------------------------------------------------------------------------------------
def test_uv_islands_of_three_quads():
    from topo4d_amd import projtex
    obj = S.three_quads()
    ids = projtex.uv_islands(obj)
    assert ids.tolist() == [1] * 4 + [2] * 4 + [3] * 4
    # numbered by the lowest face index, not by the UV vertex index; an unused UV vertex belongs to no island
    from topo4d_amd.meshrender import FaceObj
    uvs = np.concatenate([obj.uvs, [[0.5, 0.5]]])
    turned = FaceObj(obj.vertices, uvs, obj.faces_ori[::-1], obj.uv_faces_ori[::-1])
    assert projtex.uv_islands(turned).tolist() == [3] * 4 + [2] * 4 + [1] * 4 + [0]
    # two quads that share an edge in UV space are one island
    shared = FaceObj(obj.vertices, obj.uvs, obj.faces_ori, [[0, 1, 2, 3], [3, 2, 5, 6], [8, 9, 10, 11]])
    assert projtex.uv_islands(shared).tolist() == [1, 1, 1, 1, 0, 1, 1, 0, 2, 2, 2, 2]


def test_uv_islands_refuses_what_it_cannot_label():
    from topo4d_amd import projtex
    from topo4d_amd.meshrender import FaceObj
    n = 256
    verts = np.zeros((3 * n, 3))
    uvs = np.zeros((3 * n, 2))
    tris = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(n)]
    with pytest.raises(ValueError, match="256 islands"):
        projtex.uv_islands(FaceObj(verts, uvs, tris, [list(t) for t in tris]))
    assert projtex.uv_islands(FaceObj(verts[:-3], uvs[:-3], tris[:-1], [list(t) for t in tris[:-1]])).max() == 255
    with pytest.raises(ValueError):                                  # a UV face that names a UV vertex the mesh has not
        projtex.uv_islands(FaceObj(verts[:3], uvs[:3], tris[:1], [[0, 1, 3]]))
    with pytest.raises(ValueError):                                  # a pentagon
        projtex.uv_islands(FaceObj(verts[:5], uvs[:5], [[0, 1, 2, 3, 4]], [[0, 1, 2, 3, 4]]))
    with pytest.raises(ValueError):                                  # (with or without a device)
        projtex.island_labels(FaceObj(verts, uvs, tris, [list(t) for t in tris]), 16, 16)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_fill_and_fill_islands_check_their_arguments_before_they_need_a_device():
    from topo4d_amd import texfinish
    img, valid = torch.zeros(8, 9, 3, dtype=torch.uint8), torch.ones(8, 9, dtype=torch.uint8)
    labels = torch.ones(8, 9, dtype=torch.uint8)
    bad = [dict(image=img.float()), dict(image=torch.zeros(8, 9, 2, dtype=torch.uint8)), dict(image=img.numpy()),
           dict(valid=valid[:7]), dict(valid=valid.float()), dict(valid=None), dict(domain=valid[:, :8]), dict(domain=valid.to(torch.int32))]
    for kw in bad:
        with pytest.raises(ValueError):
            texfinish.fill(**{**dict(image=img, valid=valid, domain=None), **kw})
    for kw in bad[:6] + [dict(labels=labels[:7]), dict(labels=labels.bool()), dict(labels=labels.to(torch.int64)), dict(labels=None)]:
        with pytest.raises(ValueError):
            texfinish.fill_islands(**{**dict(image=img, valid=valid, labels=labels), **kw})
    with pytest.raises(RuntimeError, match="no CPU path"):           # well-formed, but on the host
        texfinish.fill(img, valid)
    with pytest.raises(RuntimeError, match="no CPU path"):
        texfinish.fill(img, valid.bool(), valid)
    with pytest.raises(RuntimeError, match="no CPU path"):
        texfinish.fill_islands(img[..., 0], valid, labels)


def test_the_exports_refuse_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, two, three, four, five = (C.c_void_p(64 * k) for k in range(1, 6))   # "some addresses": a refused call reads none of them

    def rejected(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()                                  # every refusal leaves a message

    nb = lib.t4d_texture_fill_scratch_bytes(100, 70, 3)
    # the levels 50x35 ... 1x1 of 16-bit colours, each rounded up to 256 bytes, and never 0
    dims = [(50, 35), (25, 18), (13, 9), (7, 5), (4, 3), (2, 2), (1, 1)]
    assert nb >= sum(h * w * 3 * 2 for h, w in dims) and nb <= sum(h * w * 3 * 2 + 256 for h, w in dims) + 256
    assert lib.t4d_texture_fill_scratch_bytes(1, 1, 1) > 0
    for h, w, c in ((0, 70, 3), (100, 0, 3), (100, 70, 2), (65537, 70, 3), (100, 65537, 1), (-1, 4, 4)):
        assert lib.t4d_texture_fill_scratch_bytes(h, w, c) == 0
        assert lib.t4d_last_error()
        rejected(lib.t4d_texture_fill(one, two, None, h, w, c, three, four, five, 1 << 40, None))
    fill = lambda *a, nbytes=nb: lib.t4d_texture_fill(*a[:3], 100, 70, 3, *a[3:], nbytes, None)
    rejected(fill(None, two, None, three, four, five))
    rejected(fill(one, None, None, three, four, five))
    rejected(fill(one, two, None, None, four, five))
    rejected(fill(one, two, None, three, None, five))
    rejected(fill(one, two, None, three, four, None))
    rejected(fill(one, two, None, one, four, five))                  # inputs and outputs are separate buffers
    rejected(fill(one, two, None, three, two, five))
    rejected(fill(one, two, four, three, four, five))
    rejected(fill(one, two, None, three, four, five, nbytes=nb - 1), SIZE)
    rejected(fill(one, two, three, four, five, one, nbytes=0), SIZE)


def test_the_flag_on_both_command_lines():
    from topo4d_amd import projtex, train
    assert projtex.build_parser().parse_args([]).tex_fill is False
    assert projtex.build_parser().parse_args(["--tex_fill"]).tex_fill is True
    assert not hasattr(train.build_parser().parse_args([]), "tex_fill")       # absent unless given, like the other added flags
    t = train.build_parser().parse_args(["--tex_project", "--tex_fill"])
    assert t.tex_project is True and t.tex_fill is True


def test_train_with_the_flag_needs_the_projection(tmp_path):
    from topo4d_amd import train
    argv = ["-e", "exp", "-s", "seq", "-id", str(tmp_path / "in"), "-did", str(tmp_path / "dense"), "-od", str(tmp_path / "out"),
            "--tex_fill"]
    with pytest.raises(SystemExit, match="--tex_project"):
        train.train(train.build_parser().parse_args(argv))
    assert not (tmp_path / "out").exists() or not any((tmp_path / "out").rglob("*.npz"))
