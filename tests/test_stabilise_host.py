"""CPU: the stabilisation rule as tests/stabilise_ref.py restates it, on fields whose answer is known by hand (the first four
tests check that restatement, which the GPU tests compare the kernels with, and run no product code); every argument
error of topo4d_amd.drift.dense_flow, warp and correct_vertices and of the two C entry points; the parser and the options of
drift.json with and without --stabilise.  Nothing here needs a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import stabilise_ref as sref


def test_a_constant_displacement_spreads_unchanged():
    """(A hand check of the restatement tests/stabilise_ref.py alone: it runs no product code.)  Every node holds d = (1.5, -0.25) at level 1: q = (768, -128), and a weighted mean of equal values is that value, on every
    texel within reach of a node; the nodes are at doubled indices 15, 47, 79, 111 and T = 32, so the first and the last texel
    (doubled 0 and 126) are 15 away from one and are supported"""
    H = W = 64
    labels = np.ones((H, W), np.uint8)
    d = np.zeros((4, 4, 2))
    d[..., 0], d[..., 1] = 1.5, -0.25
    flow, support = sref.dense_flow(d, np.ones((4, 4), bool), labels, 8, 8, 1)
    assert flow.dtype == np.int32 and support.dtype == np.uint8 and support.all()
    assert (flow[..., 0] == 768).all() and (flow[..., 1] == -128).all()


def test_bilinear_weights_by_hand():
    """(A hand check of the restatement alone: it runs no product code.)  B = S = 8, L = 0: nodes at doubled indices 7 and 23 (between texels 3|4 and 11|12), T = 16.  Texel 5 (doubled 10) weighs
    them 16 - 3 = 13 and 16 - 13 = 3: with q = 0 and 256 that is (2 * 3 * 256 + 16) // 32 = 48, and texel 4 weighs them 15 and 1;
    rows likewise, and a node that is not kept leaves the rest renormalised"""
    labels = np.ones((16, 16), np.uint8)
    d = np.zeros((2, 2, 2))
    d[:, 1, 1] = 1.0                                            # dx = 1 texel on the right-hand nodes
    kept = np.ones((2, 2), bool)
    flow, support = sref.dense_flow(d, kept, labels, 8, 8, 0)
    assert support.all() and (flow[..., 0] == 0).all()
    assert flow[5, 5, 1] == 48 and flow[0, 5, 1] == 48 and flow[5, 4, 1] == (2 * 256 + 16) // 32 and flow[5, 12, 1] == 256
    assert flow[5, 0, 1] == 0                                   # left of the first node only that node is within reach
    kept[0, 1] = False
    flow, support = sref.dense_flow(d, kept, labels, 8, 8, 0)
    wy0, wy1 = 16 - 3, 16 - 13                                  # texel row 5
    den = wy0 * 13 + wy1 * 13 + wy1 * 3
    assert flow[5, 5, 1] == (2 * wy1 * 3 * 256 + den) // (2 * den)
    assert flow[0, 15, 1] == 0 and support[0, 15] == 0          # row 0 reaches only the upper nodes, column 15 only the right-hand ones
    assert support[0, 5] == 1 and flow[0, 5, 1] == 0
    # a negative value rounds half up like a positive one: floor((2 num + den) / (2 den))
    d[...] = 0.0
    d[0, 0, 0] = -1.0 / 256                                     # q = -1 on one node
    flow, _ = sref.dense_flow(d, np.ones((2, 2), bool), labels, 8, 8, 0)
    assert flow[3, 3, 0] == -1                                  # texel 3 is within reach of that node alone
    assert flow[7, 7, 0] == 0                                   # weights 9 and 7 per axis: -81/256 = -0.32 -> 0
    assert flow[5, 5, 0] == (2 * -(13 * 13) + 256) // 512 == -1     # 13 and 3 per axis: -169/256 = -0.66 -> -1


def test_labels_restrict_nodes_and_texels():
    """(A hand check of the restatement alone: it runs no product code.)  Two islands, a texel without one, no node kept, no block."""
    labels = np.ones((16, 16), np.uint8)
    labels[:, 8:] = 2
    labels[0, 0] = 0
    d = np.zeros((2, 2, 2))
    d[:, 0, 0], d[:, 1, 0] = 1.0, -1.0                          # the nodes' label texels are (4, 4), (4, 12), ...: labels 1 and 2
    flow, support = sref.dense_flow(d, np.ones((2, 2), bool), labels, 8, 8, 0)
    assert (flow[:, :8, 0][labels[:, :8] == 1] == 256).all() and (flow[:, 8:, 0] == -256).all()
    assert support[0, 0] == 0 and flow[0, 0, 0] == 0 and support.sum() == 255
    flow, support = sref.dense_flow(d, np.zeros((2, 2), bool), labels, 8, 8, 0)
    assert not flow.any() and not support.any()
    flow, support = sref.dense_flow(np.zeros((0, 2, 2)), np.zeros((0, 2), bool), labels[:7], 8, 8, 0)
    assert flow.shape == (7, 16, 2) and not flow.any() and not support.any()


def test_warp_by_hand():
    """(A hand check of the restatement alone: it runs no product code.)  Whole-texel and quarter-texel flows, taps dropped outside
    the image, across an island border and on an invalid texel."""
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    ones = np.ones((6, 7), np.uint8)
    flow = np.zeros((6, 7, 2), np.int32)
    out, valid = sref.warp(img, ones, ones, flow)
    assert np.array_equal(out, img) and valid.all()
    flow[..., 0], flow[..., 1] = 256, -512                      # whole texels: out(y, x) = img(y + 1, x - 2)
    out, valid = sref.warp(img, ones, ones, flow)
    assert np.array_equal(out[:5, 2:], img[1:, :5]) and valid[:5, 2:].all()
    assert not valid[5].any() and not valid[:, :2].any() and not out[5].any()
    flow[...] = 0
    flow[..., 1] = 64                                           # a quarter texel: (3 a + b + 2) >> 2 per channel
    out, valid = sref.warp(img, ones, ones, flow)
    a, b = img[:, :-1].astype(int), img[:, 1:].astype(int)
    assert np.array_equal(out[:, :-1], (2 * (192 * 256 * a + 64 * 256 * b) + 65536) // (2 * 65536))
    assert np.array_equal(out[:, -1], img[:, -1]) and valid.all()   # the tap outside is dropped: the one left is renormalised
    labels = ones.copy()
    labels[:, 4:] = 2
    out, valid = sref.warp(img, ones, labels, flow)
    assert np.array_equal(out[:, 3], img[:, 3])                 # the tap across the island border is dropped
    hole = ones.copy()
    hole[2, 2] = 0
    out, valid = sref.warp(img[..., 0], hole, ones, flow)
    assert out.shape == (6, 7) and np.array_equal(out[2, 1], img[2, 1, 0]) and out[2, 2] == img[2, 3, 0] and valid.all()
    labels[3, 3] = 0
    assert sref.warp(img, ones, labels, flow)[1][3, 3] == 0


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_bad_arguments_without_a_device():
    from topo4d_amd import drift
    labels = torch.ones(64, 96, dtype=torch.uint8)
    d, kept = torch.zeros(3, 5, 2, dtype=torch.float64), torch.ones(3, 5, dtype=torch.bool)       # 32 x 48 at level 1, B 16, S 8
    ok = dict(block=16, stride=8, level=1, reach=1)
    for change in (dict(block=15), dict(stride=17), dict(level=9), dict(level=-1), dict(level=6), dict(reach=0), dict(reach=5),
                   dict(block=8, stride=4)):
        with pytest.raises(ValueError):
            drift.dense_flow(d, kept, labels, **{**ok, **change})
    for bad_d in (d.float(), d[:2], d[..., :1]):
        with pytest.raises(ValueError, match="d must be"):
            drift.dense_flow(bad_d, kept, labels, **ok)
    with pytest.raises(ValueError, match="kept"):
        drift.dense_flow(d, kept[:2], labels, **ok)
    with pytest.raises(ValueError, match="labels"):
        drift.dense_flow(d, kept, labels.bool(), **ok)
    for value in (float("nan"), float("inf"), 2.0 ** 22 / 512 + 1):
        with pytest.raises(ValueError, match="finite"):
            drift.dense_flow(torch.full_like(d, value), kept, labels, **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):     # everything right but the device
        drift.dense_flow(d, kept, labels, **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):     # check=False: the values are not read
        drift.dense_flow(torch.full_like(d, float("nan")), kept, labels, **ok, check=False)
    big = torch.ones(48 << 7, 48 << 7, dtype=torch.uint8)      # one block of 48 at level 7: a tent of 4 * 2 * 48 * 128 = 49152 > 46340
    with pytest.raises(ValueError, match="46340"):
        drift.dense_flow(torch.zeros(1, 1, 2, dtype=torch.float64), torch.ones(1, 1, dtype=torch.bool), big, 48, 48, 7, reach=4)
    with pytest.raises(RuntimeError, match="no CPU path"):     # reach 3: 36864, within the bound
        drift.dense_flow(torch.zeros(1, 1, 2, dtype=torch.float64), torch.ones(1, 1, dtype=torch.bool), big, 48, 48, 7, reach=3)
    assert drift.node_values(torch.tensor([[[0.5 / 512, 1.5 / 512]]], dtype=torch.float64), 1).tolist() == [[[0, 2]]]   # half to even

    img, m = torch.zeros(64, 96, 3, dtype=torch.uint8), torch.ones(64, 96, dtype=torch.uint8)
    flow = torch.zeros(64, 96, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="image"):
        drift.warp(img.float(), m, labels, flow)
    with pytest.raises(ValueError, match="image"):
        drift.warp(img[..., :2], m, labels, flow)
    with pytest.raises(ValueError, match="valid"):
        drift.warp(img, m[:10], labels, flow)
    with pytest.raises(ValueError, match="labels"):
        drift.warp(img, m, labels.bool(), flow)
    for bad in (flow.long(), flow[:10], flow[..., :1]):
        with pytest.raises(ValueError, match="flow"):
            drift.warp(img, m, labels, bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        drift.warp(img, m, labels, flow)

    from tests import projtex_scenes as scenes
    obj, verts = scenes.patch_scene()
    with pytest.raises(ValueError, match="flow"):
        drift.correct_vertices(obj, verts, flow[:10], m, labels)
    with pytest.raises(ValueError, match="support"):
        drift.correct_vertices(obj, verts, flow, m.float(), labels)
    with pytest.raises(ValueError, match="vertices"):
        drift.correct_vertices(obj, verts[:, :2], flow, m, labels)
    with pytest.raises(ValueError, match="faces name vertex"):
        drift.correct_vertices(obj, verts[:10], flow, m, labels)
    with pytest.raises(RuntimeError, match="no CPU path"):
        drift.correct_vertices(obj, verts, flow, m, labels)
    with pytest.raises(ValueError, match="reach"):
        drift.stabilise_pair(obj, img, m, obj, img, m, reach=7)


def test_sample_positions_on_the_cpu_equals_the_restatement():
    """the vertex rule's sampling is plain torch and runs on CPU tensors too: the same float64 values as the restatement, on
    positions inside, on the rim, outside and across an island border"""
    from topo4d_amd import drift
    rng = np.random.default_rng(1)
    pos = rng.standard_normal((9, 11, 3)).astype(np.float32)
    labels = np.ones((9, 11), np.uint8)
    labels[:, 6:] = 2
    labels[0, 0] = 0
    py = np.array([0.0, 3.25, 8.0, 8.5, -0.5, 4.75, 4.75, 2.0, -3.0])
    px = np.array([0.0, 4.5, 10.0, 2.0, 3.0, 5.5, 5.5, 10.75, 2.0])
    label = np.array([1, 1, 2, 1, 1, 1, 2, 2, 1], np.uint8)
    want, ok = sref.sample_positions(pos, labels, py, px, label)
    got, ok_t = drift.sample_positions(torch.from_numpy(pos), torch.from_numpy(labels), torch.from_numpy(py), torch.from_numpy(px),
                                       torch.from_numpy(label))
    assert np.array_equal(got.numpy(), want) and np.array_equal(ok_t.numpy(), ok)
    assert ok.tolist() == [False, True, True, True, True, True, True, True, False]
    assert np.array_equal(want[2], pos[8, 10].astype(np.float64)) and np.array_equal(want[5], 0.25 * pos[4, 5].astype(np.float64) + 0.75 * pos[5, 5].astype(np.float64))


def test_the_c_entry_points_refuse_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    ARG = _lib.T4D_ERR_ARG
    one, none = C.c_void_p(64), None                           # "some address": never dereferenced by a call that is refused

    def refused(rc):
        assert rc == ARG, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    good = (64, 96, 16, 8, 1, 1)
    for shape in ((0, 96, 16, 8, 1, 1), (64, 0, 16, 8, 1, 1), (65537, 96, 16, 8, 1, 1), (64, 96, 15, 8, 1, 1), (64, 96, 6, 3, 1, 1),
                  (64, 96, 66, 8, 1, 1), (64, 96, 16, 0, 1, 1), (64, 96, 16, 17, 1, 1), (64, 96, 16, 8, -1, 1), (64, 96, 16, 8, 9, 1),
                  (64, 96, 16, 8, 1, 0), (64, 96, 16, 8, 1, 5), (63, 96, 16, 8, 1, 1), (64, 96, 16, 8, 6, 1)):
        refused(lib.t4d_drift_dense(one, one, one, *shape, one, one, none))
    for k in (0, 1, 2, 9, 10):
        args = [one, one, one, *good, one, one]
        args[k] = none
        refused(lib.t4d_drift_dense(*args, none))
    refused(lib.t4d_drift_dense(one, one, one, *good, C.c_void_p(68), one, none))       # a misaligned flow
    refused(lib.t4d_drift_dense(one, one, one, 6144, 6144, 48, 48, 7, 4, one, one, none))     # a tent of 49152 > 46340
    assert b"46340" in lib.t4d_last_error()
    refused(lib.t4d_drift_dense(C.c_void_p(66), one, one, *good, one, one, none))
    for shape in ((0, 96, 3), (64, 0, 3), (64, 65537, 3), (64, 96, 2), (64, 96, 0), (64, 96, 5)):
        refused(lib.t4d_drift_warp(one, one, one, one, *shape, C.c_void_p(128), C.c_void_p(192), none))
    for k in (0, 1, 2, 3, 7, 8):
        args = [one, one, one, one, 64, 96, 3, C.c_void_p(128), C.c_void_p(192)]
        args[k] = none
        refused(lib.t4d_drift_warp(*args, none))
    refused(lib.t4d_drift_warp(one, one, one, C.c_void_p(68), 64, 96, 3, C.c_void_p(128), C.c_void_p(192), none))
    refused(lib.t4d_drift_warp(one, one, one, one, 64, 96, 3, C.c_void_p(130), C.c_void_p(192), none))
    refused(lib.t4d_drift_warp(one, one, one, one, 64, 96, 3, C.c_void_p(128), C.c_void_p(193), none))
    refused(lib.t4d_drift_warp(one, one, one, C.c_void_p(256), 64, 96, 3, one, C.c_void_p(192), none))     # out_image is image


# ---- command line ------------------------------------------------------------------------------------------------------------
BASE = ["-e", "exp", "-s", "seq", "-od", "out"]
PLAIN = dict(texture="face_proj.png", ref="first", level=2, block=32, stride=16, radius=8, ratio=0.8, unit=1000.0, min_count=512)


def test_the_parser_and_the_options():
    from topo4d_amd import drift, evaluate
    p = drift.build_parser()
    a = p.parse_args(BASE)
    assert (a.stabilise, a.reach, a.correct_obj) == (False, 1, False)
    assert drift.options_of(a) == {**{k: v for k, v in PLAIN.items() if k != "min_count"}, "stride": None}   # as before the flags
    o, checked = drift.tree_options(a)
    assert o == PLAIN and list(o) == list(PLAIN) and checked == (32, 16, 8, 512)     # no new key, and the keys in their order
    a = p.parse_args(BASE + ["--stabilise", "--reach", "3", "--correct_obj", "--save_fields"])
    assert (a.stabilise, a.reach, a.correct_obj, a.save_fields) == (True, 3, True, True)
    o, _ = drift.tree_options(a)
    assert o == {**PLAIN, "stabilise": True, "reach": 3}
    assert drift.tree_options(p.parse_args(BASE + ["--stabilise"]))[0]["reach"] == 1
    for reach in ("2", "5"):                                    # without --stabilise it says nothing, whatever its value
        assert drift.tree_options(p.parse_args(BASE + ["--reach", reach]))[0] == PLAIN
    with pytest.raises(SystemExit, match="46340"):
        drift.tree_options(p.parse_args(BASE + ["--stabilise", "--level", "7", "--block", "48", "--stride", "48", "--reach", "4"]))
    with pytest.raises(SystemExit, match="--ref first"):
        drift.tree_options(p.parse_args(BASE + ["--stabilise", "--ref", "previous"]))
    for reach in ("0", "5"):
        with pytest.raises(SystemExit, match="reach"):
            drift.tree_options(p.parse_args(BASE + ["--stabilise", "--reach", reach]))
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ["--reach", "two"])
    assert drift.stab_names("face_proj.png") == ("face_proj_stab.png", "face_proj_stab_weight.png")
    assert drift.stab_names("face.png") == ("face_stab.png", "face_stab_weight.png")
    # evaluate has the matcher's flags and none of these
    e = evaluate.build_parser().parse_args(["-e", "e", "-s", "s", "--drift"])
    assert not any(hasattr(e, k) for k in ("stabilise", "drift_stabilise", "reach", "drift_reach", "correct_obj"))
    assert drift.tree_options(e, drift.options_of(e, "drift_"))[0] == PLAIN
    with pytest.raises(SystemExit):
        evaluate.build_parser().parse_args(["-e", "e", "-s", "s", "--drift", "--stabilise"])
