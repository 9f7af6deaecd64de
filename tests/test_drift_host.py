"""CPU: the drift matcher's rule as tests/drift_ref.py restates it, on textures whose answer is known; every argument error of
topo4d_amd.drift.match and of the C entry points; the parser; drift_stats on a hand-made field.

Figures of the restatement at 96 x 96, B = 16, S = 8, R = 4 on smooth_random(seed 1), printed by the tests: an integer shift is
found on every block at which it is admissible (120 of 121: at one corner block the shift leaves fewer than min_count pairs);
under a gain of 0.7 and noise of 0.01 likewise; a shift of (1.5, 0.25) is found within 0.23 texel on every kept block."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import drift_ref as ref

H = W = 96
B, S, R = 16, 8, 4
MIN = B * B // 2
ONES = np.ones((H, W), np.uint8)


@pytest.fixture(scope="module")
def field():
    return ref.smooth_random(H, W, 1)


def interior(nby, nbx, h=H, w=W):
    """blocks whose texels and search window keep the census margin of 3 from the image border"""
    y, x = np.arange(nby) * S, np.arange(nbx) * S
    oky, okx = (y >= R + 3) & (y + B + R + 3 <= h), (x >= R + 3) & (x + B + R + 3 <= w)
    return oky[:, None] & okx[None, :]


@pytest.mark.parametrize("d", [(2, -3), (0, 0), (-3, 1)])
def test_an_integer_roll_is_found_exactly(field, d):
    a = ref.to_u8(field)
    b = np.roll(a, d, (0, 1))                                   # b(p + d) = a(p)
    table = ref.match(a, ONES, b, ONES, ONES, B, S, R, MIN)
    assert table.shape == (11, 11, 16) and table.dtype == np.int32
    _, n = ref.costs(a, ONES, b, ONES, ONES, B, S, R)
    admissible = n[d[0] + R, d[1] + R] >= MIN                   # everywhere but where p + d leaves the image for too many texels
    inner = interior(11, 11)
    assert inner.sum() == 81 and admissible[inner].all()
    exact = (table[..., 0] == d[0]) & (table[..., 1] == d[1])
    print("exact blocks", int(exact.sum()), "admissible", int(admissible.sum()))
    assert exact[admissible].all()
    assert (table[..., 2][admissible] == 0).all()               # identical census words: c = 0 at exactly d
    assert (table[..., 3][inner] == B * B).all()
    _, kept = ref.flow(table, R)
    assert kept[admissible].all()
    dd, _ = ref.flow(table, R)
    assert np.abs(dd - table[..., :2]).max() <= 0.5             # the offset never leaves the best's texel
    assert sorted(np.unique(table[..., 14:]).tolist()) == [0]


def test_gain_and_noise_leave_the_integer_part(field):
    d = (2, -3)
    a = ref.to_u8(field)
    noise = np.random.default_rng(3).standard_normal((H, W))
    b = ref.to_u8(np.clip(0.7 * np.roll(field, d, (0, 1)) + 0.01 * noise, 0, 1))
    table = ref.match(a, ONES, b, ONES, ONES, B, S, R, MIN)
    _, n = ref.costs(a, ONES, b, ONES, ONES, B, S, R)
    admissible = n[d[0] + R, d[1] + R] >= MIN
    exact = (table[..., 0] == d[0]) & (table[..., 1] == d[1])
    _, kept = ref.flow(table, R)
    print("kept", int(kept.sum()), "exact", int(exact.sum()), "admissible", int(admissible.sum()))
    assert exact[admissible].all() and kept[admissible].all() and admissible.sum() >= 120


def test_a_sub_texel_shift(field):
    """Bound: a quarter texel, half of the 0.5 the integer part alone leaves at a shift of 1.5, so the test fails for an offset
    of the wrong size (halved, it leaves 0.33) as for none at all.  The parabola through three census costs is biased towards
    the integer: the cost is closer to a V than to a parabola, and for an exact V of slope 1 the estimate t / (2 (1 - |t|)) of an
    offset t is short by up to 0.09 (at |t| = 0.29); bilinear resampling and 8-bit rounding of the moved texture add the rest.
    The restatement's figure on this texture is 0.227 over 121 kept blocks.  The 0.21 that the issue quotes for a texture of
    its author's was not reproduced: smooth_random with 1 to 4 blur passes and seeds 0 to 2 gives 0.218 to 0.267."""
    shift = np.array([1.5, 0.25])
    a, b = ref.to_u8(field), ref.to_u8(ref.shift_periodic(field, *shift))
    table = ref.match(a, ONES, b, ONES, ONES, B, S, R, MIN)
    d, kept = ref.flow(table, R)
    err = np.abs(d - shift).max(-1)
    print("kept", int(kept.sum()), "largest error", err[kept].max())
    assert kept.sum() >= 100 and err[kept].max() < 0.25
    assert np.abs(d - table[..., :2]).max() <= 0.5
    from topo4d_amd import drift                                # the module's flow on the same table: float64 torch, CPU-capable
    d_t, kept_t = drift.flow(torch.from_numpy(table), R)
    assert np.array_equal(d_t.numpy(), d) and np.array_equal(kept_t.numpy(), kept)


def test_a_flat_image_is_kept_nowhere():
    flat = np.full((H, W), 90, np.uint8)
    table = ref.match(flat, ONES, flat, ONES, ONES, B, S, R, MIN)
    assert (table[..., 2] == 0).all() and (table[..., 12] == 0).all() and (table[..., 3] >= MIN).all()
    assert (table[..., :2] == 0).all()                          # every cost ties: the smallest dy^2 + dx^2 wins
    assert not ref.flow(table, R)[1].any()


def test_a_best_on_the_rim_is_dropped(field):
    a = ref.to_u8(field)
    for d in ((R, 0), (-1, -R), (R, R)):
        table = ref.match(a, ONES, np.roll(a, d, (0, 1)), ONES, ONES, B, S, R, MIN)
        found = (table[..., 0] == d[0]) & (table[..., 1] == d[1])
        assert found.sum() >= 49 and not ref.flow(table, R)[1][found].any()
        outside = {(-1, 0): 4, (1, 0): 6, (0, -1): 8, (0, 1): 10}   # the neighbour beyond the rim is (0, 0)
        for (ey, ex), k in outside.items():
            if abs(d[0] + ey) > R or abs(d[1] + ex) > R:
                assert (table[..., k:k + 2][found] == 0).all()
    shifted = ref.to_u8(ref.shift_periodic(field, 3.6, 0.0))    # beyond the last measurable sub-texel position
    table = ref.match(a, ONES, shifted, ONES, ONES, B, S, R, MIN)
    _, kept = ref.flow(table, R)
    assert not (kept & (np.abs(table[..., :2]).max(-1) >= R)).any()
    print("kept at a shift of 3.6", int(kept.sum()), "of", kept.size)
    assert kept.sum() < kept.size // 2                          # 3.6 rounds to the rim


def test_no_pair_crosses_two_islands(field):
    """Two islands with a strip of label 0 between them: the costs of the whole layout are the sums of the costs of each island
    alone, which cannot hold a pair of two labels."""
    labels = np.zeros((H, W), np.uint8)
    labels[:, :46], labels[:, 48:] = 1, 2                   # two texels apart: within reach of R = 4
    a = ref.to_u8(field)
    b = np.roll(a, (1, 4), (0, 1))
    c, n = ref.costs(a, ONES, b, ONES, labels, B, S, R)
    parts = [ref.costs(a, ONES, b, ONES, np.where(labels == k, labels, 0).astype(np.uint8), B, S, R) for k in (1, 2)]
    assert (n == parts[0][1] + parts[1][1]).all() and (c == parts[0][0] + parts[1][0]).all()
    one = ref.costs(a, ONES, b, ONES, (labels != 0).astype(np.uint8), B, S, R)[1]
    assert (one >= n).all() and (one > n).any()                 # with one label the pairs across the strip would count
    Ca, oka = ref.census(a, ONES, labels)
    assert not oka[:, 46:48].any() and oka[3:-3, 3:46].all() and oka[3:-3, 48:-3].all()


def test_census_bits_and_validity():
    L = np.full((9, 9), 100, np.uint8)
    L[1, 1], L[4, 5], L[7, 7] = 5, 7, 9                          # neighbours (-3,-3), (0,+1), (+3,+3) of the centre (4, 4)
    valid = np.ones((9, 9), np.uint8)
    C_, ok = ref.census(L, valid, valid)
    assert ok.sum() == 9 and ok[3:6, 3:6].all()
    assert int(C_[4, 4]) == (1 << 0) | (1 << 24) | (1 << 47)     # row-major without the centre: 0, 3 * 7 + 4 - 1, 47
    valid[1, 7] = 0
    assert not ref.census(L, valid, np.ones((9, 9), np.uint8))[1][4, 4]
    assert ref.luma(np.array([[[255, 255, 255], [10, 200, 30], [1, 0, 0]]], np.uint8)).tolist() == [[255, (770 + 30000 + 870 + 128) >> 8, 0]]
    assert int(ref.popcount(np.array([0xFFFF0000FFFF], np.uint64))[0]) == 32


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_match_refuses_bad_arguments_without_a_device():
    from topo4d_amd import drift
    img = torch.zeros(40, 48, 3, dtype=torch.uint8)
    m = torch.ones(40, 48, dtype=torch.uint8)
    ok = dict(block=16, stride=8, radius=4, min_count=None)
    bad = [dict(block=15), dict(block=6), dict(block=66), dict(stride=0), dict(stride=17), dict(radius=-1), dict(radius=17),
           dict(min_count=0), dict(min_count=257)]
    for change in bad:
        with pytest.raises(ValueError):
            drift.match(img, m, img, m, m, **{**ok, **change})
    with pytest.raises(ValueError, match="image_a"):
        drift.match(img.float(), m, img, m, m, **ok)
    with pytest.raises(ValueError, match="image_b"):
        drift.match(img, m, img[:20], m, m, **ok)
    with pytest.raises(ValueError, match="image_a"):
        drift.match(torch.zeros(40, 48, 2, dtype=torch.uint8), m, img, m, m, **ok)
    with pytest.raises(ValueError, match="valid_a"):
        drift.match(img, m[:10], img, m, m, **ok)
    with pytest.raises(ValueError, match="valid_b"):
        drift.match(img, m, img, m.float(), m, **ok)
    with pytest.raises(ValueError, match="labels"):
        drift.match(img, m, img, m, m.bool(), **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):     # everything right but the device
        drift.match(img, m, img, m, m, **ok)
    assert drift.check_options(32) == (32, 16, 8, 512)
    assert drift.blocks(7, 40, 8, 4) == (0, 9) and drift.blocks(96, 96, 16, 8) == (11, 11)
    with pytest.raises(ValueError):
        drift.flow(torch.zeros(2, 2, 15, dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        drift.flow(torch.zeros(2, 2, 16, dtype=torch.int32), 4, ratio=1.5)


def test_the_c_entry_points_refuse_bad_arguments_before_touching_a_device():
    from topo4d_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    ARG, SIZE = _lib.T4D_ERR_ARG, _lib.T4D_ERR_STATE_SIZE
    one, none = C.c_void_p(64), None                           # "some address": never dereferenced by a call that is refused

    def refused(rc, code=ARG):
        assert rc == code, (rc, lib.t4d_last_error())
        assert lib.t4d_last_error()

    nb = lib.t4d_drift_scratch_bytes(96, 96, 16, 8, 4)
    assert nb >= 2 * 96 * 96 * 8
    for shape in ((0, 96, 16, 8, 4), (96, 0, 16, 8, 4), (96, 96, 15, 8, 4), (96, 96, 6, 3, 4), (96, 96, 66, 8, 4), (96, 96, 16, 0, 4),
                  (96, 96, 16, 17, 4), (96, 96, 16, 8, -1), (96, 96, 16, 8, 17), (65537, 96, 16, 8, 4)):
        assert lib.t4d_drift_scratch_bytes(*shape) == 0 and lib.t4d_last_error()
        refused(lib.t4d_drift_match(one, one, one, one, one, shape[0], shape[1], shape[2], shape[3], shape[4], 1, one, one, 1 << 40, none))
    good = (96, 96, 16, 8, 4, 128)
    for k in range(5):
        ptrs = [one] * 5
        ptrs[k] = none
        refused(lib.t4d_drift_match(*ptrs, *good, one, one, nb, none))
    refused(lib.t4d_drift_match(one, one, one, one, one, *good, none, one, nb, none))
    refused(lib.t4d_drift_match(one, one, one, one, one, *good, one, none, nb, none))
    refused(lib.t4d_drift_match(one, one, one, one, one, 96, 96, 16, 8, 4, 0, one, one, nb, none))
    refused(lib.t4d_drift_match(one, one, one, one, one, 96, 96, 16, 8, 4, 257, one, one, nb, none))
    refused(lib.t4d_drift_match(one, one, one, one, one, *good, one, one, nb - 1, none), SIZE)
    refused(lib.t4d_drift_match(one, one, one, one, one, *good, one, C.c_void_p(68), nb, none))        # a misaligned scratch
    # no whole block: nothing to do is not an error, and nothing is launched
    small = lib.t4d_drift_scratch_bytes(7, 40, 8, 4, 2)
    assert small > 0
    assert lib.t4d_drift_match(one, one, one, one, one, 7, 40, 8, 4, 2, 32, one, one, small, none) == _lib.T4D_OK


def test_the_parser():
    from topo4d_amd import drift, evaluate
    p = drift.build_parser()
    a = p.parse_args(["-e", "exp", "-s", "seq", "-od", "out"])
    assert (a.exp, a.seq, a.output_dir, a.frames, a.save_fields) == ("exp", "seq", "out", None, False)
    assert drift.options_of(a) == dict(texture="face_proj.png", ref="first", level=2, block=32, stride=None, radius=8, ratio=0.8,
                                       unit=1000.0)
    a = p.parse_args(["-e", "e", "-s", "s", "-od", "o", "--frames", "2-4", "--texture", "face.png", "--ref", "previous", "--level", "1",
                      "--block", "16", "--stride", "4", "--radius", "5", "--ratio", "0.7", "--unit", "1", "--save_fields"])
    assert a.frames == [2, 3, 4] and a.save_fields
    assert drift.options_of(a) == dict(texture="face.png", ref="previous", level=1, block=16, stride=4, radius=5, ratio=0.7, unit=1.0)
    with pytest.raises(SystemExit):
        p.parse_args(["-e", "e", "-s", "s", "-od", "o", "--ref", "last"])
    e = evaluate.build_parser().parse_args(["-e", "e", "-s", "s"])
    assert e.drift is False
    e = evaluate.build_parser().parse_args(["-e", "e", "-s", "s", "--drift", "--drift_level", "1", "--drift_ref", "previous"])
    assert e.drift and drift.options_of(e, "drift_")["level"] == 1 and drift.options_of(e, "drift_")["ref"] == "previous"
    for bad in (dict(block=15), dict(radius=17), dict(ratio=0.0), dict(level=9)):
        args = p.parse_args(["-e", "e", "-s", "s", "-od", "o"])
        with pytest.raises(SystemExit):
            drift.drift_tree(args, options={**drift.options_of(args), **bad})


def test_drift_stats_on_a_hand_made_field():
    from topo4d_amd import drift
    texels = torch.tensor([[1.0, 2.0, 3.0, 100.0], [4.0, 5.0, 6.0, 7.0], [8.0, 9.0, 10.0, 200.0]], dtype=torch.float64)
    units = texels * 0.5
    kept = torch.ones(3, 4, dtype=torch.bool)
    kept[0, 3] = kept[2, 3] = False
    s = drift.drift_stats(texels, units, kept, unit=10.0)
    assert (s["blocks"], s["kept"], s["kept_fraction"]) == (12, 10, 10 / 12)
    assert (s["mean_texels"], s["median_texels"], s["p90_texels"], s["max_texels"]) == (5.5, 5.0, 9.0, 10.0)
    assert (s["mean"], s["median"], s["p90"], s["max"]) == (27.5, 25.0, 45.0, 50.0)
    none = drift.drift_stats(texels, units, torch.zeros(3, 4, dtype=torch.bool))
    assert none == {"blocks": 12, "kept": 0, "kept_fraction": 0.0}
    assert drift.drift_stats(texels[:0], units[:0], kept[:0]) == {"blocks": 0, "kept": 0, "kept_fraction": 0.0}
    one = drift.drift_stats(texels, units, kept & (texels == 4.0))
    assert (one["median"], one["p90"], one["max"], one["mean"]) == (2.0, 2.0, 2.0, 2.0)


def test_flow_and_metric_by_hand():
    """a table row whose parabola is known: q- = 3, q0 = 1, q+ = 2 -> (3 - 2) / (2 (3 - 2 + 2)) = 1/6, for the restatement and for
    topo4d_amd.drift.flow alike"""
    from topo4d_amd import drift
    row = np.zeros((1, 1, 16), np.int32)
    row[0, 0] = [1, -2, 10, 10, 30, 10, 20, 10, 40, 10, 40, 10, 50, 10, 0, 0]

    def both(table, radius, ratio=0.8):
        d, kept = ref.flow(table, radius, ratio)
        d_t, kept_t = drift.flow(torch.from_numpy(table.copy()), radius, ratio)
        assert d_t.dtype == torch.float64 and np.array_equal(d_t.numpy(), d) and np.array_equal(kept_t.numpy(), kept)
        return d, kept

    d, kept = both(row, 4)
    assert kept.all() and d[0, 0, 0] == 1 + 1.0 / 6.0 and d[0, 0, 1] == -2.0
    assert not both(row, 2)[1].any()                            # |dx| = 2 is the rim of radius 2
    assert not both(row, 4, ratio=0.1)[1].any()                 # q_best = 1 > 0.1 * 5
    steep = row.copy()
    steep[0, 0, 4:8] = [100, 10, 10, 10]                        # q- = 10, q+ = 1: 9 / (2 * 9) = 0.5, the clamp's edge
    assert both(steep, 4)[0][0, 0, 0] == 1.5
    steep[0, 0, 2] = 0                                          # q0 = 0: 9 / 22
    assert both(steep, 4)[0][0, 0, 0] == 1 + 9.0 / 22.0
    lone = row.copy()
    lone[0, 0, 6:8] = 0                                         # (dy + 1, dx) inadmissible: no offset on that axis
    assert both(lone, 4)[0][0, 0].tolist() == [1.0, -2.0]
    row[0, 0, 12:14] = [10, 10]                                 # the second as good as the best
    assert not both(row, 4)[1].any()
    row[0, 0, 12:14] = [0, 0]
    assert not both(row, 4)[1].any()
    # metric: a plane whose texel is 2 units wide and 3 units high; the module's metric runs on CPU tensors as well
    h = w = 24
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    pos = np.stack([2.0 * x, 3.0 * y, 0 * x], -1)
    labels = np.ones((h, w), np.uint8)
    dd = np.zeros((3, 3, 2))
    dd[..., 0], dd[..., 1] = 1.0, -2.0

    def both_metric():
        units, kept = ref.metric(dd, np.ones((3, 3), bool), pos, labels, 8, 8)
        units_t, kept_t = drift.metric(torch.from_numpy(dd), torch.ones(3, 3, dtype=torch.bool), torch.from_numpy(pos),
                                       torch.from_numpy(labels.copy()), 8, 8)
        assert np.array_equal(units_t.numpy(), units) and np.array_equal(kept_t.numpy(), kept)
        return units, kept

    units, kept = both_metric()
    assert (units == 5.0).all() and kept.all()                  # |(2 * -2, 3 * 1)| = 5
    labels[12, 13] = 0                                          # the right-hand neighbour of block (1, 1)'s centre (12, 12)
    assert both_metric()[1].sum() == 8
    assert drift.length(torch.tensor([[[3.0, -4.0]]], dtype=torch.float64)).item() == 5.0 == ref.length(np.array([[[3.0, -4.0]]])).item()
