"""Designed inputs for the PNG encoder's byte-for-byte tests (tests/test_png_ref_host.py on the CPU, tests/test_gpu_png_bytes.py on
the GPU).  Every case is an image of one to three 16 KiB segments with a claim about the branch of the rule it reaches; the claim is
checked on the census tests/png_ref.encode returns, never taken from the construction.

    CASES: {name: Case(image, bits, claim)}      claim(census list) raises AssertionError when the case does not hold it
"""
from collections import namedtuple

import numpy as np

from tests import png_ref

Case = namedtuple("Case", "image bits claim")
CASES = {}


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _small_values(n):
    """n byte values of small |int8|, none of them 0 or 1: 255, 2, 254, 3, ..."""
    out = []
    for k in range(2, 2 + n):
        out += [256 - (k - 1), k]
    return out[:n]


# ---- the length limiter at 15 bits -------------------------------------------------------------------------------------------------
def _chain_image(rare_freqs, seed, h=128, w=127):
    """A 1-channel image whose filtered stream (filter 0 on every row, which the census confirms) holds the byte values of
    _small_values with the frequencies `rare_freqs`, each followed by at least one byte of a filler that alternates 0, 1 and so
    never forms a run.  0 and 1 take the rest of the segment and are the two most frequent symbols.  The row length is odd, so the
    filler changes phase from row to row and neither Up nor Sub beats None."""
    vals = _small_values(len(rare_freqs))
    others = np.repeat(np.array(vals, np.uint8), rare_freqs)
    np.random.default_rng(seed).shuffle(others)
    filler = h * w - others.size
    base, extra = divmod(filler, others.size)
    assert base >= 1
    pix, phase = [], 0
    for i, o in enumerate(others.tolist()):
        pix.append(o)
        for _ in range(base + (1 if i < extra else 0)):
            pix.append(phase)
            phase ^= 1
    return np.array(pix, np.uint8).reshape(h, w)


def _claim_limiter15(depth_ok, steps_ok, clamped_ok):
    def claim(census):
        assert len(census) == 1
        c = census[0]
        assert not c["filters"].any(), "filter 0 must win every row for the histogram to be the designed one"
        assert c["classes"] == {"literal"}
        assert depth_ok(c["lit_depth"]) and c["lit"]["two_queue_depth"] == c["lit_depth"], (c["lit_depth"], c["lit"])
        assert max(c["lit_len"]) == 15 and c["huffman"]
        assert steps_ok(c["lit"]["kraft_steps"]) and clamped_ok(c["lit"]["clamped_leaves"]), c["lit"]
    return claim


F = _fib(24)
# 19 symbols 1 (end of block), 1, 2, 3, 5, ... with the two largest raised: natural depth 18
CASES["limiter15_fib19"] = Case(_chain_image(F[1:17], 1), 8, _claim_limiter15(lambda d: d >= 17, lambda s: s >= 2, lambda n: n >= 3))
# 17 symbols: depth exactly 16, two leaves to clamp, one unit of excess
CASES["limiter15_depth16"] = Case(_chain_image(F[1:15], 2), 8, _claim_limiter15(lambda d: d == 16, lambda s: s == 1, lambda n: n == 2))
# eight symbols of frequency 1 under a chain of 8 x (1, 2, 3, 5, ...): eight leaves at depth 17
CASES["limiter15_many_clamped"] = Case(_chain_image([1] * 7 + [8 * f for f in F[1:13]], 3), 8,
                                       _claim_limiter15(lambda d: d >= 17, lambda s: s >= 4, lambda n: n >= 8))


# ---- every length symbol, remainders, runs across slices and segments --------------------------------------------------------------
def _runs_image():
    """One row.  Sub wins it (the census confirms), so the filtered stream is a non-zero byte where the pixel changes and zeros
    while it holds: zero runs of any wanted length.  Stream position = 1 + pixel index."""
    zero_runs = [1 + b for b in png_ref.LEN_BASE[:28]]                  # a literal, then a remainder match of every base 3..227
    zero_runs += [1 + 257, 1 + 258, 1 + 258 + 1, 1 + 258 + 2, 1 + 2 * 258 + 2, 1 + 258 + 3, 2, 3]
    pix, v = [], 0
    for k, z in enumerate(zero_runs):
        v = (v + 37 + k) % 256
        pix += [v] * (1 + z)
    # a zero run that starts at the last byte of a thread slice (64 bytes in a full segment) and covers more than three slices
    target = ((len(pix) + 1 + 2) // 64 + 1) * 64 + 63                   # stream position of the run's first zero
    while len(pix) + 1 + 1 < target:
        v = (v + 1) % 256
        pix.append(v)
    pix.append((v + 5) % 256)
    assert len(pix) + 1 == target
    pix += [pix[-1]] * 200
    # single pixels up to the segment's end, then a run that crosses it
    while len(pix) + 1 < png_ref.SEG - 100:
        v = (pix[-1] + 1) % 256
        pix.append(v)
    pix += [(pix[-1] + 9) % 256] * 400
    pix += [3, 3, 3, 9]
    return np.array(pix, np.uint8).reshape(1, -1), target


def _claim_runs(target):
    def claim(census):
        assert len(census) == 2 and census[0]["n"] == png_ref.SEG
        assert list(census[0]["filters"]) == [1]
        classes = census[0]["classes"] | census[1]["classes"]
        for sym in range(257, 285):                                     # 285 is length 258: never a remainder, always the full match
            assert ("rem_match", sym) in classes, sym
        assert "match258" in classes and census[0]["lit_freq"][285] >= 6
        for rem in (0, 1, 2):
            assert ("rem_literals_after_258", rem) in classes, rem
        runs0 = census[0]["runs"]
        assert (target, target + 200) in runs0 and target % 64 == 63    # starts on a slice's last byte, spans slices
        assert runs0[-1][1] == png_ref.SEG and runs0[-1][1] - runs0[-1][0] > 64 and census[1]["runs"][0][1] > 64
    return claim


_img, _target = _runs_image()
CASES["runs_every_length_symbol"] = Case(_img, 8, _claim_runs(_target))


# ---- filter ties --------------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def _filter_image(c=1, w=24, seed=4):
    rng = np.random.default_rng(seed)
    n = w * c
    noise = lambda: rng.integers(0, 256, n).astype(np.int64)
    rows = [noise()]                                                    # first row: Up is None, Paeth is Sub
    rows.append(rng.integers(-2, 3, n) & 255)                           # small values under noise: None wins
    rows.append(np.full(n, 100))                                        # a flat row under small values: Sub wins
    rows.append(noise())
    rows.append(rows[-1].copy())                                        # a copy of the row above: Up wins
    rows.append(noise())
    up, cur = rows[-1], np.zeros(n, np.int64)
    for x in range(n):
        cur[x] = ((cur[x - c] if x >= c else 0) + up[x]) >> 1           # Average's own prediction: Average wins
    rows.append(cur)
    rows.append(noise())
    up, cur = rows[-1], np.zeros(n, np.int64)
    for x in range(n):
        cur[x] = _paeth(cur[x - c] if x >= c else 0, up[x], up[x - c] if x >= c else 0)
    rows.append(cur)                                                    # Paeth's own prediction: Paeth wins
    rows.append(np.zeros(n, np.int64))                                  # all zero under a non-zero row ...
    rows.append(np.zeros(n, np.int64))                                  # ... and all zero under zeros: five equal scores
    rows.append((np.arange(n) % 2) * 3 + 1)                             # under zeros: None = Up < Sub = Paeth
    return np.array(rows, np.uint8).reshape(len(rows), w, c)


def _claim_filters(census):
    cost, filters = census[0]["filter_cost"], census[0]["filters"]
    assert cost[0, 0] == cost[0, 2] and cost[0, 1] == cost[0, 4] and filters[0] in (0, 1, 3)
    all_equal = [r for r in range(len(cost)) if len(set(cost[r])) == 1]
    assert all_equal and all(filters[r] == 0 for r in all_equal)
    two = [r for r in range(len(cost)) if (cost[r] == cost[r].min()).sum() == 2]
    assert two and all(filters[r] == int(np.flatnonzero(cost[r] == cost[r].min())[0]) for r in two)
    for f in range(5):
        alone = [r for r in range(1, len(cost)) if filters[r] == f and (cost[r] == cost[r].min()).sum() == 1]
        assert alone, f"filter {f} wins no row alone"


CASES["filter_ties_c1"] = Case(_filter_image(1), 8, _claim_filters)
CASES["filter_ties_c3"] = Case(_filter_image(3), 8, _claim_filters)
CASES["filter_ties_c4"] = Case(_filter_image(4, seed=5), 8, _claim_filters)
_b = _filter_image(2, seed=20).astype(np.int32)                         # two bytes per sample; bits above 15 are ignored
CASES["filter_ties_16bit"] = Case(_b[:, :, 0] * 256 + _b[:, :, 1] + (7 << 16), 16, _claim_filters)


# ---- the length limiter at 7 bits ------------------------------------------------------------------------------------------------------
def _claim_limiter7(census):
    c = census[0]
    assert c["cl_depth"] >= 8 and c["cl"]["two_queue_depth"] == c["cl_depth"] and c["cl"]["kraft_steps"] >= 1, (c["cl_depth"], c["cl"])
    assert max(c["cl_len"]) == 7 and c["huffman"]


# found by looking at the census of small mixed images: this one's code-length histogram has a natural depth of 8
CASES["limiter7"] = Case(_filter_image(3, seed=4), 8, _claim_limiter7)


# ---- the stored / Huffman decision --------------------------------------------------------------------------------------------------
def _thinned_noise(full_rows, h=127, w=128, seed=5):
    """Noise over all 256 values in the first rows, over 180 values in the rest: the Huffman size moves by a few bytes per row."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 180, (h, w))
    img[:full_rows] = rng.integers(0, 256, (full_rows, w))
    return img.astype(np.uint8)


def _claim_edge(lo, hi, want_huffman):
    def claim(census):
        assert len(census) == 1
        d = census[0]["huff_bytes"] - census[0]["stored_bytes"]
        assert lo <= d <= hi and census[0]["huffman"] == want_huffman == (d < 0), d
    return claim


# the numbers of full-alphabet rows come from a scan of all 128 with the restatement; the claims hold the cases to it
CASES["edge_huffman_by_one_byte"] = Case(_thinned_noise(52), 8, _claim_edge(-1, -1, True))
CASES["edge_tie_is_stored"] = Case(_thinned_noise(53), 8, _claim_edge(0, 0, False))
CASES["edge_stored_by_one_byte"] = Case(_thinned_noise(56), 8, _claim_edge(1, 1, False))
CASES["edge_huffman_by_four_bytes"] = Case(_thinned_noise(50), 8, _claim_edge(-8, -2, True))


# ---- segment sizes ------------------------------------------------------------------------------------------------------------------
def _mixed(shape, seed, bits=8):
    """Smooth in the left half, noise in the right, a flat band in the middle: every filter and both block kinds occur"""
    rng = np.random.default_rng(seed)
    h, w, c = shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    top = 65536 if bits == 16 else 256
    img = ((x * 3 + y * 5)[..., None] * (top // 256) + np.arange(c) * 40) % top
    img[:, w // 2:] = rng.integers(0, top, (h, w - w // 2, c))
    img[h // 3:h // 3 + 2] = 77
    return img.astype(np.int32 if bits == 16 else np.uint8)


def _claim_sizes(*ns):
    def claim(census):
        assert [c["n"] for c in census] == list(ns), [c["n"] for c in census]
    return claim


S = png_ref.SEG
CASES["one_byte_short_of_a_segment"] = Case(_mixed((127, 128, 1), 6), 8, _claim_sizes(S - 1))
CASES["exactly_one_segment"] = Case(_mixed((128, 127, 1), 7), 8, _claim_sizes(S))
CASES["one_short_extra_segment"] = Case(_mixed((129, 127, 1), 8), 8, _claim_sizes(S, 128))
CASES["last_segment_of_one_byte"] = Case(_mixed((5, 3276, 1), 9), 8, _claim_sizes(S, 1))
CASES["segment_sizes_rgba"] = Case(_mixed((132, 31, 4), 11), 8, _claim_sizes(S, 132 * 125 - S))
CASES["segment_sizes_rgb"] = Case(_mixed((127, 43, 3), 12), 8, _claim_sizes(S, 127 * 130 - S))
CASES["segment_sizes_16bit_grey"] = Case(_mixed((128, 63, 1), 13, 16)[..., 0], 16, _claim_sizes(128 * 127))
CASES["segment_sizes_16bit_rgb"] = Case(_mixed((129, 21, 3), 14, 16), 16, _claim_sizes(129 * 127))
CASES["segment_sizes_16bit_rgba"] = Case(_mixed((130, 16, 4), 15, 16), 16, _claim_sizes(S, 130 * 129 - S))
