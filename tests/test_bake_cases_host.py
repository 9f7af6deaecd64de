"""CPU: the inputs of tests/test_gpu_bake_edges.py (oracle.texture_oracle.edge_cases, built by tests/bake_cases.py).

1. Truth: the port's image and depth have the digests of the REAL reference's (golden G17, written by oracle/build_ref.py), and equal
   the reference bit for bit where oracle/_ref is built - signed zeros, infinities and all.
2. Coverage: every case reaches the part of csrc/t4d_texture.hip it is there for.  These are conditions on the inputs (through
   bake_cases.bin_model, the kernel's binning restated in numpy) and on the reference's outputs; if a generator changes and one no
   longer holds, the GPU test of that name has stopped testing what it says.
"""
import os

import numpy as np
import pytest

from oracle import texture_oracle as TX
from tests import bake_cases as BC

G17 = os.path.join(os.path.dirname(__file__), "golden", "g17_bake_edges.npz")
ALL_WIDTHS = set(range(1, BC.TILE + 1))


@pytest.fixture(scope="module")
def cases():
    return TX.edge_cases()


@pytest.fixture(scope="module")
def port(cases):
    """name -> (image, depth) of the port, computed once."""
    return {name: TX.render_colors_port(*args, **kw) for name, (args, kw) in cases.items()}


def _bins(cases, name, rows=None):
    verts, tris, _, h, w = cases[name][0]
    return BC.bin_model(verts, tris, h, w, rows)


def test_port_has_the_digests_of_the_real_reference(cases, port):
    g = np.load(G17)
    names = [str(n) for n in g["names"]]
    assert names == list(cases), "golden G17 lists other cases: rerun oracle/build_ref.py"
    for k, name in enumerate(names):
        image, depth = port[name]
        assert TX.digest(image) == str(g["image"][k]), f"{name}: the port's image differs from the reference's"
        assert TX.digest(depth) == str(g["depth"][k]), f"{name}: the port's depth differs from the reference's"


def test_digest_is_bitwise():
    z = np.zeros(4, np.float32)
    assert TX.digest(z) != TX.digest(-z)
    a = np.full(1, np.nan, np.float32)
    b = a.copy(); b.view(np.uint32)[0] ^= 1
    assert TX.digest(a) != TX.digest(b) and TX.digest(a) == TX.digest(a.copy())
    with pytest.raises(AssertionError):
        BC.assert_bits_equal(z, -z, "signed zeros")
    BC.assert_bits_equal(a, a.copy(), "the same NaN")


def test_port_equals_the_real_reference_bitwise(cases, port):
    """Where oracle/_ref is built (elsewhere G17's digests above stand for it)."""
    for name, (args, kw) in cases.items() if TX.have_ref() else ():
        image, depth = TX.render_colors_ref(*args, **kw)
        BC.assert_bits_equal(port[name][0], image, f"{name} image")
        BC.assert_bits_equal(port[name][1], depth, f"{name} depth")


def test_bin_model_counts_what_a_plain_loop_counts():
    case = BC.soup(300, 150, 140, 3, margin=40)
    for rows in (None, (37, 101)):
        r0, r1 = rows or (0, case.h)
        counts = np.zeros(((r1 - 1) // 32 - r0 // 32 + 1, (case.w + 31) // 32), np.int64)
        widths = set()
        for tri in case.tris:
            x, y = case.verts[tri, 0], case.verts[tri, 1]
            x0, x1 = max(int(np.ceil(x.min())), 0), min(int(np.floor(x.max())), case.w - 1)
            y0, y1 = max(int(np.ceil(y.min())), 0), min(int(np.floor(y.max())), case.h - 1)
            if x1 < x0 or y1 < y0 or y1 < r0 or y0 >= r1:
                continue
            y0, y1 = max(y0, r0), min(y1, r1 - 1)
            for by in range(y0 // 32, y1 // 32 + 1):
                for bx in range(x0 // 32, x1 // 32 + 1):
                    counts[by - r0 // 32, bx] += 1
                    widths.add(min(x1, 32 * bx + 31) - max(x0, 32 * bx) + 1)
        b = BC.bin_model(case.verts, case.tris, case.h, case.w, rows)
        assert (b.counts == counts).all() and b.pairs == counts.sum() and b.widths == widths
        assert b.max_wg_area == counts.size                          # 300 scattered triangles in two workgroups: each spans the image


def test_a_every_box_width_on_both_list_paths(cases):
    fast, general = _bins(cases, "a_fast_n100"), _bins(cases, "a_general_n500")
    assert fast.counts.min() > 0 and fast.counts.max() <= BC.STAGE, "one staging round: the fast path"
    assert general.counts.min() > 2 * BC.STAGE, "three staging rounds and more in every tile"
    assert fast.widths == ALL_WIDTHS and general.widths == ALL_WIDTHS


def test_a_width_boxes_are_drawn_whole(cases, port):
    for name in ("a_width_boxes", "a_width_boxes_c4"):
        (verts, tris, colors, h, w), kw = cases[name]
        b = _bins(cases, name)
        assert b.widths == ALL_WIDTHS and (b.counts == 1).all()
        image, depth = port[name]
        want = np.full((h, w), BC.FRESH_DEPTH, np.float32)
        for k in range(32):
            x0, y0 = 32 * (k % 8), 32 * (k // 8)
            want[y0:y0 + 32, x0:x0 + k + 1] = verts[3 * k, 2]
        BC.assert_bits_equal(depth, want, f"{name}: every texel of every box, and no other, is drawn at vertex 0's depth")


@pytest.mark.parametrize("n", (1, 119, 120, 121, 240, 241, 360, 361))
def test_b_the_one_tile_lists_exactly_n(cases, port, n):
    for name in (f"b_n{n}", f"b_n{n}_dup"):
        assert _bins(cases, name).counts.tolist() == [[n]]
    if n > 1:                                                        # the copies tie everywhere and the order decides
        (verts, tris, colors, h, w), kw = cases[f"b_n{n}_dup"]
        rev = TX.render_colors_port(verts, tris[::-1], colors, h, w, **kw)
        assert (BC.bits(rev[0]) != BC.bits(port[f"b_n{n}_dup"][0])).any()
        BC.assert_bits_equal(rev[1], port[f"b_n{n}_dup"][1], "depth does not depend on the order")


def test_c_lattice_zeros_and_degenerate_winners(cases, port):
    verts = cases["c_lattice_depths"][0][0]
    assert (verts[:, :2] * 2 == np.round(verts[:, :2] * 2)).all()
    assert set(BC.bits(verts[:, 2]).tolist()) == {0, 0x80000000, 0x3f800000, 0xbf800000}, "both zeros among four depth levels"
    # zeros alone: +0 and -0 tie, the lower index keeps its sign in the depth buffer, and the order decides the image
    (verts, tris, colors, h, w), kw = cases["c_signed_zeros"]
    depth = BC.bits(port["c_signed_zeros"][1])
    assert (depth == 0x80000000).mean() > 0.1 and (depth == 0).mean() > 0.1
    rev = TX.render_colors_port(verts, tris[::-1], colors, h, w, **kw)
    assert (BC.bits(rev[0]) != BC.bits(port["c_signed_zeros"][0])).mean() > 0.5
    # ... and an order that took -0 for less than +0 would give another image than the reference's
    plus = verts.copy(); plus[:, 2] = 0.0
    first_plus = TX.render_colors_port(plus, tris, colors, h, w, **kw)
    BC.assert_bits_equal(first_plus[0], port["c_signed_zeros"][0], "the signs of the zeros change no winner")
    minus = verts.copy(); minus[BC.bits(verts[:, 2]) == 0x80000000, 2] = -1e-30
    below = TX.render_colors_port(minus, tris, colors, h, w, **kw)
    assert (BC.bits(below[0]) != BC.bits(port["c_signed_zeros"][0])).mean() > 0.2, "-0 ranked below +0 would change winners"
    for name in ("c_degenerate", "c_degenerate_far"):
        (verts, tris, colors, h, w), kw = cases[name]
        keep = np.arange(30, tris.shape[0])                         # soup(degenerate=30): the first thirty
        # degenerate in the reference's own arithmetic: inverDeno's denominator is exactly 0
        p = verts[tris[:30], :2]
        v0, v1 = p[:, 2] - p[:, 0], p[:, 1] - p[:, 0]
        d00, d01, d11 = (v0 * v0).sum(1, dtype=np.float32), (v0 * v1).sum(1, dtype=np.float32), (v1 * v1).sum(1, dtype=np.float32)
        assert (d00 * d11 - d01 * d01 == 0).all()
        without = TX.render_colors_port(verts, tris[keep], colors, h, w, **kw)
        assert (BC.bits(without[0]) != BC.bits(port[name][0])).any(), f"{name}: a degenerate triangle wins a texel"
    verts = cases["c_degenerate_far"][0][0]
    assert np.abs(verts[:, :2]).max() > 2000 and np.abs(verts[:, :2]).max() < 1e6


def test_d_special_depths_reach_the_depth_buffer(cases, port):
    verts = cases["d_special_depths"][0][0]
    z = verts[:, 2]
    assert np.isnan(z).any() and (z == np.inf).any() and (z == -np.inf).any() and (BC.bits(z) == 0x80000000).any()
    assert (z == BC.FRESH_DEPTH).any() and (z == np.float32(-1e6)).any() and (z == np.float32(1e-40)).any()
    special = ~np.isfinite(z) | (np.abs(z) < 1e-30) | (z < -9e5)
    assert 0.10 < special.mean() < 0.20
    depth = port["d_special_depths"][1]
    denormal = (np.abs(depth) < np.finfo(np.float32).tiny) & (depth != 0)
    assert (depth == BC.FRESH_DEPTH).any(), "some texel ends undrawn"
    assert (depth == np.inf).any(), "some texel ends at +inf"
    assert ((BC.bits(depth) == 0x80000000) | denormal).any(), "some texel ends at -0 or a denormal"
    assert np.isinf(depth).mean() < 0.5 and not np.isnan(depth).any()


def test_d_triangles_exactly_at_the_initial_depth_are_not_drawn(cases, port):
    (verts, tris, colors, h, w), kw = cases["d_initial_depth"]
    assert len(set(BC.bits(verts[:, 2]).tolist())) == 3 and (verts[:, 2] == BC.FRESH_DEPTH).any()
    image, depth = port["d_initial_depth"]
    assert (depth > BC.FRESH_DEPTH).any() and (depth == BC.FRESH_DEPTH).any() and not (depth < BC.FRESH_DEPTH).any()
    # a `>=` in the depth test is what a buffer one float lower shows: it must draw texels that the reference leaves alone
    lower = np.full((h, w), np.nextafter(BC.FRESH_DEPTH, np.float32(-np.inf)), np.float32)
    ge = TX.render_colors_port(verts, tris, colors, h, w, c=3, return_depth=True, image0=kw["BG"], depth0=lower)
    drawn_at_initial = (ge[1] == BC.FRESH_DEPTH) & (BC.bits(ge[0]) != BC.bits(image)).any(-1)
    assert drawn_at_initial.sum() > 100 and (depth[drawn_at_initial] == BC.FRESH_DEPTH).all()


def test_e_duplicates_tie_everywhere(cases, port):
    (verts, tris, colors, h, w), kw = cases["e_duplicates"]
    assert tris.shape[0] == 200 and not port["e_duplicates"][1][port["e_duplicates"][1] != BC.FRESH_DEPTH].any()
    rev = TX.render_colors_port(verts, tris[::-1], colors, h, w, **kw)
    assert (BC.bits(rev[0]) != BC.bits(port["e_duplicates"][0])).mean() > 0.5, "the order decides most texels"


def test_f_channels_and_visible_background(cases, port):
    for name, c in (("f_c1", 1), ("f_c2", 2), ("f_c4", 4), ("f_c5", 5), ("f_c4_n500", 4)):
        args, kw = cases[name]
        assert kw["c"] == c and kw["BG"].shape == (64, 64, c) and args[2].shape[1] == c
        image, depth = port[name]
        undrawn = depth == BC.FRESH_DEPTH
        assert undrawn.any() and not undrawn.all()
        BC.assert_bits_equal(image[undrawn], kw["BG"][undrawn], f"{name}: background where nothing is drawn")
        counts = _bins(cases, name).counts
        assert counts.min() > BC.STAGE if name == "f_c4_n500" else (counts.min() > 0 and counts.max() <= BC.STAGE)


def test_g_images_inside_the_ring(cases):
    for (h, w), inner in (((1, 1), 0), ((2, 3), 0), ((4, 4), 0), ((5, 5), 1), ((3, 40), 0)):
        assert cases[f"g_{h}x{w}"][0][3:] == (h, w)
        y, x = np.mgrid[:h, :w]
        ring = (x < 2) | (x > w - 3) | (y < 2) | (y > h - 3)
        assert (~ring).sum() == inner
        assert _bins(cases, f"g_{h}x{w}").counts.min() > 0


def test_h_binning_at_size(cases):
    for n, bins, chunks in ((120, 1089, 2), (160, 2145, 3)):
        shuffled, ordered = _bins(cases, f"h_n{n}"), _bins(cases, f"h_n{n}_sorted")
        assert shuffled.counts.size == ordered.counts.size == bins and -(-bins // BC.SCAN_CHUNK) == chunks
        assert shuffled.max_wg_area > BC.HIST, "a shuffled index buffer: per-pair atomics"
        assert ordered.max_wg_area <= 130, "sorted by first vertex: the workgroup histogram"
        assert (shuffled.counts == ordered.counts).all() and shuffled.counts.max() <= BC.STAGE
    band = _bins(cases, "h_n160", TX.ROWS_H)
    assert band.counts.size > BC.SCAN_CHUNK and band.max_wg_area > BC.HIST and band.pairs < _bins(cases, "h_n160").pairs
    band = _bins(cases, "h_n160_sorted", TX.ROWS_H)
    assert band.counts.size > BC.SCAN_CHUNK and band.max_wg_area <= 130


def test_i_the_callers_buffer_beats_some_triangles(cases, port):
    (verts, tris, colors, h, w), kw = cases["i_hostile"]
    image, depth = port["i_hostile"]
    d0 = kw["depth0"]
    kept = BC.bits(depth) == BC.bits(d0)
    ordinary = np.isfinite(d0) & (d0 != BC.FRESH_DEPTH)
    assert (kept & ordinary).any() and (~kept & ordinary).any(), "the buffer's ordinary depths win in places and lose in others"
    assert 0.2 < (d0 == BC.FRESH_DEPTH).mean() < 0.3 and (d0 == np.inf).any() and kept[d0 == np.inf].all()
    BC.assert_bits_equal(image[kept], kw["image0"][kept], "the caller's image where its depth stands")
    assert _bins(cases, "i_hostile", TX.BAND_I).counts.min() > 2 * BC.STAGE
    # where the buffer holds exactly what the best triangle reaches, `>` draws nothing: the caller's image stays
    fresh = port["a_general_n500"][1]
    equal = (BC.bits(d0) == BC.bits(fresh)) & ordinary
    assert 0.05 < equal.mean() < 0.15 and kept[equal].all()
