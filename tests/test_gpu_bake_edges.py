"""GPU: the texture bake (csrc/t4d_texture.hip) against the reference's CPU rasterizer, bit for bit, on what a jittered grid of
pixel-sized triangles never feeds it: every tile-clipped box width of the texel loop's division-free `p / rw`, lists that end exactly
at and one past a staging round, three rounds and more, depths that tie between different triangles and across rounds, signed zeros,
denormals, infinities, NaN and depths at or below the initial one, degenerate and lattice-aligned triangles, triangles far outside the
image, 1 / 2 / 4 / 5 channels, images inside the border ring, more than 1024 tiles through both binning paths and a multi-chunk
scan, a caller's depth buffer that already beats some triangles, and a pair arena of exactly the needed size.

The inputs are oracle.texture_oracle.edge_cases (tests/bake_cases.py builds them); tests/test_bake_cases_host.py holds the CPU port to
the real reference on every one of them (golden G17) and asserts, through a numpy model of the binning, that each case reaches the
part of the kernel it is named for.  Every comparison is on the uint32 view: -0 is not +0 here.

Not covered: the `ntri > 2^25` term of the fast path's condition (the key's low word then has no room for the staged slot).  It takes
33 million triangles, which is no test of seconds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import texture_oracle as TX
from tests import bake_cases as BC

pytestmark = pytest.mark.gpu

CASES = TX.edge_cases()
_REF = {}


def _ref(name):
    """(image, depth) of the CPU reference for a case, computed once and read only."""
    if name not in _REF:
        args, kw = CASES[name]
        _REF[name] = TX.render_colors_cpu(*args, **kw)
    return _REF[name]


def _gpu(name, rows=None):
    from topo4d_amd import texture
    (verts, tris, colors, h, w), kw = CASES[name]
    image, depth = texture.render_colors(verts, tris, colors, h, w, c=kw["c"], BG=kw.get("BG"), rows=rows, return_depth=True)
    return image.cpu().numpy(), depth.cpu().numpy()


def _check(name, got, want):
    BC.assert_bits_equal(got[1], want[1], f"{name} depth")
    BC.assert_bits_equal(got[0], want[0], f"{name} image")


def _abi(name, *, fresh, cap, image=None, depth=None, bg=None, rows=None, scratch_fill=0xff, ntri=None):
    """One call of t4d_texture_render_colors (fresh) or t4d_texture_bake through the C ABI over a scratch buffer filled with
    `scratch_fill`: (return code, pairs_needed, image, depth) - the buffers as numpy arrays after the call."""
    from topo4d_amd import _lib
    lib = _lib.load()
    (verts, tris, colors, h, w), kw = CASES[name]
    c = kw["c"]
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()
    v, t, col = dev(verts, np.float32), dev(tris, np.int32), dev(colors, np.float32)
    image = torch.full((h, w, c), float("nan"), device="cuda") if image is None else dev(image, np.float32)
    depth = torch.full((h, w), float("nan"), device="cuda") if depth is None else dev(depth, np.float32)
    nb = lib.t4d_texture_bake_scratch_bytes(h, w, cap)
    assert nb > 0
    sc = torch.full((nb,), scratch_fill, dtype=torch.uint8, device="cuda")
    need = C.c_int64(-1)
    r0, r1 = rows or (0, h)
    p = lambda x: C.c_void_p(x.data_ptr())
    ntri = int(t.shape[0]) if ntri is None else ntri
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if fresh:
        bg = None if bg is None else dev(bg, np.float32)
        rc = lib.t4d_texture_render_colors(p(v), p(t), p(col), None if bg is None else p(bg), int(v.shape[0]), ntri, h, w, c, r0, r1,
                                           p(image), p(depth), p(sc), nb, cap, C.byref(need), stream)
    else:
        rc = lib.t4d_texture_bake(p(v), p(t), p(col), int(v.shape[0]), ntri, h, w, c, r0, r1, p(image), p(depth), p(sc), nb, cap,
                                  C.byref(need), stream)
    torch.cuda.synchronize()
    return rc, int(need.value), image.cpu().numpy(), depth.cpu().numpy()


# a: every box width 1..32 on the fast path (lists of at most 120) and on the general path (lists above 240: three rounds and more);
#    width_boxes: one box of every width with every one of its texels drawn, so every quotient of the loop's `p / rw` shows
# b: one tile listing exactly n triangles, depth levels that tie; _dup: half of them duplicated, so equal keys straddle the rounds
# c: half-pixel lattice with signed zeros; degenerate triangles (the whole bbox is drawn); the same 3000 texels outside the image
# d: -0, denormals, -999999, -1e6, +-inf and NaN among the vertex depths
# e: every triangle four times with other colours: the lowest index wins every texel
# f: 1 and 2 channels (fast path), 4 and 5 (general path forced by the channel count), 4 with long lists; background at the rim
# g: images inside the 2-pixel ring: every texel (all but one at 5 x 5) extrapolates
# h: 1089 and 2145 tiles: scans of two and three chunks; shuffled = per-pair atomics, sorted = the workgroup histogram
@pytest.mark.parametrize("name", [n for n in CASES if n != "i_hostile"])
def test_case_is_bit_identical_to_the_reference(name):
    _check(name, _gpu(name), _ref(name))


@pytest.mark.parametrize("name", ["h_n160", "h_n160_sorted"])
def test_h_row_band_at_size(name):
    r0, r1 = TX.ROWS_H
    image, depth = _gpu(name, rows=TX.ROWS_H)
    ref_image, ref_depth = _ref(name)
    _check(name + " band", (image[r0:r1], depth[r0:r1]), (ref_image[r0:r1], ref_depth[r0:r1]))
    for part in (slice(0, r0), slice(r1, None)):
        assert not BC.bits(image[part]).any(), "rows outside the band keep the zero background"
        assert (depth[part] == BC.FRESH_DEPTH).all()


def _far_apart_soups(h, w, corners, n=100, side=96, seed=81):
    """One-channel soups of n large triangles in side x side boxes whose top-left corners are `corners` (x, y)."""
    parts = [BC.soup(n, side, side, seed + k, margin=8, c=1) for k in range(len(corners))]
    verts = np.concatenate([p.verts + np.float32([x, y, 0]) for p, (x, y) in zip(parts, corners)])
    tris = np.concatenate([p.tris + 3 * n * k for k, p in enumerate(parts)]).astype(np.int32)
    return verts, tris, np.concatenate([p.colors for p in parts])


@pytest.mark.parametrize("h,w", [pytest.param(8192, 8448, id="67584_bins_second_trip_over_the_chunk_sums")])
def test_scan_of_more_than_64_chunks(h, w):
    """264 x 256 tiles are 66 scan chunks: the workgroup of chunk 65 takes a second trip through the sums of the chunks before it
    (the h cases stop at three chunks, an 8192^2 bake at 64).  Triangles lie in chunk 0, in chunk 64 and in chunk 65 up to the last
    bin, so the second trip's term is not zero and the last offset is used."""
    verts, tris, colors = _far_apart_soups(h, w, [(0, 0), (4000, 8000), (w - 96, h - 96)])
    counts = BC.bin_model(verts, tris, h, w).counts.ravel()
    assert counts.size == 66 * BC.SCAN_CHUNK and counts[:BC.SCAN_CHUNK].any() and counts[-1] > 0
    assert counts[64 * BC.SCAN_CHUNK:65 * BC.SCAN_CHUNK].any() and counts[65 * BC.SCAN_CHUNK:].any()
    from topo4d_amd import texture
    image, depth = texture.render_colors(verts, tris, colors, h, w, c=1, return_depth=True)
    want = TX.render_colors_cpu(verts, tris, colors, h, w, c=1, return_depth=True)
    _check("66 chunks", (image.cpu().numpy(), depth.cpu().numpy()), want)


def test_i_in_out_entry_over_a_hostile_buffer():
    """t4d_texture_bake over a caller's random image and a depth buffer that beats some triangles everywhere, is at the initial depth
    in a quarter of the texels and at +inf in a few, in the band (5, 70): the reference's result inside the band, the caller's
    bits outside."""
    kw = CASES["i_hostile"][1]
    r0, r1 = TX.BAND_I
    rc, need, image, depth = _abi("i_hostile", fresh=False, cap=65536, image=kw["image0"], depth=kw["depth0"], rows=TX.BAND_I)
    assert rc == 0
    ref_image, ref_depth = _ref("i_hostile")
    _check("i_hostile band", (image[r0:r1], depth[r0:r1]), (ref_image[r0:r1], ref_depth[r0:r1]))
    for part in (slice(0, r0), slice(r1, None)):
        _check("i_hostile outside the band", (image[part], depth[part]), (kw["image0"][part], kw["depth0"][part]))


def test_j_exact_pair_capacity():
    from topo4d_amd._lib import T4D_ERR_PAIR_OVERFLOW
    name = "a_general_n500"
    verts, tris, _, h, w = CASES[name][0]
    pairs = BC.bin_model(verts, tris, h, w).pairs
    rc, need, image, depth = _abi(name, fresh=True, cap=65536)
    assert rc == 0 and need == pairs
    _check(name + " ample capacity", (image, depth), _ref(name))
    rc, need, image, depth = _abi(name, fresh=True, cap=pairs)
    assert rc == 0 and need == pairs
    _check(name + " exact capacity", (image, depth), _ref(name))
    rc, need, _, _ = _abi(name, fresh=True, cap=pairs - 1)
    assert rc == T4D_ERR_PAIR_OVERFLOW and need == pairs


def test_j_no_triangles():
    name = "a_fast_n100"
    h, w = CASES[name][0][3:]
    rc, need, image, depth = _abi(name, fresh=True, cap=1024, ntri=0)
    assert rc == 0 and need == 0
    assert not BC.bits(image).any() and (depth == BC.FRESH_DEPTH).all()
    rng = np.random.default_rng(5)
    bg = rng.normal(size=(h, w, 3)).astype(np.float32)
    rc, need, image, depth = _abi(name, fresh=True, cap=1024, ntri=0, bg=bg)
    assert rc == 0 and need == 0 and (depth == BC.FRESH_DEPTH).all()
    BC.assert_bits_equal(image, bg, "no triangles: the background")
    image0, depth0 = rng.normal(size=(h, w, 3)).astype(np.float32), rng.normal(size=(h, w)).astype(np.float32)
    rc, need, image, depth = _abi(name, fresh=False, cap=1024, ntri=0, image=image0, depth=depth0)
    assert rc == 0 and need == 0
    _check("no triangles, in/out entry", (image, depth), (image0, depth0))


def test_twice_over_dirtied_scratch_is_bit_equal():
    name = "a_general_n500"
    first = _abi(name, fresh=True, cap=65536, scratch_fill=0xff)
    second = _abi(name, fresh=True, cap=65536, scratch_fill=0x5a)
    assert first[0] == 0 and second[0] == 0 and first[1] == second[1]
    _check(name + " second run", second[2:], first[2:])
    _check(name, first[2:], _ref(name))
