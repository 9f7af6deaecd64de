"""TEST INFRASTRUCTURE (numpy only, no GPU): inputs for the texture bake that a jittered grid of pixel-sized triangles cannot
produce, and a model of the kernel's binning that says which part of csrc/t4d_texture.hip an input reaches.

  soup / anchored   triangle soups over private vertices: any size, any overlap, outside the image, on the pixel lattice,
                    degenerate, duplicated, with depth levels that tie
  special_depths    plants -0, denormals, the initial depth and what lies below it, +-inf and NaN into a case's depths
  bin_model         per-tile list lengths, pair count, tile-clipped box widths and workgroup boxes, by the kernel's own bbox rule
  assert_bits_equal float32 arrays compared through their uint32 view: -0 is not +0, and a NaN only equals the same NaN

x and y stay far inside +-1e6: `(int)ceilf` of NaN or of a huge value is undefined in the reference, so there is no truth to compare
with.  NaN and inf go into the depth only.
"""
from collections import namedtuple

import numpy as np

TILE = 32            # kTile of csrc/t4d_texture.hip
STAGE = 120          # kStage: records per staging round; a list of at most this many takes the fast path
HIST = 1024          # kTexHist: a workgroup whose box of tiles is larger bins with per-pair atomics
SCAN_CHUNK = 1024    # kScanChunk: bins per scan workgroup
BIN_BLOCK = 256      # kBlock: triangles per binning workgroup
FRESH_DEPTH = np.float32(-999999.0)

SPECIAL_DEPTHS = (-0.0, 1e-40, -1e-40, -999999.0, -1e6, np.inf, -np.inf, np.nan)

Case = namedtuple("Case", "verts tris colors h w c degenerate")      # degenerate: indices (into tris) of the degenerate triangles
Bins = namedtuple("Bins", "counts pairs widths max_wg_area")


def _soup(n, h, w, seed, margin, lattice, depth_levels, c, degenerate, dup, anchor):
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(-margin, w + margin, 3 * n), rng.uniform(-margin, h + margin, 3 * n)], 1)
    if anchor:                                                        # vertex 0 of every triangle: an integer pixel of the image
        xy[0::3, 0] = rng.integers(0, w, n)
        xy[0::3, 1] = rng.integers(0, h, n)
    if lattice:
        xy = np.round(xy * 2) / 2
    z = rng.normal(0, 1, 3 * n) if depth_levels is None else rng.choice(np.asarray(depth_levels, np.float32), 3 * n)
    verts = np.concatenate([xy, z[:, None]], 1).astype(np.float32)
    if anchor:
        tris = np.arange(3 * n, dtype=np.int32).reshape(n, 3)          # (the anchors are the rows 0, 3, 6, ..: vertex 0 of each)
        tris = tris[rng.permutation(n)]
    else:
        tris = rng.permutation(3 * n).astype(np.int32).reshape(n, 3)
    # degenerate triangles sit on the half-pixel lattice whatever `lattice` says: there v0 = p2 - p0 and v1 = p1 - p0 are exact, and
    # v0 = 2 v1 makes dot00 dot11 and dot01 dot01 the same float32 product, so the reference's `== 0` test fires (inverDeno = 0,
    # u = v = 0: the whole bbox is drawn with vertex 0's colour and depth)
    for k in range(min(degenerate, n)):
        i0, i1, i2 = tris[k]
        verts[[i0, i1, i2], :2] = np.round(verts[[i0, i1, i2], :2] * 2) / 2
        if k % 2 == 0:
            verts[i1, :2] = verts[i0, :2]                              # a repeated vertex
        else:
            verts[i2, :2] = verts[i0, :2] + 2 * (verts[i1, :2] - verts[i0, :2])      # exactly collinear
    colors = rng.uniform(0, 1, size=(3 * n, c)).astype(np.float32)
    deg = np.arange(min(degenerate, n))
    if dup > 1:                                                       # the copies: same geometry and depth, other colours
        nv = verts.shape[0]
        verts = np.concatenate([verts] * dup)
        colors = np.concatenate([colors] + [rng.uniform(0, 1, size=(nv, c)).astype(np.float32) for _ in range(dup - 1)])
        tris = np.concatenate([tris + k * nv for k in range(dup)]).astype(np.int32)
        order = rng.permutation(tris.shape[0])
        tris = tris[order]
        deg = np.flatnonzero(np.isin(order % n, deg))
    return Case(verts, np.ascontiguousarray(tris), colors, h, w, c, deg)


def soup(n, h, w, seed, *, margin, lattice=False, depth_levels=None, c=3, degenerate=0, dup=1):
    """n triangles over 3n private vertices, uniform in [-margin, w + margin] x [-margin, h + margin] (lattice: rounded to half
    pixels), depth normal or drawn from depth_levels, the triangles a random permutation of the vertices.  degenerate: the first k
    triangles get a repeated vertex (even k) or become exactly collinear (odd k).  dup: the whole soup dup times, the copies with
    colours of their own, shuffled - bit-equal depths meet everywhere and the lowest index must win."""
    return _soup(n, h, w, seed, margin, lattice, depth_levels, c, degenerate, dup, False)


def anchored(n, h, w, seed, *, margin, lattice=False, depth_levels=None, c=3, degenerate=0, dup=1):
    """soup, but vertex 0 of every triangle is an integer pixel inside the image: no triangle is culled, so the list of a one-tile
    image holds exactly n * dup."""
    return _soup(n, h, w, seed, margin, lattice, depth_levels, c, degenerate, dup, True)


def width_boxes(seed, c=3):
    """One degenerate triangle per tile of a 128 x 256 image (4 x 8 tiles), its bbox k = 1..32 texels wide and a whole tile high.
    inverDeno = 0 draws the whole bbox with vertex 0's colour and depth, and nothing else is there: EVERY index p of the texel
    loop's `p / rw` decides a texel's fate, at every width - in a soup a box's first column is mostly outside its triangle, and a
    quotient that is wrong only where a row begins goes unseen."""
    rng = np.random.default_rng(seed)
    h, w = 4 * TILE, 8 * TILE
    verts = np.zeros((96, 3), np.float32)
    for k in range(32):
        x0, y0 = TILE * (k % 8), TILE * (k // 8)
        verts[3 * k:3 * k + 2, :2] = (x0, y0)                         # p0 = p1: a repeated vertex
        verts[3 * k + 2, :2] = (x0 + k, y0 + TILE - 1)                # bbox: k + 1 wide
    verts[:, 2] = rng.normal(0, 1, 96)
    tris = np.arange(96, dtype=np.int32).reshape(32, 3)[rng.permutation(32)]
    return Case(verts, np.ascontiguousarray(tris), rng.uniform(0, 1, size=(96, c)).astype(np.float32), h, w, c, np.arange(32))


def first_triangles(case, n):
    """The case cut to its first n triangles (the vertices stay)."""
    return case._replace(tris=np.ascontiguousarray(case.tris[:n]), degenerate=case.degenerate[case.degenerate < n])


def special_depths(case, seed, fraction=0.15, values=SPECIAL_DEPTHS, shift=-3.0):
    """About `fraction` of the vertices take a depth from `values`, three at a time: the vertices of one triangle in `fraction` of
    the triangles (a vertex belongs to one triangle only), so that a triangle of nothing but zeros and denormals exists.  The
    ordinary depths move by `shift`: under N(-3, 1) such a triangle can be the nearest somewhere and end up in the depth buffer."""
    rng = np.random.default_rng(seed)
    verts = case.verts.copy()
    verts[:, 2] += np.float32(shift)
    pick = case.tris[rng.uniform(size=case.tris.shape[0]) < fraction].ravel()
    verts[pick, 2] = rng.choice(np.asarray(values, np.float32), pick.size)
    return case._replace(verts=verts)


def bin_model(verts, tris, h, w, rows=None):
    """What k_tex_bin makes of float32 inputs, by its own bbox rule (ceil(min), floor(max), clipped to the image and the row band):
    counts [tile rows of the band, tile columns] triangles per tile; pairs = their sum; widths = the set of box widths after
    clipping to a tile (the texel loop's `rw`); max_wg_area = the largest box of tiles, width x height, that the triangles of one
    binning workgroup (256 consecutive ones) touch between them."""
    verts = np.asarray(verts, np.float32)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    r0, r1 = (0, h) if rows is None else rows
    x, y = verts[tris, 0], verts[tris, 1]
    x_min = np.maximum(np.ceil(x.min(1)).astype(np.int64), 0)
    x_max = np.minimum(np.floor(x.max(1)).astype(np.int64), w - 1)
    y_min = np.maximum(np.ceil(y.min(1)).astype(np.int64), 0)
    y_max = np.minimum(np.floor(y.max(1)).astype(np.int64), h - 1)
    on = (x_max >= x_min) & (y_max >= y_min) & ~((y_max < r0) | (y_min >= r1))
    tby0 = r0 // TILE
    nbx, nby = (w + TILE - 1) // TILE, (r1 - 1) // TILE - tby0 + 1
    bx0, bx1 = x_min // TILE, x_max // TILE
    by0, by1 = np.maximum(y_min, r0) // TILE - tby0, np.minimum(y_max, r1 - 1) // TILE - tby0
    # counts: +1 over every triangle's box of tiles, as a 2-D difference array
    diff = np.zeros((nby + 1, nbx + 1), np.int64)
    for sy, ys in ((1, by0[on]), (-1, by1[on] + 1)):
        for sx, xs in ((1, bx0[on]), (-1, bx1[on] + 1)):
            np.add.at(diff, (ys, xs), sy * sx)
    counts = diff.cumsum(0).cumsum(1)[:nby, :nbx]
    pairs = int(((bx1 - bx0 + 1) * (by1 - by0 + 1))[on].sum())
    assert pairs == int(counts.sum())
    # widths of the box inside each tile column it spans
    xa, xb, ca, cb = x_min[on], x_max[on], bx0[on], bx1[on]
    one = ca == cb
    widths = set((xb - xa + 1)[one].tolist()) | set((TILE - xa % TILE)[~one].tolist()) | set((xb % TILE + 1)[~one].tolist())
    if (cb - ca >= 2).any():
        widths.add(TILE)
    # workgroup boxes
    area = 0
    big = np.iinfo(np.int64).max
    for s in range(0, tris.shape[0], BIN_BLOCK):
        m = on[s:s + BIN_BLOCK]
        if not m.any():
            continue
        e = slice(s, s + BIN_BLOCK)
        bw = np.where(m, bx1[e], -1).max() - np.where(m, bx0[e], big).min() + 1
        bh = np.where(m, by1[e], -1).max() - np.where(m, by0[e], big).min() + 1
        area = max(area, int(bw * bh))
    return Bins(counts, pairs, widths, area)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, want, what=""):
    """got and want are the same float32 bit patterns (np.testing.assert_array_equal would take -0 for +0 and any NaN for any
    other)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = bits(got) != bits(want)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ bitwise, first at {at}: "
                             f"{got[at]!r} (0x{int(bits(got)[at]):08x}) != {want[at]!r} (0x{int(bits(want)[at]):08x})")
