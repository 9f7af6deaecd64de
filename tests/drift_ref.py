"""The drift matcher's rule (include/topo4d_raster.h: t4d_drift_match) and topo4d_amd.drift's flow and metric, restated in numpy.
Written apart from the kernel's structure: one whole-image Hamming map per candidate displacement, box sums over cumulative sums,
and the best and the second by one pass over the candidates in the order of the tie rule.  Everything in match is integer
arithmetic and flow / metric are float64 operations in the module's order, so the device results must equal these bit for bit."""
from __future__ import annotations

import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def luma(image: np.ndarray) -> np.ndarray:
    image = np.asarray(image, np.uint8)
    if image.ndim == 2 or image.shape[2] == 1:
        return image.reshape(image.shape[0], image.shape[1]).copy()
    r, g, b = (image[..., k].astype(np.int64) for k in range(3))
    return ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)


def popcount(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x).astype(np.int64)
    return _POP[x.view(np.uint8).reshape(x.shape + (8,))].sum(-1)


def census(L: np.ndarray, valid: np.ndarray, labels: np.ndarray):
    """(C uint64 [h,w], ok bool [h,w]): the census word and "census-valid" of every texel; C is 0 where ok is False"""
    h, w = L.shape
    C, ok = np.zeros((h, w), np.uint64), np.zeros((h, w), bool)
    if h < 7 or w < 7:
        return C, ok
    Li, v = L.astype(np.int64), np.asarray(valid) != 0
    inner = (slice(3, h - 3), slice(3, w - 3))
    good = np.asarray(labels)[inner] != 0
    word = np.zeros((h - 6, w - 6), np.uint64)
    k = 0
    for j in range(-3, 4):
        for i in range(-3, 4):
            sl = (slice(3 + j, h - 3 + j), slice(3 + i, w - 3 + i))
            good = good & v[sl]
            if j == 0 and i == 0:
                continue
            word |= (Li[sl] < Li[inner]).astype(np.uint64) << np.uint64(k)
            k += 1
    ok[inner] = good
    C[inner] = np.where(good, word, np.uint64(0))
    return C, ok


def blocks(h: int, w: int, B: int, S: int):
    return ((h - B) // S + 1 if h >= B else 0), ((w - B) // S + 1 if w >= B else 0)


def box_sums(m: np.ndarray, B: int, S: int) -> np.ndarray:
    """int64 [nby,nbx]: the sum of m over every block"""
    h, w = m.shape
    nby, nbx = blocks(h, w, B, S)
    I = np.zeros((h + 1, w + 1), np.int64)
    I[1:, 1:] = m.astype(np.int64).cumsum(0).cumsum(1)
    y, x = np.arange(nby) * S, np.arange(nbx) * S
    return I[np.ix_(y + B, x + B)] - I[np.ix_(y, x + B)] - I[np.ix_(y + B, x)] + I[np.ix_(y, x)]


def costs(La, va, Lb, vb, labels, B: int, S: int, R: int):
    """(c, n int64 [2R+1,2R+1,nby,nbx]) indexed by (dy + R, dx + R)"""
    h, w = La.shape
    nby, nbx = blocks(h, w, B, S)
    D = 2 * R + 1
    Ca, oka = census(La, va, labels)
    Cb, okb = census(Lb, vb, labels)
    lab = np.asarray(labels)
    c, n = np.zeros((D, D, nby, nbx), np.int64), np.zeros((D, D, nby, nbx), np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ya, yb = max(0, -dy), min(h, h - dy)                # rows of p with p + d inside
            xa, xb = max(0, -dx), min(w, w - dx)
            pair, ham = np.zeros((h, w), bool), np.zeros((h, w), np.int64)
            if ya < yb and xa < xb:
                p, q = (slice(ya, yb), slice(xa, xb)), (slice(ya + dy, yb + dy), slice(xa + dx, xb + dx))
                pr = oka[p] & okb[q] & (lab[p] == lab[q])
                pair[p] = pr
                ham[p] = np.where(pr, popcount(Ca[p] ^ Cb[q]), 0)
            n[dy + R, dx + R] = box_sums(pair, B, S)
            c[dy + R, dx + R] = box_sums(ham, B, S)
    return c, n


def _first(c, n, R: int, allowed):
    """per block the first candidate of the rule's order among `allowed` [D,D,nby,nbx]: (found, dy, dx, c, n)"""
    shape = c.shape[2:]
    found = np.zeros(shape, bool)
    bdy, bdx = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    bc, bn = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    order = sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda d: (d[0] * d[0] + d[1] * d[1], d[0], d[1]))
    for dy, dx in order:                                         # ties keep the earlier candidate: only strictly smaller replaces
        cc, nn, al = c[dy + R, dx + R], n[dy + R, dx + R], allowed[dy + R, dx + R]
        take = al & (~found | (cc * bn < bc * nn))
        found |= take
        bdy, bdx = np.where(take, dy, bdy), np.where(take, dx, bdx)
        bc, bn = np.where(take, cc, bc), np.where(take, nn, bn)
    return found, bdy, bdx, bc, bn


def match(La, va, Lb, vb, labels, B: int, S: int, R: int, min_count: int) -> np.ndarray:
    """int32 [nby,nbx,16]: the table of t4d_drift_match"""
    La, Lb = luma(La), luma(Lb)
    h, w = La.shape
    nby, nbx = blocks(h, w, B, S)
    out = np.zeros((nby, nbx, 16), np.int32)
    if nby == 0 or nbx == 0:
        return out
    c, n = costs(La, va, Lb, vb, labels, B, S, R)
    adm = n >= min_count
    found, dy, dx, bc, bn = _first(c, n, R, adm)
    off = np.arange(-R, R + 1)
    far = (np.abs(off[:, None, None, None] - dy[None, None]) > 1) | (np.abs(off[None, :, None, None] - dx[None, None]) > 1)
    has2, _, _, sc, sn = _first(c, n, R, adm & far & found[None, None])
    out[..., 0], out[..., 1] = np.where(found, dy, 0), np.where(found, dx, 0)
    out[..., 2], out[..., 3] = np.where(found, bc, 0), np.where(found, bn, 0)
    by, bx = np.mgrid[0:nby, 0:nbx]
    for k, (ey, ex) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
        ny, nx = dy + ey, dx + ex
        inside = found & (np.abs(ny) <= R) & (np.abs(nx) <= R)
        iy, ix = np.clip(ny + R, 0, 2 * R), np.clip(nx + R, 0, 2 * R)
        ok = inside & adm[iy, ix, by, bx]
        out[..., 4 + 2 * k] = np.where(ok, c[iy, ix, by, bx], 0)
        out[..., 5 + 2 * k] = np.where(ok, n[iy, ix, by, bx], 0)
    out[..., 12], out[..., 13] = np.where(has2, sc, 0), np.where(has2, sn, 0)
    return out


def flow(table: np.ndarray, radius: int, ratio: float = 0.8):
    """(d float64 [nby,nbx,2], kept bool [nby,nbx]) by topo4d_amd.drift's rule, in its order of operations"""
    t = table.astype(np.float64)
    q = lambda k: t[..., k] / np.maximum(t[..., k + 1], 1.0)
    has = lambda k: table[..., k + 1] > 0
    q0, q2 = q(2), q(12)
    kept = has(2) & has(12) & (table[..., 12] > 0) & (q0 <= ratio * q2)
    kept &= np.maximum(np.abs(table[..., 0]), np.abs(table[..., 1])) < radius
    d = []
    for axis, k in ((0, 4), (1, 8)):
        qm, qp = q(k), q(k + 2)
        den = (qm - 2.0 * q0) + qp
        ok = has(2) & has(k) & has(k + 2) & (den > 0.0)
        off = np.clip((qm - qp) / (2.0 * np.where(ok, den, 1.0)), -0.5, 0.5)
        d.append(t[..., axis] + np.where(ok, off, 0.0))
    return np.stack(d, -1), kept


def length(d: np.ndarray) -> np.ndarray:
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])


def metric(d, kept, pos, labels, B: int, S: int):
    """(drift float64 [nby,nbx], kept) by topo4d_amd.drift's rule"""
    h, w = labels.shape
    nby, nbx = blocks(h, w, B, S)
    cy, cx = np.meshgrid(np.arange(nby) * S + B // 2, np.arange(nbx) * S + B // 2, indexing="ij")
    p = np.asarray(pos).astype(np.float64)
    jx = (p[cy, cx + 1] - p[cy, cx - 1]) * 0.5
    jy = (p[cy + 1, cx] - p[cy - 1, cx]) * 0.5
    v = jx * d[..., 1:2] + jy * d[..., 0:1]
    drift = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    lab = labels[cy, cx]
    same = (lab != 0) & (labels[cy, cx + 1] == lab) & (labels[cy, cx - 1] == lab) & (labels[cy + 1, cx] == lab) & (labels[cy - 1, cx] == lab)
    return drift, kept & same


# ---- textures of the tests ---------------------------------------------------------------------------------------------------
def smooth_random(h: int, w: int, seed: int = 0, passes: int = 2) -> np.ndarray:
    """float64 [h,w] in [0, 1]: white noise under `passes` periodic 3x3 box blurs, stretched to the full range"""
    f = np.random.default_rng(seed).random((h, w))
    for _ in range(passes):
        f = sum(np.roll(np.roll(f, j, 0), i, 1) for j in (-1, 0, 1) for i in (-1, 0, 1)) / 9.0
    return (f - f.min()) / (f.max() - f.min())


def to_u8(f: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(f * 255.0), 0, 255).astype(np.uint8)


def shift_periodic(f: np.ndarray, dy: float, dx: float) -> np.ndarray:
    """g(p + d) = f(p) on the periodic image by bilinear resampling: a feature of f at p lies at p + (dy, dx) in g"""
    h, w = f.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    sy, sx = y - dy, x - dx
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    fy, fx = sy - y0, sx - x0
    at = lambda yy, xx: f[yy % h, xx % w]
    return (at(y0, x0) * (1 - fy) * (1 - fx) + at(y0, x0 + 1) * (1 - fy) * fx + at(y0 + 1, x0) * fy * (1 - fx) + at(y0 + 1, x0 + 1) * fy * fx)
