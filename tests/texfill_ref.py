"""The push-pull hole fill of include/topo4d_raster.h (t4d_texture_fill) and texfinish.fill_islands as numpy: the yardstick of
tests/test_gpu_texfill.py and the subject of tests/test_texfill_host.py.

Every level is one array and every step one whole-level operation: no tiles, no halos, nothing shared with
csrc/t4d_texfill.hip.  Colours are int64 in units of 1/256 of an 8-bit step."""
import numpy as np


def _pull(c, v):
    """the next level of colours c [h,w,ch] (0 where not valid) and valid v [h,w]: (2 s + n) / (2 n) per 2x2 block"""
    h, w = v.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    cp = np.zeros((2 * h2, 2 * w2, c.shape[2]), np.int64)
    vp = np.zeros((2 * h2, 2 * w2), np.int64)                   # children outside the level do not exist
    cp[:h, :w], vp[:h, :w] = c, v
    blocks = lambda a: a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    s, n = blocks(cp), blocks(vp)[..., None]
    return np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), 0), n[..., 0] > 0


def _push(P, h, w):
    """the completed level P bilinearly enlarged to [h,w]: taps 9 : 3 : 3 : 1 on the parent and its neighbours towards the texel"""
    y, x = np.mgrid[0:h, 0:w]
    px, py = x >> 1, y >> 1
    nx = np.clip(px + np.where(x & 1, 1, -1), 0, P.shape[1] - 1)
    ny = np.clip(py + np.where(y & 1, 1, -1), 0, P.shape[0] - 1)
    return (9 * P[py, px] + 3 * P[py, nx] + 3 * P[ny, px] + P[ny, nx] + 8) >> 4


def pyramid(image, valid):
    """([C0, C1, ...], [V0, V1, ...]) of the pull, down to the 1x1 level"""
    image = np.asarray(image, np.uint8)
    v = np.asarray(valid) != 0
    c = np.where(v[..., None], 256 * image.reshape(v.shape + (-1,)).astype(np.int64), 0)
    cs, vs = [c], [v]
    while vs[-1].shape != (1, 1):
        c, v = _pull(cs[-1], vs[-1])
        cs.append(c)
        vs.append(v)
    return cs, vs


def completed(image, valid):
    """level 0 after the push, int64 [h,w,ch] in units of 1/256; None without any valid texel.  (It does not depend on the domain:
    a test that fills one image under several domains computes it once.)"""
    cs, vs = pyramid(image, valid)
    if not vs[-1][0, 0]:
        return None
    P = cs[-1]
    for k in range(len(cs) - 2, -1, -1):
        P = np.where(vs[k][..., None], cs[k], _push(P, *vs[k].shape))
    return P


def fill(image, valid, domain=None, level0=False):
    """(image, filled uint8 [h,w]) after t4d_texture_fill's rule; level0: completed(image, valid) of an earlier call"""
    image = np.asarray(image, np.uint8)
    v0 = np.asarray(valid) != 0
    assert v0.shape == image.shape[:2]
    dom = np.ones_like(v0) if domain is None else np.asarray(domain) != 0
    P = completed(image, v0) if level0 is False else level0
    if P is None:                                               # no valid texel at all
        return image.copy(), np.zeros(v0.shape, np.uint8)
    take = dom & ~v0
    out = np.where(take[..., None], (P + 128) >> 8, image.reshape(v0.shape + (-1,)).astype(np.int64))
    return out.astype(np.uint8).reshape(image.shape), take.astype(np.uint8)


def fill_islands(image, valid, labels):
    """(image, filled): fill per label i >= 1 that holds a valid texel and a hole, from that island's valid texels alone"""
    image = np.asarray(image, np.uint8)
    v = np.asarray(valid) != 0
    labels = np.asarray(labels, np.uint8)
    out, filled = image.copy(), np.zeros(v.shape, np.uint8)
    for i in range(1, int(labels.max()) + 1 if labels.size else 1):
        isl = labels == i
        if not (isl & v).any() or not (isl & ~v).any():
            continue
        o, f = fill(image, v & isl, isl)
        out[f != 0] = o[f != 0]
        filled |= f
    return out, filled


def nearest_fill(image, valid):
    """every texel takes the nearest valid texel (brute force; ties to the smallest (y', x')): what the fill is compared with"""
    image = np.asarray(image)
    v = np.asarray(valid) != 0
    ys, xs = np.nonzero(v)
    out = image.copy()
    for y, x in zip(*np.nonzero(~v)):
        k = np.argmin((ys - y) ** 2 + (xs - x) ** 2)
        out[y, x] = image[ys[k], xs[k]]
    return out
