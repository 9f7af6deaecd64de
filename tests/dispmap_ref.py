"""The displacement-map rules of include/topo4d_raster.h (t4d_disp_quantize, t4d_disp_smooth, t4d_disp_normals) and the 16-bit
push-pull fill (t4d_texture_fill16, texfinish.fill16_islands) as numpy: the yardstick of tests/test_gpu_dispmap.py and the subject
of tests/test_dispmap_host.py.

Every step is one whole-image operation in int64 or float64: no tiles, no halos, nothing shared with the kernels.  numpy's float64
operations round once each and np.rint rounds half to even, which is the arithmetic the header prescribes."""
import numpy as np

ZERO, STEPS = 32768, 32767
WEIGHTS = (1, 4, 6, 4, 1)


def quantize(disp, hit, dist):
    """(code int32 [h,w], has uint8 [h,w])"""
    disp = np.asarray(disp, np.float32)
    ok = (np.asarray(hit) != 0) & np.isfinite(disp)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint((disp.astype(np.float64) / np.float64(dist)) * 32767.0)
    q = np.clip(np.where(ok, q, 0.0), -32767.0, 32767.0)
    return (ZERO + q.astype(np.int64)).astype(np.int32), ok.astype(np.uint8)


def _shift(a, j, i, fill=0):
    """b[y][x] = a[y+j][x+i], `fill` outside the image"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = slice(max(j, 0), h + min(j, 0)), slice(max(-j, 0), h + min(-j, 0))
    xs, xd = slice(max(i, 0), w + min(i, 0)), slice(max(-i, 0), w + min(-i, 0))
    out[yd, xd] = a[ys, xs]
    return out


def smooth(code, has, labels, rounds):
    """int32 [h,w] after `rounds` rounds"""
    assert 0 <= rounds <= 8
    cur = np.asarray(code).astype(np.int64) & 0xFFFF
    key = np.where(np.asarray(has) != 0, np.asarray(labels).astype(np.int64), 0)       # 0: the texel is nobody's tap
    centre = key != 0
    for _ in range(rounds):
        S, Wt = np.zeros_like(cur), np.zeros_like(cur)
        for j in range(-2, 3):
            for i in range(-2, 3):
                wgt = WEIGHTS[j + 2] * WEIGHTS[i + 2]
                counts = centre & (_shift(key, j, i) == key)
                S += np.where(counts, wgt * _shift(cur, j, i), 0)
                Wt += np.where(counts, wgt, 0)
        cur = np.where(centre, (2 * S + Wt) // np.maximum(2 * Wt, 1), cur)
    return cur.astype(np.int32)


def _slope(code, pos, key, axis, unit):
    """the slope along image axis 0 (y) or 1 (x), float64 [h,w]; 0 where the texel has no value"""
    h, w = key.shape
    step = (1, 0) if axis == 0 else (0, 1)
    idx = np.indices((h, w))
    centre = key != 0
    plus = centre & (_shift(key, step[0], step[1]) == key)
    minus = centre & (_shift(key, -step[0], -step[1]) == key)
    p = [idx[0] + np.where(plus, step[0], 0), idx[1] + np.where(plus, step[1], 0)]
    m = [idx[0] - np.where(minus, step[0], 0), idx[1] - np.where(minus, step[1], 0)]
    T = pos[p[0], p[1]].astype(np.float64) - pos[m[0], m[1]].astype(np.float64)
    a = np.sqrt((T[..., 0] * T[..., 0] + T[..., 1] * T[..., 1]) + T[..., 2] * T[..., 2])
    dc = (code[p[0], p[1]] - code[m[0], m[1]]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (dc * np.float64(unit)) / a
    return np.where(centre & (plus | minus) & (a != 0.0), s, 0.0)


def _encode(v):
    with np.errstate(invalid="ignore"):
        q = np.rint((v * 0.5 + 0.5) * 65535.0)
    return np.where(q >= 0.0, np.minimum(q, 65535.0), 0.0).astype(np.int32)            # a NaN gives 0


def normals(code, has, labels, pos, unit):
    """int32 [h,w,3]"""
    code = np.asarray(code).astype(np.int64) & 0xFFFF
    pos = np.asarray(pos, np.float32)
    key = np.where(np.asarray(has) != 0, np.asarray(labels).astype(np.int64), 0)
    sx, sy = _slope(code, pos, key, 1, unit), _slope(code, pos, key, 0, unit)
    length = np.sqrt((sx * sx + sy * sy) + 1.0)
    return np.stack([_encode(-sx / length), _encode(sy / length), _encode(1.0 / length)], -1)


def decode_normals(normal):
    """float64 [h,w,3]: the stored components back in -1..1"""
    return np.asarray(normal).astype(np.float64) / 65535.0 * 2.0 - 1.0


# ---- the push-pull fill on 16-bit samples: colours are int64 in units of 1/256 of a 16-bit step ------------------------------
def _pull(c, v):
    h, w = v.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    cp = np.zeros((2 * h2, 2 * w2, c.shape[2]), np.int64)
    vp = np.zeros((2 * h2, 2 * w2), np.int64)                   # children outside the level do not exist
    cp[:h, :w], vp[:h, :w] = c, v
    blocks = lambda a: a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    s, n = blocks(cp), blocks(vp)[..., None]
    return np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), 0), n[..., 0] > 0


def _push(P, h, w):
    y, x = np.mgrid[0:h, 0:w]
    px, py = x >> 1, y >> 1
    nx = np.clip(px + np.where(x & 1, 1, -1), 0, P.shape[1] - 1)
    ny = np.clip(py + np.where(y & 1, 1, -1), 0, P.shape[0] - 1)
    return (9 * P[py, px] + 3 * P[py, nx] + 3 * P[ny, px] + P[ny, nx] + 8) >> 4


def fill16(image, valid, domain=None):
    """(image int32, filled uint8 [h,w]) after t4d_texture_fill16's rule"""
    image = np.asarray(image, np.int32)
    v0 = np.asarray(valid) != 0
    assert v0.shape == image.shape[:2]
    samples = image.reshape(v0.shape + (-1,)).astype(np.int64) & 0xFFFF
    dom = np.ones_like(v0) if domain is None else np.asarray(domain) != 0
    cs, vs = [np.where(v0[..., None], 256 * samples, 0)], [v0]
    while vs[-1].shape != (1, 1):
        c, v = _pull(cs[-1], vs[-1])
        cs.append(c)
        vs.append(v)
    if not vs[-1][0, 0]:                                        # no valid texel at all
        return samples.astype(np.int32).reshape(image.shape), np.zeros(v0.shape, np.uint8)
    P = cs[-1]
    for k in range(len(cs) - 2, -1, -1):
        P = np.where(vs[k][..., None], cs[k], _push(P, *vs[k].shape))
    take = dom & ~v0
    out = np.where(take[..., None], (P + 128) >> 8, samples)
    return out.astype(np.int32).reshape(image.shape), take.astype(np.uint8)


def fill16_islands(image, valid, labels):
    """(image, filled): fill16 per label i >= 1 that holds a valid texel and a hole, from that island's valid texels alone"""
    image = np.asarray(image, np.int32)
    v = np.asarray(valid) != 0
    labels = np.asarray(labels, np.uint8)
    out, filled = image.copy(), np.zeros(v.shape, np.uint8)
    for i in range(1, int(labels.max()) + 1 if labels.size else 1):
        isl = labels == i
        if not (isl & v).any() or not (isl & ~v).any():
            continue
        o, f = fill16(image, v & isl, isl)
        out[f != 0] = o[f != 0]
        filled |= f
    return out, filled


def finish(labels, pos, disp, hit, dist, fill=False, smooth_rounds=0, with_normals=False):
    """dispmap.finish from the maps it derives from the mesh (labels: projtex.island_labels, pos: projtex.surface_maps)"""
    code, has = quantize(disp, hit, dist)
    filled = np.zeros(has.shape, np.uint8)
    if fill:
        code, filled = fill16_islands(code, has, labels)
        has = has | filled
    if smooth_rounds:
        code = smooth(code, has, labels, smooth_rounds)
    out = {"code": code, "has": has, "filled": filled}
    if with_normals:
        out["normal"] = normals(code, has, labels, pos, np.float64(dist) / 32767.0)
    return out
