"""The rules of texture finishing (include/topo4d_raster.h) as a numpy brute force: the yardstick of tests/test_gpu_texfinish.py.

pad visits every offset of the disc and keeps the lexicographic minimum of (d^2, y', x') - no row / column decomposition, nothing
shared with csrc/t4d_texfinish.hip; erode runs its rounds one after another; halve follows its formula."""
import numpy as np


def coverage_from_depth(depth):
    return (np.asarray(depth, np.float32) > np.float32(-999999.0)).astype(np.uint8)


def quantize(x):
    return (np.asarray(x, np.float32) * 255).astype(np.uint8)


def erode(cov, rounds):
    c = np.asarray(cov) != 0
    for _ in range(rounds):
        p = np.pad(c, 1, constant_values=True)                 # neighbours outside the image count as covered
        c = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return c.astype(np.uint8)


def pad(image, cov, radius):
    """(image, coverage) after t4d_texture_pad's rule.  One pass per offset of the disc, in descending order of (d^2, dy, dx):
    a later, lexicographically smaller offset overwrites an earlier one, so every texel ends with its smallest."""
    image = np.asarray(image)                                  # any dtype: an image of texel numbers gives the source map
    c = np.asarray(cov) != 0
    h, w = c.shape
    R = int(radius)
    offsets = sorted(((dx * dx + dy * dy, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)
                      if dx * dx + dy * dy <= R * R), reverse=True)
    out, out_cov = image.copy(), c.copy()
    for _, dy, dx in offsets:                                  # texel (y, x) looks at (y + dy, x + dx)
        y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        if y0 >= y1 or x0 >= x1:
            continue
        dst = (slice(y0, y1), slice(x0, x1))
        src = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
        take = c[src] & ~c[dst]
        out[dst][take] = image[src][take]
        out_cov[dst] |= take
    return out, out_cov.astype(np.uint8)


def halve(image, cov):
    image = np.asarray(image, np.uint8)
    c = (np.asarray(cov) != 0)
    h, w = c.shape
    assert h % 2 == 0 and w % 2 == 0
    img = image.reshape(h, w, -1).astype(np.int64)
    m = c.astype(np.int64)[..., None]
    blocks = lambda a: a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
    s, cnt = blocks(img * m), blocks(m)
    out = np.where(cnt > 0, (2 * s + cnt) // np.maximum(2 * cnt, 1), 0).astype(np.uint8)
    return out.reshape((h // 2, w // 2) + image.shape[2:]), (cnt[..., 0] > 0).astype(np.uint8)


def finish(image, cov, pad_radius=0, erode_rounds=0, sizes=()):
    image = np.asarray(image, np.uint8)
    res = image.shape[0]
    cov0 = erode(cov, erode_rounds)
    out = {res: pad(image, cov0, pad_radius)[0]}
    cur, cur_cov = image, cov0
    while sizes and cur.shape[0] > min(sizes):
        cur, cur_cov = halve(cur, cur_cov)
        if cur.shape[0] in sizes:
            out[cur.shape[0]] = pad(cur, cur_cov, pad_radius)[0]
    return out
