"""The temporal fusion rule (include/topo4d_raster.h: t4d_seqtex_select, t4d_seqtex_complete), restated in numpy.  Written apart
from the kernel's structure: select sorts every texel's samples over the frames with the invalid ones keyed above 255 and takes the
rank with take_along_axis; complete is a handful of whole-image masks.  Integer arithmetic, so the device results must equal these
bit for bit."""
from __future__ import annotations

import numpy as np


def select(images, valids, num: int = 1, den: int = 2):
    """(image uint8 [h,w,c] or [h,w] as given, count uint8 [h,w]) of t4d_seqtex_select for lists of images and validities"""
    shape = np.asarray(images[0]).shape
    v = np.stack([np.asarray(x) != 0 for x in valids])                                   # [F,h,w]
    img = np.stack([np.asarray(x).reshape(v.shape[1], v.shape[2], -1) for x in images]).astype(np.int64)
    n = v.sum(0)
    k = (np.maximum(n - 1, 0) * num) // den
    srt = np.sort(np.where(v[..., None], img, 256), axis=0)                              # invalid samples last
    out = np.take_along_axis(srt, np.broadcast_to(k[None, ..., None], (1,) + img.shape[1:]), 0)[0]
    return np.where(n[..., None] > 0, out, 0).astype(np.uint8).reshape(shape), n.astype(np.uint8)


def spread(images, valids):
    """uint8, the shape of one image: select at (3, 4) minus select at (1, 4), 0 where count < 4"""
    hi, n = select(images, valids, 3, 4)
    lo, _ = select(images, valids, 1, 4)
    return np.where((n >= 4).reshape(n.shape + (1,) * (hi.ndim - 2)), hi - lo, 0).astype(np.uint8)


def complete(image, valid, base, count, min_count: int = 1, min_votes: int = 3, tol: int = 255):
    """(image uint8 of the given shape, source uint8 [h,w]) of t4d_seqtex_complete"""
    image, base, count = np.asarray(image), np.asarray(base), np.asarray(count).astype(np.int64)
    h, w = count.shape
    v = np.asarray(valid) != 0
    far = np.abs(image.reshape(h, w, -1).astype(np.int64) - base.reshape(h, w, -1)).max(-1)
    own = v & ~((count >= min_votes) & (far > tol))
    fused = ~own & (count >= min_count)
    source = np.where(own, 1, np.where(fused, np.where(v, 3, 2), 0)).astype(np.uint8)
    pick = source.reshape((h, w) + (1,) * (image.ndim - 2))
    return np.where(pick == 1, image, np.where(pick != 0, base, 0)).astype(np.uint8), source


def select_brute(images, valids, num: int = 1, den: int = 2):
    """select as a plain triple loop over the texels and channels: what the sort restates"""
    F = len(images)
    h, w = np.asarray(valids[0]).shape
    img = [np.asarray(x).reshape(h, w, -1) for x in images]
    c = img[0].shape[2]
    out, count = np.zeros((h, w, c), np.uint8), np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            frames = [t for t in range(F) if valids[t][y][x] != 0]
            count[y, x] = len(frames)
            for ch in range(c):
                if frames:
                    out[y, x, ch] = sorted(int(img[t][y, x, ch]) for t in frames)[((len(frames) - 1) * num) // den]
    return out.reshape(np.asarray(images[0]).shape), count
