"""
Yardsticks of the two-band projection of topo4d_amd.projtex (k_low_band and k_projtex_bands in csrc/t4d_projtex.hip), in float64
on the host:

    low_band(photos, depth, radius)                                    the whole t4d_projtex_low_band: low [V,3,H,W] float32
    project_bands(pos, nrm, coverage, views, H, W, photos, low, depth, ...)   the whole t4d_project_texture_bands:
                                                                       (low_color, weight, count, high, best_weight)
    twoband(...)                                                       low_band, project_bands and float32(low_color + high)

Both perform the kernels' operations in the kernels' order over all pixels / texels at once (numpy never fuses a multiply-add), so
every output bit agrees.  project_bands takes steps 1..6 from tests/projtex_ref.view_samples: once over the photograph for s, once
over its low band for l.
"""
from __future__ import annotations

import numpy as np

from tests.projtex_ref import view_samples


def low_band(photos, depth, radius: int):
    """low [V,3,H,W] float32 of photos [V,3,H,W] and depth [V,1,H,W] (the mask is depth > 0): A sums the row's taps k = -R .. R in
    ascending order where they lie in the image and on the mask (a tap elsewhere is skipped, never multiplied by 0), B sums A over
    the rows k = -R .. R inside the image, N counts the taps, low = B / N where N > 0 and 0 elsewhere"""
    photos = np.asarray(photos, dtype=np.float32)
    V, _, H, W = photos.shape
    mask = np.asarray(depth, dtype=np.float32).reshape(V, 1, H, W) > 0
    R = int(radius)
    I = photos.astype(np.float64)
    A, N1 = np.zeros((V, 3, H, W)), np.zeros((V, 1, H, W), dtype=np.int64)
    with np.errstate(all="ignore"):
        for k in range(-R, R + 1):
            lo, hi = max(0, -k), min(W, W - k)                   # the columns c with 0 <= c + k < W
            if lo >= hi:
                continue
            m = mask[..., lo + k:hi + k]
            A[..., lo:hi] = np.where(m, A[..., lo:hi] + I[..., lo + k:hi + k], A[..., lo:hi])
            N1[..., lo:hi] += m
        B, N = np.zeros((V, 3, H, W)), np.zeros((V, 1, H, W), dtype=np.int64)
        for k in range(-R, R + 1):
            lo, hi = max(0, -k), min(H, H - k)                   # the rows r with 0 <= r + k < H
            if lo >= hi:
                continue
            B[:, :, lo:hi] = B[:, :, lo:hi] + A[:, :, lo + k:hi + k]
            N[:, :, lo:hi] += N1[:, :, lo + k:hi + k]
        low = np.where(N > 0, B / np.maximum(N, 1).astype(np.float64), 0.0)
    return low.astype(np.float32)


def project_bands(pos, nrm, coverage, views, H: int, W: int, photos, low, depth, power: int = 2, cos_min: float = 0.1,
                  fade_px: float = 16.0, depth_tol: float = 0.002, gains=None):
    """(low_color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8, high [h,w,3] float32, best_weight [h,w] float32)"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    photos, low, depth = np.asarray(photos, np.float32), np.asarray(low, np.float32), np.asarray(depth, np.float32)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    th, tw = np.asarray(pos).shape[:2]
    sw, bw, cnt = np.zeros((th, tw)), np.zeros((th, tw)), np.zeros((th, tw), dtype=np.int64)
    sl, hb = np.zeros((th, tw, 3)), np.zeros((th, tw, 3))
    with np.errstate(all="ignore"):
        for v in range(len(views)):
            g = None if gains is None else gains[v]
            ok, _, w, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depth[v], power, cos_min, fade_px, depth_tol, g)
            ok_l, _, w_l, l = view_samples(pos, nrm, coverage, views[v], H, W, low[v], depth[v], power, cos_min, fade_px, depth_tol, g)
            assert np.array_equal(ok, ok_l) and np.array_equal(w[ok], w_l[ok])
            cnt += ok
            sw = np.where(ok, sw + w, sw)
            sl = np.where(ok[..., None], sl + w[..., None] * l, sl)
            take = ok & (w > bw)
            bw = np.where(take, w, bw)
            hb = np.where(take[..., None], s - l, hb)
        sl = np.where((cnt > 0)[..., None], sl / sw[..., None], 0.0)
    return sl.astype(np.float32), sw.astype(np.float32), cnt.astype(np.uint8), hb.astype(np.float32), bw.astype(np.float32)


def twoband(pos, nrm, coverage, views, H: int, W: int, photos, depth, radius: int, **kw):
    """(color [h,w,3] float32, weight, count) of mode "twoband" for views of one size: color = float32(low_color + high)"""
    lc, weight, count, high, _ = project_bands(pos, nrm, coverage, views, H, W, photos, low_band(photos, depth, radius), depth, **kw)
    return lc + high, weight, count
