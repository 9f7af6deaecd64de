"""
Yardsticks of the camera equalisation of topo4d_amd.projtex (k_pair_stats and the gains of k_projtex in csrc/t4d_projtex.hip), in
float64 on the host:

    view_samples(pos, nrm, coverage, view, H, W, photo, depth, ...)   steps 1..6 of one view over all texels: (accepted, cos, w, s)
    project_texture_gains(..., gains)                                 the whole t4d_project_texture_gains: (color, weight, count)
    pair_stats(pos, nrm, coverage, views, sizes, photos, depths, ...) the whole t4d_projtex_pair_stats: (count [V,V], sums [V,V,3])
    pair_stats_slow(...)                                              the same, texel by texel: a check of pair_stats on a tiny case

view_samples performs the kernel's operations in the kernel's order (as tests/projtex_ref.project_texture does, whose helpers it
borrows; numpy never fuses a multiply-add), so every output bit agrees.  The participation rule and the pair sums are a plain
double loop over the views.
"""
from __future__ import annotations

import numpy as np

from tests.projtex_ref import NEAR, _mat, camera_centre

SCALE = 65536.0


def _maps(pos, nrm):
    return tuple(a if a.dtype == np.float64 else a.astype(np.float32).astype(np.float64) for a in (np.asarray(pos), np.asarray(nrm)))


def view_samples(pos, nrm, coverage, view, H: int, W: int, photo, depth, power: int = 2, cos_min: float = 0.1, fade_px: float = 16.0,
                 depth_tol: float = 0.002, gain=None):
    """(ok bool [h,w], cos [h,w], w [h,w], s [h,w,3]) of one packed view record, photo [3,H,W] and depth [H,W]: whether steps 1..5
    accept the view at each texel, and its cosine, weight and sample (times gain [3] when given); only meaningful where ok"""
    pos, nrm = _maps(pos, nrm)
    photo = np.asarray(photo, dtype=np.float32).reshape(3, H, W)
    d = np.asarray(depth, dtype=np.float32).reshape(H, W).astype(np.float64)
    view = np.asarray(view, dtype=np.float32).reshape(-1)
    th, tw = pos.shape[:2]
    cos_min, fade_px, lim = float(cos_min), float(fade_px), 1.0 + float(depth_tol)
    X, Y, Z = pos[..., 0], pos[..., 1], pos[..., 2]
    nx, ny, nz = nrm[..., 0], nrm[..., 1], nrm[..., 2]
    with np.errstate(all="ignore"):
        nl = np.sqrt((nx * nx + ny * ny) + nz * nz)
        live = (np.asarray(coverage) != 0) & (nl > 0.0)
        nhx, nhy, nhz = nx / nl, ny / nl, nz / nl
        xmax, ymax = float(W - 1), float(H - 1)
        vm, pm = _mat(view, 0), _mat(view, 16)
        cx = ((pm(0, 0) * X + pm(0, 1) * Y) + pm(0, 2) * Z) + pm(0, 3)
        cy = ((pm(1, 0) * X + pm(1, 1) * Y) + pm(1, 2) * Z) + pm(1, 3)
        cw = ((pm(3, 0) * X + pm(3, 1) * Y) + pm(3, 2) * Z) + pm(3, 3)
        px = ((cx / cw + 1.0) * float(W) - 1.0) * 0.5
        py = ((cy / cw + 1.0) * float(H) - 1.0) * 0.5
        z = ((vm(2, 0) * X + vm(2, 1) * Y) + vm(2, 2) * Z) + vm(2, 3)
        ok = live & (z > NEAR)
        fx0, fy0 = np.floor(px), np.floor(py)
        ok &= (fx0 >= 0.0) & (fx0 + 1.0 <= xmax) & (fy0 >= 0.0) & (fy0 + 1.0 <= ymax)
        c = camera_centre(view)
        ex, ey, ez = c[0] - X, c[1] - Y, c[2] - Z
        el = np.sqrt((ex * ex + ey * ey) + ez * ez)
        cs = (nhx * (ex / el) + nhy * (ey / el)) + nhz * (ez / el)
        ok &= cs >= cos_min
        ix = np.where(ok, fx0, 0.0).astype(np.int64)
        iy = np.where(ok, fy0, 0.0).astype(np.int64)
        ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)           # (only read where ok: the clamp never acts there)
        for dd in (d[iy, ix], d[iy, ix1], d[iy1, ix], d[iy1, ix1]):
            ok &= (dd > 0.0) & (z <= dd * lim)
        w = np.ones((th, tw))
        for _ in range(int(power)):
            w = w * cs
        if fade_px > 0.0:
            m = np.minimum(np.minimum(px, xmax - px), np.minimum(py, ymax - py))
            f = m / fade_px
            w = np.where(f < 1.0, w * f, w)
        ok &= w > 0.0
        fx, fy = px - fx0, py - fy0
        gx, gy = 1.0 - fx, 1.0 - fy
        s = np.empty((th, tw, 3))
        for ch in range(3):
            q = photo[ch].astype(np.float64)
            a = gx * q[iy, ix] + fx * q[iy, ix1]
            b = gx * q[iy1, ix] + fx * q[iy1, ix1]
            s[..., ch] = gy * a + fy * b
            if gain is not None:
                s[..., ch] = s[..., ch] * float(gain[ch])
    return ok, cs, w, s


def project_texture_gains(pos, nrm, coverage, views, H: int, W: int, photos, depth, power: int = 2, cos_min: float = 0.1,
                          fade_px: float = 16.0, depth_tol: float = 0.002, mode: str = "weighted", gains=None):
    """(color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8) as tests/projtex_ref.project_texture gives them, every
    view's sample multiplied by gains[v] (float64 [V,3]; None: as they are)"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    photos, depth = np.asarray(photos, np.float32), np.asarray(depth, np.float32)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    th, tw = np.asarray(pos).shape[:2]
    best = {"weighted": False, "best": True}[mode]
    sw, sc, cnt = np.zeros((th, tw)), np.zeros((th, tw, 3)), np.zeros((th, tw), dtype=np.int64)
    with np.errstate(all="ignore"):
        for v in range(len(views)):
            ok, _, w, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depth[v], power, cos_min, fade_px, depth_tol,
                                       None if gains is None else gains[v])
            cnt += ok
            if best:
                take = ok & (w > sw)
                sw = np.where(take, w, sw)
                sc = np.where(take[..., None], s, sc)
            else:
                sw = np.where(ok, sw + w, sw)
                sc = np.where(ok[..., None], sc + w[..., None] * s, sc)
        if not best:
            sc = np.where((cnt > 0)[..., None], sc / sw[..., None], 0.0)
    return sc.astype(np.float32), sw.astype(np.float32), cnt.astype(np.uint8)


def taking_part(pos, nrm, coverage, views, sizes, photos, depths, power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002,
                stat_cos_min=0.5, stat_lo=0.02, stat_hi=0.98, gains=None):
    """(part bool [V,h,w], q int64 [V,h,w,3]): where each view takes part, and its integer sample there (0 elsewhere).  sizes
    [V] of (h, w); photos [V] of [3,h_v,w_v]; depths [V] of [h_v,w_v] (or [1,h_v,w_v])"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    part, q = [], []
    for v in range(len(views)):
        H, W = (int(x) for x in sizes[v])
        ok, cs, _, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depths[v], power, cos_min, fade_px, depth_tol,
                                    None if gains is None else gains[v])
        with np.errstate(all="ignore"):
            p = ok & (cs >= float(stat_cos_min)) & ((s >= float(stat_lo)) & (s <= float(stat_hi))).all(-1)
            qi = np.rint(np.where(p[..., None], s, 0.0) * SCALE).astype(np.int64)          # half to even, as llrint
        part.append(p)
        q.append(qi)
    return np.stack(part), np.stack(q)


def pair_stats(*args, **kw):
    """(count int64 [V,V], sums int64 [V,V,3]): over the texels where views i and j both take part, their number and the sum of
    view i's integer samples"""
    part, q = taking_part(*args, **kw)
    V = len(part)
    count, sums = np.zeros((V, V), np.int64), np.zeros((V, V, 3), np.int64)
    for i in range(V):
        for j in range(V):
            both = part[i] & part[j]
            count[i, j] = both.sum()
            sums[i, j] = q[i][both].sum(0)
    return count, sums


def pair_stats_slow(*args, **kw):
    """pair_stats texel by texel, as the rule is written down: for a tiny case only"""
    part, q = taking_part(*args, **kw)
    V, th, tw = part.shape
    count, sums = np.zeros((V, V), np.int64), np.zeros((V, V, 3), np.int64)
    for y in range(th):
        for x in range(tw):
            there = [v for v in range(V) if part[v, y, x]]
            for i in there:
                for j in there:
                    count[i, j] += 1
                    for c in range(3):
                        sums[i, j, c] += int(q[i, y, x, c])
    return count, sums
