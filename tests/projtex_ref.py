"""
Yardsticks of topo4d_amd.projtex (csrc/t4d_projtex.hip), in float64 on the host:

    view_samples(pos, nrm, coverage, view, H, W, photo, depth, ...)        steps 1..6 of one view over all texels: (accepted, cos, w, s)
    project_texture(pos, nrm, coverage, views, H, W, photos, depth, ...)   the whole t4d_project_texture[_gains]: (color, weight, count)
    camera_centre(view)                                                    -R^T t of a packed view record, in the kernel's order
    visible_brute_force(points, view, vertices, tris)                      an independent visibility: the segment from the camera
                                                                           centre to each point against every triangle

view_samples, the one restatement of steps 1..6, performs the kernel's operations in the kernel's order over all texels at once
(numpy never fuses a multiply-add), so every output bit agrees; the equalisation and two-band yardsticks are built on it too.  visible_brute_force shares no code with it: Moller-Trumbore in float64.
"""
from __future__ import annotations

import numpy as np

NEAR = 0.01


def _mat(view, lo):
    m = np.asarray(view, dtype=np.float32).reshape(-1)[lo:lo + 16].astype(np.float64)
    return lambda r, c: m[c * 4 + r]


def camera_centre(view):
    vm = _mat(view, 0)
    t0, t1, t2 = vm(0, 3), vm(1, 3), vm(2, 3)
    return np.array([-((vm(0, j) * t0 + vm(1, j) * t1) + vm(2, j) * t2) for j in range(3)], dtype=np.float64)


def view_samples(pos, nrm, coverage, view, H: int, W: int, photo, depth, power: int = 2, cos_min: float = 0.1, fade_px: float = 16.0,
                 depth_tol: float = 0.002, gain=None):
    """(ok bool [h,w], cos [h,w], w [h,w], s [h,w,3]) of one packed view record, photo [3,H,W] and depth [H,W]: whether steps 1..5
    accept the view at each texel, and its cosine, weight and sample (times gain [3] when given); only meaningful where ok.  pos /
    nrm [h,w,3] are taken as float32 (the kernel's inputs; float64 maps are taken as they are)"""
    pos, nrm = (a if a.dtype == np.float64 else a.astype(np.float32).astype(np.float64) for a in (np.asarray(pos), np.asarray(nrm)))
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


def project_texture(pos, nrm, coverage, views, H: int, W: int, photos, depth, power: int = 2, cos_min: float = 0.1,
                    fade_px: float = 16.0, depth_tol: float = 0.002, mode: str = "weighted", gains=None):
    """(color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8) of pos / nrm [h,w,3], coverage [h,w], packed views [V,40],
    photos [V,3,H,W] and depth [V,1,H,W]: step 7 over view_samples, every view's sample multiplied by gains[v] (float64 [V,3];
    None: as they are)"""
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


def visible_brute_force(points, view, vertices, tris, eps: float = 1e-4):
    """bool [n]: no triangle crosses the open segment from the camera centre to points[i] (Moller-Trumbore, float64).  A hit
    counts when it lies in the triangle (edges included, to 1e-12) and ends before the point by more than `eps` of the segment (the points
    are float32 and sit on their own triangle only to rounding)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(vertices, dtype=np.float64)
    vm = np.asarray(view, dtype=np.float32)[:16].astype(np.float64).reshape(4, 4).T          # world -> camera
    eye = -vm[:3, :3].T @ vm[:3, 3]
    d = p - eye
    seen = np.ones(len(p), dtype=bool)
    for i0, i1, i2 in np.asarray(tris, dtype=np.int64):
        e1, e2 = v[i1] - v[i0], v[i2] - v[i0]
        h = np.cross(d, e2)
        det = h @ e1
        s = eye - v[i0]
        q = np.cross(s, e1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            bu, bv, t = (h @ s) * inv, (d @ q) * inv, (q @ e2) * inv
        hit = (np.abs(det) > 1e-14) & (bu >= -1e-12) & (bv >= -1e-12) & (bu + bv <= 1 + 1e-12) & (t > 0) & (t < 1.0 - eps)
        seen &= ~hit
    return seen
