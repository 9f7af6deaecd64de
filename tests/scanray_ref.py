"""
The yardstick of the ray query (t4d_closest_raycast, csrc/t4d_closest.hip): the hit rule of include/topo4d_raster.h applied in
float64 numpy to every (ray, triangle) pair.  It fixes, and the kernel repeats operation for operation:

  dot3(u, v) = (u0 v0 + u1 v1) + u2 v2 and x = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0), every product, sum and difference
  rounded (no fused multiply-add).  For ray (o, d) and triangle (a, b, c), in this order:
    1. e1 = b - a, e2 = c - a, pv = d x e2, det = dot3(e1, pv); det == 0 is a miss.
    2. same_side: det >= 0 is a miss (only triangles whose normal (b - a) x (c - a) points along d count).
    3. tv = o - a, u = dot3(tv, pv) / det; a miss unless u >= 0 and u <= 1.
    4. qv = tv x e1, v = dot3(d, qv) / det; a miss unless v >= 0 and u + v <= 1.
    5. t = dot3(e2, qv) / det; a miss unless t >= t_lo and t <= t_hi.
    6. Box condition: on every axis the computed point p = o + t d satisfies p >= min(a, b, c) - margin and
       p <= max(a, b, c) + margin, with the margin of the index's grid (grid_margin below restates closest_grid).
  Quotients, not a reciprocal; a NaN fails every comparison.
  Choice: the smallest |t|, then t >= 0 before t < 0, then the lowest triangle index.
  A miss is t = 0, prim = -1, uv = 0; a ray with a non-finite origin or direction, an all-zero direction, or t_lo > t_hi misses
  every triangle.
"""
import math

import numpy as np


def mean_extent(vertices, faces):
    """The mean over the triangles of the longest side of their axis-aligned box, as ClosestPointIndex passes it to the build
    (numpy's summation order: the last bits may differ from the device's mean, so a GPU test passes the index's own value)."""
    c = np.asarray(vertices, np.float64)[np.asarray(faces).reshape(-1, 3)]
    return float((c.max(1) - c.min(1)).max(1).mean())


def grid_margin(vertices, faces, extent=None):
    """(cell, margin) of the grid t4d_closest_build makes over these triangles: closest_grid of csrc/t4d_closest.hip restated."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    n = len(np.asarray(faces).reshape(-1, 3))
    lo, hi = v.min(0), v.max(0)
    e = [float(hi[a] - lo[a]) for a in range(3)]
    emax = max(e)
    area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2])
    cell = 2.0 * math.sqrt(area / float(n)) if area > 0.0 else 2.0 * emax / float(n)
    ext = mean_extent(v, faces) if extent is None else float(extent)
    if ext > cell:
        cell = ext
    cell = max(cell, emax * 2.0 ** -10)
    if not (cell > 0.0) or not math.isfinite(cell):
        cell = 1.0
    while True:
        dim = [min(4096, int(math.floor((e[a] + cell) / cell) + 1.0)) for a in range(3)]
        if dim[0] * dim[1] * dim[2] <= 1 << 22 and max(dim) < 4096:
            break
        cell *= 1.25
    mag = 0.0
    for a in range(3):
        glo = float(lo[a]) - 0.5 * cell
        mag = max(mag, abs(glo), abs(glo + float(dim[a] + 1) * cell))
    return cell, 2.0 ** -40 * (mag + cell)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def ray_pairs(o, d, a, b, c, t_lo, t_hi, same_side, margin):
    """(hit bool, t, u, v) of every pair of broadcastable o, d, a, b, c [..., 3]."""
    shape = np.broadcast(o[..., 0], a[..., 0]).shape
    o, d, a, b, c = ([np.broadcast_to(x[..., k], shape) for k in range(3)] for x in (o, d, a, b, c))
    with np.errstate(all="ignore"):
        e1 = [b[k] - a[k] for k in range(3)]
        e2 = [c[k] - a[k] for k in range(3)]
        pv = _cross(d, e2)
        det = _dot(e1, pv)
        hit = ~(det == 0.0)
        if same_side:
            hit &= ~(det >= 0.0)
        tv = [o[k] - a[k] for k in range(3)]
        u = _dot(tv, pv) / det
        hit &= (u >= 0.0) & (u <= 1.0)
        qv = _cross(tv, e1)
        v = _dot(d, qv) / det
        hit &= (v >= 0.0) & (u + v <= 1.0)
        t = _dot(e2, qv) / det
        hit &= (t >= t_lo) & (t <= t_hi)
        for k in range(3):
            p = o[k] + t * d[k]
            mn = np.minimum(a[k], np.minimum(b[k], c[k]))
            mx = np.maximum(a[k], np.maximum(b[k], c[k]))
            hit &= (p >= mn - margin) & (p <= mx + margin)
    return hit, t, u, v


def raycast(origins, dirs, vertices, faces, t_lo, t_hi, same_side=False, extent=None, chunk_pairs=1 << 19):
    """(t float64 [R], prim int32 [R], uv float64 [R,2]) by the rule above over all rays x all triangles.  extent: the mean
    extent the index was built with (None: mean_extent of the triangles)."""
    o = np.ascontiguousarray(origins, np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, np.float64).reshape(-1, 3)
    vtx = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    a, b, c = vtx[f[:, 0]], vtx[f[:, 1]], vtx[f[:, 2]]
    margin = grid_margin(vtx, f, extent)[1]
    t_lo, t_hi = np.float64(t_lo), np.float64(t_hi)
    R, n = len(o), len(f)
    out_t = np.zeros(R, np.float64)
    out_prim = np.full(R, -1, np.int32)
    out_uv = np.zeros((R, 2), np.float64)
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0.0).any(1) & bool(t_lo <= t_hi)
    step = max(1, chunk_pairs // n)
    for s in range(0, R, step):
        hit, t, u, v = ray_pairs(o[s:s + step, None, :], d[s:s + step, None, :], a[None], b[None], c[None], t_lo, t_hi, same_side, margin)
        hit = hit & valid[s:s + step, None]
        at = np.where(hit, np.abs(t), np.inf)
        cand = hit & (at == at.min(axis=1, keepdims=True))
        fwd = cand & (t >= 0.0)
        use = np.where(fwd.any(1, keepdims=True), fwd, cand)
        k = np.argmax(use, axis=1)                                 # the first candidate: the lowest index
        rows = np.nonzero(hit.any(1))[0]
        out_t[s + rows] = t[rows, k[rows]]
        out_prim[s + rows] = k[rows]
        out_uv[s + rows, 0] = u[rows, k[rows]]
        out_uv[s + rows, 1] = v[rows, k[rows]]
    return out_t, out_prim, out_uv
