"""
The yardstick of the closest-point query (csrc/t4d_closest.hip): a float64 numpy brute force over every (query, primitive)
pair.  It fixes, and the kernel repeats operation for operation:

  dot(u, v) = (u0 v0 + u1 v1) + u2 v2, every product and sum rounded (no fused multiply-add); d2 = dot(p - c, p - c).
  Triangle (a, b, c): Ericson's region walk (Real-Time Collision Detection 5.1.5), with quotients where the book multiplies by
  a reciprocal: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, interior, tested in that order.
  Degenerate rule: a triangle whose unnormalised normal (b - a) x (c - a) is exactly (0, 0, 0), and an interior case whose
  weights va, vb, vc are not all >= 0 with a sum > 0, take the nearest of the edges ab, bc, ca (the first wins a tie); an edge
  is a + t e clamped to its ends (t <= 0 or a zero-length edge: a; t >= 1: b).  The result is always a point of the primitive.
  Tie rule: among primitives of equal d2 the lowest index.
  max_dist rule: a query is matched iff d2 <= max_dist * max_dist; unmatched: index -1, d2 +inf, closest 0.
  Sign: that of dot(p - closest, (b - a) x (c - a)) of the chosen triangle; 0 for points.
"""
import numpy as np


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sub(u, v):
    return [u[0] - v[0], u[1] - v[1], u[2] - v[2]]


def _dist2(p, c):
    return _dot(_sub(p, c), _sub(p, c))


def _where3(m, u, v):
    return [np.where(m, u[k], v[k]) for k in range(3)]


def _segment(p, a, b):
    """(d2, closest) of segments a-b; p, a, b lists of three broadcastable arrays."""
    e = _sub(b, a)
    ap = _sub(p, a)
    ee = _dot(e, e)
    with np.errstate(all="ignore"):
        t = np.where(ee > 0.0, _dot(ap, e) / np.where(ee > 0.0, ee, 1.0), 0.0)
    mid = [a[k] + t * e[k] for k in range(3)]
    c = _where3(~(t > 0.0), a, _where3(t >= 1.0, b, mid))
    c = [np.broadcast_to(x, np.broadcast(p[0], a[0]).shape) for x in c]
    return _dist2(p, c), c


def _edges(p, a, b, c):
    best, out = _segment(p, a, b)
    for u, v in ((b, c), (c, a)):
        d, q = _segment(p, u, v)
        m = d < best
        best = np.where(m, d, best)
        out = _where3(m, q, out)
    return best, out


def triangle_pairs(p, a, b, c):
    """(d2, closest [...,3]) for broadcastable p, a, b, c of shape [..., 3]."""
    shape = np.broadcast(p[..., 0], a[..., 0]).shape
    p, a, b, c = ([np.broadcast_to(x[..., k], shape).reshape(-1) for k in range(3)] for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac = _sub(b, a), _sub(c, a)
        nx = ab[1] * ac[2] - ab[2] * ac[1]
        ny = ab[2] * ac[0] - ab[0] * ac[2]
        nz = ab[0] * ac[1] - ab[1] * ac[0]
        flat = (nx == 0.0) & (ny == 0.0) & (nz == 0.0)
        ap = _sub(p, a)
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = _sub(p, b)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = _sub(p, c)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        g43, g56 = d4 - d3, d5 - d6
        in_a = (d1 <= 0.0) & (d2 <= 0.0)
        in_b = (d3 >= 0.0) & (d4 <= d3)
        on_ab = (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0)
        in_c = (d6 >= 0.0) & (d5 <= d6)
        on_ac = (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0)
        on_bc = (va <= 0.0) & (g43 >= 0.0) & (g56 >= 0.0)
        s = (va + vb) + vc
        unsafe = ~(s > 0.0) | ~(va >= 0.0) | ~(vb >= 0.0) | ~(vc >= 0.0)
        v = d1 / (d1 - d3)
        p_ab = [a[k] + v * ab[k] for k in range(3)]
        w = d2 / (d2 - d6)
        p_ac = [a[k] + w * ac[k] for k in range(3)]
        w = g43 / (g43 + g56)
        p_bc = [b[k] + w * (c[k] - b[k]) for k in range(3)]
        v, w = vb / s, vc / s
        p_in = [(a[k] + ab[k] * v) + ac[k] * w for k in range(3)]
        out = p_in
        for m, q in ((on_bc, p_bc), (on_ac, p_ac), (in_c, c), (on_ab, p_ab), (in_b, b), (in_a, a)):
            out = _where3(m, q, out)
        dd = _dist2(p, out)
        walked = in_a | in_b | on_ab | in_c | on_ac | on_bc
        fb = flat | (~walked & unsafe)                    # the pairs that take the edge rule
        if fb.any():
            k = np.nonzero(fb)[0]
            de, qe = _edges([x[k] for x in p], [x[k] for x in a], [x[k] for x in b], [x[k] for x in c])
            dd = dd.copy()
            dd[k] = de
            out = [x.copy() for x in out]
            for j in range(3):
                out[j][k] = qe[j]
    return dd.reshape(shape), np.stack(out, -1).reshape(shape + (3,))


def closest_point(points, vertices, faces=None, max_dist=None, chunk_pairs=1 << 19):
    """(d2 float64 [Q], index int32 [Q], closest float64 [Q,3]) by brute force."""
    q = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    tri = faces is not None and len(faces) > 0
    if tri:
        f = np.asarray(faces).reshape(-1, 3)
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = len(f) if tri else len(v)
    Q = len(q)
    d2 = np.empty(Q, np.float64)
    idx = np.empty(Q, np.int32)
    cl = np.empty((Q, 3), np.float64)
    step = max(1, chunk_pairs // n)
    for s in range(0, Q, step):
        p = q[s:s + step, None, :]
        if tri:
            dd, cc = triangle_pairs(p, a[None], b[None], c[None])
        else:
            cc = np.broadcast_to(v[None], (p.shape[0], n, 3))
            dd = _dist2([p[..., k] for k in range(3)], [cc[..., k] for k in range(3)])
        k = np.argmin(dd, axis=1)                         # the first minimum: the lowest index
        rows = np.arange(len(k))
        d2[s:s + step] = dd[rows, k]
        idx[s:s + step] = k
        cl[s:s + step] = cc[rows, k]
    return apply_max_dist(d2, idx, cl, max_dist)


def apply_max_dist(d2, idx, closest, max_dist):
    """The max_dist rule on a brute-force result (copies); None leaves every query matched."""
    d2, idx, closest = d2.copy(), idx.copy(), closest.copy()
    if max_dist is not None:
        md = np.float64(max_dist)
        miss = ~(d2 <= md * md)
        d2[miss] = np.inf
        idx[miss] = -1
        closest[miss] = 0.0
    return d2, idx, closest


def signed_distance(points, vertices, faces, d2, idx, closest):
    """float64 [Q]: sqrt(d2) with the sign rule above; 0 for point primitives and unmatched queries."""
    q = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.zeros(len(q), np.float64)
    if faces is None or len(faces) == 0:
        return out
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    m = idx >= 0
    t = f[idx[m]]
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    ab, ac = [b[:, k] - a[:, k] for k in range(3)], [c[:, k] - a[:, k] for k in range(3)]
    n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
    d = [q[m][:, k] - closest[m][:, k] for k in range(3)]
    s = _dot(d, n)
    out[m] = np.sign(s) * np.sqrt(d2[m])
    return out


def direction_stats(d2, idx, signed, thresholds, unit=1.0):
    """The statistics score_scan reports for one direction, from the per-query output (numpy's own summation order)."""
    m = idx >= 0
    n = int(m.sum())
    out = {"count": n, "unmatched": int((~m).sum())}
    if n == 0:
        return out
    d = np.sqrt(d2[m]) * unit
    srt = np.sort(d)
    out["mean"] = float(d.sum() / n)
    out["rms"] = float(np.sqrt((d * d).sum() / n))
    out["median"] = float(srt[(n - 1) // 2])
    out["p90"] = float(srt[min(n - 1, -(-9 * n // 10) - 1)])
    out["max"] = float(srt[-1])
    out["signed_mean"] = float((signed[m] * unit).sum() / n)
    out["within"] = {repr(float(t)): float((d <= t).sum() / n) for t in thresholds}
    return out
