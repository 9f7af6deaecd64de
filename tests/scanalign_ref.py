"""
The yardstick of the scan alignment's device half (csrc/t4d_align.hip), in numpy float64, operation for operation:

  transform(points, matrix)       out = M p + t, each component ((m0 x + m1 y) + m2 z) + t, every product and sum rounded.
  pair_terms(...)                 the class of every pair and the 51 terms it adds to the record (zeros unless kept), with
                                  dot(u, v) = (u0 v0 + u1 v1) + u2 v2 and the layout of include/topo4d_raster.h.
  reduce_record(terms)            the kernel's reduction order: G = min(ceil(Q / 256), 1024) workgroups of 256 lanes; lane l of
                                  all L = 256 G adds the pairs l, l + L, ... to zeros in that order; a wave of 64 lanes folds
                                  v[t] = v[t] + v[t + w] for w = 32 .. 1; four waves give (w0 + w1) + (w2 + w3); the workgroup
                                  sums are added to zeros in index order.  (A pair that is not kept adds 0.0, which changes no
                                  sum: none can be -0.0.)
  align_loop(...)                 the whole loop of topo4d_amd.scanalign.align_scan over tests/scanscore_ref.closest_point, with
                                  the package's own host solvers (solve_plane, solve_point: numpy on one record) in between.
                                  It is independent of the package for the device half and the loop's control only: an error
                                  in a solver would be the same bits on both sides.  The solvers are held by
                                  tests/test_scanalign_host.py and by the recovery tests, which compare with a known motion.
"""
import math

import numpy as np

from tests import scanscore_ref

RECORD, GROUP, WAVE, MAX_GROUPS = 51, 256, 64, 1024
COUNT, SUM_D2, SUM_R2, JTR, JTJ, SUM_Q, SUM_G, SUM_QG, SUM_QQ, SUM_GG = 0, 5, 6, 7, 13, 34, 37, 40, 49, 50
UNMATCHED, GATED, DEGENERATE, OFF_NORMAL, KEPT = range(5)


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def transform(points, matrix):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    m = np.asarray(matrix, np.float64)[:3]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)], 1)


def pair_terms(points, vertices, faces, d2, idx, closest, origin, gate2, cos2):
    """(class int [Q], terms float64 [Q,51])"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3)
    d2, idx, cl = np.asarray(d2, np.float64), np.asarray(idx), np.asarray(closest, np.float64).reshape(-1, 3)
    o = np.asarray(origin, np.float64)
    Q = len(p)
    matched = (idx >= 0) & (idx < len(f))
    tri = f[np.where(matched, idx, 0)]
    a, b, c = ([v[tri[:, k], j] for j in range(3)] for k in range(3))
    with np.errstate(all="ignore"):
        ab, ac = [b[j] - a[j] for j in range(3)], [c[j] - a[j] for j in range(3)]
        n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
        nn = _dot(n, n)
        pt, cp = [p[:, j] for j in range(3)], [cl[:, j] for j in range(3)]
        e = [pt[j] - cp[j] for j in range(3)]
        en = _dot(e, n)
        gated = (d2 > gate2) if gate2 >= 0.0 else np.zeros(Q, bool)
        off = (d2 > 0.0) & (en * en < (cos2 * d2) * nn)
        cls = np.where(~matched, UNMATCHED, np.where(gated, GATED, np.where(nn == 0.0, DEGENERATE, np.where(off, OFF_NORMAL, KEPT))))
        length = np.sqrt(nn)
        nh = [n[j] / length for j in range(3)]
        r = _dot(e, nh)
        q = [pt[j] - o[j] for j in range(3)]
        g = [cp[j] - o[j] for j in range(3)]
        J = [q[1] * nh[2] - q[2] * nh[1], q[2] * nh[0] - q[0] * nh[2], q[0] * nh[1] - q[1] * nh[0], nh[0], nh[1], nh[2]]
        terms = np.zeros((Q, RECORD), np.float64)
        terms[:, SUM_D2] = d2
        terms[:, SUM_R2] = r * r
        k = JTJ
        for i in range(6):
            terms[:, JTR + i] = r * J[i]
            for j in range(i, 6):
                terms[:, k] = J[i] * J[j]
                k += 1
        for i in range(3):
            terms[:, SUM_Q + i] = q[i]
            terms[:, SUM_G + i] = g[i]
            for j in range(3):
                terms[:, SUM_QG + 3 * i + j] = q[i] * g[j]
        terms[:, SUM_QQ] = _dot(q, q)
        terms[:, SUM_GG] = _dot(g, g)
    terms[cls != KEPT] = 0.0
    for k in range(5):
        terms[:, COUNT + k] = cls == k
    return cls, terms


def groups_of(Q):
    return min(max(1, -(-Q // GROUP)), MAX_GROUPS)


def reduce_record(terms):
    terms = np.asarray(terms, np.float64).reshape(-1, RECORD)
    Q = len(terms)
    if Q == 0:
        return np.zeros(RECORD)
    G = groups_of(Q)
    L = G * GROUP
    K = -(-Q // L)
    t = np.zeros((K * L, RECORD))
    t[:Q] = terms
    t = t.reshape(K, L, RECORD)
    lane = np.zeros((L, RECORD))
    for k in range(K):
        lane = lane + t[k]
    a = lane.reshape(G, GROUP // WAVE, WAVE, RECORD).copy()
    w = WAVE // 2
    while w > 0:
        a[:, :, :w] = a[:, :, :w] + a[:, :, w:2 * w]
        w //= 2
    waves = a[:, :, 0]
    group = (waves[:, 0] + waves[:, 1]) + (waves[:, 2] + waves[:, 3])
    rec = np.zeros(RECORD)
    for b in range(G):
        rec = rec + group[b]
    return rec


def record(points, vertices, faces, d2, idx, closest, origin, gate2=-1.0, cos2=0.0):
    return reduce_record(pair_terms(points, vertices, faces, d2, idx, closest, origin, gate2, cos2)[1])


def naive_record(points, vertices, faces, d2, idx, closest, origin, gate2=-1.0, cos2=0.0):
    """the same sums in numpy's own order: what a solver test needs, and a check of the layout against plain linear algebra"""
    return pair_terms(points, vertices, faces, d2, idx, closest, origin, gate2, cos2)[1].sum(0)


def align_loop(mesh_vertices, mesh_faces, scan_points, init=None, metric="plane", scale=False, max_iter=30, max_dist=None, gate_sigma=3.0,
               normal_cos=0.5, tol=1e-6, stride=1, query=None):
    """dict(matrix, iterations, converged, counts, rms_before, rms_after): align_scan's loop.  query(points, max_dist): the closest
    points (default: the brute force of tests/scanscore_ref.py)."""
    from topo4d_amd import scanalign as SA
    mv = np.ascontiguousarray(mesh_vertices, np.float64)
    p0 = np.ascontiguousarray(np.asarray(scan_points, np.float64)[::stride])
    if query is None:
        query = lambda pts, md: scanscore_ref.closest_point(pts, mv, mesh_faces, max_dist=md)
    pose = np.eye(4) if init is None else np.array(init, np.float64)
    corners = SA.box_corners(mv)
    diag = float(np.linalg.norm(corners[7] - corners[0]))
    origin = mv.mean(0)
    cos2 = float(normal_cos) * float(normal_cos)

    def evaluate(gate):
        moved = transform(p0, pose)
        d2, idx, cl = query(moved, max_dist)
        rec = record(moved, mv, mesh_faces, d2, idx, cl, origin, -1.0 if gate is None else gate * gate, cos2)
        n = SA.kept_pairs(rec)
        return rec, math.sqrt(rec[SUM_D2] / n)

    gate = None if max_dist is None else float(max_dist)
    iterations, converged, rms_before = 0, True, None
    for phase_metric, with_scale in ([("point", True)] if scale else []) + [(metric, False)]:
        phase_converged = False
        for _ in range(int(max_iter)):
            rec, rms = evaluate(gate)
            if rms_before is None:
                rms_before = rms
            A, b = SA.step_of(rec, phase_metric, with_scale, origin)
            pose[:3, :3], pose[:3, 3] = A @ pose[:3, :3], A @ pose[:3, 3] + b
            iterations += 1
            gate = float(gate_sigma) * rms if max_dist is None else min(float(max_dist), float(gate_sigma) * rms)
            motion = float(np.sqrt((((corners @ A.T + b) - corners) ** 2).sum(1)).max())
            if motion <= float(tol) * diag:
                phase_converged = True
                break
        converged = converged and phase_converged
    rec, rms_after = evaluate(gate)
    return dict(matrix=pose, iterations=iterations, converged=converged, counts={n: int(rec[COUNT + k]) for k, n in enumerate(SA.CLASSES)},
                rms_before=rms_before, rms_after=rms_after)


# ---- scenes the host and the GPU tests share -----------------------------------------------------------------------------------
def surface_point(u, w):
    """the asymmetric height field the scenes are cut from, at parameters u, w (arrays); the mesh covers [-1, 1]^2"""
    x, y = 1.3 * u + 0.1 * w * w, w + 0.05 * u
    z = 0.35 * np.sin(1.7 * u + 0.4) * np.cos(1.1 * w - 0.3) + 0.25 * u * w + 0.15 * u * u - 0.2 * w ** 3
    return np.stack([x, y, z], -1)


def open_surface(n=11):
    """An asymmetric open height field, (n - 1)^2 * 2 triangles (200 for n = 11): no symmetry leaves a motion undetermined."""
    u, w = np.meshgrid(np.linspace(-1.0, 1.0, n), np.linspace(-1.0, 1.0, n), indexing="ij")
    v = surface_point(u, w).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)]).astype(np.int32)
    return np.ascontiguousarray(v), f


def beyond_rim(n, seed, lo=1.1, hi=1.6):
    """n points of the same height field past the mesh's rim at u = 1 ("shoulders": the scan goes on where the mesh ends)"""
    rng = np.random.default_rng(seed)
    return surface_point(rng.uniform(lo, hi, n), rng.uniform(-0.8, 0.8, n))


def sample_surface(v, f, n, seed):
    """n points on the triangles themselves (zero true residual), area-weighted"""
    rng = np.random.default_rng(seed)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    pick = rng.choice(len(f), n, p=area / area.sum())
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    return w[:, :1] * a[pick] + w[:, 1:2] * b[pick] + w[:, 2:] * c[pick]


def rigid(rotvec_deg, translation, scale=1.0):
    from topo4d_amd.scanalign import rodrigues
    m = np.eye(4)
    m[:3, :3] = scale * rodrigues(np.radians(np.asarray(rotvec_deg, np.float64)))
    m[:3, 3] = translation
    return m


def apply(matrix, points):
    return points @ matrix[:3, :3].T + matrix[:3, 3]


def pose_error(got, want):
    """(rotation error in radians, translation error, scale error) between two 4x4s whose 3x3 parts are scaled rotations; the
    angle from the skew part as well as the trace, so that it is accurate near 0"""
    sg, sw = np.cbrt(np.linalg.det(got[:3, :3])), np.cbrt(np.linalg.det(want[:3, :3]))
    d = (got[:3, :3] / sg) @ (want[:3, :3] / sw).T
    sin = 0.5 * math.sqrt((d[2, 1] - d[1, 2]) ** 2 + (d[0, 2] - d[2, 0]) ** 2 + (d[1, 0] - d[0, 1]) ** 2)
    ang = math.atan2(sin, (np.trace(d) - 1.0) / 2.0)
    return ang, float(np.linalg.norm(got[:3, 3] - want[:3, 3])), abs(float(sg - sw))
