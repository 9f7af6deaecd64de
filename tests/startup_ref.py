"""
The yardstick of the startup fit's device half (csrc/t4d_nricp.hip), in numpy float64, operation for operation and sum for sum as
include/topo4d_raster.h states them.  A field is an array [3,4,N] (coordinate column, row, vertex).

  reduce_sums(terms)        the fixed reduction order of every sum over the vertices: G = min(ceil(N / 256), 1024) workgroups of
                            256 lanes; lane l of all L = 256 G adds the vertices l, l + L, ... to zeros; a wave of 64 folds
                            v[t] = v[t] + v[t + w], w = 32 .. 1; four waves give (w0 + w1) + (w2 + w3); the workgroup sums are
                            added to zeros in index order.
  classify(...)             class, w, target and the record of every vertex (t4d_nricp_classify).
  assemble(...)             s, the right-hand side B and the Cholesky factors of the preconditioner's blocks (t4d_nricp_assemble).
  precondition(chol, R)     Z = M^-1 R (t4d_nricp_precond).
  apply_operator(...)       Q = K P and P[c] . Q[c] (t4d_nricp_apply).
  cg_start / cg_run         the conjugate-gradient records (t4d_nricp_cg_start, t4d_nricp_cg_run).
  positions(v, X, prev)     X^T (v, 1) and the largest squared move (t4d_nricp_positions).
  solve(...) / fit(...)     the host's loops of topo4d_amd.startup.solve and fit_template, over tests/scanscore_ref.closest_point
                            and tests/objexport_ref.trimesh_vertex_normals.  The package's vertex normals agree with that
                            restatement to 1e-12, not bit for bit, so `flipped` is the one class of a whole fit that is compared
                            through an input that is not identical; the classification tests give both sides one set of normals.

The host's own numpy steps (the neighbour CSR, the normalised frame, components, turned triangles) are restated here in their
plainest form and compared with the package's in tests/test_startup_host.py.
"""
import math

import numpy as np

from tests import objexport_ref, scanscore_ref

GROUP, WAVE, MAX_GROUPS = 256, 64, 1024
RECORD, SUM_D2 = 8, 7
STATE, STATE_REC, RZ, RR, PQ, ALPHA, BETA, ITER, STATE_BB = 40, 16, 0, 3, 6, 9, 12, 15, 32
UNMATCHED, GATED, DEGENERATE, OFF_NORMAL, FLIPPED, WEIGHTLESS, KEPT = range(7)
CLASSES = ("unmatched", "gated", "degenerate", "off_normal", "flipped", "weightless", "kept")
MIN_PAIRS = 6


def _dot3(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _dot4(u, v):
    return ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) + u[3] * v[3]


def groups_of(n):
    return min(max(1, -(-n // GROUP)), MAX_GROUPS)


def reduce_sums(terms):
    terms = np.asarray(terms, np.float64)
    n, width = terms.shape
    G = groups_of(n)
    L = G * GROUP
    K = -(-n // L)
    t = np.zeros((K * L, width))
    t[:n] = terms
    t = t.reshape(K, L, width)
    lane = np.zeros((L, width))
    for k in range(K):
        lane = lane + t[k]
    a = lane.reshape(G, GROUP // WAVE, WAVE, width).copy()
    w = WAVE // 2
    while w > 0:
        a[:, :, :w] = a[:, :, :w] + a[:, :, w:2 * w]
        w //= 2
    waves = a[:, :, 0]
    group = (waves[:, 0] + waves[:, 1]) + (waves[:, 2] + waves[:, 3])
    out = np.zeros(width)
    for b in range(G):
        out = out + group[b]
    return out


# ---- classification ---------------------------------------------------------------------------------------------------------------
def classify(points, scan_vertices, scan_faces, d2, idx, closest, normals=None, weights=None, gate2=-1.0, cos2=0.25, normal_cos=0.5):
    """(cls int32 [N], w [N], target [N,3], record [8]); scan_faces None: a cloud."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    d2, idx, cl = np.asarray(d2, np.float64), np.asarray(idx), np.asarray(closest, np.float64).reshape(-1, 3)
    n = len(p)
    is_tri = scan_faces is not None and len(scan_faces) > 0
    n_prims = len(scan_faces) if is_tri else len(scan_vertices)
    matched = (idx >= 0) & (idx < n_prims)
    wt = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    degenerate = off = flipped = np.zeros(n, bool)
    if is_tri:
        v = np.asarray(scan_vertices, np.float64)
        tri = np.asarray(scan_faces)[np.where(matched, idx, 0)]
        a, b, c = ([v[tri[:, k], j] for j in range(3)] for k in range(3))
        with np.errstate(all="ignore"):
            ab, ac = [b[j] - a[j] for j in range(3)], [c[j] - a[j] for j in range(3)]
            nv = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
            nn = _dot3(nv, nv)
            e = [p[:, j] - cl[:, j] for j in range(3)]
            en = _dot3(e, nv)
            degenerate = nn == 0.0
            off = (d2 > 0.0) & (en * en < (cos2 * d2) * nn)
            if normals is not None:
                length = np.sqrt(nn)
                nh = [nv[j] / length for j in range(3)]
                m = np.asarray(normals, np.float64)
                flipped = _dot3([m[:, j] for j in range(3)], nh) < normal_cos
    gated = (d2 > gate2) if gate2 >= 0.0 else np.zeros(n, bool)
    cls = np.where(~matched, UNMATCHED, np.where(gated, GATED, np.where(degenerate, DEGENERATE, np.where(off, OFF_NORMAL, np.where(
        flipped, FLIPPED, np.where(wt == 0.0, WEIGHTLESS, KEPT)))))).astype(np.int32)
    keep = cls == KEPT
    w = np.where(keep, wt, 0.0)
    target = np.where(keep[:, None], cl, 0.0)
    terms = np.zeros((n, RECORD))
    for k in range(7):
        terms[:, k] = cls == k
    terms[:, SUM_D2] = np.where(keep, d2, 0.0)
    return cls, w, target, reduce_sums(terms)


# ---- the system ---------------------------------------------------------------------------------------------------------------------
def neighbour_csr(faces, n):
    nbrs = [set() for _ in range(n)]
    for f in np.asarray(faces).reshape(-1, 3):
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if a != b:
                nbrs[int(a)].add(int(b))
                nbrs[int(b)].add(int(a))
    off = np.concatenate([[0], np.cumsum([len(s) for s in nbrs])]).astype(np.int32)
    return off, np.asarray([j for s in nbrs for j in sorted(s)], np.int32)


def assemble(v, nbr_off, w, c, lw=None, lt=None, a2=1.0, a2g=1.0, beta2=0.0):
    """(s [N], B field, chol [10,N])"""
    v, w, c = np.asarray(v, np.float64), np.asarray(w, np.float64), np.asarray(c, np.float64)
    n = len(v)
    vt = [v[:, 0], v[:, 1], v[:, 2], np.ones(n)]
    bl = beta2 * np.asarray(lw, np.float64) if lw is not None else np.zeros(n)
    s = w + bl
    B = np.zeros((3, 4, n))
    for col in range(3):
        lterm = bl * np.asarray(lt, np.float64)[:, col] if lw is not None else np.zeros(n)
        m = w * c[:, col] + lterm
        for r in range(4):
            B[col, r] = vt[r] * m if r < 3 else m
    deg = np.diff(nbr_off).astype(np.float64)
    g = [a2, a2, a2, a2g]
    at = lambda r, q: r * (r + 1) // 2 + q
    A = np.zeros((10, n))
    for r in range(4):
        for q in range(r + 1):
            A[at(r, q)] = (s * vt[r]) * vt[q]
        A[at(r, r)] = A[at(r, r)] + deg * g[r]
    L = np.zeros((10, n))
    with np.errstate(all="ignore"):
        for j in range(4):
            total = A[at(j, j)].copy()
            for k in range(j):
                total = total - L[at(j, k)] * L[at(j, k)]
            d = np.sqrt(total)
            L[at(j, j)] = d
            for r in range(j + 1, 4):
                t = A[at(r, j)].copy()
                for k in range(j):
                    t = t - L[at(r, k)] * L[at(j, k)]
                L[at(r, j)] = t / d
    lone = deg == 0
    for r in range(4):
        for q in range(r + 1):
            L[at(r, q)][lone] = 1.0 if r == q else 0.0
    return s, B, L


def precondition(chol, R):
    L, R = np.asarray(chol, np.float64), np.asarray(R, np.float64)
    Z = np.zeros_like(R)
    with np.errstate(all="ignore"):
        for col in range(3):
            r = R[col]
            y0 = r[0] / L[0]
            y1 = (r[1] - L[1] * y0) / L[2]
            y2 = ((r[2] - L[3] * y0) - L[4] * y1) / L[5]
            y3 = (((r[3] - L[6] * y0) - L[7] * y1) - L[8] * y2) / L[9]
            z3 = y3 / L[9]
            z2 = (y2 - L[8] * z3) / L[5]
            z1 = ((y1 - L[4] * z2) - L[7] * z3) / L[2]
            z0 = (((y0 - L[1] * z1) - L[3] * z2) - L[6] * z3) / L[0]
            Z[col] = [z0, z1, z2, z3]
    return Z


def operator(v, nbr_off, nbr, s, a2, a2g, P):
    """Q = K P"""
    v, P, s = np.asarray(v, np.float64), np.asarray(P, np.float64), np.asarray(s, np.float64)
    n = len(v)
    off = np.asarray(nbr_off, np.int64)
    deg = np.diff(off)
    lap = np.zeros_like(P)
    for k in range(int(deg.max()) if n else 0):
        has = k < deg
        j = np.asarray(nbr, np.int64)[np.where(has, off[:-1] + k, 0)]
        lap = lap + np.where(has, P - P[:, :, j], 0.0)
    Q = np.zeros_like(P)
    for col in range(3):
        pc = P[col]
        t = _dot3([v[:, 0], v[:, 1], v[:, 2]], pc) + pc[3]
        d = s * t
        for r in range(4):
            Q[col, r] = (a2 if r < 3 else a2g) * lap[col, r] + (v[:, r] * d if r < 3 else d)
    return Q


def column_dots(U, V):
    """[3]: U[c] . V[c] by the fixed reduction"""
    return reduce_sums(np.stack([_dot4(U[col], V[col]) for col in range(3)], 1))


def apply_operator(v, nbr_off, nbr, s, a2, a2g, P):
    Q = operator(v, nbr_off, nbr, s, a2, a2g, P)
    return Q, column_dots(P, Q)


def identity_field(n):
    X = np.zeros((3, 4, n))
    for c in range(3):
        X[c, c] = 1.0
    return X


def cg_start(v, nbr_off, nbr, s, a2, a2g, chol, B, X):
    """dict(X, R, Z, P, state): X is copied"""
    Q = operator(v, nbr_off, nbr, s, a2, a2g, X)
    R = B - Q
    Z = precondition(chol, R)
    state = np.zeros(STATE)
    state[RZ:RZ + 3], state[RR:RR + 3], state[STATE_BB:STATE_BB + 3] = column_dots(R, Z), column_dots(R, R), column_dots(B, B)
    return dict(X=np.array(X, np.float64), R=R, Z=Z, P=Z.copy(), Q=Q, state=state)


def cg_run(v, nbr_off, nbr, s, a2, a2g, chol, cg, done, iters, stop_mask=0):
    st = cg["state"]
    for k in range(iters):
        parity = (done + k) & 1
        cur, nxt = st[STATE_REC * parity:STATE_REC * parity + STATE_REC], st[STATE_REC * (1 - parity):STATE_REC * (1 - parity) + STATE_REC]
        X, R, P = cg["X"], cg["R"], cg["P"]
        Q, pq = apply_operator(v, nbr_off, nbr, s, a2, a2g, P)
        alpha = np.zeros(3)
        for c in range(3):
            alpha[c] = 0.0 if ((stop_mask >> c) & 1) or pq[c] == 0.0 else cur[RZ + c] / pq[c]
        for c in range(3):
            if alpha[c] != 0.0:
                X[c] = X[c] + alpha[c] * P[c]
                R[c] = R[c] - alpha[c] * Q[c]
        Z = precondition(chol, R)
        rz, rr = column_dots(R, Z), column_dots(R, R)
        beta = np.zeros(3)
        for c in range(3):
            beta[c] = 0.0 if alpha[c] == 0.0 else rz[c] / cur[RZ + c]
            P[c] = Z[c] if beta[c] == 0.0 else Z[c] + beta[c] * P[c]
        nxt[RZ:RZ + 3], nxt[RR:RR + 3], nxt[PQ:PQ + 3], nxt[ALPHA:ALPHA + 3], nxt[BETA:BETA + 3] = rz, rr, pq, alpha, beta
        nxt[ITER] = cur[ITER] + 1.0
        cg["Z"], cg["Q"] = Z, Q


def positions(v, X, prev=None):
    v, X = np.asarray(v, np.float64), np.asarray(X, np.float64)
    pos = np.stack([_dot3([v[:, 0], v[:, 1], v[:, 2]], X[c]) + X[c, 3] for c in range(3)], 1)
    if prev is None:
        return pos, 0.0
    e = pos - np.asarray(prev, np.float64)
    return pos, float(_dot3([e[:, 0], e[:, 1], e[:, 2]], [e[:, 0], e[:, 1], e[:, 2]]).max())


def solve(v, nbr_off, nbr, s, a2, a2g, chol, B, X, tol, max_cg, check_every=32):
    """topo4d_amd.startup.solve: (X, iterations per column, relative residuals, the state records the host read)"""
    cg = cg_start(v, nbr_off, nbr, s, a2, a2g, chol, B, X)
    done, mask, stopped_at, seen = 0, 0, [None] * 3, []
    tol2 = float(tol) * float(tol)
    while True:
        st = cg["state"]
        seen.append(st.copy())
        rec, bb = st[STATE_REC * (done & 1):STATE_REC * (done & 1) + STATE_REC], st[STATE_BB:STATE_BB + 3]
        for c in range(3):
            if stopped_at[c] is None and (rec[RR + c] <= tol2 * bb[c] or done >= max_cg):
                stopped_at[c], mask = done, mask | (1 << c)
        if mask == 7:
            break
        step = min(int(check_every), int(max_cg) - done)
        cg_run(v, nbr_off, nbr, s, a2, a2g, chol, cg, done, step, mask)
        done += step
    rel = [math.sqrt(rec[RR + c] / bb[c]) if bb[c] > 0.0 else 0.0 for c in range(3)]
    return cg["X"], stopped_at, rel, seen


def dense_system(v, nbr_off, nbr, s, a2, a2g):
    """K as a dense [4N,4N] matrix, unknown 4 i + r: plain linear algebra for the solver's tests, in numpy's own order."""
    n = len(v)
    K = np.zeros((4 * n, 4 * n))
    g = np.array([a2, a2, a2, a2g])
    vt = np.concatenate([v, np.ones((n, 1))], 1)
    for i in range(n):
        for j in nbr[nbr_off[i]:nbr_off[i + 1]]:
            for r in range(4):
                K[4 * i + r, 4 * i + r] += g[r]
                K[4 * i + r, 4 * j + r] -= g[r]
        K[4 * i:4 * i + 4, 4 * i:4 * i + 4] += s[i] * np.outer(vt[i], vt[i])
    return K


def field_to_dense(F):
    """[4N,3] with row 4 i + r"""
    return np.transpose(np.asarray(F), (2, 1, 0)).reshape(-1, 3)


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
def transform(points, matrix):
    p, m = np.asarray(points, np.float64), np.asarray(matrix, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)], 1)


def frame_of(vertices):
    lo, hi = vertices.min(0), vertices.max(0)
    d = hi - lo
    return (lo + hi) * 0.5, math.sqrt(float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def component_labels(nbr_off, nbr):
    n = len(nbr_off) - 1
    label = -np.ones(n, np.int64)
    for root in range(n):
        if label[root] >= 0:
            continue
        label[root], stack = root, [root]
        while stack:
            i = stack.pop()
            for j in nbr[nbr_off[i]:nbr_off[i + 1]]:
                if label[j] < 0:
                    label[j] = root
                    stack.append(int(j))
    return label


def fit(vertices, faces, scan_vertices, scan_faces, pre, weights=None, landmarks=None, stiffness=(50.0, 20.0, 5.0, 2.0, 0.8, 0.5, 0.35, 0.2),
        inner=3, gamma=1.0, landmark_weight=1.0, normal_cos=0.5, max_dist=None, gate_sigma=3.0, tol=1e-8, max_cg=2000, check_every=32,
        move_tol=1e-5, query=None):
    """topo4d_amd.startup.fit_template after its pre-alignment `pre` (4x4): dict(vertices, steps, components_without_data,
    flipped_triangles).  ValueError for fewer than MIN_PAIRS kept vertices at the first step."""
    tv, faces = np.asarray(vertices, np.float64), np.asarray(faces)
    n = len(tv)
    placed = transform(tv, pre)
    centre, diag = frame_of(placed)
    unit = lambda x: (x - centre) / diag
    v, sv = unit(placed), unit(np.asarray(scan_vertices, np.float64))
    is_tri = scan_faces is not None and len(scan_faces) > 0
    if query is None:
        query = lambda pts, md: scanscore_ref.closest_point(pts, sv, scan_faces if is_tri else None, max_dist=md)
    lw = lt = None
    if landmarks is not None:
        rows = np.asarray(landmarks, np.float64)
        lw, lt = np.zeros(n), np.zeros((n, 3))
        lw[rows[:, 0].astype(np.int64)] = 1.0
        lt[rows[:, 0].astype(np.int64)] = rows[:, 1:]
        lt = unit(lt)
    st = [float(a) for a in stiffness]
    lws = [float(b) for b in landmark_weight] if isinstance(landmark_weight, (list, tuple)) else [float(landmark_weight)] * len(st)
    off, nbr = neighbour_csr(faces, n)
    gate = None if max_dist is None else float(max_dist) / diag
    limit = gate
    cos2 = float(normal_cos) * float(normal_cos)
    X = identity_field(n)
    pos, _ = positions(v, X)
    steps, s = [], None
    for alpha, beta in zip(st, lws):
        a2 = alpha * alpha
        a2g = a2 * (float(gamma) * float(gamma))
        for it in range(inner):
            d2, idx, cl = query(pos, limit)
            normals = objexport_ref.trimesh_vertex_normals(pos, faces) if is_tri else None
            cls, w, target, rec = classify(pos, sv, scan_faces if is_tri else None, d2, idx, cl, normals, weights,
                                           -1.0 if gate is None else gate * gate, cos2, float(normal_cos))
            kept = int(rec[KEPT])
            counts = {name: int(rec[k]) for k, name in enumerate(CLASSES)}
            if not steps and kept < MIN_PAIRS:
                raise ValueError(f"only {kept} vertices keep a data term at the first step")
            rms = math.sqrt(rec[SUM_D2] / kept) if kept else 0.0
            if not steps:                                       # the sigma gate is set once, from the first step's kept pairs
                gate = float(gate_sigma) * rms if limit is None else min(limit, float(gate_sigma) * rms)
            s, B, chol = assemble(v, off, w, target, lw, lt, a2, a2g, beta * beta)
            X, iters, rel, _ = solve(v, off, nbr, s, a2, a2g, chol, B, X, tol, max_cg, check_every)
            pos, move2 = positions(v, X, prev=pos)
            move = math.sqrt(move2)
            steps.append({"stiffness": alpha, "landmark_weight": beta, "step": it, "counts": counts, "rms": rms * diag, "cg_iterations": iters,
                          "residuals": rel, "move": move * diag})
            if move <= float(move_tol):
                break
    fitted = pos * diag + centre
    label = component_labels(off, nbr)
    without = [{"size": int((label == k).sum()), "first_vertex": int(k)} for k in np.unique(label) if not (s[label == k] > 0).any()]
    normal = lambda x: np.cross(x[faces[:, 1]] - x[faces[:, 0]], x[faces[:, 2]] - x[faces[:, 0]])
    turned = [int(k) for k in np.nonzero((normal(placed) * normal(fitted)).sum(1) < 0.0)[0]]
    return dict(vertices=fitted, steps=steps, components_without_data=without, flipped_triangles=turned, placed=placed, centre=centre,
                diagonal=diag)


# ---- scenes the host and the GPU tests share -----------------------------------------------------------------------------------
def deform(points):
    """the smooth known deformation of the prototype scene, on scanalign_ref's open surface: mostly across the surface, which is
    what closest points can see (a displacement along the surface only slides it over itself, away from the rim)"""
    p = np.asarray(points, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([x + 0.01 * np.sin(1.5 * y + 0.3), y + 0.01 * np.cos(1.2 * x - 0.2) * z, z + 0.07 * np.sin(1.1 * x + 0.4) * np.cos(0.9 * y)], 1)


def prototype_scene(n_template=21, n_scan=61):
    """(template vertices, template faces, scan vertices, scan faces, the ideal fit: the template's vertices moved by `deform`)"""
    from tests import scanalign_ref
    tv, tf = scanalign_ref.open_surface(n_template)
    sv, sf = scanalign_ref.open_surface(n_scan)
    return tv, tf, np.ascontiguousarray(deform(sv)), sf, deform(tv)


def grid_mesh(n_vert, seed=0):
    """a strip of triangles over n_vert >= 3 jittered vertices (two rows), every vertex in a face: (vertices, faces)"""
    rng = np.random.default_rng(seed)
    cols = (n_vert + 1) // 2
    xy = np.array([[c, r] for c in range(cols) for r in range(2)], np.float64)[:n_vert]
    v = np.concatenate([xy / max(cols - 1, 1), np.zeros((n_vert, 1))], 1) + rng.uniform(-0.02, 0.02, (n_vert, 3))
    f = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(n_vert - 2)], np.int32)
    return np.ascontiguousarray(v - v.mean(0)), f
