"""The tessellation and displacement rules of include/topo4d_raster.h (t4d_tess_faces, t4d_tess_points, t4d_tess_displace) as
numpy: the yardstick of tests/test_gpu_tessellate.py and the subject of tests/test_tessellate_host.py.

The topology is walked triangle by triangle with a dictionary of edges and a dictionary of lattice points; per fine vertex it keeps
a record (kind, owner, lattice point), which the kernels never build.  The arithmetic is whole-array float64: numpy rounds every
operation once and never contracts, which is the arithmetic the header prescribes."""
import numpy as np

ZERO = 32768
CORNER, EDGE, INNER = 0, 1, 2


class Topology:
    """faces int32 [N^2 T,3] and, per fine vertex: kind, owner (a triangle, -1 for a corner in no triangle), a / b / c (the
    owner's corners the vertex is mixed from: (lo, hi, -) for an edge vertex) and i / j / k ((N - s, s, 0) for an edge vertex)."""

    def __init__(self, tris, n_corner, level):
        tris = np.asarray(tris, np.int64).reshape(-1, 3)
        N, T = int(level), len(tris)
        pairs = np.sort(np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]), axis=1)
        edges = np.unique(pairs, axis=0)
        edge_id = {tuple(e): n for n, e in enumerate(edges.tolist())}
        E, I = len(edges), (N - 1) * (N - 2) // 2
        inner = {}
        for j in range(1, N - 1):
            for k in range(1, N - j):
                inner[(j, k)] = len(inner)
        assert len(inner) == I
        self.level, self.n_corner, self.n_edges, self.n_tri = N, int(n_corner), E, T
        self.n_vertices = M = int(n_corner) + E * (N - 1) + T * I
        self.kind = np.full(M, -1, np.int64)
        self.owner = np.full(M, -1, np.int64)
        self.abc = np.zeros((M, 3), np.int64)
        self.ijk = np.zeros((M, 3), np.int64)
        self.kind[:n_corner] = CORNER
        self.abc[:n_corner, 0] = np.arange(n_corner)
        self.ijk[:n_corner, 0] = N

        def on_edge(p, q, steps):                               # the vertex `steps` from p on the edge p -> q
            lo, hi = min(p, q), max(p, q)
            s = steps if p == lo else N - steps
            return n_corner + edge_id[(lo, hi)] * (N - 1) + (s - 1), lo, hi, s

        faces = []
        for t, (a, b, c) in enumerate(tris.tolist()):
            def vid(i, j, k):
                if i == N:
                    m = a
                elif j == N:
                    m = b
                elif k == N:
                    m = c
                elif k == 0:
                    m, lo, hi, s = on_edge(a, b, j)
                elif i == 0:
                    m, lo, hi, s = on_edge(b, c, k)
                elif j == 0:
                    m, lo, hi, s = on_edge(c, a, i)
                else:
                    m = n_corner + E * (N - 1) + t * I + inner[(j, k)]
                    self.kind[m], self.owner[m], self.abc[m], self.ijk[m] = INNER, t, (a, b, c), (i, j, k)
                    return m
                if max(i, j, k) < N and self.kind[m] < 0:      # an edge vertex: the lowest triangle that has the edge comes first
                    self.kind[m], self.owner[m], self.abc[m], self.ijk[m] = EDGE, t, (lo, hi, 0), (N - s, s, 0)
                return m

            for corner in (a, b, c):                            # a corner belongs to the first triangle that names it
                if self.owner[corner] < 0:
                    self.owner[corner] = t
            for r in range(N):
                for s in range(r + 1):
                    i, j, k = N - r, r - s, s
                    faces.append([vid(i, j, k), vid(i - 1, j + 1, k), vid(i - 1, j, k + 1)])
                    if s < r:
                        faces.append([vid(i, j, k), vid(i - 1, j, k + 1), vid(i, j - 1, k + 1)])
        self.faces = np.asarray(faces, np.int32).reshape(-1, 3)
        assert (self.kind >= 0).all()


def _mix(values, topo):
    """float64 [M,D]: the rules of t4d_tess_points over topo's records"""
    v = np.asarray(values, np.float64)
    N = np.float64(topo.level)
    A, B, C = (v[topo.abc[:, n]] for n in range(3))
    i, j, k = (topo.ijk[:, n].astype(np.float64)[:, None] for n in range(3))
    edge = ((i * A) + (j * B)) / N                              # (N - s) X_lo + s X_hi
    inner = (((i * A) + (j * B)) + (k * C)) / N
    kind = topo.kind[:, None]
    return np.where(kind == CORNER, A, np.where(kind == EDGE, edge, inner))


def points(values, topo):
    return _mix(values, topo)


def _owner_uv_corners(topo, tris, uv_tris):
    """int64 [M,3]: the owner's UV corners that stand at the mesh corners abc (column 2 unused for corners and edge vertices)"""
    tris, uv_tris = np.asarray(tris, np.int64), np.asarray(uv_tris, np.int64)
    out = np.zeros((topo.n_vertices, 3), np.int64)
    own = np.maximum(topo.owner, 0)
    for col in range(3):
        want = topo.abc[:, col]
        first = np.full(topo.n_vertices, -1, np.int64)
        for c in (2, 1, 0):
            first = np.where(tris[own, c] == want, uv_tris[own, c], first)
        out[:, col] = np.where(first >= 0, first, 0)
    return out


def displace(vertices, normals, uvs, tris, uv_tris, uv_islands, topo, code, has, labels, unit):
    """(float64 [M,3], sampled uint8 [M]) by the rules of t4d_tess_displace.  uv_islands: projtex.uv_islands (int [n_uv])."""
    X, Nv, UV = np.asarray(vertices, np.float64), np.asarray(normals, np.float64), np.asarray(uvs, np.float64)
    code = np.asarray(code).astype(np.int64) & 0xFFFF
    has, labels = np.asarray(has) != 0, np.asarray(labels).astype(np.int64)
    h, w = code.shape
    uv_tris = np.asarray(uv_tris, np.int64)
    owned = topo.owner >= 0
    own = np.maximum(topo.owner, 0)
    P, n = _mix(X, topo), _mix(Nv, topo)
    uv_topo = Topology.__new__(Topology)                        # the same records over the owner's UV corners
    uv_topo.level, uv_topo.kind, uv_topo.ijk, uv_topo.n_vertices = topo.level, topo.kind, topo.ijk, topo.n_vertices
    uv_topo.abc = _owner_uv_corners(topo, tris, uv_tris)
    uv = _mix(UV, uv_topo)
    u, v = uv[:, 0], uv[:, 1]
    L = np.asarray(uv_islands, np.int64)[uv_tris[own, 0]]
    with np.errstate(all="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = owned & (length != 0.0) & np.isfinite(length) & np.isfinite(u) & np.isfinite(v) & np.isfinite(P).all(1) & np.isfinite(n).all(1)
        us, vs = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        x = us * np.float64(w - 1)
        y = (np.float64(h) - vs * np.float64(h - 1)) - 1.0
        xf = np.clip(np.floor(x), 0.0, float(max(w - 2, 0)))
        yf = np.clip(np.floor(y), 0.0, float(max(h - 2, 0)))
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        fx, fy = np.clip(x - xf, 0.0, 1.0), np.clip(y - yf, 0.0, 1.0)
        S, W = np.zeros(len(P)), np.zeros(len(P))
        total, count = np.zeros(len(P), np.int64), np.zeros(len(P), np.int64)
        for yy, xx, wgt in ((y0, x0, (1.0 - fx) * (1.0 - fy)), (y0, x1, fx * (1.0 - fy)), (y1, x0, (1.0 - fx) * fy), (y1, x1, fx * fy)):
            counts = has[yy, xx] & (labels[yy, xx] == L)
            c = code[yy, xx] - ZERO
            S = S + np.where(counts, wgt * c.astype(np.float64), 0.0)
            W = W + np.where(counts, wgt, 0.0)
            total += np.where(counts, c, 0)
            count += counts
        any_tap = ok & (count > 0)
        weighted = (S / np.where(W > 0.0, W, 1.0)) * np.float64(unit)
        plain = (total.astype(np.float64) / np.maximum(count, 1).astype(np.float64)) * np.float64(unit)
        d = np.where(W > 0.0, weighted, np.where(count > 0, plain, 0.0))
        moved = P + d[:, None] * (n / np.where(ok, length, 1.0)[:, None])
    return np.where(ok[:, None], moved, P), any_tap.astype(np.uint8)


# ---- properties the host test checks -----------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_use(faces):
    """(undirected edges [n,2], how many triangles use each)"""
    return np.unique(np.sort(directed_edges(faces), axis=1), axis=0, return_counts=True)


def area(vertices, faces):
    v = np.asarray(vertices, np.float64)
    a, b, c = (v[np.asarray(faces, np.int64)[:, n]] for n in range(3))
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
