"""Clouds, a reference and a restatement of the walk for the exact kNN of csrc/t4d_dense.hip (t4d_knn_mean_sq_dist).

  CASES       name -> builder(seed): seeded float64 clouds [n,3]; `cloud(name)` builds one with its seed in SEEDS, once.  SMALL are
              the ones with n <= 4096 (every degenerate cloud is among them: an all-in-one-cell or all-fall-through cloud costs n^2
              distance evaluations in one kernel), LARGE the threshold and workload-size ones.
  reference   the expected means in float64 for every row: knn_mean_sq_dist_numpy up to 4096 points, above that candidates from
              scipy's cKDTree with the distances recomputed, each row certified or redone by brute force (reference_tree).
  expected    reference(cloud(name), k), computed once and shared read-only.
  walk_plan   the rule of k_grid / k_knn_grid restated in numpy, for the small cases: per query the shell radius at which the walk
              ends, whether the cube covered the grid, whether the query falls through to the brute pass, and the value the walk
              gives.  It shows on the CPU which branch a case reaches; it is not the reference for values.  It restates kMaxShells,
              the cell rule and the stop rule's margin: if one of them changes in the kernel, change it here.
"""
import functools

import numpy as np

EXTRA = 8                   # candidates asked from the tree beyond the k+1 that make the answer
MAX_SHELLS = 4              # kMaxShells
BRUTE_LIMIT = 4096          # reference() is the plain brute force up to here; no degenerate case may be larger
KS = (1, 2, 4, 8, 15)


# ----------------------------------------------------------------------------------------------------------------------------
# clouds
# ----------------------------------------------------------------------------------------------------------------------------
def sphere(seed, n=3000):
    """random points on an ellipsoid surface, semi-axes (80, 110, 90)"""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * np.array([80.0, 110.0, 90.0])


HALO_RANGE = (1.05, 3.0)    # tuned on the CPU: together with the other small cases every shell radius 0..4 ends a walk


def halo(seed):
    """sphere plus 96 surface points scaled radially: a sparse second layer whose neighbours lie shells away"""
    s = sphere(seed)
    rng = np.random.default_rng(seed + 1000)
    extra = s[rng.choice(s.shape[0], 96, replace=False)] * np.linspace(HALO_RANGE[0], HALO_RANGE[1], 96)[:, None]
    return np.concatenate([s, extra])


def plane(seed):
    """z constant: one extent 0, dim = 1 on that axis"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-50, 50, 1500), rng.uniform(0, 120, 1500), np.full(1500, 7.25)], 1)


def line_axis(seed):
    """y and z constant: area 0, the cell falls back to emax * 2^-20, every point alone in its cell, every query falls through"""
    x = np.random.default_rng(seed).uniform(0, 1000, 800)
    return np.stack([x, np.full(800, -3.5), np.full(800, 12.0)], 1)


def line_diag(seed):
    t = np.random.default_rng(seed).uniform(0, 100, 800)
    return np.stack([t, t, t], 1)


def same(seed):
    """one point repeated: all extents 0, the cell is forced to 1.0"""
    p = np.random.default_rng(seed).uniform(-10, 10, 3)
    return np.tile(p, (2048, 1))


def dups(seed):
    """sphere with 500 rows repeated exactly, 100 of them three times"""
    s = sphere(seed)
    rows = np.random.default_rng(seed + 1000).choice(s.shape[0], 500, replace=False)
    return np.concatenate([s, s[rows], s[rows[:100]]])


def two_clusters(seed):
    """two Gaussian blobs 10^4 sigma apart: the bounding box is nearly empty, each blob sits in one cell"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(size=(600, 3)), rng.normal(size=(600, 3)) + np.array([6000.0, 0.0, 8000.0])])


def volume(seed):
    """uniform in a cube: not a surface, several points per cell"""
    return np.random.default_rng(seed).uniform(0, 100, (1500, 3))


def lattice(seed):
    """12 x 12 x 10 integer lattice in a seeded row order: exact ties at every rank"""
    g = np.stack(np.meshgrid(np.arange(12.0), np.arange(12.0), np.arange(10.0), indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(g.shape[0])]


def lattice_far(seed):
    return (lattice(seed) * 0.25 + np.array([4096.0, -2048.0, 1024.0])).astype(np.float32).astype(np.float64)


def far_f64(seed):
    """extent 0.2 at 1e7: the coordinates' spacing (1.9e-9) is above the stop rule's margin (1e-9 of the grid's extent)"""
    return sphere(seed) * 1e-3 + 1e7


def outliers(seed):
    """two far points inflate the bounding box: the sphere collapses into a few cells, the far points fall through"""
    return np.concatenate([sphere(seed, 1000), [[1e5, 1e5, 1e5], [-1e5, 0.0, 0.0]]])


def minimal(seed, k):
    """n = k + 1"""
    return np.random.default_rng(seed).uniform(-1, 1, (k + 1, 3))


def bbox_edge(seed, n):
    """sphere with its six extreme points in the last rows: a bounding-box pass that drops the tail gets the grid wrong"""
    s = sphere(seed, n)
    last = np.unique(np.concatenate([s.argmin(0), s.argmax(0)]))
    keep = np.ones(n, bool)
    keep[last] = False
    return np.concatenate([s[keep], s[last]])


STOP_EDGE_GROUPS = 62


def stop_edge(seed):
    """A cloud built against the stop rule at k = 4.  Eight corners fix the box at [0, 64]^3; with n = 384 the cell is exactly 16.
    Each of 62 groups sits in an interior cell of its own: a query 3 away from one of the cell's faces (the three axes in turn),
    three companions within 1.5 of it, a fourth in its cell at distance D = 3 (1 + 2^-19), and a point just across that face at
    distance T = 3 (1 + 2^-20).  The answer holds T and not D, and the walk may not stop at radius 0: its fifth candidate there
    is D, farther than the face.  A stop rule more than 4e-6 too eager (relative, in squared distance) returns D instead.  The
    query of group g is row 8 + 6 g."""
    rng = np.random.default_rng(seed)
    corners = np.array([[x, y, z] for x in (0.0, 64.0) for y in (0.0, 64.0) for z in (0.0, 64.0)])
    cells = np.stack(np.unravel_index(rng.permutation(64), (4, 4, 4)), 1).astype(np.float64)
    out = [corners]
    for g in range(STOP_EDGE_GROUPS):
        a = g % 3                                                    # the face: axis a, the side that has a whole cell behind it
        b, c = (a + 1) % 3, (a + 2) % 3
        up = cells[g][a] <= 1
        sign = 1.0 if up else -1.0
        q = cells[g] * 16.0 + 8.0 - sign * 4.0                       # off the cell's centre: clear of the neighbours' points
        q[a] = cells[g][a] * 16.0 + (13.0 if up else 3.0)
        pts = np.tile(q, (6, 1))
        pts[1:4, a] -= sign * rng.uniform(0.25, 0.75, 3)             # companions: away from the face, within 1.5 of the query
        pts[1:4, b] += rng.uniform(-1.0, 1.0, 3)
        pts[1:4, c] += rng.uniform(-0.75, 0.75, 3)
        pts[4, b] += 3.0 + 6.0 * 2.0 ** -20                          # D, in the query's cell
        pts[5, a] += sign * (3.0 + 3.0 * 2.0 ** -20)                 # T, across the face
        out.append(pts)
    rest = cells[STOP_EDGE_GROUPS:] * 16.0 + 8.0                     # two cells left: two filler points each make n = 384
    out.append(np.concatenate([rest, rest + 2.0]))
    return np.concatenate(out)


def head_dense(seed):
    """the dense vertices of a lat-long head (about 2k frontal quads) at density 24: the smallest capture-like lattice with
    n > 2^20 (a table of 2^22 slots: four carry passes of k_scan_i32_sums)"""
    from tests.test_gpu_densify import head_mesh
    from topo4d_amd import densify
    params, faces, uv_faces, uvs, uv_counts, masks = head_mesh(40, 100, seed=seed)
    mesh = densify.build_dense_mesh_numpy(params["means3D"], faces, uv_faces, uvs, uv_counts, masks, 24)
    return np.asarray(mesh["dense_vertex"], np.float64)


CASES = {"sphere": sphere, "halo": halo, "plane": plane, "line_axis": line_axis, "line_diag": line_diag, "same": same, "dups": dups,
         "two_clusters": two_clusters, "volume": volume, "lattice": lattice, "lattice_far": lattice_far, "far_f64": far_f64,
         "outliers": outliers,
         "minimal_k1": functools.partial(minimal, k=1), "minimal_k15": functools.partial(minimal, k=15),
         "scan_edge_512": functools.partial(sphere, n=512), "scan_edge_513": functools.partial(sphere, n=513),
         "bbox_edge_262143": functools.partial(bbox_edge, n=262143), "bbox_edge_262144": functools.partial(bbox_edge, n=262144),
         "bbox_edge_262145": functools.partial(bbox_edge, n=262145),
         "scan_edge_524288": functools.partial(sphere, n=1 << 19), "scan_edge_524289": functools.partial(sphere, n=(1 << 19) + 1),
         "head_dense": head_dense, "stop_edge": stop_edge}
SEEDS = {name: 11 + i for i, name in enumerate(CASES)}
SEEDS["head_dense"] = 3
LARGE = ("bbox_edge_262143", "bbox_edge_262144", "bbox_edge_262145", "scan_edge_524288", "scan_edge_524289", "head_dense")
SMALL = tuple(name for name in CASES if name not in LARGE)


@functools.lru_cache(maxsize=None)
def cloud(name):
    pts = np.ascontiguousarray(CASES[name](SEEDS[name]), np.float64)
    assert pts.ndim == 2 and pts.shape[1] == 3 and np.isfinite(pts).all()
    assert (pts.shape[0] <= BRUTE_LIMIT) == (name in SMALL), name
    pts.setflags(write=False)
    return pts


# ----------------------------------------------------------------------------------------------------------------------------
# reference
# ----------------------------------------------------------------------------------------------------------------------------
def _mean_of_sorted(d, k):
    acc = np.zeros(d.shape[0])
    for m in range(k + 1):                                          # left to right, the point's own zero included
        acc = acc + d[:, m]
    return acc / k


def brute_rows(pts, rows, k):
    """per-row brute force over all points"""
    out = np.empty(len(rows))
    for s in range(0, len(rows), 64):
        q = pts[rows[s:s + 64]]
        dx, dy, dz = (q[:, None, a] - pts[None, :, a] for a in range(3))
        dist = (dx * dx + dy * dy) + dz * dz
        out[s:s + 64] = _mean_of_sorted(np.sort(np.partition(dist, k, axis=1)[:, :k + 1], axis=1), k)
    return out


def reference_tree(pts, k, extra=EXTRA, workers=8):
    """The tree proposes k+1+extra candidates per row; their squared distances are recomputed as ((dx*dx + dy*dy) + dz*dz), sorted,
    and the first k+1 summed left to right.  A row is certified when its recomputed (k+1)-th value times (1 + 2^-40) is below its
    largest candidate value: then no point outside the candidate set can belong to the answer, whatever rounding the tree used.
    The other rows are redone by brute force.  Returns (means, uncertified rows)."""
    from scipy.spatial import cKDTree
    n = pts.shape[0]
    m = min(k + 1 + extra, n)
    idx = cKDTree(pts).query(pts, m, workers=workers)[1].reshape(n, m)
    out = np.empty(n)
    open_rows = []
    for s in range(0, n, 1 << 18):
        c = pts[idx[s:s + (1 << 18)]]                               # [rows, m, 3]
        q = pts[s:s + (1 << 18), None, :]
        dx, dy, dz = q[..., 0] - c[..., 0], q[..., 1] - c[..., 1], q[..., 2] - c[..., 2]
        d = np.sort((dx * dx + dy * dy) + dz * dz, axis=1)
        out[s:s + (1 << 18)] = _mean_of_sorted(d, k)
        if m < n:                                                   # with every point a candidate there is nothing outside
            open_rows.append(s + np.nonzero(~(d[:, k] * (1.0 + 2.0 ** -40) < d[:, -1]))[0])
    open_rows = np.concatenate(open_rows) if open_rows else np.zeros(0, np.int64)
    if open_rows.size:
        out[open_rows] = brute_rows(pts, open_rows, k)
    return out, open_rows


def reference(pts, k, info=None):
    """The expected means for every row; info (a dict) receives the uncertified rows of the tree path."""
    from topo4d_amd import densify
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    if pts.shape[0] <= BRUTE_LIMIT:
        return densify.knn_mean_sq_dist_numpy(pts, k)
    out, open_rows = reference_tree(pts, k)
    if info is not None:
        info["uncertified"] = open_rows
    return out


UNCERTIFIED = {}            # (name, k) -> uncertified rows of the large cases, filled by expected()


@functools.lru_cache(maxsize=None)
def expected(name, k):
    info = {}
    out = reference(cloud(name), k, info)
    if "uncertified" in info:
        UNCERTIFIED[(name, k)] = info["uncertified"]
    out.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the walk of k_grid / k_knn_grid, restated
# ----------------------------------------------------------------------------------------------------------------------------
def grid_of(pts):
    """k_grid: (lo, cell, dim)"""
    n = pts.shape[0]
    lo, hi = pts.min(0), pts.max(0)
    e0, e1, e2 = hi - lo
    emax = max(e0, e1, e2)
    area = 2.0 * (e0 * e1 + e1 * e2 + e0 * e2)
    cell = 2.0 * np.sqrt(area / float(n))
    cell = max(cell, emax * 2.0 ** -20)
    if not cell > 0.0:
        cell = 1.0
    dim = np.floor((hi - lo) / cell).astype(np.int64) + 1
    return lo, float(cell), dim


def walk_plan(pts, k, chunk=256, eager=0.0):
    """Per query: `radius` (the shell radius r at which the walk ends, MAX_SHELLS for a fall-through), `covered` (ended because
    the cube covers the whole grid), `fell` (goes to the brute pass), `mean` (the walk's value, NaN for a fall-through); and the
    grid's `cell` and `dim`.  eager > 0 states a wrong rule, one that stops while the k-th neighbour is still up to sqrt(1 + eager)
    times farther than the nearest open face: the host test uses it to show that a case would notice such a kernel."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n, K = pts.shape[0], k + 1
    lo, cell, dim = grid_of(pts)
    c = np.clip(np.floor((pts - lo) / cell).astype(np.int64), 0, dim - 1)
    margin = 1e-9 * (cell + float(dim.max()) * cell)
    radius = np.full(n, -1)
    covered, fell, mean = np.zeros(n, bool), np.zeros(n, bool), np.full(n, np.nan)
    for s in range(0, n, chunk):
        q, cq = pts[s:s + chunk], c[s:s + chunk]
        m = q.shape[0]
        dx, dy, dz = (q[:, None, a] - pts[None, :, a] for a in range(3))
        dist = (dx * dx + dy * dy) + dz * dz
        cheb = np.abs(cq[:, None, :] - c[None, :, :]).max(-1)
        live = np.ones(m, bool)
        for r in range(MAX_SHELLS + 1):
            seen = np.sort(np.partition(np.where(cheb <= r, dist, np.inf), K - 1, axis=1)[:, :K], axis=1)
            face = np.full(m, np.inf)
            for a in range(3):
                below = q[:, a] - (lo[a] + (cq[:, a] - r).astype(np.float64) * cell)
                above = (lo[a] + (cq[:, a] + r + 1).astype(np.float64) * cell) - q[:, a]
                face = np.where(cq[:, a] - r > 0, np.minimum(face, below), face)
                face = np.where(cq[:, a] + r < dim[a] - 1, np.minimum(face, above), face)
            cover = face == np.inf
            f = face - margin
            with np.errstate(invalid="ignore"):
                stop = cover | (np.isfinite(seen[:, K - 1]) & (f > 0.0) & (seen[:, K - 1] <= f * f * (1.0 + eager)))
            done = live & stop
            rows = s + np.nonzero(done)[0]
            radius[rows], covered[rows], mean[rows] = r, cover[done], _mean_of_sorted(seen[done], k)
            live &= ~stop
        rows = s + np.nonzero(live)[0]
        radius[rows], fell[rows] = MAX_SHELLS, True
    return {"radius": radius, "covered": covered, "fell": fell, "mean": mean, "cell": cell, "dim": dim}
