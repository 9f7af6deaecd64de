"""
Designed inputs of the face.obj export's per-vertex and per-line checks, shared by tests/test_obj_cases_host.py (CPU) and
tests/test_gpu_obj_cases.py.  Plain numpy, no topo4d_amd code; every case is a closed description with a fixed seed.

Meshes (mesh(name): float32 vertices [P,3], int64 faces [F,3], and `marks`, the rows each class expects):

  head      the 8,280-vertex scaffold head of tests/test_gpu_objexport.head_surface
  fan       a hub in 2,000 triangles of a wavy rim; every fourth rim vertex starts one more triangle along the rim, so rim
            vertices have valence 2 or 3; the faces are listed in shuffled order
  repeats   a small soup plus faces that name a vertex twice and three times (their angles at the vertex are summed, then
            multiplied by the zero normal of a zero cross product), and one vertex whose only face is itself three times
  thin      triangles with a smallest angle of 2.5e-9 (degenerate by tol.merge = 1e-8) and of 4e-8 (not), at each corner;
            right triangles with legs of 1.5e-7 (cross product 2.25e-14 <= tol.zero = 1e-13: a zero normal, angles kept) and of
            1.5e-6 (2.25e-12, a normal); a vertex shared by a tiny and an ordinary triangle.  Nothing within a factor 4 of
            either threshold, so one ulp in acos or sqrt cannot change a class
  cancel    a soup, vertices whose only faces are one triangle in both windings with the vertex named first (the same angle
            and exactly opposite normals: the sum is exactly 0), and collinear triangles whose vertices have no other face
  edge<n>   n = 1, 255, 256, 257, 511, 513, 65537 vertices on a bumpy sphere, faces (i, i+1, i+2) mod n; n = 1 is the face
            (0, 0, 0).  The block edges of every per-vertex kernel and the trips of the offsets' scan
  hi        a 364 x 364 lat-long grid, 132,496 vertices and 264,264 triangles: a level-2 face_hi.obj of the head

Push parameter sets (push_case(kind, normals)): see PUSH_KINDS and push_case.  Text rows: float_rows, face_lists.

C_REF is the constant of the normals' bound, measured by tests/test_obj_cases_host.py::test_normals_constant.
"""
import functools
import types

import numpy as np

# The largest error / (2^-53 kappa_v) of the float64 restatement against the long-double rule over every designed mesh,
# rounded up; tests/test_obj_cases_host.py recomputes it and holds it to this value.
C_REF = 8.0

EDGE_COUNTS = (1, 255, 256, 257, 511, 513, 65537)
MESH_NAMES = ("head", "fan", "repeats", "thin", "cancel") + tuple(f"edge{n}" for n in EDGE_COUNTS) + ("hi",)
SMALL_MESHES = tuple(n for n in MESH_NAMES if n not in ("hi", "edge65537"))
THIN_DEGENERATE, THIN_KEPT = 2.5e-9, 4e-8
TINY_LEG = 1.5e-7
FAN_TRIANGLES = 2000


def _mesh(vertices, faces, **marks):
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    v.setflags(write=False)
    f.setflags(write=False)
    return types.SimpleNamespace(vertices=v, faces=f, marks={k: np.asarray(a, dtype=np.int64) for k, a in marks.items()})


def _soup(n, seed):
    """n points on a bumpy sphere and the faces (i, i+1, i+2) mod n: every vertex in three random triangles."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = d * rng.uniform(0.8, 1.2, (n, 1))
    i = np.arange(n)
    return pts, np.stack([i, (i + 1) % n, (i + 2) % n], axis=1)


def _head():
    from tests.test_gpu_objexport import head_surface
    return _mesh(*head_surface())


def _fan():
    n = FAN_TRIANGLES
    t = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(t), np.sin(t), 0.05 * np.sin(7 * t)], axis=1)
    verts = np.vstack([[0.0, 0.0, 0.5], rim])
    i = np.arange(n)
    spokes = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1)
    j = np.arange(0, n - 4, 4)
    along = np.stack([1 + j, 1 + j + 2, 1 + j + 1], axis=1)
    faces = np.vstack([spokes, along])
    faces = faces[np.random.default_rng(5).permutation(len(faces))]
    return _mesh(verts, faces, hub=[0])


def _repeats():
    pts, faces = _soup(12, 21)
    verts = np.vstack([pts, [[0.3, -0.2, 1.5]]])
    extra = [[0, 0, 1], [2, 3, 2], [4, 4, 4], [5, 6, 6], [7, 8, 7], [12, 12, 12]]
    return _mesh(verts, np.vstack([faces, extra]), repeated=np.arange(12, 18), zero=[12])


def _thin():
    verts, faces, degenerate, flat = [], [], [], []

    def add(tri, roll=0):
        base = len(verts)
        verts.extend(tri)
        faces.append([base + (k + roll) % 3 for k in range(3)])
        return len(faces) - 1

    x = 0.0
    for angle, into in ((THIN_DEGENERATE, degenerate), (THIN_KEPT, None)):
        for roll in range(3):                                          # the thin angle at corner 0, 2 and 1 of the face
            f = add([[x, 0.0, 0.0], [x + 1.0, 0.0, 0.0], [x + 1.0, angle, 0.0]], roll)
            if into is not None:
                into.append(f)
            x += 2.0
    for scale, into in ((1.0, flat), (10.0, None)):
        for roll in range(3):
            leg = TINY_LEG * scale
            f = add([[0.0, 0.0, 0.0], [leg, 0.0, 0.0], [0.0, 0.0, leg]] if roll == 1 else
                    [[0.0, 0.0, 0.0], [leg, 0.0, 0.0], [0.0, leg, 0.0]], roll)
            if into is not None:
                into.append(f)
    # one vertex at the origin in a tiny triangle (its angle counts, its normal is zero) and in an ordinary one
    shared = len(verts)
    f = add([[0.0, 0.0, 0.0], [TINY_LEG, 0.0, 0.0], [0.0, TINY_LEG, 0.0]])
    flat.append(f)
    verts.extend([[0.0, 1.0, 0.5], [0.0, 0.3, 1.0]])
    faces.append([shared, shared + 3, shared + 4])
    return _mesh(verts, faces, degenerate_faces=degenerate, zero_normal_faces=flat, shared=[shared])


def _cancel():
    pts, faces = _soup(30, 22)
    rng = np.random.default_rng(23)
    verts, faces = list(pts), faces.tolist()
    zero = []
    for j in range(8):                                                 # one triangle in both windings, the vertex first
        v = len(verts)
        verts.append(rng.normal(size=3) * 1.5)
        faces += [[v, 3 * j, 3 * j + 1], [v, 3 * j + 1, 3 * j]]
        zero.append(v)
    for j, axis in enumerate(np.eye(3)):                               # collinear triangles of their own vertices
        v = len(verts)
        verts += [axis * (5.0 + k) + np.roll(axis, 1) * j for k in range(3)]
        faces += [[v, v + 1, v + 2], [v + 2, v, v + 1]][:1 + j % 2]
        zero += [v, v + 1, v + 2]
    return _mesh(verts, faces, zero=zero)


def _edge(n):
    if n == 1:
        return _mesh([[0.25, -1.0, 3.0]], [[0, 0, 0]], zero=[0])
    return _mesh(*_soup(n, 100 + n))


HI_LAT = HI_LON = 364


def _hi():
    i, j = np.meshgrid(np.arange(HI_LAT), np.arange(HI_LON), indexing="ij")
    theta = np.pi * (0.03 + 0.94 * i / (HI_LAT - 1))
    phi = 2 * np.pi * j / HI_LON
    rng = np.random.default_rng(31)
    radius = 1.0 + 0.05 * np.sin(5 * phi) * np.cos(3 * theta) + 0.0005 * rng.normal(size=theta.shape)
    pts = np.stack([0.8 * radius * np.sin(theta) * np.cos(phi), radius * np.cos(theta), 0.9 * radius * np.sin(theta) * np.sin(phi)],
                   axis=-1).reshape(-1, 3)
    v = lambda a, b: (a * HI_LON + b % HI_LON).ravel()
    a, b = i[:-1], j[:-1]
    quads = np.stack([v(a, b), v(a + 1, b), v(a + 1, b + 1), v(a, b + 1)], axis=1)
    faces = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    return _mesh(pts, faces)


def hi_uv():
    """(uvs [P + 364, 2], uv_faces [F,3]) of `hi`: a seam column where the longitude wraps, as head_mesh has it."""
    i, j = np.meshgrid(np.arange(HI_LAT), np.arange(HI_LON), indexing="ij")
    uvs = np.vstack([np.stack([j / HI_LON, i / (HI_LAT - 1)], axis=-1).reshape(-1, 2),
                     np.stack([np.ones(HI_LAT), np.arange(HI_LAT) / (HI_LAT - 1)], axis=1)])
    u = lambda a, b: np.where(b == HI_LON, HI_LAT * HI_LON + a, a * HI_LON + b % HI_LON).ravel()
    a, b = i[:-1], j[:-1]
    quads = np.stack([u(a, b), u(a + 1, b), u(a + 1, b + 1), u(a, b + 1)], axis=1)
    return uvs, np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name.startswith("edge"):
        return _edge(int(name[4:]))
    return {"head": _head, "fan": _fan, "repeats": _repeats, "thin": _thin, "cancel": _cancel, "hi": _hi}[name]()


def broken_mesh():
    """A soup of 40 vertices with 3 corners out of range (-1, 40 and 2^31 - 1) and 2 vertices (38, 39) in no face."""
    pts, faces = _soup(38, 41)
    faces = np.vstack([faces, [[0, -1, 1], [40, 2, 3], [4, 5, 2 ** 31 - 1]]])
    return np.vstack([pts, pts[:2] + 1.0]).astype(np.float32), faces, 3, 2


# ---- the push ---------------------------------------------------------------------------------------------------------------
PUSH_KINDS = ("unit", "typical", "clamp_edge", "overflow", "vanish", "vanish_nan", "zero_normal")
CLAMP = np.float32(0.001)
EDGE_STEP = 2.0 ** -10


def quaternions(n, rng):
    """Random rotations as float32 quaternions whose norms run from 1e-2 to 1e2; none is zero."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return (q * 10.0 ** rng.uniform(-2, 2, (n, 1))).astype(np.float32)


def push_case(kind, normals, seed=0):
    """The inputs of k_obj_frame_vertices for one class, one row per row of `normals` (float64 [n,3], non-zero unless the class
    says otherwise), and what each row's cast must be: (log_scales, rotations, normals, expect), expect a [n] array of
    "clamp" (exactly float32(0.001)), "zero" (exactly 0), "nan" or "free" (bounded against the rule).

      unit         log_scales = 0: exp is exactly 1, the cast is 1 / |R^-1 n| ~ 1 and clamps
      typical      log_scales uniform in [-11, -4]
      clamp_edge   one scale on all three axes, log(0.001 (1 + 2^-10)) on even rows (clamps) and log(0.001 (1 - 2^-10)) on
                   odd rows (does not): the cast is that scale over |R^-1 n|
      overflow     log_scales = 89 (exp overflows float32) on one, two and all three axes in turn, 0 on the others: the terms
                   of the overflowing axes are 0; with all three acc = 0, then inf, then 0.001
      vanish       log_scales = -60: s is normal and s * s is below half the smallest denormal, exactly 0; acc = inf, cast 0
      vanish_nan   even rows: vanish with the normal along an axis and the rotation (q, 0, 0, 0), so two of the three
                   (R^-1 n)_a are exactly 0 and 0 / 0 makes the row NaN, as torch does; odd rows: vanish
      zero_normal  the normals replaced by 0 (what `cancel` gives): 1 / 0 = inf clamps, and the push is 0.001 * 0"""
    rng = np.random.default_rng([seed, PUSH_KINDS.index(kind)])
    normals = np.array(normals, dtype=np.float64)
    n = len(normals)
    rot = quaternions(n, rng)
    row = np.arange(n)
    ls = np.zeros((n, 3), np.float32)
    expect = np.full(n, "clamp", dtype=object)
    if kind == "typical":
        ls = rng.uniform(-11, -4, (n, 3)).astype(np.float32)
        expect[:] = "free"
    elif kind == "clamp_edge":
        ls[:] = np.log(0.001 * np.where(row % 2 == 0, 1 + EDGE_STEP, 1 - EDGE_STEP))[:, None]
        expect[row % 2 == 1] = "free"
    elif kind == "overflow":
        axes = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
        for k, ax in enumerate(axes):
            ls[np.ix_(row[row % 7 == k], ax)] = 89.0
    elif kind in ("vanish", "vanish_nan"):
        ls[:] = -60.0
        expect[:] = "zero"
        if kind == "vanish_nan":
            even = row % 2 == 0
            normals[even] = np.eye(3)[(row[even] // 2) % 3] * np.where(row[even] % 4 == 0, 1.0, -1.0)[:, None]
            rot[even] = 0.0
            rot[even, 0] = (10.0 ** rng.uniform(-2, 2, int(even.sum()))).astype(np.float32)
            expect[even] = "nan"
    elif kind == "zero_normal":
        normals[:] = 0.0
        ls = rng.uniform(-11, -4, (n, 3)).astype(np.float32)
    elif kind != "unit":
        raise ValueError(kind)
    return ls, rot, normals, expect


def cast_float64(log_scales, rotations, normals):
    """The unclamped cast in float64 from the same float32 inputs: sqrt(1 / sum_a ((R^-1 n)_a / exp(log_s_a))^2), R^-1 = R^T
    of the normalised quaternion."""
    q = np.asarray(rotations, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    nr = np.einsum("nba,nb->na", R, np.asarray(normals, np.float32).astype(np.float64))
    s = np.exp(np.asarray(log_scales, np.float32).astype(np.float64))
    return np.sqrt(1.0 / ((nr / s) ** 2).sum(1))


# ---- text -------------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 255, 256, 257, 65535, 65536, 65537, 65536 + 257, 131073)


def float_rows(rows, cols, seed):
    """[rows, cols] float64 whose printed lengths run from 3 to 24 characters within one block: 0.0, -0.0, integers of one to
    three digits, random bit patterns (17 significant digits, every exponent, an occasional NaN payload), 17-digit values near
    1, 1e16 and 1e-05 (where repr changes notation), subnormals, inf and nan.  Row 0 is the shortest line and, with more than
    one row, row 1 the longest."""
    rng = np.random.default_rng([seed, rows, cols])
    n = rows * cols
    pick = rng.integers(0, 10, n)
    bits = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)
    vals = np.select([pick == 0, pick == 1, pick == 2, pick == 3, pick == 4, pick == 5, pick == 6, pick == 7],
                     [0.0, -0.0, rng.integers(-99, 1000, n).astype(np.float64), rng.uniform(-2, 2, n),
                      rng.choice([1e16, 1e-05, 9999999999999998.0, 0.0001, -1e16, 1e22], n),
                      rng.choice([5e-324, -5e-324, 2.2250738585072009e-308, 1.2345678901234e-310], n),
                      rng.choice([np.inf, -np.inf, np.nan], n), rng.uniform(-1e3, 1e3, n)], bits).reshape(rows, cols)
    vals[0] = 0.0
    if rows > 1:
        vals[1] = -1.2345678901234567e-105
    return vals


INDEX_POOL = np.array([10 ** k + d for k in range(1, 19) for d in (-2, -1, 0)] + [-1, -2, -11, 2 ** 62 - 1, -(2 ** 62 - 1)] +
                      list(range(0, 3000, 7)), dtype=np.int64)
CORNER_COUNTS = (0, 1, 2, 3, 4, 5, 40)


def face_lists(n_faces, seed, counts=None):
    """n_faces faces as int64 arrays of 0, 1, 2, 3, 4, 5 and 40 corners (the first seven faces have one count each), with
    indices from INDEX_POOL: every 10^k - 2, 10^k - 1 and 10^k for k = 1..18 (the printed index is one more), -1, -2 and -11
    (printed 0, -1, -10), +-(2^62 - 1) and small ones.  counts: the corners per face, to build a uv list of other lengths."""
    rng = np.random.default_rng([seed, n_faces])
    if counts is None:
        counts = rng.choice(CORNER_COUNTS, n_faces, p=[0.05, 0.05, 0.1, 0.4, 0.3, 0.08, 0.02])
        counts[:7] = CORNER_COUNTS[:min(7, n_faces)]
    flat = rng.choice(INDEX_POOL, int(np.sum(counts)))
    flat[:len(INDEX_POOL)] = INDEX_POOL[:len(flat)]
    return np.split(flat, np.cumsum(counts)[:-1]), np.asarray(counts)
