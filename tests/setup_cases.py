"""Designed inputs for the coarse setup kernels: the smallest shapes at which each can still go wrong.  Everything is seeded and
built on the host; tests/test_setup_ref_host.py asserts that each case really contains the edge it is named for, and
tests/test_gpu_setup_cases.py runs them on the device against tests/setup_ref.py."""
import numpy as np

from tests import setup_ref

F32_EPS_BELOW_ONE = 2.0 ** -24                                  # the float32 spacing just below 1


# ---- vertex -> corner CSR --------------------------------------------------------------------------------------------------
CSR_SIZES = (1, 255, 256, 257, 513, 1000)                       # fill 1, 1-, 1, 1+, 2+ and 3+ trips of the 256-wide scan
CSR_HUB_VALENCE = 300


def csr_case(n_vert, n_bad=0):
    """(faces int32 [F,3], unreferenced vertex ids).  A hub vertex in CSR_HUB_VALENCE faces, faces listing a vertex twice and
    three times, and - from 255 vertices on - blocks no face references at the start, in the middle and at the end.  n_bad
    corners are then overwritten with indices outside [0, n_vert)."""
    rng = np.random.default_rng(1000 + n_vert)
    if n_vert == 1:
        faces = np.zeros((5, 3), np.int32)
        unref = np.zeros(0, np.int64)
    else:
        mid = n_vert // 2
        unref = np.concatenate([np.arange(0, 4), np.arange(mid, mid + 7), np.arange(n_vert - 5, n_vert)])
        live = np.setdiff1d(np.arange(n_vert), unref)
        hub = int(live[len(live) // 3])
        cover = np.resize(live, 3 * ((len(live) + 2) // 3)).reshape(-1, 3)      # every live vertex at least once
        soup = rng.choice(live, (200, 3))
        spokes = np.stack([np.full(CSR_HUB_VALENCE, hub), rng.choice(live, CSR_HUB_VALENCE), rng.choice(live, CSR_HUB_VALENCE)], 1)
        a, b, c = (int(x) for x in live[[5, 9, 14]])
        twice = np.array([[a, a, b], [b, c, b], [c, hub, hub], [a, a, a], [hub, hub, hub]])
        faces = np.concatenate([cover, soup, spokes, twice])
        faces = faces[rng.permutation(len(faces))].astype(np.int32)
    if n_bad:
        flat = faces.reshape(-1)
        where = np.linspace(1, flat.size - 1, n_bad).astype(np.int64) if flat.size > n_bad else np.arange(n_bad)
        flat[where] = np.resize(np.array([n_vert, -1, 2 ** 31 - 1, n_vert + 7, -2 ** 31], np.int64), n_bad).astype(np.int32)
    return faces, unref


# ---- vertex colours --------------------------------------------------------------------------------------------------------
TEXTURES = {"1x1": (1, 1, 3), "2x3": (2, 3, 3), "37x29": (37, 29, 3), "16x16rgba": (16, 16, 4)}     # width, height, channels
COLOR_HUB_CORNERS = 300


def texture(name):
    W, H, ch = TEXTURES[name]
    return np.random.default_rng(sum(map(ord, name))).integers(0, 256, (H, W, ch), dtype=np.uint8)


def rounds_up_to_integer(W):
    """u just below k / W whose float64 product u * W is the integer k itself: (u, k) for every such k."""
    out = []
    for k in range(1, W):
        u = float(np.nextafter(k / W, -np.inf))
        if u * W == float(k) and u < k / W:
            out.append((u, k))
    return out


def color_uvs(name):
    """The accepted UVs of one texture, float64 [n,2]: texel corners and centres, integer / negative / -0.0 / 1e-300 u, values in
    (-3, 3), u whose product with the width rounds up to an integer, and positions inside the last column and the last row.  v
    never lands on an integer: there the reference raises (color_refusals)."""
    W, H, _ = TEXTURES[name]
    rng = np.random.default_rng(7 + W * 100 + H)
    uv = []
    for i in range(W):
        for j in range(H):
            uv.append(((i + 0.5) / W, 1 - (j + 0.5) / H))                       # centres
            if j > 0:
                uv.append((i / W, 1 - j / H))                                   # corners (row 0 would be v % 1 == 0)
    for u in (-2.0, -1.0, -0.0, 0.0, 1.0, 2.0, 1e-300, -1.5, 2.25):
        uv.append((u, 0.37))
        uv.append((u, -1.63))
    for u, _k in rounds_up_to_integer(W):
        uv.append((u, 0.61))
    for t in (0.01, 0.3, 0.5, 0.999):
        uv.append(((W - 1 + t) / W, 0.45))                                      # inside the last column
        uv.append((0.2, (1 - t) / H))                                           # inside the last row
        uv.append(((W - 1 + t) / W - 2, (1 - t) / H + 1))                       # both, through the % 1
    uv += rng.uniform(-3, 3, (150, 2)).tolist()
    uv = np.asarray(uv, np.float64)
    img = texture(name)
    ok = np.array([setup_ref.corner_color(img, u, v) is not None for u, v in uv])
    return uv[ok]


def color_case(name, n_vert=40):
    """(image, corner_uvs [3F,2], faces int32 [F,3], n_vert): color_uvs(name) cycled over at least COLOR_HUB_CORNERS + 4 n_vert
    corners; every vertex has a corner and vertex 0 has COLOR_HUB_CORNERS more."""
    uv = color_uvs(name)
    rng = np.random.default_rng(len(uv))
    n = 3 * ((max(len(uv), COLOR_HUB_CORNERS + 4 * n_vert) + 2) // 3)
    corner_uvs = np.resize(uv, (n, 2))
    verts = np.concatenate([rng.permutation(n_vert), np.zeros(COLOR_HUB_CORNERS, np.int64),
                            rng.integers(0, n_vert, n - n_vert - COLOR_HUB_CORNERS)])
    return texture(name), corner_uvs, verts[rng.permutation(n)].reshape(-1, 3).astype(np.int32), n_vert


# corner index -> UV the reference raises on; more than 256 corners apart, the lowest past the first 256-corner workgroup
COLOR_REFUSALS = {301: (float("nan"), 0.5), 600: (0.5, 0.0), 900: (0.25, 1.0), 1201: (-1e-20, 0.5)}


def color_refusal_case(which=tuple(COLOR_REFUSALS)):
    img, uv, faces, n_vert = color_case("37x29")
    uv = np.resize(uv, (1260, 2)).copy()
    faces = np.resize(faces.reshape(-1), 1260).reshape(-1, 3)
    for c in which:
        uv[c] = COLOR_REFUSALS[c]
    return img, uv, faces, n_vert


# ---- quaternions -----------------------------------------------------------------------------------------------------------
def quaternion_normals():
    """(normals float64 [N,3], {group: row slice}).  Groups: ordinary unit normals; the six axes; +-x tilted so that the float32
    unit vector's x is 1 or 2 float32 ulp short of +-1; ordinary normals scaled by 1e-3, 1e3 (harmless) and 1e-30, 1e30 (the
    float32 squares underflow to 0 / overflow to inf); a zero normal and a NaN component."""
    rng = np.random.default_rng(45)
    plain = rng.normal(size=(64, 3))
    plain /= np.linalg.norm(plain, axis=1, keepdims=True)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    tilted = []
    for k in (1, 2):
        for sx in (1.0, -1.0):
            for sy in (1.0, -1.0):
                tilted.append([sx * (1 - k * F32_EPS_BELOW_ONE), sy * np.sqrt(2 * k * F32_EPS_BELOW_ONE), 0.0])
    groups, rows, at = {}, [], 0
    for name, block in (("plain", plain), ("axes", axes), ("tilted", np.array(tilted)), ("x1e-3", plain[:8] * 1e-3),
                        ("x1e3", plain[8:16] * 1e3), ("x1e-30", plain[16:24] * 1e-30), ("x1e30", plain[24:32] * 1e30),
                        ("zero", np.zeros((1, 3))), ("nan", np.array([[0.3, np.nan, 0.1], [np.nan, 0.0, 1.0]]))):
        rows.append(block)
        groups[name] = slice(at, at + len(block))
        at += len(block)
    return np.concatenate(rows), groups


# ---- the one ring ----------------------------------------------------------------------------------------------------------
ONE_RING_SHAPES = [(1, 1), (1, 8), (1, 13), (257, 1), (257, 8), (257, 13)]
EXP_ONE_BELOW = 2.0 ** -55            # 2000 wh at or below this: exp(-2000 wh) > 1 - 2^-55, any faithful exp returns exactly 1
EXP_ONE_ABOVE = 2.0 ** -51            # at or above this: exp(-2000 wh) < 1 - 3 * 2^-53, no faithful exp returns 1
STEP = 2.0 ** -34                     # the float32 spacing in [2^-11, 2^-10)
ANCHOR = 20                           # the vertex the threshold pairs are measured from
# vertex -> its offset from ANCHOR in units of STEP.  (7, 3, 1): 4.47e-10 away, wh = 59 * 2^-68 = 2.0e-19, 2000 wh = 3.6 * 2^-53:
# the float64 exponential is 0.9999999999999996, which float32 rounds to 1.0f - kept, not zeroed.
BELOW_ONE = {21: (1, 0, 0), 22: (1, 1, 1)}
ABOVE_ONE = {23: (7, 3, 1), 24: (9, 0, 0), 25: (0, 16, 0), 26: (40, -30, 20)}
ISSUE_PAIR = 23
# neighbours (in eye_del) of a vertex at the origin (not in it) for which sum((d * 1000)^2) and sum(d^2) * 1e6 differ in the last
# bit AND the two exponentials fall on different sides of a float32 rounding boundary, each at least 4 float64 ulp from it.
# Found by a seeded random search over float32 offsets; test_setup_ref_host.py checks the property with mpmath.
EYE_LAST_BIT = [("0x1.e8b122p-15", "0x1.259016p-14", "-0x1.9caf6p-14"),
                ("0x1.95a39ep-14", "-0x1.cd78cp-15", "0x1.f69198p-14"),
                ("-0x1.475ad8p-13", "-0x1.8f4ad6p-14", "-0x1.129ee2p-14"),
                ("0x1.0cee36p-13", "-0x1.1fc36ep-14", "-0x1.a1f692p-14"),
                ("0x1.4b3388p-13", "-0x1.7fa87ep-14", "0x1.3d31bp-14"),
                ("0x1.4f14a4p-13", "-0x1.398d2p-14", "-0x1.bfeafp-14")]
EYE_ORIGINS, EYE_TARGETS = 50, 60     # origin vertices 50.., their neighbours 60..
EYE_COMBOS = {40: 44, 41: 45, 42: 46, 43: 47}                   # v -> j, the same two positions under each membership
EYE_DEL = [40, 44, 41, 46, 10 ** 6, -1, 100, 101]               # (in, in), (in, out), (out, in), (out, out); values no index equals


def one_ring_case(P, K):
    """(means3D float32 [P,3], nbr int64 [P,K], eye_del list).  For P == 257 slot 0 of the designed vertices holds: coincident
    pairs (10 <-> 11, and 255 <-> 256 across the first workgroup's end for K == 1); pairs on both sides of the exp == 1
    threshold and none between; far pairs whose weight is a float32 denormal, a float64 denormal and 0; the four eye memberships
    over one geometry; the EYE_LAST_BIT entries.  Padded slots (j == v) end every third row."""
    rng = np.random.default_rng(P * 100 + K)
    if P == 1:
        return np.array([[0.1, -0.2, 0.3]], np.float32), np.zeros((1, K), np.int64), [0]
    x = rng.uniform(-0.05, 0.05, (P, 3)).astype(np.float32)
    nbr = rng.integers(0, P, (P, K))
    nbr[::3, K - max(1, K // 3):] = np.arange(P)[::3, None]
    x[11], x[256] = x[10], x[255]
    pairs = {10: 11, 11: 10, 255: 256, 256: 255}
    x[ANCHOR] = np.array([1.25, 1.5, 1.75], np.float32) * np.float32(2.0 ** -11)
    for v, steps in {**BELOW_ONE, **ABOVE_ONE}.items():
        x[v] = (x[ANCHOR].astype(np.float64) + np.array(steps) * STEP).astype(np.float32)
        pairs[v] = ANCHOR
    pairs[ANCHOR] = 21
    x[30] = 10.0
    x[32] = x[33] + np.array([0.2236, 0, 0], np.float32)         # exp(-100): a float32 denormal
    x[34] = x[35] + np.array([0.61, 0, 0], np.float32)           # exp(-744.2): a float64 denormal, float32 0
    pairs.update({30: 31, 31: 30, 32: 33, 34: 35})
    for v, j in EYE_COMBOS.items():
        x[v] = np.array([0.01, 0.02, -0.01], np.float32)
        x[j] = x[v] + np.array([1e-5, 2e-5, -1.5e-5], np.float32)
        pairs[v] = j
    eye = list(EYE_DEL)
    for i, a in enumerate(EYE_LAST_BIT):
        x[EYE_ORIGINS + i] = 0.0
        x[EYE_TARGETS + i] = np.array([float.fromhex(h) for h in a], np.float32)
        pairs[EYE_ORIGINS + i] = EYE_TARGETS + i
        eye.append(EYE_TARGETS + i)
    for v, j in pairs.items():
        nbr[v, 0] = j
    return x, nbr.astype(np.int64), eye


def one_ring_refusal_case(n_bad):
    x, nbr, eye = one_ring_case(257, 8)
    flat = nbr.reshape(-1)
    flat[[300, 700, 1500][:n_bad]] = [257, -1, 2 ** 40][:n_bad]
    return x, nbr, eye


# ---- region weights --------------------------------------------------------------------------------------------------------
REGION_P, REGION_K = 37, 7                                      # 259 elements: one past a 256-thread workgroup
REGION_FACTORS = [0.1, 0.5 / 3.5, 5.0 / 20.0, 0.0, 0.1 / 3.5, 50.0 / 20.0, 1.0 / 20.0]
EVERY_MASK_ROW = 3


def region_input():
    rng = np.random.default_rng(99)
    w = rng.uniform(0.0, 1.0, (REGION_P, REGION_K)).astype(np.float32)
    w[5, 2], w[8, 0], w[36, 6] = 0.0, 1e-42, 1.0
    return w


def region_cases():
    """{name: (masks, factors float32)}; a mask is a list of rows (duplicates kept, as a caller may pass them)."""
    rng = np.random.default_rng(5)
    P = REGION_P
    nz = [f for f in REGION_FACTORS if f != 0.0]
    cases = {"none": ([], [])}
    cases["one_duplicated_rows"] = ([[4, 4, 9, 36, 9, 4, 0]], [0.1])
    # 11 masks: empty ones first, in the middle and last; 0.0 before and after nonzero factors; random membership
    masks = [sorted(rng.choice(P, int(rng.integers(3, 20)), replace=False).tolist()) for _ in range(11)]
    for m in (0, 5, 10):
        masks[m] = []
    cases["eleven_with_empty"] = (masks, [0.5 / 3.5, 0.1, 0.0, 5.0 / 20.0, 0.1 / 3.5, 0.7, 50.0 / 20.0, 0.0, 1.0 / 20.0, 0.1, 0.3])
    masks = [sorted(set(rng.choice(P, int(rng.integers(3, 20)), replace=False).tolist()) - {6} | {EVERY_MASK_ROW}) for _ in range(11)]
    masks[2] = masks[2] + masks[2][:3]
    cases["eleven_row_in_all"] = (masks, [nz[i % len(nz)] for i in range(11)])
    cases["eleven_all_empty"] = ([[] for _ in range(11)], [0.1] * 11)
    masks = [sorted(set(rng.choice(P, int(rng.integers(2, 9)), replace=False).tolist()) - {6, 7} | {EVERY_MASK_ROW}) for _ in range(32)]
    masks[31] = masks[31] + [6]
    masks[0] = masks[0] + [7]
    cases["thirty_two"] = (masks, rng.uniform(0.8, 1.25, 32).tolist())
    return {k: (m, np.asarray(f, np.float32)) for k, (m, f) in cases.items()}


# ---- flatten edges ---------------------------------------------------------------------------------------------------------
FLATTEN_SIZES = (255, 256, 257, 1500)
TRIP = 256
# candidate positions whose edge gets a third (or fourth) face: before, at and after the ends of the first two trips
DROP_AT = (3, 100, 254, 255, 256, 257, 300, 510, 511, 512, 513, 700, 1400)


def _n_candidates(faces):
    return len(setup_ref.candidate_edges(np.asarray(faces)))


def flatten_case(n_edges):
    """faces int64 [F,3] with exactly n_edges candidate edges (1500: at least).  A triangulated grid whose faces list their
    corners in a seeded rotation, taken face by face until the candidate count is reached; two faces listing a vertex twice on
    edges that already have two faces (one as face 0, one late); then faces duplicated (same corner order, so no new candidate)
    until the candidates at DROP_AT have three or four faces.  Boundary edges keep one face."""
    rng = np.random.default_rng(n_edges)
    cols = 12
    rows = n_edges // 20 + 3
    vid = lambda r, c: r * (cols + 1) + c
    pool = []
    for r in range(rows):
        for c in range(cols):
            a, b, d, e = vid(r, c), vid(r, c + 1), vid(r + 1, c), vid(r + 1, c + 1)
            for tri in ([a, b, e], [a, e, d]):
                k = int(rng.integers(0, 3))
                tri = tri[k:] + tri[:k]
                pool.append(tri[::-1] if rng.integers(0, 2) else tri)
    faces = pool[:24]
    pool = pool[24:]

    def two_face_edge(fs, skip=()):
        holders = {}
        for k, f in enumerate(fs):
            for x in set(f):
                holders.setdefault(x, set()).add(k)
        for a, b in setup_ref.candidate_edges(np.asarray(fs)):
            if a != b and len(holders[a] & holders[b]) == 2 and (a, b) not in skip:
                return a, b
        raise AssertionError("no two-face edge")

    a, c = two_face_edge(faces)
    faces = [[a, a, c]] + faces                                     # the lowest face id of edge (a, c)
    a2, c2 = two_face_edge(faces[1:], skip={(a, c)})
    faces = faces + [[c2, a2, c2]]                                  # ... and the highest of (a2, c2)
    for tri in pool:
        if _n_candidates(faces) >= n_edges:
            break
        if _n_candidates(faces + [tri]) <= n_edges:
            faces.append(tri)
    cand = setup_ref.candidate_edges(np.asarray(faces))
    for n, pos in enumerate(p for p in DROP_AT if p < len(cand)):
        a, b = cand[pos]
        host = next(f for f in faces if a in f and b in f and len(set(f)) == 3)
        held = sum(1 for f in faces if a in f and b in f)
        faces = faces + [host] * max(1, 3 + n % 2 - held)           # three faces, or four (or more, where copies overlap)
    return np.asarray(faces, np.int64)


FULLY_DEGENERATE = np.array([[0, 1, 2], [2, 1, 3], [4, 4, 4]], np.int64)


# ---- FlattenLoss_v2's mask -------------------------------------------------------------------------------------------------
def neighbor_mask_cases():
    """[(neighbor_num int64 [P], K)]: every count from 0 to K, P * K * 3 just past 256."""
    return [(np.arange(90, dtype=np.int64) % 2, 1), (np.arange(11, dtype=np.int64) % 9, 8)]
