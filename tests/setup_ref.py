"""Plain restatements of the coarse setup (topo4d_amd/coarse.py over csrc/t4d_setup.hip and t4d_obj_vertex_faces), written from
the reference's behaviour (train.py:177-206, 545-581; helpers.py:181-209, 300-333; external.py:45-61; loss_util.py:114-170,
223-255) with numpy and Python floats.  Each function returns what the device entry returns, plus what the reference would
refuse.  tests/test_setup_ref_host.py anchors them to golden G15 on the CPU; tests/test_gpu_setup_cases.py holds the kernels to
them off the golden scene.  Nothing here touches the device."""
import math

import numpy as np


# ---- vertex -> corner CSR --------------------------------------------------------------------------------------------------
def vertex_corner_csr(faces, n_vert):
    """(offsets int32 [n_vert+1], entries int32 (corner ids 3*f+k, ascending per vertex), n_out_of_range, n_unreferenced) of a
    triangle list; corners naming a vertex outside [0, n_vert) are counted and left out."""
    corners = np.asarray(faces, np.int64).reshape(-1)
    rows = [[] for _ in range(n_vert)]
    bad = 0
    for c, v in enumerate(corners.tolist()):
        if 0 <= v < n_vert:
            rows[v].append(c)
        else:
            bad += 1
    offsets = np.zeros(n_vert + 1, np.int32)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    entries = np.array([c for r in rows for c in r], np.int32).reshape(-1)
    return offsets, entries, bad, sum(1 for r in rows if not r)


# ---- vertex colours --------------------------------------------------------------------------------------------------------
def corner_color(image_u8, u, v):
    """One bilinear texture sample as the reference takes it, in Python floats: (r, g, b) ints, or None where PIL's getpixel
    (column == width, row == height) or int() (NaN) would raise."""
    H, W = image_u8.shape[:2]
    u, v = float(u) % 1, float(v) % 1                          # Python's %: the divisor's sign, +0.0 for a zero remainder
    x, y = u * W, (1 - v) * H
    if math.isnan(x) or math.isnan(y):
        return None
    x1, y1 = int(x), int(y)
    if not (0 <= x1 < W and 0 <= y1 < H):
        return None
    x2, y2 = min(x1 + 1, W - 1), min(y1 + 1, H - 1)
    out = []
    for k in range(3):
        q11, q21 = int(image_u8[y1, x1, k]), int(image_u8[y1, x2, k])
        q12, q22 = int(image_u8[y2, x1, k]), int(image_u8[y2, x2, k])
        top = (x2 - x) * q11 + (x - x1) * q21
        bottom = (x2 - x) * q12 + (x - x1) * q22
        out.append(int((y2 - y) * top + (y - y1) * bottom))    # int(): toward zero
    return tuple(out)


def vertex_colors(image_u8, corner_uvs, faces, n_vert):
    """(colors int32 [n_vert,3], rgb float32 [n_vert,3], n_raise, first_raise, n_unreferenced).  colors: per vertex the mean of
    its corners' samples, truncated; rgb = float32(colors / 255.0).  n_raise corners would raise in the reference (first_raise:
    the lowest such corner index, or None); they contribute nothing here, and a vertex without a sample gets zeros."""
    image_u8 = np.asarray(image_u8)
    uv = np.asarray(corner_uvs, np.float64).reshape(-1, 2)
    corners = np.asarray(faces, np.int64).reshape(-1)
    per = [[] for _ in range(n_vert)]
    raised = []
    for c, vert in enumerate(corners.tolist()):
        col = corner_color(image_u8, uv[c, 0], uv[c, 1])
        if col is None:
            raised.append(c)
        else:
            per[vert].append(col)
    colors = np.zeros((n_vert, 3), np.int32)
    for vert, cols in enumerate(per):
        if cols:
            colors[vert] = np.mean(np.array(cols, np.int64), axis=0).astype(int)
    rgb = (colors.astype(np.float64) / 255.0).astype(np.float32)
    unref = int(n_vert - len(set(corners.tolist())))
    return colors, rgb, len(raised), (raised[0] if raised else None), unref


# ---- quaternions -----------------------------------------------------------------------------------------------------------
def quaternions_torch(normals_f64):
    """The rotation taking +x to each float32 normal, [N,4] float32, with CPU torch ops in the reference's order: unit vector,
    axis = cross(+x, unit), angle = acos(dot(+x, unit)), (cos(angle/2), axis * sin(angle/2))."""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(normals_f64, np.float64)).float()
    unit = d / torch.norm(d, dim=1, keepdim=True)
    ex = torch.tensor([1.0, 0.0, 0.0]).repeat(d.shape[0], 1)
    axis = torch.linalg.cross(ex, unit, dim=1)
    angle = torch.acos(torch.sum(ex * unit, dim=1))
    half = angle / 2
    return torch.cat((torch.cos(half).unsqueeze(1), axis * torch.sin(half).unsqueeze(1)), dim=1).numpy()


def unit_normals_f32(normals_f64):
    """float32(normal) / its float32 length, every operation rounded to float32, squares summed left to right."""
    with np.errstate(all="ignore"):
        d = np.asarray(normals_f64, np.float64).astype(np.float32)
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return d / np.sqrt(s)[:, None]


def quaternions_f64(normals_f64):
    """The same rotation from the same float32 unit vector, everything after it in float64: [N,4] float64."""
    with np.errstate(all="ignore"):
        u = unit_normals_f32(normals_f64).astype(np.float64)
        zero = np.zeros(len(u))
        axis = np.stack([zero * u[:, 2] - zero * u[:, 1], zero * u[:, 0] - u[:, 2], u[:, 1] - zero * u[:, 0]], 1)
        half = np.arccos(u[:, 0] + zero * u[:, 1] + zero * u[:, 2]) / 2
        return np.concatenate([np.cos(half)[:, None], axis * np.sin(half)[:, None]], 1)


# ---- the one ring ----------------------------------------------------------------------------------------------------------
def neighbor_priors(means3D_f32, nbr, eye_del, true_values=True):
    """The one-ring priors from float64(float32 means) and padded neighbour indices [P,K].  A dict:
        weight   float32 [P,K]   float32(exp(-2000 wh)) with numpy's exp, entries whose float64 value is exactly 1 set to 0
        dist     float32 [P,K]   float32(sqrt(squared distance))
        arg      float64 [P,K]   -2000 wh, the exponential's argument (wh: the squared distance, or for a neighbour in eye_del
                                 of a vertex not in it the sum of the squared (difference * 1000))
        zeroed   bool [P,K]      where the reference's `== 1` rule fired
        true_exp [P,K] objects   exp(arg) from mpmath at 60 digits (None with true_values=False)
        bad      int             neighbour indices outside [0, P) (their entries are 0 / 0)"""
    import mpmath
    x = np.asarray(means3D_f32, np.float32).astype(np.float64)
    nbr = np.asarray(nbr, np.int64)
    P, K = nbr.shape
    eye = set(int(e) for e in np.asarray(eye_del).reshape(-1).tolist())
    sq, wh = np.zeros((P, K)), np.zeros((P, K))
    ok = np.ones((P, K), bool)
    for v in range(P):
        for s in range(K):
            j = int(nbr[v, s])
            if not 0 <= j < P:
                ok[v, s] = False
                continue
            d = x[v] - x[j]
            sq[v, s] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            if j in eye and v not in eye:
                e = d * 1000
                wh[v, s] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            else:
                wh[v, s] = sq[v, s]
    arg = -2000 * wh
    with np.errstate(under="ignore"):
        w = np.exp(arg)
    zeroed = (w == 1) & ok
    w[zeroed] = 0.0
    w[~ok] = 0.0
    with np.errstate(under="ignore"):
        weight = w.astype(np.float32)
    dist = np.sqrt(sq).astype(np.float32)
    true_exp = np.empty((P, K), object)
    with mpmath.workdps(60):
        for v in range(P if true_values else 0):
            for s in range(K):
                true_exp[v, s] = mpmath.exp(mpmath.mpf(float(arg[v, s])))
    return {"weight": weight, "dist": dist, "arg": arg, "zeroed": zeroed, "true_exp": true_exp, "bad": int((~ok).sum())}


def float32_interval(true_value, ulps=1):
    """(lo, hi) float32: the values float32(d) can take for a double d within `ulps` float64 ulp of the mpmath number
    `true_value` >= 0 (the ulp of the binade holding it; 2^-1074 below the normal range)."""
    import mpmath
    with mpmath.workdps(60):
        t = mpmath.mpf(true_value)
        if t == 0:
            e = -1074
        else:
            e = max(int(mpmath.floor(mpmath.log(t, 2))) - 52, -1074)
        ulp = mpmath.ldexp(mpmath.mpf(1), e)
        # the doubles in [t - ulps*ulp, t + ulps*ulp]: round the ends inward
        lo, hi = t - ulps * ulp, t + ulps * ulp
        dlo = float(lo)
        if mpmath.mpf(dlo) < lo:
            dlo = float(np.nextafter(dlo, np.inf))
        dhi = float(hi)
        if mpmath.mpf(dhi) > hi:
            dhi = float(np.nextafter(dhi, -np.inf))
        dlo = max(dlo, 0.0)
    with np.errstate(under="ignore"):
        return np.float32(dlo), np.float32(dhi)


# ---- region weights --------------------------------------------------------------------------------------------------------
def region_weights(w_f32, masks, factors_f32):
    """A copy of w [P,K] float32 in which, for every mask in list order, the mask's set of rows is multiplied once by that
    mask's float32 factor, each product rounded to float32."""
    out = np.array(w_f32, np.float32, copy=True)
    for rows, f in zip(masks, np.asarray(factors_f32, np.float32).reshape(-1)):
        rows = sorted(set(int(r) for r in np.asarray(rows).reshape(-1).tolist()))
        if rows:
            with np.errstate(under="ignore"):
                out[rows] = out[rows] * np.float32(f)
    return out


# ---- flatten edges ---------------------------------------------------------------------------------------------------------
def candidate_edges(faces):
    """The constructors' candidate edges: the ascending pairs (corner 0, corner 1) of every face, then (corner 1, corner 2) of
    every face, made unique through a CPython set of tuples and listed in the set's order."""
    f = np.asarray(faces)
    pairs = np.sort(np.concatenate((f[:, 0:2], f[:, 1:3]), axis=0))
    seen = set()
    for p in pairs:
        seen.add(tuple(p))
    return [(int(a), int(b)) for a, b in seen]


def flatten_edges(faces, candidates=None):
    """(v0s, v1s, v2s, v3s, raises) of a flatten term, int64.  In candidate order: an edge held by more than two faces is
    skipped before anything else looks at it; every other edge takes the next rank; of its faces, in ascending id, the first
    gives v2 and the second v3, each the first corner that is neither end.  The edges of exactly two faces are the output, with
    v2 and v3 their own and v0s / v1s read from the CANDIDATE list at the edge's rank.  raises: a ranked edge meets a face
    without such a corner (the reference fails with an IndexError)."""
    f = np.asarray(faces, np.int64)
    cand = candidate_edges(f) if candidates is None else [(int(a), int(b)) for a, b in np.asarray(candidates).tolist()]
    holders = {}
    for k, face in enumerate(f.tolist()):
        for x in face:
            holders.setdefault(x, set()).add(k)
    third_first, third_second, two_face_ranks, rank, raises = [], [], [], 0, False
    for a, b in cand:
        shared = sorted(holders[a] & holders[b])
        if len(shared) > 2:
            continue
        if len(shared) == 2:
            two_face_ranks.append(rank)
        for n, k in enumerate(shared):
            rest = [x for x in f[k].tolist() if x != a and x != b]
            if not rest:
                raises = True
                rest = [-1]
            (third_first if n == 0 else third_second).append(rest[0])
        rank += 1
    c = np.asarray(cand, np.int64).reshape(-1, 2)
    r = np.asarray(two_face_ranks, np.int64)
    return c[r, 0], c[r, 1], np.asarray(third_first, np.int64)[r], np.asarray(third_second, np.int64), raises


# ---- FlattenLoss_v2's mask -------------------------------------------------------------------------------------------------
def neighbor_mask(neighbor_num, K):
    """int64 [P,K,3]: 1 in the first neighbor_num[p] slots of row p, on all three channels."""
    n = np.asarray(neighbor_num, np.int64)
    m = (np.arange(K)[None, :] < n[:, None]).astype(np.int64)
    return np.repeat(m[:, :, None], 3, axis=2)
