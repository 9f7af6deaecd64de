"""CPU: the yardstick of tests/test_gpu_setup_cases.py is anchored here.  tests/setup_ref.py, run on golden G15's own inputs (the
OBJ, trans_g, the JPEG as PIL decodes it, facial_regions), must reproduce what the reference produced for G15; and every designed
case of tests/setup_cases.py must really contain the edge it is named for, so a case that stops covering it fails without a GPU."""
import hashlib
import io

import numpy as np
import pytest

from tests import objexport_ref, setup_cases as cases, setup_ref
from tests.test_setup_host import EDGE_TERMS, golden, write_scene
from topo4d_amd import coarse


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- G15 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.fixture(scope="module")
def scene(g, tmp_path_factory):
    mesh = coarse.read_obj(write_scene(tmp_path_factory.mktemp("g15ref"), g))
    inv = np.linalg.inv(g["trans_g"])
    vertices = mesh.vertices @ inv[:3, :3].T
    vertices = vertices + inv[:3, 3]
    return mesh, vertices


@pytest.fixture(scope="module")
def ring(g, scene):
    mesh, vertices = scene
    means = vertices.astype(np.float32)
    assert sha(means) == str(g["means3D_sha256"])
    _, padded = coarse.one_ring(mesh.faces_ori, len(vertices))
    return setup_ref.neighbor_priors(means, padded, g["facial_regions"]["eye_del_masks"], true_values=False)


def test_colors_reproduce_g15(g, scene):
    from PIL import Image
    mesh, vertices = scene
    img = np.asarray(Image.open(io.BytesIO(g["jpeg"])))
    colors, rgb, n_raise, first, unref = setup_ref.vertex_colors(img, mesh.corner_uvs, mesh.faces, len(vertices))
    assert (n_raise, first, unref) == (0, None, 0)
    assert np.array_equal(colors, g["colors"].astype(np.int32))
    assert sha(rgb) == str(g["rgb_colors_sha256"])


def test_one_ring_reproduces_g15(g, ring):
    assert ring["bad"] == 0
    assert sha(ring["dist"]) == str(g["neighbor_dist_sha256"])
    # the reference used numpy's exp and so does the restatement: with this numpy build the digest itself reproduces (were it
    # not to, the sampled rows below are what the issue falls back to)
    assert np.array_equal(ring["weight"][g["sample_rows"]], g["neighbor_weight_sample"])
    assert sha(ring["weight"]) == str(g["neighbor_weight_sha256"])
    assert ring["zeroed"].any()


def test_region_weights_reproduce_g15(g, ring):
    fr, P = g["facial_regions"], ring["weight"].shape[0]
    for name, (key, blocks) in coarse.REGION_WEIGHT_BLOCKS.items():
        lw = coarse.LOSSES_WEIGHTS[key]
        masks = [coarse._mask_rows(fr, m, P) for m, _ in blocks]
        factors = np.array([c / lw for _, c in blocks], np.float32)
        assert sha(setup_ref.region_weights(ring["weight"], masks, factors)) == str(g[f"{name}_sha256"]), name


def test_flatten_edges_reproduce_g15(g):
    fr = g["facial_regions"]
    for t in EDGE_TERMS:
        *quad, raises = setup_ref.flatten_edges(fr[coarse.FLAT_EDGE_TERMS[t]])
        assert not raises
        for s, got in zip(("v0s", "v1s", "v2s", "v3s"), quad):
            assert np.array_equal(got, g["edges"][t][s]), (t, s)


def test_quaternions_reproduce_g15(g, scene):
    mesh, vertices = scene
    normals = objexport_ref.trimesh_vertex_normals(vertices, mesh.faces)
    rows, ref = g["unnorm_rotations_rows"], g["unnorm_rotations_sample"]
    tol = np.maximum(1e-6, 2 * np.spacing(np.abs(ref).astype(np.float32)))
    q = setup_ref.quaternions_torch(normals)[rows]
    assert np.all(np.abs(q - ref) <= tol), float(np.abs(q - ref).max())
    q64 = setup_ref.quaternions_f64(normals)[rows]
    assert np.all(np.abs(q64 - ref) <= tol), float(np.abs(q64 - ref).max())


def test_csr_and_mask_restatements_on_g15(g, scene):
    mesh, vertices = scene
    off, ent, bad, unref = setup_ref.vertex_corner_csr(mesh.faces, len(vertices))
    assert (bad, unref) == (0, 0) and off[-1] == mesh.faces.size
    flat = mesh.faces.reshape(-1)
    for v in (0, 1, 4000, len(vertices) - 1):
        assert ent[off[v]:off[v + 1]].tolist() == np.nonzero(flat == v)[0].tolist()
    K = int(g["region_mask_K"])
    m = setup_ref.neighbor_mask(g["neighbor_num"], K)
    assert m.shape == (len(vertices), K, 3) and m.sum() == 3 * int(g["neighbor_num"].sum())


# ---- the designed cases hold what they claim ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_vert", cases.CSR_SIZES)
def test_csr_cases(n_vert):
    faces, unref = cases.csr_case(n_vert)
    off, ent, bad, n_unref = setup_ref.vertex_corner_csr(faces, n_vert)
    assert bad == 0 and n_unref == len(unref) and (0 <= faces).all() and (faces < n_vert).all()
    valence = np.diff(off)
    assert np.all(valence[unref] == 0) and valence.max() >= (cases.CSR_HUB_VALENCE if n_vert > 1 else 15)
    per_face = [len(set(f)) for f in faces.tolist()]
    assert 1 in per_face and (n_vert == 1 or 2 in per_face)
    if n_vert > 1:
        assert unref.min() == 0 and unref.max() == n_vert - 1 and n_vert // 2 in unref
    for n_bad in (1, 5):
        fb, _ = cases.csr_case(n_vert, n_bad)
        assert setup_ref.vertex_corner_csr(fb, n_vert)[2] == n_bad


@pytest.mark.parametrize("name", list(cases.TEXTURES))
def test_color_cases(name):
    img, uv, faces, n_vert = cases.color_case(name)
    W, H, ch = cases.TEXTURES[name]
    assert img.shape == (H, W, ch) and len(uv) == faces.size and len(uv) < 4000
    colors, rgb, n_raise, first, unref = setup_ref.vertex_colors(img, uv, faces, n_vert)
    assert (n_raise, first, unref) == (0, None, 0)
    assert np.bincount(faces.reshape(-1)).max() >= cases.COLOR_HUB_CORNERS
    u, v = uv[:, 0], uv[:, 1]
    um = np.array([float(a) % 1 for a in u])
    vm = np.array([float(a) % 1 for a in v])
    x, y = um * W, (1 - vm) * H
    assert (np.floor(x) == W - 1).any() and (np.floor(y) == H - 1).any()         # a corner on the last column / row
    assert ((u < 0) & (u == np.round(u))).any() and (u == 1e-300).any()
    assert any(a == 0 and np.signbit(a) for a in u)                               # -0.0
    assert ((u < -2) | (v < -2)).any() and ((u > 2) | (v > 2)).any()
    if W > 1 and H > 1:
        last_col = (np.floor(x) == W - 1) & (x != np.floor(x)) & (np.floor(y) < H - 1)
        assert last_col.any()
        c = int(np.nonzero(last_col)[0][0])
        assert setup_ref.corner_color(img, u[c], v[c]) == (0, 0, 0)               # the reference's quirk: x2 == x1
        assert ((x == np.floor(x)) & (x > 0)).any() and ((x - np.floor(x)) == 0.5).any()   # texel corners and centres
    if name == "37x29":
        ups = cases.rounds_up_to_integer(W)
        assert ups and all(a in u for a, _ in ups)
        assert (colors > 0).any() and len(np.unique(colors)) > 20


def test_color_refusal_case():
    img, uv, faces, n_vert = cases.color_refusal_case()
    *_, n_raise, first, _ = setup_ref.vertex_colors(img, uv, faces, n_vert)
    idx = sorted(cases.COLOR_REFUSALS)
    assert (n_raise, first) == (4, idx[0]) and idx[0] >= 256 and min(np.diff(idx)) > 256
    for c in idx:
        *_, n_raise, first, _ = setup_ref.vertex_colors(*_one_refusal(c))
        assert (n_raise, first) == (1, c)


def _one_refusal(c):
    img, uv, faces, n_vert = cases.color_refusal_case((c,))
    return img, uv, faces, n_vert


def test_quaternion_cases():
    normals, groups = cases.quaternion_normals()
    assert len(normals) != 3                                         # torch.cross without dim would pick axis 0
    u = setup_ref.unit_normals_f32(normals)
    one = np.float32(1)
    eps = np.float32(cases.F32_EPS_BELOW_ONE)
    t = np.abs(u[groups["tilted"], 0])
    assert sorted(set(t.tolist())) == [float(one - 2 * eps), float(one - eps)]
    assert np.array_equal(np.abs(u[groups["axes"]]).max(1), np.ones(6, np.float32))
    assert np.isnan(u[groups["x1e-30"]]).all() or np.isinf(u[groups["x1e-30"]]).any()      # squares underflow: division by 0
    assert np.all(u[groups["x1e30"]] == 0)                                                  # squares overflow: division by inf
    assert np.isnan(u[groups["zero"]]).all() and np.isnan(u[groups["nan"]]).all()
    q32, q64 = setup_ref.quaternions_torch(normals), setup_ref.quaternions_f64(normals)
    assert np.array_equal(np.isnan(q32), np.isnan(q64))
    ok = ~np.isnan(q32)
    assert np.abs(q32[ok] - q64[ok]).max() <= 1e-6
    for name in ("plain", "axes", "tilted", "x1e-3", "x1e3"):
        assert np.isfinite(q32[groups[name]]).all(), name


@pytest.mark.parametrize("P,K", cases.ONE_RING_SHAPES)
def test_one_ring_cases(P, K):
    import mpmath
    x, nbr, eye = cases.one_ring_case(P, K)
    assert x.dtype == np.float32 and nbr.shape == (P, K)
    r = setup_ref.neighbor_priors(x, nbr, eye)
    assert r["bad"] == 0
    assert (nbr == np.arange(P)[:, None]).any()                      # padded slots
    t = -r["arg"]                                                    # 2000 wh
    if P == 1:
        assert r["zeroed"].all() and not r["weight"].any() and not r["dist"].any()
        return
    # both sides of the threshold, nothing between but the issue's own pair (3.6 * 2^-53: still no faithful exp gives 1)
    between = (t > cases.EXP_ONE_BELOW) & (t < cases.EXP_ONE_ABOVE)
    assert np.argwhere(between).tolist() == [[cases.ISSUE_PAIR, 0]]
    wh = t[cases.ISSUE_PAIR, 0] / 2000
    assert abs(wh - 2.0e-19) < 1e-21 and t[cases.ISSUE_PAIR, 0] > 3 * 2.0 ** -53
    assert np.exp(-2000 * wh) == 0.9999999999999996
    for v in cases.BELOW_ONE:
        assert 0 < t[v, 0] <= cases.EXP_ONE_BELOW and r["zeroed"][v, 0] and r["dist"][v, 0] > 0
    for v in cases.ABOVE_ONE:
        assert (v == cases.ISSUE_PAIR or t[v, 0] >= cases.EXP_ONE_ABOVE) and not r["zeroed"][v, 0]
    assert np.array_equal(r["zeroed"], t <= cases.EXP_ONE_BELOW)
    # weights kept at exactly 1.0f: a comparison after the float32 cast would zero them
    kept_one = (r["weight"] == np.float32(1)) & ~r["zeroed"]
    assert kept_one[cases.ISSUE_PAIR, 0] and kept_one.sum() >= 3
    # coincident vertices on real slots, and far pairs: a float32 denormal, a float64 denormal, an exact 0
    assert t[10, 0] == 0 and nbr[10, 0] == 11 and r["weight"][10, 0] == 0 and r["dist"][10, 0] == 0
    assert 0 < r["weight"][32, 0] < np.finfo(np.float32).tiny
    assert 0 < np.exp(r["arg"][34, 0]) < np.finfo(np.float64).tiny and r["weight"][34, 0] == 0
    assert np.exp(r["arg"][30, 0]) == 0 and r["dist"][30, 0] > 10
    # the four eye memberships over one geometry: only (v out, j in) takes the x1000 rule
    w = {v: r["weight"][v, 0] for v in cases.EYE_COMBOS}
    d = {v: r["dist"][v, 0] for v in cases.EYE_COMBOS}
    ins = set(eye)
    assert [(v in ins, j in ins) for v, j in cases.EYE_COMBOS.items()] == [(True, True), (True, False), (False, True), (False, False)]
    assert len(set(d.values())) == 1 and w[40] == w[41] == w[43] and 0 < w[42] < 0.5 * w[40]
    # sum((d * 1000)^2) against sum(d^2) * 1e6: the float32 results differ, and the true value leaves no doubt
    assert len(cases.EYE_LAST_BIT) >= 4
    for i in range(len(cases.EYE_LAST_BIT)):
        v, j = cases.EYE_ORIGINS + i, cases.EYE_TARGETS + i
        dd = x[v].astype(np.float64) - x[j].astype(np.float64)
        other = float(np.float32(np.exp(-2000 * (((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]) * 1e6))))
        lo, hi = setup_ref.float32_interval(r["true_exp"][v, 0], ulps=3)
        assert lo == hi == r["weight"][v, 0] and other != float(lo)
        with mpmath.workdps(60):
            t_other = mpmath.exp(mpmath.mpf(float(-2000 * (((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]) * 1e6))))
        lo2, hi2 = setup_ref.float32_interval(t_other, ulps=3)
        assert lo2 == hi2 == np.float32(other)
    if K == 1:
        assert nbr[255, 0] == 256 and nbr[256, 0] == 255             # a coincident pair across the first workgroup's end
    for n_bad in (1, 3):
        xb, nb, eb = cases.one_ring_refusal_case(n_bad)
        assert int(((nb < 0) | (nb >= 257)).sum()) == n_bad


def test_float32_interval():
    import mpmath
    with mpmath.workdps(60):
        assert setup_ref.float32_interval(mpmath.mpf(0.5)) == (np.float32(0.5), np.float32(0.5))
        lo, hi = setup_ref.float32_interval(mpmath.mpf(1) - mpmath.mpf(2) ** -25)          # a float32 midpoint below 1
        assert (lo, hi) == (np.float32(1) - np.float32(2.0 ** -24), np.float32(1))
        assert setup_ref.float32_interval(mpmath.mpf(0)) == (np.float32(0), np.float32(0))
        assert setup_ref.float32_interval(mpmath.exp(-2000)) == (np.float32(0), np.float32(0))


def test_region_cases():
    w = cases.region_input()
    P, K = w.shape
    assert P * K > 256 > (P - 1) * K
    rc = cases.region_cases()
    assert sorted(len(m) for m, _ in rc.values()) == [0, 1, 11, 11, 11, 32]
    m, f = rc["eleven_with_empty"]
    assert m[0] == [] and m[5] == [] and m[10] == [] and any(m[1:5]) and any(m[6:10])
    z = [i for i, v in enumerate(f.tolist()) if v == 0.0]
    assert z and any(f[i] != 0 for i in range(z[0])) and any(f[i] != 0 for i in range(z[-1] + 1, 11))
    assert not any(rows for rows in rc["eleven_all_empty"][0])
    assert len(rc["one_duplicated_rows"][0][0]) > len(set(rc["one_duplicated_rows"][0][0]))
    for name in ("eleven_row_in_all", "thirty_two"):
        m, f = rc[name]
        assert all(cases.EVERY_MASK_ROW in rows for rows in m) and (f != 0).all()        # a row that is a member of all masks
        seq = setup_ref.region_weights(w, m, f)
        # one pre-multiplied product per row is NOT what the reference does: it must differ somewhere in float32
        pre = w.copy()
        for p in range(P):
            prod = np.float32(1)
            for rows, c in zip(m, f):
                if p in rows:
                    prod = np.float32(prod * c)
            pre[p] = w[p] * prod
        assert (seq != pre).any(), name
        assert (seq[cases.EVERY_MASK_ROW] != 0).any()
    m, _ = rc["thirty_two"]
    assert [i for i, rows in enumerate(m) if 6 in rows] == [31] and [i for i, rows in enumerate(m) if 7 in rows] == [0]
    # a duplicated row is multiplied once
    one = setup_ref.region_weights(w, [[4, 4]], [0.5])
    assert np.array_equal(one[4], w[4] * np.float32(0.5))


@pytest.mark.parametrize("n_edges", cases.FLATTEN_SIZES)
def test_flatten_cases(n_edges):
    faces = cases.flatten_case(n_edges)
    cand = setup_ref.candidate_edges(faces)
    assert np.array_equal(np.asarray(cand), coarse.flatten_candidate_edges(faces))
    E = len(cand)
    assert E == n_edges or (n_edges == 1500 and 1500 <= E <= 1502)
    holders = {}
    for k, f in enumerate(faces.tolist()):
        for a in f:
            holders.setdefault(a, set()).add(k)
    count = np.array([len(holders[a] & holders[b]) for a, b in cand])
    want = [p for p in cases.DROP_AT if p < E]
    assert all(count[p] > 2 for p in want)                           # an edge of three or four faces at each named position
    assert (count == 3).any() and (count == 4).any() and (count == 1).any() and (count == 2).any()
    for end in range(cases.TRIP, min(E, 2 * cases.TRIP + 1), cases.TRIP):   # before, at and after the first two trips' ends
        assert count[end - 1] > 2 and count[end] > 2 and (count[:end - 1] > 2).any()
        assert end + 1 >= E or (count[end + 1:] > 2).any()           # (257 candidates end at position 256)
    v0, v1, v2, v3, raises = setup_ref.flatten_edges(faces)
    assert not raises and len(v0) == int((count == 2).sum()) == len(v3)
    # the rank shift is live: some output row's (v0, v1) is NOT the edge its v2 / v3 come from, and in the multi-trip cases
    # the shift at the last trip's first edge is larger than anywhere in the first trip
    own = np.asarray(cand)[count == 2]
    assert (own[:, 0] != v0).any() or (own[:, 1] != v1).any()
    if E > cases.TRIP:
        dropped_before = np.cumsum(count > 2)
        assert dropped_before[-1] > dropped_before[cases.TRIP - 1] > 0
    # faces listing a vertex twice that still have a third corner: the first face, and a late one; their edges are dropped
    twice = [k for k, f in enumerate(faces.tolist()) if len(set(f)) == 2]
    assert twice[0] == 0 and len(twice) == 2
    for k in twice:
        a, b = sorted(set(faces[k].tolist()))
        assert len(holders[a] & holders[b]) > 2


def test_flatten_fully_degenerate_case_raises_in_the_reference():
    assert setup_ref.flatten_edges(cases.FULLY_DEGENERATE)[4]


def test_neighbor_mask_cases():
    for nnum, K in cases.neighbor_mask_cases():
        assert set(nnum.tolist()) == set(range(K + 1))
        assert len(nnum) * K * 3 > 256 > (len(nnum) - 1) * K * 3 or len(nnum) * K * 3 > 256
        m = setup_ref.neighbor_mask(nnum, K)
        assert m.dtype == np.int64 and m.sum() == 3 * nnum.sum()
