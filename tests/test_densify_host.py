"""CPU: the host side of the dense-mesh build (topo4d_amd/densify.py) against golden G13 - the reference's own
get_face_faces / build_dense_vertices_2 / triangulate_faces on seeded synthetic meshes (tools/gen_golden_dense.py) - and the
argument checks of the new C entry points, which run without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G13 = os.path.join(ROOT, "tests", "golden", "g13_dense_build.npz")
CASES = ("d1", "d2", "d3", "d7", "d30")
KEYS = ("dense_quad_faces", "dense_vertex_father", "dense_vertex_weight", "dense_faces", "dense_uv_faces", "dense_vertex", "dense_uvs")


def golden_case(g, name):
    """The reference's inputs of one G13 case: means3D, faces_ori / uv_faces_ori (lists of lists), uvs_ori, uv_counts,
    face_masks, density."""
    lens = g[f"{name}/face_lens"].astype(np.int64)
    st = np.concatenate([[0], np.cumsum(lens)[:-1]])
    fl, ufl = g[f"{name}/faces"], g[f"{name}/uv_faces"]
    faces = [fl[s:s + n].tolist() for s, n in zip(st, lens)]
    uv_faces = [ufl[s:s + n].tolist() for s, n in zip(st, lens)]
    return (g[f"{name}/means3D"], faces, uv_faces, g[f"{name}/uvs_ori"], g[f"{name}/uv_counts"].astype(np.int64),
            g[f"{name}/face_masks"], int(g[f"{name}/density"]))


def assert_mesh_equal(out, g, name):
    for k in KEYS:
        ref = g[f"{name}/{k}"]
        got = np.asarray(out[k])
        if k == "dense_vertex":
            ref = ref.astype(np.float64)                                 # stored as float32: the reference's values are float32
        assert got.shape == ref.shape, (name, k, got.shape, ref.shape)
        assert np.array_equal(got, ref), (name, k, np.argwhere(got != ref)[:5])
        assert got.dtype.kind == ref.dtype.kind, (name, k, got.dtype, ref.dtype)


@pytest.fixture(scope="module")
def g13():
    return np.load(G13)


@pytest.mark.parametrize("name", CASES)
def test_numpy_yardstick_is_the_reference_bit_for_bit(g13, name):
    from topo4d_amd import densify
    assert_mesh_equal(densify.build_dense_mesh_numpy(*golden_case(g13, name)), g13, name)


@pytest.mark.parametrize("name", CASES)
def test_plan_counts_offsets_and_owners(g13, name):
    from topo4d_amd import densify
    P, faces, uv_faces, uvs, uv_counts, masks, d = golden_case(g13, name)
    plan = densify.plan_dense_mesh(faces, uv_faces, uv_counts, masks, d, P.shape[0], uvs.shape[0])
    assert np.array_equal(plan["quad_faces"], g13[f"{name}/dense_quad_faces"])
    nb = np.array([bin(int(f)).count("1") for f in plan["flags"]])
    assert np.array_equal(plan["count"], (d + 2) ** 2 - 4 - d * nb)
    assert np.array_equal(plan["offset"], np.concatenate([[0], np.cumsum(plan["count"])[:-1]]))
    assert plan["n_points"] == g13[f"{name}/dense_vertex_father"].shape[0]
    # the father column is the processing order of the quads, each quad's points contiguous from its offset
    father = g13[f"{name}/dense_vertex_father"][:, 0]
    assert np.array_equal(father, np.repeat(np.arange(plan["quad_faces"].shape[0]), plan["count"]))
    # every borrowed slot names an earlier quad holding the same vertex pair, which does not borrow it itself
    src = plan["src"]
    fq = plan["quad_faces"]
    ends = [(0, 3), (0, 1), (1, 2), (3, 2)]
    for q, s in zip(*np.nonzero(src >= 0)):
        oq, os_ = divmod(int(src[q, s]), 4)
        assert oq < q and src[oq, os_] == -1
        assert sorted(fq[q, list(ends[s])]) == sorted(fq[oq, list(ends[os_])])


def test_golden_covers_every_case_the_issue_names(g13):
    from topo4d_amd import densify
    P, faces, uv_faces, uvs, uv_counts, masks, d = golden_case(g13, "d3")
    plan = densify.plan_dense_mesh(faces, uv_faces, uv_counts, masks, d, P.shape[0], uvs.shape[0])
    fq, src = plan["quad_faces"], plan["src"]
    ends = np.array([(0, 3), (0, 1), (1, 2), (3, 2)])
    a, b = fq[:, ends[:, 0]], fq[:, ends[:, 1]]
    borrowed = src >= 0
    assert (a[borrowed] > b[borrowed]).any() and (a[borrowed] < b[borrowed]).any()     # both orientations borrowed
    assert (uv_counts == 2).any() and len(plan["tri_faces"]) > 0 and len(plan["rest_faces"]) > 0
    owners, n = np.unique(src[borrowed], return_counts=True)
    assert (n >= 2).any()                                                               # an edge shared by three quads
    seam = (uv_counts[a] == 2) & (uv_counts[b] == 2)
    half = (uv_counts[a] == 2) ^ (uv_counts[b] == 2)
    assert (seam & ~borrowed).any() and (half & borrowed).any()                         # seam edges duplicated, half-seam shared
    assert (uv_counts[fq] == 2).all(axis=1).any()                                       # an all-seam quad


def test_face_split_uses_any_vertex_in_face_masks():
    from topo4d_amd import densify
    faces = [[0, 1, 2, 3], [4, 5, 6, 7], [0, 4, 8], [8, 9, 10, 11], [1, 9, 12, 13]]
    plan = densify.plan_dense_mesh(faces, faces, np.ones(14, np.int64), np.array([9, 3]), 2, 14, 14)
    assert plan["quad_faces"].tolist() == [[0, 1, 2, 3], [8, 9, 10, 11], [1, 9, 12, 13]]
    assert plan["quad_faces_idx"].tolist() == [0, 3, 4]
    assert plan["rest_faces"].tolist() == [[4, 5, 6, 7]] and plan["tri_faces"].tolist() == [[0, 4, 8]]
    boolean = np.zeros(14, bool)
    boolean[[9, 3]] = True
    assert np.array_equal(densify.plan_dense_mesh(faces, faces, np.ones(14), boolean, 2, 14, 14)["quad_faces"], plan["quad_faces"])
    with pytest.raises(ValueError):
        densify.plan_dense_mesh(faces, faces, np.ones(14), [9], 0, 14, 14)
    with pytest.raises(ValueError):
        densify.plan_dense_mesh(faces, faces, np.ones(14), [9], 2, 12, 14)            # vertex index out of range


@pytest.mark.parametrize("key,k", [("points_k1", 1), ("points_k4", 4), ("points_k8", 8)])
def test_numpy_knn_matches_the_stored_brute_force(g13, key, k):
    from topo4d_amd import densify
    got = densify.knn_mean_sq_dist_numpy(g13["knn/points"], k, chunk=64)
    assert np.array_equal(got, g13[f"knn/{key}"])


def test_numpy_knn_on_the_dense_and_coarse_points(g13):
    from topo4d_amd import densify
    assert np.array_equal(densify.knn_mean_sq_dist_numpy(g13["d3/dense_vertex"], 4), g13["knn/dense_k4"])
    assert np.array_equal(densify.knn_mean_sq_dist_numpy(g13["d3/means3D"], 1), g13["knn/coarse_k1"])
    pts = g13["knn/points"]
    assert densify.knn_mean_sq_dist_numpy(pts, 1)[0] == 0.0                             # row 0 has an exact duplicate (row 10)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from topo4d_amd import _lib
    lib = _lib.load()
    m = _lib.T4DDenseMesh()
    assert lib.t4d_dense_scratch_bytes(C.byref(m)) == 0                                  # density 0
    assert b"t4d_dense_scratch_bytes" in lib.t4d_last_error()
    m.density, m.n_vert, m.n_uv, m.n_quads, m.n_points = 2, 4, 4, 1, 12
    m.n_faces = 2 * 9
    assert lib.t4d_dense_scratch_bytes(C.byref(m)) == 0                                  # NULL pointers
    assert lib.t4d_dense_build(C.byref(m), None, 256, None) == _lib.T4D_ERR_ARG
    assert lib.t4d_dense_build(None, None, 0, None) == _lib.T4D_ERR_ARG
    dummy = C.c_void_p(16)                                                               # never dereferenced: validation fails first
    for name in ("vertices", "uvs", "quads", "uv_quads", "plan", "src", "dense_vertex", "vertex_father", "vertex_weight",
                 "dense_uvs", "faces", "uv_faces"):
        setattr(m, name, dummy)
    assert lib.t4d_dense_scratch_bytes(C.byref(m)) == 256
    m.n_faces = 17                                                                       # inconsistent face count
    assert lib.t4d_dense_scratch_bytes(C.byref(m)) == 0
    m.n_faces, m.n_points = 18, 13                                                       # more points than (d+2)^2 - 4
    assert lib.t4d_dense_build(C.byref(m), dummy, 256, None) == _lib.T4D_ERR_ARG
    m.n_points = 12
    assert lib.t4d_dense_build(C.byref(m), dummy, 255, None) == _lib.T4D_ERR_STATE_SIZE
    assert lib.t4d_knn_scratch_bytes(10, 0) == 0 and lib.t4d_knn_scratch_bytes(4, 4) == 0
    assert lib.t4d_knn_scratch_bytes(10, _lib.T4D_KNN_MAX_K + 1) == 0
    assert lib.t4d_knn_scratch_bytes(1000, 4) > 1000 * 24
    assert lib.t4d_knn_mean_sq_dist(None, 10, 4, dummy, None, dummy, 1 << 20, None) == _lib.T4D_ERR_ARG
    assert lib.t4d_knn_mean_sq_dist(dummy, 10, 4, dummy, None, dummy, 16, None) == _lib.T4D_ERR_STATE_SIZE
