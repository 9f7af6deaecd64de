"""CPU: topo4d_amd.coarse's host pieces against golden G15 (tools/gen_golden_setup.py: the reference's own initialize_params and
initialize_losses), the OBJ reader's refusals, and the argument checks of the t4d_setup_* entry points.  No device call is made."""
import ctypes as C
import lzma
import os

import numpy as np
import pytest

from topo4d_amd import coarse

HERE = os.path.dirname(os.path.abspath(__file__))
G15 = os.path.join(HERE, "golden", "g15_coarse_setup.npz")
EDGE_TERMS = ("flat", "flat_lip_bottom", "flat_lip", "flat_mouth", "flat_lid_top", "flat_lid_bottom")
REGION_TERMS = ("flat_eye", "flat_lip_socket", "flat_face_bottom")


def face_adjacency(faces, n):
    """Per vertex the sorted other corners of the faces holding it (G15 stores v1s..v3s as slots of v0's list)."""
    adj = [set() for _ in range(n)]
    for f in np.asarray(faces).tolist():
        for a in f:
            adj[a].update(b for b in f if b != a)
    return [sorted(s) for s in adj]


def golden():
    """G15 decoded: the scene's files (bytes), facial_regions as the pickle holds it (region_masks a dict; static_masks a list),
    the delta-coded index arrays, and everything else as stored (digests under *_sha256)."""
    z = dict(np.load(G15))
    g = {k: z[k] for k in z if not k.startswith("fr_") and not k.endswith(("_v0_delta", "_slots", "_region"))}
    for k in ("mtl", "jpeg", "png_rgba"):
        g[k] = z[k].tobytes()
    g["obj"] = lzma.decompress(z["obj_xz"].tobytes())
    lists, wide = set(z["fr_list_keys"].tolist()), set(z["fr_int64_keys"].tolist())
    fr = {"region_masks": {}}
    for k in z:
        if k.startswith("fr_region_masks__"):
            fr["region_masks"][k[len("fr_region_masks__"):]] = z[k]
        elif k.startswith("fr_") and k not in ("fr_list_keys", "fr_int64_keys"):
            a = z[k].astype(np.int64) if k[3:] in wide else z[k]
            fr[k[3:]] = a.tolist() if k[3:] in lists else a
    g["facial_regions"] = fr
    P = z["neighbor_indices_delta"].shape[0]
    g["neighbor_indices"] = z["neighbor_indices_delta"].astype(np.int64) + np.arange(P)[:, None]
    g["edges"] = {}
    for t in EDGE_TERMS:
        v0 = np.cumsum(z[f"{t}_v0_delta"].astype(np.int64))
        adj = face_adjacency(fr[coarse.FLAT_EDGE_TERMS[t]], P)
        slots = z[f"{t}_slots"].astype(np.int64)
        g["edges"][t] = {"v0s": v0}
        for j, s in enumerate(("v1s", "v2s", "v3s")):
            g["edges"][t][s] = np.array([adj[a][k] for a, k in zip(v0.tolist(), slots[j].tolist())], np.int64)
    g["region"] = {t: z[f"{t}_region"].astype(np.int64) for t in REGION_TERMS}
    g["losses_weights"] = dict(zip(z["losses_weights_names"].tolist(), z["losses_weights"].tolist()))
    return g


def write_scene(tmp_path, g, texture="jpeg"):
    d = tmp_path / "seq"
    d.mkdir(exist_ok=True)
    (d / "face_v5.obj").write_bytes(g["obj"])
    (d / "face.mtl").write_bytes(g["mtl"])
    (d / "texture.jpg").write_bytes(g[texture])
    return str(d / "face_v5.obj")


@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.fixture(scope="module")
def mesh(g, tmp_path_factory):
    return coarse.read_obj(write_scene(tmp_path_factory.mktemp("g15"), g))


# ---- read_obj ----------------------------------------------------------------------------------------------------------
def test_read_obj_matches_the_scene(g, mesh):
    P = g["neighbor_indices"].shape[0]
    assert mesh.vertices.dtype == np.float64 and mesh.vertices.shape == (P, 3)
    assert mesh.tex_coords.dtype == np.float64 and mesh.tex_coords.shape[1] == 2
    assert len(mesh.faces_ori) == len(mesh.uv_faces_ori)
    assert {len(f) for f in mesh.faces_ori} == {3, 4}
    tri = coarse.triangulate_faces(mesh.faces_ori)
    assert np.array_equal(mesh.faces, np.asarray(tri))
    assert np.array_equal(mesh.uv_faces, np.asarray(coarse.triangulate_faces(mesh.uv_faces_ori)))
    assert np.array_equal(mesh.corner_uvs, mesh.tex_coords[mesh.uv_faces.reshape(-1)])
    assert mesh.texture.endswith("texture.jpg") and os.path.exists(mesh.texture)
    # the one-ring of the stored faces is the reference's
    ori, padded = coarse.one_ring(mesh.faces_ori, P)
    assert np.array_equal(padded, g["neighbor_indices"])
    # the region masks the reference built from that one-ring: neighbor_num, and the reference's set order
    assert np.array_equal(np.array([len(l) for l in ori]), g["neighbor_num"])


def test_read_obj_uvs_and_quads(mesh):
    # quads fan as (0,1,2), (0,2,3), and both halves keep their corners' UVs
    k = next(i for i, f in enumerate(mesh.faces_ori) if len(f) == 4)
    t = sum(2 if len(f) == 4 else 1 for f in mesh.faces_ori[:k])
    q, uq = mesh.faces_ori[k], mesh.uv_faces_ori[k]
    assert mesh.faces[t].tolist() == [q[0], q[1], q[2]] and mesh.faces[t + 1].tolist() == [q[0], q[2], q[3]]
    assert mesh.uv_faces[t + 1].tolist() == [uq[0], uq[2], uq[3]]
    # the scene has UVs below 0 and at or above 1 (the `% 1` path)
    assert (mesh.tex_coords < 0).any() and (mesh.tex_coords >= 1).any()


def test_vertex_uvs_set_order(g, mesh):
    uvs = coarse.vertex_uvs(mesh)
    assert np.array_equal(np.array([len(x) for x in uvs]), g["uv_counts"])
    assert {2, 3} <= set(g["uv_counts"].tolist())


def test_flatten_candidate_edges_are_the_reference_set_order(g):
    fr = g["facial_regions"]
    for t in EDGE_TERMS:
        e = coarse.flatten_candidate_edges(fr[coarse.FLAT_EDGE_TERMS[t]])
        # every stored (v0, v1) is a candidate, in the candidates' order (no term of the real topology drops an edge)
        ref = np.stack([g["edges"][t]["v0s"], g["edges"][t]["v1s"]], 1)
        pos = {tuple(r): i for i, r in enumerate(e.tolist())}
        idx = [pos[tuple(r)] for r in ref.tolist()]
        assert idx == sorted(idx), t


def test_region_mask_set_order(g, mesh):
    """region_topology's host part: the reference's list(set(...)) for the three FlattenLoss_v2 terms."""
    fr = g["facial_regions"]
    calls = {"flat_eye": (["EyeLidOuterTop", "EyeLidTop", "EyeLidBottom"], [], []),
             "flat_lip_socket": ([], fr["lip_socket_flat_masks"].tolist(), []),
             "flat_face_bottom": (["LipOuterTop", "LipOuterBottom", "Chin", "NeckFront", "LipBottom", "LipTop", "LipInnerBottom",
                                  "LipInnerTop", "EyeLidOuterBottom", "EyeLidBottom", "MouthSocket", "EyeSocket"],
                                 fr["face_flat_masks"].tolist(), fr["lip_flat_edge_masks"].tolist())}
    for t, (ml, pre, ex) in calls.items():
        rm = []
        for r in ml:
            rm += fr["region_masks"][r].tolist()
        rm += pre
        rm = list(set(list(set(rm) - set(ex))))
        assert np.array_equal(np.array(rm), g["region"][t]), t


def test_losses_weights_are_the_reference(g):
    assert coarse.LOSSES_WEIGHTS == g["losses_weights"]
    assert list(coarse.LOSSES_WEIGHTS) == list(g["losses_weights"])


# ---- refusals ----------------------------------------------------------------------------------------------------------
BASE = "mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0.1 0.1\nvt 0.9 0.1\nvt 0.9 0.9\nvt 0.1 0.9\nvn 0 0 1\n"


def _obj(tmp_path, body, name="a.obj"):
    p = tmp_path / name
    p.write_text(BASE + body)
    (tmp_path / "m.mtl").write_text("newmtl m\nmap_Kd tex.png\n")
    return str(p)


def test_read_obj_accepts_a_plain_quad(tmp_path):
    m = coarse.read_obj(_obj(tmp_path, "f 1/1/1 2/2/1 3/3/1 4/4/1\n"))
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert m.texture == os.path.join(str(tmp_path), "tex.png")


@pytest.mark.parametrize("body,what", [
    ("f 1/1 2/2 3/3 4/4\n", "not v/vt/vn"),
    ("f 1//1 2//1 3//1 4//1\n", "not v/vt/vn"),
    ("f 1 2 3 4\n", "not v/vt/vn"),
    ("f -1/1/1 2/2/1 3/3/1 4/4/1\n", "non-positive"),
    ("f 1/1/1 2/2/1 3/3/1 9/4/1\n", "names vertex"),
    ("f 1/1/1 2/2/1 3/3/1 4/9/1\n", "texture coordinate"),
    ("f 1/1/1 2/2/1 3/3/1 4/4/2\n", "names normal"),
    ("f 1/1/1 2/2/1 3/3/1 4/4/1 1/1/1\n", "5 corners"),
    ("f 1/1/1 2/2/1 3/3/1\n", "in no face"),
    ("v 0 0 0 1 1 1\nf 1/1/1 2/2/1 3/3/1 4/4/1 \n", "6 values"),
])
def test_read_obj_refuses(tmp_path, body, what):
    with pytest.raises(ValueError, match=what):
        coarse.read_obj(_obj(tmp_path, body))


# ---- the entry points' argument checks ---------------------------------------------------------------------------------
def _lib():
    from topo4d_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_setup_exports_refuse_bad_arguments():
    lib = _lib()
    dummy = C.c_void_p(16)                                         # never dereferenced: every call below is refused first
    null = None
    assert lib.t4d_setup_colors_scratch_bytes(0) == 0 and b"n_corners" in lib.t4d_last_error()
    assert lib.t4d_setup_region_scratch_bytes(0) == 0
    assert lib.t4d_setup_edges_scratch_bytes(0) == 0
    assert lib.t4d_setup_colors_scratch_bytes(10) >= 120
    assert lib.t4d_setup_edges_scratch_bytes(10) >= 120
    assert lib.t4d_setup_region_scratch_bytes(10) >= 40
    # vertex colours: NULLs, sizes, channels, scratch
    args = [dummy, 8, 8, 3, dummy, 6, dummy, dummy, 4, dummy, dummy, dummy, dummy, 1 << 20, null]
    for i in (0, 4, 6, 7, 9, 10, 11, 12):
        a = list(args)
        a[i] = null
        assert lib.t4d_setup_vertex_colors(*a) == 1, i
    for i, bad in ((1, 0), (2, -1), (3, 1), (3, 2), (5, 0), (8, 0)):
        a = list(args)
        a[i] = bad
        assert lib.t4d_setup_vertex_colors(*a) == 1, (i, bad)
    a = list(args)
    a[13] = 8
    assert lib.t4d_setup_vertex_colors(*a) == 4 and b"scratch" in lib.t4d_last_error()
    # quaternions, one-ring, neighbour mask
    assert lib.t4d_setup_quaternions(null, 4, dummy, null) == 1
    assert lib.t4d_setup_quaternions(dummy, 0, dummy, null) == 1
    ring = [dummy, 10, 4, dummy, dummy, dummy, dummy, dummy, null]
    for i in (0, 3, 4, 5, 6, 7):
        a = list(ring)
        a[i] = null
        assert lib.t4d_setup_one_ring(*a) == 1, i
    for i in (1, 2):
        a = list(ring)
        a[i] = 0
        assert lib.t4d_setup_one_ring(*a) == 1, i
    assert lib.t4d_setup_neighbor_mask(null, 4, 2, dummy, null) == 1
    assert lib.t4d_setup_neighbor_mask(dummy, 4, 0, dummy, null) == 1
    # region weights: NULLs, sizes, mask count, offsets, scratch
    off = (C.c_int32 * 3)(0, 2, 3)
    reg = [dummy, 10, 4, dummy, dummy, off, 2, dummy, dummy, dummy, 1 << 20, null]
    for i in (0, 4, 5, 7, 8, 9):
        a = list(reg)
        a[i] = null
        assert lib.t4d_setup_region_weights(*a) == 1, i
    for i, bad in ((1, 0), (2, 0), (6, -1), (6, 33)):
        a = list(reg)
        a[i] = bad
        assert lib.t4d_setup_region_weights(*a) == 1, (i, bad)
    a = list(reg)
    a[3] = null                                                   # rows missing while the masks hold 3
    assert lib.t4d_setup_region_weights(*a) == 1
    a = list(reg)
    a[5] = (C.c_int32 * 3)(0, 2, 1)                               # decreasing offsets
    assert lib.t4d_setup_region_weights(*a) == 1
    a = list(reg)
    a[10] = 4
    assert lib.t4d_setup_region_weights(*a) == 4
    # flatten edges
    fe = [dummy, 10, dummy, dummy, dummy, 5, dummy, dummy, dummy, dummy, 1 << 20, null]
    for i in (0, 2, 3, 4, 6, 7, 8, 9):
        a = list(fe)
        a[i] = null
        assert lib.t4d_setup_flatten_edges(*a) == 1, i
    for i in (1, 5):
        a = list(fe)
        a[i] = 0
        assert lib.t4d_setup_flatten_edges(*a) == 1, i
    a = list(fe)
    a[10] = 8
    assert lib.t4d_setup_flatten_edges(*a) == 4
