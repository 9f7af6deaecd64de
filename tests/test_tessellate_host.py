"""CPU: the numpy restatement of the tessellation rules (tests/tessellate_ref.py) against the properties the rules promise - the
counts, every id used, a consistent orientation, a closed mesh staying closed, the area kept - the host tables of
topo4d_amd.tessellate against the same restatement, and the argument errors that are raised before anything needs a device."""
import numpy as np
import pytest
import torch

from tests import tessellate_ref as ref
from tests.test_gpu_scanbake import sphere_obj, square
from topo4d_amd import meshrender
from topo4d_amd import tessellate as TS

LEVELS = [1, 2, 3, 5]


def single():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.25, 1.0, 0.0]])
    return meshrender.FaceObj(v, v[:, :2].copy(), [[0, 1, 2]], [[0, 1, 2]])


def octahedron():
    """closed: 6 vertices, 8 triangles, 12 edges; every face has UV vertices of its own (8 islands)"""
    v = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    uvs = np.array([[(n % 4) * 0.25 + du, (n // 4) * 0.5 + dv] for n in range(8) for du, dv in ((0.02, 0.02), (0.2, 0.02), (0.02, 0.4))])
    return meshrender.FaceObj(v, uvs, f, [[3 * n, 3 * n + 1, 3 * n + 2] for n in range(8)])


MESHES = {"single": single, "square": square, "octahedron": octahedron, "sphere": lambda: sphere_obj(6, 8)[0]}


@pytest.fixture(scope="module", params=sorted(MESHES))
def mesh(request):
    obj = MESHES[request.param]()
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    return request.param, obj, faces, uv_faces


@pytest.mark.parametrize("level", LEVELS)
def test_the_rule_keeps_its_promises(mesh, level):
    name, obj, faces, uv_faces = mesh
    N, T, n_v = level, len(faces), len(obj.vertices)
    coarse_edges, coarse_use = ref.edge_use(faces)
    E = len(coarse_edges)
    for tris, n_corner in ((faces, n_v), (uv_faces, len(obj.uvs))):
        topo = ref.Topology(tris, n_corner, N)
        n_edges = len(ref.edge_use(tris)[0])
        assert topo.n_vertices == n_corner + n_edges * (N - 1) + T * (N - 1) * (N - 2) // 2
        assert topo.faces.shape == (N * N * T, 3) and topo.faces.dtype == np.int32
        assert np.array_equal(np.unique(topo.faces), np.arange(topo.n_vertices))          # every id used (these meshes have no loose vertex)
        directed = ref.directed_edges(topo.faces)
        assert len(np.unique(directed, axis=0)) == len(directed)                        # every directed edge once
        if N == 1:
            assert np.array_equal(topo.faces, tris)
    topo = ref.Topology(faces, n_v, N)
    assert topo.n_vertices == n_v + E * (N - 1) + T * (N - 1) * (N - 2) // 2
    _, use = ref.edge_use(topo.faces)
    # a coarse edge used u times splits into N fine edges used u times; the 3 N (N - 1) / 2 edges inside a triangle are used twice
    assert sorted(use.tolist()) == sorted(np.repeat(coarse_use, N).tolist() + [2] * (T * 3 * N * (N - 1) // 2))
    if name == "octahedron":
        assert (use == 2).all()                                 # closed stays closed
    fine = ref.points(obj.vertices, topo)
    assert np.array_equal(fine[:n_v], obj.vertices)
    coarse_area = ref.area(obj.vertices, faces)
    assert abs(ref.area(fine, topo.faces) - coarse_area) <= 1e-12 * max(1.0, coarse_area)
    # owners: a corner's is the first triangle that names it, an edge vertex's the lowest triangle with its edge, and both name it
    for m in range(n_v):
        assert topo.owner[m] == np.nonzero((faces == m).any(1))[0][0]
    on_edge = np.nonzero(topo.kind == ref.EDGE)[0]
    for m in on_edge[:: max(1, len(on_edge) // 50)]:
        lo, hi = topo.abc[m, :2]
        has_edge = (faces == lo).any(1) & (faces == hi).any(1)
        assert topo.owner[m] == np.nonzero(has_edge)[0][0] and lo < hi


@pytest.mark.parametrize("level", [1, 2, 5])
def test_the_host_tables_agree_with_the_restatement(mesh, level):
    _, obj, faces, uv_faces = mesh
    for tris, n_corner in ((faces, len(obj.vertices)), (uv_faces, len(obj.uvs))):
        edges, tri_edge = TS.edge_tables(tris, n_corner, "faces")
        topo = ref.Topology(tris, n_corner, level)
        want, _ = ref.edge_use(tris)
        assert edges.dtype == np.int32 and tri_edge.dtype == np.int32 and tri_edge.shape == tris.shape
        assert np.array_equal(edges[:, :2], want) and (edges[:, 0] < edges[:, 1]).all()
        for k, (p, q) in enumerate(((0, 1), (1, 2), (2, 0))):
            assert np.array_equal(edges[tri_edge[:, k], :2], np.sort(tris[:, [p, q]], axis=1))
        for e, (lo, hi, owner) in enumerate(edges.tolist()):
            assert owner == np.nonzero((tris == lo).any(1) & (tris == hi).any(1))[0][0]
        assert TS.fine_sizes(n_corner, len(edges), len(tris), level) == (topo.n_vertices, len(topo.faces))


def test_a_flat_displacement_on_the_restatement():
    """the sampling rule on a hand-worked map: a constant code moves every vertex of the square by (code - 32768) * unit along +z,
    whatever the weights; a vertex none of whose taps counts stays; a tap of another island does not count"""
    obj = square()
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    topo = ref.Topology(faces, 4, 3)
    normals = np.tile([0.0, 0.0, 2.0], (4, 1))                  # not of unit length: the rule normalises
    islands = np.ones(4, np.int64)
    code = np.full((5, 7), 32768 + 100, np.int32)
    has, labels = np.ones((5, 7), np.uint8), np.ones((5, 7), np.uint8)
    flat = ref.points(obj.vertices, topo)
    out, sampled = ref.displace(obj.vertices, normals, obj.uvs, faces, uv_faces, islands, topo, code, has, labels, 0.001)
    assert sampled.all() and np.array_equal(out[:, :2], flat[:, :2]) and np.abs(out[:, 2] - 0.1).max() <= 1e-15
    out, sampled = ref.displace(obj.vertices, normals, obj.uvs, faces, uv_faces, islands, topo, code, has * 0, labels, 0.001)
    assert not sampled.any() and np.array_equal(out, flat)
    out, sampled = ref.displace(obj.vertices, normals, obj.uvs, faces, uv_faces, islands, topo, code, has, labels * 2, 0.001)
    assert not sampled.any() and np.array_equal(out, flat)
    # the v flip: the top row of the image is v = 1
    ramp = code.copy()
    ramp[0] = 32768 + 300
    out, _ = ref.displace(obj.vertices, normals, obj.uvs, faces, uv_faces, islands, topo, ramp, has, labels, 0.001)
    top = flat[:, 1] == 1.0
    assert top.sum() == 4 and np.abs(out[top, 2] - 0.3).max() <= 1e-15 and np.abs(out[flat[:, 1] == 0.0, 2] - 0.1).max() <= 1e-15
    # weights of zero on the only counting taps: the plain mean of the counting taps
    only = np.zeros((5, 7), np.uint8)
    only[:, 1] = 1                                              # u = 0 gives x = 0: fx = 0, the taps at x1 = 1 weigh nothing
    out, sampled = ref.displace(obj.vertices, normals, obj.uvs, faces, uv_faces, islands, topo, ramp, only, labels, 0.001)
    left = flat[:, 0] == 0.0
    assert sampled[left].all() and not sampled[flat[:, 0] == 1.0].any()
    assert np.abs(out[left & top, 2] - 0.2).max() <= 1e-15       # y = 0: rows 0 and 1 both count, (300 + 100) / 2 steps
    # a zero normal, a non-finite position
    zero = normals.copy()
    zero[0] = 0.0
    out, sampled = ref.displace(obj.vertices, zero, obj.uvs, faces, uv_faces, islands, topo, code, has, labels, 0.001)
    assert sampled[0] == 0 and np.array_equal(out[0], obj.vertices[0]) and sampled[1:4].all()


def test_argument_errors_come_before_a_device():
    obj = square()
    for bad in (0, 65, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="level"):
            TS.Tessellation(obj, bad)
        with pytest.raises(ValueError, match="level"):
            TS.check_level(bad)
    assert TS.check_level(1) == 1 and TS.check_level(np.int64(64)) == 64
    with pytest.raises(ValueError, match="uv"):                 # a face whose uv face has another length
        TS.Tessellation(meshrender.FaceObj(obj.vertices, obj.uvs, [[0, 1, 2, 3]], [[0, 1, 2]]), 2)
    with pytest.raises(ValueError, match="uv faces"):           # fewer uv faces than faces
        TS.Tessellation(meshrender.FaceObj(obj.vertices, obj.uvs, [[0, 1, 2], [0, 2, 3]], [[0, 1, 2]]), 2)
    with pytest.raises(ValueError, match="outside"):
        TS.Tessellation(meshrender.FaceObj(obj.vertices[:3], obj.uvs, [[0, 1, 2, 3]], [[0, 1, 2, 3]]), 2)
    with pytest.raises(ValueError, match="outside"):
        TS.Tessellation(meshrender.FaceObj(obj.vertices, obj.uvs[:3], [[0, 1, 2, 3]], [[0, 1, 2, 3]]), 2)
    with pytest.raises(ValueError, match="twice"):
        TS.Tessellation(meshrender.FaceObj(obj.vertices, obj.uvs, [[0, 1, 1]], [[0, 1, 2]]), 2)
    with pytest.raises(ValueError, match="2\\^31"):
        TS.fine_sizes(10, 30, 1 << 19, 64)
    assert TS.fine_sizes(4, 5, 2, 3) == (4 + 5 * 2 + 2, 18)
    # maps of the wrong dtype or shape
    code = torch.zeros(4, 5, dtype=torch.int32)
    has = torch.ones(4, 5, dtype=torch.uint8)
    labels = torch.ones(4, 5, dtype=torch.uint8)
    assert TS.check_maps(code, has, labels) == (4, 5) and TS.check_maps(code, has.bool()) == (4, 5)
    for args, what in (((code.to(torch.int64), has), "code"), ((code.numpy(), has), "code"), ((code.reshape(-1), has), "code"),
                       ((code, has.to(torch.int32)), "has"), ((code, torch.ones(5, 4, dtype=torch.uint8)), "has"),
                       ((code, has, labels.to(torch.int32)), "labels"), ((code, has, labels[:3]), "labels")):
        with pytest.raises(ValueError, match=what):
            TS.check_maps(*args)
        if len(args) == 2:
            with pytest.raises(ValueError, match=what):
                TS.displace_frame(obj, obj.vertices, args[0], args[1], 2, 0.01)
    with pytest.raises(ValueError, match="level"):
        TS.displace_frame(obj, obj.vertices, code, has, 0, 0.01)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="dist"):
            TS.displace_frame(obj, obj.vertices, code, has, 2, bad)


def test_command_lines_refuse_bad_options(tmp_path):
    from topo4d_amd import evaluate as E
    (tmp_path / "exp" / "seq").mkdir(parents=True)
    (tmp_path / "scans").mkdir()
    base = ["-e", "exp", "-s", "seq", "-od", str(tmp_path), "--set", "none", "--scans", str(tmp_path / "scans")]
    for extra in (["--disp_apply", "2"], ["--bake_disp", "0", "--disp_apply", "2"], ["--bake_disp", "0.01", "--disp_apply", "0"],
                  ["--bake_disp", "0.01", "--disp_apply", "65"], ["--bake_disp", "0.01", "--disp_save_obj"]):
        with pytest.raises(SystemExit) as e:
            E.evaluate(E.build_parser().parse_args(base + extra))
        assert "disp_apply" in str(e.value), extra
    args = E.build_parser().parse_args(base)
    assert (args.disp_apply, args.disp_save_obj) == (None, False) and E.disp_png_options(args) is None
    args = E.build_parser().parse_args(base + ["--bake_disp", "32767", "--disp_apply", "4"])
    assert E.disp_png_options(args) == {"zero": 32768, "unit": 1.0, "fill": False, "smooth": 0, "normals": False}      # implies --disp_png
    own = ["-e", "exp", "-s", "seq", "-od", str(tmp_path)]
    for extra in (["--level", "0", "--dist", "0.01"], ["--level", "65", "--dist", "0.01"], ["--level", "2", "--dist", "0"]):
        with pytest.raises(SystemExit) as e:
            TS.apply_tree(TS.build_parser().parse_args(own + extra))
        assert "level" in str(e.value)
    with pytest.raises(SystemExit):
        TS.build_parser().parse_args(own + ["--dist", "0.01"])  # --level is required
    with pytest.raises(SystemExit, match="no run"):
        TS.apply_tree(TS.build_parser().parse_args(["-e", "exp", "-s", "other", "-od", str(tmp_path), "--level", "2", "--dist", "0.01"]))
