"""CPU: the yardsticks of the face.obj export (tests/objexport_ref.py) against golden G14 (the reference's own save_mesh,
tools/gen_golden_mesh.py), the float formatter's host build (csrc/t4d_repr.h compiled with the system C++ compiler) against
Python's repr, and objexport's argument errors, which are raised before any device is needed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import objexport_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G14 = os.path.join(ROOT, "tests", "golden", "g14_save_mesh.npz")
MESHES = ("quad", "quad_b", "special")


def g14():
    return np.load(G14)


def unflat(lens, flat):
    out, i = [], 0
    for n in lens.astype(int):
        out.append([int(v) for v in flat[i:i + n]])
        i += n
    return out


def mesh(name):
    """G14's inputs in the reference's types."""
    g = g14()
    lens = g[f"{name}/face_lens"]
    counts = g[f"{name}/texture_counts"]
    tuv = g[f"{name}/texture_uvs"]
    starts = np.concatenate([[0], np.cumsum(counts)])
    texture = [[tuple(float(x) for x in tuv[j]) for j in range(starts[i], starts[i + 1])] for i in range(len(counts))]
    variables = {"faces": g[f"{name}/faces"].astype(np.int64), "trans_g": g[f"{name}/trans_g"],
                 "faces_ori": unflat(lens, g[f"{name}/faces_ori"]), "uv_faces_ori": unflat(lens, g[f"{name}/uv_faces_ori"]),
                 "uvs_ori": g[f"{name}/uvs_ori"], "uvs_texture_ori": texture}
    params = {k: g[f"{name}/{k}"] for k in ("means3D", "log_scales", "unnorm_rotations")}
    return variables, params


def repr_test_values(n_random=1 << 16, seed=0):
    """Every power of 2 and of 10 in range with both float64 neighbours, the special values, random bit patterns (all
    exponents, subnormals included) and random values in 1e-3..1e3; both signs."""
    rng = np.random.default_rng(seed)
    vals = [0.0, float("inf"), float("nan"), 5e-324, 2.0 ** 53 + 1, 2.0 ** 53 - 1, 2.0 ** 53, 1e16, 1e-5, 1e-4, 0.0001, 0.1, 1e22,
            1e23, 2.2250738585072014e-308, 1.7976931348623157e308, 123456789012345680.0, 9.999999999999999e15]
    for x in [2.0 ** e for e in range(-1074, 1024)] + [float(f"1e{e}") for e in range(-323, 309)]:
        vals += [x, np.nextafter(x, 0.0), np.nextafter(x, np.inf)]
    a = np.concatenate([np.asarray(vals, np.float64), rng.integers(0, 2 ** 64, n_random, dtype=np.uint64).view(np.float64),
                        rng.uniform(1e-3, 1e3, n_random)])
    return np.concatenate([a, -a])


def test_restated_writer_reproduces_g14():
    g = g14()
    for name in MESHES:
        variables, _ = mesh(name)
        for frame in (1, 2):
            data = ref.write_obj_with_uv(None, g[f"{name}/vertices_frame{frame}"], variables["faces_ori"], variables["uvs_ori"],
                                         variables["uv_faces_ori"])
            assert data == g[f"{name}/obj_frame{frame}"].tobytes(), (name, frame)


def test_restated_vertices_reproduce_g14():
    """save_mesh_vertices (the yardstick the GPU tests bound against) gives the vertices the reference wrote, within the bounds
    of the arithmetic it restates: torch's float32 exp / inverse / clamp chain and numpy's float64 product depend on the CPU's
    vector units and BLAS, so neither is bit-reproducible across hosts.  Frame 1: 4 ulp of sum_j |Rg_ij v_j| + |tg_i|; frame 2:
    2e-9 * ||Rg||_2 (float32 rounding of a push of at most 1e-3)."""
    g = g14()
    for name in MESHES:
        variables, params = mesh(name)
        tg = np.linalg.inv(variables["trans_g"])
        mag = np.abs(params["means3D"].astype(np.float64)) @ np.abs(tg[:3, :3]).T + np.abs(tg[:3, 3])
        v1 = ref.save_mesh_vertices(params["means3D"], None, None, None, variables["trans_g"], 1)
        assert (np.abs(v1 - g[f"{name}/vertices_frame1"]) <= 4 * np.spacing(mag)).all(), name
        v2 = ref.save_mesh_vertices(params["means3D"], params["log_scales"], params["unnorm_rotations"], variables["faces"],
                                    variables["trans_g"], 2)
        assert np.abs(v2 - g[f"{name}/vertices_frame2"]).max() <= 2e-9 * np.linalg.norm(tg[:3, :3], 2), name


def test_trimesh_restatement_reproduces_g14_normals():
    """Within 1e-14 (numpy's arccos and sqrt may use different vector code on different CPUs); exact zeros stay exact."""
    g = g14()
    for name in MESHES:
        variables, params = mesh(name)
        n = ref.trimesh_vertex_normals(params["means3D"], variables["faces"])
        want = g[f"{name}/normals"]
        assert np.abs(n - want).max() <= 1e-14, name
        np.testing.assert_array_equal(n[want == 0], 0.0)
    n = g["special/normals"]
    assert (np.abs(n).sum(1) == 0).sum() >= 2, "the degenerate face's own vertex and the cancelling vertex have zero normals"


def test_seam_map_matches_duplicate_texture_vertex_color_2():
    from topo4d_amd import objexport
    g = g14()
    for name in MESHES:
        variables, _ = mesh(name)
        want = g[f"{name}/seam_index"]
        np.testing.assert_array_equal(ref.seam_color_index(variables["uvs_ori"], variables["uvs_texture_ori"]), want)
        np.testing.assert_array_equal(objexport.seam_color_index(variables["uvs_ori"], variables["uvs_texture_ori"]), want)
    variables, _ = mesh("special")
    with pytest.raises(KeyError):
        objexport.seam_color_index(np.vstack([variables["uvs_ori"], [[7.0, 7.0]]]), variables["uvs_texture_ori"])


def test_numpy_float64_prints_as_repr():
    """The reference's f-strings format numpy float64, the formatter targets repr(float): the same strings."""
    for x in repr_test_values(1 << 12):
        assert f"{np.float64(x)}" == repr(float(x))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
def test_formatter_host_build_matches_repr(tmp_path):
    exe = tmp_path / "repr_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "repr_host.cpp")])
    vals = repr_test_values(1 << 18, seed=5)
    out = subprocess.run([str(exe)], input=vals.tobytes(), capture_output=True, check=True).stdout.decode().split("\n")[:-1]
    assert len(out) == vals.size
    bad = [(repr(float(x)), s) for x, s in zip(vals, out) if repr(float(x)) != s]
    assert not bad, bad[:10]


def test_repr_tables_are_generated():
    """csrc/t4d_repr_tables.h is exactly what tools/gen_repr_tables.py writes."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_repr_tables", os.path.join(ROOT, "tools", "gen_repr_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text = open(gen.OUT).read()
    assert "T4D_REPR_TABLE const uint64_t t4d_pow5[326][2]" in text
    for i in (0, 1, 27, 325):
        v = gen.pow5(i)
        assert f"{{0x{v & gen.MASK:016x}ull, 0x{v >> 64:016x}ull}}," in text
    for q in (0, 1, 22, 341):
        v = gen.pow5_inv(q)
        assert f"{{0x{v & gen.MASK:016x}ull, 0x{v >> 64:016x}ull}}," in text


def test_mesh_exporter_argument_errors():
    from topo4d_amd import objexport
    variables, _ = mesh("quad_b")
    n = int(variables["faces"].max()) + 1
    with pytest.raises(ValueError, match="in no face"):
        objexport.MeshExporter(variables, n_vertices=n + 1)
    bad = dict(variables, faces=np.vstack([variables["faces"], [[0, 1, n]]]))
    with pytest.raises(ValueError, match="outside"):
        objexport.MeshExporter(bad, n_vertices=n)
    neg = dict(variables, faces=np.vstack([variables["faces"], [[0, -1, 2]]]))
    with pytest.raises(ValueError, match="outside"):
        objexport.MeshExporter(neg, n_vertices=n)
    with pytest.raises(ValueError, match="triangle"):
        objexport.MeshExporter(dict(variables, faces=np.zeros((4, 4), np.int64)))
