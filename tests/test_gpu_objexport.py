"""GPU: the face.obj export of topo4d_amd/objexport.py (csrc/t4d_obj.hip, csrc/t4d_repr.h).  The formatter is byte-exact
against Python's repr; write_obj_with_uv reproduces golden G14 (the reference's own save_mesh, tools/gen_golden_mesh.py) and the
restated writer byte for byte; the vertex normals agree with the trimesh restatement to 1e-12; save_mesh's frames 1 and 2 agree
with G14 within the bounds of the float64 transform and the float32 cast chain; face.png is the reference's seam-duplicated bake;
an exporter reused across frames writes what fresh ones write."""
import os

import numpy as np
import pytest
import torch

from tests import objexport_ref as ref
from tests.test_objexport_host import MESHES, g14, mesh, repr_test_values

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")


def device_params(params, extra=None):
    out = {k: torch.as_tensor(v).to(DEV) for k, v in params.items()}
    out.update(extra or {})
    return out


def lines(data: bytes, prefix: bytes):
    return [l for l in data.split(b"\n") if l.startswith(prefix + b" ")]


def v_values(data: bytes):
    return np.array([[float(x) for x in l.split()[1:]] for l in lines(data, b"v")])


def test_formatter_is_repr_byte_for_byte():
    from topo4d_amd.objexport import format_float_repr
    rng = np.random.default_rng(14)
    vals = np.concatenate([repr_test_values(0), rng.integers(0, 2 ** 64, 1 << 20, dtype=np.uint64).view(np.float64),
                           rng.uniform(1e-3, 1e3, 1 << 20), np.array([-0.0, 2.0 ** 53 + 1, 2.0 ** 53 - 1, 1e16, 1e-5, 1e-4])])
    got = format_float_repr(torch.from_numpy(vals).to(DEV))
    assert len(got) == vals.size
    bad = [(repr(float(x)), s) for x, s in zip(vals.tolist(), got) if repr(x) != s]
    assert not bad, bad[:10]
    assert max(len(s) for s in got) <= 24


@pytest.mark.parametrize("name", MESHES)
def test_writer_reproduces_g14_bytes(tmp_path, name):
    from topo4d_amd.objexport import write_obj_with_uv
    g = g14()
    variables, _ = mesh(name)
    for frame in (1, 2):
        verts = g[f"{name}/vertices_frame{frame}"]
        path = tmp_path / f"f{frame}.obj"
        write_obj_with_uv(path, verts, variables["faces_ori"], variables["uvs_ori"], variables["uv_faces_ori"])
        assert path.read_bytes() == g[f"{name}/obj_frame{frame}"].tobytes(), (name, frame)


def test_writer_matches_restated_writer_on_random_mixed_meshes(tmp_path):
    from topo4d_amd.objexport import write_obj_with_uv
    rng = np.random.default_rng(7)
    for trial in range(4):
        n, m, nf = int(rng.integers(1, 3000)), int(rng.integers(1, 3000)), int(rng.integers(1, 4000))
        scale = 10.0 ** rng.uniform(-12, 12, (n, 1))
        verts = rng.normal(size=(n, 3)) * scale
        verts[rng.random((n, 3)) < 0.01] = 0.0
        uvs = rng.random((m, 2))
        sizes = rng.choice([3, 4], nf)
        faces = [[int(x) for x in rng.integers(0, n, k)] for k in sizes]
        uv_faces = [[int(x) for x in rng.integers(0, m, k)] for k in sizes]
        arg_faces = faces if trial % 2 == 0 else [np.asarray(f) for f in faces]
        path = tmp_path / f"r{trial}.obj"
        src = verts if trial < 2 else torch.from_numpy(verts).to(DEV)
        write_obj_with_uv(path, src, arg_faces, uvs, uv_faces)
        assert path.read_bytes() == ref.write_obj_with_uv(None, verts, faces, uvs, uv_faces), trial


def head_surface():
    """An 8,280-vertex scaffold head (69 x 120 lat-long quads, triangulated as helpers.triangulate_faces does)."""
    from tests.test_gpu_densify import head_mesh
    params, faces, _, _, _, _ = head_mesh(69, 120, seed=11)
    tri = np.asarray([t for f in faces for t in ([f[0], f[1], f[2]], [f[0], f[2], f[3]])], np.int64)
    return params["means3D"].numpy().astype(np.float32), tri


def test_vertex_normals_match_the_trimesh_restatement():
    from topo4d_amd.objexport import vertex_normals
    g = g14()
    cases = [(g[f"{name}/means3D"], g[f"{name}/faces"]) for name in MESHES] + [head_surface()]
    assert cases[-1][0].shape[0] == 8280
    for P, faces in cases:
        want = ref.trimesh_vertex_normals(P, faces)
        for dtype in (torch.float32, torch.float64):
            got = vertex_normals(torch.from_numpy(P).to(DEV, dtype), torch.from_numpy(faces).to(DEV)).cpu().numpy()
            assert np.abs(got - want).max() <= 1e-12
    got = vertex_normals(torch.from_numpy(g["special/means3D"]).to(DEV), g["special/faces"]).cpu().numpy()
    zero = np.abs(g["special/normals"]).sum(1) == 0
    assert zero.sum() == 2 and (got[zero] == 0).all(), "the degenerate face's vertex and the cancelling vertex"


def test_vertex_normals_refuse_unreferenced_and_out_of_range():
    from topo4d_amd.objexport import vertex_normals
    g = g14()
    P = torch.from_numpy(g["quad_b/means3D"]).to(DEV)
    faces = g["quad_b/faces"]
    with pytest.raises(ValueError, match="in no face"):
        vertex_normals(torch.cat([P, P[:1]]), faces)
    with pytest.raises(ValueError, match="outside"):
        vertex_normals(P, np.vstack([faces, [[0, 1, P.shape[0]]]]))


@pytest.mark.parametrize("name", MESHES)
def test_save_mesh_frames_1_and_2_against_g14(tmp_path, name):
    from topo4d_amd.objexport import MeshExporter
    g = g14()
    variables, params = mesh(name)
    exp = MeshExporter(variables)
    p = device_params(params)
    tg = np.linalg.inv(variables["trans_g"])
    Rg = tg[:3, :3]
    for frame in (1, 2):
        exp.save_mesh(str(tmp_path), p, frame, gen_texture=False)
        got = (tmp_path / "face.obj").read_bytes()
        want = g[f"{name}/obj_frame{frame}"].tobytes()
        for prefix in (b"vt", b"f"):
            assert lines(got, prefix) == lines(want, prefix), prefix
        assert len(got.split(b"\n")) == len(want.split(b"\n"))
        gv, wv = v_values(got), v_values(want)
        assert gv.shape == wv.shape == (params["means3D"].shape[0], 3)
        if frame == 1:
            mag = np.abs(params["means3D"].astype(np.float64)) @ np.abs(Rg).T + np.abs(tg[:3, 3])
            assert (np.abs(gv - wv) <= 4 * np.spacing(mag)).all()
        else:
            assert np.abs(gv - wv).max() <= 2e-9 * np.linalg.norm(Rg, 2)
            zero = np.abs(g[f"{name}/normals"]).sum(1) == 0
            if zero.any():                                          # no normal, no offset
                v1 = exp.frame_vertices(p, 1).cpu().numpy()
                np.testing.assert_array_equal(exp.frame_vertices(p, 2).cpu().numpy()[zero], v1[zero])


def texture_case(name, seed=3):
    variables, params = mesh(name)
    rng = np.random.default_rng(seed)
    n, n_uv = params["means3D"].shape[0], variables["uvs_ori"].shape[0]
    extra = 200
    variables["dense_uvs"] = np.vstack([variables["uvs_ori"], rng.random((extra, 2))])
    variables["dense_uv_faces"] = rng.integers(0, n_uv + extra, (300, 3)).tolist()
    dense = rng.uniform(-0.2, 1.2, (n + extra, 3)).astype(np.float32)
    return variables, params, dense


def test_save_mesh_texture_is_the_seam_duplicated_bake(tmp_path):
    from PIL import Image
    from topo4d_amd import texture
    from topo4d_amd.objexport import MeshExporter
    variables, params, dense = texture_case("quad")
    n = params["means3D"].shape[0]
    p = device_params(params, {"dense_rgb_colors": torch.from_numpy(dense).to(DEV)})
    MeshExporter(variables).save_mesh(str(tmp_path / "out"), p, 2, res=96, gen_texture=True)
    clamped = np.clip(dense, 0.0, 1.0)
    colors = np.array([clamped[:n][i] for i in ref.seam_color_index(variables["uvs_ori"], variables["uvs_texture_ori"])])
    colors = np.concatenate((colors, clamped[n:]), axis=0)
    texture.write_texture(str(tmp_path / "want.png"), np.array(variables["dense_uvs"]), colors, np.array(variables["dense_uv_faces"]),
                          res=96, encoder="gpu")
    got = np.asarray(Image.open(tmp_path / "out" / "face.png"))
    want = np.asarray(Image.open(tmp_path / "want.png"))
    np.testing.assert_array_equal(got, want)
    assert got.any()


def test_exporter_reused_across_frames_equals_fresh_calls(tmp_path):
    from topo4d_amd import objexport
    variables, params = mesh("quad")
    rng = np.random.default_rng(9)
    frames = []
    for t in range(2):
        q = dict(params)
        q["means3D"] = (params["means3D"] + rng.normal(size=params["means3D"].shape) * 0.01).astype(np.float32)
        frames.append(device_params(q))
    exp = objexport.MeshExporter(variables)
    reused = [exp.obj_bytes(frames[t], 2 + t) for t in range(2)]
    fresh = [objexport.MeshExporter(variables).obj_bytes(frames[t], 2 + t) for t in range(2)]
    assert reused == fresh and reused[0] != reused[1]
    for t in range(2):                                              # the drop-in, through its per-topology cache
        objexport.save_mesh(str(tmp_path / str(t)), frames[t], variables, 2 + t, gen_texture=False)
        assert (tmp_path / str(t) / "face.obj").read_bytes() == reused[t]
