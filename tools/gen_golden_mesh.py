"""
TEST INFRASTRUCTURE.  Writes tests/golden/g14_save_mesh.npz by calling the REAL reference's helpers.save_mesh
(helpers.py:963-998) and helpers.write_obj_with_uv (helpers.py:258-272) through oracle/gen_golden.py's import stubs.  Runs only
where the reference tree exists.  The fixture holds seeded inputs and what the reference wrote.

    python tools/gen_golden_mesh.py

Meshes: G13's seeded quad meshes (tools/gen_golden_dense.py: seams, a fin, a triangle fan, shuffled vertex numbers and corner
orders), with the UVs no corner uses removed (the reference's seam lookup would raise on them), plus one small mesh with a
degenerate face (a vertex at the midpoint of an edge, in one collinear triangle only, sharing its UV value with the edge's end:
a seam-dict overwrite) and a vertex whose two faces are one triangle in both windings (its face normals cancel).
variables["faces"] is helpers.triangulate_faces(faces_ori); uvs_texture_ori lists the distinct UVs of each vertex's corners,
as helpers.get_vertex_uvs builds it.

trimesh: not a dependency here, so the `trimesh` stub's Trimesh(...).vertex_normals is NOT trimesh's output: it is the float64
restatement tests/objexport_ref.trimesh_vertex_normals, which says which trimesh 4.4.1 lines it follows.  Everything after the
normals - build_rotation, torch.linalg.inv, the clamp, the float64 transform and the file - is the reference's own code.

Stored per mesh: the inputs, face.obj of frames 1 and 2 (exact bytes), the normals the stub returned, the float64 vertices the
reference passed to write_obj_with_uv in frames 1 and 2, and duplicate_texture_vertex_color_2 of colours = the row index.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import gen_golden  # noqa: E402
from gen_golden_dense import flat, synthetic_mesh  # noqa: E402
from tests import objexport_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g14_save_mesh.npz")
CASES = (("quad", 6, 7, 141), ("quad_b", 2, 2, 142))


def drop_unused_uvs(uv_faces, uvs):
    used = np.unique([u for f in uv_faces for u in f])
    remap = -np.ones(len(uvs), np.int64)
    remap[used] = np.arange(len(used))
    return [[int(remap[u]) for u in f] for f in uv_faces], uvs[used]


def special_mesh(seed):
    """A 3 x 3 quad grid, a degenerate (collinear) triangle on a new midpoint vertex, a triangle used in both windings by a
    new vertex."""
    rng = np.random.default_rng(seed)
    # positions on a 2^-10 grid: the midpoint below is exact, so the degenerate face is exactly collinear
    pos = [[round((c + rng.uniform(-0.2, 0.2)) * 1024) / 1024, round((r + rng.uniform(-0.2, 0.2)) * 1024) / 1024,
            round(rng.uniform(-0.3, 0.3) * 1024) / 1024] for r in range(4) for c in range(4)]
    uv = [[c / 5 + rng.uniform(-0.01, 0.01), r / 5 + rng.uniform(-0.01, 0.01)] for r in range(4) for c in range(4)]
    g = lambda r, c: r * 4 + c
    faces = [[g(r, c), g(r, c + 1), g(r + 1, c + 1), g(r + 1, c)] for r in range(3) for c in range(3)]
    uv_faces = [list(f) for f in faces]
    a, b = g(0, 0), g(0, 1)
    mid = len(pos)                                                  # the degenerate face's own vertex
    pos.append([(pos[a][i] + pos[b][i]) / 2 for i in range(3)])
    faces.append([a, b, mid])
    uv_faces.append([a, b, a])                                      # mid's UV value is a's: the seam dict keeps the later vertex
    v = len(pos)                                                    # the cancelling vertex
    p, q = g(3, 3), g(3, 2)
    pos.append([pos[p][0] + 0.5, pos[p][1] + 0.5, pos[p][2]])
    uv.append([0.9, 0.9])
    faces += [[v, p, q], [v, q, p]]
    uv_faces += [[len(uv) - 1, p, q], [len(uv) - 1, q, p]]
    return np.asarray(pos, np.float32), faces, uv_faces, np.asarray(uv, np.float64)


def vertex_uvs(faces, uv_faces, uvs, n):
    """helpers.get_vertex_uvs: per vertex, the distinct UVs (tuples) of its corners."""
    out = [set() for _ in range(n)]
    for f, uf in zip(faces, uv_faces):
        for vi, ui in zip(f, uf):
            out[vi].add(tuple(float(x) for x in uvs[ui]))
    return [sorted(s) for s in out]


def rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3] = q * rng.uniform(0.5, 2.0)
    m[:3, 3] = rng.normal(size=3) * 10
    return m


class _Trimesh:
    def __init__(self, vertices, faces=None, **kw):
        self.vertex_normals = objexport_ref.trimesh_vertex_normals(vertices, faces)
        _Trimesh.last = self.vertex_normals


def main():
    helpers, _ = gen_golden.import_reference_helpers()
    sys.modules["trimesh"].Trimesh = _Trimesh
    _zeros = torch.zeros
    torch.zeros = lambda *a, **k: _zeros(*a, **{x: y for x, y in k.items() if x != "device"})
    seen = {}
    _write = helpers.write_obj_with_uv

    def recording_write(file_path, vertices, faces, uvs, uv_faces):
        seen["vertices"] = np.array(vertices)
        return _write(file_path, vertices, faces, uvs, uv_faces)
    helpers.write_obj_with_uv = recording_write

    meshes = [(name,) + synthetic_mesh(R, Cn, seed)[:4] + (seed,) for name, R, Cn, seed in CASES]
    meshes.append(("special",) + special_mesh(143) + (143,))
    out = {}
    for name, P, faces, uv_faces, uvs, seed in meshes:
        uv_faces, uvs = drop_unused_uvs(uv_faces, uvs)
        n = P.shape[0]
        rng = np.random.default_rng(seed + 1000)
        texture = vertex_uvs(faces, uv_faces, uvs, n)
        tri = np.asarray(helpers.triangulate_faces(faces), np.int64)
        trans_g = rigid(rng)
        params = {"means3D": torch.from_numpy(P),
                  "log_scales": torch.from_numpy(rng.uniform(-8.0, -4.0, (n, 3)).astype(np.float32)),
                  "unnorm_rotations": torch.from_numpy(rng.normal(size=(n, 4)).astype(np.float32))}
        variables = {"faces": tri, "trans_g": trans_g, "faces_ori": faces, "uvs_ori": np.array(uvs), "uv_faces_ori": uv_faces,
                     "uvs_texture_ori": texture}
        with tempfile.TemporaryDirectory() as d:
            for frame in (1, 2):
                helpers.save_mesh(d, params, variables, frame, gen_texture=False)
                out[f"{name}/obj_frame{frame}"] = np.frombuffer(open(os.path.join(d, "face.obj"), "rb").read(), np.uint8)
                out[f"{name}/vertices_frame{frame}"] = seen["vertices"]
                if frame == 2:
                    out[f"{name}/normals"] = np.array(_Trimesh.last)
        lens, fl = flat(faces)
        _, ufl = flat(uv_faces)
        out[f"{name}/means3D"] = P
        out[f"{name}/log_scales"] = params["log_scales"].numpy()
        out[f"{name}/unnorm_rotations"] = params["unnorm_rotations"].numpy()
        out[f"{name}/trans_g"] = trans_g
        out[f"{name}/faces"] = tri.astype(np.int32)
        out[f"{name}/face_lens"] = lens
        out[f"{name}/faces_ori"] = fl
        out[f"{name}/uv_faces_ori"] = ufl
        out[f"{name}/uvs_ori"] = uvs
        out[f"{name}/texture_counts"] = np.asarray([len(t) for t in texture], np.int32)
        out[f"{name}/texture_uvs"] = np.asarray([uv for t in texture for uv in t], np.float64)
        colors = np.arange(n, dtype=np.int64)[:, None]
        out[f"{name}/seam_index"] = np.array(helpers.duplicate_texture_vertex_color_2(variables, colors))[:, 0]
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
