"""
TEST INFRASTRUCTURE.  Writes tests/golden/g13_dense_build.npz by calling the REAL reference's densification helpers -
helpers.get_face_faces (helpers.py:361-377), helpers.build_dense_vertices_2 (helpers.py:602-654) and helpers.triangulate_faces
(helpers.py:657-667) - through oracle/gen_golden.py's import stubs.  Runs only where the reference tree exists.  The fixture holds
seeded inputs and the numbers the reference returned.

    python tools/gen_golden_dense.py

The meshes are seeded and synthetic (the reference's face_v5.obj is not part of it): a jittered quad grid with shuffled vertex
numbers and randomly rotated / reversed corner orders (so that shared edges occur with face[a] > face[b] and with <), a UV seam
down one grid column (its vertices carry two UVs: seam edges are duplicated, the edges crossing it are half-seam and shared), one
quad whose four corners all carry two UVs, a "fin" quad on an interior edge (an edge shared by three quads), a triangle fan on the
boundary, and quads outside face_masks (non-frontal).  Faces are shuffled, triangles and quads interleaved.  Densities 1, 2, 3 and
7 on a 6 x 7 grid, 30 on a 2 x 2 grid with its fin.

kNN: open3d is not a dependency here, so the kNN part is NOT the reference's output: it is a float64 brute-force restatement of
o3d_knn(pts, k)[0].mean(-1) (helpers.py:147-157, train.py:131-132, :245-246) - per point, the k+1 smallest squared distances
((dx*dx + dy*dy) + dz*dz), its own zero included, summed in ascending order and divided by k - on the dense vertices of the
density-3 case and on a small set with exact duplicates and an isolated outlier.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g13_dense_build.npz")
CASES = (("d1", 6, 7, 1, 131), ("d2", 6, 7, 2, 132), ("d3", 6, 7, 3, 133), ("d7", 6, 7, 7, 137), ("d30", 2, 2, 30, 130))


def synthetic_mesh(R, Cn, seed):
    """A seeded (R x Cn)-quad mesh with every feature of the module docstring.  Returns the reference's input shapes: means3D
    float32 [n,3], faces_ori / uv_faces_ori lists of lists, uvs_ori float64 [m,2], uvs_texture_ori (list of lists), face_masks."""
    rng = np.random.default_rng(seed)
    gv = (R + 1) * (Cn + 1)
    gid = lambda r, c: r * (Cn + 1) + c
    pos = [[c + rng.uniform(-0.2, 0.2), r + rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3)] for r in range(R + 1) for c in range(Cn + 1)]
    uv = [[c / (Cn + 2) + rng.uniform(-0.01, 0.01), r / (R + 2) + rng.uniform(-0.01, 0.01)] for r in range(R + 1) for c in range(Cn + 1)]
    seam_c = Cn // 2
    seam_uv = {}                                          # second UV of a seam vertex, used by the quads right of the seam
    for r in range(R + 1):
        seam_uv[gid(r, seam_c)] = len(uv)
        uv.append([uv[gid(r, seam_c)][0] + 0.5, uv[gid(r, seam_c)][1]])
    faces, uv_faces = [], []
    for r in range(R):
        for c in range(Cn):
            q = [gid(r, c), gid(r + 1, c), gid(r + 1, c + 1), gid(r, c + 1)]
            uq = [seam_uv[v] if (v in seam_uv and c >= seam_c) else v for v in q]
            rot = int(rng.integers(4))
            q, uq = q[rot:] + q[:rot], uq[rot:] + uq[:rot]
            if rng.random() < 0.5:
                q, uq = q[::-1], uq[::-1]
            faces.append(q)
            uv_faces.append(uq)
    # the all-seam quad: the last quad of grid row 1 (frontal), every corner gets a second (unused) UV
    allseam = set(faces[Cn + Cn - 1])
    for v in allseam:
        if v not in seam_uv:
            seam_uv[v] = len(uv)
            uv.append([uv[v][0], uv[v][1] + 0.25])
    # fin: a third quad on the interior horizontal edge (1,0)-(1,1), away from the seam column and the all-seam quad
    a, b = gid(1, 0), gid(1, 1)
    x, y = len(pos), len(pos) + 1
    pos += [[pos[a][0], pos[a][1], pos[a][2] + 1.0], [pos[b][0], pos[b][1], pos[b][2] + 1.0]]
    uv += [[uv[a][0], uv[a][1] + 0.05], [uv[b][0], uv[b][1] + 0.05]]
    faces.append([b, a, x, y])
    uv_faces.append([b, a, len(uv) - 2, len(uv) - 1])
    # triangle fan on the bottom boundary (row 0) around a new centre vertex
    ctr = len(pos)
    pos.append([Cn / 2, -1.0, 0.0])
    uv.append([0.5, 0.0])
    for c in range(Cn):
        faces.append([ctr, gid(0, c + 1), gid(0, c)])
        uv_faces.append([len(uv) - 1, gid(0, c + 1), gid(0, c)])
    n = len(pos)
    # shuffle vertex numbers (orientation tests see both outcomes) and face order
    perm = rng.permutation(n)
    faces = [[int(perm[v]) for v in f] for f in faces]
    P = np.zeros((n, 3), np.float32)
    P[perm] = np.asarray(pos, np.float32)
    order = rng.permutation(len(faces))
    faces = [faces[i] for i in order]
    uv_faces = [list(map(int, uv_faces[i])) for i in order]
    # uvs_texture_ori (helpers.get_vertex_uvs): the distinct UVs of each vertex; only their number is read (helpers.py:433-465)
    texture = [[tuple(uv[v])] if v < gv else [(float(v), 0.0)] for v in range(n)]
    for v, extra in seam_uv.items():
        texture[v].append(tuple(uv[extra]))
    texture = [texture[v] for v in np.argsort(perm)]
    # face_masks: every vertex but those of the last two grid rows, so that the last quad row is non-frontal (R > 2)
    unmasked = {gid(r, c) for r in (R - 1, R) for c in range(Cn + 1)} if R > 2 else {gid(R, c) for c in range(Cn + 1)}
    face_masks = np.array(sorted(int(perm[v]) for v in range(n) if v not in unmasked), np.int64)
    return P, faces, uv_faces, np.asarray(uv, np.float64), texture, face_masks


def reference_build(helpers, means3D, faces_ori, uv_faces_ori, uvs_ori, uvs_texture_ori, face_vertex_mask, dense_num):
    """train.py:213-243 restated line for line around the reference's own helpers."""
    variables = {'faces_ori': faces_ori, 'uv_faces_ori': uv_faces_ori, 'uvs_ori': np.array(uvs_ori), 'uvs_texture_ori': uvs_texture_ori}
    vertices = means3D.copy()                                                                              # train.py:214
    quad_faces = np.array([face for face in variables['faces_ori'] if len(face) == 4])                    # train.py:217
    quad_faces_idx = np.array([idx for idx, face in enumerate(variables['faces_ori']) if len(face) == 4])  # train.py:218
    tri_faces = np.array([face for face in variables['faces_ori'] if len(face) == 3])                     # train.py:219
    tri_uv_faces = np.array([face for face in variables['uv_faces_ori'] if len(face) == 3])               # train.py:220
    quad_faces, quad_faces_idx, no_face_quad_faces, no_face_quad_faces_idx = helpers.get_face_faces(      # train.py:222-224
        np.array(quad_faces), np.array(quad_faces_idx), face_vertex_mask)
    no_face_quad_uv_faces = np.array([variables['uv_faces_ori'][i] for i in no_face_quad_faces_idx])      # train.py:225
    vertices, dense_faces, dense_uv, dense_uv_faces, new_vertex_father, new_vertex_weight = helpers.build_dense_vertices_2(
        variables, vertices, quad_faces, quad_faces_idx, dense_num, variables['uvs_texture_ori'])         # train.py:230
    dense_uv_faces = tri_uv_faces.tolist() + dense_uv_faces.tolist() + no_face_quad_uv_faces.tolist()     # train.py:232
    dense_faces = tri_faces.tolist() + dense_faces.tolist() + no_face_quad_faces.tolist()                 # train.py:233
    dense_uv_faces = helpers.triangulate_faces(dense_uv_faces)                                            # train.py:235
    dense_faces = helpers.triangulate_faces(dense_faces)                                                  # train.py:236
    return {'dense_quad_faces': quad_faces, 'dense_vertex_father': new_vertex_father,                     # train.py:238-243, :265
            'dense_vertex_weight': new_vertex_weight, 'dense_faces': dense_faces, 'dense_uv_faces': dense_uv_faces,
            'dense_vertex': np.array(vertices), 'dense_uvs': dense_uv}


def brute_knn(pts, k):
    pts = np.asarray(pts, np.float64)
    out = np.empty(pts.shape[0])
    for i in range(pts.shape[0]):
        d = pts[i] - pts
        dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        s = 0.0
        for v in np.sort(dist)[:k + 1]:
            s += v
        out[i] = s / k
    return out


def flat(faces):
    return np.asarray([len(f) for f in faces], np.int8), np.asarray([v for f in faces for v in f], np.int32)


def main():
    helpers, _ = gen_golden.import_reference_helpers()
    out = {}
    for name, R, Cn, d, seed in CASES:
        P, faces, uv_faces, uvs, texture, masks = synthetic_mesh(R, Cn, seed)
        ref = reference_build(helpers, P, faces, uv_faces, uvs, texture, masks, d)
        lens, fl = flat(faces)
        _, ufl = flat(uv_faces)
        out[f"{name}/means3D"] = P
        out[f"{name}/face_lens"] = lens
        out[f"{name}/faces"] = fl
        out[f"{name}/uv_faces"] = ufl
        out[f"{name}/uvs_ori"] = uvs
        out[f"{name}/uv_counts"] = np.asarray([len(t) for t in texture], np.int8)
        out[f"{name}/face_masks"] = masks.astype(np.int32)
        out[f"{name}/density"] = np.int32(d)
        dv = ref['dense_vertex']
        assert np.array_equal(dv.astype(np.float32).astype(np.float64), dv), "dense_vertex holds float32 values"
        out[f"{name}/dense_vertex"] = dv.astype(np.float32)
        out[f"{name}/dense_quad_faces"] = np.asarray(ref['dense_quad_faces'], np.int32)
        out[f"{name}/dense_vertex_father"] = np.asarray(ref['dense_vertex_father'], np.int32)
        out[f"{name}/dense_vertex_weight"] = np.asarray(ref['dense_vertex_weight'], np.float64)
        out[f"{name}/dense_uvs"] = np.asarray(ref['dense_uvs'], np.float64)
        for key in ('dense_faces', 'dense_uv_faces'):
            arr = np.asarray(ref[key], np.float64)
            assert np.array_equal(arr, np.round(arr)) and arr.shape[1] == 3
            out[f"{name}/{key}"] = arr.astype(np.int32)
        if name == "d3":
            out["knn/dense_k4"] = brute_knn(dv, 4)
            out["knn/coarse_k1"] = brute_knn(P, 1)
    rng = np.random.default_rng(1313)
    pts = rng.normal(size=(300, 3))
    pts[10:20] = pts[0:10]                                                          # exact duplicates
    pts[50] = pts[51]
    pts[299] = [40.0, -35.0, 60.0]                                                  # an isolated outlier
    out["knn/points"] = pts
    for k in (1, 4, 8):
        out[f"knn/points_k{k}"] = brute_knn(pts, k)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
