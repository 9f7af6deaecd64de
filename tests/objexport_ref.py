"""
Host restatements the face.obj export is checked against (tests/test_objexport_host.py, tests/test_gpu_objexport.py,
tools/gen_golden_mesh.py, tools/bench_objexport.py).  Plain numpy / torch on the CPU, no topo4d_amd code.

  write_obj_with_uv      helpers.write_obj_with_uv (helpers.py:258-272), writing to a path or returning the bytes
  trimesh_vertex_normals trimesh 4.4.1 Trimesh(vertices, faces).vertex_normals, restated (trimesh is not a dependency here):
                         trimesh/base.py Trimesh.vertex_normals -> geometry.weighted_vertex_normals (the sparse path:
                         geometry.index_sparse, a scipy CSR product: per vertex, ascending face order), with
                         Trimesh.face_normals -> triangles.normals (util.unitize(cross, check_valid=True), zero rows where
                         invalid), Trimesh.face_angles -> triangles.angles, and util.unitize (tol.zero = 1e-13: rows at or below
                         it are multiplied by their norm, not divided by it)
  seam_color_index       helpers.duplicate_texture_vertex_color_2 (helpers.py:923-934) as an index array
  save_mesh_vertices     the vertex arithmetic of helpers.save_mesh (helpers.py:963-979), torch / numpy on the CPU
"""
import io

import numpy as np
import torch

TOL_ZERO = np.finfo(np.float64).resolution * 100     # trimesh.constants.tol.zero
TOL_MERGE = 1e-8                                     # trimesh.constants.tol.merge


def write_obj_with_uv(file_path, vertices, faces, uvs, uv_faces):
    """helpers.py:258-272 line for line; file_path None returns the bytes."""
    file = io.StringIO()
    for vertex in vertices:
        file.write(f'v {vertex[0]} {vertex[1]} {vertex[2]}\n')
    for uv in uvs:
        file.write(f'vt {uv[0]} {uv[1]}\n')
    for face, uv_face in zip(faces, uv_faces):
        face_str = 'f'
        for v_idx, uv_idx in zip(face, uv_face):
            face_str += f' {v_idx + 1}/{uv_idx + 1}'
        file.write(face_str + '\n')
    data = file.getvalue().encode()
    if file_path is None:
        return data
    with open(file_path, 'wb') as f:
        f.write(data)


def unitize(vectors, check_valid=False):
    """trimesh.util.unitize for an (m, 3) array."""
    vectors = np.asarray(vectors, dtype=np.float64)
    norm = np.sqrt(np.dot(vectors * vectors, [1.0] * vectors.shape[1]))
    valid = norm > TOL_ZERO
    norm[valid] **= -1
    unit = vectors * norm.reshape((-1, 1))
    if check_valid:
        return unit[valid], valid
    return unit


def face_normals(triangles):
    """Trimesh.face_normals: unit cross products, zero where the cross product's norm is at or below tol.zero."""
    crosses = np.cross(triangles[:, 1] - triangles[:, 0], triangles[:, 2] - triangles[:, 0])
    unit, valid = unitize(crosses, check_valid=True)
    padded = np.zeros((len(triangles), 3), dtype=np.float64)
    padded[valid] = unit
    return padded


def face_angles(triangles):
    """trimesh.triangles.angles."""
    u = unitize(triangles[:, 1] - triangles[:, 0])
    v = unitize(triangles[:, 2] - triangles[:, 0])
    w = unitize(triangles[:, 2] - triangles[:, 1])
    result = np.zeros((len(triangles), 3), dtype=np.float64)
    result[:, 0] = np.arccos(np.clip(np.dot(u * v, [1.0] * 3), -1, 1))
    result[:, 1] = np.arccos(np.clip(np.dot(-u * w, [1.0] * 3), -1, 1))
    result[:, 2] = np.pi - result[:, 0] - result[:, 1]
    result[(result < TOL_MERGE).any(axis=1), :] = 0.0
    return result


def trimesh_vertex_normals(vertices, faces):
    """Trimesh(vertices, faces).vertex_normals in float64, for a mesh whose vertices are all referenced and distinct (what
    process=True would otherwise merge or drop)."""
    vertices = np.asarray(vertices, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64)
    triangles = vertices[faces]
    normals, angles = face_normals(triangles), face_angles(triangles)
    rows = faces.ravel()
    cols = np.repeat(np.arange(len(faces)), 3)
    order = np.lexsort((cols, rows))                     # the CSR order: by vertex, then ascending face
    rows, cols, data = rows[order], cols[order], angles.ravel()[order]
    # a face listing a vertex twice: scipy sums the duplicate (vertex, face) entries before the product
    key = rows * len(faces) + cols
    first = np.concatenate([[True], key[1:] != key[:-1]])
    seg = np.cumsum(first) - 1
    weight = np.zeros(int(first.sum()))
    np.add.at(weight, seg, data)
    summed = np.zeros((len(vertices), 3), dtype=np.float64)
    np.add.at(summed, rows[first], weight[:, None] * normals[cols[first]])
    return unitize(summed)


def seam_color_index(uvs_ori, uvs_texture_ori):
    """duplicate_texture_vertex_color_2(variables, colors) == colors[seam_color_index(...)] (the same dict, the same overwrite
    order, a KeyError on a UV no vertex lists)."""
    uv_dict = {}
    for idx, uvs_ in enumerate(uvs_texture_ori):
        for uv in uvs_:
            uv_dict[tuple(uv)] = idx
    return np.asarray([uv_dict[tuple(uv)] for uv in np.asarray(uvs_ori)], dtype=np.int64)


def build_rotation(q):
    """external.py:26-43 on the CPU."""
    norm = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    q = q / norm[:, None]
    rot = torch.zeros((q.size(0), 3, 3))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rot[:, 0, 0] = 1 - 2 * (y * y + z * z)
    rot[:, 0, 1] = 2 * (x * y - r * z)
    rot[:, 0, 2] = 2 * (x * z + r * y)
    rot[:, 1, 0] = 2 * (x * y + r * z)
    rot[:, 1, 1] = 1 - 2 * (x * x + z * z)
    rot[:, 1, 2] = 2 * (y * z - r * x)
    rot[:, 2, 0] = 2 * (x * z - r * y)
    rot[:, 2, 1] = 2 * (y * z + r * x)
    rot[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return rot


def save_mesh_vertices(means3D, log_scales, unnorm_rotations, faces, trans_g, frame, normals=None):
    """helpers.py:965-979: the float64 vertices save_mesh writes (CPU tensors / arrays in, numpy out)."""
    means3D = torch.as_tensor(means3D, dtype=torch.float32)
    if frame != 1:
        vertices = means3D.clone()
        if normals is None:
            normals = trimesh_vertex_normals(vertices.numpy(), faces)
        normals = torch.from_numpy(np.array(normals, dtype=np.float64))
        scales = torch.exp(torch.as_tensor(log_scales, dtype=torch.float32))
        rots = build_rotation(torch.as_tensor(unnorm_rotations, dtype=torch.float32))
        normals_rot = torch.linalg.inv(rots.float()) @ normals.unsqueeze(-1).float()
        cast_scales = torch.sqrt(1.0 / (torch.sum((normals_rot.squeeze(2) ** 2) / (scales ** 2), dim=1)))
        cast_scales = torch.clamp(cast_scales, 0.0, 0.001)
        vertices = (vertices + cast_scales.unsqueeze(-1) * normals).numpy()
    else:
        vertices = means3D.numpy()
    tg = np.linalg.inv(trans_g)
    vertices = vertices @ tg[:3, :3].T
    return vertices + tg[:3, 3]
