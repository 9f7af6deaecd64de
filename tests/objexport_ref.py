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
  vertex_corner_csr      the vertex -> corner CSR and the two status counts of t4d_obj_vertex_faces
  normal_condition       the trimesh rule in long double, and each vertex's condition number (tests/obj_cases.py)
  frame_vertices_rule    k_obj_frame_vertices operation by operation: float32 cast chain, float64 push and transform
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


def vertex_corner_csr(faces, n_vert):
    """The vertex -> corner CSR as t4d_obj_vertex_faces defines it: (offsets int32 [n_vert + 1], entries int32, corners out of
    range, empty rows).  Corner 3 * face + k belongs to the vertex it names; a row lists its corners ascending; a corner naming
    a vertex outside [0, n_vert) is counted and left out."""
    named = np.asarray(faces, dtype=np.int64).reshape(-1)
    ok = (named >= 0) & (named < n_vert)
    counts = np.bincount(named[ok], minlength=n_vert)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    corners = np.nonzero(ok)[0]
    entries = corners[np.argsort(named[ok], kind="stable")].astype(np.int32)
    return offsets, entries, int((~ok).sum()), int((counts == 0).sum())


def normal_condition(vertices, faces):
    """(kappa [P], normals [P,3]) in np.longdouble (a 64-bit mantissa on x86): the trimesh rule of trimesh_vertex_normals
    evaluated in long double, and per vertex

        kappa_v = (sum_f |w_f| / || sum_f w_f n_f ||) / (the smallest sine of any angle of any face in the sum),

    the factor by which one rounding of a face's angle (acos loses 1 / sin of it) or of its normal (the cross product of two
    edges loses 1 / sin of their angle) grows in the unit sum.  w_f: the face's angles at the vertex, 0 for a face degenerate by
    tol.merge; n_f: its unit normal, 0 at or below tol.zero.  Such faces add exactly nothing in any precision, so the minimum
    runs over the others (which only lowers kappa); a vertex whose sum is exactly 0 has kappa = inf and a zero normal."""
    L = np.longdouble
    V = np.asarray(vertices, dtype=np.float64).astype(L)
    faces = np.asarray(faces, dtype=np.int64)
    tri = V[faces]
    ab, ac, bc = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], tri[:, 2] - tri[:, 1]

    def norm(x):
        return np.sqrt((x * x).sum(1))

    def unit(x):
        n = norm(x)
        return x * np.where(n > TOL_ZERO, L(1) / np.where(n > 0, n, L(1)), n)[:, None]

    cross = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                      ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1)
    has_normal = norm(cross) > TOL_ZERO
    normals = np.where(has_normal[:, None], unit(cross), L(0))
    u, v, w = unit(ab), unit(ac), unit(bc)
    angles = np.zeros((len(faces), 3), dtype=L)
    angles[:, 0] = np.arccos(np.clip((u * v).sum(1), -1, 1))
    angles[:, 1] = np.arccos(np.clip((-u * w).sum(1), -1, 1))
    angles[:, 2] = L(np.pi) - angles[:, 0] - angles[:, 1]
    degenerate = (angles < TOL_MERGE).any(axis=1)
    sines = np.sin(angles).min(axis=1)
    angles[degenerate] = 0
    in_sum = has_normal & ~degenerate
    rows = faces.ravel()
    weight = np.zeros(len(V), dtype=L)
    np.add.at(weight, rows, np.abs(angles).ravel())
    summed = np.zeros((len(V), 3), dtype=L)
    np.add.at(summed, rows, (angles[:, :, None] * normals[:, None, :]).reshape(-1, 3))
    least = np.full(len(V), np.inf, dtype=L)
    np.minimum.at(least, rows, np.repeat(np.where(in_sum, sines, L(np.inf)), 3))
    length = norm(summed)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(length > 0, weight / length / least, L(np.inf))
    return kappa, unit(summed)


def frame_vertices_rule(means3D, log_scales, rotations, normals, transform):
    """k_obj_frame_vertices (csrc/t4d_obj.hip) operation by operation: (vertices float64 [P,3], cast float32 [P] or None).
    normals None is frame 1.  Every float32 step is one numpy float32 operation per element in the kernel's order (numpy does
    not contract), the push v + double(cast) * n and ((v0 r0 + v1 r1) + v2 r2) + t are float64; a NaN cast stays NaN.
    transform: [3,4] float64 (rows of Rg, then tg).  Only exp is a library function."""
    f = np.float32
    one, two = f(1.0), f(2.0)
    v = np.asarray(means3D, dtype=f).astype(np.float64)
    t = np.asarray(transform, dtype=np.float64).reshape(3, 4)
    cast = None
    if normals is not None:
        nd = np.asarray(normals, dtype=np.float64)
        q = np.asarray(rotations, dtype=f)
        ls = np.asarray(log_scales, dtype=f)
        with np.errstate(all="ignore"):
            r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            qn = np.sqrt(((r * r + x * x) + y * y) + z * z)
            r, x, y, z = r / qn, x / qn, y / qn, z / qn
            R = [one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
                 two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
                 two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]
            c00, c01, c02 = R[4] * R[8] - R[5] * R[7], R[5] * R[6] - R[3] * R[8], R[3] * R[7] - R[4] * R[6]
            det = (R[0] * c00 + R[1] * c01) + R[2] * c02
            Ri = [c00 / det, (R[2] * R[7] - R[1] * R[8]) / det, (R[1] * R[5] - R[2] * R[4]) / det,
                  c01 / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[2] * R[3] - R[0] * R[5]) / det,
                  c02 / det, (R[1] * R[6] - R[0] * R[7]) / det, (R[0] * R[4] - R[1] * R[3]) / det]
            nf = nd.astype(f)
            acc = np.zeros(len(v), dtype=f)
            for a in range(3):
                nr = (Ri[3 * a] * nf[:, 0] + Ri[3 * a + 1] * nf[:, 1]) + Ri[3 * a + 2] * nf[:, 2]
                s = np.exp(ls[:, a])
                acc = acc + (nr * nr) / (s * s)
            cast = np.sqrt(one / acc)
            cast = np.where(np.isnan(cast), cast, np.minimum(np.maximum(cast, f(0.0)), f(0.001))).astype(f)
            v = v + cast.astype(np.float64)[:, None] * nd
    with np.errstate(all="ignore"):
        out = np.stack([((v[:, 0] * t[a, 0] + v[:, 1] * t[a, 1]) + v[:, 2] * t[a, 2]) + t[a, 3] for a in range(3)], axis=1)
    return out, cast


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
