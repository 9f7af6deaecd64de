"""Scenes of the projtex tests (tests/test_gpu_projtex.py; their CPU halves run without a GPU): packed views with a roll, a
meshrender.FaceObj of quads with one UV island each, and the float64 texel maps of a regular UV grid."""
from __future__ import annotations

import numpy as np

H, W = 40, 48                                  # images 48 x 40


def camera(eye, target, h=H, w=W, f=None, roll=0.0):
    """(world-to-camera 4x4, intrinsics 3x3) of a pinhole camera at `eye` looking at `target`, rolled by `roll` radians about its
    optical axis, principal point at the image centre"""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 1.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    x, y = np.cos(roll) * x + np.sin(roll) * y, -np.sin(roll) * x + np.cos(roll) * y
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([x, y, z])
    w2c[:3, 3] = -w2c[:3, :3] @ eye
    f = f or 1.2 * max(h, w)
    return w2c, np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]])


def view(eye, target, h=H, w=W, f=None, roll=0.0):
    """a packed view record (tests.test_meshrender_host.look_at_view's layout) of camera(...)"""
    from topo4d_amd.cameras import _clip_from_camera
    w2c, K = camera(eye, target, h, w, f, roll)
    clip = _clip_from_camera(w, h, K, 0.01, 100)
    rec = np.zeros(40, np.float32)
    rec[:16] = w2c.astype(np.float32).T.reshape(-1)
    rec[16:32] = (w2c.astype(np.float32).T @ clip.astype(np.float32).T).reshape(-1)
    return rec


def face_obj(quads, islands):
    """FaceObj of quads [n,4,3] (corner order gives the facing), quad k on the UV rectangle islands[k] = (u0, v0, u1, v1)"""
    from topo4d_amd.meshrender import FaceObj
    quads = np.asarray(quads, np.float64)
    uvs = []
    for u0, v0, u1, v1 in islands:
        uvs += [(u0, v0), (u0, v1), (u1, v1), (u1, v0)]
    idx = [list(range(4 * k, 4 * k + 4)) for k in range(len(quads))]
    return FaceObj(quads.reshape(-1, 3).astype(np.float32).astype(np.float64), np.asarray(uvs, np.float64), idx, [list(i) for i in idx])


def rect(x0, y0, x1, y1, z, dz=0.0, flip=False):
    """a quad facing -z (towards cameras at negative z; flip: +z), tilted by dz along x"""
    q = [(x0, y0, z), (x0, y1, z), (x1, y1, z + dz), (x1, y0, z + dz)]
    return q[::-1] if flip else q


def three_quads():
    """two overlapping quads (the second floats in front of the first's right half) and one that faces away"""
    quads = [rect(-1.0, -0.8, 0.4, 0.8, 0.0), rect(-0.2, -0.5, 1.0, 0.9, -0.35, dz=0.1), rect(-0.9, -0.9, -0.3, -0.2, -0.5, flip=True)]
    return face_obj(quads, [(0.04, 0.05, 0.46, 0.95), (0.54, 0.5, 0.96, 0.95), (0.54, 0.05, 0.96, 0.42)])


def three_views():
    """one off-axis, one rolled, one close"""
    return np.stack([view([0.9, 0.5, -2.6], [0.1, 0.0, 0.0], f=44.0), view([-0.3, -0.2, -2.4], [0.0, 0.1, 0.0], f=40.0, roll=0.6),
                     view([0.2, 0.1, -1.0], [0.1, 0.1, 0.0], f=30.0)])


def occlusion_scene():
    """(FaceObj, view) of the occlusion test.  Quad 0 is the large one: it lies inside the single camera's image, at least 3 px
    from its edges.  Quad 1 is the small one, 0.5 in front of it, over one of its corners, so that two sides of its shadow
    (about 15 px each) cross the large quad and the shadow holds well over 100 texels.  Quad 2 is a far backdrop that overfills
    the image, on a UV island of a few texels: without it the bilinear taps of the large quad's own outline would fall on the
    background, which rule 3 rejects and a ray cast knows nothing about."""
    quads = [rect(-1.0, -0.8, 1.0, 0.7, 0.0), rect(0.25, 0.04, 0.92, 0.67, -0.5), rect(-4.0, -3.5, 4.0, 3.5, 1.0)]
    islands = [(0.03, 0.03, 0.97, 0.8), (0.05, 0.86, 0.17, 0.96), (0.9, 0.9, 0.95, 0.95)]
    return face_obj(quads, islands), view([0.05, -0.03, -3.0], [0.0, 0.0, 0.0], f=60.0)


# ---- the round trip: a gently curved patch of 6 x 6 quads on a regular UV grid -----------------------------------------------
PATCH_N = 6
PATCH_UV = (0.1, 0.9)


def patch_scene():
    """(FaceObj, float64 vertices [49,3]) of z = 0.15 (x^2 + y^2) over [-1, 1]^2, facing -z, uv = the grid over PATCH_UV^2"""
    from topo4d_amd.meshrender import FaceObj
    n = PATCH_N
    g = np.linspace(-1.0, 1.0, n + 1)
    t = np.linspace(PATCH_UV[0], PATCH_UV[1], n + 1)
    verts = np.array([(x, y, 0.15 * (x * x + y * y)) for y in g for x in g], np.float32).astype(np.float64)
    uvs = np.array([(u, v) for v in t for u in t], np.float64)
    at = lambda i, j: j * (n + 1) + i
    faces = [[at(i, j), at(i, j + 1), at(i + 1, j + 1), at(i + 1, j)] for j in range(n) for i in range(n)]
    return FaceObj(verts, uvs, faces, [list(f) for f in faces]), verts


def patch_views(h=80, w=96):
    return np.stack([view([0.0, 0.0, -3.0], [0, 0, 0], h, w, f=105.0), view([1.2, 0.3, -2.8], [0, 0, 0], h, w, f=100.0),
                     view([-1.0, -0.5, -2.9], [0, 0, 0], h, w, f=100.0, roll=0.3)])


def smooth_texture(th: int, tw: int) -> np.ndarray:
    """float32 [th,tw,3]: f(u, v) at the texel centres, u = x / (tw - 1), v = (th - 1 - y) / (th - 1)"""
    y, x = np.mgrid[0:th, 0:tw].astype(np.float64)
    u, v = x / (tw - 1), (th - 1 - y) / (th - 1)
    rgb = np.stack([0.5 + 0.3 * np.sin(5.0 * u + 2.0 * v), 0.5 + 0.3 * np.cos(4.0 * v - 3.0 * u), 0.4 + 0.25 * np.sin(3.0 * (u + v) + 1.0)], -1)
    return rgb.astype(np.float32)


def vertex_normals64(verts, tris):
    """area-weighted vertex normals in float64 (what trimesh computes for a mesh without sharp corners, to rounding)"""
    n = np.zeros_like(verts)
    fn = np.cross(verts[tris[:, 1]] - verts[tris[:, 0]], verts[tris[:, 2]] - verts[tris[:, 0]])
    for k in range(3):
        np.add.at(n, tris[:, k], fn)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def patch_maps64(res: int):
    """(pos, nrm float64 [res,res,3], coverage bool) of patch_scene at res x res: each texel centre inside the UV grid takes the
    barycentric mix of its triangle's corners (the quad's fan (0,1,2), (0,2,3)), in float64"""
    from topo4d_amd.meshrender import triangulate
    obj, verts = patch_scene()
    tris, _ = triangulate(obj.faces_ori, obj.uv_faces_ori)
    normals = vertex_normals64(verts, tris)
    n = PATCH_N
    lo, hi = PATCH_UV[0] * (res - 1), PATCH_UV[1] * (res - 1)
    y, x = np.mgrid[0:res, 0:res].astype(np.float64)
    tx, ty = x, (res - 1) - y                                    # texel -> u (res - 1), v (res - 1)
    cov = (tx >= lo) & (tx <= hi) & (ty >= lo) & (ty <= hi)
    cell = (hi - lo) / n
    i = np.clip(np.floor((tx - lo) / cell), 0, n - 1).astype(np.int64)
    j = np.clip(np.floor((ty - lo) / cell), 0, n - 1).astype(np.int64)
    a, b = (tx - lo) / cell - i, (ty - lo) / cell - j           # in-cell coordinates along u and v
    at = lambda ii, jj: jj * (n + 1) + ii
    c0, c1, c2, c3 = at(i, j), at(i, j + 1), at(i + 1, j + 1), at(i + 1, j)
    upper = b >= a                                               # triangle (0,1,2) holds v >= u of the cell, (0,2,3) the rest
    out = []
    for attr in (verts, normals):
        t012 = attr[c0] * (1 - b)[..., None] + attr[c1] * (b - a)[..., None] + attr[c2] * a[..., None]
        t023 = attr[c0] * (1 - a)[..., None] + attr[c2] * b[..., None] + attr[c3] * (a - b)[..., None]
        out.append(np.where(upper[..., None], t012, t023))
    return out[0], out[1], cov


# ---- CPU stand-ins and the bookkeeping of the occlusion test -----------------------------------------------------------------
def quad_maps64(obj, th: int, tw: int):
    """(pos, nrm float64 [th,tw,3], coverage bool) of a face_obj() scene: its quads are parallelograms on UV rectangles, so the
    bake's interpolation is the affine map of the island"""
    pos, nrm, cov = np.zeros((th, tw, 3)), np.zeros((th, tw, 3)), np.zeros((th, tw), bool)
    y, x = np.mgrid[0:th, 0:tw].astype(np.float64)
    u, v = x / (tw - 1), (th - 1 - y) / (th - 1)
    for k in range(len(obj.faces_ori)):
        q, t = obj.vertices[4 * k:4 * k + 4], obj.uvs[4 * k:4 * k + 4]
        u0, v0, u1, v1 = t[0, 0], t[0, 1], t[2, 0], t[2, 1]
        inside = (u >= u0) & (u <= u1) & (v >= v0) & (v <= v1)
        a, b = (u - u0) / (u1 - u0), (v - v0) / (v1 - v0)
        p = q[0] + (q[3] - q[0]) * a[..., None] + (q[1] - q[0]) * b[..., None]
        pos[inside], nrm[inside] = p[inside], np.cross(q[1] - q[0], q[2] - q[0])
        cov |= inside
    return pos, nrm, cov


def _segment_distance(px, py, a, b):
    ab = b - a
    t = np.clip(((px - a[0]) * ab[0] + (py - a[1]) * ab[1]) / (ab @ ab), 0.0, 1.0)
    return np.hypot(px - (a[0] + t * ab[0]), py - (a[1] + t * ab[1]))


def occlusion_truth(points, obj, vw, h=H, w=W, margin=1.5):
    """(seen, in_image, excluded) of world points [n,3] in occlusion_scene: seen = the ray cast of
    projtex_ref.visible_brute_force; in_image = the projection lies inside the image; excluded = it lies within `margin` px of
    the front quad's silhouette or of the image edge"""
    from tests import meshrender_ref, projtex_ref
    from topo4d_amd.meshrender import triangulate
    tris, _ = triangulate(obj.faces_ori, obj.uv_faces_ori)
    px, py, _ = meshrender_ref.project(points, vw, h, w)
    edge = np.minimum(np.minimum(px, w - 1 - px), np.minimum(py, h - 1 - py))
    seen = projtex_ref.visible_brute_force(points, vw, obj.vertices, tris)
    fx, fy, _ = meshrender_ref.project(obj.vertices[4:8], vw, h, w)
    corners = np.stack([fx, fy], 1)
    dist = np.min([_segment_distance(px, py, corners[k], corners[(k + 1) % 4]) for k in range(4)], axis=0)
    return seen, edge >= 0, (dist <= margin) | (np.abs(edge) <= margin)


def erode(cov, rounds: int):
    """texfinish.erode on the host: a texel stays if it and its 4-neighbours inside the image are covered"""
    c = np.asarray(cov, bool)
    for _ in range(rounds):
        p = np.pad(c, 1, constant_values=True)
        c = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return c
