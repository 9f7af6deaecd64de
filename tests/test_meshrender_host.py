"""CPU: the face.obj reader and triangulation of topo4d_amd.meshrender on golden G14 (the reference's own save_mesh files) and
on malformed files, and the float64 yardstick of the mesh render (tests/meshrender_ref.py) against an independent ray-triangle
intersection and on the top-left rule.  No device is needed."""
import os

import numpy as np
import pytest

from tests import meshrender_ref as ref
from topo4d_amd import meshrender

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G14 = os.path.join(ROOT, "tests", "golden", "g14_save_mesh.npz")


def _unflat(lens, flat):
    out, i = [], 0
    for n in lens.astype(int):
        out.append([int(v) for v in flat[i:i + n]])
        i += n
    return out


@pytest.mark.parametrize("name", ["quad", "quad_b", "special"])
@pytest.mark.parametrize("frame", [1, 2])
def test_read_face_obj_reads_save_mesh_files(tmp_path, name, frame):
    g = np.load(G14)
    path = tmp_path / "face.obj"
    path.write_bytes(g[f"{name}/obj_frame{frame}"].tobytes())
    obj = meshrender.read_face_obj(str(path))
    assert np.array_equal(obj.vertices, g[f"{name}/vertices_frame{frame}"])
    assert np.array_equal(obj.uvs, g[f"{name}/uvs_ori"])
    lens = g[f"{name}/face_lens"]
    assert obj.faces_ori == _unflat(lens, g[f"{name}/faces_ori"])
    assert obj.uv_faces_ori == _unflat(lens, g[f"{name}/uv_faces_ori"])
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    assert faces.dtype == np.int32 and faces.shape == uv_faces.shape
    assert np.array_equal(faces, g[f"{name}/faces"])          # helpers.triangulate_faces of the same polygons


@pytest.mark.parametrize("text, what", [
    ("v 0 0 0\nv 1 0 0\nvt 0 0\nf 1/1 2/1 3/1\n", "vertex index 3"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/2 3/1\n", "texture coordinate index 2"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1 2 3\n", "not v/vt"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1//1 2/1 3/1\n", "not v/vt"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 0/1 2/1 3/1\n", "vertex index 0"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nf 1/1 2/1\n", "2 corners"),
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\n", "no faces"),
    ("v 0 0\nvt 0 0\nf 1/1 1/1 1/1\n", "'v' line"),
])
def test_read_face_obj_rejects_malformed_files(tmp_path, text, what):
    path = tmp_path / "bad.obj"
    path.write_text(text)
    with pytest.raises(ValueError, match=what):
        meshrender.read_face_obj(str(path))


def test_triangulate_fans_quads_and_checks_lengths():
    faces, uv = meshrender.triangulate([[0, 1, 2, 3], [4, 5, 6]], [[10, 11, 12, 13], [14, 15, 16]])
    assert faces.tolist() == [[0, 1, 2], [0, 2, 3], [4, 5, 6]]
    assert uv.tolist() == [[10, 11, 12], [10, 12, 13], [14, 15, 16]]
    with pytest.raises(ValueError):
        meshrender.triangulate([[0, 1, 2, 3]], [[0, 1, 2]])
    with pytest.raises(ValueError):
        meshrender.triangulate([[0, 1, 2, 3, 4]], [[0, 1, 2, 3, 4]])
    with pytest.raises(ValueError):
        meshrender.triangulate([[0, 1, 2]], [])


def test_renderer_has_no_cpu_path():
    with pytest.raises(ValueError):
        meshrender.MeshRenderer(np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), np.zeros((1, 2)), np.zeros((2, 2, 3), np.uint8),
                                device="cpu")
    import torch
    with pytest.raises(ValueError):
        meshrender.image_metrics(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))


# ---- the yardstick against an independent ray cast ----------------------------------------------------------------------------
def look_at_view(eye, target, H, W, f=None):
    """a packed view record (viewmatrix, projmatrix as setup_camera lays them out) of a pinhole camera at `eye`"""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 1.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    w2c = np.eye(4)
    w2c[:3, :3] = np.stack([x, y, z])
    w2c[:3, 3] = -w2c[:3, :3] @ eye
    f = f or 1.2 * max(H, W)
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]])
    from topo4d_amd.cameras import _clip_from_camera
    clip = _clip_from_camera(W, H, K, 0.01, 100).astype(np.float64)
    view = np.zeros(40, np.float32)
    view[:16] = w2c.astype(np.float32).T.reshape(-1)
    view[16:32] = (w2c.astype(np.float32).T @ clip.astype(np.float32).T).reshape(-1)
    return view


def _ray_cast(vertices, tris, uvs_c, view, H, W):
    """per pixel: (face, view depth, uv) of the nearest hit by Moller-Trumbore in the world frame, on the ray of the pixel centre
    through the same float32 matrices: the two planes clip.x = ndc_x clip.w and clip.y = ndc_y clip.w meet in it"""
    v64 = np.asarray(vertices, np.float32).astype(np.float64)
    vm = view[:16].astype(np.float64).reshape(4, 4).T
    P = view[16:32].astype(np.float64).reshape(4, 4).T
    eye = np.linalg.solve(P[[0, 1, 3], :3], -P[[0, 1, 3], 3])
    ys, xs = np.mgrid[0:H, 0:W]
    ndc_x, ndc_y = (2.0 * xs + 1.0) / W - 1.0, (2.0 * ys + 1.0) / H - 1.0
    n1 = P[0, :3][None, None] - ndc_x[..., None] * P[3, :3]
    n2 = P[1, :3][None, None] - ndc_y[..., None] * P[3, :3]
    d = np.cross(n1, n2)
    d *= np.sign(d @ P[3, :3])[..., None]                              # towards clip.w > 0: in front of the camera
    face = np.full((H, W), -1)
    t_best = np.full((H, W), np.inf)
    uv = np.zeros((H, W, 2))
    for f, (i0, i1, i2) in enumerate(tris):
        p0, p1, p2 = v64[i0], v64[i1], v64[i2]
        e1, e2 = p1 - p0, p2 - p0
        h = np.cross(d, e2)
        det = h @ e1
        s = eye - p0
        q = np.cross(s, e1)
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            bu = (h @ s) * inv
            bv = (d @ q) * inv
            t = (q @ e2) * inv
        ok = (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0) & np.isfinite(t)
        better = ok & (t < t_best)
        t_best = np.where(better, t, t_best)
        face = np.where(better, f, face)
        uvp = (1 - bu - bv)[..., None] * uvs_c[f, 0] + bu[..., None] * uvs_c[f, 1] + bv[..., None] * uvs_c[f, 2]
        uv = np.where(better[..., None], uvp, uv)
    hit = eye[None, None] + t_best[..., None] * d
    depth = hit @ vm[2, :3] + vm[2, 3]
    return face, depth, uv


def _random_mesh(rng, n_tri, spread=0.6, scale=0.25):
    centres = rng.uniform(-spread, spread, size=(n_tri, 3))
    verts = (centres[:, None, :] + rng.normal(scale=scale, size=(n_tri, 3, 3))).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * n_tri).reshape(-1, 3)
    uvs = rng.uniform(0, 1, size=(3 * n_tri, 2)).astype(np.float32)
    return verts, tris, uvs


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_yardstick_matches_a_ray_cast(seed):
    """where the ray cast and the yardstick pick the same triangle, depth and UV agree to 1e-9; they pick the same one almost
    everywhere (pixels on an edge or at a depth tie may go either way)"""
    rng = np.random.default_rng(seed)
    H, W = 23, 31
    verts, tris, uvs = _random_mesh(rng, 24, scale=0.8)
    view = look_at_view([0.3, -0.2, -2.0], [0, 0, 0], H, W, f=0.9 * W)
    sx, sy, sz = ref.project(verts, view, H, W)
    key = ref.raster_screen(sx, sy, sz, tris, H, W)
    face_rc, depth_rc, uv_rc = _ray_cast(verts, tris, uvs[tris].astype(np.float64), view, H, W)
    hit = key != np.uint64(0xFFFFFFFFFFFFFFFF)
    face = np.where(hit, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    assert hit.sum() > 0.2 * H * W
    same = face == face_rc
    assert same.mean() > 0.97
    ys, xs = np.nonzero(same & hit)
    for y, x in zip(ys, xs):
        i = tris[face[y, x]]
        A, _, owns = ref.setup(sx[i], sy[i], sz[i], H, W)
        inside, q, S = ref.eval_pixels(sx[i], sy[i], sz[i], A, owns, np.array([float(x)]), np.array([float(y)]))
        assert inside[0]
        depth = 1.0 / S[0]
        uv = sum((q[j][0] / S[0]) * uvs[i[j]].astype(np.float64) for j in range(3))
        assert abs(depth - depth_rc[y, x]) <= 1e-9 * abs(depth), (y, x)
        assert np.abs(uv - uv_rc[y, x]).max() <= 1e-9, (y, x)


def _fan(cx, cy, n, r, rng):
    """rim of a star-shaped fan around (cx, cy): n points at jittered angles (every gap below pi) and radii"""
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False) + rng.uniform(-0.3, 0.3, n) * 2 * np.pi / n
    rad = r * rng.uniform(0.8, 1.0, n)
    return np.c_[cx + rad * np.cos(ang), cy + rad * np.sin(ang)]


@pytest.mark.parametrize("exact", [True, False])
def test_top_left_rule_covers_a_closed_fan_once(exact):
    """no pixel covered twice, none dropped inside a closed fan: on a lattice where edges run through pixel centres (exact
    zeros everywhere) and on random float fans"""
    H = W = 40
    rng = np.random.default_rng(5)
    for trial in range(6):
        if exact:
            rim = np.array([[5, 5], [20, 3], [35, 5], [36, 20], [35, 35], [20, 37], [5, 35], [3, 20]], float)
            c = np.array([20.0, 20.0]) if trial % 2 == 0 else np.array([18.0, 21.0])
            rim = rim[::-1] if trial >= 3 else rim                        # both windings
        else:
            c = rng.uniform(15, 25, 2)
            rim = _fan(c[0], c[1], 7 + trial, 14.0, rng)
        n = len(rim)
        sx = np.r_[c[0], rim[:, 0]]
        sy = np.r_[c[1], rim[:, 1]]
        sz = np.full(n + 1, 2.0)
        count = np.zeros((H, W), int)
        for k in range(n):
            tri = [0, 1 + k, 1 + (k + 1) % n]
            key = ref.raster_screen(sx, sy, sz, [tri], H, W)
            count += key != np.uint64(0xFFFFFFFFFFFFFFFF)
        assert count.max() == 1, "a pixel covered twice"
        # every pixel strictly inside the rim polygon (convex here) is covered
        ys, xs = np.mgrid[0:H, 0:W]
        inside = np.ones((H, W), bool)
        sgn = np.sign(np.cross(rim[1] - rim[0], rim[2] - rim[0]))
        for k in range(n):
            a, b = rim[k], rim[(k + 1) % n]
            e = (b[0] - a[0]) * (ys - a[1]) - (b[1] - a[1]) * (xs - a[0])
            inside &= sgn * e > 0
        assert (count[inside] == 1).all(), "a pixel inside the fan dropped"


def test_degenerate_and_near_plane_triangles_are_dropped():
    H, W = 8, 8
    sx = np.array([1.0, 6.0, 3.5, 1.0, 6.0, 1.0])
    sy = np.array([1.0, 1.0, 6.0, 1.0, 1.0, 1.0])
    assert ref.setup(sx[[0, 1, 2]], sy[[0, 1, 2]], np.array([1.0, 1.0, 1.0]), H, W) is not None
    assert ref.setup(sx[[0, 1, 2]], sy[[0, 1, 2]], np.array([1.0, 0.01, 1.0]), H, W) is None       # z <= 0.01
    assert ref.setup(sx[[3, 4, 5]], sy[[3, 4, 5]], np.array([1.0, 1.0, 1.0]), H, W) is None       # zero area
