"""
TEST INFRASTRUCTURE.  Writes tests/golden/g15_coarse_setup.npz by calling the REAL reference's train.initialize_params
(gen_tex=False) and train.initialize_losses through oracle/gen_golden.py's import stubs.  Runs only where the reference tree
exists.  The fixture holds the scene's files as bytes, the facial_regions arrays and what the reference built.

    python tools/gen_golden_setup.py

Stubs (the packages are not dependencies here):
  pywavefront.Wavefront  a plain reader of the fixture OBJ written below (v / vt / vn / f v/vt/vn, quads fanned (0,1,2), (0,2,3),
                         one material whose map_Kd is the texture), exposing .vertices, .parser.tex_coords, .meshes and
                         materials[0].vertices in T2F_N3F_V3F order - what the reference reads of pywavefront 1.3.3
  trimesh.Trimesh        .vertices (float64) and .vertex_normals = tests/objexport_ref.trimesh_vertex_normals (no merging)
  o3d_knn                exact brute force (ascending squared distances, the point itself dropped)
  Tensor.cuda            a no-op (the reference runs on the CPU here)
Everything else - compute_vertex_colors and its PIL sampling, build_quaterion, find_adjacent_vertices, the neighbour loop, the
dense half, FlattenLoss / SoftFlattenLoss / FlattenLoss_v2 and the region weights - is the reference's own code.

The scene: a 90 x 92 grid of 8,280 vertices on a head-sized surface (so that the real facial_regions.pkl arrays index it),
odd grid rows numbered backwards; quads with about a third split into two triangles, faces shuffled within runs of 32, corners rotated; a UV seam column
(faces right of it use u + 1: the `% 1` path, 2 UVs per seam vertex) and a half-row seam (v - 1: negative UVs; 3 UVs where the
two meet); two neighbouring vertices made coincident (weight 1 -> 0); texture: a 64 x 48 baseline JPEG (4:2:0) and an RGBA PNG of
its PIL-decoded pixels.  UVs stay inside [0.01, 0.99] modulo 1, where getpixel does not raise.

Size: neighbor_dist, neighbor_weight, iso_w, rig_w, rot_w, means3D, log_scales and init_scale are stored as sha256 digests of
their bytes, with neighbor_weight also for a seeded sample of rows; the OBJ text is xz-compressed; unnorm_rotations is stored for 2,048 seeded rows; edge terms store v0s delta-coded
and v1s..v3s as slots of v0's sorted face neighbours in the term's own faces.
tests/test_setup_host.py:golden decodes the file.
"""
import hashlib
import io
import lzma
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden  # noqa: E402
from tests import objexport_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g15_coarse_setup.npz")
ROWS, COLS = 90, 92
TEX_W, TEX_H = 64, 48
SEAM_J, SEAM_I = 45, 40
TRANS_G = np.array([[0.9, -0.1, 0.05, 0.01], [0.1, 0.95, 0.0, -0.02], [-0.05, 0.02, 1.1, 0.3], [0, 0, 0, 1]], np.float64)


FACE_KEYS = {"flat": "flat_faces", "flat_lip_bottom": "lip_bottom_flat_faces", "flat_lip": "lip_flat_faces",
             "flat_mouth": "mouth_flat_faces", "flat_lid_top": "lid_top_flat_faces", "flat_lid_bottom": "lid_bottom_flat_faces"}


def face_adjacency(faces, n):
    """Per vertex the sorted other corners of the faces holding it (the decoder's table for v1s..v3s)."""
    adj = [set() for _ in range(n)]
    for f in np.asarray(faces).tolist():
        for a in f:
            adj[a].update(b for b in f if b != a)
    return [sorted(s) for s in adj]


def sha(a) -> np.ndarray:
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def scene(rng):
    """(obj text, mtl text, jpeg bytes, png bytes)."""
    from PIL import Image
    n = ROWS * COLS
    perm = np.arange(n).reshape(ROWS, COLS)                        # grid id -> vertex number: odd rows numbered backwards
    perm[1::2] = perm[1::2, ::-1]
    perm = perm.reshape(-1)
    ii, jj = np.meshgrid(np.arange(ROWS), np.arange(COLS), indexing="ij")
    th, ph = 0.3 + 2.0 * ii / ROWS, -1.2 + 2.4 * jj / COLS
    pos = np.stack([0.09 * np.sin(th) * np.sin(ph), 0.12 * np.cos(th), 0.10 * np.sin(th) * np.cos(ph)], -1).reshape(-1, 3)
    pos += rng.normal(scale=3e-4, size=pos.shape)
    pos = np.round(pos, 4)
    a, b = 30 * COLS + 10, 30 * COLS + 11                          # two neighbouring grid vertices made coincident
    pos[b] = pos[a]
    verts = np.empty_like(pos)
    verts[perm] = pos
    # UVs: one per grid vertex, plus the seam copies
    u = np.round(0.01 + 0.98 * jj / (COLS - 1), 6).reshape(-1)
    v = np.round(0.01 + 0.98 * ii / (ROWS - 1), 6).reshape(-1)
    uvs = [(float(x), float(y)) for x, y in zip(u, v)]
    seam_u, seam_v = {}, {}

    def uv_index(g, right, below):
        if right and g % COLS == SEAM_J:
            if g not in seam_u:
                seam_u[g] = len(uvs)
                uvs.append((float(u[g]) + 1.0, float(v[g])))
            return seam_u[g]
        if below and g // COLS == SEAM_I and g % COLS <= SEAM_J:
            if g not in seam_v:
                seam_v[g] = len(uvs)
                uvs.append((float(u[g]), float(v[g]) - 1.0))
            return seam_v[g]
        return g

    faces = []
    for i in range(ROWS - 1):
        for j in range(COLS - 1):
            grid = [i * COLS + j, (i + 1) * COLS + j, (i + 1) * COLS + j + 1, i * COLS + j + 1]
            right, below = j >= SEAM_J, i < SEAM_I and j < SEAM_J
            tex = [uv_index(g, right, below) for g in grid]
            corners = list(zip([int(perm[g]) for g in grid], tex))
            r = rng.integers(4)
            corners = corners[r:] + corners[:r]
            if rng.random() < 0.35:
                faces.append(corners[:3])
                faces.append([corners[0], corners[2], corners[3]])
            else:
                faces.append(corners)
    order = np.concatenate([s + rng.permutation(min(32, len(faces) - s)) for s in range(0, len(faces), 32)])   # shuffled in runs of 32
    normals = ["vn 0 0 1"]
    lines = ["# G15 coarse-setup scene", "mtllib face.mtl", "o face"]
    lines += [f"v {x!r} {y!r} {z!r}" for x, y, z in verts.tolist()]
    lines += [f"vt {x!r} {y!r}" for x, y in uvs]
    lines += normals + ["usemtl face", "s 1"]
    lines += ["f " + " ".join(f"{vi + 1}/{ti + 1}/1" for vi, ti in faces[k]) for k in order]
    obj = "\n".join(lines) + "\n"
    mtl = "newmtl face\nKd 1.0 1.0 1.0\nmap_Kd texture.jpg\n"
    yy, xx = np.meshgrid(np.arange(TEX_H), np.arange(TEX_W), indexing="ij")
    img = np.stack([(xx * 4) % 256, (yy * 5) % 256, ((xx + yy) * 3) % 256], -1).astype(np.uint8)
    img = np.clip(img.astype(np.int32) + rng.integers(-20, 21, img.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", quality=90, subsampling=2)
    jpeg = buf.getvalue()
    decoded = np.asarray(Image.open(io.BytesIO(jpeg)))
    rgba = np.concatenate([decoded, rng.integers(0, 256, decoded.shape[:2] + (1,)).astype(np.uint8)], -1)
    buf = io.BytesIO()
    Image.fromarray(rgba, "RGBA").save(buf, format="PNG")
    return obj, mtl, jpeg, buf.getvalue()


class _Wavefront:
    """pywavefront.Wavefront(path, collect_faces=True) for the fixture's OBJ (see the module docstring)."""

    def __init__(self, path, collect_faces=True, **_):
        self.vertices, tex, tri = [], [], []
        mtl = None
        for line in open(path):
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                self.vertices.append(tuple(float(x) for x in p[1:4]))
            elif p[0] == "vt":
                tex.append((float(p[1]), float(p[2])))
            elif p[0] == "mtllib":
                mtl = p[1]
            elif p[0] == "f":
                c = [tuple(int(x) - 1 for x in s.split("/")) for s in p[1:]]
                for k in range(2, len(c)):
                    tri.append((c[0], c[k - 1], c[k]))
        self.parser = types.SimpleNamespace(tex_coords=tex)
        texpath = None
        for line in open(os.path.join(os.path.dirname(path), mtl)):
            if line.startswith("map_Kd"):
                texpath = os.path.join(os.path.dirname(path), line.split()[1])
        flat = []
        for t in tri:
            for (vi, ti, _) in t:
                flat += [tex[ti][0], tex[ti][1], 0.0, 0.0, 1.0] + list(self.vertices[vi])
        material = types.SimpleNamespace(vertices=flat, texture=types.SimpleNamespace(_path=texpath))
        mesh = types.SimpleNamespace(faces=[[vi for (vi, _, _) in t] for t in tri], materials=[material])
        self.meshes = {"face": mesh}


class _Trimesh:
    def __init__(self, vertices=None, faces=None, **_):
        self.vertices = np.asarray(vertices, np.float64)
        self.faces = np.asarray(faces, np.int64)

    @property
    def vertex_normals(self):
        return objexport_ref.trimesh_vertex_normals(self.vertices, self.faces)


def _o3d_knn(pts, num_knn):
    pts = np.asarray(pts, np.float64)
    d_all, i_all = [], []
    for s in range(0, len(pts), 512):
        q = pts[s:s + 512]
        dx, dy, dz = (q[:, None, k] - pts[None, :, k] for k in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        idx = np.argsort(d, axis=1, kind="stable")[:, :num_knn + 1]
        d_all.append(np.take_along_axis(d, idx, 1)[:, 1:])
        i_all.append(idx[:, 1:])
    return np.concatenate(d_all), np.concatenate(i_all)


def main():
    gen_golden.import_reference_helpers()
    sys.modules["pywavefront"].Wavefront = _Wavefront
    sys.modules["trimesh"].Trimesh = _Trimesh
    train = gen_golden.import_reference_train()
    train.o3d_knn = _o3d_knn
    torch.Tensor.cuda = lambda self, *a, **k: self
    rng = np.random.default_rng(15)
    obj, mtl, jpeg, png = scene(rng)
    with open(os.path.join(gen_golden.REF, "assets", "facial_regions.pkl"), "rb") as f:
        fr = pickle.load(f)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "seq"))
        for name, data in (("face_v5.obj", obj.encode()), ("face.mtl", mtl.encode()), ("texture.jpg", jpeg)):
            open(os.path.join(tmp, "seq", name), "wb").write(data)
        args = types.SimpleNamespace(input_dir=tmp, seq="seq", gen_tex=False, density=1)
        cwd = os.getcwd()
        os.chdir(gen_golden.REF)                                      # ./assets/facial_regions.pkl
        try:
            params, variables = train.initialize_params(args, TRANS_G)
            variables, losses, lw, lwd = train.initialize_losses(variables)
            colors_jpeg = train.compute_vertex_colors(_Wavefront(os.path.join(tmp, "seq", "face_v5.obj")))
            open(os.path.join(tmp, "seq", "texture.jpg"), "wb").write(png)     # the RGBA PNG under the same name
            colors_png = train.compute_vertex_colors(_Wavefront(os.path.join(tmp, "seq", "face_v5.obj")))
        finally:
            os.chdir(cwd)
    assert np.array_equal(colors_jpeg, colors_png)
    P = params["means3D"].shape[0]
    f32 = lambda k: params[k].detach().numpy()
    out["obj_xz"] = np.frombuffer(lzma.compress(obj.encode(), preset=9 | lzma.PRESET_EXTREME), np.uint8)
    out["mtl"] = np.frombuffer(mtl.encode(), np.uint8)
    out["jpeg"] = np.frombuffer(jpeg, np.uint8)
    out["png_rgba"] = np.frombuffer(png, np.uint8)
    out["trans_g"] = TRANS_G
    for k, a in fr.items():                                           # int32 on disk; fr_int64_keys says which to widen back
        if k == "region_masks":
            for r, m in a.items():
                out[f"fr_region_masks__{r}"] = np.asarray(m, np.int32)
        else:
            out[f"fr_{k}"] = np.asarray(a, np.int32)
    out["fr_int64_keys"] = np.array([k for k, a in fr.items() if k != "region_masks" and np.asarray(a).dtype == np.int64])
    out["fr_list_keys"] = np.array([k for k, a in fr.items() if isinstance(a, list)])
    out["colors"] = colors_jpeg.astype(np.uint8)
    out["uv_counts"] = np.array([len(x) for x in variables["uvs_texture_ori"]], np.uint8)
    qrows = np.sort(rng.choice(P, 2048, replace=False)).astype(np.int32)
    out["unnorm_rotations_rows"] = qrows
    out["unnorm_rotations_sample"] = f32("unnorm_rotations")[qrows]
    for k in ("means3D", "rgb_colors", "log_scales"):
        out[f"{k}_sha256"] = sha(f32(k))
    out["init_scale_sha256"] = sha(variables["init_scale"].numpy())
    nbr = variables["neighbor_indices"].numpy()
    out["neighbor_indices_delta"] = (nbr - np.arange(P)[:, None]).astype(np.int16)
    for k in ("neighbor_weight", "neighbor_dist", "iso_w", "rig_w", "rot_w"):
        out[f"{k}_sha256"] = sha(variables[k].numpy())
    rows = np.sort(rng.choice(P, 256, replace=False)).astype(np.int32)
    out["sample_rows"] = rows
    out["neighbor_weight_sample"] = variables["neighbor_weight"].numpy()[rows]
    for name, obj_ in losses.items():
        if hasattr(obj_, "v0s"):
            v = [getattr(obj_, s).numpy() for s in ("v0s", "v1s", "v2s", "v3s")]
            adj = face_adjacency(fr[FACE_KEYS[name]], P)
            out[f"{name}_v0_delta"] = np.diff(v[0], prepend=0).astype(np.int16)
            out[f"{name}_slots"] = np.stack([[adj[a].index(b) for a, b in zip(v[0].tolist(), o.tolist())] for o in v[1:]]).astype(np.uint8)
        else:
            out[f"{name}_region"] = np.asarray(obj_.region_mask.numpy(), np.int16)
            out["neighbor_num"] = obj_.neighbor_num.numpy().astype(np.uint8)
            out["region_mask_K"] = np.int32(obj_.mask.shape[1])
    out["losses_weights"] = np.array([lw[k] for k in lw])
    out["losses_weights_names"] = np.array(list(lw))
    np.savez_compressed(OUT, **out)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests.test_setup_host import golden
    g = golden()
    for k in ("v0s", "v1s", "v2s", "v3s"):
        assert np.array_equal(g["edges"]["flat"][k], losses["flat"].__getattr__(k).numpy())
    assert np.array_equal(g["neighbor_indices"], nbr)
    print(OUT, os.path.getsize(OUT), "bytes; P", P, "K", nbr.shape[1], "faces", len(variables["faces_ori"]),
          "uvs", len(variables["uvs_ori"]), {k: v.shape for k, v in out.items() if v.ndim and v.size > 1000})


if __name__ == "__main__":
    main()
