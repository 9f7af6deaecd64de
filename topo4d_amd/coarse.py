"""
The start of a Topo4D run on the GPU: the coarse half of `initialize_params` (train.py:115-206) and `initialize_losses`
(train.py:511-587) with the loss_util constructors it calls, over csrc/t4d_setup.hip (include/topo4d_raster.h).  Nothing here
needs pywavefront, trimesh, open3d or loss_util.

    read_obj(path)                       the OBJ / MTL as pywavefront 1.3.3 and helpers.load_faces_vertices read it (host)
    vertex_colors(texture, mesh)         compute_vertex_colors (helpers.py:181-209, 300-333)          t4d_setup_vertex_colors
    vertex_uvs(mesh)                     get_vertex_uvs (helpers.py:212-234)                          host, CPython set order
    one_ring(faces_ori, n_vert)          find_adjacent_vertices (helpers.py:670-688) + the padding of train.py:168-176 (host)
    neighbor_priors(means3D, nbr, eye)   the distance / weight loop of train.py:177-206                t4d_setup_one_ring
    rotations_from_normals(normals)      external.build_quaterion (external.py:45-61) in float32       t4d_setup_quaternions
    region_weights(w, regions, weights)  iso_w / rig_w / rot_w (train.py:545-581)                      t4d_setup_region_weights
    flatten_edges(faces)                 the FlattenLoss / SoftFlattenLoss constructors (loss_util.py:114-170, 262-318)
                                         host candidate edges in the reference's set order, device faces per edge and compaction
    region_topology(...)                 the FlattenLoss_v2 constructor (loss_util.py:223-255)         t4d_setup_neighbor_mask
    initialize_params(args, trans_g)     train.py:115-269 (the dense half through densify.init_dense_gaussians)
    initialize_losses(variables)         train.py:511-587

Exactness: every array equals the reference's bit for bit on golden G15, except unnorm_rotations, which is within
2 float32 ulp or 1e-6 of it: the reference evaluates acos / sin / cos with CPU torch, the device with its own float32 functions.
neighbor_weight goes through a float64 exp that, like numpy's, is not correctly rounded: off the golden scene it may differ by
one float32 ulp.  The host parts (set orders) run the reference's own expressions over CPython's set, so their order is the
reference's by construction.  There is no CPU path for the device parts.
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import ptr

MAX_CAMS = 24

# train.py:514-535: the FlattenLoss / SoftFlattenLoss terms and their facial_regions face arrays; LOSS_ORDER: the dict's order
FLAT_EDGE_TERMS = {"flat": "flat_faces", "flat_lip_bottom": "lip_bottom_flat_faces", "flat_lip": "lip_flat_faces",
                   "flat_mouth": "mouth_flat_faces", "flat_lid_top": "lid_top_flat_faces", "flat_lid_bottom": "lid_bottom_flat_faces"}
LOSS_ORDER = ("flat", "flat_lip_bottom", "flat_eye", "flat_lip_socket", "flat_face_bottom", "flat_lip", "flat_mouth", "flat_lid_top",
              "flat_lid_bottom")
LOSSES_WEIGHTS = {'im': 1.0, 'rigid': 3.5, 'rot': 20.0, 'iso': 20.0,
                  'flat': 2e-4, 'flat_lip_bottom': 2e-4,
                  'flat_lid_top': 2e-4, 'flat_lid_bottom': 1e-2, 'flat_lip': 1e-4, 'flat_mouth': 1e-3,
                  'flat_eye': 1e4, 'flat_face_bottom': 1e3, 'flat_lip_socket': 1e3,
                  'scale': 10.0, 'scale_max': 10.0}
LOSSES_WEIGHTS_DENSE = {'im': 1.0, 'soft_color': 0.02}
# train.py:545-581: per weight array, its losses_weights key and the ordered (mask, factor c) list; a mask is a facial_regions key
# or ("region_masks", name)
_R = lambda name: ("region_masks", name)
REGION_WEIGHT_BLOCKS = {
    "iso_w": ("iso", [("eye_lid_up_masks", 0.0), (_R("EyeLidOuterTop"), 0.0), (_R("EyeLidTop"), 0.0), ("mouth_inner_masks", 5.0),
                      (_R("Chin"), 0.0), (_R("LipOuterTop"), 0.0), (_R("LipOuterBottom"), 1.0), (_R("EyeSocket"), 0.0),
                      (_R("MouthSocket"), 0.0), (_R("NeckFront"), 0.0), ("face_flat_masks", 0.0)]),
    "rig_w": ("rigid", [("eye_lid_up_masks", 0.0), (_R("EyeLidOuterTop"), 0.0), (_R("EyeLidTop"), 0.0), ("mouth_inner_masks", 0.5),
                        (_R("Chin"), 0.0), (_R("LipOuterTop"), 0.0), (_R("LipOuterBottom"), 0.1), (_R("MouthSocket"), 0.0),
                        (_R("EyeSocket"), 0.0), (_R("NeckFront"), 0.0), ("face_flat_masks", 0.0)]),
    "rot_w": ("rot", [(_R("EyeLidOuterTop"), 50.0), (_R("EyeLidTop"), 50.0), (_R("EyeLidBottom"), 100.0), (_R("EyeSocket"), 100.0),
                      ("eye_inner_masks", 100.0)]),
}


_WHAT = "the coarse setup"


def _status(t: torch.Tensor) -> List[int]:
    return [int(v) for v in t.cpu()]


# ---- the OBJ ---------------------------------------------------------------------------------------------------------------
@dataclass
class ObjMesh:
    """What the reference reads from face_v5.obj.  vertices float64 [N,3] (scene.vertices); tex_coords float64 [T,2]
    (scene.parser.tex_coords); faces_ori / uv_faces_ori: 0-based polygons (load_faces_vertices); faces / uv_faces int64 [F,3]: the
    triangulation (0,1,2), (0,2,3) of every quad (mesh.faces, triangulate_faces); corner_uvs float64 [F*3,2]: the UV of
    triangle corner 3*f+k (the T2F part of materials[0].vertices at f*24+k*8); texture: map_Kd, relative to the .mtl (None:
    no material)."""
    vertices: np.ndarray
    tex_coords: np.ndarray
    faces_ori: list
    uv_faces_ori: list
    faces: np.ndarray
    uv_faces: np.ndarray
    corner_uvs: np.ndarray
    texture: Optional[str]


def _read_mtl(path: str) -> Optional[str]:
    texture = None
    with open(path, "r") as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 2 and parts[0] == "map_Kd":
                texture = os.path.join(os.path.dirname(path), line.strip()[len("map_Kd"):].strip())
                break
    return texture


def read_obj(path: str) -> ObjMesh:
    """Read an OBJ as the reference does through pywavefront 1.3.3 (collect_faces=True, T2F_N3F_V3F) and load_faces_vertices
    (helpers.py:336-358).  pywavefront is not a dependency: its behaviour for the files Topo4D reads is restated here - "v",
    "vt" (u, v; a third value ignored) and "f" lines with v/vt/vn corners, polygons fanned from corner 0, one material whose
    map_Kd names the texture.  ValueError where the reference would break or silently misalign: a corner without a vt or vn
    index (the reference hard-codes the 8-float stride), a negative or out-of-range index, a polygon of more than 4 corners,
    a "v" line with more than 3 values (vertex colours change pywavefront's layout), and a vertex no face references
    (compute_vertex_colors would return a shorter array)."""
    verts, uvs, n_normals = [], [], 0
    faces_ori, uv_faces_ori = [], []
    mtllib = None
    with open(path, "r") as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            tag = parts[0]
            if tag == "v":
                if len(parts) != 4:
                    raise ValueError(f"{path}:{lineno}: a 'v' line with {len(parts) - 1} values (need exactly 3)")
                verts.append((float(parts[1]), float(parts[2]), float(parts[3])))
            elif tag == "vt":
                if len(parts) < 3:
                    raise ValueError(f"{path}:{lineno}: a 'vt' line needs u and v")
                uvs.append((float(parts[1]), float(parts[2])))
            elif tag == "vn":
                n_normals += 1
            elif tag == "f":
                corners = parts[1:]
                if not 3 <= len(corners) <= 4:
                    raise ValueError(f"{path}:{lineno}: a face of {len(corners)} corners (the reference takes triangles and quads)")
                fv, ft = [], []
                for c in corners:
                    idx = c.split("/")
                    if len(idx) != 3 or not all(idx):
                        raise ValueError(f"{path}:{lineno}: corner '{c}' is not v/vt/vn (the reference reads a T2F_N3F_V3F layout)")
                    iv, it, iN = (int(s) for s in idx)
                    if min(iv, it, iN) < 1:
                        raise ValueError(f"{path}:{lineno}: corner '{c}' has a non-positive index")
                    fv.append(iv - 1)
                    ft.append(it - 1)
                    if iN > n_normals:
                        raise ValueError(f"{path}:{lineno}: corner '{c}' names normal {iN} of {n_normals}")
                faces_ori.append(fv)
                uv_faces_ori.append(ft)
            elif tag == "mtllib":
                mtllib = line.strip()[len("mtllib"):].strip()
    vertices = np.asarray(verts, np.float64).reshape(-1, 3)
    tex_coords = np.asarray(uvs, np.float64).reshape(-1, 2)
    tri, uv_tri = triangulate_faces(faces_ori), triangulate_faces(uv_faces_ori)
    faces = np.asarray(tri, np.int64).reshape(-1, 3)
    uv_faces = np.asarray(uv_tri, np.int64).reshape(-1, 3)
    if faces.size == 0:
        raise ValueError(f"{path}: no faces")
    if faces.max() >= len(vertices):
        raise ValueError(f"{path}: a face names vertex {int(faces.max()) + 1} of {len(vertices)}")
    if uv_faces.max() >= len(tex_coords):
        raise ValueError(f"{path}: a face names texture coordinate {int(uv_faces.max()) + 1} of {len(tex_coords)}")
    unref = np.bincount(faces.ravel(), minlength=len(vertices)) == 0
    if unref.any():
        raise ValueError(f"{path}: {int(unref.sum())} vertices are in no face (first: {int(np.nonzero(unref)[0][0]) + 1}); "
                         "compute_vertex_colors would return fewer colours than vertices")
    texture = None
    if mtllib is not None:
        texture = _read_mtl(os.path.join(os.path.dirname(path), mtllib))
    return ObjMesh(vertices, tex_coords, faces_ori, uv_faces_ori, faces, uv_faces, tex_coords[uv_faces.reshape(-1)], texture)


def triangulate_faces(faces) -> list:
    """helpers.triangulate_faces (helpers.py:657-667): a quad -> (0,1,2), (0,2,3); a triangle as it is; anything else dropped."""
    out = []
    for face in faces:
        if len(face) == 4:
            out.append([face[0], face[1], face[2]])
            out.append([face[0], face[2], face[3]])
        elif len(face) == 3:
            out.append(face)
    return out


def vertex_uvs(mesh: ObjMesh) -> list:
    """get_vertex_uvs (helpers.py:212-234): per vertex, list(set(...)) of the UV tuples of its triangle corners, in CPython's
    set order over the same insertion order."""
    per = {}
    uv = mesh.corner_uvs.tolist()
    for c, v in enumerate(mesh.faces.reshape(-1).tolist()):
        per.setdefault(v, []).append(uv[c])
    return [list(set(tuple(item) for item in value)) for _, value in sorted(per.items())]


# ---- textures and colours --------------------------------------------------------------------------------------------------
def load_texture(texture, device=None) -> torch.Tensor:
    """The texture as uint8 [H,W,C] (C = 3 or 4) on the device: a baseline JPEG through ingest.decode_jpeg (byte-identical to
    PIL), anything else through PIL.  texture: a path, the file's bytes, or an array / tensor already decoded.  ValueError for
    any mode but RGB / RGBA (get_color_from_texture indexes three channels of getpixel's tuple)."""
    from . import ingest
    dev = _lib.hip_device(device, _WHAT)
    if isinstance(texture, (np.ndarray, torch.Tensor)):
        img = torch.from_numpy(np.array(texture)) if isinstance(texture, np.ndarray) else texture
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] not in (3, 4):
            raise ValueError(f"texture must be uint8 [H,W,3|4], got {img.dtype} {tuple(img.shape)}")
        return img.to(dev).contiguous()
    data = texture if isinstance(texture, (bytes, bytearray)) else open(texture, "rb").read()
    header = ingest._header_or_none(bytes(data))
    if header.gpu:
        return ingest.decode_jpeg([bytes(data)], device=dev, headers=[header])[0]
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if im.mode not in ("RGB", "RGBA"):
        raise ValueError(f"texture mode {im.mode}: the reference reads three channels of each pixel (need RGB or RGBA)")
    return torch.from_numpy(np.array(im)).to(dev)


class _TriangleCSR:
    """t4d_obj_vertex_faces over int32 triangles [F,3]: offsets [n_vert+1], entries (corner ids 3*f+k ascending per vertex)."""

    def __init__(self, faces: np.ndarray, n_vert: int, dev):
        self.faces = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev)
        n_faces = int(self.faces.shape[0])
        self.offsets = torch.empty(n_vert + 1, dtype=torch.int32, device=dev)
        self.entries = torch.empty(3 * n_faces, dtype=torch.int32, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)
        scratch, nscratch = _lib.scratch("t4d_obj_csr_scratch_bytes", dev, n_vert)
        _lib.call("t4d_obj_vertex_faces", ptr(self.faces), n_faces, n_vert, ptr(self.offsets), ptr(self.entries), ptr(status),
                  ptr(scratch), nscratch, _lib.stream(dev))
        self.bad, self.unreferenced = _status(status)
        if self.bad:
            raise ValueError(f"faces: {self.bad} corners name a vertex outside [0, {n_vert})")


def vertex_colors(texture, mesh: ObjMesh, device=None):
    """compute_vertex_colors (helpers.py:181-209): (colors int32 [N,3], the integer means as the reference returns them, and
    rgb_colors float32 [N,3] = colors / 255.0), both on the device.  ValueError where get_color_from_texture would raise: a
    corner whose UV lands on column `width` or row `height` (x1 == width: u % 1 == 1.0 after rounding), or a NaN UV."""
    dev = _lib.hip_device(device, _WHAT)
    img = load_texture(texture, dev)
    n_vert = int(mesh.vertices.shape[0])
    csr = _TriangleCSR(mesh.faces, n_vert, dev)
    uv = torch.from_numpy(np.ascontiguousarray(mesh.corner_uvs, np.float64)).to(dev)
    n_corners = int(uv.shape[0])
    scratch, nscratch = _lib.scratch("t4d_setup_colors_scratch_bytes", dev, n_corners)
    colors = torch.empty(n_vert, 3, dtype=torch.int32, device=dev)
    rgb = torch.empty(n_vert, 3, dtype=torch.float32, device=dev)
    status = torch.empty(3, dtype=torch.int32, device=dev)
    H, W, ch = (int(s) for s in img.shape)
    _lib.call("t4d_setup_vertex_colors", ptr(img), W, H, ch, ptr(uv), n_corners, ptr(csr.offsets), ptr(csr.entries), n_vert,
              ptr(colors), ptr(rgb), ptr(status), ptr(scratch), nscratch, _lib.stream(dev))
    bad, first, unref = _status(status)
    if bad:
        f, k = divmod(first, 3)
        raise ValueError(f"{bad} triangle corners sample outside the {W}x{H} texture (first: face {f} corner {k}, uv "
                         f"{tuple(mesh.corner_uvs[first])}); PIL's getpixel would raise")
    if unref:
        raise ValueError(f"{unref} vertices are in no face")
    return colors, rgb


def rotations_from_normals(normals: torch.Tensor) -> torch.Tensor:
    """build_quaterion(torch.from_numpy(normals).float()) (train.py:136, external.py:45-61) in float32 on the device: [N,4].
    Within 2 float32 ulp or 1e-6 of CPU torch (acos / sin / cos are the device's own)."""
    n = normals.detach().to(torch.float64).contiguous()
    out = torch.empty(n.shape[0], 4, dtype=torch.float32, device=n.device)
    _lib.call("t4d_setup_quaternions", ptr(n), int(n.shape[0]), ptr(out), _lib.stream(n.device))
    return out


# ---- the one-ring ----------------------------------------------------------------------------------------------------------
def one_ring(faces_ori, n_vert: int):
    """find_adjacent_vertices(vertices, faces_ori) (helpers.py:670-688: a quad joins all four corners, diagonals included) in
    CPython's set order, and the padding of train.py:170-176: (neighbor_indices_ori, list of lists; neighbor_indices, int64
    [n_vert, max_ns] padded with the vertex's own index)."""
    adjacent = {i: set() for i in range(n_vert)}
    for quad in faces_ori:
        if len(quad) == 4:
            v1, v2, v3, v4 = quad
            adjacent[v1].update([v2, v3, v4])
            adjacent[v2].update([v1, v3, v4])
            adjacent[v3].update([v1, v2, v4])
            adjacent[v4].update([v1, v2, v3])
        else:
            v1, v2, v3 = quad
            adjacent[v1].update([v2, v3])
            adjacent[v2].update([v1, v3])
            adjacent[v3].update([v1, v2])
    ori = [list(adjacent[i]) for i in range(n_vert)]
    K = max(len(lst) for lst in ori)
    padded = np.empty((n_vert, K), np.int64)
    for i, lst in enumerate(ori):
        padded[i, :len(lst)] = lst
        padded[i, len(lst):] = i
    return ori, padded


def neighbor_priors(means3D: torch.Tensor, neighbor_indices, eye_del_masks):
    """train.py:177-206 on the device: (neighbor_weight, neighbor_dist), float32 [P,K], from float64(float32 means3D) - the
    reference's trimesh copy of params['means3D'] - and the padded neighbour indices.  A pair (v, j) with j in eye_del_masks and
    v not has its squared distance x 1000^2 in the weight; weight = exp(-2000 wh), 0 where that is 1.0; dist = sqrt(sq)."""
    x = means3D.detach().float().contiguous()
    dev = x.device
    P = int(x.shape[0])
    nbr = torch.as_tensor(neighbor_indices).to(device=dev, dtype=torch.int64).contiguous()
    K = int(nbr.shape[1])
    eye = np.zeros(P, np.uint8)
    e = np.asarray(eye_del_masks, np.int64).reshape(-1)
    eye[e[(e >= 0) & (e < P)]] = 1                                  # `in` over the array: other values never match an index
    eye_d = torch.from_numpy(eye).to(dev)
    weight = torch.empty(P, K, dtype=torch.float32, device=dev)
    dist = torch.empty(P, K, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("t4d_setup_one_ring", ptr(x), P, K, ptr(nbr), ptr(eye_d), ptr(weight), ptr(dist), ptr(status), _lib.stream(dev))
    if _status(status)[0]:
        raise ValueError(f"neighbor_indices: {_status(status)[0]} entries outside [0, {P})")
    return weight, dist


# ---- initialize_losses' pieces ---------------------------------------------------------------------------------------------
def _mask_rows(facial_regions, key, P: int) -> np.ndarray:
    a = facial_regions[key[0]][key[1]] if isinstance(key, tuple) else facial_regions[key]
    r = np.asarray(a, np.int64).reshape(-1)
    r = np.where(r < 0, r + P, r)                                   # torch's indexing wraps negative indices
    if r.size and (r.min() < 0 or r.max() >= P):
        raise ValueError(f"facial_regions {key}: an index outside [-{P}, {P})")
    return r


def region_weights(neighbor_weight: torch.Tensor, facial_regions: dict, losses_weights: dict):
    """iso_w, rig_w, rot_w of train.py:545-581: copies of neighbor_weight with `w[mask, :] *= c / losses_weights[k]` applied in
    the reference's order, each a float32 multiply by float32(c / w) that a row takes once per mask however often the mask lists
    it.  A block whose weight is 0 leaves its copy as it is."""
    w = neighbor_weight.detach().float().contiguous()
    dev = w.device
    P, K = (int(s) for s in w.shape)
    scratch, nscratch = _lib.scratch("t4d_setup_region_scratch_bytes", dev, P)
    out = []
    for name, (key, blocks) in REGION_WEIGHT_BLOCKS.items():
        lw = losses_weights[key]
        if lw == 0:
            out.append(w.clone())
            continue
        rows = [_mask_rows(facial_regions, m, P) for m, _ in blocks]
        off = np.zeros(len(rows) + 1, np.int32)
        off[1:] = np.cumsum([r.size for r in rows])
        factors = torch.tensor(np.array([c / lw for _, c in blocks], np.float32)).to(dev)
        rows_d = torch.from_numpy(np.concatenate(rows).astype(np.int32)).to(dev)
        off_d = torch.from_numpy(off).to(dev)
        res = torch.empty_like(w)
        _lib.call("t4d_setup_region_weights", ptr(w), P, K, ptr(rows_d), ptr(off_d), off.ctypes.data_as(C.POINTER(C.c_int32)),
                  len(rows), ptr(factors), ptr(res), ptr(scratch), nscratch, _lib.stream(dev))
        out.append(res)
    return tuple(out)


def flatten_candidate_edges(faces) -> np.ndarray:
    """The constructors' candidate edges, by their own expression (loss_util.py:121): sorted (0,1) and (1,2) of every face, made
    unique through a CPython set and listed in its order.  int64 [E,2]."""
    f = np.asarray(faces)
    vertices = list(set([tuple(v) for v in np.sort(np.concatenate((f[:, 0:2], f[:, 1:3]), axis=0))]))
    return np.asarray(vertices, np.int64).reshape(-1, 2)


def flatten_edges(faces, n_vert: Optional[int] = None, device=None):
    """(v0s, v1s, v2s, v3s) of FlattenLoss(faces) / SoftFlattenLoss(faces) (loss_util.py:114-170, 262-318), int64 CPU tensors
    like the modules' buffers.  Edges of more than two faces are dropped, v2 / v3 are the third corners of the lowest and the
    next face id, and only the two-face edges are kept, in candidate order.  As in the reference, v0s / v1s are read at the
    edge's rank among the edges NOT dropped, which is the edge itself unless an earlier edge had more than two faces.
    ValueError where the reference's `v[0]` fails: a face with no corner besides the ends, on an edge that is not dropped."""
    dev = _lib.hip_device(device, _WHAT)
    f = np.asarray(faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"faces must be a non-empty integer [F,3] array, got {f.dtype} {f.shape}")
    if f.min() < 0:
        raise ValueError("faces: a negative vertex index")
    n = int(n_vert) if n_vert is not None else int(f.max()) + 1
    if f.max() >= n:
        raise ValueError(f"faces: vertex {int(f.max())} outside [0, {n})")
    edges = flatten_candidate_edges(f)
    csr = _TriangleCSR(f, n, dev)
    E = int(edges.shape[0])
    scratch, nscratch = _lib.scratch("t4d_setup_edges_scratch_bytes", dev, E)
    edges_d = torch.from_numpy(edges.astype(np.int32)).to(dev)
    out = torch.empty(4, E, dtype=torch.int64, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call("t4d_setup_flatten_edges", ptr(csr.faces), n, ptr(csr.offsets), ptr(csr.entries), ptr(edges_d), E, ptr(out), ptr(n_out),
              ptr(status), ptr(scratch), nscratch, _lib.stream(dev))
    bad_end, no_third = _status(status)
    if bad_end or no_third:
        raise ValueError(f"faces: {bad_end} edge ends out of range, {no_third} faces without a third corner (degenerate)")
    host = out[:, :int(n_out.item())].cpu()
    return tuple(host[i].contiguous() for i in range(4))


def region_topology(neighbor_indices_ori, facial_regions: dict, mask_list=(), pre_mask=(), ex_mask=(), device=None):
    """FlattenLoss_v2(variables, mask_list, pre_mask, ex_mask) (loss_util.py:223-255): (neighbor_num int64 [P], mask int64
    [P,K,3] = slot < neighbor_num, region_mask int64) on the device.  region_mask is the reference's own
    list(set(list(set(regions + pre_mask) - set(ex_mask)))), or range(P) when that is empty."""
    dev = _lib.hip_device(device, _WHAT)
    nnum = torch.tensor([len(lst) for lst in neighbor_indices_ori]).to(dev)
    P, K = int(nnum.shape[0]), max(len(lst) for lst in neighbor_indices_ori)
    mask = torch.empty(P, K, 3, dtype=torch.int64, device=dev)
    _lib.call("t4d_setup_neighbor_mask", ptr(nnum), P, K, ptr(mask), _lib.stream(dev))
    rm = []
    for r in mask_list:
        rm += facial_regions["region_masks"][r].tolist()
    rm += list(pre_mask)
    rm = list(set(rm) - set(ex_mask))
    if len(rm) == 0:
        rm = [idx for idx in range(P)]
    rm = list(set(rm))
    return nnum, mask, torch.from_numpy(np.array(rm)).to(dev)


class FlattenTopology:
    """The buffers of a FlattenLoss / SoftFlattenLoss (loss_util.py:114-170, 262-318): v0s..v3s int64 (CPU, as the modules
    hold them) and nf / threshold / average.  No forward: TopologyPriors evaluates the terms."""

    def __init__(self, faces, threshold: float = 0, average: bool = False, device=None):
        f = torch.tensor(faces)
        self.nf, self.threshold, self.average = int(f.shape[0]), threshold, average
        self.v0s, self.v1s, self.v2s, self.v3s = flatten_edges(f.numpy(), device=device)


class RegionTopology:
    """The buffers of a FlattenLoss_v2 (loss_util.py:223-255): neighbor_num, mask [P,K,3], region_mask, all int64 on the device,
    and the `variables` it was built from.  No forward: TopologyPriors evaluates the terms."""

    def __init__(self, variables: dict, mask_list=(), pre_mask=(), ex_mask=(), device=None):
        self.variables = variables
        self.neighbor_num, self.mask, self.region_mask = region_topology(
            variables["neighbor_indices_ori"], variables["facial_regions"], mask_list, pre_mask, ex_mask, device=device)


# ---- the drop-ins ----------------------------------------------------------------------------------------------------------
def _load_facial_regions(path="./assets/facial_regions.pkl"):
    with open(path, "rb") as f:
        return pickle.load(f)


def coarse_params(mesh: ObjMesh, trans_g, texture=None, device=None):
    """The coarse parameters and variables of train.py:115-206 from a read OBJ: (params, variables, colors) with params the
    reference's seven nn.Parameters (float32, device) and variables its keys up to neighbor_dist (facial_regions excluded);
    colors the integer vertex colours.  texture: mesh.texture by default."""
    dev = _lib.hip_device(device, _WHAT)
    from .densify import coarse_scales
    from .objexport import vertex_normals
    trans_g = np.linalg.inv(trans_g)                                                 # train.py:124-126, float64 on the host
    vertices = mesh.vertices @ trans_g[:3, :3].T
    vertices = vertices + trans_g[:3, 3]
    colors, rgb = vertex_colors(mesh.texture if texture is None else texture, mesh, dev)
    v64 = torch.from_numpy(np.ascontiguousarray(vertices)).to(dev)
    log_scales, init_scale = coarse_scales(v64)                                      # o3d_knn on the float64 vertices
    quats = rotations_from_normals(vertex_normals(v64, mesh.faces))
    n = vertices.shape[0]
    raw = {
        'means3D': v64.float(),
        'rgb_colors': rgb,
        'unnorm_rotations': quats,
        'logit_opacities': torch.full((n, 1), 1000.0, dtype=torch.float32, device=dev),
        'log_scales': torch.from_numpy(log_scales).to(dev).float(),
        'cam_m': torch.zeros(MAX_CAMS, 3, dtype=torch.float32, device=dev),
        'cam_c': torch.zeros(MAX_CAMS, 3, dtype=torch.float32, device=dev),
    }
    params = {k: torch.nn.Parameter(v.contiguous().requires_grad_(True)) for k, v in raw.items()}
    variables = {'max_2D_radius': torch.zeros(n, dtype=torch.float32, device=dev),
                 'init_scale': torch.from_numpy(init_scale).to(dev),
                 'faces': np.asarray(mesh.faces, np.int64),
                 'trans_g': trans_g,
                 'faces_ori': mesh.faces_ori,
                 'uvs_ori': np.array(mesh.tex_coords),
                 'uv_faces_ori': mesh.uv_faces_ori,
                 'uvs_texture_ori': vertex_uvs(mesh)}
    return params, variables, colors


def initialize_params(args, trans_g, facial_regions: Optional[dict] = None, device=None):
    """train.py:115-269: (params, variables) with the reference's keys, dtypes and devices, from
    <args.input_dir>/<args.seq>/face_v5.obj, its texture and facial_regions (default: ./assets/facial_regions.pkl, as the
    reference).  The dense half is densify.init_dense_gaussians(..., args.density if args.gen_tex else 1)."""
    from .densify import init_dense_gaussians
    dev = _lib.hip_device(device, _WHAT)
    rt_dir = os.path.join(args.input_dir, args.seq)
    mesh = read_obj(os.path.join(rt_dir, "face_v5.obj"))
    params, variables, _ = coarse_params(mesh, trans_g, device=dev)
    if facial_regions is None:
        facial_regions = _load_facial_regions()
    variables['facial_regions'] = facial_regions
    ori, padded = one_ring(variables['faces_ori'], mesh.vertices.shape[0])
    weight, dist = neighbor_priors(params['means3D'], padded, facial_regions["eye_del_masks"])
    variables["neighbor_indices_ori"] = ori
    variables["neighbor_indices"] = torch.from_numpy(padded).to(dev).contiguous()
    variables["neighbor_weight"] = weight
    variables["neighbor_dist"] = dist
    init_dense_gaussians(params, variables, facial_regions, args.density if args.gen_tex else 1)
    return params, variables


def initialize_losses(variables: dict, device=None):
    """train.py:511-587: (variables, losses, losses_weights, losses_weights_dense).  losses maps the reference's nine names, in
    its order, to FlattenTopology / RegionTopology objects with the modules' buffers; variables gains iso_w, rig_w, rot_w."""
    fr = variables["facial_regions"]
    dev = _lib.hip_device(device if device is not None else (variables["neighbor_weight"].device
                                                             if torch.is_tensor(variables.get("neighbor_weight")) else None), _WHAT)
    edge = lambda k, soft: FlattenTopology(fr[FLAT_EDGE_TERMS[k]], threshold=180 if soft else 0, device=dev)
    losses = {
        'flat': edge('flat', False),
        'flat_lip_bottom': edge('flat_lip_bottom', False),
        'flat_eye': RegionTopology(variables, mask_list=["EyeLidOuterTop", "EyeLidTop", "EyeLidBottom"], device=dev),
        'flat_lip_socket': RegionTopology(variables, mask_list=[], pre_mask=fr["lip_socket_flat_masks"].tolist(), device=dev),
        'flat_face_bottom': RegionTopology(variables,
                                           mask_list=["LipOuterTop", "LipOuterBottom", "Chin", "NeckFront",
                                                      "LipBottom", "LipTop", "LipInnerBottom", "LipInnerTop",
                                                      "EyeLidOuterBottom", "EyeLidBottom",
                                                      "MouthSocket", "EyeSocket"],
                                           pre_mask=fr["face_flat_masks"].tolist(),
                                           ex_mask=fr["lip_flat_edge_masks"].tolist(), device=dev),
        'flat_lip': edge('flat_lip', True),
        'flat_mouth': edge('flat_mouth', True),
        'flat_lid_top': edge('flat_lid_top', True),
        'flat_lid_bottom': edge('flat_lid_bottom', True),
    }
    losses_weights = dict(LOSSES_WEIGHTS)
    losses_weights_dense = dict(LOSSES_WEIGHTS_DENSE)
    with torch.no_grad():
        iso_w, rig_w, rot_w = region_weights(variables["neighbor_weight"], fr, losses_weights)
    variables["iso_w"] = iso_w
    variables["rig_w"] = rig_w
    variables["rot_w"] = rot_w
    return variables, losses, losses_weights, losses_weights_dense
