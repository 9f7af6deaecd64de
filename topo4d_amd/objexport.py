"""
The face.obj of helpers.save_mesh (helpers.py:963-998) on the GPU, over csrc/t4d_obj.hip (include/topo4d_raster.h):

    vertex_normals(vertices, faces)                           trimesh 4.4.1 Trimesh(vertices, faces).vertex_normals, float64
    write_obj_with_uv(file_path, vertices, faces, uvs, uv_faces)  helpers.py:258-272, byte for byte
    format_float_repr(x)                                      repr(float(v)) of every value (the formatter alone, for tests)
    seam_color_index(uvs_ori, uvs_texture_ori)                duplicate_texture_vertex_color_2 (helpers.py:923-934) as indices
    MeshExporter(variables)                                   one topology's cached state; .save_mesh(out_dir, params, frame, ...)
    save_mesh(out_dir, params, variables, frame, res, gen_texture)  the drop-in for helpers.save_mesh

Per frame only the "v" block is formatted and crosses to the host; the "vt" and "f" blocks of faces_ori / uvs_ori /
uv_faces_ori are formatted once per topology and kept as host bytes.  Floats are written as Python's repr (what the reference's
f-strings print for numpy float64).  Vertex normals are a float64 restatement of trimesh: they match it to
rounding, not bit for bit.  Preconditions of the reference (trimesh's process=True merges coincident vertices and drops
unreferenced ones, after which save_mesh's shapes no longer agree): every vertex must be referenced by variables["faces"]
(checked once per topology, ValueError otherwise); coincident vertices are not detected.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import ptr

T4D_OBJ_V, T4D_OBJ_VT, T4D_OBJ_F = 0, 1, 2
FLOAT_CHARS = 24

_EXPORTERS = []
_WHAT = "the OBJ export"


def _float64(x, dev, what: str) -> torch.Tensor:
    """A float64 device tensor of x.  float32 input is refused: numpy prints float32 with float32's own shortest repr."""
    if isinstance(x, torch.Tensor):
        if x.dtype == torch.float32:
            raise ValueError(f"{what}: float32 values print differently from float64; pass float64")
        return x.detach().to(device=dev, dtype=torch.float64).contiguous()
    arr = np.asarray(x)
    if arr.dtype == np.float32:
        raise ValueError(f"{what}: float32 values print differently from float64; pass float64")
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).to(dev)


def _max_bytes(kind: int, rows: int, corners: int = 0) -> int:
    n = _lib.load().t4d_obj_text_max_bytes(kind, rows, corners)
    if n == 0 and rows > 0:
        raise _lib.error("t4d_obj_text_max_bytes", exc=ValueError)
    return int(n)


def _float_lines(values: torch.Tensor, kind: int) -> bytes:
    """The "v" ([rows,3]) or "vt" ([rows,2]) lines of float64 device values."""
    rows = int(values.shape[0])
    if rows == 0:
        return b""
    dev = values.device
    cap = _max_bytes(kind, rows)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    scratch, nscratch = _lib.scratch("t4d_obj_text_scratch_bytes", dev, kind, rows, 0)
    length = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call("t4d_obj_float_lines", kind, ptr(values), rows, ptr(out), cap, ptr(length), ptr(scratch), nscratch, _lib.stream(dev))
    return _lib.read_back(out, length, cap, "t4d_obj_float_lines", empty_ok=True)


def _corner_lists(faces, uv_faces):
    """face offsets and the (vertex, uv) corners write_obj_with_uv emits: zip(faces, uv_faces), then zip(face, uv_face)."""
    def flat(fs):
        if isinstance(fs, torch.Tensor):
            fs = fs.detach().cpu().numpy()
        if isinstance(fs, np.ndarray) and fs.ndim == 2:
            return np.full(fs.shape[0], fs.shape[1], np.int64), fs.astype(np.int64).ravel()
        lens = np.fromiter((len(f) for f in fs), np.int64, len(fs))
        return lens, np.fromiter((v for f in fs for v in f), np.int64, int(lens.sum()))
    lens, v = flat(faces)
    uv_lens, uv = flat(uv_faces)
    n = min(len(lens), len(uv_lens))
    start = lambda ls: np.concatenate([[0], np.cumsum(ls)[:-1]]).astype(np.int64)
    if not (len(lens) == len(uv_lens) and np.array_equal(lens, uv_lens)):
        keep = np.minimum(lens[:n], uv_lens[:n])
        pick = lambda ls, flat_: flat_[np.concatenate([s + np.arange(k) for s, k in zip(start(ls)[:n], keep)])
                                        if n else np.zeros(0, np.int64)]
        v, uv, lens = pick(lens, v), pick(uv_lens, uv), keep
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if np.abs(v).max(initial=0) >= 1 << 62 or np.abs(uv).max(initial=0) >= 1 << 62:
        raise ValueError("write_obj_with_uv: face indices must be below 2^62 in magnitude")
    return off, v, uv


def _face_lines(faces, uv_faces, dev) -> bytes:
    off, v, uv = _corner_lists(faces, uv_faces)
    n_faces, corners = len(off) - 1, int(off[-1])
    if n_faces == 0:
        return b""
    cap = _max_bytes(T4D_OBJ_F, n_faces, corners)
    d_off, d_v, d_uv = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (off, v, uv))
    if corners == 0:
        d_v = d_uv = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    scratch, nscratch = _lib.scratch("t4d_obj_text_scratch_bytes", dev, T4D_OBJ_F, n_faces, corners)
    length = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call("t4d_obj_face_lines", ptr(d_off), ptr(d_v), ptr(d_uv), n_faces, corners, ptr(out), cap, ptr(length), ptr(scratch),
              nscratch, _lib.stream(dev))
    return _lib.read_back(out, length, cap, "t4d_obj_face_lines", empty_ok=True)


def _rows(x, cols: int, what: str, dev) -> torch.Tensor:
    t = _float64(x, dev, what)
    if t.numel() == 0:
        return t.reshape(0, cols)
    if t.dim() != 2 or t.shape[1] < cols:
        raise ValueError(f"{what} must be [n, >={cols}], got {tuple(t.shape)}")
    return t[:, :cols].contiguous()


def write_obj_with_uv(file_path, vertices, faces, uvs, uv_faces) -> None:
    """helpers.py:258-272: the same bytes.  vertices [n,3] and uvs [m,2] float64 (numpy arrays or tensors; only the first 3 /
    2 columns are printed, as the f-strings do), faces / uv_faces lists of lists of any length, int arrays or tensors."""
    dev = vertices.device if isinstance(vertices, torch.Tensor) and vertices.is_cuda else _lib.hip_device(None, _WHAT)
    data = _float_lines(_rows(vertices, 3, "vertices", dev), T4D_OBJ_V) + _float_lines(_rows(uvs, 2, "uvs", dev), T4D_OBJ_VT) + \
        _face_lines(faces, uv_faces, dev)
    with open(file_path, "wb") as f:
        f.write(data)


def format_float_repr(x: torch.Tensor) -> list:
    """[repr(float(v)) for v in x] from the device formatter; x a float64 tensor (moved to the device if it is not there)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64:
        raise ValueError("format_float_repr expects a float64 tensor")
    dev = x.device if x.is_cuda else _lib.hip_device(None, _WHAT)
    vals = x.detach().reshape(-1).to(dev).contiguous()
    n = vals.numel()
    if n == 0:
        return []
    chars = torch.empty((n, FLOAT_CHARS), dtype=torch.uint8, device=dev)
    lens = torch.empty(n, dtype=torch.uint8, device=dev)
    _lib.call("t4d_obj_format_doubles", ptr(vals), n, ptr(chars), ptr(lens), _lib.stream(dev))
    c, l = chars.cpu().numpy(), lens.cpu().numpy()
    return [c[i, :l[i]].tobytes().decode() for i in range(n)]


def _check_faces(faces, n_vert: int) -> np.ndarray:
    """variables["faces"] as int32 [F,3]: ValueError for an index outside [0, n_vert) or an unreferenced vertex."""
    f = np.asarray(faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] == 0 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"faces must be a non-empty integer [F,3] triangle list, got {f.dtype} {f.shape}")
    if f.min() < 0 or f.max() >= n_vert:
        raise ValueError(f"faces index a vertex outside [0, {n_vert}): min {int(f.min())}, max {int(f.max())}")
    unref = np.bincount(f.ravel(), minlength=n_vert) == 0
    if unref.any():
        raise ValueError(f"{int(unref.sum())} of {n_vert} vertices are in no face (first: {int(np.nonzero(unref)[0][0])}); "
                         "trimesh would drop them and helpers.save_mesh would fail on shape")
    return np.ascontiguousarray(f, dtype=np.int32)


class _VertexFaces:
    """The vertex -> corner CSR of one triangle list on the device (t4d_obj_vertex_faces)."""

    def __init__(self, faces: torch.Tensor, n_vert: int):
        dev = faces.device
        self.faces, self.n_vert, self.n_faces = faces, int(n_vert), int(faces.shape[0])
        self.offsets = torch.empty(self.n_vert + 1, dtype=torch.int32, device=dev)
        self.entries = torch.empty(3 * self.n_faces, dtype=torch.int32, device=dev)
        status = torch.empty(2, dtype=torch.int32, device=dev)
        scratch, nscratch = _lib.scratch("t4d_obj_csr_scratch_bytes", dev, self.n_vert)
        _lib.call("t4d_obj_vertex_faces", ptr(faces), self.n_faces, self.n_vert, ptr(self.offsets), ptr(self.entries), ptr(status),
                  ptr(scratch), nscratch, _lib.stream(dev))
        bad, unref = (int(v) for v in status.cpu())
        if bad:
            raise ValueError(f"faces: {bad} corners index a vertex outside [0, {self.n_vert})")
        if unref:
            raise ValueError(f"{unref} of {self.n_vert} vertices are in no face; trimesh would drop them")
        self.face_scratch = _lib.scratch("t4d_obj_normals_scratch_bytes", dev, self.n_faces)[0]

    def normals(self, vertices: torch.Tensor) -> torch.Tensor:
        if vertices.dtype not in (torch.float32, torch.float64) or tuple(vertices.shape) != (self.n_vert, 3):
            raise ValueError(f"vertices must be float32/float64 [{self.n_vert},3], got {vertices.dtype} {tuple(vertices.shape)}")
        v = vertices.detach().contiguous()
        out = torch.empty((self.n_vert, 3), dtype=torch.float64, device=v.device)
        _lib.call("t4d_obj_vertex_normals", ptr(v), 1 if v.dtype == torch.float64 else 0, self.n_vert, ptr(self.faces), self.n_faces,
                  ptr(self.offsets), ptr(self.entries), ptr(out), ptr(self.face_scratch), self.face_scratch.numel(),
                  _lib.stream(v.device))
        return out


def vertex_normals(vertices: torch.Tensor, faces) -> torch.Tensor:
    """trimesh.Trimesh(vertices, faces).vertex_normals (train.py:135-136, helpers.py:967): vertices float32 / float64 [P,3] on a
    HIP device, faces int [F,3] (tensor or array); returns [P,3] float64 on the same device.  ValueError when a face index is
    out of range or a vertex is in no face."""
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda:
        raise RuntimeError("topo4d_amd has no CPU path: vertex_normals needs the vertices on a HIP device")
    f = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.asarray(faces))
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0:
        raise ValueError(f"faces must be a non-empty [F,3] triangle list, got {tuple(f.shape)}")
    f = f.to(device=vertices.device, dtype=torch.int32).contiguous()
    return _VertexFaces(f, int(vertices.shape[0])).normals(vertices)


def seam_color_index(uvs_ori, uvs_texture_ori) -> np.ndarray:
    """duplicate_texture_vertex_color_2(variables, colors) == colors[seam_color_index(uvs_ori, uvs_texture_ori)]: the
    reference's dict from a UV to the last vertex listing it, looked up for every row of uvs_ori (KeyError on a miss)."""
    uv_dict = {}
    for idx, uvs_ in enumerate(uvs_texture_ori):
        for uv in uvs_:
            uv_dict[tuple(uv)] = idx
    return np.fromiter((uv_dict[tuple(uv)] for uv in np.asarray(uvs_ori)), np.int64, len(uvs_ori))


class MeshExporter:
    """save_mesh's state for one topology: the checked triangle list and its CSR, the static "vt" / "f" bytes of faces_ori,
    uvs_ori and uv_faces_ori, the inverse of trans_g (computed once, in float64 on the host) and, on first use, the seam map.
    n_vertices defaults to faces.max() + 1; every vertex below it must be in a face."""

    def __init__(self, variables: dict, n_vertices: int = None, device=None):
        faces = variables["faces"]
        n_vert = int(n_vertices) if n_vertices is not None else int(np.asarray(
            faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces).max()) + 1
        faces32 = _check_faces(faces, n_vert)                      # argument errors first, with or without a device
        tg = np.linalg.inv(np.asarray(variables["trans_g"], dtype=np.float64))
        self.variables = variables
        self.n_vert = n_vert
        self.transform = (C.c_double * 12)(*tg[:3, :3].ravel().tolist(), *tg[:3, 3].tolist())
        self.dev = _lib.hip_device(device, _WHAT)
        self.csr = _VertexFaces(torch.from_numpy(faces32).to(self.dev), n_vert)
        self.static = _float_lines(_rows(variables["uvs_ori"], 2, "uvs_ori", self.dev), T4D_OBJ_VT) + \
            _face_lines(variables["faces_ori"], variables["uv_faces_ori"], self.dev)
        self._seam = None

    def frame_vertices(self, params: dict, frame: int) -> torch.Tensor:
        """The float64 [P,3] vertices save_mesh writes for `frame` (helpers.py:965-979), on the device."""
        means = params["means3D"].detach()
        if means.dtype != torch.float32 or tuple(means.shape) != (self.n_vert, 3) or means.device != self.dev:
            raise ValueError(f"params['means3D'] must be float32 [{self.n_vert},3] on {self.dev}, got "
                             f"{means.dtype} {tuple(means.shape)} on {means.device}")
        means = means.contiguous()
        out = torch.empty((self.n_vert, 3), dtype=torch.float64, device=self.dev)
        if frame != 1:
            normals = self.csr.normals(means)
            ls = params["log_scales"].detach().to(torch.float32).contiguous()
            rot = params["unnorm_rotations"].detach().to(torch.float32).contiguous()
            if tuple(ls.shape) != (self.n_vert, 3) or tuple(rot.shape) != (self.n_vert, 4):
                raise ValueError("params['log_scales'] [P,3] and params['unnorm_rotations'] [P,4] expected")
            _lib.call("t4d_obj_frame_vertices", ptr(means), ptr(ls), ptr(rot), ptr(normals), self.n_vert, self.transform,
                      ptr(out), _lib.stream(self.dev))
        else:
            _lib.call("t4d_obj_frame_vertices", ptr(means), None, None, None, self.n_vert, self.transform, ptr(out),
                      _lib.stream(self.dev))
        return out

    def obj_bytes(self, params: dict, frame: int) -> bytes:
        """The whole face.obj of `frame`: the fresh "v" block, then the cached static bytes."""
        return _float_lines(self.frame_vertices(params, frame), T4D_OBJ_V) + self.static

    def seam_colors(self, dense_rgb_colors: torch.Tensor) -> torch.Tensor:
        """save_mesh's colours for the bake (helpers.py:992-996): the clamped dense colours with the first P rows duplicated
        along the seams, as one device gather."""
        if self._seam is None:
            idx = seam_color_index(self.variables["uvs_ori"], self.variables["uvs_texture_ori"])
            self._seam = torch.from_numpy(idx).to(self.dev)
        dense = dense_rgb_colors.detach().clamp(0.0, 1.0)
        return torch.cat([dense[:self.n_vert][self._seam], dense[self.n_vert:]], dim=0)

    def save_mesh(self, out_dir, params: dict, frame: int, res: int = 1024, gen_texture: bool = True, encoder: str = "gpu",
                  pad: int = 0, erode: int = 0, sizes=()) -> None:
        """helpers.save_mesh for this topology: out_dir/face.obj and, with gen_texture, out_dir/face.png.  pad / erode / sizes:
        texture.write_texture's finishing (a gutter round the UV islands, face_<size>.png for smaller levels); the defaults
        write the reference's file."""
        os.makedirs(out_dir, exist_ok=True)
        data = self.obj_bytes(params, frame)
        with open(os.path.join(out_dir, "face.obj"), "wb") as f:
            f.write(data)
        if gen_texture:
            from .texture import write_texture
            write_texture(os.path.join(out_dir, "face.png"), self.variables["dense_uvs"], self.seam_colors(params["dense_rgb_colors"]),
                          self.variables["dense_uv_faces"], res=res, device=self.dev, encoder=encoder, pad=pad, erode=erode,
                          sizes=sizes)


_TOPOLOGY_KEYS = ("faces", "faces_ori", "uvs_ori", "uv_faces_ori", "trans_g")


def save_mesh(out_dir, params: dict, variables: dict, frame: int, res: int = 1024, gen_texture: bool = True, pad: int = 0,
              erode: int = 0, sizes=()) -> None:
    """The drop-in for helpers.save_mesh (train.py:755): a MeshExporter per topology (the same variables objects and vertex
    count), face.png through texture.write_texture(..., encoder="gpu"); pad / erode / sizes as MeshExporter.save_mesh."""
    n_vert = int(params["means3D"].shape[0])
    objs = tuple(variables[k] for k in _TOPOLOGY_KEYS)
    for key, exporter in _EXPORTERS:
        if key[0] == n_vert and exporter.variables is variables and all(a is b for a, b in zip(key[1], objs)):
            break
    else:
        exporter = MeshExporter(variables, n_vertices=n_vert, device=params["means3D"].device)
        _EXPORTERS[:] = [((n_vert, objs), exporter)] + _EXPORTERS[:3]
    exporter.save_mesh(out_dir, params, frame, res=res, gen_texture=gen_texture, pad=pad, erode=erode, sizes=sizes)
