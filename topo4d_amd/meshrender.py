"""
A run's exported meshes rendered into the capture views and scored against the photographs, on the GPU.

    read_face_obj(path)                          the "v" / "vt" / "f v/vt" files objexport.write_obj_with_uv writes
    triangulate(faces_ori, uv_faces_ori)         quads fanned (0,1,2), (0,2,3), as helpers.triangulate_faces
    MeshRenderer(faces, uv_faces, uvs, texture)  topology + texture on the device; .render(vertices, cams) -> (image, depth, index)
    image_metrics(render, target, coverage)      per-view PSNR / L1 / MSE / SSIM, [V, 6] float64

over `t4d_mesh_render` and `t4d_image_metrics` (include/topo4d_raster.h, csrc/t4d_meshrender.hip).  The render's rules are
fixed there so that tests/meshrender_ref.py (numpy, float64) reproduces every output bit.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import T4D_ERR_PAIR_OVERFLOW, T4D_OK, ptr

T4D_MESH_BILINEAR, T4D_MESH_NEAREST = 0, 1
T4D_METRICS_FIELDS = 6
METRIC_NAMES = ("psnr_full", "count", "l1", "mse", "psnr", "ssim")
_MAPPINGS = {"bilinear": T4D_MESH_BILINEAR, "nearest": T4D_MESH_NEAREST}


class FaceObj(NamedTuple):
    vertices: np.ndarray          # float64 [N,3]
    uvs: np.ndarray               # float64 [T,2]
    faces_ori: list               # 0-based polygons (3 or 4 corners)
    uv_faces_ori: list


def _index(s: str, n: int, what: str, path, lineno: int) -> int:
    try:
        i = int(s)
    except ValueError:
        raise ValueError(f"{path}:{lineno}: '{s}' is not a {what} index") from None
    if not 1 <= i <= n:
        raise ValueError(f"{path}:{lineno}: {what} index {i} outside 1..{n}")
    return i - 1


def read_face_obj(path) -> FaceObj:
    """Read a face.obj as write_obj_with_uv (helpers.py:258-272) writes it: "v x y z", "vt u v" and "f v/vt ..." lines with 1-based
    indices (a "v/vt/vn" corner's normal index is ignored).  coarse.read_obj refuses these files (they have no "vn").  ValueError
    for a missing or out-of-range index, a face of fewer than 3 or more than 4 corners, or a file without faces."""
    verts, uvs, faces, uv_faces = [], [], [], []
    pending = []
    with open(path, "r") as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                if len(parts) < 4:
                    raise ValueError(f"{path}:{lineno}: a 'v' line needs x, y and z")
                verts.append((float(parts[1]), float(parts[2]), float(parts[3])))
            elif parts[0] == "vt":
                if len(parts) < 3:
                    raise ValueError(f"{path}:{lineno}: a 'vt' line needs u and v")
                uvs.append((float(parts[1]), float(parts[2])))
            elif parts[0] == "f":
                if not 3 <= len(parts) - 1 <= 4:
                    raise ValueError(f"{path}:{lineno}: a face of {len(parts) - 1} corners (triangles and quads only)")
                pending.append((lineno, parts[1:]))
    for lineno, corners in pending:                               # (indices may name lines further down the file)
        fv, ft = [], []
        for c in corners:
            idx = c.split("/")
            if len(idx) < 2 or not idx[0] or not idx[1]:
                raise ValueError(f"{path}:{lineno}: corner '{c}' is not v/vt")
            fv.append(_index(idx[0], len(verts), "vertex", path, lineno))
            ft.append(_index(idx[1], len(uvs), "texture coordinate", path, lineno))
        faces.append(fv)
        uv_faces.append(ft)
    if not faces:
        raise ValueError(f"{path}: no faces")
    return FaceObj(np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(uvs, np.float64).reshape(-1, 2), faces, uv_faces)


def triangulate(faces_ori, uv_faces_ori) -> Tuple[np.ndarray, np.ndarray]:
    """(faces, uv_faces) int32 [F,3]: a quad -> (0,1,2), (0,2,3), a triangle as it is (helpers.triangulate_faces); ValueError
    for another corner count or a face whose uv face has another length."""
    if len(faces_ori) != len(uv_faces_ori):
        raise ValueError(f"triangulate: {len(faces_ori)} faces but {len(uv_faces_ori)} uv faces")
    tri, uv_tri = [], []
    for k, (f, t) in enumerate(zip(faces_ori, uv_faces_ori)):
        f, t = list(f), list(t)
        if len(f) != len(t) or len(f) not in (3, 4):
            raise ValueError(f"triangulate: face {k} has {len(f)} corners and {len(t)} uv corners (need 3 or 4 of each)")
        tri.append([f[0], f[1], f[2]])
        uv_tri.append([t[0], t[1], t[2]])
        if len(f) == 4:
            tri.append([f[0], f[2], f[3]])
            uv_tri.append([t[0], t[2], t[3]])
    return np.asarray(tri, np.int32).reshape(-1, 3), np.asarray(uv_tri, np.int32).reshape(-1, 3)


def _int_rows(x, what: str, dev) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x))
    if t.dim() != 2 or t.shape[1] != 3 or t.is_floating_point():
        raise ValueError(f"{what} must be an integer [F,3] array, got {t.dtype} {tuple(t.shape)}")
    return t.to(torch.int32).contiguous().to(dev)


class MeshRenderer:
    """Topology and texture of one mesh on the device.  faces / uv_faces: [F,3] integer triangles into the render's vertices
    and into uvs [T,2]; texture [Ht,Wt,3] uint8 or float32 (face.png decoded, or texture.render_colors' bake).  Index errors
    raise ValueError here, once."""

    def __init__(self, faces, uv_faces, uvs, texture, device=None):
        self.dev = _lib.hip_device(device, "the mesh renderer", ValueError)
        self.faces = _int_rows(faces, "faces", self.dev)
        self.uv_faces = _int_rows(uv_faces, "uv_faces", self.dev)
        if self.faces.shape != self.uv_faces.shape:
            raise ValueError(f"faces {tuple(self.faces.shape)} and uv_faces {tuple(self.uv_faces.shape)} differ")
        u = torch.as_tensor(np.asarray(uvs.detach().cpu() if isinstance(uvs, torch.Tensor) else uvs))
        if u.dim() != 2 or u.shape[1] != 2 or u.shape[0] < 1:
            raise ValueError(f"uvs must be [T,2] with T >= 1, got {tuple(u.shape)}")
        self.uvs = u.to(torch.float32).contiguous().to(self.dev)
        tex = texture if isinstance(texture, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(texture))
        if tex.dim() != 3 or tex.shape[2] != 3 or tex.shape[0] < 1 or tex.shape[1] < 1 or tex.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"texture must be uint8 or float32 [Ht,Wt,3], got {tex.dtype} {tuple(tex.shape)}")
        self.texture = tex.to(self.dev).contiguous()
        n_uv = int(self.uvs.shape[0])
        if self.uv_faces.numel() and (int(self.uv_faces.min()) < 0 or int(self.uv_faces.max()) >= n_uv):
            raise ValueError(f"uv_faces index outside [0, {n_uv})")
        self.n_vert_needed = int(self.faces.max()) + 1 if self.faces.numel() else 0
        if self.faces.numel() and int(self.faces.min()) < 0:
            raise ValueError("faces hold a negative index")
        self._cap = {}
        self._scratch = None

    def render(self, vertices: torch.Tensor, cams, bg=None, mapping: str = "bilinear"):
        """(image [V,3,H,W] float32, depth [V,1,H,W] float32 (0: empty), face index [V,H,W] int32 (-1: empty)).  vertices [N,3] in
        the training world frame (float32, or float64 rounded to float32); cams: a sequence of GaussianRasterizationSettings of
        one size, or (packed view records [V, T4D_VIEW_FLOATS], H, W).  bg: 3 floats (default black)."""
        if mapping not in _MAPPINGS:
            raise ValueError(f"mapping must be 'bilinear' or 'nearest', got {mapping!r}")
        views, H, W = _views(cams, self.dev)
        V = int(views.shape[0])
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_floating_point():
            raise ValueError("vertices must be a float [N,3] tensor")
        if vertices.device != self.dev:
            raise ValueError(f"vertices must live on {self.dev}, got {vertices.device}")
        v = vertices.detach().to(torch.float32).contiguous()
        if int(v.shape[0]) < max(self.n_vert_needed, 1):
            raise ValueError(f"faces name vertex {self.n_vert_needed - 1} but only {int(v.shape[0])} vertices were given")
        bgv = (0.0, 0.0, 0.0) if bg is None else tuple(float(x) for x in (bg.tolist() if isinstance(bg, torch.Tensor) else bg))
        if len(bgv) != 3:
            raise ValueError("bg must hold 3 values")
        lib = _lib.load()
        image = torch.empty(V, 3, H, W, dtype=torch.float32, device=self.dev)
        depth = torch.empty(V, 1, H, W, dtype=torch.float32, device=self.dev)
        index = torch.empty(V, H, W, dtype=torch.int32, device=self.dev)
        F = int(self.faces.shape[0])
        key = (V, H, W)
        cap = self._cap.get(key, max(65536, 8 * F * V))
        need = C.c_int64(0)
        host_bg = (C.c_float * 3)(*bgv)
        is_f32 = 1 if self.texture.dtype == torch.float32 else 0
        stream = _lib.stream(self.dev)
        for _ in range(4):
            self._scratch, nbytes = _lib.scratch("t4d_mesh_render_scratch_bytes", self.dev, V, F, H, W, cap, reuse=self._scratch)
            rc = lib.t4d_mesh_render(ptr(v), int(v.shape[0]), ptr(self.faces), ptr(self.uv_faces), F, ptr(self.uvs),
                                     int(self.uvs.shape[0]), ptr(self.texture), is_f32, int(self.texture.shape[0]),
                                     int(self.texture.shape[1]), ptr(views), V, H, W, host_bg, _MAPPINGS[mapping], ptr(image),
                                     ptr(depth), ptr(index), ptr(self._scratch), nbytes, cap, C.byref(need), stream)
            if rc == T4D_OK:
                break
            if rc == T4D_ERR_PAIR_OVERFLOW:
                cap = int(need.value * 1.25) + 1024
                continue
            raise _lib.error("t4d_mesh_render", rc)
        else:
            raise RuntimeError("mesh render: pair capacity kept overflowing")
        self._cap[key] = cap
        return image, depth, index


def _views(cams, dev) -> Tuple[torch.Tensor, int, int]:
    if isinstance(cams, tuple) and len(cams) == 3 and isinstance(cams[0], torch.Tensor):
        views, H, W = cams
        H, W = int(H), int(W)
        if views.dim() != 2 or views.shape[1] != _lib.T4D_VIEW_FLOATS or views.dtype != torch.float32 or views.shape[0] < 1:
            raise ValueError(f"packed views must be float32 [V, {_lib.T4D_VIEW_FLOATS}], got {views.dtype} {tuple(views.shape)}")
        if views.device != dev:
            raise ValueError(f"packed views must live on {dev}")
        return views.contiguous(), H, W
    from .rasterizer import pack_views
    cams = list(cams)
    if not cams:
        raise ValueError("no cameras")
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    if any(int(c.image_height) != H or int(c.image_width) != W for c in cams):
        raise ValueError("all cameras of one render must share one image size")
    return pack_views(cams, dev).contiguous(), H, W


_METRIC_SCRATCH = {}


def image_metrics(render: torch.Tensor, target: torch.Tensor, coverage: Optional[torch.Tensor] = None,
                  mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[V, 6] float64 on the device, columns METRIC_NAMES: full-image PSNR as external.calc_psnr(render[v], target[v]).mean(), then
    over the pixels with coverage >= 0 ([V,H,W] int32: MeshRenderer.render's face index; None: all) and mask > 0.5 ([V,1,H,W]; None:
    all): pixel count, mean L1, MSE, PSNR, mean SSIM (external.calc_ssim's window).  Means run over pixels and channels."""
    for name, t in (("render", render), ("target", target)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 [V,3,H,W], got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
    if render.shape != target.shape or render.device != target.device:
        raise ValueError("render and target must have one shape and device")
    if not render.is_cuda:
        raise ValueError("topo4d_amd has no CPU path: image_metrics needs the images on a HIP device")
    V, _, H, W = (int(s) for s in render.shape)
    cov = None
    if coverage is not None:
        if coverage.shape != (V, H, W) or coverage.dtype != torch.int32 or coverage.device != render.device:
            raise ValueError(f"coverage must be int32 [{V},{H},{W}] on {render.device}")
        cov = coverage.contiguous()
    m = None
    if mask is not None:
        if mask.shape != (V, 1, H, W) or mask.device != render.device or not mask.is_floating_point():
            raise ValueError(f"mask must be float [{V},1,{H},{W}] on {render.device}")
        m = mask.to(torch.float32).contiguous()
    scratch, nbytes = _lib.scratch("t4d_image_metrics_scratch_bytes", render.device, V, H, W, reuse=_METRIC_SCRATCH.get(render.device))
    _METRIC_SCRATCH[render.device] = scratch
    out = torch.empty(V, T4D_METRICS_FIELDS, dtype=torch.float64, device=render.device)
    r, t = render.contiguous(), target.contiguous()
    _lib.call("t4d_image_metrics", V, H, W, ptr(r), ptr(t), ptr(m), ptr(cov), ptr(out), ptr(scratch), nbytes,
              _lib.stream(render.device))
    return out
