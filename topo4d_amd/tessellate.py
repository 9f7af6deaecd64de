"""
Applying a finished displacement map (dispmap.finish, face_disp.png) to the tracked mesh, on the GPU, over csrc/t4d_tessellate.hip
(include/topo4d_raster.h states the exact rules, tests/tessellate_ref.py restates them):

    Tessellation(face_obj, level, device=None)    the flat level-N tessellation of one topology (a sequence shares it): N segments
                                                  per edge, N^2 fine triangles per triangle of meshrender.triangulate
      .n_vertices, .n_faces, .n_uvs, .level
      .faces int32 [N^2 T,3], .uv_faces int32 [N^2 T,3], .uvs float64 [Mt,2]     on the device
      .vertices(vertices)                         float64 [M,3]: the flat tessellation of the mesh vertices (no map)
      .displace(vertices, code, has, labels, unit)  (float64 [M,3], sampled uint8 [M]): every fine vertex pushed along the
                                                  interpolated objexport.vertex_normals normal by the code map sampled at its UV
    displace_frame(face_obj, vertices, code, has, level, dist, device=None)
                                                  -> {"tess", "vertices", "sampled"}: labels from projtex.island_labels, unit =
                                                  dist / 32767
    write_frame(frame_dir, tess, fine_vertices)   face_hi.obj through objexport.write_obj_with_uv

This is the bake's own ray walked back: scanbake shot a ray per texel from the linearly interpolated position along the linearly
interpolated normal, and the displaced vertex is that position plus the stored distance along that normal.  A fine vertex on a UV
seam is displaced once, by the map of its owner's island (the first corner that names a mesh vertex, the lowest triangle of an
edge), so the fine mesh stays as closed as the tracked one; a tap counts only where it has a value and carries that island's label,
which is why the 16-bit maps need no gutter.  The unique-edge tables are made on the host with numpy, once per topology; the index
lists and every per-vertex value are written on the device.

Known limits: the tessellation is flat (linear), there is no smoothing subdivision; a seam vertex takes its owner's island only;
the map is quantised and sampled bilinearly; face_hi.obj carries no normals, like face.obj.  There is no CPU path.

`python -m topo4d_amd.tessellate -e EXP -s SEQ -od DIR [--frames 1-10] --level N --dist DIST [--use_hit]` applies the
%06d/face_disp.png of an output tree that already exists to its %06d/face.obj and writes %06d/face_hi.obj, the file
`evaluate --bake_disp DIST ... --disp_apply N --disp_save_obj` writes.  Every island texel counts as having a value (right for a
filled map; code 32768 is no displacement anyway); --use_hit restricts that to the texels of face_disp_hit.png, for maps that were
not filled.  Frames without face.obj and face_disp.png are left alone.
"""
from __future__ import annotations

import argparse
import math
import os
from typing import Tuple

import numpy as np
import torch

from . import _args, _lib, _run
from ._lib import on_device, ptr

MAX_LEVEL = 64
OBJ_NAME = "face_hi.obj"
_LIMIT = 1 << 31


def check_level(level) -> int:
    """The level as an int; ValueError unless it is a whole number in 1..64 (callable without a device)."""
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 1 <= int(level) <= MAX_LEVEL:
        raise ValueError(f"level must be a whole number of segments per edge in [1, {MAX_LEVEL}], got {level!r}")
    return int(level)


def check_maps(code, has, labels=None) -> Tuple[int, int]:
    """(h, w) of a code map (int32 [h,w]) with its `has` (uint8 or bool) and, if given, its labels (uint8), all of one size;
    ValueError otherwise (callable without a device)."""
    from .dispmap import _map
    h, w = _map(code, "code", (torch.int32,))
    _args.mask(has, "has", h, w)
    if labels is not None:
        _args.mask(labels, "labels", h, w, (torch.uint8,))
    return h, w


def edge_tables(tris: np.ndarray, n_corner: int, what: str) -> Tuple[np.ndarray, np.ndarray]:
    """(edges int32 [E,3], tri_edge int32 [T,3]) of triangles int [T,3] over n_corner vertices (host): the undirected edges as
    sorted pairs (lo < hi) in lexicographic order with, third, the lowest triangle that has the edge; and per triangle the edges of
    (a, b), (b, c), (c, a).  ValueError for an index outside [0, n_corner) or a triangle that names a vertex twice."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    if t.shape[0] < 1:
        raise ValueError(f"{what}: no triangles")
    if t.min() < 0 or t.max() >= n_corner:
        raise ValueError(f"{what} name a vertex outside [0, {n_corner}): min {int(t.min())}, max {int(t.max())}")
    twice = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 2] == t[:, 0])
    if twice.any():
        raise ValueError(f"{what}: triangle {int(np.nonzero(twice)[0][0])} names a vertex twice; it has no three edges to split")
    pairs = np.sort(np.stack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 1).reshape(-1, 2), axis=1)      # row 3 t + k
    uniq, first, inverse = np.unique(pairs, axis=0, return_index=True, return_inverse=True)
    edges = np.concatenate([uniq, (first // 3)[:, None]], 1)                      # the first row of an edge is in its lowest triangle
    return np.ascontiguousarray(edges, np.int32), np.ascontiguousarray(inverse.reshape(-1, 3), np.int32)


def fine_sizes(n_corner: int, n_edges: int, n_tri: int, level: int) -> Tuple[int, int]:
    """(fine vertices M, fine triangles N^2 T); ValueError when either reaches 2^31."""
    n = int(level)
    m, f = n_corner + n_edges * (n - 1) + n_tri * ((n - 1) * (n - 2) // 2), n * n * n_tri
    if m >= _LIMIT or f >= _LIMIT:
        raise ValueError(f"level {n} gives {f} triangles and {m} vertices; both must be below 2^31")
    return m, f


def _vertices(x, n: int, dev) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype != torch.float64 or tuple(t.shape) != (n, 3):
        raise ValueError(f"vertices must be float64 [{n},3], got {t.dtype} {tuple(t.shape)}")
    return t.detach().to(dev).contiguous()


class Tessellation:
    """The level-N tessellation of one topology: its tables and index lists on the device.  ValueError for a level outside 1..64, a
    face whose uv face has another length, an index out of range, a triangle that names a vertex twice, and sizes of 2^31 or more -
    all before a device is looked for."""

    def __init__(self, face_obj, level: int, device=None):
        from . import meshrender, projtex
        self.level = check_level(level)
        faces, uv_faces = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
        self.n_corner, self.n_uv_corner = int(len(face_obj.vertices)), int(len(face_obj.uvs))
        edges, tri_edge = edge_tables(faces, self.n_corner, "faces")
        uv_edges, uv_tri_edge = edge_tables(uv_faces, self.n_uv_corner, "uv_faces")
        self.n_tri, self.n_edges, self.n_uv_edges = int(faces.shape[0]), int(edges.shape[0]), int(uv_edges.shape[0])
        self.n_vertices, self.n_faces = fine_sizes(self.n_corner, self.n_edges, self.n_tri, self.level)
        self.n_uvs, _ = fine_sizes(self.n_uv_corner, self.n_uv_edges, self.n_tri, self.level)
        corner_owner = np.full(self.n_corner, -1, np.int32)
        named, first = np.unique(faces.reshape(-1), return_index=True)
        corner_owner[named] = first
        islands = projtex.uv_islands(face_obj)
        self._topology = (faces, uv_faces, np.array(face_obj.uvs, np.float64))
        self.dev = _lib.hip_device(device, "the tessellation", ValueError)
        put = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a, dtype)).to(self.dev)
        self._tri, self._uv_tri = put(faces, np.int32), put(uv_faces, np.int32)
        self._edges, self._uv_edges = put(edges, np.int32), put(uv_edges, np.int32)
        self._corner_owner = put(corner_owner, np.int32)
        self._tri_island = put(islands[uv_faces[:, 0]], np.int32)
        self._coarse_uvs = put(face_obj.uvs, np.float64).reshape(-1, 2)
        self._referenced = None if (corner_owner >= 0).all() else put(corner_owner >= 0, np.bool_)
        self._csr = None
        with torch.cuda.device(self.dev):
            self.faces = self._index_list(self._tri, put(tri_edge, np.int32), self.n_corner, self.n_edges)
            self.uv_faces = self._index_list(self._uv_tri, put(uv_tri_edge, np.int32), self.n_uv_corner, self.n_uv_edges)
            self.uvs = self._points(self._coarse_uvs, self._uv_edges, self._uv_tri, self.n_uvs)

    def _index_list(self, tri, tri_edge, n_corner: int, n_edges: int) -> torch.Tensor:
        out = torch.empty((self.n_faces, 3), dtype=torch.int32, device=self.dev)
        _lib.call("t4d_tess_faces", ptr(tri), ptr(tri_edge), self.n_tri, n_corner, n_edges, self.level, ptr(out), _lib.stream(self.dev))
        return out

    def _points(self, values, edges, tri, n_fine: int) -> torch.Tensor:
        dim = int(values.shape[1])
        out = torch.empty((n_fine, dim), dtype=torch.float64, device=self.dev)
        _lib.call("t4d_tess_points", ptr(values), dim, int(values.shape[0]), ptr(edges), int(edges.shape[0]), ptr(tri), self.n_tri,
                  self.level, ptr(out), _lib.stream(self.dev))
        return out

    def matches(self, face_obj, level: int = None) -> bool:
        """Is this the tessellation of `face_obj`'s topology (the same vertex count, triangulated faces, uv faces and uvs)?"""
        from . import meshrender
        if level is not None and int(level) != self.level:
            return False
        if len(face_obj.vertices) != self.n_corner or len(face_obj.uvs) != self.n_uv_corner:
            return False
        try:
            faces, uv_faces = meshrender.triangulate(face_obj.faces_ori, face_obj.uv_faces_ori)
        except ValueError:
            return False
        return np.array_equal(faces, self._topology[0]) and np.array_equal(uv_faces, self._topology[1]) and \
            np.array_equal(np.asarray(face_obj.uvs, np.float64), self._topology[2])

    def vertices(self, vertices) -> torch.Tensor:
        """float64 [M,3]: the flat tessellation of the mesh vertices (float64 [n,3], array or tensor): a corner is copied, an edge
        vertex is ((N - s) X_lo + s X_hi) / N, an interior one ((i A + j B) + k C) / N."""
        v = _vertices(vertices, self.n_corner, self.dev)
        with torch.cuda.device(self.dev):
            return self._points(v, self._edges, self._tri, self.n_vertices)

    def _normals(self, v: torch.Tensor) -> torch.Tensor:
        """objexport.vertex_normals of the mesh; a vertex in no face (which that function refuses) gets a zero normal, after the
        others' were taken on the mesh without it - they do not depend on it."""
        from . import objexport
        if self._csr is None:
            if self._referenced is None:
                self._csr = objexport._VertexFaces(self._tri, self.n_corner)
            else:
                new_id = torch.cumsum(self._referenced.to(torch.int32), 0, dtype=torch.int32) - 1
                self._csr = objexport._VertexFaces(new_id[self._tri.long()].contiguous(), int(self._referenced.sum()))
        if self._referenced is None:
            return self._csr.normals(v)
        out = torch.zeros_like(v)
        out[self._referenced] = self._csr.normals(v[self._referenced].contiguous())
        return out

    def displace(self, vertices, code: torch.Tensor, has: torch.Tensor, labels: torch.Tensor, unit: float):
        """(float64 [M,3], sampled uint8 [M]): the fine vertices of `vertices` (float64 [n,3]) displaced by the code map (int32
        [h,w]; has uint8 or bool, labels uint8: projtex.island_labels at the map's size) with `unit` scan units per code step.
        sampled is 0 where no tap counted (the vertex stays on the flat tessellation), or the normal was zero or anything was
        non-finite."""
        h, w = check_maps(code, has, labels)
        u = float(unit)
        if not math.isfinite(u):
            raise ValueError(f"unit must be finite, got {unit}")
        v = _vertices(vertices, self.n_corner, self.dev)
        c = on_device(code, "code", self.dev)
        m, lab = on_device(has, "has", self.dev), on_device(labels, "labels", self.dev)
        with torch.cuda.device(self.dev):
            normals = self._normals(v)
            out = torch.empty((self.n_vertices, 3), dtype=torch.float64, device=self.dev)
            sampled = torch.empty(self.n_vertices, dtype=torch.uint8, device=self.dev)
            _lib.call("t4d_tess_displace", ptr(v), ptr(normals), ptr(self._coarse_uvs), ptr(self._corner_owner), ptr(self._edges),
                      ptr(self._tri), ptr(self._uv_tri), ptr(self._tri_island), self.n_corner, self.n_uv_corner, self.n_edges,
                      self.n_tri, self.level, ptr(c), ptr(m), ptr(lab), h, w, u, ptr(out), ptr(sampled), _lib.stream(self.dev))
        return out, sampled


def displace_frame(face_obj, vertices, code: torch.Tensor, has: torch.Tensor, level: int, dist: float, device=None, tess=None) -> dict:
    """{"tess": Tessellation, "vertices": float64 [M,3], "sampled": uint8 [M]}: `face_obj` with `vertices` tessellated at `level`
    and displaced by a finished code map (dispmap.finish's "code" and "has") baked with the reach `dist`; the labels are
    projtex.island_labels at the map's size.  tess: a Tessellation to reuse when it matches the topology and the level."""
    from . import dispmap, projtex
    h, w = check_maps(code, has)                                # argument errors first, with or without a device
    n = check_level(level)
    dispmap.check_options(dist)
    if tess is None or not tess.matches(face_obj, n):
        tess = Tessellation(face_obj, n, device=device)
    dev = _lib.hip_device(device, "the tessellation", ValueError) if device is not None else tess.dev
    with torch.cuda.device(dev):
        labels = projtex.island_labels(face_obj, h, w, device=dev)
        fine, sampled = tess.displace(vertices, code.to(dev), has.to(dev), labels, dispmap.code_unit(dist))
    return {"tess": tess, "vertices": fine, "sampled": sampled}


def write_frame(frame_dir: str, tess: Tessellation, fine_vertices: torch.Tensor) -> str:
    """face_hi.obj in `frame_dir`: the fine vertices with the tessellation's uvs and index lists, as objexport.write_obj_with_uv
    writes them; returns the path."""
    from .objexport import write_obj_with_uv
    if not isinstance(fine_vertices, torch.Tensor) or fine_vertices.dtype != torch.float64 or \
            tuple(fine_vertices.shape) != (tess.n_vertices, 3):
        raise ValueError(f"fine_vertices must be a float64 [{tess.n_vertices},3] tensor, got "
                         f"{getattr(fine_vertices, 'dtype', type(fine_vertices))} {list(getattr(fine_vertices, 'shape', ()))}")
    path = os.path.join(frame_dir, OBJ_NAME)
    write_obj_with_uv(path, fine_vertices, tess.faces, tess.uvs, tess.uv_faces)
    return path


# ---- command line ----------------------------------------------------------------------------------------------------------
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m topo4d_amd.tessellate",
                                description="Apply every frame's face_disp.png to its face.obj: tessellate, displace, write face_hi.obj.")
    _run.add_run_flags(p, "exp", "seq", "output_dir", frames_help="Frames to displace: '1-10', '1,5,9' (default: every frame directory).")
    p.add_argument("--level", type=int, required=True, metavar="N", help=f"Segments per edge of the tessellation, 1..{MAX_LEVEL}.")
    p.add_argument("--dist", type=float, required=True, metavar="DIST", help="The reach the maps were baked with (evaluate --bake_disp).")
    p.add_argument("--use_hit", action="store_true",
                   help="Only the texels of face_disp_hit.png have a value (for maps that were not filled); default: every island texel.")
    return p


def apply_tree(args, device=None) -> list:
    """The files written for the run <od>/<exp>/<seq>; frames without face.obj or face_disp.png (with --use_hit: or
    face_disp_hit.png) are left alone."""
    from PIL import Image
    from . import dispmap, projtex, scanbake
    try:
        check_level(args.level)
        dispmap.check_options(args.dist)
    except ValueError as e:
        raise SystemExit(f"--level / --dist: {e}") from None
    dev = torch.device(device if device is not None else "cuda")
    run_dir = _run.run_dir_of(args)
    written, tess = [], None
    with torch.cuda.device(dev):
        for t in _run.frames_of(args, run_dir):
            paths = _run.frame_files(run_dir, t, "face.obj", dispmap.PNG_NAME, *((scanbake.HIT_NAME,) if args.use_hit else ()))
            if paths is None:
                continue
            frame_dir = _run.frame_dir(run_dir, t)
            obj = _run.read_frame_obj(frame_dir)
            png = np.array(Image.open(paths[1]))
            if png.dtype != np.uint16 or png.ndim != 2:
                raise SystemExit(f"{paths[1]}: not a 16-bit grey PNG")
            h, w = png.shape
            code = torch.from_numpy(png.astype(np.int32)).to(dev)
            if args.use_hit:
                hit = _run.read_hit_mask(paths[2])
                if hit.shape != (h, w):
                    raise SystemExit(f"{paths[2]}: not of {dispmap.PNG_NAME}'s size")
                has = torch.from_numpy(hit).to(dev)
            else:
                has = (projtex.island_labels(obj, h, w, device=dev) != 0).to(torch.uint8)
            result = displace_frame(obj, obj.vertices, code, has, args.level, args.dist, device=dev, tess=tess)
            tess = result["tess"]
            written.append(write_frame(frame_dir, tess, result["vertices"]))
    return written


def main(argv=None) -> None:
    _run.print_written(apply_tree(build_parser().parse_args(argv)))


if __name__ == "__main__":
    main()
