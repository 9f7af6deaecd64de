"""
A frame's exported mesh scored against that frame's 3D scan (the multi-view-stereo mesh or cloud the capture's Metashape
project exports), on the GPU.

    read_scan(path)                               PLY (ascii / binary_little_endian) or OBJ -> Scan(vertices, faces | None)
    ClosestPointIndex(vertices, faces=None)       grid index on the device; .query(points, max_dist) -> (d2, index, closest),
                                                  .raycast(origins, dirs, t_lo, t_hi) -> (t, prim, uv)
    score_scan(mesh_vertices, mesh_faces, scan)   scan -> mesh (accuracy) and mesh -> scan (completeness) statistics

over `t4d_closest_build` / `t4d_closest_query` / `t4d_closest_signed` / `t4d_closest_raycast` (include/topo4d_raster.h,
csrc/t4d_closest.hip).  The rules of the query and of the ray cast are fixed there so that tests/scanscore_ref.py and
tests/scanray_ref.py (numpy, float64) reproduce every output bit.  The statistics are
torch reductions over the per-query output (a full-size direction is 2 million doubles: a sort and five sums, about as fast as a
kernel of our own would be, and torch's sum uses no atomics, so two runs agree to the bit).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import T4D_ERR_PAIR_OVERFLOW, T4D_OK, ptr

T4D_CLOSEST_INPUT_ORDER = 1
T4D_RAY_SAME_SIDE = 2
DEFAULT_THRESHOLDS = (0.5, 1.0, 2.0)


class Scan(NamedTuple):
    vertices: np.ndarray                # float64 [N,3]
    faces: Optional[np.ndarray]         # int32 [F,3], or None for a bare cloud


# ---- readers ----------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _fan(polys, path) -> Optional[np.ndarray]:
    tri = []
    for p in polys:
        for k in range(1, len(p) - 1):
            tri.append((p[0], p[k], p[k + 1]))
    return np.asarray(tri, np.int32).reshape(-1, 3) if tri else None


def _finish(path, vertices, faces) -> Scan:
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    if len(v) == 0:
        raise ValueError(f"{path}: no vertices")
    bad = int((~np.isfinite(v)).sum())
    if bad:
        raise ValueError(f"{path}: {bad} non-finite vertex coordinates")
    if faces is not None and len(faces):
        f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
        if f.min() < 0 or f.max() >= len(v):
            k = int(np.nonzero(((f < 0) | (f >= len(v))).any(1))[0][0])
            raise ValueError(f"{path}: face {k} has a vertex index outside 0..{len(v) - 1}")
        return Scan(v, f.astype(np.int32))
    return Scan(v, None)


def _read_ply(path) -> Scan:
    with open(path, "rb") as fh:
        data = fh.read()
    if not data.startswith(b"ply"):
        raise ValueError(f"{path}: byte 0: not a PLY file")
    end = data.find(b"end_header")
    nl = data.find(b"\n", end) if end >= 0 else -1
    if end < 0 or nl < 0:
        raise ValueError(f"{path}: truncated: no end_header line")
    fmt, elements = None, []
    for lineno, line in enumerate(data[:end].decode("ascii", "replace").splitlines(), 1):
        w = line.split()
        if not w or w[0] in ("ply", "comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1] if len(w) > 1 else None
        elif w[0] == "element" and len(w) == 3:
            elements.append({"name": w[1], "count": int(w[2]), "props": []})
        elif w[0] == "property" and elements:
            if w[1] == "list" and len(w) == 5:
                kinds = (w[2], w[3])
            elif len(w) == 3:
                kinds = (w[1],)
            else:
                raise ValueError(f"{path}:{lineno}: malformed property line")
            if any(k not in _PLY_TYPES for k in kinds):
                raise ValueError(f"{path}:{lineno}: unknown property type in '{line.strip()}'")
            elements[-1]["props"].append((w[-1], kinds))
        else:
            raise ValueError(f"{path}:{lineno}: unexpected header line '{line.strip()}'")
    if fmt == "binary_big_endian":
        raise ValueError(f"{path}: big-endian PLY is not supported (ascii and binary_little_endian are)")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unknown PLY format {fmt!r}")
    body = nl + 1
    vertices, faces = None, None
    if fmt == "ascii":
        lines = data[body:].decode("ascii", "replace").splitlines()
        header_lines = data[:body].count(b"\n")
        row = 0
        for el in elements:
            if row + el["count"] > len(lines):
                raise ValueError(f"{path}:{header_lines + len(lines) + 1}: truncated: element '{el['name']}' needs {el['count']} "
                                 f"lines, {len(lines) - row} are left")
            rows = lines[row:row + el["count"]]
            if el["name"] == "vertex":
                names = [n for n, _ in el["props"]]
                if any(len(k) != 1 for _, k in el["props"]) or not all(c in names for c in "xyz"):
                    raise ValueError(f"{path}: the vertex element needs scalar x, y, z properties")
                cols = [names.index(c) for c in "xyz"]
                try:
                    tab = np.array([r.split() for r in rows], dtype=object)
                    vertices = np.array(tab[:, cols], dtype=np.float64) if el["count"] else np.zeros((0, 3))
                except (ValueError, IndexError):
                    for k, r in enumerate(rows):
                        w = r.split()
                        try:
                            [float(w[c]) for c in cols]
                        except (ValueError, IndexError):
                            raise ValueError(f"{path}:{header_lines + row + k + 1}: not a vertex line: '{r.strip()}'") from None
                    raise
            elif el["name"] == "face":
                lp = [i for i, (n, k) in enumerate(el["props"]) if len(k) == 2 and n in ("vertex_indices", "vertex_index")]
                if not lp or lp[0] != 0:
                    raise ValueError(f"{path}: the face element needs a leading vertex_indices list")
                polys = []
                for k, r in enumerate(rows):
                    w = r.split()
                    try:
                        n = int(w[0])
                        poly = [int(x) for x in w[1:1 + n]]
                        if len(poly) != n:
                            raise IndexError
                    except (ValueError, IndexError):
                        raise ValueError(f"{path}:{header_lines + row + k + 1}: not a face line: '{r.strip()}'") from None
                    polys.append(poly)
                faces = _fan(polys, path)
            row += el["count"]
    else:
        off = body
        for el in elements:
            listy = [len(k) == 2 for _, k in el["props"]]
            if not any(listy):
                dt = np.dtype([(n, "<" + _PLY_TYPES[k[0]]) for n, k in el["props"]])
                need = dt.itemsize * el["count"]
                if off + need > len(data):
                    raise ValueError(f"{path}: truncated at byte {len(data)}: element '{el['name']}' ends at byte {off + need}")
                if el["name"] == "vertex":
                    if not all(c in dt.names for c in "xyz"):
                        raise ValueError(f"{path}: the vertex element needs scalar x, y, z properties")
                    tab = np.frombuffer(data, dt, el["count"], off)
                    vertices = np.stack([tab[c].astype(np.float64) for c in "xyz"], 1)
                off += need
                continue
            if el["name"] == "vertex":
                raise ValueError(f"{path}: the vertex element needs scalar x, y, z properties")
            is_face = el["name"] == "face" and el["props"] and len(el["props"][0][1]) == 2 and \
                el["props"][0][0] in ("vertex_indices", "vertex_index")
            if el["name"] == "face" and not is_face:
                raise ValueError(f"{path}: the face element needs a leading vertex_indices list")
            if is_face and len(el["props"]) == 1 and el["count"] > 0:
                ct, it = (np.dtype("<" + _PLY_TYPES[k]) for k in el["props"][0][1])
                dt = np.dtype([("n", ct), ("i", it, (3,))])
                if off + dt.itemsize * el["count"] <= len(data):
                    tab = np.frombuffer(data, dt, el["count"], off)
                    if (tab["n"] == 3).all():                            # every face a triangle: one vectorised read
                        faces = tab["i"].astype(np.int64)
                        off += dt.itemsize * el["count"]
                        continue
            polys = []
            for k in range(el["count"]):                                # general lists, row by row
                for j, (n, kinds) in enumerate(el["props"]):
                    if len(kinds) == 1:
                        size = np.dtype(_PLY_TYPES[kinds[0]]).itemsize
                        if off + size > len(data):
                            raise ValueError(f"{path}: truncated at byte {len(data)} inside {el['name']} {k}")
                        off += size
                        continue
                    ct, it = (np.dtype("<" + _PLY_TYPES[x]) for x in kinds)
                    if off + ct.itemsize > len(data):
                        raise ValueError(f"{path}: truncated at byte {len(data)} inside {el['name']} {k}")
                    cnt = int(np.frombuffer(data, ct, 1, off)[0])
                    off += ct.itemsize
                    if off + cnt * it.itemsize > len(data):
                        raise ValueError(f"{path}: truncated at byte {len(data)} inside {el['name']} {k}")
                    if is_face and j == 0:
                        polys.append(np.frombuffer(data, it, cnt, off).astype(np.int64).tolist())
                    off += cnt * it.itemsize
            if is_face:
                faces = _fan(polys, path)
    if vertices is None:
        raise ValueError(f"{path}: no vertex element")
    return _finish(path, vertices, faces)


def _read_obj(path) -> Scan:
    verts, pending = [], []
    with open(path, "r") as f:
        for lineno, line in enumerate(f, 1):
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                try:
                    verts.append((float(w[1]), float(w[2]), float(w[3])))
                except (ValueError, IndexError):
                    raise ValueError(f"{path}:{lineno}: a 'v' line needs x, y and z") from None
            elif w[0] == "f":
                if len(w) < 4:
                    raise ValueError(f"{path}:{lineno}: a face of {len(w) - 1} corners")
                pending.append((lineno, len(verts), w[1:]))
    polys = []
    for lineno, seen, corners in pending:                         # (a positive index may name a line further down)
        poly = []
        for c in corners:
            s = c.split("/")[0]
            try:
                i = int(s)
            except ValueError:
                raise ValueError(f"{path}:{lineno}: corner '{c}' has no vertex index") from None
            k = i - 1 if i > 0 else seen + i
            if i == 0 or not 0 <= k < len(verts):
                raise ValueError(f"{path}:{lineno}: vertex index {i} outside 1..{len(verts)}")
            poly.append(k)
        polys.append(poly)
    return _finish(path, np.asarray(verts, np.float64).reshape(-1, 3), _fan(polys, path))


def read_scan(path) -> Scan:
    """Read a scan: PLY (ascii or binary_little_endian; vertex x y z as float or double, other vertex properties skipped, an
    optional face element with a vertex_indices / vertex_index list) or OBJ ('v', and 'f' corners as a, a/b, a/b/c, a//c, negative
    indices counted back from the face's line).  Polygons are fanned (0,k,k+1).  ValueError names the file and the line or byte for
    a truncated file, a big-endian PLY, an index out of range, and states the count of non-finite coordinates."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".ply":
        return _read_ply(path)
    if ext == ".obj":
        return _read_obj(path)
    raise ValueError(f"{path}: not a .ply or .obj file")


# ---- the index --------------------------------------------------------------------------------------------------------------
_WHAT = "the closest-point query"


def _points(x, what: str, dev) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1 or not t.is_floating_point():
        raise ValueError(f"{what} must be a floating-point [N,3] array with N >= 1, got {t.dtype} {tuple(t.shape)}")
    if t.dtype != torch.float64:
        raise ValueError(f"{what} must be float64 (the query is exact in float64), got {t.dtype}")
    return t.detach().to(dev).contiguous()


class ClosestPointIndex:
    """Grid index over triangles (vertices float64 [N,3], faces integer [F,3]) or, without faces, over the points themselves.
    Built once, reusable across queries; holds its own copy of the primitives.  ValueError for wrong shapes / dtypes, non-finite
    vertices, or a face index beyond the vertices."""

    def __init__(self, vertices, faces=None, device=None):
        self.dev = _lib.hip_device(device, _WHAT, ValueError)
        v = _points(vertices, "vertices", self.dev)
        if not bool(torch.isfinite(v).all()):
            raise ValueError("vertices hold non-finite coordinates")
        f = None
        if faces is not None:
            ft = faces if isinstance(faces, torch.Tensor) else torch.as_tensor(np.asarray(faces))
            if ft.dim() != 2 or ft.shape[1] != 3 or ft.is_floating_point() or ft.dtype == torch.bool:
                raise ValueError(f"faces must be an integer [F,3] array, got {ft.dtype} {tuple(ft.shape)}")
            if ft.shape[0] > 0:
                if int(ft.min()) < 0 or int(ft.max()) >= v.shape[0]:
                    raise ValueError(f"faces hold an index outside [0, {v.shape[0]})")
                f = ft.to(self.dev).to(torch.int32).contiguous()
        self.n_vert = int(v.shape[0])
        self.n_faces = 0 if f is None else int(f.shape[0])
        self.n_prims = self.n_faces or self.n_vert
        self.is_tri = f is not None
        with torch.cuda.device(self.dev):
            bbox = torch.cat([v.amin(0), v.amax(0)]).cpu().numpy()
            extent = 0.0
            if f is not None:
                corners = v[f.long()]                                 # [F,3,3]
                extent = float((corners.amax(1) - corners.amin(1)).amax(1).mean())
            bb = (C.c_double * 6)(*bbox.tolist())
            self.mean_extent = extent                                 # (what fixed the grid, with the vertices' box)
            capacity = 16 * self.n_prims + 1024
            lib = _lib.load()
            for _ in range(3):
                nbytes = lib.t4d_closest_index_bytes(self.n_vert, self.n_faces, bb, extent, capacity)
                if nbytes == 0:
                    raise _lib.error("t4d_closest_index_bytes", exc=ValueError)
                self._index = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
                needed = C.c_int64(0)
                rc = lib.t4d_closest_build(ptr(v), self.n_vert, ptr(f), self.n_faces, bb, extent, ptr(self._index), nbytes, capacity,
                                           C.byref(needed), _lib.stream(self.dev))
                if rc == T4D_OK:
                    break
                if rc != T4D_ERR_PAIR_OVERFLOW:
                    raise _lib.error("t4d_closest_build", rc)
                capacity = int(needed.value)
            else:
                raise _lib.error("t4d_closest_build", rc)
        self.entries = int(needed.value)
        self._scratch = None

    def _query_scratch(self, n: int) -> torch.Tensor:
        self._scratch = _lib.scratch("t4d_closest_query_scratch_bytes", self.dev, n, reuse=self._scratch)[0]
        return self._scratch

    def query(self, points, max_dist: Optional[float] = None, input_order: bool = False):
        """(d2 float64 [Q], index int32 [Q], closest float64 [Q,3]) on the device.  max_dist (file units): a query farther than
        that from every primitive is unmatched (index -1, d2 +inf, closest 0).  input_order walks the queries as given instead of
        grouped by cell: the same results, for measurement."""
        p = _points(points, "points", self.dev)
        if not bool(torch.isfinite(p).all()):
            raise ValueError("points hold non-finite coordinates")
        if max_dist is not None and not (float(max_dist) >= 0.0):
            raise ValueError(f"max_dist must be >= 0 or None, got {max_dist}")
        q = int(p.shape[0])
        d2 = torch.empty(q, dtype=torch.float64, device=self.dev)
        idx = torch.empty(q, dtype=torch.int32, device=self.dev)
        closest = torch.empty((q, 3), dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            s = self._query_scratch(q)
            _lib.call("t4d_closest_query", ptr(self._index), self._index.numel(), ptr(p), q,
                      -1.0 if max_dist is None else float(max_dist), T4D_CLOSEST_INPUT_ORDER if input_order else 0,
                      ptr(d2), ptr(idx), ptr(closest), ptr(s), s.numel(), _lib.stream(self.dev))
        return d2, idx, closest

    def raycast(self, origins, dirs, t_lo: float, t_hi: float, same_side: bool = False, input_order: bool = False):
        """(t float64 [R], prim int32 [R], uv float64 [R,2]) on the device: per ray o + t d the triangle met at the smallest |t|
        within [t_lo, t_hi] (then t >= 0 before t < 0, then the lowest index), by the hit rule of include/topo4d_raster.h; the hit
        is a + u (b - a) + v (c - a).  A miss is t = 0, prim = -1, uv = 0; a ray with a non-finite origin or direction, an all-zero
        direction, or t_lo > t_hi misses everything.  same_side: only triangles whose normal points along d count.  input_order
        as in query.  ValueError for an index built without faces, wrong shapes or dtypes, and limits that are not finite."""
        if not self.is_tri:
            raise ValueError("raycast needs an index built with faces: a ray meets only triangles")
        o = _points(origins, "origins", self.dev)
        d = _points(dirs, "dirs", self.dev)
        if o.shape != d.shape:
            raise ValueError(f"origins and dirs must have one shape, got {tuple(o.shape)} and {tuple(d.shape)}")
        t_lo, t_hi = float(t_lo), float(t_hi)
        if not (math.isfinite(t_lo) and math.isfinite(t_hi) and math.isfinite(t_hi - t_lo)):
            raise ValueError(f"t_lo and t_hi must be finite with a finite difference, got {t_lo} and {t_hi}")
        r = int(o.shape[0])
        t = torch.empty(r, dtype=torch.float64, device=self.dev)
        prim = torch.empty(r, dtype=torch.int32, device=self.dev)
        uv = torch.empty((r, 2), dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            s = self._query_scratch(r)
            _lib.call("t4d_closest_raycast", ptr(self._index), self._index.numel(), ptr(o), ptr(d), r, t_lo, t_hi,
                      (T4D_RAY_SAME_SIDE if same_side else 0) | (T4D_CLOSEST_INPUT_ORDER if input_order else 0),
                      ptr(t), ptr(prim), ptr(uv), ptr(s), s.numel(), _lib.stream(self.dev))
        return t, prim, uv

    def signed_distance(self, points, d2, index, closest) -> torch.Tensor:
        """float64 [Q]: sqrt(d2) with the sign of (p - closest) . n of the chosen triangle; 0 for points and unmatched queries."""
        p = _points(points, "points", self.dev)
        q = int(p.shape[0])
        if tuple(d2.shape) != (q,) or tuple(index.shape) != (q,) or tuple(closest.shape) != (q, 3) or d2.dtype != torch.float64 or \
                index.dtype != torch.int32 or closest.dtype != torch.float64:
            raise ValueError("signed_distance: d2 / index / closest are not a query's output for these points")
        out = torch.empty(q, dtype=torch.float64, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.call("t4d_closest_signed", ptr(self._index), self._index.numel(), ptr(p), q, ptr(d2.contiguous()),
                      ptr(index.contiguous()), ptr(closest.contiguous()), ptr(out), _lib.stream(self.dev))
        return out


# ---- statistics -------------------------------------------------------------------------------------------------------------
def direction_stats(d2: torch.Tensor, index: torch.Tensor, signed: torch.Tensor, thresholds: Sequence[float], unit: float = 1.0) -> dict:
    """count, unmatched, mean, rms, median (lower), p90, max, signed_mean, within, over the matched queries, in unit x file units."""
    m = index >= 0
    n = int(m.sum())
    out = {"count": n, "unmatched": int(index.numel()) - n}
    if n == 0:
        return out
    d = torch.sqrt(d2[m]) * unit
    srt = torch.sort(d).values
    picks = torch.stack([srt[(n - 1) // 2], srt[min(n - 1, -(-9 * n // 10) - 1)], srt[-1], d.sum(), (d * d).sum(),
                         (signed[m] * unit).sum()]).cpu().tolist()
    out["mean"] = picks[3] / n
    out["rms"] = math.sqrt(picks[4] / n)
    out["median"], out["p90"], out["max"] = picks[0], picks[1], picks[2]
    out["signed_mean"] = picks[5] / n
    under = torch.stack([(d <= float(t)).sum() for t in thresholds]).cpu().tolist() if len(thresholds) else []
    out["within"] = {repr(float(t)): c / n for t, c in zip(thresholds, under)}
    return out


def shoot_normals(target: ClosestPointIndex, mesh_vertices: torch.Tensor, mesh_faces, dist: float):
    """raycast of `target` from every mesh vertex (float64 [N,3], on the device) along its objexport.vertex_normals normal, within
    -dist .. +dist: (t, prim, uv).  The normals are of unit length up to rounding, so t is a distance in file units."""
    from . import objexport
    return target.raycast(mesh_vertices, objexport.vertex_normals(mesh_vertices, mesh_faces), -dist, dist)


def score_scan(mesh_vertices, mesh_faces, scan: Scan, max_dist: Optional[float] = None,
               thresholds: Sequence[float] = DEFAULT_THRESHOLDS, unit: float = 1.0, device=None, per_element: bool = False,
               shoot: Optional[float] = None) -> dict:
    """{"scan_to_mesh": {...}, "mesh_to_scan": {...}}: every scan vertex against the mesh triangles (accuracy), every mesh vertex
    against the scan's triangles, or its points when it has no faces (completeness).  max_dist in file units; thresholds and every
    reported distance in unit x file units.  per_element adds "arrays": face_count int64 [F] and face_mean float64 [F] (scan
    points that landed on each mesh face and their mean distance, NaN where none) and vertex_dist float64 [N] (mesh_to_scan per
    mesh vertex, +inf where unmatched), numpy.  shoot (file units, needs a scan with faces) adds "mesh_to_scan_normal": every mesh
    vertex shot along its objexport.vertex_normals normal, both ways, within shoot; the statistics are direction_stats over |t|
    with the sign of t, and "unmatched" counts the vertices whose ray met nothing."""
    if len(thresholds) > 8:
        raise ValueError("at most 8 thresholds")
    if shoot is not None and not (math.isfinite(float(shoot)) and float(shoot) >= 0.0):
        raise ValueError(f"shoot must be a finite distance >= 0 or None, got {shoot}")
    if shoot is not None and (scan.faces is None or len(scan.faces) == 0):
        raise ValueError("shoot needs a scan with faces: a ray meets only triangles")
    dev = _lib.hip_device(device, _WHAT, ValueError)
    mv = _points(torch.as_tensor(np.asarray(mesh_vertices, np.float64)) if not isinstance(mesh_vertices, torch.Tensor) else mesh_vertices,
                 "mesh_vertices", dev)
    sv = _points(torch.from_numpy(np.ascontiguousarray(scan.vertices, np.float64)), "scan vertices", dev)
    mesh = ClosestPointIndex(mv, mesh_faces, device=dev)
    if not mesh.is_tri:
        raise ValueError("mesh_faces: the mesh needs at least one triangle")
    target = ClosestPointIndex(sv, scan.faces, device=dev)
    out = {}
    d2, idx, cl = mesh.query(sv, max_dist)
    out["scan_to_mesh"] = direction_stats(d2, idx, mesh.signed_distance(sv, d2, idx, cl), thresholds, unit)
    e2, jdx, cm = target.query(mv, max_dist)
    out["mesh_to_scan"] = direction_stats(e2, jdx, target.signed_distance(mv, e2, jdx, cm), thresholds, unit)
    if shoot is not None:
        t, prim, _ = shoot_normals(target, mv, mesh_faces, float(shoot))
        out["mesh_to_scan_normal"] = direction_stats(t * t, prim, t, thresholds, unit)
    if per_element:
        m = idx >= 0
        hit = idx[m].long()
        count = torch.bincount(hit, minlength=mesh.n_faces)
        total = torch.bincount(hit, weights=torch.sqrt(d2[m]) * unit, minlength=mesh.n_faces)
        out["arrays"] = {"face_count": count.cpu().numpy(), "face_mean": (total / count).cpu().numpy(),
                         "vertex_dist": (torch.sqrt(e2) * unit).cpu().numpy()}
    return out
