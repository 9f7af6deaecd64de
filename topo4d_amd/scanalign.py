"""
A frame's 3D scan aligned rigidly (or by a similarity) to that frame's mesh before it is scored: iterated closest points on the GPU.

    align_scan(mesh_vertices, mesh_faces, scan, ...) -> Alignment      the 4x4 that takes scan coordinates to mesh coordinates
    transform_points(points, matrix, out=None)                          M p + t on the device (t4d_align_transform)
    accumulate(index, points, d2, prim, closest, origin, gate2, cos2)   the pairs of one query as one record (t4d_align_accumulate)
    solve_plane(record) / solve_point(record, with_scale) / rodrigues(w)   the host half: numpy float64 on one record

over `t4d_closest_query` (scanscore.ClosestPointIndex) and `t4d_align_transform` / `t4d_align_accumulate`
(include/topo4d_raster.h, csrc/t4d_align.hip).  The mesh index is built once: the scan moves, the mesh does not.  Per iteration
the scan's points are moved from their original coordinates by the current pose (no drift builds up), queried, and reduced on the
device into one record of 51 doubles, which is all that is read back; the 6x6 or 3x3 solve is numpy on the host.  The device
half is a function of its inputs alone and tests/scanalign_ref.py restates it bit for bit.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import ptr
from .scanscore import ClosestPointIndex, Scan, _points

RECORD = 51                                                     # T4D_ALIGN_RECORD_DOUBLES and the offsets of the header
COUNT, SUM_D2, SUM_R2, JTR, JTJ, SUM_Q, SUM_G, SUM_QG, SUM_QQ, SUM_GG = 0, 5, 6, 7, 13, 34, 37, 40, 49, 50
CLASSES = ("unmatched", "gated", "degenerate", "off_normal", "kept")
METRICS = ("plane", "point")
MIN_PAIRS = 6
SINGULAR = 1e-12                                                # smallest / largest eigenvalue (singular value) of a system that is solved
_WHAT = "the scan alignment"


class Alignment(NamedTuple):
    matrix: np.ndarray                  # float64 [4,4]: scan coordinates -> mesh coordinates, `init` included
    scale: float                        # cbrt(det) of its 3x3 part
    iterations: int
    converged: bool                     # every phase stopped by its tolerance, none by max_iter
    counts: dict                        # the classes of the last evaluation, at the returned pose
    rms_before: float                   # point-to-surface rms over the kept pairs at the initial pose
    rms_after: float                    # and at the returned one
    rotation_deg: float                 # the angle of the 3x3 part's rotation
    translation: np.ndarray             # float64 [3]

    def as_dict(self) -> dict:
        return {"matrix": self.matrix.tolist(), "scale": self.scale, "iterations": self.iterations, "converged": self.converged,
                "counts": dict(self.counts), "rms_before": self.rms_before, "rms_after": self.rms_after,
                "rotation_deg": self.rotation_deg, "translation": self.translation.tolist()}


# ---- the device half --------------------------------------------------------------------------------------------------------
def _matrix12(matrix) -> np.ndarray:
    m = np.asarray(matrix, np.float64)
    if m.shape == (4, 4):
        if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("a 4x4 matrix must end in the row 0 0 0 1")
        m = m[:3]
    if m.shape != (3, 4) or not np.isfinite(m).all():
        raise ValueError(f"the matrix must be a finite 3x4 or 4x4 array, got shape {m.shape}")
    return np.ascontiguousarray(m)


def transform_points(points: torch.Tensor, matrix, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [Q,3] on the device: M p + t per point, each component ((m0 x + m1 y) + m2 z) + t with every product and sum
    rounded.  matrix: [M | t] as 3x4, or a 4x4 ending in 0 0 0 1.  out: a tensor to write (it may be `points`)."""
    m = _matrix12(matrix)
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float64:
        raise ValueError("points must be a float64 [Q,3] tensor")
    p = _lib.on_device(points, "points")
    if out is None:
        out = torch.empty_like(p)
    elif out.shape != p.shape or out.dtype != torch.float64 or out.device != p.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous float64 tensor of the points' shape on their device")
    with torch.cuda.device(p.device):
        _lib.call("t4d_align_transform", ptr(p), int(p.shape[0]), (C.c_double * 12)(*m.reshape(-1).tolist()), ptr(out),
                  _lib.stream(p.device))
    return out


def accumulate(index: ClosestPointIndex, points: torch.Tensor, d2: torch.Tensor, prim: torch.Tensor, closest: torch.Tensor, origin,
               gate2: float = -1.0, cos2: float = 0.0, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [51] on the device: the record of include/topo4d_raster.h over the pairs (points[i], closest[i]) that
    index.query(points) gave.  gate2 < 0: no gate.  ValueError for an index without faces and for tensors that are not a query's."""
    if not index.is_tri:
        raise ValueError("the alignment needs an index built with faces: its residual is taken along the triangle's normal")
    q = int(points.shape[0]) if isinstance(points, torch.Tensor) and points.dim() == 2 else -1
    if q < 0 or tuple(points.shape) != (q, 3) or tuple(d2.shape) != (q,) or tuple(prim.shape) != (q,) or tuple(closest.shape) != (q, 3) or \
            points.dtype != torch.float64 or d2.dtype != torch.float64 or prim.dtype != torch.int32 or closest.dtype != torch.float64:
        raise ValueError("accumulate: points / d2 / prim / closest are not a query's input and output")
    o = np.asarray(origin, np.float64).reshape(-1)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("origin must hold three finite numbers")
    gate2, cos2 = float(gate2), float(cos2)
    if not math.isfinite(gate2) or not (0.0 <= cos2 <= 1.0):
        raise ValueError(f"need a finite gate2 and 0 <= cos2 <= 1, got {gate2} and {cos2}")
    dev = index.dev
    tensors = [_lib.on_device(t, n, dev, "the index's") for t, n in ((points, "points"), (d2, "d2"), (prim, "prim"), (closest, "closest"))]
    record = torch.empty(RECORD, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        s, nbytes = _lib.scratch("t4d_align_scratch_bytes", dev, q, reuse=scratch)
        _lib.call("t4d_align_accumulate", ptr(index._index), index._index.numel(), ptr(tensors[0]), q, ptr(tensors[1]), ptr(tensors[2]),
                  ptr(tensors[3]), (C.c_double * 3)(*o.tolist()), gate2, cos2, ptr(record), ptr(s), s.numel(), _lib.stream(dev))
    return record


# ---- the host half ----------------------------------------------------------------------------------------------------------
def rodrigues(w) -> np.ndarray:
    """The rotation by |w| radians about w, exactly orthonormal up to rounding: I + sin(t) K + (1 - cos(t)) K K, K = [w / |w|]x."""
    w = np.asarray(w, np.float64).reshape(3)
    theta = math.sqrt(float((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]))
    if theta == 0.0:
        return np.eye(3)
    k = w / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)


def kept_pairs(record) -> int:
    n = int(record[COUNT + 4])
    if n < MIN_PAIRS:
        raise ValueError(f"only {n} pairs are kept ({dict(zip(CLASSES, (int(x) for x in record[COUNT:COUNT + 5])))}): an alignment needs "
                         f"at least {MIN_PAIRS}")
    return n


def solve_plane(record):
    """(R, u): the point-to-plane Gauss-Newton step of a record, about the record's origin: x -> R x + u, R = rodrigues(w), with
    (w, u) the solution of (sum J^T J) (w, u) = -(sum r J).  ValueError for fewer than 6 kept pairs and for a singular system (a
    flat or rotationally symmetric surface leaves a motion undetermined)."""
    record = np.asarray(record, np.float64)
    kept_pairs(record)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = record[JTJ:JTJ + 21]
    A = A + A.T - np.diag(np.diag(A))
    ev = np.linalg.eigvalsh(A)
    if not (np.isfinite(ev).all() and ev[0] > SINGULAR * ev[-1]):
        raise ValueError(f"the point-to-plane system is singular (eigenvalues {ev[0]:.3g} .. {ev[-1]:.3g})")
    x = np.linalg.solve(A, -record[JTR:JTR + 6])
    return rodrigues(x[:3]), x[3:].copy()


def solve_point(record, with_scale: bool = False):
    """(c, R, u): the least-squares similarity (Umeyama; Kabsch with c = 1 when with_scale is False) of a record's kept pairs, about
    the record's origin: x -> c R x + u.  The determinant fix keeps R a rotation.  ValueError for fewer than 6 kept pairs and
    for points that lie on a line."""
    record = np.asarray(record, np.float64)
    n = kept_pairs(record)
    qm, gm = record[SUM_Q:SUM_Q + 3] / n, record[SUM_G:SUM_G + 3] / n
    cov = record[SUM_QG:SUM_QG + 9].reshape(3, 3) / n - np.outer(qm, gm)          # [i][j]: q_i g_j about the means
    var = record[SUM_QQ] / n - float(qm @ qm)
    U, D, Vt = np.linalg.svd(cov.T)
    if not (np.isfinite(D).all() and var > 0.0 and D[1] > SINGULAR * D[0]):
        raise ValueError(f"the point-to-point system is singular (singular values {D[0]:.3g} {D[1]:.3g} {D[2]:.3g})")
    d = 1.0 if np.linalg.det(U) * np.linalg.det(Vt) >= 0.0 else -1.0
    R = U @ np.diag([1.0, 1.0, d]) @ Vt
    c = float((D[0] + D[1]) + d * D[2]) / var if with_scale else 1.0
    return c, R, gm - c * (R @ qm)


def step_of(record, metric: str, with_scale: bool, origin):
    """(A, b) of the update x -> A x + b in mesh coordinates that a record asks for (its own solve is about `origin`)."""
    if metric == "plane" and not with_scale:
        R, u = solve_plane(record)
        A = R
    else:
        c, R, u = solve_point(record, with_scale)
        A = c * R
    o = np.asarray(origin, np.float64)
    return A, (o - A @ o) + u


def describe(matrix):
    """(scale, rotation angle in degrees, translation) of a 4x4 whose 3x3 part is a scaled rotation."""
    M = np.asarray(matrix, np.float64)[:3, :3]
    scale = float(np.cbrt(np.linalg.det(M)))
    cosang = (np.trace(M) / scale - 1.0) / 2.0 if scale != 0.0 else 1.0
    return scale, math.degrees(math.acos(min(1.0, max(-1.0, float(cosang))))), np.asarray(matrix, np.float64)[:3, 3].copy()


def check_options(metric="plane", max_iter=30, max_dist=None, gate_sigma=3.0, normal_cos=0.5, tol=1e-6, stride=1) -> None:
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {', '.join(METRICS)}, got {metric!r}")
    if not (isinstance(max_iter, (int, np.integer)) and 1 <= max_iter <= 1000):
        raise ValueError(f"max_iter must be an integer in 1..1000, got {max_iter!r}")
    if not (isinstance(stride, (int, np.integer)) and stride >= 1):
        raise ValueError(f"stride must be an integer >= 1, got {stride!r}")
    if max_dist is not None and not (math.isfinite(float(max_dist)) and float(max_dist) >= 0.0):
        raise ValueError(f"max_dist must be a finite distance >= 0 or None, got {max_dist}")
    if not (math.isfinite(float(gate_sigma)) and float(gate_sigma) > 0.0):
        raise ValueError(f"gate_sigma must be finite and > 0, got {gate_sigma}")
    if not (0.0 <= float(normal_cos) <= 1.0):
        raise ValueError(f"normal_cos must lie in [0, 1], got {normal_cos}")
    if not (math.isfinite(float(tol)) and float(tol) >= 0.0):
        raise ValueError(f"tol must be finite and >= 0, got {tol}")


def box_corners(vertices: np.ndarray) -> np.ndarray:
    lo, hi = vertices.min(0), vertices.max(0)
    return np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])


def align_scan(mesh_vertices, mesh_faces, scan, *, init=None, metric: str = "plane", scale: bool = False, max_iter: int = 30,
               max_dist: Optional[float] = None, gate_sigma: float = 3.0, normal_cos: float = 0.5, tol: float = 1e-6, stride: int = 1,
               device=None) -> Alignment:
    """The transform that takes `scan` (a scanscore.Scan, or float64 [N,3] points) onto the mesh (float64 [V,3], integer [F,3]).

    init: a 4x4 applied first, the starting pose (any invertible 3x3 part: a change of unit belongs here); the result includes
    it.  metric: "plane" minimises the residuals along the mesh normals (Gauss-Newton on 6 parameters, the rotation vector turned
    into an exact Rodrigues rotation), "point" the distances to the closest points (Kabsch by SVD).  scale: first similarity
    iterations (Umeyama) until they converge, then `metric` iterations with the scale held; each phase runs up to max_iter
    iterations.  Every stride-th scan point is used.

    Pairs: the first evaluation leaves out the pairs farther apart than max_dist (file units; None: none); every later one those
    beyond min(max_dist, gate_sigma x the rms distance of the kept pairs before it).  A pair whose residual makes an angle with
    the triangle's normal of cosine below normal_cos is left out as well: a scan point beyond an open rim of the mesh (neck,
    hairline, ears) has its closest point on the rim and says nothing about the surface.  Zero-area triangles are left out.

    Stop: when an update moves no corner of the mesh's bounding box by more than tol x its diagonal (converged), or at max_iter; with scale=True `converged` says so of
    both phases.  The similarity phase closes in on a scale only linearly (measured on a 200-triangle test surface: a scale 7 % off
    is 0.8 % off after 100 iterations and 0.2 % after 400), so with the default max_iter it ends unconverged on anything but a small
    scale error: a change of unit belongs in init.
    One more evaluation at the returned pose gives counts and rms_after.

    The defaults are conventional values (3 sigma, 60 degrees, 30 iterations), not tuned on a capture.  Known limits: a local
    method, which needs a start within the basin of the answer (init, the CLI's --scan_transform); no global, pose-free
    registration; no landmarks; rigid or similarity only, nothing non-rigid.

    ValueError: a bad argument, fewer than 6 kept pairs at any evaluation, a singular system."""
    check_options(metric, max_iter, max_dist, gate_sigma, normal_cos, tol, stride)
    dev = _lib.hip_device(device, _WHAT, ValueError)
    mv = mesh_vertices.detach().cpu().numpy() if isinstance(mesh_vertices, torch.Tensor) else np.asarray(mesh_vertices)
    if mv.ndim != 2 or mv.shape[1] != 3 or mv.shape[0] < 1 or mv.dtype != np.float64:
        raise ValueError(f"mesh_vertices must be a float64 [V,3] array, got {mv.dtype} {mv.shape}")
    mv = np.ascontiguousarray(mv)
    sv = scan.vertices if isinstance(scan, Scan) else scan
    sv = sv.detach().cpu().numpy() if isinstance(sv, torch.Tensor) else np.asarray(sv)
    if sv.ndim != 2 or sv.shape[1] != 3 or sv.shape[0] < 1 or sv.dtype != np.float64 or not np.isfinite(sv).all():
        raise ValueError(f"the scan must hold finite float64 [N,3] points, got {sv.dtype} {sv.shape}")
    pose = np.eye(4) if init is None else np.array(init, np.float64)
    if pose.shape != (4, 4) or not np.isfinite(pose).all() or not np.array_equal(pose[3], [0.0, 0.0, 0.0, 1.0]) or \
            np.linalg.det(pose[:3, :3]) == 0.0:
        raise ValueError("init must be a finite invertible 4x4 matrix that ends in the row 0 0 0 1")
    index = ClosestPointIndex(torch.from_numpy(mv), mesh_faces, device=dev)
    if not index.is_tri:
        raise ValueError("mesh_faces: the mesh needs at least one triangle")
    corners = box_corners(mv)
    diag = float(np.linalg.norm(corners[7] - corners[0]))
    origin = mv.mean(0)
    cos2 = float(normal_cos) * float(normal_cos)
    p0 = _points(torch.from_numpy(np.ascontiguousarray(sv[::stride])), "scan points", dev)
    moved = torch.empty_like(p0)
    scratch = _lib.scratch("t4d_align_scratch_bytes", dev, int(p0.shape[0]))[0]

    def evaluate(gate):
        transform_points(p0, pose[:3], out=moved)
        d2, idx, cl = index.query(moved, max_dist)
        rec = accumulate(index, moved, d2, idx, cl, origin, -1.0 if gate is None else gate * gate, cos2, scratch=scratch).cpu().numpy()
        n = kept_pairs(rec)
        return rec, math.sqrt(rec[SUM_D2] / n)

    gate = None if max_dist is None else float(max_dist)
    iterations, converged, rms_before = 0, True, None
    with torch.cuda.device(dev):
        for phase_metric, with_scale in ([("point", True)] if scale else []) + [(metric, False)]:
            phase_converged = False
            for _ in range(int(max_iter)):
                rec, rms = evaluate(gate)
                if rms_before is None:
                    rms_before = rms
                A, b = step_of(rec, phase_metric, with_scale, origin)
                pose[:3, :3], pose[:3, 3] = A @ pose[:3, :3], A @ pose[:3, 3] + b
                iterations += 1
                gate = float(gate_sigma) * rms if max_dist is None else min(float(max_dist), float(gate_sigma) * rms)
                motion = float(np.sqrt((((corners @ A.T + b) - corners) ** 2).sum(1)).max())
                if motion <= float(tol) * diag:
                    phase_converged = True
                    break
            converged = converged and phase_converged
        rec, rms_after = evaluate(gate)
    s, angle, translation = describe(pose)
    counts = {name: int(rec[COUNT + k]) for k, name in enumerate(CLASSES)}
    return Alignment(pose, s, iterations, converged, counts, float(rms_before), float(rms_after), angle, translation)
