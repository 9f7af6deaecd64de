"""
The startup model fitted to a frame's scan: non-rigid ICP on the GPU (Amberg, Romdhani, Vetter, "Optimal Step Nonrigid ICP",
CVPR 2007), so that `<input_dir>/<seq>/face_v5.obj` no longer has to come from a manual alignment in another tool.

    fit_template(mesh, scan, ...) -> Fit             the template (coarse.read_obj) moved onto the scan (scanscore.read_scan)
    write_startup_obj(template_path, vertices, out)  the template's file with new 'v' lines, every other line byte-identical
    python -m topo4d_amd.startup --template OBJ --scan FILE --out DIR   writes DIR/face_v5.obj and DIR/startup_fit.json

    classify / assemble / precondition / apply_operator / cg_start / cg_run / positions    one thin wrapper per export

over `t4d_closest_query` (scanscore.ClosestPointIndex), scanalign.align_scan, objexport's vertex normals and the t4d_nricp_*
entry points (include/topo4d_raster.h states the rule in full, csrc/t4d_nricp.hip runs it, tests/startup_ref.py restates it in
numpy bit for bit).  There is no CPU path.

The fit.  Pre-alignment: without `init`, scanalign.align_scan takes the scan onto the template and its matrix is inverted on the
host, so that the template moves into the scan's frame (the calibrated frame face_v5.obj must be in; `scale` adds one scale); with
`init` that matrix is the pre-alignment as it is, so that a fit's own `prealign` reproduces the fit.  The solve then runs in a
normalised frame, origin at the pre-aligned template's box centre and the box diagonal as unit, which template vertices, scan
points and landmarks enter by one float64 rule (x - centre) / diagonal.  Per stiffness value up to `inner` outer steps: query the
moved vertices against the scan index (built once), classify them, solve the normal equations for the three coordinate columns by
block-Jacobi conjugate gradients on the device (warm-started; the host reads one 40-double record every `check_every` iterations
and stops a column at ||r||^2 <= tol^2 ||b||^2 or at max_cg), move the vertices.  A stiffness value ends early once no vertex moved
by more than move_tol x the diagonal.

The defaults (stiffness 50 .. 0.2, 3 steps each, gamma 1, 60 degrees, 3 sigma) are conventional values, not tuned on a capture.

Known limits.
  - The subject's own texture is not re-projected onto the fitted mesh; `projtex` can do that afterwards.
  - No global registration: the fit is local and needs `init` or a template near the scan.
  - Parts the scan never shows (the mouth bag, the back of the eyeballs) follow the stiffness or stay at the pre-aligned pose.
  - The data term is point-to-point; there is no point-to-plane term.
  - `facial_regions.pkl` is not transferred to another topology.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import shutil
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib, scanalign
from ._lib import ptr
from .scanscore import ClosestPointIndex, Scan

RECORD, SUM_D2 = 8, 7                                           # T4D_NRICP_RECORD_DOUBLES and the offsets of the header
STATE, STATE_REC, RZ, RR, PQ, ALPHA, BETA, ITER, STATE_BB, MAX_RUN = 40, 16, 0, 3, 6, 9, 12, 15, 32, 4096
CLASSES = ("unmatched", "gated", "degenerate", "off_normal", "flipped", "weightless", "kept")
KEPT = 6
MIN_PAIRS = 6
DEFAULT_STIFFNESS = (50.0, 20.0, 5.0, 2.0, 0.8, 0.5, 0.35, 0.2)
_WHAT = "the startup fit"
_F64 = torch.float64


class Fit(NamedTuple):
    vertices: np.ndarray                # float64 [N,3], file coordinates of the scan's frame
    prealign: np.ndarray                # float64 [4,4]: template file coordinates -> the scan's frame
    centre: np.ndarray                  # the normalised frame: x -> (x - centre) / diagonal
    diagonal: float
    steps: list                         # one dict per outer step
    components_without_data: list       # {"size", "first_vertex"} of the components that kept no data in the last step
    flipped_triangles: list             # the triangles whose normal turned against the pre-aligned template's
    score_before: Optional[dict]        # scanscore.score_scan of the pre-aligned template and of the fit
    score_after: Optional[dict]

    def as_dict(self) -> dict:
        return {"prealign": self.prealign.tolist(), "centre": self.centre.tolist(), "diagonal": self.diagonal, "steps": self.steps,
                "components_without_data": self.components_without_data, "flipped_triangles": self.flipped_triangles,
                "score_before": self.score_before, "score_after": self.score_after}


# ---- the host's share: plain numpy float64, restated in tests/startup_ref.py -------------------------------------------------
def neighbour_csr(faces, n: int):
    """(nbr_off int32 [n + 1], nbr int32): every vertex's neighbours over the unique undirected edges of the triangles, ascending."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    both = np.unique(np.concatenate([e, e[:, ::-1]]), axis=0) if len(e) else np.zeros((0, 2), np.int64)
    off = np.concatenate([[0], np.cumsum(np.bincount(both[:, 0], minlength=n))]).astype(np.int32)
    return off, np.ascontiguousarray(both[:, 1], np.int32)


def transform(points, matrix) -> np.ndarray:
    p, m = np.asarray(points, np.float64), np.asarray(matrix, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[k, 0] * x + m[k, 1] * y) + m[k, 2] * z) + m[k, 3] for k in range(3)], 1)


def frame_of(vertices):
    """(centre, diagonal) of the normalised frame: the box centre (lo + hi) / 2 and the box diagonal."""
    lo, hi = vertices.min(0), vertices.max(0)
    d = hi - lo
    return (lo + hi) * 0.5, math.sqrt(float((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))


def components(nbr_off, nbr) -> np.ndarray:
    """int64 [n]: per vertex the lowest vertex index of its connected component."""
    n = len(nbr_off) - 1
    label = np.arange(n, dtype=np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(nbr_off))
    while True:
        new = label.copy()
        np.minimum.at(new, src, label[nbr])
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def components_without(label, s) -> list:
    total = np.bincount(label, weights=(np.asarray(s) > 0).astype(np.float64), minlength=len(label))
    size = np.bincount(label, minlength=len(label))
    return [{"size": int(size[k]), "first_vertex": int(k)} for k in np.nonzero((size > 0) & (total == 0))[0]]


def turned_triangles(before, after, faces) -> list:
    def normal(v):
        a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
        return np.cross(b - a, c - a)
    return [int(k) for k in np.nonzero((normal(before) * normal(after)).sum(1) < 0.0)[0]]


def landmark_arrays(landmarks, n: int):
    """(lw float64 [n], lt float64 [n,3]) of landmark rows (vertex index, x, y, z); (None, None) without landmarks."""
    if landmarks is None:
        return None, None
    rows = np.asarray(landmarks, np.float64)
    if rows.ndim != 2 or rows.shape[1] != 4 or rows.shape[0] < 1 or not np.isfinite(rows).all():
        raise ValueError(f"landmarks must be finite rows of vertex index, x, y, z, got shape {rows.shape}")
    idx = rows[:, 0].astype(np.int64)
    if (idx != rows[:, 0]).any() or idx.min() < 0 or idx.max() >= n or len(np.unique(idx)) != len(idx):
        raise ValueError(f"landmarks: the vertex indices must be distinct integers in [0, {n})")
    lw, lt = np.zeros(n), np.zeros((n, 3))
    lw[idx], lt[idx] = 1.0, rows[:, 1:]
    return lw, lt


def check_options(stiffness, inner, gamma, landmark_weight, normal_cos, max_dist, gate_sigma, tol, max_cg, check_every, move_tol):
    """(stiffness list, landmark weight list): ValueError for an option out of range."""
    st = [float(a) for a in (stiffness if isinstance(stiffness, (list, tuple, np.ndarray)) else [stiffness])]
    if not st or not all(math.isfinite(a) and a > 0.0 for a in st) or any(b >= a for a, b in zip(st, st[1:])):
        raise ValueError(f"stiffness must be a decreasing list of finite values > 0, got {stiffness!r}")
    lw = [float(b) for b in landmark_weight] if isinstance(landmark_weight, (list, tuple, np.ndarray)) else [float(landmark_weight)] * len(st)
    if len(lw) != len(st) or not all(math.isfinite(b) and b >= 0.0 for b in lw):
        raise ValueError(f"landmark_weight must be one finite value >= 0 or one per stiffness value, got {landmark_weight!r}")
    for name, value, lo in (("inner", inner, 1), ("max_cg", max_cg, 1), ("check_every", check_every, 1)):
        if not (isinstance(value, (int, np.integer)) and value >= lo):
            raise ValueError(f"{name} must be an integer >= {lo}, got {value!r}")
    if check_every > MAX_RUN:
        raise ValueError(f"check_every must be at most {MAX_RUN}, got {check_every}")
    if not (math.isfinite(float(gamma)) and float(gamma) > 0.0):
        raise ValueError(f"gamma must be finite and > 0, got {gamma}")
    if not (math.isfinite(float(tol)) and float(tol) >= 0.0 and math.isfinite(float(move_tol)) and float(move_tol) >= 0.0):
        raise ValueError(f"tol and move_tol must be finite and >= 0, got {tol} and {move_tol}")
    scanalign.check_options(max_dist=max_dist, gate_sigma=gate_sigma, normal_cos=normal_cos)
    return st, lw


# ---- the device half: one wrapper per export ------------------------------------------------------------------------------------
def _rows(t, n: int, cols: int, what: str, dtype=_F64, optional: bool = False):
    if t is None and optional:
        return None
    shape = (n,) if cols == 0 else (n, cols)
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtype:
        raise ValueError(f"{what} must be a {str(dtype).replace('torch.', '')} tensor of shape {list(shape)}")
    return t


def _field(t, n: int, what: str):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (3, 4, n) or t.dtype != _F64:
        raise ValueError(f"{what} must be a float64 field [3,4,{n}]")
    return t


def _count(v, what: str = "v") -> int:
    if not isinstance(v, torch.Tensor) or v.dim() != 2 or v.shape[1] != 3 or v.shape[0] < 1 or v.dtype != _F64:
        raise ValueError(f"{what} must be a float64 [N,3] tensor with N >= 1")
    return int(v.shape[0])


def _stiffness(a2, a2g):
    a2, a2g = float(a2), float(a2g)
    if not (math.isfinite(a2) and math.isfinite(a2g) and a2 > 0.0 and a2g > 0.0):
        raise ValueError(f"need finite a2 > 0 and a2g > 0, got {a2} and {a2g}")
    return a2, a2g


def _csr(nbr_off, nbr, n: int):
    if not isinstance(nbr_off, torch.Tensor) or tuple(nbr_off.shape) != (n + 1,) or nbr_off.dtype != torch.int32:
        raise ValueError(f"nbr_off must be an int32 tensor of shape [{n + 1}]")
    if nbr is not None and (not isinstance(nbr, torch.Tensor) or nbr.dim() != 1 or nbr.dtype != torch.int32):
        raise ValueError("nbr must be a one-dimensional int32 tensor")


def _placed(dev, *pairs):
    """the tensors as the library takes them; an empty one (the neighbours of a mesh without an edge) as one unused word, since
    the library reads a NULL pointer as a missing buffer"""
    out = [None if t is None else _lib.on_device(t, name, dev) for t, name in pairs]
    return [t if t is None or t.numel() > 0 else torch.zeros(1, dtype=t.dtype, device=dev) for t in out]


def _scratch(dev, n: int, reuse=None):
    return _lib.scratch("t4d_nricp_scratch_bytes", dev, n, reuse=reuse)[0]


def classify(index: ClosestPointIndex, points, d2, prim, closest, normals=None, weights=None, gate2: float = -1.0, cos2: float = 0.25,
             normal_cos: float = 0.5, scratch=None):
    """(cls int32 [N], w float64 [N], target float64 [N,3], record float64 [8]) on the device: t4d_nricp_classify over what
    index.query(points) gave.  normals None: no `flipped` test (a cloud has no normals to compare with); weights None: all 1."""
    n = _count(points, "points")
    _rows(d2, n, 0, "d2"), _rows(prim, n, 0, "prim", torch.int32), _rows(closest, n, 3, "closest")
    _rows(normals, n, 3, "normals", optional=True), _rows(weights, n, 0, "weights", optional=True)
    gate2, cos2, normal_cos = float(gate2), float(cos2), float(normal_cos)
    if not math.isfinite(gate2) or not (0.0 <= cos2 <= 1.0) or not (-1.0 <= normal_cos <= 1.0):
        raise ValueError(f"need a finite gate2, 0 <= cos2 <= 1 and -1 <= normal_cos <= 1, got {gate2}, {cos2}, {normal_cos}")
    dev = index.dev
    p, d2, prim, closest, normals, weights = _placed(dev, (points, "points"), (d2, "d2"), (prim, "prim"), (closest, "closest"),
                                                     (normals, "normals"), (weights, "weights"))
    cls = torch.empty(n, dtype=torch.int32, device=dev)
    w = torch.empty(n, dtype=_F64, device=dev)
    target = torch.empty((n, 3), dtype=_F64, device=dev)
    record = torch.empty(RECORD, dtype=_F64, device=dev)
    with torch.cuda.device(dev):
        s = _scratch(dev, n, scratch)
        _lib.call("t4d_nricp_classify", ptr(index._index), index._index.numel(), ptr(p), n, ptr(d2), ptr(prim), ptr(closest), ptr(normals),
                  ptr(weights), gate2, cos2, normal_cos, ptr(cls), ptr(w), ptr(target), ptr(record), ptr(s), s.numel(), _lib.stream(dev))
    return cls, w, target, record


def assemble(v, nbr_off, w, c, lw=None, lt=None, a2: float = 1.0, a2g: float = 1.0, beta2: float = 0.0):
    """(s float64 [N], B field, chol float64 [10,N]) on the device: t4d_nricp_assemble."""
    n = _count(v)
    _csr(nbr_off, None, n)
    _rows(w, n, 0, "w"), _rows(c, n, 3, "c"), _rows(lw, n, 0, "lw", optional=True), _rows(lt, n, 3, "lt", optional=True)
    if (lw is None) != (lt is None):
        raise ValueError("lw and lt come together")
    a2, a2g = _stiffness(a2, a2g)
    beta2 = float(beta2)
    if not (math.isfinite(beta2) and beta2 >= 0.0):
        raise ValueError(f"beta2 must be finite and >= 0, got {beta2}")
    v = _lib.on_device(v, "v")
    dev = v.device
    nbr_off, w, c, lw, lt = _placed(dev, (nbr_off, "nbr_off"), (w, "w"), (c, "c"), (lw, "lw"), (lt, "lt"))
    s = torch.empty(n, dtype=_F64, device=dev)
    b = torch.empty((3, 4, n), dtype=_F64, device=dev)
    chol = torch.empty((10, n), dtype=_F64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("t4d_nricp_assemble", ptr(v), n, ptr(nbr_off), ptr(w), ptr(c), ptr(lw), ptr(lt), a2, a2g, beta2, ptr(s), ptr(b), ptr(chol),
                  _lib.stream(dev))
    return s, b, chol


def _chol(chol) -> int:
    if not isinstance(chol, torch.Tensor) or chol.dim() != 2 or chol.shape[0] != 10 or chol.shape[1] < 1 or chol.dtype != _F64:
        raise ValueError("chol must be a float64 [10,N] tensor with N >= 1")
    return int(chol.shape[1])


def precondition(chol, r):
    """Z = M^-1 R (a field) from the factors of assemble: t4d_nricp_precond."""
    n = _chol(chol)
    _field(r, n, "r")
    chol = _lib.on_device(chol, "chol")
    r, = _placed(chol.device, (r, "r"))
    z = torch.empty_like(r)
    with torch.cuda.device(chol.device):
        _lib.call("t4d_nricp_precond", ptr(chol), n, ptr(r), ptr(z), _lib.stream(chol.device))
    return z


def apply_operator(v, nbr_off, nbr, s, a2, a2g, p, scratch=None):
    """(Q = K P, float64 [3] of P[c] . Q[c]) on the device: t4d_nricp_apply."""
    n = _count(v)
    _csr(nbr_off, nbr, n)
    _rows(s, n, 0, "s"), _field(p, n, "p")
    a2, a2g = _stiffness(a2, a2g)
    v = _lib.on_device(v, "v")
    dev = v.device
    nbr_off, nbr, s, p = _placed(dev, (nbr_off, "nbr_off"), (nbr, "nbr"), (s, "s"), (p, "p"))
    q = torch.empty_like(p)
    dots = torch.empty(3, dtype=_F64, device=dev)
    with torch.cuda.device(dev):
        sc = _scratch(dev, n, scratch)
        _lib.call("t4d_nricp_apply", ptr(v), n, ptr(nbr_off), ptr(nbr), ptr(s), a2, a2g, ptr(p), ptr(q), ptr(dots), ptr(sc), sc.numel(),
                  _lib.stream(dev))
    return q, dots


class CG(NamedTuple):
    """The vectors of one conjugate-gradient run on the device: x is updated in place; state is the 40-double record."""
    x: torch.Tensor
    r: torch.Tensor
    z: torch.Tensor
    p: torch.Tensor
    q: torch.Tensor
    state: torch.Tensor
    scratch: torch.Tensor


def _system(v, nbr_off, nbr, s, a2, a2g, chol):
    n = _count(v)
    _csr(nbr_off, nbr, n)
    _rows(s, n, 0, "s")
    if _chol(chol) != n:
        raise ValueError(f"chol must be a float64 [10,{n}] tensor")
    a2, a2g = _stiffness(a2, a2g)
    v = _lib.on_device(v, "v")
    return (n, v.device, a2, a2g) + tuple(_placed(v.device, (v, "v"), (nbr_off, "nbr_off"), (nbr, "nbr"), (s, "s"), (chol, "chol")))


def cg_start(v, nbr_off, nbr, s, a2, a2g, chol, b, x, scratch=None) -> CG:
    """R = B - K X, Z = M^-1 R, P = Z and record 0 of the state: t4d_nricp_cg_start.  x (a field) is the warm start, kept as it is."""
    n = _count(v)
    _field(b, n, "b"), _field(x, n, "x")
    n, dev, a2, a2g, v, nbr_off, nbr, s, chol = _system(v, nbr_off, nbr, s, a2, a2g, chol)
    b, x = _placed(dev, (b, "b"), (x, "x"))
    r, z, p, q = (torch.empty_like(x) for _ in range(4))
    state = torch.empty(STATE, dtype=_F64, device=dev)
    with torch.cuda.device(dev):
        sc = _scratch(dev, n, scratch)
        _lib.call("t4d_nricp_cg_start", ptr(v), n, ptr(nbr_off), ptr(nbr), ptr(s), a2, a2g, ptr(chol), ptr(b), ptr(x), ptr(r), ptr(z), ptr(p),
                  ptr(q), ptr(state), ptr(sc), sc.numel(), _lib.stream(dev))
    return CG(x, r, z, p, q, state, sc)


def cg_run(v, nbr_off, nbr, s, a2, a2g, chol, cg: CG, done: int, iters: int, stop_mask: int = 0) -> None:
    """`iters` more iterations after `done`, three launches each; bit c of stop_mask freezes column c: t4d_nricp_cg_run."""
    if not (isinstance(done, (int, np.integer)) and done >= 0 and isinstance(iters, (int, np.integer)) and 0 <= iters <= MAX_RUN and
            isinstance(stop_mask, (int, np.integer)) and 0 <= stop_mask <= 7):
        raise ValueError(f"need done >= 0, 0 <= iters <= {MAX_RUN} and a stop_mask in 0..7, got {done!r}, {iters!r}, {stop_mask!r}")
    n, dev, a2, a2g, v, nbr_off, nbr, s, chol = _system(v, nbr_off, nbr, s, a2, a2g, chol)
    for t, name in zip(cg[:5], "xrzpq"):
        _field(t, n, name)
        if not t.is_cuda or t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"topo4d_amd has no CPU path: {name} must be contiguous on the system's HIP device")
    with torch.cuda.device(dev):
        _lib.call("t4d_nricp_cg_run", ptr(v), n, ptr(nbr_off), ptr(nbr), ptr(s), a2, a2g, ptr(chol), ptr(cg.x), ptr(cg.r), ptr(cg.z), ptr(cg.p),
                  ptr(cg.q), ptr(cg.state), int(done), int(iters), int(stop_mask), ptr(cg.scratch), cg.scratch.numel(), _lib.stream(dev))


def positions(v, x, prev=None, out=None, scratch=None):
    """(pos float64 [N,3] = X^T (v, 1), float64 [1]: the largest squared move against prev (0 without)): t4d_nricp_positions."""
    n = _count(v)
    _field(x, n, "x"), _rows(prev, n, 3, "prev", optional=True), _rows(out, n, 3, "out", optional=True)
    v = _lib.on_device(v, "v")
    dev = v.device
    x, prev = _placed(dev, (x, "x"), (prev, "prev"))
    if out is not None and (not out.is_cuda or out.device != dev or not out.is_contiguous()):
        raise RuntimeError("topo4d_amd has no CPU path: out must be contiguous on the vertices' HIP device")
    pos = torch.empty((n, 3), dtype=_F64, device=dev) if out is None else out
    move2 = torch.empty(1, dtype=_F64, device=dev)
    with torch.cuda.device(dev):
        sc = _scratch(dev, n, scratch)
        _lib.call("t4d_nricp_positions", ptr(v), n, ptr(x), ptr(prev), ptr(pos), ptr(move2), ptr(sc), sc.numel(), _lib.stream(dev))
    return pos, move2


def identity_field(n: int, device) -> torch.Tensor:
    """X = [I; 0] for every vertex."""
    x = torch.zeros((3, 4, n), dtype=_F64, device=device)
    for c in range(3):
        x[c, c] = 1.0
    return x


def solve(v, nbr_off, nbr, s, a2, a2g, chol, b, x, tol: float, max_cg: int, check_every: int = 32, scratch=None):
    """Conjugate gradients on x (in place) until every column has ||r||^2 <= tol^2 ||b||^2 or max_cg iterations are made; the
    host looks every check_every iterations.  Returns (iterations per column, relative residuals per column)."""
    cg = cg_start(v, nbr_off, nbr, s, a2, a2g, chol, b, x, scratch=scratch)
    done, mask, stopped_at = 0, 0, [None] * 3
    tol2 = float(tol) * float(tol)
    while True:
        st = cg.state.cpu().numpy()
        rec, bb = st[STATE_REC * (done & 1):STATE_REC * (done & 1) + STATE_REC], st[STATE_BB:STATE_BB + 3]
        if not np.isfinite(st).all():
            raise ValueError("the startup fit's system is not positive definite in float64 (a non-finite residual)")
        for c in range(3):
            if stopped_at[c] is None and (rec[RR + c] <= tol2 * bb[c] or done >= max_cg):
                stopped_at[c], mask = done, mask | (1 << c)
        if mask == 7:
            break
        step = min(int(check_every), int(max_cg) - done)
        cg_run(v, nbr_off, nbr, s, a2, a2g, chol, cg, done, step, mask)
        done += step
    rel = [math.sqrt(rec[RR + c] / bb[c]) if bb[c] > 0.0 else 0.0 for c in range(3)]
    return stopped_at, rel


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
def fit_template(mesh, scan: Scan, *, init=None, scale: bool = False, weights=None, landmarks=None,
                 stiffness: Sequence[float] = DEFAULT_STIFFNESS, inner: int = 3, gamma: float = 1.0, landmark_weight=1.0,
                 normal_cos: float = 0.5, max_dist: Optional[float] = None, gate_sigma: float = 3.0, tol: float = 1e-8, max_cg: int = 2000,
                 check_every: int = 32, move_tol: float = 1e-5, score: bool = True, device=None) -> Fit:
    """The template `mesh` (coarse.ObjMesh: vertices float64 [N,3], faces [F,3]) fitted to `scan` (scanscore.Scan, with or
    without faces), as the module's text describes.

    init: 4x4 taking template coordinates into the scan's frame, used as the pre-alignment as it is (None: scanalign.align_scan,
    with `scale` adding one scale, and max_dist, gate_sigma, normal_cos as here).  weights: float64 [N] >= 0, 0 = no data term.
    landmarks: rows of vertex index and target x y z in the scan's frame, weighted by landmark_weight^2 (one value, or one per
    stiffness value).  max_dist is in file units; the first step gates at max_dist alone and every later one at min(max_dist,
    gate_sigma x the rms distance of the pairs the first step kept).  The sigma gate is set once: scanalign renews it every
    iteration, where a rigid residual has a floor, but a non-rigid fit takes the kept pairs' rms towards zero, the gate follows it,
    and the vertices that are still on their way are locked out one after the other (on the tests' prototype scene 112 of 441
    by the last step).  A component of the mesh that keeps no data keeps its pose and is listed in the result.

    ValueError: a bad argument, fewer than 6 kept vertices at the first step (before anything is written), a template with a
    vertex in no face."""
    st, lws = check_options(stiffness, inner, gamma, landmark_weight, normal_cos, max_dist, gate_sigma, tol, max_cg, check_every, move_tol)
    dev = _lib.hip_device(device, _WHAT, ValueError)
    tv = np.asarray(mesh.vertices)
    faces = np.asarray(mesh.faces)
    if tv.ndim != 2 or tv.shape[1] != 3 or tv.shape[0] < 1 or tv.dtype != np.float64 or not np.isfinite(tv).all():
        raise ValueError(f"the template must hold finite float64 [N,3] vertices, got {tv.dtype} {tv.shape}")
    n = int(tv.shape[0])
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.min() < 0 or faces.max() >= n:
        raise ValueError(f"the template's faces must be [F,3] indices in [0, {n})")
    wts = None
    if weights is not None:
        wts = np.asarray(weights)
        if wts.shape != (n,) or wts.dtype != np.float64 or not np.isfinite(wts).all() or wts.min() < 0.0:
            raise ValueError(f"weights must be finite float64 [{n}] values >= 0")
    lw_np, lt_np = landmark_arrays(landmarks, n)
    sv = np.asarray(scan.vertices, np.float64)
    if init is None:
        align = scanalign.align_scan(tv, faces, scan, scale=scale, max_dist=max_dist, gate_sigma=gate_sigma, normal_cos=normal_cos, device=dev)
        pre = np.linalg.inv(align.matrix)
    else:
        pre = np.array(init, np.float64)
        if pre.shape != (4, 4) or not np.isfinite(pre).all() or not np.array_equal(pre[3], [0.0, 0.0, 0.0, 1.0]) or np.linalg.det(pre[:3, :3]) == 0.0:
            raise ValueError("init must be a finite invertible 4x4 matrix that ends in the row 0 0 0 1")
    placed = transform(tv, pre)
    centre, diag = frame_of(placed)
    if not diag > 0.0:
        raise ValueError("the template's bounding box is a point")
    unit = lambda x: (x - centre) / diag
    off_np, nbr_np = neighbour_csr(faces, n)
    label = components(off_np, nbr_np)
    gate = None if max_dist is None else float(max_dist) / diag
    limit = gate
    cos2 = float(normal_cos) * float(normal_cos)
    is_tri = scan.faces is not None and len(scan.faces) > 0
    from . import objexport
    with torch.cuda.device(dev):
        on = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        v, off, nbr, wt, lw = on(unit(placed)), on(off_np), on(nbr_np), on(wts), on(lw_np)
        lt = None if lt_np is None else on(unit(lt_np))
        index = ClosestPointIndex(on(unit(sv)), scan.faces if is_tri else None, device=dev)
        corners = objexport._VertexFaces(on(faces.astype(np.int32)), n) if is_tri else None
        scratch = _scratch(dev, n)
        x = identity_field(n, dev)
        pos, _ = positions(v, x, scratch=scratch)
        steps, s = [], None
        for alpha, beta in zip(st, lws):
            a2 = alpha * alpha
            a2g = a2 * (float(gamma) * float(gamma))
            for it in range(int(inner)):
                d2, prim, closest = index.query(pos, limit)
                normals = corners.normals(pos) if corners is not None else None
                cls, w, target, record = classify(index, pos, d2, prim, closest, normals, wt, -1.0 if gate is None else gate * gate, cos2,
                                                  float(normal_cos), scratch=scratch)
                rec = record.cpu().numpy()
                kept = int(rec[KEPT])
                counts = {name: int(rec[k]) for k, name in enumerate(CLASSES)}
                if not steps and kept < MIN_PAIRS:
                    raise ValueError(f"only {kept} vertices keep a data term at the first step ({counts}): a fit needs at least {MIN_PAIRS}")
                rms = math.sqrt(rec[SUM_D2] / kept) if kept else 0.0
                if not steps:                                       # the sigma gate is set once, from the first step's kept pairs
                    gate = float(gate_sigma) * rms if limit is None else min(limit, float(gate_sigma) * rms)
                s, b, chol = assemble(v, off, w, target, lw, lt, a2, a2g, beta * beta)
                iters, rel = solve(v, off, nbr, s, a2, a2g, chol, b, x, tol, max_cg, check_every, scratch=scratch)
                pos, move2 = positions(v, x, prev=pos, out=pos, scratch=scratch)
                move = math.sqrt(float(move2.item()))
                steps.append({"stiffness": alpha, "landmark_weight": beta, "step": it, "counts": counts, "rms": rms * diag, "cg_iterations": iters,
                              "residuals": rel, "move": move * diag})
                if move <= float(move_tol):
                    break
        fitted = pos.cpu().numpy() * diag + centre
        without = components_without(label, s.cpu().numpy())
    turned = turned_triangles(placed, fitted, faces)
    before = after = None
    if score:
        from .scanscore import score_scan
        strip = lambda d: {k: d[k] for k in ("scan_to_mesh", "mesh_to_scan")}
        before = strip(score_scan(placed, faces, scan, max_dist=max_dist, device=dev))
        after = strip(score_scan(fitted, faces, scan, max_dist=max_dist, device=dev))
    return Fit(fitted, pre, centre, diag, steps, without, turned, before, after)


# ---- files and the command line -----------------------------------------------------------------------------------------------
def write_startup_obj(template_path, vertices, out_path) -> None:
    """The template's OBJ with its 'v' lines replaced, in order, by 'v x y z' in Python's repr of the float64 coordinates (which
    parse back to the same bits); every other line, and every line ending, is kept byte for byte."""
    v = np.asarray(vertices)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype != np.float64 or not np.isfinite(v).all():
        raise ValueError(f"vertices must be finite float64 [N,3], got {v.dtype} {v.shape}")
    with open(template_path, "rb") as f:
        lines = f.readlines()
    out, k = [], 0
    for line in lines:
        parts = line.split()
        if parts and parts[0] == b"v":
            if k >= len(v):
                raise ValueError(f"{template_path}: more 'v' lines than the {len(v)} vertices given")
            body = line.rstrip(b"\r\n")
            out.append(("v " + " ".join(repr(float(c)) for c in v[k])).encode() + line[len(body):])
            k += 1
        else:
            out.append(line)
    if k != len(v):
        raise ValueError(f"{template_path}: {k} 'v' lines for {len(v)} vertices")
    with open(out_path, "wb") as f:
        f.writelines(out)


def copy_material(template_path, out_dir) -> list:
    """Copy the template's MTL (its 'mtllib' line) and the texture its map_Kd names beside the written OBJ; the names copied."""
    src_dir, copied = os.path.dirname(os.path.abspath(template_path)), []
    with open(template_path, "r") as f:
        names = [line.strip()[len("mtllib"):].strip() for line in f if line.split()[:1] == ["mtllib"]]
    for name in names:
        mtl = os.path.join(src_dir, name)
        if not os.path.isfile(mtl):
            raise ValueError(f"{template_path}: the material file {name} is not beside it")
        os.makedirs(os.path.dirname(os.path.join(out_dir, name)) or out_dir, exist_ok=True)
        shutil.copyfile(mtl, os.path.join(out_dir, name))
        copied.append(name)
        with open(mtl, "r") as f:
            maps = [line.strip()[len("map_Kd"):].strip() for line in f if line.split()[:1] == ["map_Kd"]]
        for tex in maps:
            src = os.path.join(os.path.dirname(mtl), tex)
            if not os.path.isfile(src):
                raise ValueError(f"{mtl}: the texture {tex} is not beside it")
            dst = os.path.join(os.path.dirname(os.path.join(out_dir, name)), tex)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            shutil.copyfile(src, dst)
            copied.append(tex)
    return copied


def _floats(text: str) -> list:
    return [float(t) for t in text.replace(",", " ").split()]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m topo4d_amd.startup", description="Fit the startup mesh to a frame's scan (non-rigid ICP).")
    ap.add_argument("--template", required=True, help="OBJ in the tracked topology")
    ap.add_argument("--scan", required=True, help="the frame's scan, PLY or OBJ, mesh or cloud")
    ap.add_argument("--out", required=True, help="directory for face_v5.obj and startup_fit.json")
    ap.add_argument("--init", help="text file of a 4x4 matrix, template -> scan: the pre-alignment as it is")
    ap.add_argument("--scale", action="store_true", help="let the rigid pre-alignment find one scale")
    ap.add_argument("--weights", help=".npy of float64 [N] data weights")
    ap.add_argument("--landmarks", help="text file, one row per landmark: vertex index, x, y, z")
    ap.add_argument("--stiffness", type=_floats, default=list(DEFAULT_STIFFNESS))
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--landmark_weight", type=_floats, default=[1.0])
    ap.add_argument("--normal_cos", type=float, default=0.5)
    gate = ap.add_mutually_exclusive_group()
    gate.add_argument("--max_dist", type=float, default=None)
    gate.add_argument("--gate_sigma", type=float, default=3.0)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max_cg", type=int, default=2000)
    ap.add_argument("--copy_material", action="store_true")
    args = ap.parse_args(argv)
    from .coarse import read_obj
    from .scanscore import read_scan
    mesh, scan = read_obj(args.template), read_scan(args.scan)
    lw = args.landmark_weight[0] if len(args.landmark_weight) == 1 else args.landmark_weight
    fit = fit_template(mesh, scan, init=None if args.init is None else np.loadtxt(args.init).reshape(4, 4), scale=args.scale,
                       weights=None if args.weights is None else np.load(args.weights),
                       landmarks=None if args.landmarks is None else np.loadtxt(args.landmarks, ndmin=2), stiffness=args.stiffness,
                       inner=args.inner, gamma=args.gamma, landmark_weight=lw, normal_cos=args.normal_cos, max_dist=args.max_dist,
                       gate_sigma=args.gate_sigma, tol=args.tol, max_cg=args.max_cg)
    os.makedirs(args.out, exist_ok=True)
    write_startup_obj(args.template, fit.vertices, os.path.join(args.out, "face_v5.obj"))
    if args.copy_material:
        copy_material(args.template, args.out)
    with open(os.path.join(args.out, "startup_fit.json"), "w") as f:
        json.dump(fit.as_dict(), f, indent=1)
    last = fit.steps[-1]
    print(f"startup: {len(fit.steps)} steps, rms over kept {fit.steps[0]['rms']:.6g} -> {last['rms']:.6g}, {len(fit.flipped_triangles)} "
          f"triangles turned, {len(fit.components_without_data)} components without data")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
