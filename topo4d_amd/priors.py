"""
The topology priors of Topo4D's geometry loop - the regularisers of get_loss (train.py:328-368) - as one fused HIP evaluation
(t4d_priors_eval: two launches, forward and backward, no host synchronisation, bit-identical from run to run):

    later frames   rigid, rot, iso (train.py:330-346); flat, flat_lip_bottom (FlattenLoss); flat_eye, flat_face_bottom,
                   flat_lip_socket (FlattenLoss_v2); flat_lid_top, flat_lid_bottom, flat_lip, flat_mouth (SoftFlattenLoss
                   against the cos_init cached on frame 0)
    frame 0        scale, scale_max (train.py:359-363) and the four soft terms without cos_init, whose cos becomes cos_init
                   (train.py:364-368)

    priors = TopologyPriors.from_topo4d(variables, losses_list, losses_weights)    # once, after initialize_losses
    priors.begin_frame(params)                # each later frame, where train.py calls initialize_per_timestep (train.py:420-438)
    optimise_views(params, dataset, opt, n, priors=priors, is_initial_timestep=...)   # or GraphedViews(..., priors=priors)

`evaluate_torch` is the same set of terms in plain torch (any device): the CPU yardstick the fused kernels are checked against,
itself pinned to tests/golden/g12_topology_priors.npz (the reference's own get_loss).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import ptr

# loss slots of t4d_priors_eval (include/topo4d_raster.h T4D_PRIOR_*), then the total
TERMS = ("scale", "scale_max", "rigid", "rot", "iso", "flat", "flat_lip_bottom", "flat_eye", "flat_face_bottom", "flat_lip_socket",
         "flat_lid_top", "flat_lid_bottom", "flat_lip", "flat_mouth")
EDGE_TERMS = ("flat", "flat_lip_bottom", "flat_lid_top", "flat_lid_bottom", "flat_lip", "flat_mouth")
SOFT_TERMS = EDGE_TERMS[2:]
REGION_TERMS = ("flat_eye", "flat_face_bottom", "flat_lip_socket")
INITIAL_TERMS = ("scale", "scale_max") + SOFT_TERMS
LATER_TERMS = ("rigid", "rot", "iso", "flat", "flat_lip_bottom", "flat_lip_socket", "flat_eye", "flat_face_bottom") + SOFT_TERMS
# losses_weights of train.py:535-540
DEFAULT_WEIGHTS = {"rigid": 3.5, "rot": 20.0, "iso": 20.0, "flat": 2e-4, "flat_lip_bottom": 2e-4, "flat_lid_top": 2e-4,
                   "flat_lid_bottom": 1e-2, "flat_lip": 1e-4, "flat_mouth": 1e-3, "flat_eye": 1e4, "flat_face_bottom": 1e3,
                   "flat_lip_socket": 1e3, "scale": 10.0, "scale_max": 10.0}


def _np(t, dtype):
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(t), dtype=dtype)


def _csr(keys: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """offsets [n+1] and the positions of `keys` grouped by key, ascending within a key (a stable sort)."""
    order = np.argsort(keys, kind="stable").astype(np.int32)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(keys, minlength=n), out=off[1:])
    return off.astype(np.int32), order


class TopologyPriors:
    """The packed topology, weights, per-frame state and scratch of the fused priors.

    Plain-array constructor (the tests use it): `neighbor_indices` [P,K] padded with the vertex's own index (train.py:170-176),
    `neighbor_dist` / `rig_w` / `rot_w` / `iso_w` [P,K], `init_scale` [P], `neighbor_num` [P] (the one-ring sizes) and
    `nbr_mask` [P,K] (FlattenLoss_v2's padding mask; default k < neighbor_num), `edges` {name: (v0s, v1s, v2s, v3s)} for the
    six edge terms, `regions` {name: vertex list} for the three FlattenLoss_v2 terms.  A missing term contributes nothing."""

    def __init__(self, neighbor_indices, neighbor_dist, rig_w, rot_w, iso_w, init_scale, neighbor_num, edges: Dict[str, Sequence],
                 regions: Dict[str, Sequence], nbr_mask=None, weights: Optional[Dict[str, float]] = None, device="cuda"):
        nbr = _np(neighbor_indices, np.int64)
        if nbr.ndim != 2:
            raise ValueError("neighbor_indices must be [P, K]")
        P, K = nbr.shape
        if nbr.min() < 0 or nbr.max() >= P:
            raise ValueError("neighbor_indices out of range")
        self.P, self.K = int(P), int(K)
        self.device = torch.device(device)
        nnum = _np(neighbor_num, np.int32).reshape(P)
        mask = (np.arange(K)[None, :] < nnum[:, None]).astype(np.float32) if nbr_mask is None else _np(nbr_mask, np.float32).reshape(P, K)
        w = dict(DEFAULT_WEIGHTS)
        if weights:
            w.update({k: float(v) for k, v in weights.items() if k in DEFAULT_WEIGHTS})
        self.weights = w
        self.edges_np = {}
        for name in EDGE_TERMS:
            e = edges.get(name)
            a = np.zeros((4, 0), np.int64) if e is None else np.stack([_np(x, np.int64).reshape(-1) for x in e])
            if a.size and (a.min() < 0 or a.max() >= P):
                raise ValueError(f"{name}: edge index out of range")
            self.edges_np[name] = a
        self.regions_np = {}
        for name in REGION_TERMS:
            r = regions.get(name)
            a = np.zeros(0, np.int64) if r is None else _np(r, np.int64).reshape(-1)
            if a.size and (a.min() < 0 or a.max() >= P):
                raise ValueError(f"{name}: region index out of range")
            self.regions_np[name] = a
        self.nbr_np, self.mask_np, self.nnum_np = nbr, mask, nnum

        # transposed incidence lists (CSR): the (Gaussian, slot) pairs naming each vertex, and the position records of the
        # flatten terms naming it, per frame kind (0: frame 0, 1: later frames) - the record layout of t4d_priors_record_layout
        self.nbr_t_off, self.nbr_t_idx = _csr(nbr.reshape(-1), P)
        base, n_rec = {}, 0
        for name in EDGE_TERMS:
            base[name] = n_rec
            n_rec += 4 * self.edges_np[name].shape[1]
        for name in REGION_TERMS:
            base[name] = n_rec
            n_rec += (K + 1) * self.regions_np[name].size
        self.record_base, self.n_records = base, n_rec
        self.rec_csr = []
        for active in (SOFT_TERMS, EDGE_TERMS + REGION_TERMS):
            verts, recs = [], []
            for name in active:
                if name in EDGE_TERMS:
                    e = self.edges_np[name]
                    n = e.shape[1]
                    ids = base[name] + 4 * np.arange(n)[None, :] + np.arange(4)[:, None]
                    verts.append(e.reshape(-1)); recs.append(ids.reshape(-1))
                else:
                    r = self.regions_np[name]
                    ids = base[name] + (K + 1) * np.arange(r.size)[:, None] + np.arange(K + 1)[None, :]
                    vs = np.concatenate([nbr[r], r[:, None]], 1)
                    keep = np.concatenate([mask[r] != 0, np.ones((r.size, 1), bool)], 1)   # padded slots contribute nothing
                    verts.append(vs[keep]); recs.append(ids[keep])
            v = np.concatenate(verts) if verts else np.zeros(0, np.int64)
            rid = np.concatenate(recs) if recs else np.zeros(0, np.int64)
            order = np.lexsort((rid, v))
            off = np.zeros(P + 1, np.int64)
            np.cumsum(np.bincount(v, minlength=P), out=off[1:])
            self.rec_csr.append((off.astype(np.int32), rid[order].astype(np.int32)))

        dev = self.device
        f32 = lambda a: torch.as_tensor(_np(a, np.float32), device=dev).contiguous()
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.int32), device=dev).contiguous()
        self.nbr = i32(nbr)
        self.device = dev = self.nbr.device                 # (with its index: "cuda" -> "cuda:0")
        self.neighbor_dist, self.rig_w, self.rot_w, self.iso_w = (f32(x).reshape(P, K) for x in (neighbor_dist, rig_w, rot_w, iso_w))
        self.init_scale = f32(init_scale).reshape(P)
        self.nbr_mask = f32(mask)
        self.neighbor_num = i32(nnum)
        self.edges = {k: i32(v) for k, v in self.edges_np.items()}
        self.regions = {k: i32(v) for k, v in self.regions_np.items()}
        self._csr_dev = [i32(self.nbr_t_off), i32(self.nbr_t_idx)] + [i32(a) for pair in self.rec_csr for a in pair]
        # per-frame state (initialize_per_timestep, train.py:420-438) and the cached cos of frame 0 (train.py:365-368)
        self.prev_inv_rot_fg = torch.zeros(P, 4, dtype=torch.float32, device=dev)
        self.prev_offset = torch.zeros(P, K, 3, dtype=torch.float32, device=dev)
        self.cos_init = {k: torch.zeros(self.edges_np[k].shape[1], dtype=torch.float32, device=dev) for k in SOFT_TERMS}
        self.losses = torch.zeros(len(TERMS) + 1, dtype=torch.float32, device=dev)
        self._struct = None
        self._scratch = None
        self.grads = None

    # -------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_topo4d(cls, variables: dict, losses_list: dict, losses_weights: Optional[dict] = None, device=None):
        """From Topo4D's own objects after initialize_params / initialize_losses (train.py:177-200, :515-581):
        variables['neighbor_indices' | 'neighbor_dist' | 'rig_w' | 'rot_w' | 'iso_w' | 'init_scale'], the FlattenLoss /
        SoftFlattenLoss buffers .v0s..v3s and the FlattenLoss_v2 .region_mask / .mask / .neighbor_num, as they are."""
        nbr = variables["neighbor_indices"]
        dev = device if device is not None else (nbr.device if torch.is_tensor(nbr) else "cuda")
        edges = {k: (losses_list[k].v0s, losses_list[k].v1s, losses_list[k].v2s, losses_list[k].v3s)
                 for k in EDGE_TERMS if losses_list.get(k) is not None}
        regions = {k: losses_list[k].region_mask for k in REGION_TERMS if losses_list.get(k) is not None}
        v2 = next((losses_list[k] for k in REGION_TERMS if losses_list.get(k) is not None), None)
        if v2 is not None:
            nnum, mask = v2.neighbor_num, _np(v2.mask, np.float32)
            mask = mask[..., 0] if mask.ndim == 3 else mask
        else:
            nnum, mask = (_np(nbr, np.int64) != np.arange(len(nbr))[:, None]).sum(1), None
        return cls(nbr, variables["neighbor_dist"], variables["rig_w"], variables["rot_w"], variables["iso_w"], variables["init_scale"],
                   nnum, edges, regions, nbr_mask=mask, weights=losses_weights, device=dev)

    # -------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def begin_frame(self, params: dict) -> None:
        """The prior state initialize_per_timestep builds at the start of every later frame (train.py:420-438): the inverse of
        the normalised rotation (conjugate) and the one-ring offsets, copied into the buffers the fused evaluation (and any
        recorded graph) reads.  The caller still replaces unnorm_rotations by normalize(normalize(.)) in its optimiser as
        train.py:432-435 does (update_params_and_optimizer)."""
        rot = torch.nn.functional.normalize(params["unnorm_rotations"].detach().to(self.device))
        inv = rot.clone()
        inv[:, 1:] = -1 * inv[:, 1:]
        self.prev_inv_rot_fg.copy_(inv)
        x = params["means3D"].detach().to(self.device)
        self.prev_offset.copy_(x[self.nbr.long()] - x[:, None])

    # -------------------------------------------------------------------------------------------------------------------
    def _pack(self):
        if self._struct is not None:
            return self._struct
        s = _lib.T4DPriors()
        s.P, s.K = self.P, self.K
        p = lambda t: t.data_ptr() if t.numel() else None
        s.nbr, s.nbr_dist, s.rig_w, s.rot_w, s.iso_w = (p(t) for t in (self.nbr, self.neighbor_dist, self.rig_w, self.rot_w, self.iso_w))
        s.nbr_mask, s.nbr_num, s.init_scale = p(self.nbr_mask), p(self.neighbor_num), p(self.init_scale)
        for i, k in enumerate(EDGE_TERMS):
            s.n_edges[i] = self.edges_np[k].shape[1]
            s.edges[i] = p(self.edges[k])
        for i, k in enumerate(REGION_TERMS):
            s.n_region[i] = self.regions_np[k].size
            s.region[i] = p(self.regions[k])
        s.nbr_t_off, s.nbr_t_idx = p(self._csr_dev[0]), p(self._csr_dev[1])
        s.rec_off[0], s.rec_idx[0], s.rec_off[1], s.rec_idx[1] = (p(t) for t in self._csr_dev[2:])
        for i, k in enumerate(TERMS):
            s.weights[i] = self.weights[k]
        s.prev_inv_rot, s.prev_offset = p(self.prev_inv_rot_fg), p(self.prev_offset)
        for i, k in enumerate(SOFT_TERMS):
            s.cos_init[i] = p(self.cos_init[k])
        self._struct = s
        return s

    def record_layout(self):
        """(n_records, {term: first record}) as the library computes it (t4d_priors_record_layout)."""
        base = (C.c_int64 * 9)()
        n = _lib.load().t4d_priors_record_layout(C.byref(self._pack()), base)
        return int(n), dict(zip(EDGE_TERMS + REGION_TERMS, [int(b) for b in base]))

    def detail(self, is_initial_timestep: bool) -> Dict[str, torch.Tensor]:
        """loss_detail of the last evaluation: views of the device buffer the next evaluation overwrites."""
        return {k: self.losses[TERMS.index(k)] for k in (INITIAL_TERMS if is_initial_timestep else LATER_TERMS)}

    def evaluate(self, params: dict, is_initial_timestep: bool, grads: Optional[Sequence[torch.Tensor]] = None, accumulate: bool = True,
                 upstream: Optional[torch.Tensor] = None):
        """The fused priors on the current stream: returns (total, loss_detail) as device scalars (views of `self.losses`, which
        the next evaluation overwrites).  `grads` = (d_means3D, d_unnorm_rotations, d_log_scales) receive upstream * dL/d(raw
        tensor), ADDED to what they hold (accumulate) or written over it; None: `self.grads`, overwritten.  `upstream`: an
        optional device scalar multiplier of the gradients."""
        lib = _lib.load()
        x, q, ls = (params[k].detach() for k in ("means3D", "unnorm_rotations", "log_scales"))
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("TopologyPriors.evaluate runs on the GPU (evaluate_torch is the plain-torch version)")
        for name, t, shape in (("means3D", x, (self.P, 3)), ("unnorm_rotations", q, (self.P, 4)), ("log_scales", ls, (self.P, 3))):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or tuple(t.shape) != shape:
                raise ValueError(f"TopologyPriors.evaluate: {name} must be a contiguous float32 tensor of shape {shape} on {dev}")
        if grads is None:
            if self.grads is None:
                self.grads = (torch.zeros_like(x), torch.zeros_like(q), torch.zeros_like(ls))
            grads, accumulate = self.grads, False
        for g, t in zip(grads, (x, q, ls)):
            if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != t.shape or g.device != dev:
                raise ValueError("TopologyPriors.evaluate: gradient buffers must be contiguous float32 tensors shaped like the parameters")
        if upstream is not None and (upstream.dtype != torch.float32 or upstream.numel() != 1 or upstream.device != dev):
            raise ValueError("TopologyPriors.evaluate: upstream must be a float32 device scalar")
        s = self._pack()
        if self._scratch is None:
            nbytes = lib.t4d_priors_scratch_bytes(C.byref(s))
            if nbytes == 0:
                raise _lib.error("t4d_priors_scratch_bytes")
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.call("t4d_priors_eval", C.byref(s), int(bool(is_initial_timestep)), ptr(x), ptr(q), ptr(ls), ptr(grads[0]), ptr(grads[1]),
                  ptr(grads[2]), ptr(upstream), _lib.T4D_PRIORS_ACCUMULATE if accumulate else 0, ptr(self.losses), ptr(self._scratch),
                  self._scratch.numel(), _lib.stream(dev))
        return self.losses[len(TERMS)], self.detail(is_initial_timestep)

    def as_extra_loss(self, is_initial_timestep: bool):
        """`extra_loss(params, rendervar) -> scalar` for photometric_iteration / optimise_views / GraphedViews: the fused
        evaluation behind an autograd.Function on the raw parameters."""
        def extra(params, rendervar=None):
            return _PriorsFunction.apply(params["means3D"], params["unnorm_rotations"], params["log_scales"], self, bool(is_initial_timestep))
        return extra

    # -------------------------------------------------------------------------------------------------------------------
    def evaluate_torch(self, params: dict, is_initial_timestep: bool):
        """The same terms in plain torch on this object's device, differentiable (the CPU yardstick).  Frame 0 writes the
        detached cos of the soft terms into `cos_init`, as get_loss does.  Returns (total, loss_detail)."""
        dev = self.device
        x = params["means3D"]
        ls = params["log_scales"]
        rot = torch.nn.functional.normalize(params["unnorm_rotations"])
        w = self.weights
        L = {}
        if is_initial_timestep:
            s = torch.exp(ls)
            L["scale"] = s.min(dim=1).values.sum()
            L["scale_max"] = torch.relu(s.max(dim=1).values - self.init_scale * 1.5).sum()
            for k in SOFT_TERMS:
                cos = self._edge_cos(x, k)
                self.cos_init[k].copy_(cos.detach())
                L[k] = ((cos + 1) ** 2).sum()
        else:
            nbr = self.nbr.long()
            rel = _quat_mult(rot, self.prev_inv_rot_fg)
            R = _build_rotation(rel)
            off = x[nbr] - x[:, None]
            v = (R.transpose(2, 1)[:, None] @ off[..., None]).squeeze(-1)
            L["rigid"] = torch.sqrt(((v - self.prev_offset) ** 2).sum(-1) * self.rig_w + 1e-20).mean()
            L["rot"] = torch.sqrt(((rel[nbr] - rel[:, None]) ** 2).sum(-1) * self.rot_w + 1e-20).mean()
            mag = torch.sqrt((off ** 2).sum(-1) + 1e-20)
            L["iso"] = torch.sqrt((mag - self.neighbor_dist) ** 2 * self.iso_w + 1e-20).mean()
            for k in ("flat", "flat_lip_bottom"):
                cos = self._edge_cos(x, k)
                cos = torch.where(cos > 1.0, -1.0, cos)
                L[k] = ((cos + 1) ** 2).sum()
            for k in REGION_TERMS:
                r = self.regions[k].long()
                ave = (x[nbr] * self.nbr_mask[..., None]).sum(1) / self.neighbor_num[:, None]
                L[k] = ((ave[r] - x[r]) ** 2).mean() if r.numel() else x.new_zeros(())    # a missing term contributes nothing
            for k in SOFT_TERMS:
                cos = self._edge_cos(x, k)
                L[k] = (1 - torch.cos(torch.abs(torch.arccos(cos) - torch.arccos(self.cos_init[k])))).sum()
        order = INITIAL_TERMS if is_initial_timestep else LATER_TERMS
        detail = {k: w[k] * L[k] for k in order}
        total = sum(detail[k] for k in order)
        return total, detail

    def _edge_cos(self, x, name):
        """cos of the dihedral angle across each interior edge (FlattenLoss / SoftFlattenLoss geometry, eps 1e-6)."""
        eps = 1e-6
        e = self.edges[name].long()
        v0, v1, v2, v3 = x[e[0]], x[e[1]], x[e[2]], x[e[3]]
        a = v1 - v0

        def side(b):
            al2, bl2 = (a * a).sum(-1), (b * b).sum(-1)
            al1, bl1 = (al2 + eps).sqrt(), (bl2 + eps).sqrt()
            ab = (a * b).sum(-1)
            cosi = ab / (al1 * bl1 + eps)
            sin = (1 - cosi ** 2 + eps).sqrt()
            cb = b - a * (ab / (al2 + eps))[:, None]
            return cb, bl1 * sin
        cb1, l1 = side(v2 - v0)
        cb2, l2 = side(v3 - v0)
        return (cb1 * cb2).sum(-1) / (l1 * l2 + eps)


def _quat_mult(a, b):
    w1, x1, y1, z1 = a.unbind(-1)
    w2, x2, y2, z2 = b.unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def _build_rotation(q):
    q = q / torch.sqrt((q * q).sum(-1))[:, None]
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)


class _PriorsFunction(torch.autograd.Function):
    """total = the fused priors of (means3D, unnorm_rotations, log_scales); the gradients are computed by the same evaluation
    into fresh buffers and scaled by the incoming gradient in backward."""

    @staticmethod
    def forward(ctx, means3D, unnorm_rotations, log_scales, priors: TopologyPriors, is_initial: bool):
        grads = (torch.empty_like(means3D), torch.empty_like(unnorm_rotations), torch.empty_like(log_scales))
        total, _ = priors.evaluate({"means3D": means3D, "unnorm_rotations": unnorm_rotations, "log_scales": log_scales}, is_initial,
                                   grads=grads, accumulate=False)
        ctx.save_for_backward(*grads)
        return total.clone()

    @staticmethod
    def backward(ctx, g):
        gx, gq, gs = ctx.saved_tensors
        return gx * g, gq * g, gs * g, None, None
