"""
A per-term, per-vertex yardstick for the topology priors' gradients (t4d_priors_eval), from a float64 restatement of the terms
alone (no product kernels, no GPU).

tests/test_gpu_priors.py holds the SUM of all terms, at weights spanning eight decades, to 1e-4 of each tensor's largest entry:
rigid's whole position gradient is 3.6e-5 of that entry on G12 and could be zero.  Here every term is taken alone and every
vertex answers to its own scale:

    elements   {term: per-element losses, float64, the reference's denominators}: [P, K] for rigid / rot / iso (/ P K), [n_edges]
               for the six edge terms, [n_region] for the three region terms (row sum / 3 n_region), [P] for scale / scale_max -
               the formulas of train.py:328-368, helpers.py:126-144 and loss_util.py; weight * elements.sum() is
               evaluate_torch's detail[term] (itself pinned to G12) to 1e-12 relative
    t          weight * the float64 gradient of sum_e L_e - the truth
    n          the RMS over K_SIGNS = 4 backward passes of weight * sum_e s_e L_e, seeded signs s_e = +-1 per element: the size
               the row's sum has when nothing cancels by luck
    S_i        max over the components of row i of max(|t|, n)

so that a vertex at rest whose neighbour contributions cancel answers to the size of those contributions, not to zero.

check_rows: max|g - t| over row i <= PRIORS_REL * S_i wherever S_i > 0, EXACTLY zero wherever S_i == 0 (log_scales in later
frames, unnorm_rotations in frame 0 and in every term but rigid / rot, vertices no element of the term names), no NaN or inf.

The one kink.  iso is sqrt((|off| - dist)^2 w + 1e-20), in effect sqrt(w) | |off| - dist |: where both ends of a pair moved
alike, |off| - dist is rounding noise and the element's gradient jumps between +-coef sqrt(w) off / |off|.  An element is a TIE
if, in float64, | |off| - dist | < 2^-20 |off|; a row a tie names, as the Gaussian or as the neighbour, is held to
PRIORS_REL * S_i + sum over its ties of 2 coef sqrt(w_e) - the jump's size.  Ties may touch at most 0.5 % of the term's live
rows (G12: 17 ties, 18 of 5,166 rows) and touch none on the synthetic cases.  rigid and rot have the same form at d = 0; no
element of any case sits there (tests/test_priors_rows_host.py asserts all of this from the float64 inputs alone).

The module also names the CASES, each in both frame kinds: G12 (the real facial topology, P = 8,280, K = 14) and the lat-lon head
of tests/test_gpu_priors.grid_priors at 12 x 20 (P = 240: one partly filled block of the vertex launch) and 19 x 27 (P = 513 =
2 * 256 + 1: a single thread in the last block of the vertex launch and of the neighbour segment).  The two grids exercise what
G12 leaves idle: relative rotations far from the identity and raw quaternions of norm 0.5 .. 2, every iso element away from its
kink, soft terms on both sides of their cos_init, an absent edge term and an absent region term, an edge term of exactly 256
elements, masked middle neighbour slots, rows of three equal scales and scale_max on both sides of its threshold.  Their
vertices are placed so that the dihedral terms are well conditioned in float32 (`_grid`: no edge close to flat or folded, no
sliver triangle, no soft element at its cos_init): the fp32 plain-torch evaluation has to meet PRIORS_REL / 4 on every row of
every case, and a smooth head does not let it - a near-flat edge loses (cos + 1) and acos' argument to cancellation, in any
fp32 evaluation.  Seeds and conditions were chosen on the CPU from the references alone.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

import numpy as np
import torch

from tests.test_priors_host import KEYS, _golden, frame0_cos_init
from topo4d_amd import priors as T

PRIORS_REL = 1e-4
K_SIGNS = 4
SIGN_SEED = 9200
TIE = 2.0 ** -20                 # | |off| - dist | below this share of |off|: an iso tie
TIE_ROWS = 0.005                 # ties may touch this share of iso's live rows
CLEAR = 2.0 ** -10               # the grids keep every live iso element this far from its kink
NBR_TERMS = ("rigid", "rot", "iso")


# ----------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# ----------------------------------------------------------------------------------------------------------------------
def _dihedral(x, e):
    """loss_util.py FlattenLoss.forward:171-208: (cos of the angle between the two triangles' heights over the edge (v0, v1), and
    the sines of the two triangles' angles at v0)."""
    eps = 1e-6
    v0, v1, v2, v3 = (x[..., e[j], :] for j in range(4))
    a = v1 - v0

    def height(b):
        al2, bl2 = a.pow(2).sum(-1), b.pow(2).sum(-1)
        al1, bl1 = (al2 + eps).sqrt(), (bl2 + eps).sqrt()
        ab = (a * b).sum(-1)
        cos = ab / (al1 * bl1 + eps)
        sin = (1 - cos.pow(2) + eps).sqrt()
        return b - a * (ab / (al2 + eps))[..., None], bl1 * sin, sin
    cb1, l1, s1 = height(v2 - v0)
    cb2, l2, s2 = height(v3 - v0)
    return (cb1 * cb2).sum(-1) / (l1 * l2 + eps), s1, s2


def _dihedral_cos(x, e):
    return _dihedral(x, e)[0]


def _rel_rot(pr, q):
    """helpers.quat_mult(F.normalize(unnorm_rotations), prev_inv_rot_fg) (train.py:330-331)."""
    n = q / q.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    w1, x1, y1, z1 = n.unbind(-1)
    w2, x2, y2, z2 = pr.prev_inv_rot_fg.double().unbind(-1)
    return torch.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                        w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def _rotate_back(rel, off):
    """R(rel)^T off, R = build_rotation(rel) (external.py:26-43: it normalises again, without an epsilon), per neighbour slot."""
    u = rel / rel.pow(2).sum(-1, keepdim=True).sqrt()
    r, x, y, z = (u[:, j, None] for j in range(4))
    ox, oy, oz = off.unbind(-1)
    return torch.stack([(1 - 2 * (y * y + z * z)) * ox + 2 * (x * y + r * z) * oy + 2 * (x * z - r * y) * oz,
                        2 * (x * y - r * z) * ox + (1 - 2 * (x * x + z * z)) * oy + 2 * (y * z + r * x) * oz,
                        2 * (x * z + r * y) * ox + 2 * (y * z - r * x) * oy + (1 - 2 * (x * x + y * y)) * oz], -1)


def elements(pr, params, is_initial):
    """{term: float64 per-element losses, unweighted, with the reference's denominators} of the terms of this frame kind.  `pr`: a
    TopologyPriors on the CPU (topology and per-frame state); `params`: float64 tensors (leaves, to differentiate)."""
    x, q, ls = (params[k].double() for k in KEYS)
    L = {}
    if is_initial:
        s = torch.exp(ls)
        L["scale"] = s.min(dim=1).values
        L["scale_max"] = torch.relu(s.max(dim=1).values - (pr.init_scale * 1.5).double())     # the threshold: a float32 constant
        for k in T.SOFT_TERMS:
            L[k] = (_dihedral_cos(x, pr.edges[k].long()) + 1).pow(2)
        return L
    nbr, PK = pr.nbr.long(), pr.P * pr.K
    rel = _rel_rot(pr, q)
    off = x[nbr] - x[:, None]
    d = _rotate_back(rel, off) - pr.prev_offset.double()
    L["rigid"] = (d.pow(2).sum(-1) * pr.rig_w.double() + 1e-20).sqrt() / PK                 # weighted_l2_loss_v2
    L["rot"] = ((rel[nbr] - rel[:, None]).pow(2).sum(-1) * pr.rot_w.double() + 1e-20).sqrt() / PK
    mag = (off.pow(2).sum(-1) + 1e-20).sqrt()
    L["iso"] = ((mag - pr.neighbor_dist.double()).pow(2) * pr.iso_w.double() + 1e-20).sqrt() / PK   # weighted_l2_loss_v1
    for k in ("flat", "flat_lip_bottom"):
        cos = _dihedral_cos(x, pr.edges[k].long())
        L[k] = (torch.where(cos > 1.0, -1.0, cos) + 1).pow(2)
    ave = (x[nbr] * pr.nbr_mask.double()[..., None]).sum(1) / pr.neighbor_num.double()[:, None]
    for k in T.REGION_TERMS:
        r = pr.regions[k].long()
        L[k] = (ave[r] - x[r]).pow(2).sum(-1) / max(3 * r.numel(), 1)
    for k in T.SOFT_TERMS:
        cos = _dihedral_cos(x, pr.edges[k].long())
        L[k] = 1 - torch.cos(torch.abs(torch.arccos(cos) - torch.arccos(pr.cos_init[k].double())))
    return L


def terms_of(is_initial):
    return T.INITIAL_TERMS if is_initial else T.LATER_TERMS


# ----------------------------------------------------------------------------------------------------------------------
# the yardstick
# ----------------------------------------------------------------------------------------------------------------------
class Yard(NamedTuple):
    loss: Dict[str, float]                      # weight * sum of the elements
    truth: Dict[str, Dict[str, np.ndarray]]     # [term][tensor] -> [P, w] float64
    S: Dict[str, Dict[str, np.ndarray]]         # [term][tensor] -> [P]
    extra: np.ndarray                           # [P]: iso's allowance on means3D rows that ties name (0 elsewhere)
    info: dict                                  # the kink statistics the host test asserts


def _grads(loss, leaves):
    g = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    return [np.zeros(tuple(p.shape)) if a is None else a.numpy().copy() for a, p in zip(g, leaves)]


def iso_state(pr, params):
    """(live [P,K], rel [P,K] = | |off| - dist | / |off|, jump [P,K] = 2 coef sqrt(w)) of iso, float64 inputs alone."""
    x = params["means3D"].detach().double()
    nbr = pr.nbr.long()
    mag = ((x[nbr] - x[:, None]).pow(2).sum(-1) + 1e-20).sqrt()
    w = pr.iso_w.double()
    rel = (mag - pr.neighbor_dist.double()).abs() / mag
    return (w > 0).numpy(), rel.numpy(), (2 * pr.weights["iso"] / (pr.P * pr.K) * w.sqrt()).numpy()


def yardstick(pr, params, is_initial) -> Yard:
    p64 = {k: params[k].detach().double().clone().requires_grad_(True) for k in KEYS}
    leaves = [p64[k] for k in KEYS]
    L = elements(pr, p64, is_initial)
    loss, truth, S = {}, {}, {}
    for term in terms_of(is_initial):
        e, w = L[term], pr.weights[term]
        loss[term] = w * float(e.detach().sum())
        t = _grads(w * e.sum(), leaves) if e.numel() else [np.zeros(tuple(p.shape)) for p in leaves]
        sq = [np.zeros_like(a) for a in t]
        for j in range(K_SIGNS if e.numel() else 0):
            g = torch.Generator().manual_seed(SIGN_SEED + 16 * j + T.TERMS.index(term))
            s = torch.randint(0, 2, e.shape, generator=g).double() * 2 - 1
            for a, b in zip(sq, _grads(w * (s * e).sum(), leaves)):
                a += b ** 2
        truth[term] = dict(zip(KEYS, t))
        S[term] = {k: np.maximum(np.abs(a), np.sqrt(b / K_SIGNS)).max(axis=1) for k, a, b in zip(KEYS, t, sq)}
    extra, info = np.zeros(pr.P), {}
    if not is_initial:
        live, rel, jump = iso_state(pr, params)
        tie = live & (rel < TIE)
        nbr = pr.nbr_np
        np.add.at(extra, np.nonzero(tie)[0], jump[tie])
        np.add.at(extra, nbr[tie], jump[tie])
        named = np.zeros(pr.P, bool)
        named[np.nonzero(live)[0]] = True
        named[nbr[live]] = True
        info = {"iso_live": int(live.sum()), "iso_ties": int(tie.sum()), "iso_live_rows": int(named.sum()),
                "iso_tie_rows": int((extra > 0).sum()), "iso_min_rel": float(rel[live].min()) if live.any() else np.inf}
        with torch.no_grad():
            x, nb = p64["means3D"], pr.nbr.long()
            relq = _rel_rot(pr, p64["unnorm_rotations"])
            d = _rotate_back(relq, x[nb] - x[:, None]) - pr.prev_offset.double()
            po = pr.prev_offset.double().pow(2).sum(-1).sqrt()
            dq = (relq[nb] - relq[:, None]).pow(2).sum(-1).sqrt()
            info["rigid_at_kink"] = int(((d.pow(2).sum(-1).sqrt() < TIE * po) & (pr.rig_w > 0)).sum())
            info["rot_at_kink"] = int(((dq < TIE) & (pr.rot_w > 0)).sum())
    if "flat_lid_top" in L:
        with torch.no_grad():
            sign = {}
            for k in T.SOFT_TERMS:
                if is_initial or not L[k].numel():
                    continue
                t = torch.arccos(_dihedral_cos(p64["means3D"], pr.edges[k].long())) - torch.arccos(pr.cos_init[k].double())
                sign[k] = (float((t > 0).double().mean()), float((t < 0).double().mean()))
            info["soft_sign_share"] = sign
    return Yard(loss, truth, S, extra, info)


def named_by(pr, term, i, limit=6):
    """The elements of `term` that name vertex i, for a failure message."""
    if term in NBR_TERMS:
        own = [f"({i},{k})->{int(pr.nbr_np[i, k])}" for k in range(pr.K)]
        g, k = np.nonzero(pr.nbr_np == i)
        other = [f"({a},{b})" for a, b in zip(g, k) if a != i]
        return f"own slots {own[:limit]}, named by slots {other[:limit]}" + (" ..." if len(other) > limit else "")
    if term in T.EDGE_TERMS:
        e = np.nonzero((pr.edges_np[term] == i).any(axis=0))[0]
        return f"edges {[(int(j), pr.edges_np[term][:, j].tolist()) for j in e[:limit]]}" + (" ..." if len(e) > limit else "")
    if term in T.REGION_TERMS:
        r = pr.regions_np[term]
        ring = ((pr.nbr_np[r] == i) & (pr.mask_np[r] != 0)).any(axis=1)
        e = np.nonzero((r == i) | ring)[0]
        return f"region elements {[(int(j), int(r[j])) for j in e[:limit]]}" + (" ..." if len(e) > limit else "")
    return f"element {i}"


def row_ratios(g, t, S, extra=None):
    """(err [P], ratio [P]) of one tensor: err = max|g - t| over the row, ratio = max(err - extra, 0) / S_i where S_i > 0, else 0."""
    g, t = np.asarray(g, np.float64).reshape(len(S), -1), np.asarray(t, np.float64).reshape(len(S), -1)
    err = np.abs(g - t).max(axis=1)
    over = err if extra is None else np.maximum(err - extra, 0.0)
    held = S > 0
    return err, np.where(held, over / np.where(held, S, 1.0), 0.0)


def check_rows(g, t, S, bound, extra=None, what="", names: Optional[Callable[[int], str]] = None):
    """Every row of the gradient `g` ([P, w]) against the float64 truth `t`, relative to its own scale S_i (module docstring);
    `extra` [P]: an absolute allowance per row (iso's ties).  `what` names term and tensor, `names(i)` the elements that name
    vertex i.  Returns the worst err / S_i."""
    g = np.asarray(g, np.float64).reshape(len(S), -1)
    bad = np.nonzero(~np.isfinite(g).all(axis=1))[0]
    assert len(bad) == 0, f"{what}: vertex {bad[0]}: gradient {g[bad[0]]} is not finite ({len(bad)} rows)"
    null = np.nonzero((S == 0) & (np.abs(g).max(axis=1) != 0))[0]
    who = lambda i: "" if names is None else f"; {names(int(i))}"
    assert len(null) == 0, f"{what}: vertex {null[0]}: row scale 0 but gradient {g[null[0]]} ({len(null)} rows){who(null[0])}"
    err, ratio = row_ratios(g, t, S, extra)
    i = int(ratio.argmax())
    assert ratio[i] <= bound, (f"{what}: vertex {i}: err {err[i]:.3e} vs its row scale S_i {S[i]:.3e}" +
                               (f" (+ tie allowance {extra[i]:.3e})" if extra is not None and extra[i] else "") +
                               f": err / S_i {ratio[i]:.3e} > {bound:g} ({int((ratio > bound).sum())} rows over){who(i)}")
    return float(ratio[i])


def extra_of(yard, term, key):
    return yard.extra if term == "iso" and key == "means3D" else None


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    build: Callable            # (device, weights or None) -> TopologyPriors with the frame's state (later frames: begin_frame, cos_init)
    params: Dict[str, torch.Tensor]       # float32, CPU
    is_initial: bool


def only(pr_weights, term):
    """The weights of a one-term evaluation: that term at its weight, every other term 0."""
    return {k: (v if k == term else 0.0) for k, v in pr_weights.items()}


def _g12_priors(z, device, weights):
    w = dict(zip([str(s) for s in z["weight_names"]], z["weights"]))
    w.update(weights or {})
    edges = {k: tuple(z[f"{k}_{s}"] for s in ("v0s", "v1s", "v2s", "v3s")) for k in T.EDGE_TERMS}
    regions = {k: z[f"{k}_region"] for k in T.REGION_TERMS}
    return T.TopologyPriors(z["neighbor_indices"], z["neighbor_dist"], z["rig_w"], z["rot_w"], z["iso_w"], z["init_scale"],
                            z["neighbor_num"], edges, regions, weights=w, device=device)


def _g12(is_initial):
    z = _golden()
    p0 = {k: torch.tensor(z[f"f0_in_{k}"]) for k in KEYS}
    cos0 = None if is_initial else frame0_cos_init(z)       # the reference's cos_init (tests/test_priors_host.py)

    def build(device="cpu", weights=None):
        pr = _g12_priors(z, device, weights)
        if not is_initial:
            pr.begin_frame(p0)
            for k, c in cos0.items():
                pr.cos_init[k].copy_(c)
        return pr
    return Case("g12", build, p0 if is_initial else {k: torch.tensor(z[f"f1_in_{k}"]) for k in KEYS}, is_initial)


# the grids' topology: flat_lid_top and flat_face_bottom absent, flat_lip exactly one full block, a masked middle slot on every
# seventh vertex
GRID_SHAPES = {"grid240": (12, 20, 21), "grid513": (19, 27, 21)}         # n_lat, n_lon, seed
GRID_TOPOLOGY = dict(n_edges={"flat_lid_top": 0, "flat_lip": 256}, no_regions=("flat_face_bottom",), drop_slot_every=7)
GRID_LAT_MAX = 50.0              # degrees: the band of the head the grids cover
GRID_FOLD = 0.8                  # the undisplaced mesh: every third vertex above the ellipsoid by this share of the latitude spacing h,
GRID_ROUGH = 0.1                 # and every vertex moved from there by N(0, 1) times this share of h
GRID_COS_MAX = 0.95              # every edge element, before and after the displacement: |cos| of its dihedral angle at most this,
GRID_SIN_MIN = 0.3               # and the sine of both triangles' angles at v0 at least this
GRID_SEAM = 0.4                  # where the fold leaves an edge flat (the seam of a grid whose n_lon is no multiple of 3), its vertices are
                                 # drawn again with this share of h
GRID_TURN_MIN = 0.05             # radians: every soft element's angle differs from its cos_init's by at least this
GRID_MOVE = 0.15                 # the displacement of every vertex from there, as a share of h


def _settled(start, share, again, g, checks):
    """start + share N(0, 1) per vertex, then, vertex by vertex, the vertices named by an element that fails a check are drawn
    again (start + again N(0, 1)) until every element that names the vertex passes: no element that passed fails afterwards.
    `checks`: [(vertices [r, n] of the n elements, ok(X [..., P, 3], elements) -> bool [..., n])]."""
    P = start.shape[0]
    x = start + share * torch.randn(P, 3, generator=g)
    for _ in range(100):
        rows = set()
        for idx, ok in checks:
            rows |= set(idx[:, ~ok(x, torch.arange(idx.shape[1]))].reshape(-1).tolist())
        if not rows:
            return x.contiguous()
        for v in sorted(rows):
            X = x.expand(256, P, 3).clone()
            X[:, v] = start[v] + again * torch.randn(256, 3, generator=g)
            good = torch.ones(256, dtype=torch.bool)
            for idx, ok in checks:
                good &= ok(X, torch.nonzero((idx == v).any(0))[:, 0]).all(-1)
            if good.any():
                x[v] = X[int(torch.nonzero(good)[0]), v]
    raise AssertionError(f"no mesh met the conditions ({len(rows)} vertices left)")


def _grid(name):
    """Both frame kinds of a grid: one mesh, one set of parameters."""
    from scaffold import scene
    from tests.test_gpu_priors import grid_priors
    n_lat, n_lon, seed = GRID_SHAPES[name]
    P = n_lat * n_lon
    g = torch.Generator().manual_seed(seed)
    # the undisplaced mesh: the band of scaffold.scene's head between latitudes +-GRID_LAT_MAX in grid_priors' vertex order - the
    # rows next to the poles are triangles eight times longer than wide, whose sin = sqrt(1 - cos^2 + eps) no fp32 evaluation
    # resolves - folded so that no dihedral angle is close to flat, where (cos + 1)^2 and acos lose their digits alike: the
    # vertices of every triangle away from the seam have the three values of (i + j) mod 3, and those of one value stand above the
    # ellipsoid (the four vertices of an edge and its two triangles are coplanar where the opposite vertices' height is the mean
    # of the edge's: no three heights in arithmetic progression); then roughened
    lat = torch.linspace(-GRID_LAT_MAX, GRID_LAT_MAX, n_lat, dtype=torch.float64) * (np.pi / 180)
    lon = torch.arange(n_lon, dtype=torch.float64) * (2 * np.pi / n_lon)
    la, lo = torch.meshgrid(lat, lon, indexing="ij")
    unit = torch.stack([la.cos() * lo.sin(), la.sin(), la.cos() * lo.cos()], -1).reshape(P, 3)
    h = float(lat[1] - lat[0]) * scene.SEMI_AXES[1]
    smooth = (unit * torch.tensor(scene.SEMI_AXES, dtype=torch.float64)).float()
    topo = grid_priors(n_lat, n_lon, smooth, seed=seed, device="cpu", **GRID_TOPOLOGY)
    every = torch.cat([topo.edges[k].long() for k in T.EDGE_TERMS], 1)

    def shaped(X, sel):
        cos, s1, s2 = _dihedral(X.double(), every[:, sel])
        return (cos.abs() <= GRID_COS_MAX) & (torch.minimum(s1, s2) >= GRID_SIN_MIN)
    fold = torch.tensor([0.0, 0.0, 1.0])[(torch.arange(n_lat)[:, None] + torch.arange(n_lon)[None, :]).reshape(P) % 3]
    x0 = _settled(smooth + GRID_FOLD * h * fold[:, None] * unit.float(), GRID_ROUGH * h, GRID_SEAM * h, g, [(every, shaped)])
    q_prev = torch.nn.functional.normalize(torch.randn(P, 4, generator=g))
    prev = {"means3D": x0, "unnorm_rotations": q_prev, "log_scales": torch.full((P, 3), float(np.log(h / 2)))}
    cos0 = {}

    def build(device="cpu", weights=None, is_initial=False):
        pr = grid_priors(n_lat, n_lon, x0, seed=seed, device=device, weights=weights, **GRID_TOPOLOGY)
        if not is_initial:
            pr.begin_frame(prev)
            if not cos0:                                     # cos_init at the undisplaced mesh, from the plain-torch evaluation
                ref = grid_priors(n_lat, n_lon, x0, seed=seed, device="cpu", **GRID_TOPOLOGY)
                ref.evaluate_torch(prev, True)
                cos0.update({k: v.clone() for k, v in ref.cos_init.items()})
            for k, c in cos0.items():
                pr.cos_init[k].copy_(c)
        return pr

    pr = build()
    # current rotations: drawn independently of the previous ones, norms in [0.5, 2] - large relative angles, F.normalize's den != 1
    q = torch.nn.functional.normalize(torch.randn(P, 4, generator=g)) * (0.5 + 1.5 * torch.rand(P, 1, generator=g))
    # every vertex displaced: the edges keep their shape, every soft element's angle moves by GRID_TURN_MIN at the least (a vertex
    # may be named by one soft element alone, whose gradient is proportional to sin of that move and has its relative error), and
    # no live iso element is closer than 2 CLEAR to its kink
    soft = torch.cat([pr.edges[k].long() for k in T.SOFT_TERMS], 1)
    angle0 = torch.arccos(_dihedral_cos(x0.double(), soft).float().double())
    pairs = torch.stack([torch.arange(P)[:, None].expand(P, pr.K), pr.nbr.long()]).reshape(2, -1)[:, (pr.iso_w > 0).reshape(-1)]
    dist = pr.neighbor_dist.double().reshape(-1)[(pr.iso_w > 0).reshape(-1)]

    def turned(X, sel):
        return (torch.arccos(_dihedral_cos(X.double(), soft[:, sel])) - angle0[sel]).abs() >= GRID_TURN_MIN

    def clear(X, sel):
        mag = (X.double()[..., pairs[1, sel], :] - X.double()[..., pairs[0, sel], :]).pow(2).sum(-1).sqrt()
        return (mag - dist[sel]).abs() >= 2 * CLEAR * mag
    x = _settled(x0, GRID_MOVE * h, GRID_MOVE * h, g, [(every, shaped), (soft, turned), (pairs, clear)])
    # log_scales: the largest scale of a row is 1.5 init_scale x 0.7 or x 1.3 (scale_max on both sides of its threshold); every
    # fifth row has three equal entries, the others one column at the largest and two below it
    top = torch.log(pr.init_scale * 1.5 * torch.where(torch.rand(P, generator=g) < 0.5, 0.7, 1.3))
    below = -(0.05 + 0.3 * torch.randn(P, 3, generator=g).abs())
    below[torch.arange(P), torch.randint(0, 3, (P,), generator=g)] = 0.0
    below[::5] = 0.0
    ls = top[:, None] + below
    params = {"means3D": x.contiguous(), "unnorm_rotations": q.contiguous(), "log_scales": ls.contiguous()}
    return {"initial": Case(name, lambda device="cpu", weights=None: build(device, weights, True), params, True),
            "later": Case(name, build, params, False)}


NAMES = ("g12", "grid240", "grid513")
FRAMES = ("initial", "later")
_CASES: Dict[tuple, Case] = {}
_PREPARED: Dict[tuple, tuple] = {}


def case(name, frame) -> Case:
    if (name, frame) not in _CASES:
        if name == "g12":
            _CASES[(name, frame)] = _g12(frame == "initial")
        else:
            _CASES.update({(name, f): c for f, c in _grid(name).items()})
    return _CASES[(name, frame)]


def prepared(name, frame):
    """(case, the CPU TopologyPriors at the default weights, the float64 yardstick), computed once per process, left unchanged."""
    if (name, frame) not in _PREPARED:
        c = case(name, frame)
        pr = c.build()
        _PREPARED[(name, frame)] = (c, pr, yardstick(pr, c.params, c.is_initial))
    return _PREPARED[(name, frame)]
