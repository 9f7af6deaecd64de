"""
Yardsticks of the photo-consistency check of topo4d_amd.projtex (k_projtex_consist and the masks of k_projtex / k_projtex_bands in
csrc/t4d_projtex.hip), on the host:

    samples(pos, nrm, coverage, views, sizes, photos, depths, ...)     steps A.1..A.3 per view: (accepted, voter bool [V,h,w], q int64 [V,h,w,3])
    consistency(...)                                                   the whole t4d_projtex_consistency: (skip uint32 [h,w], votes uint8 [h,w])
    project_texture(..., skip=None, skip_base=0)                       the whole t4d_project_texture_skip: (color, weight, count)
    project_bands(..., skip=None, skip_base=0)                         the whole t4d_project_texture_bands_skip
    popcount(skip)                                                     the number of rejected views per texel

Steps 1..6 are tests/projtex_ref.view_samples, which performs the kernel's operations in the kernel's order, so every q agrees bit
for bit; everything after it is integer arithmetic.  consistency runs texel by texel, as the rule is written down in
include/topo4d_raster.h.  The masked blends are those of tests/projtex_ref.py and tests/projtex_bands_ref.py with a masked view
taken as one the rule does not accept.
"""
from __future__ import annotations

import numpy as np

from tests.projtex_ref import view_samples

SCALE = 65536.0
CLAMP = 4.0


def samples(pos, nrm, coverage, views, sizes, photos, depths, power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002, gains=None,
            vote_cos_min=0.5):
    """(accepted bool [V,h,w], voter bool [V,h,w], q int64 [V,h,w,3]).  sizes [V] of (h, w); photos [V] of [3,h_v,w_v]; depths [V]
    of [h_v,w_v] (or [1,h_v,w_v])"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    acc, vot, q = [], [], []
    for v in range(len(views)):
        H, W = (int(x) for x in sizes[v])
        ok, cs, _, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depths[v], power, cos_min, fade_px, depth_tol,
                                    None if gains is None else gains[v])
        with np.errstate(all="ignore"):
            clamped = np.where(s >= 0.0, np.where(s <= CLAMP, s, CLAMP), 0.0)      # a NaN fails the first comparison: 0
            qi = np.rint(np.where(ok[..., None], clamped, 0.0) * SCALE).astype(np.int64)   # half to even, as llrint
            acc.append(ok)
            vot.append(ok & (cs >= float(vote_cos_min)))
        q.append(qi)
    return np.stack(acc), np.stack(vot), np.stack(q)


def texel_rule(accepted, voters, q, qt: int, min_votes: int):
    """(skip word, n) of one texel: accepted / voters the lists of view indices, q {view: (q0, q1, q2)}; steps A.3..A.6"""
    n = len(voters)
    if n < min_votes:
        return 0, n
    m = [sorted((q[v][c], v) for v in voters)[(n - 1) // 2][0] for c in range(3)]
    outliers = [v for v in accepted if max(abs(q[v][c] - m[c]) for c in range(3)) > qt]
    if len(outliers) == len(accepted):
        return 0, n
    return sum(1 << v for v in outliers), n


def consistency(pos, nrm, coverage, views, sizes, photos, depths, power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002, gains=None,
                reject_tol=0.1, vote_cos_min=0.5, min_votes=3):
    """(skip uint32 [h,w], votes uint8 [h,w])"""
    acc, vot, q = samples(pos, nrm, coverage, views, sizes, photos, depths, power, cos_min, fade_px, depth_tol, gains, vote_cos_min)
    V, th, tw = acc.shape
    qt = int(np.rint(float(reject_tol) * SCALE))
    skip, votes = np.zeros((th, tw), np.uint32), np.zeros((th, tw), np.uint8)
    for y in range(th):
        for x in range(tw):
            accepted = [v for v in range(V) if acc[v, y, x]]
            if not accepted:
                continue
            voters = [v for v in accepted if vot[v, y, x]]
            word, n = texel_rule(accepted, voters, {v: tuple(int(a) for a in q[v, y, x]) for v in accepted}, qt, int(min_votes))
            skip[y, x], votes[y, x] = word, n
    return skip, votes


def popcount(skip):
    s = np.asarray(skip).astype(np.int64) & 0xFFFFFFFF
    return sum((s >> i) & 1 for i in range(32)).astype(np.uint8)


def _masked(skip, skip_base: int, v: int, shape):
    """bool [h,w]: where view v of the launch is masked"""
    if skip is None:
        return np.zeros(shape, bool)
    return ((np.asarray(skip).astype(np.int64) & 0xFFFFFFFF) >> (int(skip_base) + v)) & 1 != 0


def project_texture(pos, nrm, coverage, views, H: int, W: int, photos, depth, power: int = 2, cos_min: float = 0.1,
                    fade_px: float = 16.0, depth_tol: float = 0.002, mode: str = "weighted", gains=None, skip=None, skip_base: int = 0):
    """tests/projtex_ref.project_texture with the mask: (color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8)"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    photos, depth = np.asarray(photos, np.float32), np.asarray(depth, np.float32)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    th, tw = np.asarray(pos).shape[:2]
    best = {"weighted": False, "best": True}[mode]
    sw, sc, cnt = np.zeros((th, tw)), np.zeros((th, tw, 3)), np.zeros((th, tw), dtype=np.int64)
    with np.errstate(all="ignore"):
        for v in range(len(views)):
            ok, _, w, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depth[v], power, cos_min, fade_px, depth_tol,
                                       None if gains is None else gains[v])
            ok = ok & ~_masked(skip, skip_base, v, (th, tw))
            cnt += ok
            if best:
                take = ok & (w > sw)
                sw = np.where(take, w, sw)
                sc = np.where(take[..., None], s, sc)
            else:
                sw = np.where(ok, sw + w, sw)
                sc = np.where(ok[..., None], sc + w[..., None] * s, sc)
        if not best:
            sc = np.where((cnt > 0)[..., None], sc / sw[..., None], 0.0)
    return sc.astype(np.float32), sw.astype(np.float32), cnt.astype(np.uint8)


def project_bands(pos, nrm, coverage, views, H: int, W: int, photos, low, depth, power: int = 2, cos_min: float = 0.1,
                  fade_px: float = 16.0, depth_tol: float = 0.002, gains=None, skip=None, skip_base: int = 0):
    """tests/projtex_bands_ref.project_bands with the mask: (low_color, weight, count, high, best_weight)"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    photos, low, depth = np.asarray(photos, np.float32), np.asarray(low, np.float32), np.asarray(depth, np.float32)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    th, tw = np.asarray(pos).shape[:2]
    sw, bw, cnt = np.zeros((th, tw)), np.zeros((th, tw)), np.zeros((th, tw), dtype=np.int64)
    sl, hb = np.zeros((th, tw, 3)), np.zeros((th, tw, 3))
    with np.errstate(all="ignore"):
        for v in range(len(views)):
            g = None if gains is None else gains[v]
            ok, _, w, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depth[v], power, cos_min, fade_px, depth_tol, g)
            _, _, _, l = view_samples(pos, nrm, coverage, views[v], H, W, low[v], depth[v], power, cos_min, fade_px, depth_tol, g)
            ok = ok & ~_masked(skip, skip_base, v, (th, tw))
            cnt += ok
            sw = np.where(ok, sw + w, sw)
            sl = np.where(ok[..., None], sl + w[..., None] * l, sl)
            take = ok & (w > bw)
            bw = np.where(take, w, bw)
            hb = np.where(take[..., None], s - l, hb)
        sl = np.where((cnt > 0)[..., None], sl / sw[..., None], 0.0)
    return sl.astype(np.float32), sw.astype(np.float32), cnt.astype(np.uint8), hb.astype(np.float32), bw.astype(np.float32)
