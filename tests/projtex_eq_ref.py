"""
Yardsticks of the camera equalisation of topo4d_amd.projtex (k_pair_stats and the gains of k_projtex in csrc/t4d_projtex.hip), in
float64 on the host:

    project_texture_gains(..., gains)                                 tests/projtex_ref.project_texture under its earlier name
    pair_stats(pos, nrm, coverage, views, sizes, photos, depths, ...) the whole t4d_projtex_pair_stats: (count [V,V], sums [V,V,3])
    pair_stats_slow(...)                                              the same, texel by texel: a check of pair_stats on a tiny case

Steps 1..6 are tests/projtex_ref.view_samples, which performs the kernel's operations in the kernel's order, so every output bit
agrees.  The participation rule and the pair sums are a plain double loop over the views.
"""
from __future__ import annotations

import numpy as np

from tests.projtex_ref import project_texture as project_texture_gains, view_samples  # noqa: F401 (the gains are an argument there)

SCALE = 65536.0


def taking_part(pos, nrm, coverage, views, sizes, photos, depths, power=2, cos_min=0.1, fade_px=16.0, depth_tol=0.002,
                stat_cos_min=0.5, stat_lo=0.02, stat_hi=0.98, gains=None):
    """(part bool [V,h,w], q int64 [V,h,w,3]): where each view takes part, and its integer sample there (0 elsewhere).  sizes
    [V] of (h, w); photos [V] of [3,h_v,w_v]; depths [V] of [h_v,w_v] (or [1,h_v,w_v])"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    part, q = [], []
    for v in range(len(views)):
        H, W = (int(x) for x in sizes[v])
        ok, cs, _, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depths[v], power, cos_min, fade_px, depth_tol,
                                    None if gains is None else gains[v])
        with np.errstate(all="ignore"):
            p = ok & (cs >= float(stat_cos_min)) & ((s >= float(stat_lo)) & (s <= float(stat_hi))).all(-1)
            qi = np.rint(np.where(p[..., None], s, 0.0) * SCALE).astype(np.int64)          # half to even, as llrint
        part.append(p)
        q.append(qi)
    return np.stack(part), np.stack(q)


def pair_stats(*args, **kw):
    """(count int64 [V,V], sums int64 [V,V,3]): over the texels where views i and j both take part, their number and the sum of
    view i's integer samples"""
    part, q = taking_part(*args, **kw)
    V = len(part)
    count, sums = np.zeros((V, V), np.int64), np.zeros((V, V, 3), np.int64)
    for i in range(V):
        for j in range(V):
            both = part[i] & part[j]
            count[i, j] = both.sum()
            sums[i, j] = q[i][both].sum(0)
    return count, sums


def pair_stats_slow(*args, **kw):
    """pair_stats texel by texel, as the rule is written down: for a tiny case only"""
    part, q = taking_part(*args, **kw)
    V, th, tw = part.shape
    count, sums = np.zeros((V, V), np.int64), np.zeros((V, V, 3), np.int64)
    for y in range(th):
        for x in range(tw):
            there = [v for v in range(V) if part[v, y, x]]
            for i in there:
                for j in there:
                    count[i, j] += 1
                    for c in range(3):
                        sums[i, j, c] += int(q[i, y, x, c])
    return count, sums
