#!/usr/bin/env python
"""CPU model (no GPU needed): what the separable moment reduction of k_render_bwd costs in rounding.

    python tools/experiments/model_bwd_moment_numerics.py [--views 0,9]

The backward render sums, per (Gaussian, tile) pair, e = G dL/dalpha and its first and second moments about the splat centre
over the tile's pixels.  The kernel accumulates RAW moments about a fixed origin (pixel = origin + (X, Y)) and shifts them to the
splat centre once per pair and wave (t4d_raster_render_bwd.h: reduce_moments_row, moments_about_centre); the shift cancels.
This script restates three orders of operations in float32 on the SAME float32 e of every (pixel, listed splat) - taken from the C
oracle's lists, centres, conics and last contributors, the recursion itself evaluated in float64 - and compares the five
shifted sums of every pair with their float64 values:

  centred      products e d, e d d^T per pixel, then summed                      (the order before the moment reduction)
  tile origin  raw moments (of e truncated to 18 bits, as built) about the centre of the 16x16 tile, ONE shift per pair
  wave origin  raw moments about the centre of each wave's 8x8 block, a shift per wave, then the four waves summed   (as built)

on the config-2 scene and on a scene of the smallest splats the 0.3 px^2 dilation allows (scales -> 0: the cut-off radius is at
its floor, so |centre - origin| / radius - what the cancellation grows with - is at its largest).
Errors are given relative to the largest entry of each sum over all pairs of the view (the way the tests bound a gradient tensor:
GRAD_REL = 2e-4 of the tensor's largest entry) and, as `worst_entry`, relative to the entry itself for entries above 1e-3 of the
largest.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from model_bwd_decompositions import tile_tables  # noqa: E402

NAMES = ("e_dx", "e_dy", "e_dxdx", "e_dxdy", "e_dydy")


def shifted(M, px, py):
    """moments_about_centre: M = [M00, M10, M01, M20, M11, M02] (float32 arrays), p = centre - origin (float32); evaluated in float64
    (numpy has no fused multiply-add: the products below are exact or within 1e-16 of it) and rounded to float32 once."""
    M00, M10, M01, M20, M11, M02 = (m.astype(np.float64) for m in M)
    px, py = px.astype(np.float64), py.astype(np.float64)
    sx, sy = px * M00 - M10, py * M00 - M01
    return np.stack([sx, sy, px * sx - (px * M10 - M20), px * sy - (py * M10 - M11), py * sy - (py * M01 - M02)]).astype(np.float32)


def moment_e(e):
    """e as the moments take it: 18 significant bits, truncated (its products with X^a Y^b are then exact)."""
    return (e.view(np.uint32) & np.uint32(0xffffffc0)).view(np.float32)


def tile_sums(tt, rgb, dLdC):
    """The five sums of every pair of one tile: float64 truth and the three float32 orders.  Each [5, n]."""
    ids, xy, co, contrib, last, (tx, ty) = tt
    n = len(ids)
    tid = np.arange(256)
    w, r, i = tid >> 6, (tid >> 4) & 3, tid & 15
    lx = ((w & 1) << 3) + ((r & 1) << 2) + (i & 3)
    ly = ((w >> 1) << 3) + ((r >> 1) << 2) + (i >> 2)
    px, py = tx * 16 + lx, ty * 16 + ly
    dx32 = xy[None, :, 0].astype(np.float32) - px[:, None].astype(np.float32)       # exact in float32
    dy32 = xy[None, :, 1].astype(np.float32) - py[:, None].astype(np.float32)
    dx, dy = dx32.astype(np.float64), dy32.astype(np.float64)
    c = co.astype(np.float64)
    G = np.exp(-0.5 * (c[None, :, 0] * dx * dx + c[None, :, 2] * dy * dy) - c[None, :, 1] * dx * dy)
    a = np.minimum(0.99, c[None, :, 3] * G) * contrib
    om = 1.0 - a
    T = np.cumprod(np.concatenate([np.ones((256, 1)), om[:, :-1]], 1), 1)            # transmittance in front of splat i
    q = dLdC @ rgb[ids].astype(np.float64).T                                         # [256, n]
    wq = a * T * q
    S = np.cumsum(wq[:, ::-1], 1)[:, ::-1] - wq                                      # colour behind splat i, dotted
    e = (G * (T * q - S / om) * contrib).astype(np.float32)
    e64 = e.astype(np.float64)
    truth = np.stack([(e64 * dx).sum(0), (e64 * dy).sum(0), (e64 * dx * dx).sum(0), (e64 * dx * dy).sum(0), (e64 * dy * dy).sum(0)])

    def sum_waves(v):                       # float32 sums: the 64 pixels of a wave, then the four waves
        return v.reshape(4, 64, n).sum(1, dtype=np.float32)

    ed_x, ed_y = e * dx32, e * dy32
    centred = np.stack([sum_waves(v).sum(0, dtype=np.float32) for v in (ed_x, ed_y, ed_x * dx32, ed_x * dy32, ed_y * dy32)])

    et = moment_e(e)

    def moments(X, Y):                      # X, Y: [256] float32 lane constants -> six [4 waves, n] raw moments, x first then y
        eX = et * X[:, None]
        return [sum_waves(v) for v in (et, eX, et * Y[:, None], eX * X[:, None], eX * Y[:, None], et * (Y * Y)[:, None])]

    f = np.float32
    Xt, Yt = lx.astype(f) - f(7.5), ly.astype(f) - f(7.5)
    Mt = [m.sum(0, dtype=f) for m in moments(Xt, Yt)]
    cx, cy = xy[:, 0].astype(f), xy[:, 1].astype(f)
    tile = shifted(Mt, cx - f(tx * 16 + 7.5), cy - f(ty * 16 + 7.5))
    Xw, Yw = (lx & 7).astype(f) - f(3.5), (ly & 7).astype(f) - f(3.5)
    Mw = moments(Xw, Yw)
    wave = np.zeros((5, n), f)
    for wv in range(4):
        wave = (wave + shifted([m[wv] for m in Mw], cx - f(tx * 16 + (wv & 1) * 8 + 3.5), cy - f(ty * 16 + (wv >> 1) * 8 + 3.5))).astype(f)
    return truth, centred, tile, wave


def view_errors(st, rgb, H, W, seed):
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rng = np.random.default_rng(seed)
    cols = [[], [], [], []]
    for t in range(gx * gy):
        tt = tile_tables(st, t, gx, H, W)
        if tt is None:
            continue
        dLdC = rng.standard_normal((256, 3)) / (3 * H * W)
        for k, v in enumerate(tile_sums(tt, rgb, dLdC)):
            cols[k].append(v.astype(np.float64))
    truth, *orders = [np.concatenate(c, 1) for c in cols]
    out = {}
    big = np.abs(truth).max(1)
    for name, o in zip(("centred", "tile_origin", "wave_origin"), orders):
        err = np.abs(o - truth)
        keep = np.abs(truth) > 1e-3 * big[:, None]
        out[name] = {"vs_largest": {n: float(err[k].max() / big[k]) for k, n in enumerate(NAMES)},
                     "worst_entry": {n: float((err[k][keep[k]] / np.abs(truth[k][keep[k]])).max()) for k, n in enumerate(NAMES)}}
    out["pairs"] = int(truth.shape[1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="0,9")
    a = ap.parse_args()
    from oracle import c_oracle
    from scaffold import reference_boundary as boundary, scene
    cfg = scene.CONFIGS["C2"]
    H, W = cfg["H"], cfg["W"]
    cams = scene.camera_rig(H, W, n_views=24)
    res = {}
    for label, opacity, tiny in (("config 2", "A", False), ("smallest splats", "B", True)):
        params = scene.make_gaussians(cfg["n_lat"], cfg["n_lon"], opacity=opacity, seed=0)
        if tiny:
            params["log_scales"] = params["log_scales"] * 0 - 14.0          # 2D covariance = the 0.3 px^2 dilation alone
        rv = {k: v.detach() for k, v in boundary.params2rendervar(params).items()}
        rgb = rv["colors_precomp"].numpy()
        for v in (int(x) for x in a.views.split(",")):
            r = c_oracle.OracleRender(cams[v], rv["means3D"], rv["opacities"], rv["scales"], rv["rotations"], rv["colors_precomp"])
            res[f"{label}, view {v}"] = view_errors(r.state(), rgb, H, W, seed=v)
    worst = {o: max(max(r[o]["vs_largest"].values()) for r in res.values()) for o in ("centred", "tile_origin", "wave_origin")}
    print(json.dumps({"views": res, "worst_vs_largest": worst, "bound": "GRAD_REL / 10 = 2e-5"}, indent=1))


if __name__ == "__main__":
    main()
