"""The stabilisation rule (include/topo4d_raster.h: t4d_drift_dense, t4d_drift_warp) and topo4d_amd.drift.correct_vertices,
restated in numpy.  Written apart from the kernels' structure: the dense flow is, per label, two integer matrix products of the
separable weights with the node values over the whole image, the warp is four whole-image gathers, and the vertex means are a plain
loop over the UV vertices.  dense_flow and warp are integer arithmetic and correct_vertices is float64 in the module's order, so the
device results must equal these bit for bit."""
from __future__ import annotations

import numpy as np


def node_values(d: np.ndarray, level: int) -> np.ndarray:
    """int64 [nby,nbx,2]: q = rint(d 2^level 256)"""
    return np.rint(np.asarray(d, np.float64) * float((1 << level) * 256)).astype(np.int64)


def dense_sums(d, kept, labels, B: int, S: int, L: int, reach: int = 1):
    """(num int64 [H,W,2], den int64 [H,W]): the sums of w q and of w of t4d_drift_dense's rule, 0 where no node takes part"""
    labels = np.asarray(labels)
    H, W = labels.shape
    kept = np.asarray(kept) != 0
    nby, nbx = kept.shape
    if nby == 0 or nbx == 0:
        return np.zeros((H, W, 2), np.int64), np.zeros((H, W), np.int64)
    q = node_values(d, L)
    cy, cx = np.arange(nby) * S + B // 2, np.arange(nbx) * S + B // 2
    ny, nx = (cy << (L + 1)) - 1, (cx << (L + 1)) - 1
    node_label = labels[np.ix_(cy << L, cx << L)].astype(np.int64)
    part = np.where(kept & (node_label != 0), node_label, 0)
    T = reach * 2 * S * (1 << L)
    wy = np.maximum(0, T - np.abs(2 * np.arange(H, dtype=np.int64)[:, None] - ny[None, :]))        # [H,nby]
    wx = np.maximum(0, T - np.abs(2 * np.arange(W, dtype=np.int64)[:, None] - nx[None, :]))        # [W,nbx]
    num, den = np.zeros((H, W, 2), np.int64), np.zeros((H, W), np.int64)
    for l in np.unique(part):
        if l == 0:
            continue
        m = (part == l).astype(np.int64)
        here = labels == l
        den[here] = (wy @ m @ wx.T)[here]
        for k in range(2):
            num[..., k][here] = (wy @ (m * q[..., k]) @ wx.T)[here]
    return num, den


def dense_flow(d, kept, labels, B: int, S: int, L: int, reach: int = 1):
    """(flow int32 [H,W,2], support uint8 [H,W]) of t4d_drift_dense"""
    num, den = dense_sums(d, kept, labels, B, S, L, reach)
    flow, support = np.zeros(num.shape, np.int32), np.zeros(den.shape, np.uint8)
    has = den > 0
    safe = np.where(has, den, 1)
    for k in range(2):
        flow[..., k] = np.where(has, (2 * num[..., k] + den) // (2 * safe), 0)
    support[has] = 1
    return flow, support


def warp(image, valid, labels, flow):
    """(image uint8 of the given shape, valid uint8 [H,W]) of t4d_drift_warp"""
    image, labels = np.asarray(image, np.uint8), np.asarray(labels)
    H, W = labels.shape
    img = image.reshape(H, W, -1).astype(np.int64)
    ok_b = np.asarray(valid) != 0
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    Y, X = 256 * y + flow[..., 0].astype(np.int64), 256 * x + flow[..., 1].astype(np.int64)
    y0, x0, ty, tx = Y >> 8, X >> 8, Y & 255, X & 255
    total, s = np.zeros((H, W), np.int64), np.zeros(img.shape, np.int64)
    for a, wa in ((0, 256 - ty), (1, ty)):
        for b, wb in ((0, 256 - tx), (1, tx)):
            yy, xx = y0 + a, x0 + b
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            yc, xc = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
            adm = inside & ok_b[yc, xc] & (labels[yc, xc] == labels) & (labels != 0)
            w = np.where(adm, wa * wb, 0)
            total += w
            s += w[..., None] * img[yc, xc]
    has = total > 0
    safe = np.where(has, total, 1)[..., None]
    out = np.where(has[..., None], (2 * s + total[..., None]) // (2 * safe), 0).astype(np.uint8)
    return out.reshape(image.shape), has.astype(np.uint8)


def sample_positions(pos, labels, py, px, label):
    """(values float64 [n,3], ok bool [n]) by topo4d_amd.drift.sample_positions' rule, in its order of operations"""
    H, W = labels.shape
    y0, x0 = np.floor(py), np.floor(px)
    ty, tx = py - y0, px - x0
    y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
    weights, values = [], []
    for a, wy in ((0, 1.0 - ty), (1, ty)):
        for b, wx in ((0, 1.0 - tx), (1, tx)):
            yy, xx = y0 + a, x0 + b
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            yc, xc = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
            ok = inside & (labels[yc, xc] == label) & (label != 0)
            weights.append(np.where(ok, wy * wx, 0.0))
            values.append(pos[yc, xc].astype(np.float64))
    total = ((weights[0] + weights[1]) + weights[2]) + weights[3]
    s = ((weights[0][:, None] * values[0] + weights[1][:, None] * values[1]) + weights[2][:, None] * values[2]) + weights[3][:, None] * values[3]
    ok = total > 0.0
    return np.where(ok[:, None], s / np.where(ok, total, 1.0)[:, None], 0.0), ok


def correct_vertices(uv_texels, owner, vertices, pos, flow, support, labels):
    """(vertices float64 [N,3], moved bool [N]) by topo4d_amd.drift.correct_vertices' rule.  uv_texels [n_uv,>=2]: texture.process_uv
    of the UVs at the size of labels ((x, y) per row); owner int [n_uv]: projtex.uv_vertex_owner (-1: none); pos: the position map
    of the mesh at that size (the device's projtex.surface_maps)."""
    H, W = labels.shape
    vertices = np.asarray(vertices, np.float64)
    px, py = np.asarray(uv_texels, np.float64)[:, 0], np.asarray(uv_texels, np.float64)[:, 1]
    ry, rx = np.rint(py).astype(np.int64), np.rint(px).astype(np.int64)
    inside = (ry >= 0) & (ry < H) & (rx >= 0) & (rx < W)
    ryc, rxc = np.clip(ry, 0, H - 1), np.clip(rx, 0, W - 1)
    f = flow[ryc, rxc].astype(np.float64)
    value, ok = sample_positions(pos, labels, py + f[:, 0] / 256.0, px + f[:, 1] / 256.0, labels[ryc, rxc])
    ok = ok & inside & (support[ryc, rxc] != 0)
    total, count = np.zeros_like(vertices), np.zeros(len(vertices), np.float64)
    for k in range(len(px)):                                    # ascending UV index
        if owner[k] >= 0 and ok[k]:
            total[owner[k]] = total[owner[k]] + value[k]
            count[owner[k]] += 1.0
    moved = count > 0.0
    out = vertices.copy()
    out[moved] = total[moved] / count[moved][:, None]
    return out, moved


def resample_periodic(f: np.ndarray, uy: np.ndarray, ux: np.ndarray) -> np.ndarray:
    """g(p) = f(p - u(p)) on the periodic image by bilinear resampling: to first order a feature of f at p lies at p + u in g"""
    h, w = f.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    sy, sx = y - uy, x - ux
    y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    fy, fx = sy - y0, sx - x0
    at = lambda yy, xx: f[yy % h, xx % w]
    return (at(y0, x0) * (1 - fy) * (1 - fx) + at(y0, x0 + 1) * (1 - fy) * fx + at(y0 + 1, x0) * fy * (1 - fx) + at(y0 + 1, x0 + 1) * fy * fx)
