"""
Yardsticks of topo4d_amd.meshrender (csrc/t4d_meshrender.hip), in float64 on the host:

    project(vertices, view)                  pixel x, y and view z of every vertex through one packed view record
    raster_screen(sx, sy, sz, tris, H, W)    coverage, depth and winning triangle of screen-space triangles
    render(...)                              the whole t4d_mesh_render of one view: (color [3,H,W], depth [1,H,W], index [H,W])
    metrics_f64(render, target, cover, mask) the per-view metrics of t4d_image_metrics, in float64 torch

The numpy code performs the kernel's operations in the kernel's order (numpy never fuses a multiply-add), so every output bit
agrees; it walks the triangles one after another and keeps the lexicographic minimum of (float32 depth bits, index).
"""
from __future__ import annotations

import numpy as np
import torch

NEAR = 0.01


def _mat(view, lo):
    """element (row r, col c) of the column-major 4x4 at view[lo:lo+16], as float64"""
    m = np.asarray(view, dtype=np.float32).reshape(-1)[lo:lo + 16].astype(np.float64)
    return lambda r, c: m[c * 4 + r]


def project(vertices, view, H: int, W: int):
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    pm, vm = _mat(view, 16), _mat(view, 0)
    cx = pm(0, 0) * X + pm(0, 1) * Y + pm(0, 2) * Z + pm(0, 3)
    cy = pm(1, 0) * X + pm(1, 1) * Y + pm(1, 2) * Z + pm(1, 3)
    cw = pm(3, 0) * X + pm(3, 1) * Y + pm(3, 2) * Z + pm(3, 3)
    with np.errstate(all="ignore"):
        nx, ny = cx / cw, cy / cw
        px = ((nx + 1.0) * float(W) - 1.0) * 0.5
        py = ((ny + 1.0) * float(H) - 1.0) * 0.5
    vz = vm(2, 0) * X + vm(2, 1) * Y + vm(2, 2) * Z + vm(2, 3)
    return px, py, vz


def edge_fn(ax, ay, bx, by, px, py):
    """edge function of segment a-b at p, from the lexicographically smaller end point (scalars a, b; arrays p)"""
    if ax < bx or (ax == bx and ay < by):
        return (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    return -((ax - bx) * (py - by) - (ay - by) * (px - bx))


def _owns(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return dy < 0 or (dy == 0 and dx > 0)


def setup(x, y, z, H: int, W: int):
    """(A, box, owns) of one triangle's screen corners, or None when it is dropped"""
    if not (z[0] > NEAR and z[1] > NEAR and z[2] > NEAR):
        return None
    A = edge_fn(x[0], y[0], x[1], y[1], x[2], y[2])
    if not (A > 0 or A < 0):
        return None
    with np.errstate(all="ignore"):
        lo_x, hi_x = np.ceil(min(x[0], min(x[1], x[2]))), np.floor(max(x[0], max(x[1], x[2])))
        lo_y, hi_y = np.ceil(min(y[0], min(y[1], y[2]))), np.floor(max(y[0], max(y[1], y[2])))
    if not all(np.isfinite([lo_x, hi_x, lo_y, hi_y])):
        return None
    cx0, cx1, cy0, cy1 = max(lo_x, 0.0), min(hi_x, float(W - 1)), max(lo_y, 0.0), min(hi_y, float(H - 1))
    if cx0 > cx1 or cy0 > cy1:
        return None
    pos = A > 0
    e = [(1, 2), (2, 0), (0, 1)]
    owns = [_owns(x[a], y[a], x[b], y[b]) if pos else _owns(x[b], y[b], x[a], y[a]) for a, b in e]
    return A, (int(cx0), int(cx1), int(cy0), int(cy1)), owns


def eval_pixels(x, y, z, A, owns, px, py):
    """(inside mask, q0, q1, q2, S) at pixel arrays px, py"""
    pos = A > 0
    es = [edge_fn(x[1], y[1], x[2], y[2], px, py), edge_fn(x[2], y[2], x[0], y[0], px, py),
          edge_fn(x[0], y[0], x[1], y[1], px, py)]
    if not pos:
        es = [-e for e in es]
    inside = np.ones(px.shape, dtype=bool)
    for e, o in zip(es, owns):
        inside &= (e > 0) | ((e == 0) & o)
    aA = abs(A)
    with np.errstate(all="ignore"):
        q = [(es[i] / aA) / z[i] for i in range(3)]
        S = q[0] + q[1] + q[2]
    return inside & (S > 0), q, S


def raster_screen(sx, sy, sz, tris, H: int, W: int):
    """keys [H,W] uint64 (all ones: nothing) and the per-pixel (q0, q1, q2, S) of the winner, for corners already on screen"""
    key = np.full((H, W), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    for f, (i0, i1, i2) in enumerate(np.asarray(tris, dtype=np.int64)):
        x, y, z = sx[[i0, i1, i2]], sy[[i0, i1, i2]], sz[[i0, i1, i2]]
        s = setup(x, y, z, H, W)
        if s is None:
            continue
        A, (x0, x1, y0, y1), owns = s
        gy, gx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        inside, q, S = eval_pixels(x, y, z, A, owns, gx.astype(np.float64), gy.astype(np.float64))
        if not inside.any():
            continue
        with np.errstate(all="ignore"):
            d = (1.0 / S).astype(np.float32)
        k = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        sub = key[y0:y1 + 1, x0:x1 + 1]
        key[y0:y1 + 1, x0:x1 + 1] = np.where(inside & (k < sub), k, sub)
    return key


def _texel(tex, iy, ix, c):
    t = tex[iy, ix, c]
    return t.astype(np.float64) / 255.0 if tex.dtype == np.uint8 else t.astype(np.float64)


def shade(beta, uv_corners, tex, mapping="bilinear"):
    """colour [n,3] float64 from the perspective weights beta (3 arrays) and the corner uvs [n,3,2] (float32 values)"""
    uvc = uv_corners.astype(np.float64)
    u = beta[0] * uvc[:, 0, 0] + beta[1] * uvc[:, 1, 0] + beta[2] * uvc[:, 2, 0]
    v = beta[0] * uvc[:, 0, 1] + beta[1] * uvc[:, 1, 1] + beta[2] * uvc[:, 2, 1]
    th, tw = tex.shape[:2]
    wm, hm = float(tw - 1), float(th - 1)
    tx = u * wm
    ty = (float(th) - v * hm) - 1.0
    tx = np.where(tx > 0, tx, 0.0)
    tx = np.where(tx > wm, wm, tx)
    ty = np.where(ty > 0, ty, 0.0)
    ty = np.where(ty > hm, hm, ty)
    out = np.empty((u.shape[0], 3), dtype=np.float64)
    if mapping == "nearest":
        ix, iy = np.rint(tx).astype(np.int64), np.rint(ty).astype(np.int64)
        for c in range(3):
            out[:, c] = _texel(tex, iy, ix, c)
        return out
    fx0, fy0 = np.floor(tx), np.floor(ty)
    fx, fy = tx - fx0, ty - fy0
    ix0, iy0 = fx0.astype(np.int64), fy0.astype(np.int64)
    ix1, iy1 = np.minimum(ix0 + 1, tw - 1), np.minimum(iy0 + 1, th - 1)
    for c in range(3):
        t00, t01, t10, t11 = _texel(tex, iy0, ix0, c), _texel(tex, iy0, ix1, c), _texel(tex, iy1, ix0, c), _texel(tex, iy1, ix1, c)
        out[:, c] = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t01) + fy * ((1.0 - fx) * t10 + fx * t11)
    return out


def render(vertices, tris, uv_tris, uvs, tex, view, H: int, W: int, bg=(0.0, 0.0, 0.0), mapping="bilinear"):
    """t4d_mesh_render of one view: (color [3,H,W] float32, depth [1,H,W] float32, index [H,W] int32)"""
    tris = np.asarray(tris, dtype=np.int64)
    uv_tris = np.asarray(uv_tris, dtype=np.int64)
    uvs = np.asarray(uvs, dtype=np.float32)
    tex = np.asarray(tex)
    sx, sy, sz = project(vertices, view, H, W)
    key = raster_screen(sx, sy, sz, tris, H, W)
    hit = key != np.uint64(0xFFFFFFFFFFFFFFFF)
    color = np.empty((3, H, W), dtype=np.float32)
    for c in range(3):
        color[c] = np.float32(bg[c])
    depth = np.zeros((1, H, W), dtype=np.float32)
    index = np.full((H, W), -1, dtype=np.int32)
    ys, xs = np.nonzero(hit)
    if ys.size == 0:
        return color, depth, index
    f = (key[ys, xs] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    index[ys, xs] = f
    q = [np.empty(ys.size) for _ in range(3)]
    S = np.empty(ys.size)
    for face in np.unique(f):
        sel = f == face
        i = tris[face]
        x, y, z = sx[i], sy[i], sz[i]
        A, _, owns = setup(x, y, z, H, W)
        inside, qq, ss = eval_pixels(x, y, z, A, owns, xs[sel].astype(np.float64), ys[sel].astype(np.float64))
        assert inside.all()
        for k in range(3):
            q[k][sel] = qq[k]
        S[sel] = ss
    depth[0, ys, xs] = (1.0 / S).astype(np.float32)
    beta = [q[k] / S for k in range(3)]
    col = shade(beta, uvs[uv_tris[f]], tex, mapping)
    color[:, ys, xs] = col.T.astype(np.float32)
    return color, depth, index


# ---- metrics: the float64 torch restatement of t4d_image_metrics -----------------------------------------------------------
def _window64():
    g = torch.tensor([np.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float64)
    g = g / g.sum()
    return (g[:, None] @ g[None, :])[None, None].expand(3, 1, 11, 11).contiguous()


def ssim_map64(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """external._ssim's map of [V,3,H,W] images in float64 (no mean)"""
    F = torch.nn.functional
    a, b = a.double(), b.double()
    w = _window64().to(a.device)
    conv = lambda x: F.conv2d(x, w, padding=5, groups=3)
    mu1, mu2 = conv(a), conv(b)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1_sq, conv(b * b) - mu2_sq, conv(a * b) - mu1_mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))


def metrics_f64(render: torch.Tensor, target: torch.Tensor, coverage=None, mask=None) -> torch.Tensor:
    """[V, 6] float64: psnr_full, count, l1, mse, psnr, ssim (include/topo4d_raster.h t4d_image_metrics)"""
    r, t = render.double(), target.double()
    V, _, H, W = r.shape
    d = r - t
    mse_c = (d * d).reshape(V, 3, -1).mean(-1)
    psnr_full = (20 * torch.log10(1.0 / torch.sqrt(mse_c))).mean(-1)
    sel = torch.ones(V, H, W, dtype=torch.bool, device=r.device)
    if coverage is not None:
        sel &= coverage >= 0
    if mask is not None:
        sel &= mask[:, 0] > 0.5
    sel3 = sel[:, None].expand(V, 3, H, W)
    cnt = sel.reshape(V, -1).sum(-1).double()
    n = 3 * cnt
    l1 = (d.abs() * sel3).reshape(V, -1).sum(-1) / n
    mse = (d * d * sel3).reshape(V, -1).sum(-1) / n
    psnr = 20 * torch.log10(1.0 / torch.sqrt(mse))
    ssim = (ssim_map64(r, t) * sel3).reshape(V, -1).sum(-1) / n
    return torch.stack([psnr_full, cnt, l1, mse, psnr, ssim], dim=1)
