"""
Yardsticks of the registration of topo4d_amd.projtex (t4d_project_texture_flow / t4d_project_texture_bands_flow in
csrc/t4d_projtex.hip, projtex.view_flows, project_frame(register=...)), on the host:

    pixels(pos, view, H, W)                                    step 1 of the projection rule: (px, py) of every texel
    view_samples(..., flow=)                                   rule F.1..F.5 for one view: (accepted, cos, w, s)
    project_texture(..., skip=, skip_base=, flows=)            the whole t4d_project_texture_flow: (color, weight, count)
    project_bands(..., skip=, skip_base=, flows=)              the whole t4d_project_texture_bands_flow
    flow_report(d, kept)                                       one view's entry of view_flows' report
    view_flows(renders, photos, depth, ...)                    projtex.view_flows over drift_ref and stabilise_ref
    merge_frame(parts, mode)                                   project_frame's merge of the size groups, in float32 as it runs
    register_frame(...)                                        project_frame(register=...): the whole chain

Geometry decides visibility and weight, the flow only moves the colour sample: steps 1..5 are tests/projtex_ref.view_samples' as
they stand (wrapped, not restated), and what is restated here is the projection of step 1, the flow look-up and the bilinear mix
at the moved position, in the kernel's order of float64 operations (numpy never fuses a multiply-add), so every output bit agrees.
"""
from __future__ import annotations

import math

import numpy as np

from tests import drift_ref, meshrender_ref, projtex_bands_ref, projtex_ref, stabilise_ref, texfill_ref, texfinish_ref
from tests.projtex_consist_ref import _masked


def pixels(pos, view, H: int, W: int):
    """(px, py) float64 [h,w] of step 1, as projtex_ref.view_samples forms them"""
    pos = np.asarray(pos)
    pos = pos if pos.dtype == np.float64 else pos.astype(np.float32).astype(np.float64)
    X, Y, Z = pos[..., 0], pos[..., 1], pos[..., 2]
    pm = projtex_ref._mat(np.asarray(view, dtype=np.float32).reshape(-1), 16)
    with np.errstate(all="ignore"):
        cx = ((pm(0, 0) * X + pm(0, 1) * Y) + pm(0, 2) * Z) + pm(0, 3)
        cy = ((pm(1, 0) * X + pm(1, 1) * Y) + pm(1, 2) * Z) + pm(1, 3)
        cw = ((pm(3, 0) * X + pm(3, 1) * Y) + pm(3, 2) * Z) + pm(3, 3)
        px = ((cx / cw + 1.0) * float(W) - 1.0) * 0.5
        py = ((cy / cw + 1.0) * float(H) - 1.0) * 0.5
    return px, py


def view_samples(pos, nrm, coverage, view, H: int, W: int, photo, depth, power: int = 2, cos_min: float = 0.1, fade_px: float = 16.0,
                 depth_tol: float = 0.002, gain=None, flow=None):
    """projtex_ref.view_samples with flow int16 [H,W,2] = (f_y, f_x) in 1/256 px (None: exactly projtex_ref's)"""
    ok, cs, w, s = projtex_ref.view_samples(pos, nrm, coverage, view, H, W, photo, depth, power, cos_min, fade_px, depth_tol, gain)
    if flow is None:
        return ok, cs, w, s
    flow = np.asarray(flow)
    assert flow.dtype == np.int16 and flow.shape == (H, W, 2)
    photo = np.asarray(photo, dtype=np.float32).reshape(3, H, W)
    px, py = pixels(pos, view, H, W)
    with np.errstate(all="ignore"):
        ix = np.clip(np.where(ok, np.floor(px + 0.5), 0.0), 0, W - 1).astype(np.int64)       # F.2 (only read where ok)
        iy = np.clip(np.where(ok, np.floor(py + 0.5), 0.0), 0, H - 1).astype(np.int64)
        qx = px + flow[iy, ix, 1].astype(np.float64) / 256.0                                  # F.3
        qy = py + flow[iy, ix, 0].astype(np.float64) / 256.0
        fx0, fy0 = np.floor(qx), np.floor(qy)
        ok = ok & (fx0 >= 0.0) & (fx0 + 1.0 <= float(W - 1)) & (fy0 >= 0.0) & (fy0 + 1.0 <= float(H - 1))      # F.4
        x0, y0 = np.where(ok, fx0, 0.0).astype(np.int64), np.where(ok, fy0, 0.0).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        fx, fy = qx - fx0, qy - fy0
        gx, gy = 1.0 - fx, 1.0 - fy
        s = np.empty(ok.shape + (3,))
        for ch in range(3):                                                                   # F.5
            q = photo[ch].astype(np.float64)
            a = gx * q[y0, x0] + fx * q[y0, x1]
            b = gx * q[y1, x0] + fx * q[y1, x1]
            s[..., ch] = gy * a + fy * b
            if gain is not None:
                s[..., ch] = s[..., ch] * float(gain[ch])
    return ok, cs, w, s


def project_texture(pos, nrm, coverage, views, H: int, W: int, photos, depth, power: int = 2, cos_min: float = 0.1,
                    fade_px: float = 16.0, depth_tol: float = 0.002, mode: str = "weighted", gains=None, skip=None, skip_base: int = 0,
                    flows=None):
    """(color [h,w,3] float32, weight [h,w] float32, count [h,w] uint8) of t4d_project_texture_flow; flows int16 [V,H,W,2] or None"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    photos, depth = np.asarray(photos, np.float32), np.asarray(depth, np.float32)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    th, tw = np.asarray(pos).shape[:2]
    best = {"weighted": False, "best": True}[mode]
    sw, sc, cnt = np.zeros((th, tw)), np.zeros((th, tw, 3)), np.zeros((th, tw), dtype=np.int64)
    with np.errstate(all="ignore"):
        for v in range(len(views)):
            ok, _, w, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depth[v], power, cos_min, fade_px, depth_tol,
                                       None if gains is None else gains[v], None if flows is None else flows[v])
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
                  fade_px: float = 16.0, depth_tol: float = 0.002, gains=None, skip=None, skip_base: int = 0, flows=None):
    """(low_color, weight, count, high, best_weight) of t4d_project_texture_bands_flow"""
    views = np.asarray(views, dtype=np.float32).reshape(-1, 40)
    photos, low, depth = np.asarray(photos, np.float32), np.asarray(low, np.float32), np.asarray(depth, np.float32)
    gains = None if gains is None else np.asarray(gains, np.float64).reshape(len(views), 3)
    th, tw = np.asarray(pos).shape[:2]
    sw, bw, cnt = np.zeros((th, tw)), np.zeros((th, tw)), np.zeros((th, tw), dtype=np.int64)
    sl, hb = np.zeros((th, tw, 3)), np.zeros((th, tw, 3))
    with np.errstate(all="ignore"):
        for v in range(len(views)):
            g, f = None if gains is None else gains[v], None if flows is None else flows[v]
            ok, _, w, s = view_samples(pos, nrm, coverage, views[v], H, W, photos[v], depth[v], power, cos_min, fade_px, depth_tol, g, f)
            ok_l, _, _, l = view_samples(pos, nrm, coverage, views[v], H, W, low[v], depth[v], power, cos_min, fade_px, depth_tol, g, f)
            assert np.array_equal(ok, ok_l)
            ok = ok & ~_masked(skip, skip_base, v, (th, tw))
            cnt += ok
            sw = np.where(ok, sw + w, sw)
            sl = np.where(ok[..., None], sl + w[..., None] * l, sl)
            take = ok & (w > bw)
            bw = np.where(take, w, bw)
            hb = np.where(take[..., None], s - l, hb)
        sl = np.where((cnt > 0)[..., None], sl / sw[..., None], 0.0)
    return sl.astype(np.float32), sw.astype(np.float32), cnt.astype(np.uint8), hb.astype(np.float32), bw.astype(np.float32)


# ---- the flows ---------------------------------------------------------------------------------------------------------------
def flow_report(d, kept) -> dict:
    """blocks, kept and, over the kept blocks, mean (exactly rounded sum / n), lower median, p90 (rank ceil(0.9 n)) and max of |d|"""
    d, kept = np.asarray(d, np.float64).reshape(-1, 2), np.asarray(kept).reshape(-1) != 0
    n = int(kept.sum())
    out = {"blocks": int(kept.size), "kept": n}
    if n == 0:
        return out
    length = sorted(np.sqrt(d[kept, 0] * d[kept, 0] + d[kept, 1] * d[kept, 1]).tolist())
    out["mean"], out["median"] = math.fsum(length) / n, length[(n - 1) // 2]
    out["p90"], out["max"] = length[min(n - 1, (9 * n + 9) // 10 - 1)], length[-1]
    return out


def view_flow(render, photo, depth, block: int = 32, stride=None, radius: int = 4, ratio: float = 0.8, reach: int = 1):
    """(flow int16 [H,W,2], support uint8 [H,W], d, kept) of one view: render / photo [3,H,W] float32, depth [1,H,W]"""
    stride = block // 2 if stride is None else stride
    a = texfinish_ref.quantize(np.moveaxis(np.asarray(render, np.float32), 0, -1))
    b = texfinish_ref.quantize(np.moveaxis(np.asarray(photo, np.float32), 0, -1))
    valid = ((np.asarray(depth, np.float32).reshape(a.shape[:2]) > 0) & (a != 0).any(-1)).astype(np.uint8)
    table = drift_ref.match(a, valid, b, valid, valid, block, stride, radius, block * block // 2)
    d, kept = drift_ref.flow(table, radius, ratio)
    f, support = stabilise_ref.dense_flow(d, kept, valid, block, stride, 0, reach)
    assert np.abs(f).max(initial=0) <= (radius + 0.5) * 256
    return f.astype(np.int16), support, d, kept


def view_flows(renders, photos, depth, **options):
    """(flows int16 [V,H,W,2], support uint8 [V,H,W], report) of projtex.view_flows"""
    found = [view_flow(r, p, d, **options) for r, p, d in zip(renders, photos, depth)]
    return np.stack([f[0] for f in found]), np.stack([f[1] for f in found]), [flow_report(f[2], f[3]) for f in found]


# ---- the frame -----------------------------------------------------------------------------------------------------------------
def merge_frame(parts, mode: str):
    """(color float32 [h,w,3] clamped as project_frame clamps it, weight, count) of the size groups' results, merged in float32 in
    project_frame's order: parts holds project_texture's triples, or for "twoband" project_bands' five results"""
    f32, tiny = np.float32, np.finfo(np.float32).tiny
    total = detail = count = None
    for part in parts:
        color, weight, n = part[:3]
        if mode == "twoband":
            high, best = part[3], part[4]
            if detail is None:
                detail = (high, best)
            else:
                take = best > detail[1]
                detail = (np.where(take[..., None], high, detail[0]), np.where(take, best, detail[1]))
        if total is None:
            total, count = (color, weight), n
        elif mode == "best":
            take = weight > total[1]
            total, count = (np.where(take[..., None], color, total[0]), np.where(take, weight, total[1])), count + n
        else:
            ws = (total[1] + weight).astype(f32)
            mixed = ((total[0] * total[1][..., None]).astype(f32) + (color * weight[..., None]).astype(f32)).astype(f32) \
                / np.maximum(ws, tiny)[..., None]
            total, count = (np.where((ws > 0)[..., None], mixed.astype(f32), f32(0)), ws), count + n
    color, weight = total
    if detail is not None:
        color = np.clip((color + detail[0]).astype(f32), f32(0), f32(1))
    return color.astype(f32), weight, count.astype(np.uint8)


def register_frame(pos, nrm, coverage, labels, groups, mesh, mode: str, rule: dict, register: dict, gains=None, skip=None, band_radius: int = 8):
    """(texture uint8 [h,w,3], weight, count, flows per group, support per group, report per view in group order) of
    project_frame(register=...).  groups: (views [v,40], H, W, photos, depth) per image size, in project_frame's order; mesh:
    (vertices, tris, uv_tris, uvs) of meshrender_ref.render; gains [V,3] and skip in group order; register: view_flows' options
    and rounds."""
    vertices, tris, uv_tris, uvs = mesh
    options = {k: v for k, v in register.items() if k != "rounds"}

    def blend(mode, flows):
        parts, base = [], 0
        for i, (views, H, W, photos, depth) in enumerate(groups):
            kw = dict(gains=None if gains is None else gains[base:base + len(views)], skip=skip, skip_base=base,
                      flows=None if flows is None else flows[i], **rule)
            base += len(views)
            if mode == "twoband":
                low = projtex_bands_ref.low_band(photos, depth, band_radius)
                parts.append(project_bands(pos, nrm, coverage, views, H, W, photos, low, depth, **kw))
            else:
                parts.append(project_texture(pos, nrm, coverage, views, H, W, photos, depth, mode=mode, **kw))
        color, weight, count = merge_frame(parts, mode)
        return texfinish_ref.quantize(color), weight, count

    flows = None
    for _ in range(register.get("rounds", 1)):
        tex, _, n = blend("weighted", flows)
        tex, _ = texfill_ref.fill_islands(tex, n > 0, labels)
        found = []
        for views, H, W, photos, depth in groups:
            renders = np.stack([meshrender_ref.render(vertices, tris, uv_tris, uvs, tex, v, H, W)[0] for v in views])
            found.append(view_flows(renders, photos, depth, **options))
        flows = [f[0] for f in found]
    return (*blend(mode, flows), flows, [f[1] for f in found], [r for f in found for r in f[2]])
