"""The misregistered scene of the registration tests and its two measures, restated from tests/test_projtex_bands_host.py (whose
fixture is not imported): the patch of tests/projtex_scenes.py at 128 x 128 texels under three 192 x 160 views of focal lengths
210 / 200 / 200; views 1 and 2 are photographed aiming at (0.02, 0, 0) and (0, 0.02, 0) but projected with cameras aiming at the
origin, about 1.3 px off.  The texture is smooth_texture + 0.12 x 5x5-box-filtered unit Gaussian noise.

"Detail energy", with E(T) the sum of (T_a - T_b)^2 over the pairs a, b of compared texels that are horizontal or vertical
neighbours and over the three channels: E(result - smooth_texture) / E(detail), what is left of the texel-to-texel variation.
"Largest neighbour step", on smooth_texture under exposures 1.0 / 0.85 / 1.15 without gains: the largest |difference| of two
compared texels that are horizontal or vertical neighbours, over the channels.  Compared are the texels all three views see, six
texels inside the island.

misregistered(scale) multiplies the image sides and the focal lengths by `scale`: the same cameras at a finer sampling, so the
same aiming error is about 1.3 scale px.  scale 1 is the scene as it was; the registration is measured at SCALE = 2 (384 x 320
views, about 2.6 px), for the reason tests/test_projtex_flow_host.py states."""
from __future__ import annotations

import numpy as np

from tests import meshrender_ref, projtex_scenes as S

H1, W1, RES = 160, 192, 128
EYES = ([0.0, 0.0, -3.0], 210.0, 0.0), ([1.2, 0.3, -2.8], 200.0, 0.0), ([-1.0, -0.5, -2.9], 200.0, 0.3)
AIMS = ([0.0, 0.0, 0.0], [0.02, 0.0, 0.0], [0.0, 0.02, 0.0])
EXPOSURES = (1.0, 0.85, 1.15)
SCALE = 2
REGISTER = dict(block=16, stride=8, radius=4)


def size(scale: int = 1):
    return H1 * scale, W1 * scale


def cameras(scale: int = 1, aims=None):
    """(world-to-camera, intrinsics) per view: the cameras the views are projected with (aims None) or photographed with (AIMS)"""
    H, W = size(scale)
    return [S.camera(eye, aim, H, W, f * scale, roll) for (eye, f, roll), aim in zip(EYES, aims or [[0, 0, 0]] * 3)]


def detail_texture():
    """(smooth, detail) float32 [RES,RES,3]: the texture is their sum"""
    smooth = S.smooth_texture(RES, RES)
    noise = np.random.default_rng(0).standard_normal((RES + 4, RES + 4, 3))
    box = sum(noise[dy:dy + RES, dx:dx + RES] for dy in range(5) for dx in range(5)) / 25.0
    return smooth, (0.12 * box).astype(np.float32)


def misregistered(scale: int = 1):
    """the patch under three views; views 1 and 2 are photographed with a camera that aims a little off the one they are projected with"""
    from topo4d_amd.meshrender import triangulate
    obj, verts = S.patch_scene()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    H, W = size(scale)
    views = np.stack([S.view(eye, [0, 0, 0], H, W, f=f * scale, roll=roll) for eye, f, roll in EYES])
    shot_with = np.stack([S.view(eye, aim, H, W, f=f * scale, roll=roll) for (eye, f, roll), aim in zip(EYES, AIMS)])
    smooth, detail = detail_texture()

    def shoot(tex):
        return np.stack([meshrender_ref.render(verts, tris, uv_tris, obj.uvs, tex, v, H, W)[0] for v in shot_with])

    depth = np.stack([meshrender_ref.render(verts, tris, uv_tris, obj.uvs, smooth, v, H, W)[1] for v in views])
    pos, nrm, cov = S.patch_maps64(RES)
    pos, nrm = pos.astype(np.float32), nrm.astype(np.float32)             # what a device is given: host and device figures are the same bits
    exposed = shoot(smooth) * np.array(EXPOSURES, np.float32)[:, None, None, None]
    return dict(obj=obj, verts=verts, tris=tris, uv_tris=uv_tris, views=views, h=H, w=W, depth=depth, pos=pos, nrm=nrm, cov=cov,
                smooth=smooth, detail=detail, photos_detail=shoot(smooth + detail), photos_exposed=exposed)


def neighbour_steps(t, seen):
    """the differences of the pairs of compared texels that are horizontal or vertical neighbours, all channels"""
    across = (t[:, 1:] - t[:, :-1])[seen[:, 1:] & seen[:, :-1]]
    down = (t[1:] - t[:-1])[seen[1:] & seen[:-1]]
    return np.concatenate([across.reshape(-1), down.reshape(-1)])


def largest_step(t, seen):
    return float(np.abs(neighbour_steps(np.asarray(t, np.float64), seen)).max())


def detail_energy(t, seen):
    return float((neighbour_steps(np.asarray(t, np.float64), seen) ** 2).sum())


def compared(cov, count):
    """the texels all three views see, six texels inside the island"""
    return S.erode(np.asarray(cov) != 0, 6) & (np.asarray(count) == 3)


def figures(m, out_detail: dict, out_exposed: dict, seen) -> dict:
    """{"texels", "kept": {name: detail energy kept}, "step": {name: largest neighbour step}} of float textures [h,w,3] by name"""
    smooth = m["smooth"].astype(np.float64)
    truth = detail_energy(m["detail"], seen)
    return dict(texels=int(seen.sum()),
                kept={k: detail_energy(np.asarray(o, np.float64) - smooth, seen) / truth for k, o in out_detail.items()},
                step={k: largest_step(o, seen) for k, o in out_exposed.items()})


def three_ways(m, photos, register: dict):
    """({"weighted", "best", "registered": float32 [h,w,3]}, the three counts, view_flows' report of the last round) through the
    numpy chain: the two unregistered projections and "weighted" registered by project_frame's rule (consensus, hole fill, render
    into the cameras, view_flows, projection through the flows; `register`: view_flows' options and rounds)"""
    from tests import projtex_flow_ref as flow, texfill_ref, texfinish_ref
    a = (m["pos"], m["nrm"], m["cov"], m["views"], m["h"], m["w"], photos, m["depth"])
    out = {mode: flow.project_texture(*a, mode=mode) for mode in ("weighted", "best")}
    labels = (np.asarray(m["cov"]) != 0).astype(np.uint8)                   # one island
    options = {k: v for k, v in register.items() if k != "rounds"}
    consensus = out["weighted"]
    for _ in range(register.get("rounds", 1)):
        tex, _ = texfill_ref.fill_islands(texfinish_ref.quantize(consensus[0]), consensus[2] > 0, labels)
        renders = np.stack([meshrender_ref.render(m["verts"], m["tris"], m["uv_tris"], m["obj"].uvs, tex, v, m["h"], m["w"])[0] for v in m["views"]])
        flows, _, report = flow.view_flows(renders, photos, m["depth"], **options)
        consensus = flow.project_texture(*a, mode="weighted", flows=flows)
    out["registered"] = consensus
    return {k: o[0] for k, o in out.items()}, {k: o[2] for k, o in out.items()}, report


def measure(m, register: dict) -> dict:
    """figures() of three_ways on the detailed and on the unequally exposed photographs, with the kept blocks per view of each"""
    detail, counts, report = three_ways(m, m["photos_detail"], register)
    exposed, counts_e, report_e = three_ways(m, m["photos_exposed"], register)
    seen = compared(m["cov"], counts["weighted"])
    assert all((c[seen] == 3).all() for c in (*counts.values(), *counts_e.values()))
    return dict(figures(m, detail, exposed, seen), kept_blocks=[r["kept"] for r in report], kept_blocks_exposed=[r["kept"] for r in report_e])


def check(fig: dict) -> None:
    """the four conditions on figures(): registered "weighted" against unregistered "weighted" and "best" """
    kept, step = fig["kept"], fig["step"]
    assert fig["texels"] >= 3000
    assert kept["registered"] > kept["weighted"]
    assert kept["registered"] >= 0.9 * kept["best"]
    assert step["registered"] <= 1.25 * step["weighted"]
