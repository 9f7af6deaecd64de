"""GPU: the registration of the projected texture.  t4d_project_texture_flow / t4d_project_texture_bands_flow bit for bit against
tests/projtex_flow_ref.py under designed flows; an all-zero flow against no flow; projtex.view_flows against the chain of drift_ref
and stabilise_ref restatements on known shifts; project_frame(register=...) and write_frame against the whole numpy chain on a
rig of two image sizes; and what registration buys, held to the constants of tests/test_projtex_flow_host.py.

Known shifts (test_view_flows_recovers_a_known_shift).  The photograph is the consensus image moved by a constant shift, periodically.
drift.flow adds to the integer displacement the vertex of the parabola through the costs at -1, 0, +1, (qm - qp) / (2 (qm - 2 q0 +
qp)).  At an integer shift q0 = 0, and qm, qp are the same sum of Hamming distances over the block moved by one pixel, so they differ
by the block's two edge columns: the offset is small but only zero when the image repeats with the block's period.  "tiles" is
such an image (period 16 = the block, every pixel valid): there the flow on the supported interior is (512, -256) exactly, as
asserted.  "render" is the patch with the detailed texture in patch_views' first camera: there the chain stays within (3, 3) of
(512, -256) on the supported interior, in 1/256 px: not exact, and it cannot be, since the offset belongs to drift.flow's rule,
which this feature calls and does not change.  For the fractional shift (1.5, 0.25) px the parabola's bias towards the integer
shows (tests/test_drift_host.py).  WORST holds, per case, the largest |f - 256 shift| over the supported interior pixels in
1/256 px as the numpy chain gives it; the device must give the chain's bits, so it is held to these integers exactly."""
import json
import os

import numpy as np
import pytest
import torch

from tests import drift_ref, meshrender_ref, projtex_flow_ref as flow, projtex_ref as ref
from tests import projtex_register_scene as R, projtex_scenes as S
from tests.test_projtex_flow_host import MEASURED, REGISTER, same_figures
from topo4d_amd import meshrender, projtex, texfinish

pytestmark = pytest.mark.gpu
DEV = "cuda"
PARAMS = [dict(depth_tol=0.02), dict(power=0, fade_px=0.0, cos_min=0.3, depth_tol=0.01)]
GAINS = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])
SHIFTS = {"integer": (2.0, -1.0), "fractional": (1.5, 0.25)}
MARGIN = 24                                    # interior: this far from the image edge (block + radius + the census window)
# the largest |f_y - 256 s_y|, |f_x - 256 s_x| over the supported interior pixels, as the numpy chain gives them (module docstring)
WORST = {("tiles", "integer"): (0, 0), ("tiles", "fractional"): (0, 30), ("render", "integer"): (3, 3), ("render", "fractional"): (30, 58)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def bits(t):
    a = host(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g), bits(w_)), (what, k, int((bits(g) != bits(w_)).sum()))


# ---- 1, 2: the kernels ---------------------------------------------------------------------------------------------------------------
def _scene(name, res, seed=0):
    """the maps of surface_maps, the depth of MeshRenderer.render and random photographs on the device, and the host's copies"""
    if name == "quads":
        obj, views, h, w = S.three_quads(), S.three_views(), S.H, S.W
        verts = obj.vertices
    else:
        (obj, verts), views, h, w = S.patch_scene(), S.patch_views(), 80, 96
    v = dev(verts.astype(np.float32))
    pos, nrm, cov = projtex.surface_maps(obj, v, res, device=DEV)
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, np.zeros((1, 1, 3), np.uint8), device=DEV)
    cams = (dev(np.asarray(views, np.float32)), h, w)
    depth = r.render(v, cams)[1]
    photos = dev(np.random.default_rng(seed).uniform(0, 1, size=(3, 3, h, w)).astype(np.float32))
    a = dict(pos=pos, nrm=nrm, coverage=cov, cams=cams, photos=photos, depth=depth)
    return a, (host(pos), host(nrm), host(cov), views, h, w, host(photos), host(depth))


def designed_flows(b, kw, seed=1):
    """int16 [3,h,w,2] for the host copies `b` under the rule `kw`, and what the design reaches: view 0 random within +-3 px with
    sub-pixel parts and the int16 extremes on every pixel no accepted texel reads its flow from; view 1 all zero; view 2 random,
    with four blocks that push the taps over the left, right, top and bottom edge.  reached: per edge, the accepted texels of
    view 2 whose flow comes from that block."""
    pos, nrm, cov, views, h, w, photos, depth = b
    rng = np.random.default_rng(seed)
    flows = rng.integers(-768, 769, size=(3, h, w, 2)).astype(np.int16)
    flows[1] = 0
    near = []
    for v in (0, 2):
        ok = ref.view_samples(pos, nrm, cov, views[v], h, w, photos[v], depth[v], **kw)[0]
        px, py = flow.pixels(pos, views[v], h, w)
        near.append((np.floor(py[ok] + 0.5).astype(np.int64), np.floor(px[ok] + 0.5).astype(np.int64)))
    used = np.zeros((h, w), bool)
    used[near[0]] = True
    extremes = np.where((np.add.outer(np.arange(h), np.arange(w)) % 2 == 0)[..., None], np.int16(32767), np.int16(-32768))
    flows[0][~used] = np.broadcast_to(extremes, (h, w, 2))[~used]
    pushes = {"left": (0, -w * 256), "right": (0, w * 256), "top": (-h * 256, 0), "bottom": (h * 256, 0)}
    reached = {}
    for k, (edge, f) in enumerate(pushes.items()):
        y0, x0 = (h // 8 + (k // 2) * h // 2, w // 8 + (k % 2) * w // 2)
        flows[2, y0:y0 + h // 4, x0:x0 + w // 4] = f
        reached[edge] = int(((near[1][0] >= y0) & (near[1][0] < y0 + h // 4) & (near[1][1] >= x0) & (near[1][1] < x0 + w // 4)).sum())
    assert (~used).sum() > 100 and abs(h * 256) <= 32767 and abs(w * 256) <= 32767
    return flows, reached


@pytest.mark.parametrize("name, res", [("quads", (32, 32)), ("quads", (40, 56)), ("patch", (128, 128))])
def test_bit_equal_to_the_restatement(name, res):
    a, b = _scene(name, res)
    th, tw = res
    skip = np.random.default_rng(2).integers(0, 1 << 4, size=(th, tw)).astype(np.int32)         # bits 0 .. 3; the launch's views are 1 .. 3
    low = projtex.low_band(a["photos"], a["depth"], 2)
    for kw in PARAMS:
        flows, reached = designed_flows(b, kw)
        print(name, res, kw, "accepted texels of view 2 pushed over each edge", reached)
        assert all(n > 0 for n in reached.values()), reached
        f = dev(flows)
        variants = [({}, {}), (dict(gains=GAINS), dict(gains=GAINS)), (dict(skip=dev(skip), skip_base=1), dict(skip=skip, skip_base=1)),
                    (dict(gains=GAINS, skip=dev(skip), skip_base=1), dict(gains=GAINS, skip=skip, skip_base=1))]
        for on_device, on_host in variants:
            for mode in ("weighted", "best"):
                got = projtex.project(**a, mode=mode, flows=f, **on_device, **kw)
                want = flow.project_texture(*b, mode=mode, flows=flows, **on_host, **kw)
                same(got, want, (name, res, kw, mode, sorted(on_host)))
                plain = ref.project_texture(*b, mode=mode, **kw) if not on_host else None
                if plain is not None:                             # the design bites: views are lost to the edges, colours move
                    assert (want[2] < plain[2]).sum() > 20 and (want[2] > 0).sum() > 100 and (bits(want[0]) != bits(plain[0])).any()
            got = projtex.project_bands(**a, low=low, flows=f, **on_device, **kw)
            want = flow.project_bands(*b[:7], host(low), b[7], flows=flows, **on_host, **kw)
            same(got, want, (name, res, kw, "bands", sorted(on_host)))
        assert got[0].dtype == torch.float32 and got[2].dtype == torch.uint8


@pytest.mark.parametrize("name, res", [("quads", (40, 56)), ("patch", (64, 64))])
def test_zero_is_none(name, res):
    a, b = _scene(name, res, seed=4)
    zero = torch.zeros(3, b[4], b[5], 2, dtype=torch.int16, device=DEV)
    skip = dev(np.random.default_rng(2).integers(0, 1 << 3, size=res).astype(np.int32))
    low = projtex.low_band(a["photos"], a["depth"], 3)
    for kw in PARAMS:
        for more in ({}, dict(gains=GAINS, skip=skip)):
            for mode in ("weighted", "best"):
                none = projtex.project(**a, mode=mode, **more, **kw)
                same(projtex.project(**a, mode=mode, flows=zero, **more, **kw), none, (name, mode, kw))
                assert (none[2] > 0).sum() > 100
            same(projtex.project_bands(**a, low=low, flows=zero, **more, **kw), projtex.project_bands(**a, low=low, **more, **kw), (name, "bands", kw))
    with pytest.raises(ValueError, match="flows"):
        projtex.project(**a, flows=zero[:2])
    with pytest.raises(ValueError, match="flows"):
        projtex.project(**a, flows=zero.cpu())


# ---- 3: view_flows on known shifts -----------------------------------------------------------------------------------------------------
def consensus_image(kind):
    """(render [3,h,w] float32, depth [1,h,w] float32) at 80 x 96: "tiles" repeats a smoothed random 16 x 16 tile, every pixel
    valid; "render" is the detailed patch in patch_views' first camera"""
    h, w = 80, 96
    if kind == "tiles":
        t = np.random.default_rng(5).random((3, 16, 16))
        t = sum(np.roll(t, (j, i), (1, 2)) for j in (-1, 0, 1) for i in (-1, 0, 1)) / 9.0
        t = 0.1 + 0.8 * (t - t.min()) / (t.max() - t.min())
        return np.tile(t, (1, h // 16, w // 16)).astype(np.float32), np.ones((1, h, w), np.float32)
    from topo4d_amd.meshrender import triangulate
    obj, verts = S.patch_scene()
    tris, uv_tris = triangulate(obj.faces_ori, obj.uv_faces_ori)
    smooth, detail = R.detail_texture()
    image, depth, _ = meshrender_ref.render(verts, tris, uv_tris, obj.uvs, smooth + detail, S.patch_views(h, w)[0], h, w)
    return image, depth


def moved(render, shift):
    """the photograph: b(p + shift) = a(p), periodically (an integer shift moves the very values)"""
    if all(float(s).is_integer() for s in shift):
        return np.roll(render, (int(shift[0]), int(shift[1])), (1, 2))
    return np.stack([drift_ref.shift_periodic(c.astype(np.float64), *shift) for c in render]).astype(np.float32)


def worst_on_interior(flows, support, shift):
    m = np.zeros(support.shape, bool)
    m[MARGIN:-MARGIN, MARGIN:-MARGIN] = True
    m &= support != 0
    assert m.sum() > 1000
    off = np.abs(flows[m].astype(np.int64) - np.rint(256 * np.asarray(shift)).astype(np.int64))
    return int(off[:, 0].max()), int(off[:, 1].max())


@pytest.mark.parametrize("shift", list(SHIFTS))
@pytest.mark.parametrize("kind", ["tiles", "render"])
def test_view_flows_recovers_a_known_shift(kind, shift):
    s = SHIFTS[shift]
    render, depth = consensus_image(kind)
    other, other_depth = consensus_image("render" if kind == "tiles" else "tiles")      # a second view: the views go one by one
    renders, photos, depths = np.stack([render, other]), np.stack([moved(render, s), other]), np.stack([depth, other_depth])
    flows, support, report = projtex.view_flows(dev(renders), dev(photos), dev(depths), **R.REGISTER)
    want = flow.view_flows(renders, photos, depths, **R.REGISTER)
    assert flows.dtype == torch.int16 and support.dtype == torch.uint8 and tuple(flows.shape) == (2, 80, 96, 2)
    same((flows, support), want[:2], (kind, shift))
    assert report == want[2], (report, want[2])                  # every float of the report, to the bit
    assert report[0]["kept"] >= 40 and not flows[0][support[0] == 0].any()
    assert report[1]["kept"] >= 40 and report[1]["max"] < 0.05   # the second view is its own photograph: kept, and but for the parabola's offset at rest
    worst = worst_on_interior(host(flows[0]), host(support[0]), s)
    print(kind, shift, "kept", report[0]["kept"], "of", report[0]["blocks"], "largest |f - 256 shift| on the supported interior", worst,
          "mean |d|", report[0]["mean"])
    assert worst == WORST[kind, shift]
    if (kind, shift) == ("tiles", "integer"):
        m = np.zeros((80, 96), bool)
        m[MARGIN:-MARGIN, MARGIN:-MARGIN] = True
        m &= host(support[0]) != 0
        assert (host(flows[0])[m] == np.array([512, -256])).all()


# ---- 4: the frame ------------------------------------------------------------------------------------------------------------------------
def _rig():
    """the patch with the detailed texture under four cameras of two image sizes; cameras 1 .. 3 are photographed aiming a little
    off the camera they are projected with"""
    from topo4d_amd import cameras as C
    obj, verts = S.patch_scene()
    smooth, detail = R.detail_texture()
    shots = [([0.0, 0.0, -3.0], [0.0, 0.0, 0.0], 80, 96, 105.0, 0.0), ([1.2, 0.3, -2.8], [0.03, 0.0, 0.0], 96, 80, 100.0, 0.0),
             ([-1.0, -0.5, -2.9], [0.0, 0.03, 0.0], 80, 96, 100.0, 0.3), ([0.4, -0.8, -2.9], [-0.02, -0.02, 0.0], 96, 80, 100.0, -0.2)]
    v = dev(verts.astype(np.float32))
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    painted = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, dev(smooth + detail), device=DEV)
    dataset = []
    for k, (eye, aim, h, w, f, roll) in enumerate(shots):
        cam = C.setup_camera(None, w, h, *S.camera(eye, [0, 0, 0], h, w, f, roll)[::-1], device=DEV)
        shot_with = C.setup_camera(None, w, h, *S.camera(eye, aim, h, w, f, roll)[::-1], device=DEV)
        dataset.append({"cam": cam, "im": painted.render(v, [shot_with])[0][0], "cam_name": f"cam{k}"})
    return obj, verts, v, faces, uv_faces, dataset


def _chain_inputs(obj, v, faces, uv_faces, dataset, res):
    from topo4d_amd.rasterizer import pack_views
    pos, nrm, cov = projtex.surface_maps(obj, v, res, device=DEV)
    labels = projtex.island_labels(obj, res, res, device=DEV)
    blank = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, np.zeros((1, 1, 3), np.uint8), device=DEV)
    groups, order = [], []
    for size in ((80, 96), (96, 80)):
        ks = [k for k, e in enumerate(dataset) if (int(e["cam"].image_height), int(e["cam"].image_width)) == size]
        cams = [dataset[k]["cam"] for k in ks]
        views = host(pack_views(cams, torch.device(DEV, torch.cuda.current_device())))
        groups.append((views, *size, np.stack([host(dataset[k]["im"]) for k in ks]), host(blank.render(v, cams)[1])))
        order += ks
    return (host(pos), host(nrm), host(cov), host(labels)), groups, order


@pytest.fixture(scope="module")
def rig():
    obj, verts, v, faces, uv_faces, dataset = _rig()
    maps, groups, order = _chain_inputs(obj, v, faces, uv_faces, dataset, 64)
    return dict(obj=obj, verts=verts, v=v, faces=faces, uv_faces=uv_faces, dataset=dataset, maps=maps, groups=groups, order=order)


RIG_RULE = dict(power=2, cos_min=0.1, fade_px=4.0, depth_tol=0.02)
RIG_REGISTER = dict(block=16, stride=8, radius=4, rounds=2)


@pytest.mark.parametrize("mode", ["weighted", "best", "twoband"])
def test_project_frame_registers_over_two_image_sizes(rig, mode):
    g = rig
    gains = np.array([[1.0, 1.0, 1.0], [1.05, 0.95, 1.0], [0.9, 1.0, 1.1], [1.0, 1.02, 0.97]])
    tex, weight, count, _, found = projtex._project_frame(g["obj"], g["v"], g["dataset"], 64, dict(RIG_RULE, mode=mode), gains, DEV, 2, None,
                                                          RIG_REGISTER)
    mesh = (g["verts"].astype(np.float32), g["faces"], g["uv_faces"], g["obj"].uvs)
    want = flow.register_frame(*g["maps"], g["groups"], mesh, mode, RIG_RULE, RIG_REGISTER, gains=gains[g["order"]], band_radius=2)
    assert found["order"] == g["order"] == [0, 2, 1, 3]
    for i in range(2):
        same((found["flows"][i], found["support"][i]), (want[3][i], want[4][i]), (mode, "flows of group", i))
    assert [found["report"][k] for k in g["order"]] == want[5]
    kept = [r["kept"] for r in found["report"]]
    print(mode, "kept blocks per view", kept, "mean |d|", [round(r.get("mean", 0.0), 3) for r in found["report"]])
    assert min(kept) >= 10 and any(bool(f.any()) for f in found["flows"])
    same((tex, weight, count), want[:3], mode)
    public = projtex.project_frame(g["obj"], g["v"], g["dataset"], 64, mode=mode, gains=gains, band_radius=2, register=RIG_REGISTER, **RIG_RULE)
    same(public, (tex, weight, count), (mode, "project_frame"))
    free = projtex.project_frame(g["obj"], g["v"], g["dataset"], 64, mode=mode, gains=gains, band_radius=2, **RIG_RULE)
    assert (host(free[0]) != host(tex)).any()                    # the registration moves colours
    with pytest.raises(ValueError):
        projtex.project_frame(g["obj"], g["v"], g["dataset"], 64, mode=mode, register=dict(rounds=4))


def test_write_frame_writes_what_it_wrote_and_the_report(rig, tmp_path):
    from topo4d_amd.png import encode_png
    g = rig
    obj, dataset = g["obj"], g["dataset"]
    opts = dict(projtex.DEFAULTS, **RIG_RULE)
    dirs = {k: str(tmp_path / k) for k in ("plain", "registered")}
    for d in dirs.values():
        os.makedirs(d)
    kw = dict(pad=2, sizes=[32], save_weight=True, device=DEV)
    plain = projtex.write_frame(dirs["plain"], obj, None, dataset, 64, opts, **kw)
    assert [os.path.basename(p) for p in plain] == ["face_proj.png", "face_proj_32.png", "face_proj_weight.png"]
    verts = torch.from_numpy(obj.vertices).to(DEV)
    tex, _, count = projtex.project_frame(obj, verts, dataset, 64, device=DEV, **opts)
    levels = texfinish.finish(tex, (count > 0).to(torch.uint8), pad=2, erode=0, sizes=[32])
    for name, image in (("face_proj.png", levels[64]), ("face_proj_32.png", levels[32]), ("face_proj_weight.png", count)):
        with open(os.path.join(dirs["plain"], name), "rb") as f:
            assert f.read() == bytes(encode_png(image)), name
    written = projtex.write_frame(dirs["registered"], obj, None, dataset, 64, opts, register=RIG_REGISTER, save_flows=True, **kw)
    assert [os.path.basename(p) for p in written] == ["face_proj.png", "face_proj_32.png", "face_proj_weight.png", "face_proj_register.json",
                                                      "face_proj_flows.npz"]
    tex_r, _, count_r, _, found = projtex._project_frame(obj, verts, dataset, 64, opts, None, DEV, 8, None, RIG_REGISTER)
    levels = texfinish.finish(tex_r, (count_r > 0).to(torch.uint8), pad=2, erode=0, sizes=[32])
    with open(os.path.join(dirs["registered"], "face_proj.png"), "rb") as f:
        assert f.read() == bytes(encode_png(levels[64]))
    with open(os.path.join(dirs["registered"], "face_proj_register.json")) as f:
        doc = json.load(f)
    assert doc == {"options": dict(RIG_REGISTER, ratio=0.8, reach=1), "cameras": ["cam0", "cam1", "cam2", "cam3"], "report": found["report"]}
    with np.load(os.path.join(dirs["registered"], "face_proj_flows.npz")) as z:
        assert sorted(z.files) == ["cameras_80x96", "cameras_96x80", "flows_80x96", "flows_96x80", "support_80x96", "support_96x80"]
        assert z["cameras_80x96"].tolist() == ["cam0", "cam2"] and z["cameras_96x80"].tolist() == ["cam1", "cam3"]
        for i, size in enumerate(("80x96", "96x80")):
            assert np.array_equal(z["flows_" + size], host(found["flows"][i])) and np.array_equal(z["support_" + size], host(found["support"][i]))


# ---- what registration buys, on the device ---------------------------------------------------------------------------------------------
def _three_ways_on_device(m, photos, register):
    a = dict(pos=dev(m["pos"]), nrm=dev(m["nrm"]), coverage=dev(m["cov"].astype(np.uint8)), cams=(dev(m["views"]), m["h"], m["w"]),
             photos=dev(photos), depth=dev(m["depth"]))
    out = {mode: projtex.project(**a, mode=mode) for mode in ("weighted", "best")}
    labels = a["coverage"]                                       # one island
    v = dev(m["verts"].astype(np.float32))
    options = {k: x for k, x in register.items() if k != "rounds"}
    consensus = out["weighted"]
    for _ in range(register["rounds"]):
        tex, _ = texfinish.fill_islands(texfinish.quantize(consensus[0]), (consensus[2] > 0).to(torch.uint8), labels)
        renders = meshrender.MeshRenderer(m["tris"], m["uv_tris"], m["obj"].uvs, tex, device=DEV).render(v, a["cams"], mapping="bilinear")[0]
        flows, _, report = projtex.view_flows(renders, a["photos"], a["depth"], **options)
        consensus = projtex.project(**a, mode="weighted", flows=flows)
    out["registered"] = consensus
    return {k: host(o[0]) for k, o in out.items()}, {k: host(o[2]) for k, o in out.items()}, report


def test_registration_keeps_the_detail_of_best_and_the_seams_of_weighted():
    """the figures of tests/test_projtex_flow_host.py's numpy chain, on the device: the same inputs, so the same constants"""
    m = R.misregistered(R.SCALE)
    detail, counts, report = _three_ways_on_device(m, m["photos_detail"], REGISTER)
    exposed, counts_e, report_e = _three_ways_on_device(m, m["photos_exposed"], REGISTER)
    seen = R.compared(m["cov"], counts["weighted"])
    assert all((c[seen] == 3).all() for c in (*counts.values(), *counts_e.values()))
    fig = dict(R.figures(m, detail, exposed, seen), kept_blocks=[r["kept"] for r in report], kept_blocks_exposed=[r["kept"] for r in report_e])
    print("on the device", json.dumps(fig))
    R.check(fig)
    same_figures(fig, MEASURED)
