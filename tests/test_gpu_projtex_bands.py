"""GPU: the two-band projection of topo4d_amd.projtex (k_low_band, k_projtex_bands in csrc/t4d_projtex.hip) bit for bit against
its float64 yardsticks tests/projtex_bands_ref.py, its agreement with mode "weighted" at radius 0, project_frame's merge of two
image sizes, and the command lines on a small run of topo4d_amd.train over tests/capture_scene.py's sequence."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import projtex_bands_ref as ref, projtex_scenes as S
from tests.test_gpu_projtex import PARAMS, SIZES, TOL, _io, _setup, _train, _tree, bits, dev
from topo4d_amd import meshrender, projtex

pytestmark = pytest.mark.gpu
DEV = "cuda"
GAINS = np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7]])
NAMES = ("low_color", "weight", "count", "high", "best_weight")


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def quads():
    """three_quads under three_views at 48 x 40 (no multiple of the low band's 64 x 32 tile, nor of the projection's 16): the device's
    own depth renders, random photographs with a NaN in a background pixel of every view, and their low bands per radius on the host"""
    obj, views = S.three_quads(), S.three_views()
    a, index = _setup(obj, views, (40, 56))
    depth = host(a["depth"])
    assert depth.shape == (3, 1, S.H, S.W) and 0.2 < (depth > 0).mean() < 0.9
    photos = host(a["photos"]).copy()
    for v in range(3):
        off = np.argwhere(depth[v, 0] == 0)                      # (the close view leaves only a few)
        y, x = off[len(off) // 2]
        photos[v, :, y, x] = np.nan
    return dict(obj=obj, views=views, photos=photos, depth=depth, low={r: ref.low_band(photos, depth, r) for r in (0, 1, 5, 32)})


@pytest.mark.parametrize("radius", [0, 1, 5, 32])
def test_low_band_is_bit_equal_to_the_yardstick(quads, radius):
    photos, depth = dev(quads["photos"]), dev(quads["depth"])
    low = projtex.low_band(photos, depth, radius)
    assert low.shape == photos.shape and low.dtype == torch.float32 and low.data_ptr() != photos.data_ptr()
    got, want = host(low), quads["low"][radius]
    assert np.isfinite(got).all()                                # the NaNs lie off the mesh
    assert np.array_equal(bits(got), bits(want)), (radius, int((bits(got) != bits(want)).sum()))
    on = np.broadcast_to(quads["depth"] > 0, got.shape)
    if radius == 0:
        assert np.array_equal(bits(got[on]), bits(quads["photos"][on])) and not got[~on].any()
    else:
        assert got[~on].any() and not np.array_equal(got[on], quads["photos"][on])
    if radius == 32:                                             # wider than the image: the boxes of rows 7 .. 32, columns 15 .. 32 hold all of it
        assert not np.ptp(got[:, :, 7:33, 15:33], axis=(2, 3)).any() and np.ptp(got, axis=(2, 3)).all()
    # a single view without any mesh: exact zeros
    none = projtex.low_band(photos[1:2], torch.zeros_like(depth[1:2]), radius)
    assert none.shape == (1, 3, S.H, S.W) and not bits(host(none)).any()


def test_low_band_over_many_tiles():
    """200 x 150 pixels: four by five workgroups per view and channel, the last of each row and column cut off"""
    rng = np.random.default_rng(11)
    photos = rng.uniform(0, 1, size=(2, 3, 150, 200)).astype(np.float32)
    y, x = np.mgrid[0:150, 0:200]
    depth = np.stack([(np.hypot(y - 70, x - 90) < 66), ((y + x) % 7 != 0) & (x > 30)]).astype(np.float32)[:, None] * 3.0
    for radius in (3, 8, 31):
        got = host(projtex.low_band(dev(photos), dev(depth), radius))
        want = ref.low_band(photos, depth, radius)
        assert np.array_equal(bits(got), bits(want)), (radius, int((bits(got) != bits(want)).sum()))


def _bands_args(res, n_views, quads):
    a, _ = _setup(quads["obj"], quads["views"][:n_views], res)
    a["photos"] = dev(quads["photos"][:n_views])
    assert np.array_equal(host(a["depth"]), quads["depth"][:n_views])
    return a


def _want(a, views, low, **kw):
    return ref.project_bands(host(a["pos"]), host(a["nrm"]), host(a["coverage"]), views, S.H, S.W, host(a["photos"]), low,
                             host(a["depth"]), **kw)


def _same(got, want, what):
    for g, w_, name in zip(got, want, NAMES):
        assert np.array_equal(bits(host(g)), bits(w_)), (what, name, int((bits(host(g)) != bits(w_)).sum()))


@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("res", SIZES)
def test_project_bands_is_bit_equal_to_the_yardstick(quads, res, n_views):
    a = _bands_args(res, n_views, quads)
    views = quads["views"][:n_views]
    cov = host(a["coverage"]) != 0
    low = quads["low"][5][:n_views]
    for kw in PARAMS:
        for gains in (None, GAINS[:n_views]):
            got = projtex.project_bands(**a, low=dev(low), gains=gains, **kw)
            _same(got, _want(a, views, low, gains=gains, **kw), (res, n_views, kw, gains is not None))
            assert [t.dtype for t in got] == [torch.float32, torch.float32, torch.uint8, torch.float32, torch.float32]
            assert [tuple(t.shape) for t in got] == [(*res, 3), res, res, (*res, 3), res]
            count = host(got[2])
            assert count.max() == n_views and (count[cov] == 0).any()
            for t in got:
                assert not bits(host(t))[~cov].any() and not bits(host(t))[count == 0].any()
            assert np.abs(host(got[3])).max() > 0.1 and (host(got[4]) <= host(got[1])).all()
    # the low bands are an input like any other: another radius, other outputs
    other = projtex.project_bands(**a, low=dev(quads["low"][1][:n_views]))
    _same(other, _want(a, views, quads["low"][1][:n_views]), (res, n_views, "radius 1"))
    assert not np.array_equal(host(other[0]), host(projtex.project_bands(**a, low=dev(low))[0]))


@pytest.mark.parametrize("res", SIZES)
def test_radius_zero_is_the_weighted_projection_with_no_detail(quads, res):
    a = _bands_args(res, 3, quads)
    low = projtex.low_band(a["photos"], a["depth"], 0)
    for kw in PARAMS:
        for gains in (None, GAINS):
            lc, weight, count, high, bw = projtex.project_bands(**a, low=low, gains=gains, **kw)
            assert not bits(host(high)).any()
            for mode, got in (("weighted", (lc, weight, count)), ("best", (None, bw, count))):
                want = projtex.project(**a, mode=mode, gains=gains, **kw)
                for g, w_ in zip(got, want):
                    assert g is None or np.array_equal(bits(host(g)), bits(host(w_))), (mode, kw)
            assert (count == 3).any()
    with pytest.raises(ValueError, match="project_bands"):
        projtex.project(**a, mode="twoband")
    with pytest.raises(ValueError):
        projtex.project_bands(**a, low=low[:2])
    with pytest.raises(ValueError):
        projtex.project_bands(**a, low=low.cpu())
    with pytest.raises(ValueError):
        projtex.low_band(a["photos"], a["depth"], 33)


@pytest.mark.parametrize("gains", [None, np.array([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05], [1.0, 1.0, 0.7], [0.9, 1.1, 1.2]])])
def test_project_frame_merges_the_bands_of_two_image_sizes(gains):
    """a rig with turned cameras, as tests/test_gpu_projtex.py has it: per size the yardsticks give the five maps; the low bands
    merge as weighted sums, the detail goes with the larger best weight (the earlier size on ties), the texture is their sum,
    clamped to [0, 1].  The merge itself runs in float32 and the result is quantised by truncation, so a texel may differ by one level."""
    from topo4d_amd import cameras as C
    from topo4d_amd.rasterizer import pack_views
    obj = S.three_quads()
    shots = [([0.9, 0.5, -2.6], [0.1, 0.0, 0.0], 40, 48, 44.0, 0.0), ([0.2, 0.3, -2.2], [0.0, 0.0, 0.0], 48, 40, 42.0, 1.2),
             ([-0.3, -0.2, -2.4], [0.0, 0.1, 0.0], 40, 48, 40.0, 0.6), ([0.1, -0.4, -2.5], [0.2, 0.0, 0.0], 48, 40, 40.0, -0.4)]
    rng = np.random.default_rng(5)
    dataset = []
    for eye, target, h, w, f, roll in shots:
        w2c, K = S.camera(eye, target, h, w, f, roll)
        # mild photographs (a bright field with some texture), so that the sum of the bands mostly stays inside [0, 1]
        im = 0.5 + 0.3 * rng.uniform(-1, 1, size=(3, h, w))
        dataset.append({"cam": C.setup_camera(None, w, h, K, w2c, device=DEV), "im": dev(im.astype(np.float32))})
    verts = dev(obj.vertices.astype(np.float32))
    opts = dict(power=2, cos_min=0.1, fade_px=4.0, depth_tol=0.01)
    tex, weight, count = projtex.project_frame(obj, verts, dataset, (40, 56), mode="twoband", band_radius=2, gains=gains, **opts)
    pos, nrm, cov = projtex.surface_maps(obj, verts, (40, 56), device=DEV)
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, np.zeros((1, 1, 3), np.uint8), device=DEV)
    parts = []
    for size in ((40, 48), (48, 40)):
        ks = [k for k, s in enumerate(shots) if (s[2], s[3]) == size]
        cams = [dataset[k]["cam"] for k in ks]
        depth = host(r.render(verts, cams)[1])
        photos = np.stack([host(dataset[k]["im"]) for k in ks])
        views = host(pack_views(cams, torch.device(DEV, torch.cuda.current_device())))
        out = ref.project_bands(host(pos), host(nrm), host(cov), views, *size, photos, ref.low_band(photos, depth, 2), depth,
                                gains=None if gains is None else gains[ks], **opts)
        parts.append([x.astype(np.float64) for x in out])
    (l0, w0, n0, h0, b0), (l1, w1, n1, h1, b1) = parts
    assert (n0 > 0).sum() > 100 and (n1 > 0).sum() > 100 and ((n0 > 0) & (n1 > 0)).sum() > 50
    want_w = w0 + w1
    with np.errstate(all="ignore"):
        low = np.where((want_w > 0)[..., None], (l0 * w0[..., None] + l1 * w1[..., None]) / want_w[..., None], 0.0)
    take = b1 > b0
    assert take.any() and (~take & (b0 > 0)).any()
    want_c = np.clip(low + np.where(take[..., None], h1, h0), 0.0, 1.0)
    assert np.array_equal(host(count), (n0 + n1).astype(np.uint8))
    assert np.abs(host(weight) - want_w).max() <= 1e-6 * max(1.0, want_w.max())
    levels = np.floor(want_c * 255.0)
    assert np.abs(host(tex).astype(np.float64) - levels).max() <= 1
    assert (host(tex) == levels).mean() > 0.99
    assert tex.dtype == torch.uint8 and not host(tex)[(n0 + n1) == 0].any()
    # the radius matters, and radius 0 is the weighted frame (these photographs times these gains stay below 1)
    flat = projtex.project_frame(obj, verts, dataset, (40, 56), mode="weighted", gains=gains, **opts)
    zero = projtex.project_frame(obj, verts, dataset, (40, 56), mode="twoband", band_radius=0, gains=gains, **opts)
    assert all(torch.equal(z, f) for z, f in zip(zero, flat)) and not torch.equal(tex, flat[0])
    with pytest.raises(ValueError):
        projtex.project_frame(obj, verts, dataset, (40, 56), mode="twoband", band_radius=33)


# ---- trees -----------------------------------------------------------------------------------------------------------------------
RES = ["-tr", "128"]
BAND = ["--mode", "twoband", "--band_radius", "3"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    root = tmp_path_factory.mktemp("projtex_bands_run")
    dirs = write_sequence(root, golden(), n_frames=3)
    plain = _train(dirs, str(root / "plain"), *RES, "--tex_project", *TOL, frames="1", tex=False)
    band = _train(dirs, str(root / "band"), *RES, "--tex_project", *BAND, *TOL, frames="1", tex=False)
    return dict(root=root, dirs=dirs, plain=plain, band=band)


def _project(runs, tmp_path, name, *flags):
    out = str(tmp_path / name)
    shutil.copytree(os.path.dirname(os.path.dirname(runs["plain"])), out)
    projtex.main(_io(runs) + ["-od", out, "--tex_res", "128"] + TOL + list(flags))
    return os.path.join(out, "exp", "seq")


def _frame(runs, run_dir):
    from topo4d_amd import cameras as C, evaluate as E, ingest
    cams, _, trans_g = C.get_cameras(runs["dirs"]["input_dir"], "seq", resize_factor=1)
    obj = meshrender.read_face_obj(os.path.join(run_dir, "000001", "face.obj"))
    ds = ingest.get_dataset(runs["dirs"]["dense_input_dir"], "seq", 1, cams, use_mask=False, blacklist=C.BLACKLIST,
                            rotate_mask=C.ROTATE_MASK, setup_camera=C.setup_camera, device=DEV)
    return obj, torch.from_numpy(E.training_vertices(obj.vertices, trans_g)).to(DEV), ds


def test_the_command_lines_write_the_two_band_frame_and_leave_the_rest_alone(runs, tmp_path):
    from PIL import Image
    name = os.path.join("000001", projtex.FILE_NAME)
    plain, band = _tree(runs["plain"]), _tree(runs["band"])
    assert sorted(plain) == sorted(band) and name in plain and projtex.GAINS_NAME not in band
    assert [n for n in plain if plain[n] != band[n] and not n.endswith(".npz")] == [name]
    obj, verts, ds = _frame(runs, runs["plain"])
    want = {mode: projtex.project_frame(obj, verts, ds, 128, depth_tol=0.02, mode=mode, band_radius=3) for mode in ("weighted", "twoband")}
    assert not torch.equal(want["weighted"][0], want["twoband"][0]) and torch.equal(want["weighted"][2], want["twoband"][2])
    seen = host(want["twoband"][2]) > 0
    print("texels with a view", seen.mean(), "levels that differ from weighted", (host(want["weighted"][0]) != host(want["twoband"][0])).mean())
    assert seen.mean() > 0.05 and not host(want["twoband"][0])[~seen].any()
    # python -m topo4d_amd.projtex: with the flags the two-band frame, the file train wrote; without them what it always wrote
    got = _tree(_project(runs, tmp_path, "band", *BAND, "--save_weight"))
    assert got[name] == band[name]
    assert np.array_equal(np.asarray(Image.open(os.path.join(runs["band"], name))), host(want["twoband"][0]))
    assert np.array_equal(np.asarray(Image.open(os.path.join(str(tmp_path / "band"), "exp", "seq", "000001", projtex.WEIGHT_NAME))),
                          host(want["twoband"][2]))
    default, weighted = _tree(_project(runs, tmp_path, "default")), _tree(_project(runs, tmp_path, "weighted", "--mode", "weighted", "--band_radius", "5"))
    assert default == weighted and default[name] == plain[name]
    assert np.array_equal(np.asarray(Image.open(os.path.join(runs["plain"], name))), host(want["weighted"][0]))
    # with a gutter, a smaller level and the equalisation: the options are recorded, the files are there
    run_dir = _project(runs, tmp_path, "all", *BAND, "--tex_pad", "2", "--tex_sizes", "64", "--equalize")
    doc = json.load(open(os.path.join(run_dir, projtex.GAINS_NAME)))
    assert doc["options"]["mode"] == "twoband" and doc["options"]["band_radius"] == 3
    assert np.asarray(Image.open(os.path.join(run_dir, "000001", "face_proj_64.png"))).shape == (64, 64, 3)
    gains = projtex.read_gains(os.path.join(run_dir, projtex.GAINS_NAME), [e["cam_name"] for e in ds])
    tex, _, count = projtex.project_frame(obj, verts, ds, 128, depth_tol=0.02, mode="twoband", band_radius=3, gains=gains)
    png = np.asarray(Image.open(os.path.join(run_dir, name)))
    assert np.array_equal(png[host(count) > 0], host(tex)[host(count) > 0])
    plain_doc = json.load(open(os.path.join(_project(runs, tmp_path, "eq", "--equalize"), projtex.GAINS_NAME)))
    assert "band_radius" not in plain_doc["options"] and plain_doc["gains"] == doc["gains"]
    with pytest.raises(SystemExit):
        _project(runs, tmp_path, "bad", "--mode", "twoband", "--band_radius", "33")


def test_evaluate_scores_the_two_band_texture(runs, tmp_path):
    from topo4d_amd import evaluate as E
    out = str(tmp_path / "out")
    shutil.copytree(os.path.dirname(os.path.dirname(runs["band"])), out)
    path = os.path.join(out, "exp", "seq", "eval.json")
    E.main(_io(runs) + ["-od", out, "--texture", "face_proj.png"])
    res = json.load(open(path))
    assert res["texture_file"] == "face_proj.png"
    fr = res["low"]["frames"]["000001"] if "000001" in res["low"]["frames"] else res["low"]["frames"]["1"]
    assert fr["texture"] is True
    for name, row in fr["views"].items():
        assert all(np.isfinite(row[n]) for n in ("l1", "mse", "psnr", "ssim", "psnr_full")), (name, row)
