"""GPU: topo4d_amd.projtex (csrc/t4d_projtex.hip) bit for bit against its float64 yardstick tests/projtex_ref.py, its occlusion
against an independent ray cast, a round trip through meshrender.MeshRenderer, and the command lines on a small run of
topo4d_amd.train over tests/capture_scene.py's three-frame sequence.

Round trip: the float64 pipeline on the host (meshrender_ref photographs, projtex_ref projects through float64 texel maps;
tests/test_projtex_host.py::test_round_trip_figure_of_the_float64_pipeline) has a maximum error of 3.1454e-4 against the analytic
texture, in both modes, over the 8649 texels seen by a view and two texels inside the island; ROUND_TRIP_F64 = 3.14534e-4 records it,
and the GPU result must stay within 1.5 x that."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import meshrender_ref, projtex_ref as ref, projtex_scenes as S
from tests.test_projtex_host import ROUND_TRIP_F64
from topo4d_amd import meshrender, projtex

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(64, 64), (40, 56)]                   # the second: no multiple of the 16-texel tile, not square
PARAMS = [dict(), dict(power=0, fade_px=0.0, cos_min=0.3, depth_tol=0.01)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _setup(obj, views, res, h=S.H, w=S.W, seed=0):
    """the maps of surface_maps, the depth of MeshRenderer.render and random photographs, all on the device"""
    verts = dev(obj.vertices.astype(np.float32))
    pos, nrm, cov = projtex.surface_maps(obj, verts, res, device=DEV)
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, np.zeros((1, 1, 3), np.uint8), device=DEV)
    cams = (dev(np.asarray(views, np.float32)), h, w)
    _, depth, index = r.render(verts, cams)
    photos = torch.from_numpy(np.random.default_rng(seed).uniform(0, 1, size=(len(views), 3, h, w)).astype(np.float32)).to(DEV)
    return dict(pos=pos, nrm=nrm, coverage=cov, cams=cams, photos=photos, depth=depth), index


def _want(a, views, h=S.H, w=S.W, **kw):
    return ref.project_texture(a["pos"].cpu().numpy(), a["nrm"].cpu().numpy(), a["coverage"].cpu().numpy(), views, h, w,
                               a["photos"].cpu().numpy(), a["depth"].cpu().numpy(), **kw)


def _same(got, want, what):
    for g, w_, name in zip(got, want, ("color", "weight", "count")):
        assert np.array_equal(bits(g), bits(w_)), (what, name, int((bits(g) != bits(w_)).sum()))


@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("res", SIZES)
def test_bit_equal_to_the_yardstick(res, n_views):
    obj, views = S.three_quads(), S.three_views()[:n_views]
    a, index = _setup(obj, views, res)
    cov = a["coverage"].cpu().numpy() != 0
    assert a["pos"].shape == (*res, 3) and a["nrm"].dtype == torch.float32 and 0.3 < cov.mean() < 0.8
    assert (index >= 0).float().mean() > 0.3
    for kw in PARAMS:
        for mode in ("weighted", "best"):
            got = projtex.project(**a, mode=mode, **kw)
            want = _want(a, views, mode=mode, **kw)
            _same(got, want, (res, n_views, mode, kw))
            count = got[2].cpu().numpy()
            assert not count[~cov].any() and count.max() == n_views and (count[cov] == 0).any()
            assert got[0].dtype == torch.float32 and got[1].dtype == torch.float32 and got[2].dtype == torch.uint8
    # the quad that faces away takes no colour; hidden texels of the first quad are seen by fewer views than its open ones
    vmax = obj.uvs[8:12, 1].max()
    y, x = np.mgrid[0:res[0], 0:res[1]]
    back = cov & (x / (res[1] - 1) > 0.5) & ((res[0] - 1 - y) / (res[0] - 1) < vmax + 0.02)
    assert back.sum() > 50 and not projtex.project(**a)[2].cpu().numpy()[back].any()


def test_exact_zeros_when_nothing_is_covered_or_seen():
    obj, views = S.three_quads(), S.three_views()
    a, _ = _setup(obj, views, (40, 56))
    for mode in ("weighted", "best"):
        out = projtex.project(**{**a, "coverage": torch.zeros_like(a["coverage"])}, mode=mode)
        assert all(not t.any() for t in out)
    away = np.stack([S.view([0.0, 0.0, 3.0], [0.0, 0.0, 6.0]), S.view([2.0, 0.0, 2.0], [5.0, 0.0, 2.0], roll=0.4)])
    b, index = _setup(obj, away, (40, 56))
    assert not (index >= 0).any()
    b["depth"] = torch.ones_like(b["depth"])                     # even with a depth map that hides nothing
    for mode in ("weighted", "best"):
        out = projtex.project(**b, mode=mode, cos_min=-1.0, power=0)
        assert all(not t.any() for t in out)
        _same(out, _want(b, away, mode=mode, cos_min=-1.0, power=0), mode)
    with pytest.raises(ValueError):
        projtex.project(**{**a, "photos": a["photos"][:2]})
    with pytest.raises(ValueError):
        projtex.project(**{**a, "depth": a["depth"].cpu()})


@pytest.mark.parametrize("res", SIZES)
def test_occlusion_equals_a_ray_cast(res):
    """S.occlusion_scene: the large quad lies inside the image, so nearly every covered texel projects into it, and more than 100
    of the compared texels are hidden behind the front quad (tests/test_projtex_host.py checks the same geometry on the host)"""
    obj, vw = S.occlusion_scene()
    a, index = _setup(obj, vw[None], res)
    assert ((index // 2) == 1).sum() > 150 and ((index // 2) == 0).sum() > 800 and (index >= 0).all()
    _, _, count = projtex.project(**a, power=0, cos_min=-1.0, fade_px=0.0)
    cov = a["coverage"].cpu().numpy() != 0
    seen, in_image, excluded = S.occlusion_truth(a["pos"].cpu().numpy().astype(np.float64)[cov], obj, vw)
    keep = ~excluded
    share = excluded.mean()
    got = count.cpu().numpy()[cov] > 0
    hidden = in_image & ~seen & keep
    print("covered", cov.sum(), "in the image", in_image.sum(), "excluded", excluded.sum(), "share", share, "hidden and compared",
          hidden.sum(), "seen and compared", (in_image & seen & keep).sum(), "disagree", (got != (seen & in_image))[keep].sum())
    assert share <= 0.10
    assert in_image.mean() > 0.99
    assert np.array_equal(got[keep], (seen & in_image)[keep])
    assert hidden.sum() > 100 and (in_image & seen & keep).sum() > 1000


@pytest.fixture(scope="module")
def patch():
    obj, verts = S.patch_scene()
    views = S.patch_views()
    h, w = 80, 96
    tex = S.smooth_texture(128, 128)
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, dev(tex), device=DEV)
    v = dev(verts.astype(np.float32))
    cams = (dev(views), h, w)
    photos, depth, index = r.render(v, cams, mapping="bilinear")
    pos, nrm, cov = projtex.surface_maps(obj, v, 128, device=DEV)
    return dict(obj=obj, v=v, cams=cams, photos=photos, depth=depth, index=index, pos=pos, nrm=nrm, cov=cov, tex=tex,
                faces=faces, uv_faces=uv_faces, views=views)


@pytest.mark.parametrize("mode", ["weighted", "best"])
def test_round_trip_through_the_mesh_renderer(patch, mode):
    from topo4d_amd import texfinish
    p = patch
    color, weight, count = projtex.project(p["pos"], p["nrm"], p["cov"], p["cams"], p["photos"], p["depth"], mode=mode)
    inner = (texfinish.erode(p["cov"], 2) != 0) & (count >= 1)
    err = (color.double() - dev(p["tex"]).double()).abs()[inner].max().item()
    print(mode, "texels", int(inner.sum()), "max error", err, "bound", 1.5 * ROUND_TRIP_F64)
    assert int(inner.sum()) > 8000
    assert err <= 1.5 * ROUND_TRIP_F64
    # the maps the kernel was fed against the float64 ones of the host
    pos64, nrm64, cov64 = S.patch_maps64(128)
    both = S.erode(cov64, 2) & (texfinish.erode(p["cov"], 2).cpu().numpy() != 0)
    assert both.sum() > 9000 and np.abs(p["pos"].cpu().numpy() - pos64)[both].max() < 1e-5
    # sanity ordering: rendered back into the three views, the projected texture is nearer the photographs than flat grey
    levels = texfinish.finish(texfinish.quantize(color), (count > 0).to(torch.uint8), pad=4)
    grey = torch.full_like(levels[128], 128)
    psnr = {}
    for name, tex in (("projected", levels[128]), ("grey", grey)):
        r = meshrender.MeshRenderer(p["faces"], p["uv_faces"], p["obj"].uvs, tex, device=DEV)
        image, _, index = r.render(p["v"], p["cams"])
        psnr[name] = meshrender.image_metrics(image, p["photos"], index)[:, 4].cpu().numpy()
    print(mode, psnr)
    assert (psnr["projected"] > psnr["grey"]).all()


@pytest.mark.parametrize("mode", ["weighted", "best"])
def test_project_frame_merges_views_of_two_image_sizes(mode):
    """a rig with turned cameras: project_frame projects each image size in one launch and merges them.  Against the yardstick
    per size, merged in float64: weighted sums add up, "best" keeps the larger weight and the earlier size on ties.  The merge
    itself runs in float32 and the result is quantised by truncation, so a texel may differ by one level."""
    from topo4d_amd import cameras as C
    from topo4d_amd.rasterizer import pack_views
    obj = S.three_quads()
    shots = [([0.9, 0.5, -2.6], [0.1, 0.0, 0.0], 40, 48, 44.0, 0.0), ([0.2, 0.3, -2.2], [0.0, 0.0, 0.0], 48, 40, 42.0, 1.2),
             ([-0.3, -0.2, -2.4], [0.0, 0.1, 0.0], 40, 48, 40.0, 0.6), ([0.1, -0.4, -2.5], [0.2, 0.0, 0.0], 48, 40, 40.0, -0.4)]
    rng = np.random.default_rng(5)
    dataset = []
    for eye, target, h, w, f, roll in shots:
        w2c, K = S.camera(eye, target, h, w, f, roll)
        dataset.append({"cam": C.setup_camera(None, w, h, K, w2c, device=DEV), "im": dev(rng.uniform(0, 1, size=(3, h, w)).astype(np.float32))})
    verts = dev(obj.vertices.astype(np.float32))
    opts = dict(power=2, cos_min=0.1, fade_px=4.0, depth_tol=0.01, mode=mode)
    tex, weight, count = projtex.project_frame(obj, verts, dataset, (40, 56), **opts)
    pos, nrm, cov = projtex.surface_maps(obj, verts, (40, 56), device=DEV)
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, np.zeros((1, 1, 3), np.uint8), device=DEV)
    parts = []
    for size in ((40, 48), (48, 40)):
        ks = [k for k, s in enumerate(shots) if (s[2], s[3]) == size]
        cams = [dataset[k]["cam"] for k in ks]
        depth = r.render(verts, cams)[1].cpu().numpy()
        photos = np.stack([dataset[k]["im"].cpu().numpy() for k in ks])
        views = pack_views(cams, torch.device(DEV, torch.cuda.current_device())).cpu().numpy()
        parts.append([x.astype(np.float64) for x in ref.project_texture(pos.cpu().numpy(), nrm.cpu().numpy(), cov.cpu().numpy(), views,
                                                                        *size, photos, depth, **opts)])
    (c0, w0, n0), (c1, w1, n1) = parts
    assert (n0 > 0).sum() > 100 and (n1 > 0).sum() > 100 and ((n0 > 0) & (n1 > 0)).sum() > 50
    if mode == "best":
        take = w1 > w0
        want_c, want_w = np.where(take[..., None], c1, c0), np.where(take, w1, w0)
    else:
        want_w = w0 + w1
        with np.errstate(all="ignore"):
            want_c = np.where((want_w > 0)[..., None], (c0 * w0[..., None] + c1 * w1[..., None]) / want_w[..., None], 0.0)
    assert np.array_equal(count.cpu().numpy(), (n0 + n1).astype(np.uint8))
    assert np.abs(weight.cpu().numpy() - want_w).max() <= 1e-6 * max(1.0, want_w.max())
    levels = np.floor(want_c * 255.0)
    assert np.abs(tex.cpu().numpy().astype(np.float64) - levels).max() <= 1
    assert (tex.cpu().numpy() == levels).mean() > 0.99


# ---- trees -----------------------------------------------------------------------------------------------------------------------
# At 192 x 256 a pixel spans about a hundredth of the head, so the depth under the four taps of an oblique surface differs from
# the texel's own by more than the default 0.2 %: the trees are projected with a slack that fits their image size.
TOL = ["--depth_tol", "0.02"]


def _train(dirs, out, *extra, frames="6", tex=True):
    from tests.test_setup_host import golden
    from topo4d_amd import train as T
    argv = ["-e", "exp", "-s", "seq", "-id", dirs["input_dir"], "-did", dirs["dense_input_dir"], "-od", out, "-fn", frames,
            "-tr", "64", "-dn", "2", "-dr", "4", "-ion", "12", "-on", "6", "-don", "3", "-lf", "1000", "-dlf", "1000"]
    T.train(T.build_parser().parse_args(argv + (["-t"] if tex else []) + list(extra)), facial_regions=golden()["facial_regions"], device=DEV)
    torch.cuda.synchronize()
    return os.path.join(out, "exp", "seq")


def _tree(run_dir):
    out = {}
    for d, _, names in os.walk(run_dir):
        for n in names:
            out[os.path.relpath(os.path.join(d, n), run_dir)] = open(os.path.join(d, n), "rb").read()
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    root = tmp_path_factory.mktemp("projtex_run")
    dirs = write_sequence(root, golden(), n_frames=3)
    plain = _train(dirs, str(root / "plain"))
    proj = _train(dirs, str(root / "proj"), "--tex_project", *TOL)
    return dict(root=root, dirs=dirs, plain=plain, proj=proj)


def _io(runs):
    return ["-e", "exp", "-s", "seq", "-id", runs["dirs"]["input_dir"], "-did", runs["dirs"]["dense_input_dir"], "-dr", "4"]


def test_train_with_the_flag_adds_one_file_per_frame_and_changes_nothing_else(runs):
    plain, proj = _tree(runs["plain"]), _tree(runs["proj"])
    keys = ["000001", "000002", "000003"]
    assert sorted(set(proj) - set(plain)) == [os.path.join(k, "face_proj.png") for k in keys] and not set(plain) - set(proj)
    for name, data in plain.items():
        if name.endswith(".npz"):                                # (a zip archive carries the time it was written)
            a, b = np.load(os.path.join(runs["plain"], name)), np.load(os.path.join(runs["proj"], name))
            assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files)
        else:
            assert proj[name] == data, name
    assert any(n.endswith("face.png") for n in plain) and not any("face_proj" in n for n in plain)


def test_the_command_writes_what_project_frame_returns_and_what_train_wrote(runs, tmp_path):
    from PIL import Image
    from topo4d_amd import cameras as C, evaluate as E, ingest
    out = str(tmp_path / "out")
    shutil.copytree(os.path.dirname(os.path.dirname(runs["plain"])), out)
    run_dir = os.path.join(out, "exp", "seq")
    before = _tree(run_dir)
    projtex.main(_io(runs) + ["-od", out, "--tex_res", "64", "--save_weight"] + TOL)
    after = _tree(run_dir)
    keys = ["000001", "000002", "000003"]
    assert sorted(set(after) - set(before)) == sorted(os.path.join(k, n) for k in keys for n in ("face_proj.png", "face_proj_weight.png"))
    assert all(after[n] == before[n] for n in before)
    cams, _, trans_g = C.get_cameras(runs["dirs"]["input_dir"], "seq", resize_factor=1)
    for key in keys:
        d = os.path.join(run_dir, key)
        assert after[os.path.join(key, "face_proj.png")] == open(os.path.join(runs["proj"], key, "face_proj.png"), "rb").read()
        png = np.asarray(Image.open(os.path.join(d, "face_proj.png")))
        assert png.shape == (64, 64, 3) and png.dtype == np.uint8
        obj = meshrender.read_face_obj(os.path.join(d, "face.obj"))
        ds = ingest.get_dataset(runs["dirs"]["dense_input_dir"], "seq", int(key), cams, use_mask=False, blacklist=C.BLACKLIST,
                                rotate_mask=C.ROTATE_MASK, setup_camera=C.setup_camera, device=DEV)
        verts = torch.from_numpy(E.training_vertices(obj.vertices, trans_g)).to(DEV)
        tex, weight, count = projtex.project_frame(obj, verts, ds, 64, depth_tol=0.02)
        assert np.array_equal(png, tex.cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(os.path.join(d, "face_proj_weight.png"))), count.cpu().numpy())
        print(key, "texels with a view", float((count > 0).float().mean()))
        assert (count > 0).any() and png[(count > 0).cpu().numpy()].any() and not png[(count == 0).cpu().numpy()].any()
        assert torch.equal(weight > 0, count > 0)
    # other sizes, a gutter and a smaller level, one frame, the best view
    projtex.main(_io(runs) + ["-od", out, "--tex_res", "128", "--tex_pad", "2", "--tex_sizes", "64", "--frames", "2", "--mode", "best"])
    d = os.path.join(run_dir, "000002")
    assert np.asarray(Image.open(os.path.join(d, "face_proj.png"))).shape == (128, 128, 3)
    assert np.asarray(Image.open(os.path.join(d, "face_proj_64.png"))).shape == (64, 64, 3)
    assert _tree(run_dir)[os.path.join("000001", "face_proj.png")] == after[os.path.join("000001", "face_proj.png")]
    with pytest.raises(SystemExit):
        projtex.main(_io(runs) + ["-od", out, "--tex_res", "64", "--power", "9"])


def test_train_without_the_texture_loop_writes_the_same_projection(runs):
    run_dir = _train(runs["dirs"], str(runs["root"] / "geometry_only"), "--tex_project", *TOL, frames="1", tex=False)
    names = os.listdir(os.path.join(run_dir, "000001"))
    assert "face.obj" in names and "face_proj.png" in names and "face.png" not in names
    with open(os.path.join(run_dir, "000001", "face_proj.png"), "rb") as f, open(os.path.join(runs["proj"], "000001", "face_proj.png"), "rb") as g:
        assert f.read() == g.read()


def test_evaluate_scores_the_projected_texture(runs, tmp_path):
    from topo4d_amd import evaluate as E
    out = str(tmp_path / "out")
    shutil.copytree(os.path.dirname(os.path.dirname(runs["proj"])), out)
    path = os.path.join(out, "exp", "seq", "eval.json")
    E.main(_io(runs) + ["-od", out])
    plain = open(path, "rb").read()
    assert "texture_file" not in json.loads(plain)
    E.main(_io(runs) + ["-od", out, "--texture", "face_proj.png"])
    res = json.load(open(path))
    assert res["texture_file"] == "face_proj.png"
    base = json.loads(plain)
    for key, fr in res["low"]["frames"].items():
        assert fr["texture"] is True
        for name, row in fr["views"].items():
            assert all(np.isfinite(row[n]) for n in ("l1", "mse", "psnr", "ssim", "psnr_full")), (key, name, row)
            assert row["count"] == base["low"]["frames"][key]["views"][name]["count"]
        assert fr["views"] != base["low"]["frames"][key]["views"]
    E.main(_io(runs) + ["-od", out])
    assert open(path, "rb").read() == plain                      # the default output is what it was
    E.main(_io(runs) + ["-od", out, "--texture", "missing.png"])
    assert all(fr["texture"] is False for fr in json.load(open(path))["low"]["frames"].values())
