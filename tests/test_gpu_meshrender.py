"""GPU: topo4d_amd.meshrender (csrc/t4d_meshrender.hip) against its float64 yardstick tests/meshrender_ref.py bit for bit, its
determinism, texture placement against a ray cast, alignment with the splat renderer, the metrics against a float64 torch
restatement, and topo4d_amd.evaluate end to end on a run of topo4d_amd.train over tests/capture_scene.py's sequence."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import meshrender_ref as ref
from tests.test_meshrender_host import _ray_cast, _random_mesh, look_at_view
from topo4d_amd import meshrender

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu_render(verts, tris, uv_tris, uvs, tex, views, H, W, bg=(0.0, 0.0, 0.0), mapping="bilinear"):
    r = meshrender.MeshRenderer(tris, uv_tris, uvs, torch.from_numpy(np.ascontiguousarray(tex)), device=DEV)
    vt = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(DEV)
    packed = torch.from_numpy(np.stack(views).astype(np.float32)).to(DEV)
    img, depth, idx = r.render(vt, (packed, H, W), bg=bg, mapping=mapping)
    return img.cpu().numpy(), depth.cpu().numpy(), idx.cpu().numpy()


def _texture(rng, dtype, h=37, w=29):
    if dtype == "uint8":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return rng.uniform(0, 1, size=(h, w, 3)).astype(np.float32)


def _scene(kind, rng):
    if kind == "random":
        verts, tris, uvs = _random_mesh(rng, 40, scale=0.5)
    elif kind == "overlap":                                # many triangles stacked over one another
        verts, tris, uvs = _random_mesh(rng, 60, spread=0.15, scale=0.6)
    elif kind == "ties":                                   # each triangle twice (and once more with its corners rotated): depth ties
        verts, tris, uvs = _random_mesh(rng, 20, scale=0.5)
        n = len(uvs)
        uvs = np.concatenate([uvs, rng.uniform(0, 1, size=uvs.shape).astype(np.float32)])
        all_tris = np.concatenate([tris, tris[::-1], tris[:, [1, 2, 0]]])
        uv_tris = np.concatenate([tris, tris[::-1] + n, tris[:, [1, 2, 0]] + n])
        return verts, all_tris, uv_tris, uvs
    elif kind == "clipped":                                # partly off screen and behind the near plane
        verts, tris, uvs = _random_mesh(rng, 40, spread=2.5, scale=1.2)
        verts[:, 2] -= 1.0
    elif kind == "degenerate":                             # zero-area triangles (repeated corners, collinear corners) among others
        verts, tris, uvs = _random_mesh(rng, 30, scale=0.5)
        tris = tris.copy()
        tris[::4, 1] = tris[::4, 0]
        verts = verts.copy()
        verts[tris[1::4, 2]] = 0.5 * (verts[tris[1::4, 0]] + verts[tris[1::4, 1]])
    return verts, tris, tris, uvs


SIZES = [(5, 7), (48, 64), (61, 83)]


@pytest.mark.parametrize("kind", ["random", "overlap", "ties", "clipped", "degenerate"])
@pytest.mark.parametrize("tex_dtype", ["uint8", "float32"])
@pytest.mark.parametrize("mapping", ["bilinear", "nearest"])
def test_bit_equal_to_the_yardstick(kind, tex_dtype, mapping):
    rng = np.random.default_rng(hash((kind, tex_dtype, mapping)) % 2 ** 32)
    verts, tris, uv_tris, uvs = _scene(kind, rng)
    tex = _texture(rng, tex_dtype)
    for H, W in SIZES:
        views = [look_at_view([0.4 * np.sin(a), 0.3, -2.2 * np.cos(a)], [0, 0, 0], H, W, f=0.9 * max(H, W)) for a in (0.0, 0.7, -1.1)]
        bg = (0.25, 0.5, 1.0)
        img, depth, idx = _gpu_render(verts, tris, uv_tris, uvs, tex, views, H, W, bg=bg, mapping=mapping)
        for v, view in enumerate(views):
            c, d, i = ref.render(verts, tris, uv_tris, uvs, tex, view, H, W, bg=bg, mapping=mapping)
            assert np.array_equal(i, idx[v]), (kind, H, W, v, (i != idx[v]).sum())
            assert np.array_equal(d.view(np.uint32), depth[v].view(np.uint32)), (kind, H, W, v)
            assert np.array_equal(c.view(np.uint32), img[v].view(np.uint32)), (kind, H, W, v, np.abs(c - img[v]).max())
        assert (idx >= 0).any()


def test_bit_equal_at_full_capture_size():
    rng = np.random.default_rng(11)
    H, W = 3008, 4096
    verts, tris, uvs = _random_mesh(rng, 10, scale=0.7)
    tex = _texture(rng, "uint8", 64, 64)
    views = [look_at_view([0.2, 0.1, -2.5], [0, 0, 0], H, W, f=0.9 * W), look_at_view([-0.6, 0.2, -2.4], [0, 0, 0], H, W, f=0.8 * W)]
    img, depth, idx = _gpu_render(verts, tris, tris, uvs, tex, views, H, W)
    for v, view in enumerate(views):
        c, d, i = ref.render(verts, tris, tris, uvs, tex, view, H, W)
        assert np.array_equal(i, idx[v])
        assert np.array_equal(d.view(np.uint32), depth[v].view(np.uint32))
        assert np.array_equal(c.view(np.uint32), img[v].view(np.uint32))
    assert (idx >= 0).mean() > 0.05


@pytest.mark.parametrize("H,W", [pytest.param(512, 512, id="1024_bins_one_full_chunk_no_chunk_sums"),
                                 pytest.param(512, 528, id="1056_bins_partial_last_chunk_of_two")])
def test_bit_equal_at_the_bin_scan_chunk_edge(H, W):
    """One view of exactly one scan chunk of 16 x 16 tiles, and of one chunk and 32 bins: the sizes above (at most 72 bins, and
    94 full chunks at capture size) have neither a full single chunk nor a last chunk that is partly beyond the bins.  The last
    triangle covers the view's last tile, so the last bin's offset is read."""
    rng = np.random.default_rng(W)
    verts, tris, uvs = _random_mesh(rng, 12, scale=0.7)
    verts = np.concatenate([verts, np.float32([[-9, -9, 2], [9, -9, 2], [0, 18, 2]])])      # a backdrop over the whole view
    tris = np.concatenate([tris, [[36, 37, 38]]])
    uvs = np.concatenate([uvs, np.float32([[0, 0], [1, 0], [0.5, 1]])])
    tex = _texture(rng, "uint8", 64, 64)
    view = look_at_view([0.2, 0.1, -2.5], [0, 0, 0], H, W, f=0.9 * W)
    img, depth, idx = _gpu_render(verts, tris, tris, uvs, tex, [view], H, W)
    c, d, i = ref.render(verts, tris, tris, uvs, tex, view, H, W)
    assert (i[-16:, -16:] >= 0).any() and (i[:16, :16] >= 0).any()
    assert np.array_equal(i, idx[0])
    assert np.array_equal(d.view(np.uint32), depth[0].view(np.uint32))
    assert np.array_equal(c.view(np.uint32), img[0].view(np.uint32))


def test_identical_bytes_over_repeated_launches_with_dirty_scratch():
    rng = np.random.default_rng(3)
    verts, tris, uvs = _random_mesh(rng, 300, spread=0.3, scale=0.4)
    H, W = 200, 300
    tex = torch.from_numpy(_texture(rng, "uint8", 128, 128))
    r = meshrender.MeshRenderer(tris, tris, uvs, tex, device=DEV)
    vt = torch.from_numpy(verts).to(DEV)
    packed = torch.from_numpy(np.stack([look_at_view([0.1 * k, 0, -2.0], [0, 0, 0], H, W, f=300.0) for k in range(4)])).to(DEV)
    first = [t.clone() for t in r.render(vt, (packed, H, W))]
    for k in range(3):
        r._scratch.random_(0, 256)                           # every byte the kernels read must be written first
        again = r.render(vt, (packed, H, W))
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_texture_placement_equals_ray_cast_uvs():
    """a linear ramp texture (bilinear sampling reproduces it) turns the rendered colours into the UVs"""
    rng = np.random.default_rng(7)
    H, W = 23, 31
    verts, tris, uvs = _random_mesh(rng, 24, scale=0.8)
    th, tw = 65, 129
    ys, xs = np.mgrid[0:th, 0:tw]
    tex = np.stack([xs / (tw - 1.0), (th - 1.0 - ys) / (th - 1.0), np.full(xs.shape, 0.5)], -1).astype(np.float32)
    view = look_at_view([0.3, -0.2, -2.0], [0, 0, 0], H, W, f=0.9 * W)
    img, _, idx = _gpu_render(verts, tris, tris, uvs, tex, [view], H, W)
    face_rc, _, uv_rc = _ray_cast(verts, tris, uvs[tris].astype(np.float64), view, H, W)
    same = (idx[0] == face_rc) & (face_rc >= 0)
    assert same.sum() > 0.2 * H * W and (idx[0] == face_rc).mean() > 0.97
    assert np.abs(img[0, 0][same] - uv_rc[..., 0][same]).max() < 2e-6
    assert np.abs(img[0, 1][same] - uv_rc[..., 1][same]).max() < 2e-6


def test_mesh_vertex_lines_up_with_the_splat_renderer():
    """one small opaque Gaussian at a mesh vertex renders centred on the pixel where the mesh renderer projects that vertex"""
    from topo4d_amd import cameras as C
    from topo4d_amd.rasterizer import GaussianRasterizer, pack_views
    H, W = 96, 128
    K = np.array([[110.0, 0, 61.3], [0, 108.0, 50.2], [0, 0, 1]])
    w2c = np.eye(4)
    ang = 0.3
    w2c[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
    w2c[:3, 3] = [0.1, -0.05, 2.5]
    cam = C.setup_camera(None, W, H, K, w2c, near=0.01, far=100, device=DEV)
    vertex = np.array([[0.13, -0.07, 0.2], [0.5, 0.5, 0.5], [0.4, 0.1, 0.3]], np.float32)
    view = pack_views([cam], torch.device(DEV))[0].cpu().numpy()
    px, py, _ = ref.project(vertex, view, H, W)
    # (ref.project is the mesh renderer's projection: the bit-equality tests above pin one to the other)
    mean = torch.from_numpy(vertex[:1]).to(DEV)
    rv = dict(means3D=mean, means2D=torch.zeros_like(mean), opacities=torch.ones(1, 1, device=DEV),
              scales=torch.full((1, 3), 0.04, device=DEV), rotations=torch.tensor([[1.0, 0, 0, 0]], device=DEV),
              colors_precomp=torch.ones(1, 3, device=DEV))
    im = GaussianRasterizer(raster_settings=cam)(**rv)[0][0].cpu().double().numpy()
    ys, xs = np.mgrid[0:H, 0:W]
    cx, cy = (im * xs).sum() / im.sum(), (im * ys).sum() / im.sum()
    assert abs(cx - px[0]) < 0.05 and abs(cy - py[0]) < 0.05, (cx, cy, px[0], py[0])
    assert 0.5 < im.max() and im.sum() > 3.0


def test_metrics_equal_the_float64_restatement():
    from topo4d_amd.progress import calc_psnr
    g = torch.Generator().manual_seed(4)
    V, H, W = 3, 37, 53
    target = torch.rand(V, 3, H, W, generator=g)
    render = (target + 0.1 * torch.randn(V, 3, H, W, generator=g)).clamp(0, 1)
    render[1, :, 5:20, 7:30] = target[1, :, 5:20, 7:30]               # a region of equal pixels
    cov = torch.randint(-1, 50, (V, H, W), generator=g, dtype=torch.int32)
    mask = (torch.rand(V, 1, H, W, generator=g) > 0.3).float()
    r, t, c, m = render.to(DEV), target.to(DEV), cov.to(DEV), mask.to(DEV)
    for cc, mm in ((c, m), (c, None), (None, None)):
        got = meshrender.image_metrics(r, t, cc, mm).cpu()
        want = ref.metrics_f64(render, target, None if cc is None else cov, None if mm is None else mask)
        assert torch.equal(got[:, 1], want[:, 1])
        for q in (2, 3):
            assert ((got[:, q] - want[:, q]).abs() <= 1e-9 * want[:, q].abs()).all(), (q, got[:, q], want[:, q])
        assert ((got[:, 4] - want[:, 4]).abs() < 1e-7).all()
        assert ((got[:, 5] - want[:, 5]).abs() < 2e-5).all(), (got[:, 5], want[:, 5])
        assert ((got[:, 0] - want[:, 0]).abs() < 1e-7).all()
        for v in range(V):
            assert abs(float(got[v, 0]) - float(calc_psnr(r[v], t[v]).mean())) < 1e-5


def test_argument_errors():
    with pytest.raises(ValueError):
        meshrender.MeshRenderer(np.array([[0, 1, 2]]), np.array([[0, 1, 3]]), np.zeros((3, 2)), np.zeros((2, 2, 3), np.uint8), device=DEV)
    with pytest.raises(ValueError):
        meshrender.MeshRenderer(np.array([[0, 1, 2]]), np.array([[0, 1, 2]]), np.zeros((3, 2)), np.zeros((2, 2, 4), np.uint8), device=DEV)
    r = meshrender.MeshRenderer(np.array([[0, 1, 2]]), np.array([[0, 1, 2]]), np.zeros((3, 2)), np.zeros((2, 2, 3), np.uint8), device=DEV)
    views = torch.zeros(1, 40, device=DEV)
    with pytest.raises(ValueError):
        r.render(torch.zeros(2, 3, device=DEV), (views, 8, 8))            # vertex 2 missing
    with pytest.raises(ValueError):
        r.render(torch.zeros(3, 3, device=DEV), (views, 8, 8), mapping="cubic")
    with pytest.raises(ValueError):
        meshrender.image_metrics(torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 3, 4, 5, device=DEV))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    from topo4d_amd import train as T
    g = golden()
    root = tmp_path_factory.mktemp("meshrender_run")
    dirs = write_sequence(root, g, n_frames=2)
    argv = ["-e", "exp", "-s", "seq", "-id", dirs["input_dir"], "-did", dirs["dense_input_dir"], "-od", str(root / "out"), "-fn", "2",
            "-t", "-tr", "256", "-dn", "2", "-dr", "4", "-ion", "30", "-on", "20", "-don", "5", "-lf", "1000", "-dlf", "1000"]
    first = {}
    T.train(T.build_parser().parse_args(argv), facial_regions=g["facial_regions"], device=torch.device(DEV),
            on_frame=lambda t, s: first.setdefault("means3D", s["params"]["means3D"].detach().clone()) if t == 0 else None)
    torch.cuda.synchronize()
    return dict(root=root, dirs=dirs, out=str(root / "out"), run_dir=str(root / "out" / "exp" / "seq"), means3D=first["means3D"])


def _eval(run, *extra, input_dir=None, out=None):
    from topo4d_amd import evaluate as E
    argv = ["-e", "exp", "-s", "seq", "-id", input_dir or run["dirs"]["input_dir"], "-did", run["dirs"]["dense_input_dir"],
            "-od", out or run["out"], "-dr", "4"] + list(extra)
    E.main(argv)
    with open(os.path.join(out or run["out"], "exp", "seq", "eval.json")) as f:
        return json.load(f)


def test_cli_numbers_equal_a_torch_recomputation(run):
    from PIL import Image
    from topo4d_amd import cameras as C, evaluate as E, ingest
    res = _eval(run, "--save_renders", "--set", "both")
    for which in ("low", "dense"):
        frames = res[which]["frames"]
        assert sorted(frames) == ["000001", "000002"]
        data_dir = run["dirs"]["input_dir"] if which == "low" else run["dirs"]["dense_input_dir"]
        cams, _, trans_g = C.get_cameras(run["dirs"]["input_dir"], "seq", resize_factor=4 if which == "low" else 1)
        for key, fr in frames.items():
            t = int(key)
            assert fr["texture"] is True and fr["masked"] is (which == "low")
            obj = meshrender.read_face_obj(os.path.join(run["run_dir"], key, "face.obj"))
            tex = np.array(Image.open(os.path.join(run["run_dir"], key, "face.png")).convert("RGB"))
            faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
            r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, tex, device=DEV)
            verts = torch.from_numpy(E.training_vertices(obj.vertices, trans_g)).to(DEV)
            ds = ingest.get_dataset(data_dir, "seq", t, cams, use_mask=which == "low", rotate_mask=C.ROTATE_MASK,
                                    setup_camera=C.setup_camera, device=DEV)
            img, _, idx = r.render(verts, [e["cam"] for e in ds])
            target = torch.stack([e["im"] for e in ds]).float()
            masks = E.pixel_masks(ds)
            want = ref.metrics_f64(img.cpu(), target.cpu(), idx.cpu(), None if masks is None else masks.cpu())
            assert sorted(fr["views"]) == sorted(e["cam_name"] for e in ds)
            for v, e in enumerate(ds):
                row = fr["views"][e["cam_name"]]
                assert row["trained"] is True and row["covered"] == int((idx[v] >= 0).sum())
                assert row["count"] == int(want[v, 1]) and row["count"] > 0, (which, key, e["cam_name"], row, fr["views"])
                assert abs(row["l1"] - float(want[v, 2])) <= 1e-9 * float(want[v, 2])
                assert abs(row["mse"] - float(want[v, 3])) <= 1e-9 * float(want[v, 3])
                assert abs(row["psnr"] - float(want[v, 4])) < 1e-7
                assert abs(row["ssim"] - float(want[v, 5])) < 2e-5
                assert abs(row["psnr_full"] - float(want[v, 0])) < 1e-7
                png = np.array(Image.open(os.path.join(run["run_dir"], key, f"mesh_{which}_{e['cam_name']}.png")))
                q = (img[v].mul(255).add(0.5).clamp(0, 255).to(torch.uint8)).permute(1, 2, 0).cpu().numpy()
                assert np.array_equal(png, q)
        assert res[which]["summary"]["frames"] == 2


def test_missing_texture_and_mesh_are_recorded(run, tmp_path):
    out = tmp_path / "out"
    shutil.copytree(run["out"], out)
    os.remove(out / "exp" / "seq" / "000002" / "face.png")
    os.remove(out / "exp" / "seq" / "000001" / "face.obj")
    res = _eval(run, out=str(out))
    assert res["low"]["frames"]["000001"] == {"skipped": "no face.obj"}
    assert res["low"]["frames"]["000002"]["texture"] is False
    assert all(r["count"] > 0 for r in res["low"]["frames"]["000002"]["views"].values())


def test_self_consistency_with_renders_as_views(run, tmp_path):
    """frame 1's views replaced by PNG renders of that frame's own state (means3D, face.png), un-rotated: the masked L1 over covered
    pixels stays below the uint8 quantisation bound - trans_g, the view rotations and the UV convention agree"""
    from PIL import Image
    from topo4d_amd import cameras as C
    src = run["dirs"]["input_dir"]
    dst = str(tmp_path / "low")
    shutil.copytree(src, dst)
    cams, _, _ = C.get_cameras(src, "seq", resize_factor=4)
    obj = meshrender.read_face_obj(os.path.join(run["run_dir"], "000001", "face.obj"))
    tex = np.array(Image.open(os.path.join(run["run_dir"], "000001", "face.png")).convert("RGB"))
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, tex, device=DEV)
    fdir = os.path.join(dst, "seq", "000001")
    for fname, cam in cams.items():
        name = fname.split(".")[0]
        w, h, k, w2c = cam["image_size"][1], cam["image_size"][0], cam["intrinsics"], cam["extrinsics"]
        settings = C.setup_camera(cam, w, h, k, np.concatenate([w2c, [[0, 0, 0, 1]]]), device=DEV)
        img, _, _ = r.render(run["means3D"], [settings])
        q = img[0].mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        os.remove(os.path.join(fdir, fname))
        Image.fromarray(np.ascontiguousarray(np.rot90(q, -C.ROTATE_MASK[name]))).save(os.path.join(fdir, name + ".png"))
    res = _eval(run, "--frames", "1", input_dir=dst, out=str(run["out"]))
    views = res["low"]["frames"]["000001"]["views"]
    assert len(views) == len(cams)
    for name, row in views.items():
        assert row["count"] > 100, name
        assert row["l1"] < 0.5 / 255, (name, row["l1"])
