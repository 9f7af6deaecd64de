"""GPU: texture finishing (topo4d_amd/texfinish.py, csrc/t4d_texfinish.hip) bit for bit against the brute force of
tests/texfinish_ref.py on shapes that break a tiled kernel; write_texture / save_mesh / train / evaluate / the texfinish command with
the new options, and byte-identical files without them; the seam property the feature exists for; one full-size run."""
import functools
import json
import os
import shutil
import time

import numpy as np
import pytest
import torch

from tests import texfinish_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SHAPES = [(67, 93), (130, 150)]
DENSITIES = [0.05, 0.6]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                   # a copy: the cached masks are read-only


@functools.lru_cache(maxsize=None)
def mask(h, w, density):
    """Seeded random coverage with: an empty block wider than 2 * 16 + a 1-texel line in it (an island thinner than any radius),
    so that texels in the block stay unfilled; a lone covered texel in each image corner."""
    rng = np.random.default_rng(1000 * h + w + int(100 * density))
    c = rng.uniform(size=(h, w)) < density
    c[8:58, 20:75] = False
    c[12, 24:40] = True
    for ys, xs, y, x in ((slice(0, 4), slice(0, 4), 0, 0), (slice(0, 4), slice(w - 4, w), 0, w - 1),
                         (slice(h - 4, h), slice(0, 4), h - 1, 0), (slice(h - 4, h), slice(w - 4, w), h - 1, w - 1)):
        c[ys, xs] = False
        c[y, x] = True
    c = c.astype(np.uint8)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def pad_source(h, w, density, R):
    """(flat source texel of every texel, output coverage) by the brute force, shared by the channel counts"""
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    src, cov = ref.pad(idx, mask(h, w, density), R)
    return src.reshape(-1), cov


def image(h, w, c, seed=0):
    img = np.random.default_rng(seed).integers(1, 256, size=(h, w, c), dtype=np.uint8)
    return img[..., 0] if c == 1 else img


# ---- pad -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 1, 5, 16])
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_pad_equals_the_brute_force(shape, density, R):
    from topo4d_amd import texfinish
    h, w = shape
    cov = mask(h, w, density)
    src, want_cov = pad_source(h, w, density, R)
    assert (want_cov == 0).any() and want_cov[0, 0] == 1          # the block keeps unfilled texels at every radius
    for c in (1, 3, 4):
        img = image(h, w, c, seed=c)
        # uncovered texels hold values of their own: an unfilled texel must keep its input, not turn black
        got, got_cov = texfinish.pad(dev(img), dev(cov), R)
        want = img.reshape(h * w, -1)[src].reshape(img.shape)
        np.testing.assert_array_equal(got_cov.cpu().numpy(), want_cov)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        if R == 0:
            np.testing.assert_array_equal(got.cpu().numpy(), img)
            np.testing.assert_array_equal(got_cov.cpu().numpy(), cov)
        again, again_cov = texfinish.pad(dev(img), dev(cov), R)
        assert torch.equal(again, got) and torch.equal(again_cov, got_cov)


def test_pad_radius_64_from_a_single_texel():
    """the int8 offsets at their extremes (+-64 and the 'none' value), a radius beyond half the image"""
    from topo4d_amd import texfinish
    for at in ((20, 70), (95, 0), (0, 95)):
        cov = np.zeros((96, 96), np.uint8)
        cov[at] = 1
        img = image(96, 96, 3, seed=5)
        want, want_cov = ref.pad(img, cov, 64)
        got, got_cov = texfinish.pad(dev(img), dev(cov), 64)
        np.testing.assert_array_equal(got_cov.cpu().numpy(), want_cov)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        ys, xs = np.mgrid[0:96, 0:96]
        np.testing.assert_array_equal(want_cov, ((ys - at[0]) ** 2 + (xs - at[1]) ** 2 <= 64 * 64).astype(np.uint8))
        assert (want_cov == 0).any() and int(want_cov.sum()) > 1


@pytest.mark.parametrize("R", [16, 64])
def test_pad_across_row_segments(R):
    """rows longer than the 256 texels one workgroup of the row pass stages: offsets that reach into the neighbouring segments"""
    from topo4d_amd import texfinish
    h, w = 9, 700
    rng = np.random.default_rng(R)
    cov = (rng.uniform(size=(h, w)) < 0.004).astype(np.uint8)
    cov[:, 100:420] = 0                                            # a gap over the first segment border, wider than 4 * 64
    cov[4, 255], cov[2, 512], cov[7, 511], cov[0, 699] = 1, 1, 1, 1
    img = image(h, w, 3, seed=R)
    want, want_cov = ref.pad(img, cov, R)
    got, got_cov = texfinish.pad(dev(img), dev(cov), R)
    np.testing.assert_array_equal(got_cov.cpu().numpy(), want_cov)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert want_cov[4, 170] == 0 and want_cov[4, 255 + R] == 1 and want_cov[4, 255 - R] == 1 and want_cov[4, 256 + R] == 0


@pytest.mark.parametrize("R", [0, 7, 64])
def test_pad_all_covered_and_none_covered_are_no_ops(R):
    from topo4d_amd import texfinish
    img = image(67, 93, 3, seed=2)
    for value in (0, 1, 255):
        cov = np.full((67, 93), value, np.uint8)
        got, got_cov = texfinish.pad(dev(img), dev(cov), R)
        np.testing.assert_array_equal(got.cpu().numpy(), img)
        np.testing.assert_array_equal(got_cov.cpu().numpy(), (cov != 0).astype(np.uint8))


# ---- erode, halve, coverage, quantize -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [0, 1, 2, 3, 4])
def test_erode_equals_the_brute_force(E):
    from topo4d_amd import texfinish
    masks = [mask(h, w, d) for h, w in SHAPES for d in DENSITIES]
    rng = np.random.default_rng(3)
    for h, w in SHAPES + [(16, 64), (17, 65), (1, 1), (1, 200), (200, 1)]:
        full = np.ones((h, w), np.uint8) * 255                     # touches every image edge: the edges must not erode
        holes = rng.uniform(size=(h, w)) < 0.004
        full[holes] = 0
        masks.append(full)
        masks.append((rng.uniform(size=(h, w)) < 0.97).astype(np.uint8))
    for m in masks:
        got = texfinish.erode(dev(m), E).cpu().numpy()
        np.testing.assert_array_equal(got, ref.erode(m, E))
    ones = np.ones((67, 93), np.uint8)
    np.testing.assert_array_equal(texfinish.erode(dev(ones), E).cpu().numpy(), ones)


def test_halve_equals_the_brute_force():
    from topo4d_amd import texfinish
    h, w = 66, 94
    rng = np.random.default_rng(4)
    pattern = np.zeros((h, w), np.uint8)                           # block (by, bx) holds subset (by * 47 + bx) % 16 of its 2x2 texels
    sub = (np.arange(h // 2)[:, None] * (w // 2) + np.arange(w // 2)[None, :]) % 16
    for k in range(4):
        pattern[(k >> 1)::2, (k & 1)::2] = (sub >> k) & 1
    counts = pattern.reshape(h // 2, 2, w // 2, 2).sum((1, 3))
    assert sorted(np.unique(counts)) == [0, 1, 2, 3, 4]
    for cov in (pattern, (rng.uniform(size=(h, w)) < 0.5).astype(np.uint8) * 7, np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)):
        for c in (1, 3, 4):
            img = image(h, w, c, seed=10 + c)
            got, got_cov = texfinish.halve(dev(img), dev(cov))
            want, want_cov = ref.halve(img, cov)
            assert tuple(got.shape) == want.shape == ((33, 47) if c == 1 else (33, 47, c))
            np.testing.assert_array_equal(got.cpu().numpy(), want)
            np.testing.assert_array_equal(got_cov.cpu().numpy(), want_cov)
    with pytest.raises(ValueError):
        texfinish.halve(dev(image(67, 94, 3)), dev(np.ones((67, 94), np.uint8)))


def two_islands(h=64, w=48):
    """two quads in pixel space (x, y, 0), apart from each other and from the image border"""
    quads = [((5.3, 6.2), (20.7, 4.9), (22.1, 30.4), (4.2, 28.8)), ((27.6, 35.1), (43.2, 33.7), (41.9, 58.3), (26.4, 57.2))]
    verts = np.array([[x * w / 48.0, y * h / 64.0, 0.0] for q in quads for x, y in q], np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    return verts, tris


def test_coverage_is_the_depth_test_of_a_bake():
    from topo4d_amd import texfinish, texture
    verts, tris = two_islands()
    colors = np.random.default_rng(0).uniform(0.2, 1, size=(8, 3)).astype(np.float32)
    img, depth = texture.render_colors(verts, tris, colors, 64, 48, return_depth=True)
    cov = texfinish.coverage_from_depth(depth)
    want = depth.cpu().numpy() > -999999
    assert cov.dtype == torch.uint8 and tuple(cov.shape) == (64, 48)
    np.testing.assert_array_equal(cov.cpu().numpy(), want.astype(np.uint8))
    assert 0 < want.sum() < want.size and (img.cpu().numpy()[~want] == 0).all()
    d = torch.full((5, 7), -999999.0, device=DEV)                  # 35 values: the four-at-a-time kernel and its tail
    d[2, 3], d[4, 6], d[0, 0] = 0.0, -999998.9, float("nan")
    np.testing.assert_array_equal(texfinish.coverage_from_depth(d).cpu().numpy(), ref.coverage_from_depth(d.cpu().numpy()))
    off = torch.full((36,), -999999.0, device=DEV)
    off[1::3] = 1.0
    view = off[1:].view(5, 7)                                      # not 16-byte aligned: the scalar kernel alone
    np.testing.assert_array_equal(texfinish.coverage_from_depth(view).cpu().numpy(), ref.coverage_from_depth(view.cpu().numpy()))


def test_quantize_is_numpys_cast():
    from topo4d_amd import texfinish
    k = np.arange(256, dtype=np.float64) / 255.0
    base = k.astype(np.float32)
    vals = np.concatenate([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-1)),
                           (k * (1 + 2e-7)).astype(np.float32), np.float32([0.0, 1.0, -0.0, -1e-8, -0.003, 1.003, 1.0000001, 0.9999999,
                                                                             0.5, 1 / 3, 254.5 / 255, 255.5 / 255])])
    n = 7 * 50 * 3                                                 # 1050 values: four at a time, and a tail of two
    x = np.resize(vals, n + 1).astype(np.float32)
    want = (x * 255).astype(np.uint8)
    t = dev(x)
    got = texfinish.quantize(t[:n].view(7, 50, 3))
    np.testing.assert_array_equal(got.cpu().numpy(), want[:n].reshape(7, 50, 3))
    got = texfinish.quantize(t[1:].view(7, 50, 3))                 # a pointer that is not 16-byte aligned
    np.testing.assert_array_equal(got.cpu().numpy(), want[1:].reshape(7, 50, 3))
    got = texfinish.quantize(t[:n].view(21, 50))
    np.testing.assert_array_equal(got.cpu().numpy(), want[:n].reshape(21, 50))
    assert len(np.unique(want)) == 256


def test_finish_equals_the_brute_force():
    from topo4d_amd import texfinish
    rng = np.random.default_rng(6)
    h, w = 96, 160
    img = image(h, w, 3, seed=6)
    cov = np.zeros((h, w), np.uint8)
    cov[10:50, 12:70] = 1
    cov[30:90, 100:150] = 1
    cov[60:63, 20:60] = 1
    cov[rng.uniform(size=(h, w)) < 0.01] = 1
    got = texfinish.finish(dev(img), dev(cov), pad=3, erode=1, sizes=(48, 24))
    want = ref.finish(img, cov, pad_radius=3, erode_rounds=1, sizes=(48, 24))
    assert sorted(got) == sorted(want) == [24, 48, 96]
    for size in want:
        np.testing.assert_array_equal(got[size].cpu().numpy(), want[size])
    only = texfinish.finish(dev(img), dev(cov))
    assert list(only) == [96]
    np.testing.assert_array_equal(only[96].cpu().numpy(), img)
    with pytest.raises(ValueError, match="2\\^k"):
        texfinish.finish(dev(img), dev(cov), sizes=(40,))


# ---- write_texture, save_mesh -------------------------------------------------------------------------------------------------
def uv_case(seed=0):
    """a small UV mesh with two islands for write_texture: (uvs [8,2], colours [8,3], faces [4,3])"""
    verts, tris = two_islands(64, 64)
    uvs = np.stack([verts[:, 0] / 63.0, 1.0 - verts[:, 1] / 63.0], 1)
    colors = np.random.default_rng(seed).uniform(0.1, 1.0, size=(8, 3)).astype(np.float32)
    return uvs, colors, tris


def bake_u8(uvs, colors, faces, res):
    from topo4d_amd import texture
    img, depth = texture.render_colors(texture.process_uv(uvs, res, res), faces, colors, res, res, return_depth=True)
    return (img.cpu().numpy() * 255).astype(np.uint8), (depth.cpu().numpy() > -999999).astype(np.uint8)


@pytest.mark.parametrize("encoder", ["pil", "gpu"])
def test_write_texture_without_the_options_is_unchanged(tmp_path, encoder):
    from topo4d_amd import texture
    uvs, colors, faces = uv_case()
    texture.write_texture(str(tmp_path / "a.png"), uvs, colors, faces, res=64, encoder=encoder)
    texture.write_texture(str(tmp_path / "b.png"), uvs, colors, faces, res=64, encoder=encoder, pad=0, erode=0, sizes=())
    assert (tmp_path / "a.png").read_bytes() == (tmp_path / "b.png").read_bytes()
    assert sorted(os.listdir(tmp_path)) == ["a.png", "b.png"]


def test_write_texture_with_a_gutter_and_a_smaller_level(tmp_path):
    from PIL import Image
    from topo4d_amd import texfinish, texture
    uvs, colors, faces = uv_case()
    texture.write_texture(str(tmp_path / "face.png"), uvs, colors, faces, res=64, encoder="gpu", pad=3, erode=0, sizes=(32,))
    assert sorted(os.listdir(tmp_path)) == ["face.png", "face_32.png"]
    u8, cov = bake_u8(uvs, colors, faces, 64)
    want = ref.finish(u8, cov, pad_radius=3, erode_rounds=0, sizes=(32,))
    got64, got32 = np.asarray(Image.open(tmp_path / "face.png")), np.asarray(Image.open(tmp_path / "face_32.png"))
    np.testing.assert_array_equal(got64, want[64])
    np.testing.assert_array_equal(got32, want[32])
    dev_levels = texfinish.finish(dev(u8), dev(cov), pad=3, erode=0, sizes=(32,))
    np.testing.assert_array_equal(got64, dev_levels[64].cpu().numpy())
    np.testing.assert_array_equal(got32, dev_levels[32].cpu().numpy())
    covered = cov != 0
    np.testing.assert_array_equal(got64[covered], u8[covered])     # the bake itself is untouched
    assert (got64[~covered] != 0).any() and (u8[~covered] == 0).all()


def test_save_mesh_with_and_without_the_options(tmp_path):
    from PIL import Image
    from tests.test_gpu_objexport import device_params, texture_case
    from topo4d_amd import objexport, texture
    variables, params, dense = texture_case("quad")
    n = params["means3D"].shape[0]
    p = device_params(params, {"dense_rgb_colors": torch.from_numpy(dense).to(DEV)})
    exp = objexport.MeshExporter(variables)
    exp.save_mesh(str(tmp_path / "plain"), p, 2, res=64, gen_texture=True)
    exp.save_mesh(str(tmp_path / "zero"), p, 2, res=64, gen_texture=True, pad=0, erode=0, sizes=())
    exp.save_mesh(str(tmp_path / "pad"), p, 2, res=64, gen_texture=True, pad=3, erode=0, sizes=(32,))
    objexport.save_mesh(str(tmp_path / "drop_in"), p, variables, 2, res=64, gen_texture=True, pad=3, sizes=(32,))
    for name in ("face.obj", "face.png"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "zero" / name).read_bytes()
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "zero")) == ["face.obj", "face.png"]
    assert sorted(os.listdir(tmp_path / "pad")) == ["face.obj", "face.png", "face_32.png"]
    assert (tmp_path / "pad" / "face.obj").read_bytes() == (tmp_path / "plain" / "face.obj").read_bytes()
    colors = exp.seam_colors(p["dense_rgb_colors"]).cpu().numpy()
    u8, cov = bake_u8(np.array(variables["dense_uvs"]), colors, np.array(variables["dense_uv_faces"]), 64)
    np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "plain" / "face.png")), u8)
    want = ref.finish(u8, cov, pad_radius=3, erode_rounds=0, sizes=(32,))
    for d in ("pad", "drop_in"):
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / d / "face.png")), want[64])
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / d / "face_32.png")), want[32])
    covered = cov != 0
    np.testing.assert_array_equal(want[64][covered], u8[covered])


# ---- the property the feature exists for --------------------------------------------------------------------------------------
def test_a_gutter_removes_the_dark_seams_of_a_bilinear_render():
    from tests.test_meshrender_host import look_at_view
    from topo4d_amd import meshrender, texfinish, texture
    res = 64
    verts_uv, uv_tris = two_islands(res, res)
    uvs = np.stack([verts_uv[:, 0] / (res - 1), 1.0 - verts_uv[:, 1] / (res - 1)], 1)
    _, depth = texture.render_colors(texture.process_uv(uvs, res, res), uv_tris, np.zeros((8, 3), np.float32), res, res,
                                     return_depth=True)
    cov = texfinish.coverage_from_depth(depth)
    colour = torch.tensor([255, 51, 102], dtype=torch.uint8, device=DEV)
    tex = torch.where(cov[..., None] != 0, colour, torch.zeros_like(colour)).contiguous()   # the islands in one colour, on black
    padded = texfinish.pad(tex, cov, 2)[0]
    # the two quads side by side in space, seen from the front: their borders are the UV seams
    verts = np.array([[-1.0, -0.8, 0], [-0.1, -0.8, 0], [-0.1, 0.8, 0], [-1.0, 0.8, 0],
                      [0.1, -0.8, 0], [1.0, -0.8, 0], [1.0, 0.8, 0], [0.1, 0.8, 0]], np.float32)
    view = torch.from_numpy(look_at_view((0.0, 0.0, -3.0), (0.0, 0.0, 0.0), 64, 64)[None]).to(DEV)
    v = torch.from_numpy(verts).to(DEV)
    want = (colour.cpu().numpy().astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)

    def worst(texture_u8):
        r = meshrender.MeshRenderer(uv_tris, uv_tris, uvs, texture_u8, device=DEV)
        img, _, idx = r.render(v, (view, 64, 64), mapping="bilinear")
        hit = (idx[0] >= 0).cpu().numpy()
        assert hit.sum() > 500
        px = img[0].permute(1, 2, 0).cpu().numpy().astype(np.float64)[hit]
        return np.abs(px - want).max()

    assert worst(tex) > 1.0 / 255.0                               # the file as it is: black bleeds into the seams
    assert worst(padded) <= 1e-12


# ---- train, evaluate, the command ---------------------------------------------------------------------------------------------
def _train(root, out, *extra):
    from tests.test_setup_host import golden
    from topo4d_amd import train as T
    g = golden()
    argv = ["-e", "exp", "-s", "seq", "-id", root["input_dir"], "-did", root["dense_input_dir"], "-od", out, "-fn", "2",
            "-t", "-tr", "64", "-dn", "2", "-dr", "4", "-ion", "12", "-on", "6", "-don", "3", "-lf", "1000", "-dlf", "1000"] + list(extra)
    T.train(T.build_parser().parse_args(argv), facial_regions=g["facial_regions"], device=DEV)
    torch.cuda.synchronize()
    return os.path.join(out, "exp", "seq")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from tests.capture_scene import write_sequence
    from tests.test_setup_host import golden
    root = tmp_path_factory.mktemp("texfinish_run")
    dirs = write_sequence(root, golden(), n_frames=2)
    out = str(root / "out")
    return dict(dirs=dirs, out=out, run_dir=_train(dirs, out), root=root)


def test_train_writes_the_padded_texture_and_its_level(run):
    from PIL import Image
    out = str(run["root"] / "out_pad")
    run_dir = _train(run["dirs"], out, "--tex_pad", "2", "--tex_sizes", "32")
    for key in ("000001", "000002"):
        names = sorted(os.listdir(os.path.join(run_dir, key)))
        assert "face.png" in names and "face_32.png" in names and "face.obj" in names
        big = np.asarray(Image.open(os.path.join(run_dir, key, "face.png")))
        small = np.asarray(Image.open(os.path.join(run_dir, key, "face_32.png")))
        plain = np.asarray(Image.open(os.path.join(run["run_dir"], key, "face.png")))
        assert big.shape == (64, 64, 3) and small.shape == (32, 32, 3)
        assert "face_32.png" not in os.listdir(os.path.join(run["run_dir"], key))
        # the same seeds, the same run: the bake is the plain run's, so its own non-black texels are untouched and black ones filled
        lit = plain.any(-1)
        np.testing.assert_array_equal(big[lit], plain[lit])
        assert big.any(-1).sum() > lit.sum()
        with open(os.path.join(run_dir, key, "face.obj"), "rb") as f, open(os.path.join(run["run_dir"], key, "face.obj"), "rb") as g:
            assert f.read() == g.read()


def test_the_command_finishes_an_existing_tree(run, tmp_path):
    from PIL import Image
    from topo4d_amd import meshrender, texfinish
    out = str(tmp_path / "out")
    shutil.copytree(run["out"], out)
    frame = os.path.join(out, "exp", "seq", "000001")
    before = open(os.path.join(frame, "face.png"), "rb").read()
    texfinish.main(["-e", "exp", "-s", "seq", "-od", out, "--pad", "2", "--sizes", "32"])
    for key in ("000001", "000002"):
        d = os.path.join(out, "exp", "seq", key)
        assert {"face_pad.png", "face_pad_32.png", "face.png"} <= set(os.listdir(d))
        tex = np.array(Image.open(os.path.join(d, "face.png")).convert("RGB"))
        cov = texfinish.coverage_from_obj(meshrender.read_face_obj(os.path.join(d, "face.obj")), 64, 64)
        want = texfinish.finish(dev(tex), cov, pad=2, erode=1, sizes=(32,))
        np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(d, "face_pad.png"))), want[64].cpu().numpy())
        np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(d, "face_pad_32.png"))), want[32].cpu().numpy())
        ref_levels = ref.finish(tex, cov.cpu().numpy(), pad_radius=2, erode_rounds=1, sizes=(32,))
        np.testing.assert_array_equal(want[64].cpu().numpy(), ref_levels[64])
        np.testing.assert_array_equal(want[32].cpu().numpy(), ref_levels[32])
    assert open(os.path.join(frame, "face.png"), "rb").read() == before
    texfinish.main(["-e", "exp", "-s", "seq", "-od", out, "--pad", "2", "--frames", "1", "--in_place"])
    np.testing.assert_array_equal(np.asarray(Image.open(os.path.join(frame, "face.png"))),
                                  np.asarray(Image.open(os.path.join(frame, "face_pad.png"))))
    with pytest.raises(SystemExit):
        texfinish.main(["-e", "exp", "-s", "seq", "-od", out, "--pad", "2", "--sizes", "48"])


def test_evaluate_pads_the_texture_in_memory(run, tmp_path):
    from PIL import Image
    from topo4d_amd import cameras as C, evaluate as E, ingest, meshrender, texfinish
    out = str(tmp_path / "out")
    shutil.copytree(run["out"], out)
    path = os.path.join(out, "exp", "seq", "eval.json")
    argv = ["-e", "exp", "-s", "seq", "-id", run["dirs"]["input_dir"], "-did", run["dirs"]["dense_input_dir"], "-od", out, "-dr", "4"]
    E.main(argv)
    plain = open(path, "rb").read()
    files = {k: sorted(os.listdir(os.path.join(out, "exp", "seq", k))) for k in ("000001", "000002")}
    E.main(argv + ["--tex_pad", "2"])
    res = json.load(open(path))
    assert res["tex_pad"] == 2 and res["tex_erode"] == 1
    assert files == {k: sorted(os.listdir(os.path.join(out, "exp", "seq", k))) for k in files}     # padded in memory only
    base = json.loads(plain)
    assert "tex_pad" not in base and "tex_erode" not in base
    assert {k: v for k, v in res.items() if k not in ("tex_pad", "tex_erode", "low")} == {k: v for k, v in base.items() if k != "low"}
    # frame 1 against a render with the texture finished by hand
    d = os.path.join(out, "exp", "seq", "000001")
    obj = meshrender.read_face_obj(os.path.join(d, "face.obj"))
    tex = np.array(Image.open(os.path.join(d, "face.png")).convert("RGB"))
    padded = texfinish.finish(dev(tex), texfinish.coverage_from_obj(obj, 64, 64), pad=2, erode=1)[64]
    assert not torch.equal(padded, dev(tex))
    faces, uv_faces = meshrender.triangulate(obj.faces_ori, obj.uv_faces_ori)
    cams, _, trans_g = C.get_cameras(run["dirs"]["input_dir"], "seq", resize_factor=4)
    ds = ingest.get_dataset(run["dirs"]["input_dir"], "seq", 1, cams, use_mask=True, rotate_mask=C.ROTATE_MASK,
                            setup_camera=C.setup_camera, device=DEV)
    verts = torch.from_numpy(E.training_vertices(obj.vertices, trans_g)).to(DEV)
    for texture, got in ((padded, res), (tex, base)):
        r = meshrender.MeshRenderer(faces, uv_faces, obj.uvs, texture, device=DEV)
        scores = E.evaluate_frame(r, verts, ds, E.pixel_masks(ds))
        for name, row in scores.items():
            for n in ("l1", "mse", "psnr", "ssim", "psnr_full"):
                assert got["low"]["frames"]["000001"]["views"][name][n] == pytest.approx(row[n], rel=0, abs=0), (name, n)
    E.main(argv)
    assert open(path, "rb").read() == plain
    E.main(argv + ["--tex_pad", "3", "--tex_erode", "0"])
    res = json.load(open(path))
    assert (res["tex_pad"], res["tex_erode"]) == (3, 0)
    with pytest.raises(SystemExit):
        E.main(argv + ["--tex_pad", "65"])


# ---- one full-size run --------------------------------------------------------------------------------------------------------
def test_full_size_texture():
    """the uv_mesh bake at 8192^2: a gutter of 16 texels and the levels down to 1024"""
    from scaffold.scene import uv_mesh
    from topo4d_amd import texfinish, texture
    res, R = 8192, 16
    verts, tris, colors = uv_mesh(1025, res, res, seed=0)
    img, depth = texture.render_colors(verts, tris, colors, res, res, return_depth=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u8, cov = texfinish.quantize(img), texfinish.coverage_from_depth(depth)
    levels = texfinish.finish(u8, cov, pad=R, sizes=(4096, 2048, 1024))
    torch.cuda.synchronize()
    print(f"\nquantise + coverage + finish(pad={R}, sizes to 1024) at {res}^2: {(time.perf_counter() - t0) * 1e3:.2f} ms")
    del img
    assert sorted(levels) == [1024, 2048, 4096, 8192]
    for size, level in levels.items():
        assert tuple(level.shape) == (size, size, 3) and level.dtype == torch.uint8
    covered = cov != 0
    assert 0 < int(covered.sum()) < res * res
    assert torch.equal(levels[res][covered], u8[covered])
    # where every texel came from: an image of coordinates, x and y in two bytes each, through the same pad
    ys, xs = torch.meshgrid(torch.arange(res, device=DEV), torch.arange(res, device=DEV), indexing="ij")
    coords = torch.stack([xs & 255, xs >> 8, ys & 255, ys >> 8], -1).to(torch.uint8).contiguous()
    from_, filled = texfinish.pad(coords, cov, R)
    sx = from_[..., 0].to(torch.int64) + (from_[..., 1].to(torch.int64) << 8)
    sy = from_[..., 2].to(torch.int64) + (from_[..., 3].to(torch.int64) << 8)
    d2 = (sx - xs) ** 2 + (sy - ys) ** 2
    del coords, from_
    assert bool((d2[covered] == 0).all())
    assert bool(covered.reshape(-1)[(sy * res + sx).reshape(-1)][filled.reshape(-1) != 0].all())   # every source is a baked texel
    assert bool((d2[filled == 0] == 0).all()) and bool((d2 <= R * R).all())
    host_cov = cov.cpu().numpy() != 0
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:
        dist = ndimage.distance_transform_edt(~host_cov)
        near = np.rint(dist * dist).astype(np.int64)               # exact: squared distances are integers far below 2^53
        want_filled = near <= R * R
        np.testing.assert_array_equal(filled.cpu().numpy() != 0, want_filled)
        np.testing.assert_array_equal(d2.cpu().numpy()[want_filled], near[want_filled])           # and from a nearest texel
    else:
        y0, x0, n = 0, 0, 512 + 2 * R                              # a corner crop: uv_mesh leaves a border of the image uncovered
        crop_u8 = u8[y0:y0 + n, x0:x0 + n].cpu().numpy()
        want, want_cov = ref.pad(crop_u8, host_cov[y0:y0 + n, x0:x0 + n], R)
        inner = (slice(0, 512), slice(0, 512))                     # texels whose whole disc lies inside the crop (the image corner)
        np.testing.assert_array_equal(levels[res][y0:y0 + n, x0:x0 + n].cpu().numpy()[inner], want[inner])
        np.testing.assert_array_equal(filled[y0:y0 + n, x0:x0 + n].cpu().numpy()[inner], want_cov[inner])
