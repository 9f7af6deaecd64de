"""GPU: texfinish.fill / fill_islands (csrc/t4d_texfill.hip) against the numpy restatement of the rule (tests/texfill_ref.py), bit
for bit; projtex.island_labels; and --tex_fill through projtex.write_frame, the projtex command and train."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import projtex_scenes as S, texfill_ref as ref, texfinish_ref
from topo4d_amd import meshrender, projtex, texfinish

pytestmark = pytest.mark.gpu
DEV = "cuda"
# odd sizes, the edges of the 64-texel tile, one level beyond the six a workgroup fuses (129 x 200: 8 levels), a row of 4100 texels
# (13 levels: three launches each way) and 520 x 520 (81 tiles, rows that start on 4 bytes but not on 16)
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (37, 53), (64, 64), (65, 63), (129, 200), (3, 4100), (520, 520)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(img, valid, domain, what, level0=False):
    """fill on the device equals the yardstick and writes none of its inputs"""
    args = [dev(img), dev(valid), None if domain is None else dev(domain)]
    keep = [None if a is None else a.clone() for a in args]
    out, filled = texfinish.fill(*args)
    want, want_filled = ref.fill(img, valid, domain, level0)
    assert out.dtype == torch.uint8 and filled.dtype == torch.uint8 and tuple(out.shape) == img.shape and tuple(filled.shape) == valid.shape
    bad = int((out.cpu().numpy() != want).sum()), int((filled.cpu().numpy() != want_filled).sum())
    assert bad == (0, 0), (what, bad)
    assert all(k is None or torch.equal(a, k) for a, k in zip(args, keep)), (what, "an input was written")
    return want_filled


def _valid_sets(rng, shape):
    yield "all", np.ones(shape, np.uint8)
    yield "none", np.zeros(shape, np.uint8)
    for share in (0.01, 0.5, 0.99):
        yield share, (rng.random(shape) < share).astype(np.uint8) * rng.integers(1, 256, size=shape).astype(np.uint8)


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_equal_to_the_yardstick(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    filled = 0
    for c in (1, 3, 4):
        img = rng.integers(0, 256, size=shape + (c,), dtype=np.uint8)
        if c == 1 and shape[0] % 2:
            img = img[..., 0]                                        # [h,w] is an image of one channel
        for name, valid in _valid_sets(rng, shape):
            domains = [None, (rng.random(shape) < 0.5).astype(np.uint8) * 255, (valid != 0).astype(np.uint8)]   # the last: no hole in it
            level0 = ref.completed(img, valid)                        # the same under every domain
            for k, domain in enumerate(domains):
                got = _check(img, valid, domain, (shape, c, name, k), level0)
                assert k < 2 or not got.any()
                filled += int(got.sum())
    assert filled > 0 or shape == (1, 1)


@pytest.mark.parametrize("corner", [(0, 0), (0, 79), (95, 0), (95, 79)])
def test_one_valid_texel_in_a_corner_colours_the_whole_image(corner):
    rng = np.random.default_rng(11)
    for c in (1, 3, 4):
        img = rng.integers(0, 256, size=(96, 80, c), dtype=np.uint8)
        valid = np.zeros((96, 80), np.uint8)
        valid[corner] = 1
        _check(img, valid, None, (corner, c))
        out, filled = texfinish.fill(dev(img), dev(valid))
        assert (out.cpu().numpy() == img[corner]).all() and filled.sum().item() == 96 * 80 - 1


def test_holes_that_span_several_tiles():
    """valid only inside one 64 x 64 tile of 200 x 260: every other tile is filled from levels no texel of its own reaches"""
    rng = np.random.default_rng(12)
    for c in (1, 3, 4):
        img = rng.integers(0, 256, size=(200, 260, c), dtype=np.uint8)
        valid = np.zeros((200, 260), np.uint8)
        valid[64:128, 128:192] = rng.random((64, 64)) < 0.5
        domain = (rng.random((200, 260)) < 0.7).astype(np.uint8)
        for k, dom in enumerate((None, domain, valid)):
            _check(img, valid, dom, (c, k))


def test_buffers_that_start_on_an_odd_byte():
    """rows of 64 texels start on 16 bytes only when the buffer does: the kernels then move single bytes"""
    rng = np.random.default_rng(13)
    img, valid = rng.integers(0, 256, size=(70, 64, 3), dtype=np.uint8), (rng.random((70, 64)) < 0.4).astype(np.uint8)
    flat_i, flat_v = torch.zeros(img.size + 1, dtype=torch.uint8, device=DEV), torch.zeros(valid.size + 3, dtype=torch.uint8, device=DEV)
    di, dv = flat_i[1:].view(70, 64, 3), flat_v[3:].view(70, 64)
    di.copy_(dev(img))
    dv.copy_(dev(valid))
    assert di.is_contiguous() and di.data_ptr() % 2 == 1
    out, filled = texfinish.fill(di, dv)
    want, want_filled = ref.fill(img, valid)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(filled.cpu().numpy(), want_filled)


def test_2048_squared_with_30_percent_missing():
    rng = np.random.default_rng(14)
    img = rng.integers(0, 256, size=(2048, 2048, 3), dtype=np.uint8)
    valid = (rng.random((2048, 2048)) >= 0.3).astype(np.uint8)
    valid[300:700, 900:1500] = 0                                     # and one hole of many tiles
    _check(img, valid, None, "2048")


def _three_rectangles():
    rng = np.random.default_rng(15)
    img = rng.integers(0, 256, size=(90, 140, 3), dtype=np.uint8)
    labels = np.zeros((90, 140), np.uint8)
    labels[3:60, 4:66], labels[62:88, 10:120], labels[5:55, 70:135] = 1, 2, 7
    valid = (rng.random((90, 140)) < 0.6).astype(np.uint8)
    valid[labels == 2] = 0                                           # an island without a valid texel
    valid[labels == 7] = 1                                           # an island without a hole
    valid[20:40, 20:50] = 0
    return img, valid, labels


def test_fill_islands_is_bit_equal_to_the_yardstick():
    img, valid, labels = _three_rectangles()
    want, want_filled = ref.fill_islands(img, valid, labels)
    assert np.array_equal(want_filled != 0, (labels == 1) & (valid == 0)) and want_filled.sum() > 600
    for v in (dev(valid), dev(valid) != 0):
        args = [dev(img), v, dev(labels)]
        keep = [a.clone() for a in args]
        out, filled = texfinish.fill_islands(*args)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(filled.cpu().numpy(), want_filled)
        assert all(torch.equal(a, k) for a, k in zip(args, keep))
    # one island's colours never enter another's holes: island 1 painted in one colour fills in that colour
    flat = img.copy()
    flat[labels == 1] = (9, 99, 199)
    out, filled = texfinish.fill_islands(dev(flat), dev(valid), dev(labels))
    assert (out.cpu().numpy()[want_filled != 0] == (9, 99, 199)).all()
    # a single-channel image, and no label at all
    out, filled = texfinish.fill_islands(dev(img[..., 0]), dev(valid), dev(labels))
    w1, f1 = ref.fill_islands(img[..., 0], valid, labels)
    assert np.array_equal(out.cpu().numpy(), w1) and np.array_equal(filled.cpu().numpy(), f1)
    out, filled = texfinish.fill_islands(dev(img), dev(valid), dev(np.zeros_like(labels)))
    assert np.array_equal(out.cpu().numpy(), img) and not filled.any()


def test_device_arguments_are_checked():
    img, valid = dev(np.zeros((8, 9, 3), np.uint8)), dev(np.ones((8, 9), np.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        texfinish.fill(img, valid.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        texfinish.fill(img, valid, valid.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        texfinish.fill_islands(img, valid, valid.cpu())
    with pytest.raises(ValueError):
        texfinish.fill(img, valid[:7])


@pytest.mark.parametrize("res", [(64, 64), (40, 56)])
def test_island_labels_of_three_quads(res):
    obj = S.three_quads()
    labels = projtex.island_labels(obj, *res, DEV)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == res
    got = labels.cpu().numpy()
    cov = texfinish.coverage_from_obj(obj, *res, device=DEV).cpu().numpy() != 0
    assert np.array_equal(got != 0, cov)
    assert set(np.unique(got)) == {0, 1, 2, 3}
    for k in range(3):
        one = meshrender.FaceObj(obj.vertices[4 * k:4 * k + 4], obj.uvs[4 * k:4 * k + 4], [[0, 1, 2, 3]], [[0, 1, 2, 3]])
        inner = S.erode(S.quad_maps64(one, *res)[2], 2)
        assert inner.sum() > 100 and (got[inner] == k + 1).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _one_camera_frame(obj, eye, target, f, seed):
    from topo4d_amd import cameras as C
    w2c, K = S.camera(eye, target, S.H, S.W, f)
    photo = np.random.default_rng(seed).uniform(0.2, 1.0, size=(3, S.H, S.W)).astype(np.float32)       # never black
    return [{"cam": C.setup_camera(None, S.W, S.H, K, w2c, device=DEV), "im": dev(photo), "cam_name": "cam00"}]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_write_frame_fills_the_shadow_of_the_occlusion_scene(tmp_path):
    obj, _ = S.occlusion_scene()
    dataset = _one_camera_frame(obj, [0.05, -0.03, -3.0], [0.0, 0.0, 0.0], 60.0, 21)
    opts = dict(projtex.DEFAULTS)
    plain_dir, fill_dir = str(tmp_path / "plain"), str(tmp_path / "fill")
    os.makedirs(plain_dir)
    os.makedirs(fill_dir)
    kw = dict(pad=2, sizes=[32], save_weight=True, device=DEV)
    plain = projtex.write_frame(plain_dir, obj, None, dataset, 64, opts, **kw)
    filled_files = projtex.write_frame(fill_dir, obj, None, dataset, 64, opts, fill=True, **kw)
    assert [os.path.basename(p) for p in plain] == [os.path.basename(p) for p in filled_files] == ["face_proj.png", "face_proj_32.png",
                                                                                                    "face_proj_weight.png"]
    verts = torch.from_numpy(obj.vertices).to(DEV)
    tex, _, count = projtex.project_frame(obj, verts, dataset, 64, device=DEV, **opts)
    labels = projtex.island_labels(obj, 64, 64, DEV).cpu().numpy()
    seen = count.cpu().numpy() > 0
    want, want_filled = ref.fill_islands(tex.cpu().numpy(), seen, labels)
    levels = texfinish_ref.finish(want, seen | (want_filled != 0), pad_radius=2, sizes=[32])
    assert np.array_equal(_png(filled_files[0]), levels[64]) and np.array_equal(_png(filled_files[1]), levels[32])
    # the weight file is the count either way, so its zeros inside an island mark what was filled
    assert open(filled_files[2], "rb").read() == open(plain[2], "rb").read() and np.array_equal(_png(plain[2]), count.cpu().numpy())
    got, before = _png(filled_files[0]), _png(plain[0])
    assert np.array_equal(got[seen], before[seen]) and np.array_equal(before[seen], tex.cpu().numpy()[seen])
    shadow = (labels == 1) & ~seen
    print("shadow texels of the large quad", shadow.sum(), "filled in all", int(want_filled.sum()))
    assert shadow.sum() > 100 and got[shadow].any(-1).all() and np.array_equal((want_filled != 0) & (labels == 1), shadow)
    assert not (want_filled != 0)[(labels == 0) | seen].any()        # (the backdrop's island of a few texels may hold no seen one)
    inner = S.erode(shadow, 2)                                       # beyond the plain file's gutter of 2 texels
    assert inner.sum() > 30 and not before[inner].any()


def test_write_frame_leaves_an_island_no_view_sees(tmp_path):
    obj = S.three_quads()
    dataset = _one_camera_frame(obj, [0.9, 0.5, -2.6], [0.1, 0.0, 0.0], 44.0, 22)
    files = {}
    for fill in (False, True):
        d = str(tmp_path / f"fill{int(fill)}")
        os.makedirs(d)
        files[fill] = projtex.write_frame(d, obj, None, dataset, 64, dict(projtex.DEFAULTS), save_weight=True, device=DEV, fill=fill)
    labels = projtex.island_labels(obj, 64, 64, DEV).cpu().numpy()
    count = _png(files[True][1])
    plain, filled = _png(files[False][0]), _png(files[True][0])
    away = labels == 3
    assert away.sum() > 100 and not count[away].any()               # the quad that faces away
    assert np.array_equal(plain[away], filled[away]) and not filled[away].any()
    hidden = (labels == 1) & (count == 0)                            # the first quad behind the second
    assert hidden.sum() > 20 and filled[hidden].any(-1).all() and not plain[hidden].any()
    assert np.array_equal(plain[labels == 0], filled[labels == 0])


# ---- command lines ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from tests.capture_scene import write_sequence
    from tests.test_gpu_projtex import TOL, _train
    from tests.test_setup_host import golden
    root = tmp_path_factory.mktemp("texfill_run")
    dirs = write_sequence(root, golden(), n_frames=3)
    # (-cf 1: a checkpoint after every frame but the first, so that params.npz and loss.json exist in a run of three frames)
    proj = _train(dirs, str(root / "proj"), "--tex_project", "-cf", "1", *TOL)
    fill = _train(dirs, str(root / "fill"), "--tex_project", "--tex_fill", "-cf", "1", *TOL)
    return dict(root=root, dirs=dirs, proj=proj, fill=fill)


KEYS = ["000001", "000002", "000003"]


def test_train_with_the_flag_changes_the_projected_texture_alone(runs):
    from tests.test_gpu_projtex import _tree
    proj, fill = _tree(runs["proj"]), _tree(runs["fill"])
    assert sorted(proj) == sorted(fill)
    changed = []
    for name, data in proj.items():
        if name.endswith(".npz"):                                    # (a zip archive carries the time it was written)
            a, b = np.load(os.path.join(runs["proj"], name)), np.load(os.path.join(runs["fill"], name))
            assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[k], b[k]) for k in a.files), name
        elif fill[name] != data:
            changed.append(name)
    assert sorted(changed) == [os.path.join(k, "face_proj.png") for k in KEYS]
    assert {"params.npz", "face.obj", "face.png", "loss.json"} <= {os.path.basename(n) for n in proj}      # all compared above


def test_the_command_with_the_flag_writes_what_write_frame_returns(runs, tmp_path):
    from tests.test_gpu_projtex import TOL, _io, _tree
    from topo4d_amd import cameras as C, ingest
    out = str(tmp_path / "out")
    shutil.copytree(os.path.dirname(os.path.dirname(runs["proj"])), out)
    run_dir = os.path.join(out, "exp", "seq")
    before = _tree(run_dir)
    projtex.main(_io(runs) + ["-od", out, "--tex_res", "64", "--tex_fill", "--save_weight"] + TOL)
    after = _tree(run_dir)
    assert sorted(set(after) - set(before)) == [os.path.join(k, "face_proj_weight.png") for k in KEYS]
    cams, _, trans_g = C.get_cameras(runs["dirs"]["input_dir"], "seq", resize_factor=1)
    for key in KEYS:
        name = os.path.join(key, "face_proj.png")
        assert after[name] == open(os.path.join(runs["fill"], name), "rb").read()          # what train --tex_fill wrote
        d = str(tmp_path / key)
        os.makedirs(d)
        obj = meshrender.read_face_obj(os.path.join(run_dir, key, "face.obj"))
        ds = ingest.get_dataset(runs["dirs"]["dense_input_dir"], "seq", int(key), cams, use_mask=False, blacklist=C.BLACKLIST,
                                rotate_mask=C.ROTATE_MASK, setup_camera=C.setup_camera, device=DEV)
        written = projtex.write_frame(d, obj, trans_g, ds, 64, dict(projtex.DEFAULTS, depth_tol=0.02), device=DEV, fill=True)
        assert open(written[0], "rb").read() == after[name]
        count = _png(os.path.join(run_dir, key, "face_proj_weight.png"))
        got, plain = _png(os.path.join(run_dir, key, "face_proj.png")), _png(os.path.join(runs["proj"], key, "face_proj.png"))
        labels = projtex.island_labels(obj, 64, 64, DEV).cpu().numpy()
        holes = (labels > 0) & (count == 0)
        print(key, "texels filled", holes.sum())
        assert np.array_equal(got[~holes], plain[~holes]) and holes.any() and not plain[holes].any()
    # without the flag the command writes the plain files again, byte for byte
    projtex.main(_io(runs) + ["-od", out, "--tex_res", "64"] + TOL)
    assert all(_tree(run_dir)[os.path.join(k, "face_proj.png")] == before[os.path.join(k, "face_proj.png")] for k in KEYS)
