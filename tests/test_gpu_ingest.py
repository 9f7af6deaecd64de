"""GPU: topo4d_amd.ingest against PIL and the host restatements of tests/ingest_ref.py - the JPEG decoder byte-identical to
np.asarray(Image.open(f)) over sizes, samplings, qualities, restart intervals, optimised tables, contents, mixed batches and
small sync chunks; the warp bit-exact with the restated skimage rotate; get_dataset and FramePrefetcher equal to the
reference's get_dataset restated on the host."""
import io
import itertools

import numpy as np
import pytest
import torch
from PIL import Image, ImageFile

from tests import ingest_ref as ref
from tests.test_ingest_host import content, jpeg_bytes
from topo4d_amd import ingest

pytestmark = pytest.mark.gpu
ImageFile.MAXBLOCK = 1 << 24

SIZES = [(1, 1), (7, 9), (17, 33), (375, 512), (512, 375), (257, 129)]
KINDS = ["noise", "flat", "saturated", "grad"]
KWS = [{}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 7}, {"restart_marker_rows": 1}, {"optimize": True}]


def corpus():
    files = []
    for i, ((h, w), sub, q) in enumerate(itertools.product(SIZES, (0, 1, 2), (50, 75, 95, 100))):
        files.append(jpeg_bytes(content(h, w, KINDS[i % 4], seed=i), quality=q, subsampling=sub, **KWS[i % 5]))
    for i, (kind, kw, sub) in enumerate(itertools.product(KINDS, KWS, (0, 1, 2))):
        files.append(jpeg_bytes(content(375, 512, kind, seed=100 + i), quality=95, subsampling=sub, **kw))
    return files


def check(files, out):
    assert len(out) == len(files)
    for k, (f, o) in enumerate(zip(files, out)):
        want = np.asarray(Image.open(io.BytesIO(f)))
        got = o.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (k, ingest.parse_jpeg(f).sampling)


@pytest.fixture(scope="module")
def files():
    return corpus()


@pytest.mark.parametrize("chunk_bits", [None, 256, 1000])
def test_decode_matches_pil(files, chunk_bits):
    check(files, ingest.decode_jpeg(files, chunk_bits=chunk_bits))


def test_decode_4k_frame():
    img = content(3008, 4096, "grad")
    img[::7, ::5] = np.random.default_rng(1).integers(0, 256, img[::7, ::5].shape, dtype=np.uint8)
    files = [jpeg_bytes(img, quality=95, subsampling=2), jpeg_bytes(img, quality=75, subsampling=0)]
    check(files, ingest.decode_jpeg(files))
    check(files[:1], ingest.decode_jpeg(files[:1], chunk_bits=512))


def test_mixed_batch_with_fallbacks():
    img = content(40, 56, "grad")
    files = [jpeg_bytes(img, quality=90), jpeg_bytes(img, quality=90, progressive=True), jpeg_bytes(img[..., 0], quality=90),
             jpeg_bytes(img, quality=60, subsampling=0, restart_marker_blocks=3)]
    check(files, ingest.decode_jpeg(files, chunk_bits=128))


def test_decode_is_deterministic_over_dirty_scratch(files):
    a = [t.clone() for t in ingest.decode_jpeg(files[:40], chunk_bits=256)]
    junk = torch.full((256 << 20,), 0xAB, dtype=torch.uint8, device="cuda")
    del junk
    b = ingest.decode_jpeg(files[:40], chunk_bits=256)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_truncated_segment_is_rejected():
    data = jpeg_bytes(content(48, 64, "noise"), quality=90)
    h = ingest.parse_jpeg(data)
    cut = data[:h.scan_start + (h.scan_end - h.scan_start) // 2] + b"\xff\xd9"
    for cb in (None, 256):
        with pytest.raises(ValueError, match="ended early"):
            ingest.decode_jpeg([cut], chunk_bits=cb)
    rst = jpeg_bytes(content(48, 64, "noise"), quality=90, restart_marker_blocks=2)
    h = ingest.parse_jpeg(rst)
    with pytest.raises(ValueError, match="status"):
        ingest.decode_jpeg([rst[:h.scan_start + (h.scan_end - h.scan_start) // 2] + b"\xff\xd9"])


@pytest.mark.parametrize("angle", [90, -90, 0, 180, 30, -45])
@pytest.mark.parametrize("channels", [1, 3, 4])
@pytest.mark.parametrize("zeros", [True, False])
def test_warp_matches_restatement(angle, channels, zeros):
    rng = np.random.default_rng(abs(angle) * 10 + channels + (angle < 0))
    img = rng.integers(1 if not zeros else 0, 256, (61, 93, channels), dtype=np.uint8)
    if zeros:
        img[rng.random(img.shape) < 0.5] = 0
    src = torch.from_numpy(img).cuda()
    m, shape = ingest.rotate_matrix(61, 93, angle)
    got = ingest.warp_views([src], [m], [shape])[0].cpu()
    assert torch.equal(got, ref.rotate_target(img, angle))


def test_warp_batch_with_crop():
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (375, 512, 3), dtype=np.uint8), rng.integers(3, 256, (520, 380, 4), dtype=np.uint8)]
    crops = [None, (512, 375)]
    angles = [90, -90]
    srcs = [torch.from_numpy(a).cuda() for a in imgs]
    mats, shapes = zip(*[ingest.rotate_matrix(*(c or a.shape[:2]), ang) for a, c, ang in zip(imgs, crops, angles)])
    out = ingest.warp_views(srcs, mats, shapes, crops)
    assert torch.equal(out[0].cpu(), ref.rotate_target(imgs[0], 90))
    assert torch.equal(out[1].cpu(), ref.rotate_target(imgs[1][:512, :375], -90))
    pre = torch.zeros_like(out[1])
    ingest.warp_views(srcs[1:], mats[1:], shapes[1:], crops[1:], out=[pre])
    assert torch.equal(pre, out[1])


def make_dataset(root):
    rng = np.random.default_rng(11)
    seq, frame = "seq", 4
    fdir = root / seq / ("%06d" % frame)
    mdir = root / seq / "mask" / ("%06d" % frame)
    fdir.mkdir(parents=True)
    mdir.mkdir(parents=True)
    views = {"cam00": ("jpg", dict(quality=95, subsampling=2), 1), "cam01": ("jpg", dict(quality=90, progressive=True), -1),
             "cam02": ("jpg", dict(quality=85, subsampling=0, restart_marker_rows=1), 0), "cam03": ("png", {}, 1),
             "skip04": ("jpg", dict(quality=95), 1)}
    cameras, rotate_mask = {}, {}
    for name, (ext, kw, rot) in views.items():
        img = content(96, 72, "grad", seed=len(cameras))
        img[rng.random((96, 72)) < 0.3] = 0
        Image.fromarray(img).save(fdir / f"{name}.{ext}", "JPEG" if ext == "jpg" else "PNG", **kw)
        mask = (rng.random((100, 80, 3)) < 0.5).astype(np.uint8) * 255
        Image.fromarray(mask).save(mdir / f"{name}.png")
        rotate_mask[name] = rot
        h, w = (72, 96) if rot else (96, 72)
        k = np.array([[80.0, 0, w / 2], [0, 80.0, h / 2], [0, 0, 1]])
        w2c = np.concatenate([np.eye(3), np.array([[0.1], [0.2], [3.0]])], 1)
        cameras[f"{name}.{ext}"] = {"image_size": (h, w), "intrinsics": k, "extrinsics": w2c}
    return str(root), seq, frame, cameras, rotate_mask


def setup_camera(cam, w, h, k, w2c, near=0.01, far=100):
    from scaffold import reference_boundary as boundary
    return boundary.setup_camera(w, h, k, w2c, near, far, device="cuda")


def compare(got, want):
    assert [d["cam_name"] for d in got] == [d["cam_name"] for d in want]
    assert [d["id"] for d in got] == [d["id"] for d in want]
    for g, w in zip(got, want):
        assert g["im"].is_contiguous() and torch.equal(g["im"], w["im"]), g["cam_name"]
        assert (g["mask"] is None) == (w["mask"] is None)
        if w["mask"] is not None:
            assert torch.equal(g["mask"], w["mask"]), g["cam_name"]
        assert torch.equal(g["cam"].viewmatrix, w["cam"].viewmatrix)


@pytest.mark.parametrize("use_mask", [False, True])
def test_get_dataset_matches_reference(tmp_path, use_mask):
    data_dir, seq, frame, cameras, rotate_mask = make_dataset(tmp_path)
    args = (data_dir, seq, frame, cameras, use_mask, ["skip"])
    want = ref.reference_get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera)
    got = ingest.get_dataset(*args, rotate_mask=rotate_mask, setup_camera=setup_camera)
    assert len(got) == 4
    compare(got, want)
    with ingest.FramePrefetcher(data_dir, seq, cameras, use_mask, ["skip"], rotate_mask=rotate_mask,
                                setup_camera=setup_camera) as pf:
        pf.prefetch(frame)
        compare(pf.get(frame), want)
