"""CPU: the host half of topo4d_amd.ingest - JPEG header parsing against Pillow, rotate_matrix and the restated warp, the
get_dataset file logic - and the host C++ build of csrc/t4d_jpeg.h (tests/native/jpeg_host.cpp) decoding PIL-written files
byte-identically to PIL, on the sequential path and through the chunked self-synchronising one."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageFile

from tests import ingest_ref as ref
from topo4d_amd import ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ImageFile.MAXBLOCK = 1 << 24            # PIL's optimize=True needs the whole file in one buffer


def jpeg_bytes(img, **kw):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


def content(h, w, kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (37, 180, 99), np.uint8)
    if kind == "saturated":
        a = rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255
        return a
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + 2 * y) % 256], -1).astype(np.uint8)


@pytest.mark.parametrize("sub", [0, 1, 2])
@pytest.mark.parametrize("kw", [{}, {"restart_marker_blocks": 7}, {"restart_marker_rows": 1}, {"optimize": True}])
def test_parse_matches_pillow(sub, kw):
    data = jpeg_bytes(content(37, 53, "noise"), quality=75, subsampling=sub, **kw)
    h = ingest.parse_jpeg(data)
    im = Image.open(io.BytesIO(data))
    assert h.gpu, h.reason
    assert (h.width, h.height) == im.size
    for tq, q in im.quantization.items():                  # natural order, as Pillow lists them
        assert np.array_equal(h.quant[tq], np.asarray(q))
    assert h.sampling == [((1, 1), (2, 1), (2, 2))[sub], (1, 1), (1, 1)]
    if "restart_marker_blocks" in kw:
        assert h.restart_interval == 7
    elif "restart_marker_rows" in kw:
        assert h.restart_interval == (53 + 8 * (1, 2, 2)[sub] - 1) // (8 * (1, 2, 2)[sub])
    else:
        assert h.restart_interval == 0
    assert data[h.scan_end:h.scan_end + 2] == b"\xff\xd9"


def test_fallback_files():
    img = content(24, 40, "grad")
    prog = jpeg_bytes(img, quality=80, progressive=True)
    gray = jpeg_bytes(img[..., 0], quality=80)
    b = io.BytesIO()
    Image.fromarray(np.concatenate([img, img[..., :1]], -1), "RGBA").convert("CMYK").save(b, "JPEG")
    for data, why in ((prog, "SOF2"), (gray, "1 components"), (b.getvalue(), "4 components")):
        h = ingest.parse_jpeg(data)
        assert not h.gpu and why in h.reason


def test_malformed_headers_raise():
    data = jpeg_bytes(content(16, 16, "noise"), quality=90)
    h = ingest.parse_jpeg(data)
    for bad in (b"", b"\xff\xd8", b"garbage" * 10, data[:h.scan_start - 5], data[:40], b"\xff\xd8\xff\xdb\x00\x43\x00",
                data[:h.scan_start + 10]):
        with pytest.raises(ValueError):
            ingest.parse_jpeg(bad)


@pytest.mark.parametrize("shape", [(375, 512), (512, 375), (7, 9), (1, 1), (4096, 3008)])
@pytest.mark.parametrize("angle", [90, -90, 0, 180, 30, -45])
def test_rotate_matrix_matches_restatement(shape, angle):
    m, out = ingest.rotate_matrix(shape[0], shape[1], angle)
    rm, rout = ref.skimage_rotate_params(shape[0], shape[1], angle)
    assert out == rout
    assert np.array_equal(m, rm)
    if angle in (90, -90):
        assert out == (shape[1], shape[0])


@pytest.mark.parametrize("angle", [90, -90])
def test_restated_rotation_is_rot90_up_to_contamination(angle):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (375, 512, 3), dtype=np.uint8)
    img[rng.random((375, 512, 3)) < 0.7] = 0
    got = ref.rotate_float64(img / 255.0, angle)
    want = np.rot90(img / 255.0, 1 if angle > 0 else -1)
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-12
    assert (got != want).sum() > 1000, "the warp's cos(pi/2) contamination is modelled"


def test_frame_files_order_blacklist_and_masks(tmp_path):
    d = tmp_path / "data" / "seq" / "000003"
    d.mkdir(parents=True)
    for n in ("b.jpg", "a.jpg", "c.png", "skip1.jpg", "a2.png", "x.txt"):
        (d / n).write_bytes(b"")
    files = ingest.frame_files(str(tmp_path / "data"), "seq", 3, use_mask=True, blacklist=["skip"])
    names = [os.path.basename(p) for p, _ in files]
    assert names == ["a.jpg", "b.jpg", "a2.png", "c.png"]
    assert files[0][1] == str(tmp_path / "data" / "seq" / "mask" / "000003" / "a.png")
    assert all(m is None for _, m in ingest.frame_files(str(tmp_path / "data"), "seq", 3))


def test_pool_size(monkeypatch):
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert ingest.pool_size() == 8
    monkeypatch.setenv("OMP_NUM_THREADS", "64")
    assert ingest.pool_size() == 16
    monkeypatch.setenv("OMP_NUM_THREADS", "3")
    assert ingest.pool_size() == 3


@pytest.fixture(scope="module")
def jpeg_host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs a host C++ compiler")
    exe = tmp_path_factory.mktemp("native") / "jpeg_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "jpeg_host.cpp")])
    return str(exe)


def host_decode(exe, data, chunk_bits):
    h = ingest.parse_jpeg(data)
    assert h.gpu, h.reason
    d = ingest._descriptor(h, 0, 0)
    r = subprocess.run([exe], input=bytes(d) + struct.pack("<i", chunk_bits) + data[h.scan_start:h.scan_end], capture_output=True)
    return r.returncode, r.stdout, h


MATRIX = [((h, w), sub, q, kind, kw)
          for (h, w) in [(1, 1), (7, 9), (17, 33), (257, 129), (375, 512)]
          for sub in (0, 1, 2) for q in (50, 95, 100) for kind in ("noise", "grad")
          for kw in ({}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1}, {"optimize": True})]


def test_host_build_matches_pil(jpeg_host):
    bad = []
    for i, (shape, sub, q, kind, kw) in enumerate(MATRIX):
        data = jpeg_bytes(content(*shape, kind, seed=i), quality=q, subsampling=sub, **kw)
        want = np.asarray(Image.open(io.BytesIO(data)))
        for cb in (0, 256, 1000):
            rc, out, h = host_decode(jpeg_host, data, cb)
            # one lane (chunk_bits 0), a lane per restart interval, or fewer chunk lanes than t4d_jpeg::kRounds: the sequential
            # fallback (exit 128) cannot run; tests/test_jpeg_files_host.py names cases that must and must not take it
            lanes = -(-(h.scan_end - h.scan_start) * 8 // cb) if cb else 1
            exact = cb == 0 or h.restart_interval > 0 or lanes < 12
            if rc not in ((0,) if exact else (0, 128)) or out != want.tobytes():
                bad.append((shape, sub, q, kind, kw, cb, rc))
    assert not bad, bad[:5]


def test_host_build_rejects_truncated_segment(jpeg_host):
    data = jpeg_bytes(content(64, 64, "noise"), quality=90)
    h = ingest.parse_jpeg(data)
    cut = data[:h.scan_start + (h.scan_end - h.scan_start) // 2] + b"\xff\xd9"
    for cb in (0, 256):
        rc, _, _ = host_decode(jpeg_host, cut, cb)
        assert rc & 1, rc


@pytest.mark.parametrize("sub", [0, 2])
def test_host_chunk_lanes_converge_without_fallback(jpeg_host, sub):
    """The lanes reach their fixed point within the GPU's round limit on a smooth, noisy q95 view (no sequential fallback)."""
    rng = np.random.default_rng(2)
    y, x = np.meshgrid(np.linspace(-1, 1, 752), np.linspace(-1, 1, 1024), indexing="ij")
    f = np.stack([0.5 + 0.4 * np.sin(5 * x), 0.5 + 0.4 * np.cos(4 * y), 0.5 + 0.3 * np.sin(3 * (x + y))], -1)
    img = (np.clip(f + rng.normal(0, 0.02, f.shape), 0, 1) * 255).astype(np.uint8)
    data = jpeg_bytes(img, quality=95, subsampling=sub)
    for cb in (4096, 16384):
        rc, out, _ = host_decode(jpeg_host, data, cb)
        assert rc == 0 and out == np.asarray(Image.open(io.BytesIO(data))).tobytes(), (cb, rc)
