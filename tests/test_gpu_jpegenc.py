"""GPU: topo4d_amd.jpeg.encode_jpeg (t4d_jpeg_encode) writes PIL's files byte for byte - the whole host matrix
(tests/jpegenc_cases.py), two cases that span several waves, scan chunks and stuffing chunks, and a mixed batch - is a pure function
of its inputs whatever the scratch held, writes nothing beyond a file's length, and its files decode through the project's own
decoder.  The expected bytes always come from PIL, never from the restatement."""
import ctypes as C
import io

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpegenc_cases as cases
from topo4d_amd import _lib, ingest, jpeg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_encode(arrays, quality, subsampling, scratch_fill=None, out_fill=0xA5, guard=4096):
    """t4d_jpeg_encode called directly: (out buffer on the host, lengths, descriptors, capacities); the scratch is filled with
    `scratch_fill` first, the output with `out_fill`, and `guard` more bytes follow the capacity the library is told."""
    imgs = [dev(a) for a in arrays]
    caps = [jpeg.max_encoded_bytes(a.shape[0], a.shape[1], subsampling) for a in arrays]
    descs, cap = jpeg._descriptors(imgs, caps)
    scratch, nscratch = _lib.scratch("t4d_jpeg_enc_scratch_bytes", imgs[0].device, descs, len(imgs), subsampling)
    if scratch_fill is not None:
        scratch.fill_(scratch_fill)
    out = torch.full((cap + guard,), out_fill, dtype=torch.uint8, device=DEV)
    lengths = torch.full((len(imgs),), -7, dtype=torch.int64, device=DEV)
    d_descs = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    _lib.call("t4d_jpeg_encode", descs, _lib.ptr(d_descs), len(imgs), quality, subsampling, _lib.ptr(out), cap, _lib.ptr(lengths),
              _lib.ptr(scratch), nscratch, _lib.stream(imgs[0].device))
    torch.cuda.synchronize()
    return out.cpu().numpy(), lengths.cpu().tolist(), descs, caps, cap


@pytest.mark.parametrize("subsampling", cases.SUBSAMPLINGS)
def test_matrix_equals_pil(subsampling):
    todo = [c for c in cases.matrix() if c[3] == subsampling]
    assert len(todo) >= 330
    bad = []
    for q in sorted({c[4] for c in todo}):
        group = [c for c in todo if c[4] == q]
        arrays = [cases.image_of(c) for c in group]
        assert all(jpeg.can_encode(a.shape, subsampling) for a in arrays)
        files = jpeg.encode_jpeg([dev(a) for a in arrays], quality=q, subsampling=subsampling)
        for c, a, f in zip(group, arrays, files):
            if f != cases.pil_bytes(a, q, subsampling):
                bad.append(c)
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("h,w,kind,q,s", [(264, 256, "random", 100, 0), (250, 330, "smooth", 75, 1), (94, 330, "random", 100, 2),
                                          (376, 512, "smooth", 95, 2)])
def test_larger_cases_equal_pil(h, w, kind, q, s):
    a = cases.content(h, w, kind, seed=3)
    f = jpeg.encode_jpeg(dev(a), quality=q, subsampling=s)
    want = cases.pil_bytes(a, q, s)
    assert len(f) == len(want) and f == want
    if kind == "random":
        assert len(f) > 2 * 4096 + 623 and f[623:].count(b"\xff\x00") >= 10      # several stuffing chunks, stuffed bytes in them


def mixed_batch():
    shapes = [(64, 48), (1, 1), (37, 53), (8, 8), (120, 200), (17, 9), (3, 16), (256, 40), (33, 31), (16, 16), (90, 90), (7, 7),
              (48, 64), (9, 8), (200, 120), (16, 8), (2, 2), (75, 31), (31, 75), (128, 128), (5, 40), (40, 5), (66, 66), (100, 1)]
    return [cases.content(h, w, cases.KINDS[i % len(cases.KINDS)], seed=i) for i, (h, w) in enumerate(shapes)]


@pytest.mark.parametrize("q,s", [(95, 0), (75, 1), (90, 2)])
def test_batch_of_24_mixed_images_equals_each_alone(q, s):
    arrays = mixed_batch()
    assert len(arrays) == 24
    together = jpeg.encode_jpeg([dev(a) for a in arrays], quality=q, subsampling=s)
    for i, (a, f) in enumerate(zip(arrays, together)):
        assert f == cases.pil_bytes(a, q, s), i
        if i % 5 == 0:
            assert jpeg.encode_jpeg(dev(a), quality=q, subsampling=s) == f, i


def test_small_launches_give_the_same_files(monkeypatch):
    """encode_jpeg cuts a batch whose buffers pass jpeg.batch_bytes into several launches: the files do not change."""
    arrays = mixed_batch()[:8]
    whole = jpeg.encode_jpeg([dev(a) for a in arrays], quality=85, subsampling=2)
    monkeypatch.setattr(jpeg, "batch_bytes", 1)
    assert jpeg.encode_jpeg([dev(a) for a in arrays], quality=85, subsampling=2) == whole


def test_scratch_content_and_output_bounds():
    """The same bytes over scratch full of 0xFF, over scratch full of 0x00 and again; nothing written beyond a file's length, nor
    behind the capacity."""
    arrays = mixed_batch()[:10] + [cases.content(94, 130, "random", seed=9)]
    runs = [raw_encode(arrays, 92, 2, scratch_fill=fill) for fill in (0xFF, 0x00, 0xFF)]
    out, lengths, descs, caps, cap = runs[0]
    for i, (a, n, c) in enumerate(zip(arrays, lengths, caps)):
        o = descs[i].out_offset
        assert 0 < n <= c
        assert out[o:o + n].tobytes() == cases.pil_bytes(a, 92, 2), i
        end = descs[i + 1].out_offset if i + 1 < len(arrays) else cap
        assert (out[o + n:end] == 0xA5).all(), i
    assert (out[cap:] == 0xA5).all() and out[cap:].size == 4096
    for other in runs[1:]:
        assert other[1] == lengths and np.array_equal(other[0], out)


def test_own_decoder_reads_the_files():
    arrays = [cases.content(h, w, kind, seed=h) for (h, w, kind) in [(64, 48, "smooth"), (37, 53, "random"), (94, 130, "smooth"),
                                                                      (17, 9, "binary")]]
    for s in cases.SUBSAMPLINGS:
        files = jpeg.encode_jpeg([dev(a) for a in arrays], quality=90, subsampling=s)
        assert all(ingest.parse_jpeg(f).gpu for f in files)
        decoded = ingest.decode_jpeg(files, device=DEV)
        for f, d in zip(files, decoded):
            assert np.array_equal(d.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f))))


def test_write_jpeg_writes_pils_bytes_with_every_encoder(tmp_path):
    """The 4:2:0 corner is closed: an even height that is no multiple of 16 goes through the GPU under "auto" like any other."""
    a = cases.content(376, 64, "smooth", seed=5)
    want = cases.pil_bytes(a, 95, 2)
    for enc in ("gpu", "pil", "auto"):
        p = tmp_path / f"{enc}.jpg"
        jpeg.write_jpeg(p, dev(a), quality=95, subsampling=2, encoder=enc)
        assert p.read_bytes() == want, enc
    assert jpeg.choose_encoder("auto", a.shape, 2) == "gpu"
    jpeg.write_jpeg(tmp_path / "d.jpg", dev(a))
    assert (tmp_path / "d.jpg").read_bytes() == cases.pil_bytes(a, 95, 0)


def test_to_u8_rounds_as_the_float64_rule():
    rng = np.random.default_rng(4)
    k = np.arange(256, dtype=np.float64)
    edge = np.concatenate([(k + 0.5) / 255.0, np.nextafter((k + 0.5) / 255.0, -1), np.nextafter((k + 0.5) / 255.0, 2), k / 255.0,
                           [-1.0, -1e-9, 0.0, 1.0, 1.0 + 1e-6, 7.0, np.inf, -np.inf, np.nan]]).astype(np.float32)
    x = np.concatenate([edge, rng.uniform(-0.1, 1.1, 3 * 37 * 53 - edge.size).astype(np.float32)]).reshape(3, 37, 53)
    with np.errstate(all="ignore"):
        want = np.clip(np.floor(np.nan_to_num(x.astype(np.float64), nan=0.0) * 255 + 0.5), 0, 255).astype(np.uint8).transpose(1, 2, 0)
    got = jpeg.to_u8(torch.from_numpy(x).to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (37, 53, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    one = jpeg.to_u8(torch.from_numpy(x[:1].copy()).to(DEV))
    assert np.array_equal(one.cpu().numpy(), want[..., :1])
