"""CPU: the PNG checker of the GPU encoder's tests accepts what PIL writes and rejects corrupted files; the encoder's output bound
covers the stored fallback; the argument errors of topo4d_amd/png.py come before anything touches a device."""
import io
import struct
import zlib

import numpy as np
import pytest
import torch

from tests.png_check import PngError, chunks, check_png


def _pil_png(arr, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG", **kw)
    return b.getvalue()


def _rebuild(cs):
    out = b"\x89PNG\r\n\x1a\n"
    for t, p in cs:
        out += struct.pack(">I", len(p)) + t + p + struct.pack(">I", zlib.crc32(t + p))
    return out


@pytest.mark.parametrize("shape", [(1, 1), (7, 5, 3), (33, 20, 4), (16, 300)])
def test_checker_accepts_pil_files(shape):
    rng = np.random.default_rng(0)
    arr = rng.integers(0, 256, size=shape, dtype=np.uint8)
    got = check_png(_pil_png(arr))
    np.testing.assert_array_equal(got.reshape(arr.shape), arr)


def test_checker_rejects_bad_crc_adler_and_order():
    arr = np.random.default_rng(1).integers(0, 256, size=(40, 30, 3), dtype=np.uint8)
    good = _pil_png(arr)
    check_png(good)
    # a flipped CRC byte
    bad = bytearray(good)
    bad[8 + 4 + 4 + 13] ^= 0x01                       # IHDR's CRC
    with pytest.raises(PngError):
        check_png(bytes(bad))
    # a corrupted Adler-32 trailer (chunk CRCs recomputed, so only zlib can notice)
    cs = chunks(good)
    stream = b"".join(p for t, p in cs if t == b"IDAT")
    stream = stream[:-1] + bytes([stream[-1] ^ 0xFF])
    others = [(t, p) for t, p in cs if t != b"IDAT"]
    with pytest.raises(PngError, match="zlib"):
        check_png(_rebuild([others[0], (b"IDAT", stream)] + others[1:]))
    # IEND before the IDAT, and IDATs split by another chunk
    with pytest.raises(PngError):
        check_png(_rebuild([cs[0], (b"IEND", b"")] + [c for c in cs[1:] if c[0] != b"IEND"]))
    idat = [p for t, p in cs if t == b"IDAT"][0]
    split = [cs[0], (b"IDAT", idat[:10]), (b"tEXt", b"k\x00v"), (b"IDAT", idat[10:]), (b"IEND", b"")]
    with pytest.raises(PngError, match="consecutive"):
        check_png(_rebuild(split))
    check_png(_rebuild([cs[0], (b"IDAT", idat[:10]), (b"IDAT", idat[10:]), (b"IEND", b"")]))


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 70000, 1), (70000, 1, 3), (40, 30000, 3), (1024, 1024, 4), (8192, 8192, 3)])
def test_max_encoded_bytes_covers_stored_blocks(shape):
    from topo4d_amd.png import max_encoded_bytes
    h, w, c = shape
    raw = h * (1 + w * c)
    stored = raw + 5 * -(-raw // 65535)               # deflate's own stored-block framing
    framing = 8 + 25 + 12                             # signature, IHDR, IEND
    bound = max_encoded_bytes(h, w, c)
    assert bound >= stored + framing + 12 + 6         # + at least one IDAT with the zlib header and trailer
    assert bound <= raw * 1.01 + 4096                 # and not absurdly loose
    assert max_encoded_bytes(h, w, c) == bound        # a function of the shape alone


def test_argument_errors_without_a_device():
    from topo4d_amd import png
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.encode_png(torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        png.encode_png(torch.zeros(4, 4, dtype=torch.float32))
    for bad in (torch.zeros(4, 4, 3, dtype=torch.float64), torch.zeros(4, 4, 3, dtype=torch.int32),
                torch.zeros(4, 4, 2, dtype=torch.uint8), torch.zeros(4, 4, 5, dtype=torch.uint8),
                torch.zeros(16, dtype=torch.uint8), torch.zeros(2, 4, 4, 3, dtype=torch.uint8),
                torch.zeros(0, 4, 3, dtype=torch.uint8), np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            png.encode_png(bad)
    for shape in ((4, 4, 2), (0, 4, 3), (4, 0, 1)):
        with pytest.raises(ValueError):
            png.max_encoded_bytes(*shape)


def test_c_abi_rejects_bad_arguments():
    import ctypes as C
    from topo4d_amd import _lib
    lib = _lib.load()
    one = C.c_void_p(64)                              # never dereferenced by a call that is rejected
    cap = lib.t4d_png_max_bytes(8, 8, 3)
    sb = lib.t4d_png_scratch_bytes(8, 8, 3)
    assert cap > 0 and sb > 0
    assert lib.t4d_png_max_bytes(8, 8, 2) == 0 and lib.t4d_last_error()
    assert lib.t4d_png_scratch_bytes(0, 8, 3) == 0
    enc = lib.t4d_png_encode
    assert enc(None, 0, 8, 8, 3, one, cap, one, one, sb, None) == _lib.T4D_ERR_ARG
    assert enc(one, 2, 8, 8, 3, one, cap, one, one, sb, None) == _lib.T4D_ERR_ARG
    assert enc(one, 0, 8, 8, 2, one, cap, one, one, sb, None) == _lib.T4D_ERR_ARG
    assert enc(one, 0, 8, 8, 3, one, cap - 1, one, one, sb, None) == _lib.T4D_ERR_ARG
    assert enc(one, 0, 8, 8, 3, one, cap, None, one, sb, None) == _lib.T4D_ERR_ARG
    assert enc(one, 0, 8, 8, 3, one, cap, one, one, sb - 1, None) == _lib.T4D_ERR_STATE_SIZE
