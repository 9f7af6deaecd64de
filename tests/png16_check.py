"""A strict decoder of 16-bit PNG files, for the tests of png.encode_png16 (tests/png_check.py is its 8-bit counterpart and asserts
depth 8).  The decoder is the oracle: no golden.

decode_png16(data) parses the file with struct and asserts the signature, the IHDR fields (bit depth 16, no interlace, colour type
0 / 2 / 6), every chunk's CRC-32, that the IDAT chunks are consecutive and IEND is last, and that zlib.decompress of the joined IDAT
payload succeeds (which checks the Adler-32 trailer) with H * (1 + 2 W C) bytes whose filter bytes are in 0..4.  It then undoes the
five filters itself at a byte distance of bpp = 2 C and reads the samples high byte first.  Returns (array int32 [H,W,C], filter
bytes uint8 [H])."""
import struct
import zlib

import numpy as np

from tests.png_check import CHANNELS, PngError, _need, chunks


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def unfilter(raw: bytes, h: int, stride: int, bpp: int):
    """(bytes uint8 [h, stride], filter bytes [h]) of the filtered rows `raw` (h rows of 1 + stride bytes)"""
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + stride)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for y in range(h):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        else:                                                   # 1, 3, 4 look back within the row: byte by byte
            cur = np.zeros(stride, np.int64)
            for x in range(stride):
                a = int(cur[x - bpp]) if x >= bpp else 0
                b = int(prev[x])
                c = int(prev[x - bpp]) if x >= bpp else 0
                pred = a if f == 1 else ((a + b) >> 1) if f == 3 else _paeth(a, b, c)
                cur[x] = (int(line[x]) + pred) & 255
        out[y] = cur
        prev = cur
    return out, rows[:, 0].copy()


def decode_png16(data: bytes):
    cs = chunks(data)
    _need(cs and cs[0][0] == b"IHDR" and len(cs[0][1]) == 13, "IHDR must come first with 13 bytes")
    w, h, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    _need(w >= 1 and h >= 1, "empty image")
    _need(depth == 16 and ctype in CHANNELS and comp == 0 and filt == 0 and interlace == 0, f"unexpected IHDR {cs[0][1]!r}")
    c = CHANNELS[ctype]
    _need(cs[-1] == (b"IEND", b""), "IEND must be last and empty")
    types = [t for t, _ in cs]
    _need(types.count(b"IEND") == 1 and types.count(b"IHDR") == 1, "one IHDR and one IEND")
    idat = [i for i, t in enumerate(types) if t == b"IDAT"]
    _need(idat and idat == list(range(idat[0], idat[-1] + 1)), "IDAT chunks must be consecutive")
    stream = b"".join(cs[i][1] for i in idat)
    try:
        raw = zlib.decompress(stream)                         # checks the zlib header, every block and the Adler-32
    except zlib.error as e:
        raise PngError(f"zlib: {e}") from e
    stride = 2 * w * c
    _need(len(raw) == h * (1 + stride), f"decompressed {len(raw)} bytes, expected {h * (1 + stride)}")
    _need(int(np.frombuffer(raw, np.uint8)[::1 + stride].max()) <= 4, "filter byte out of range")
    by, filters = unfilter(raw, h, stride, 2 * c)
    samples = by.reshape(h, w, c, 2).astype(np.int32)
    return samples[..., 0] * 256 + samples[..., 1], filters


def best_filters(image) -> np.ndarray:
    """The filter byte the encoder's rule picks for every row of an int [H,W,C] image of 16-bit samples: the least sum of |int8
    residual| over the row's 2 W C big-endian bytes, the lowest filter number on a tie."""
    from tests import png_ref                                 # one statement of the filter rule for 8 and 16 bits
    by, bpp, _ = png_ref.image_bytes(np.asarray(image), 16)
    return png_ref.filter_rows(by, bpp)[0]
