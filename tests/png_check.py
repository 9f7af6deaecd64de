"""A strict structural check of a PNG file, for the GPU encoder's tests (topo4d_amd/png.py).  The decoder is the oracle: no golden.

check_png(data) parses the file with struct and asserts the signature, the IHDR fields (8-bit, no interlace, colour type 0 / 2 / 6),
every chunk's CRC-32, that the IDAT chunks are consecutive and IEND is last, and that zlib.decompress of the joined IDAT payload
succeeds (which checks the Adler-32 trailer) with H*(1 + W*C) bytes whose filter bytes are in 0..4.  It returns PIL's decoded array.
"""
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 6: 4}


class PngError(AssertionError):
    pass


def _need(cond, msg):
    if not cond:
        raise PngError(msg)


def chunks(data: bytes):
    """[(type, payload)] of a PNG file, every CRC checked."""
    _need(data[:8] == SIGNATURE, "bad signature")
    out, pos = [], 8
    while pos < len(data):
        _need(pos + 12 <= len(data), "truncated chunk header")
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        ctype = data[pos + 4:pos + 8]
        _need(pos + 12 + length <= len(data), f"chunk {ctype!r} runs past the end")
        payload = data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        _need(zlib.crc32(ctype + payload) == crc, f"bad CRC in chunk {ctype!r} at byte {pos}")
        out.append((ctype, payload))
        pos += 12 + length
    return out


def check_png(data: bytes) -> np.ndarray:
    cs = chunks(data)
    _need(cs and cs[0][0] == b"IHDR" and len(cs[0][1]) == 13, "IHDR must come first with 13 bytes")
    w, h, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    _need(w >= 1 and h >= 1, "empty image")
    _need(depth == 8 and ctype in CHANNELS and comp == 0 and filt == 0 and interlace == 0, f"unexpected IHDR {cs[0][1]!r}")
    c = CHANNELS[ctype]
    _need(cs[-1] == (b"IEND", b""), "IEND must be last and empty")
    types = [t for t, _ in cs]
    _need(types.count(b"IEND") == 1 and types.count(b"IHDR") == 1, "one IHDR and one IEND")
    idat = [i for i, t in enumerate(types) if t == b"IDAT"]
    _need(idat and idat == list(range(idat[0], idat[-1] + 1)), "IDAT chunks must be consecutive")
    stream = b"".join(cs[i][1] for i in idat)
    try:
        raw = zlib.decompress(stream)                     # checks the zlib header, every block and the Adler-32
    except zlib.error as e:
        raise PngError(f"zlib: {e}") from e
    row = 1 + w * c
    _need(len(raw) == h * row, f"decompressed {len(raw)} bytes, expected {h * row}")
    filters = np.frombuffer(raw, np.uint8)[::row]
    _need(int(filters.max()) <= 4, "filter byte out of range")
    from PIL import Image
    img = np.asarray(Image.open(io.BytesIO(data)))
    return img.reshape(h, w, c)
