"""PNG files written by hand for the decoder's tests (tests/test_pngdec_host.py, tests/test_gpu_pngdec.py): numpy rows filtered with a
filter type chosen per row, a zlib or hand-made deflate stream, an arbitrary IDAT cut list, correct CRCs.  PIL's writer cannot be
made to produce most of these.  Everything is deterministic (seeded), built once per process (valid_cases, malformed_cases)."""
import functools
import io
import struct
import zlib
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

KINDS = {"grey8": (0, 8, 1), "grey16": (0, 16, 1), "greyalpha": (4, 8, 2), "rgb": (2, 8, 3), "rgba": (6, 8, 4)}   # colour type, depth, channels
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 64), (65, 63), (130, 129)]
SEG = 16384

# status bits of include/topo4d_raster.h
ERR_END, ERR_BLOCK, ERR_TABLE, ERR_CODE, ERR_LENGTH, ERR_FILTER, ERR_ADLER = 1, 2, 4, 8, 16, 32, 64


class Case(NamedTuple):
    name: str
    data: bytes
    path: Optional[int]          # the schedule the decoder must report: 1 chunk-parallel, 2 serial, None: either


class Bad(NamedTuple):
    name: str
    data: bytes
    bit: int
    pil_refuses: bool = True     # False: PIL stops reading once it has every row, or pads missing rows, and returns an array


# ---- pixels and rows --------------------------------------------------------------------------------------------------------------
def pixels(kind: str, h: int, w: int, seed: int, edges: bool = False) -> np.ndarray:
    """the array np.array(Image.open(file)) must give: uint8 [h,w] / [h,w,c] or uint16 [h,w]; edges: samples from {0, 1, 254, 255}
    (in both bytes of a 16-bit sample), so that Paeth ties and Average carries occur"""
    _, depth, c = KINDS[kind]
    rng = np.random.default_rng(seed)
    shape = (h, w) if c == 1 else (h, w, c)
    if depth == 16:
        raw = rng.choice(np.array([0, 1, 254, 255], np.uint8), (h, w, 2)) if edges else rng.integers(0, 256, (h, w, 2), np.uint8)
        return (raw[..., 0].astype(np.uint16) << 8) | raw[..., 1]
    if edges:
        return rng.choice(np.array([0, 1, 254, 255], np.uint8), shape)
    # smooth ramps plus noise: compressible, with matches at many distances
    base = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5) % 251).astype(np.uint8)
    img = base if c == 1 else np.stack([(base + 40 * k) for k in range(c)], -1).astype(np.uint8)
    noise = rng.integers(0, 4, shape, np.uint8) * (rng.random(shape) < 0.3)
    return (img + noise).astype(np.uint8)


def row_bytes(img: np.ndarray) -> np.ndarray:
    """uint8 [h, w*bpp]: the rows as the stream holds them (16-bit samples high byte first)"""
    if img.dtype == np.uint16:
        return img.astype(">u2").view(np.uint8).reshape(img.shape[0], -1)
    return img.reshape(img.shape[0], -1)


def _paeth(a, b, c):
    p = a.astype(np.int32) + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows: np.ndarray, bpp: int, filters: Sequence[int]) -> bytes:
    """the filtered byte stream: per row its filter byte, then the row filtered with it (filters above 4 are written as they are,
    with the row unfiltered)"""
    h, n = rows.shape
    out = bytearray()
    prev = np.zeros(n, np.int32)
    for y in range(h):
        cur = rows[y].astype(np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if n > bpp else np.zeros(n, np.int32)
        f = int(filters[y])
        pred = {1: a, 2: prev, 3: (a + prev) >> 1, 4: _paeth(a, prev, c)}.get(f, 0)
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


# ---- chunks -----------------------------------------------------------------------------------------------------------------------
def chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png_file(w: int, h: int, depth: int, color_type: int, payloads: Sequence[bytes], interlace: int = 0, before: bytes = b"",
             compression: int = 0, filter_method: int = 0) -> bytes:
    """signature, IHDR, `before` (whole chunks), one IDAT per payload, IEND"""
    ihdr = struct.pack(">IIBBBBB", w, h, depth, color_type, compression, filter_method, interlace)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + before + b"".join(chunk(b"IDAT", p) for p in payloads) + chunk(b"IEND", b"")


def cut(stream: bytes, sizes: Sequence[int]) -> List[bytes]:
    """the stream cut into payloads of these sizes (0 allowed), the rest as the last one"""
    out, at = [], 0
    for s in sizes:
        out.append(stream[at:at + s])
        at += s
    out.append(stream[at:])
    return out


def adler(data: bytes) -> bytes:
    return struct.pack(">I", zlib.adler32(data))


# ---- deflate streams --------------------------------------------------------------------------------------------------------------
def zlib_stream(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


def flushed_payloads(data: bytes, flush: int, seg: int = SEG, pieces: int = 1, level: int = 6) -> List[bytes]:
    """project-like payloads: the zlib header, one payload per `seg` bytes from one raw-deflate compressor closed with `flush`
    (Z_FULL_FLUSH: self-contained; Z_SYNC_FLUSH: aligned, but with references into earlier payloads), the Adler-32 trailer.
    pieces: flushes per payload (several blocks per chunk)."""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    out = [b"\x78\x01"]
    for at in range(0, len(data), seg):
        part = data[at:at + seg]
        last = at + seg >= len(data)
        step = -(-len(part) // pieces)
        body = b""
        for k in range(0, len(part), step):
            body += c.compress(part[k:k + step])
            body += c.flush(zlib.Z_FINISH if last and k + step >= len(part) else flush)
        out.append(body)
    out.append(adler(data))
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value: int, count: int):             # LSB first
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value: int, count: int):             # a Huffman code: most significant bit first
        self.bits(int(format(value, f"0{count}b")[::-1], 2), count)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self) -> bytes:
        self.align()
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _fixed_symbol(w: BitWriter, s: int):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def fixed_block(w: BitWriter, data: bytes, start: int, end: int, matches: dict, final: bool):
    """data[start:end) as one fixed-Huffman block: literals, and at the positions of `matches` {pos: (length, distance)} that match"""
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    i = start
    while i < end:
        if i in matches:
            ln, dist = matches[i]
            assert i + ln <= end and dist <= i and all(data[i + k] == data[i - dist + k % dist] for k in range(ln)), (i, ln, dist)
            li = max(k for k in range(29) if _LEN_BASE[k] <= ln) if ln < 258 else 28
            _fixed_symbol(w, 257 + li)
            w.bits(ln - _LEN_BASE[li], _LEN_EXTRA[li])
            di = max(k for k in range(30) if _DIST_BASE[k] <= dist)
            w.code(di, 5)
            w.bits(dist - _DIST_BASE[di], _DIST_EXTRA[di])
            i += ln
        else:
            _fixed_symbol(w, data[i])
            i += 1
    _fixed_symbol(w, 256)


def stored_block(w: BitWriter, body: bytes, final: bool, nlen: Optional[int] = None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(body), 16)
    w.bits((len(body) ^ 0xFFFF) if nlen is None else nlen, 16)
    w.out += body


def wrap(deflate: bytes, data: bytes) -> bytes:
    """a zlib stream around a raw deflate stream that inflates to `data`"""
    return b"\x78\x01" + deflate + adler(data)


# ---- the files --------------------------------------------------------------------------------------------------------------------
def make(kind: str, img: np.ndarray, filters, payloads_of) -> bytes:
    """the file of `img` with these row filters; payloads_of(filtered bytes) -> the IDAT payloads"""
    ct, depth, c = KINDS[kind]
    rows = row_bytes(img)
    filt = filter_rows(rows, c * depth // 8, filters)
    return png_file(img.shape[1], img.shape[0], depth, ct, payloads_of(filt))


def one_idat(level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    return lambda filt: [zlib_stream(filt, level, strategy)]


def mixed_filters(h: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 5, h)


def pil_file(img: np.ndarray) -> bytes:
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG")
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def valid_cases() -> List[Case]:
    out: List[Case] = []
    seed = 0
    # shapes and kinds: one zlib stream, one IDAT, a random filter per row
    for kind in KINDS:
        for (h, w) in SHAPES:
            seed += 1
            out.append(Case(f"{kind}-{h}x{w}", make(kind, pixels(kind, h, w, seed), mixed_filters(h, seed), one_idat()), 2))
    # filters, on content from {0, 1, 254, 255}
    for kind in ("rgb", "grey16", "greyalpha"):
        h, w = 65, 63
        img = pixels(kind, h, w, 100, edges=True)
        for f in range(5):
            out.append(Case(f"filter{f}-{kind}", make(kind, img, [f] * h, one_idat()), 2))
        out.append(Case(f"filter-mix-{kind}", make(kind, img, mixed_filters(h, 101), one_idat()), 2))
    for kind in ("rgb", "grey8", "rgba"):
        img = pixels(kind, 130, 129, 102, edges=True)
        out.append(Case(f"paeth-band-130-{kind}", make(kind, img, [4] * 130, one_idat()), 2))
        f = np.random.default_rng(103).integers(2, 5, 130)
        f[[0, 63, 64, 65]] = [0, 1, 0, 1]
        out.append(Case(f"band-starts-0-63-64-65-{kind}", make(kind, img, f, one_idat()), 2))
        f2 = np.random.default_rng(104).integers(2, 5, 130)                 # row 0 under filters 2..4: the row above is zeros
        out.append(Case(f"one-band-mixed-{kind}", make(kind, img, f2, one_idat()), 2))
    # inflate
    big = pixels("rgba", 130, 129, 200)                                      # 130 * 517 = 67,210 filtered bytes
    smooth = pixels("rgb", 100, 120, 201)                                    # 100 * 361 = 36,100: three 16 KiB segments
    for name, level, strategy in (("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("dynamic", 6, zlib.Z_DEFAULT_STRATEGY),
                                  ("huffman-only", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE), ("level9", 9, zlib.Z_DEFAULT_STRATEGY)):
        out.append(Case(f"zlib-{name}", make("rgb", smooth, mixed_filters(100, 202), one_idat(level, strategy)), 2))

    def stored_blocks(filt):                                                 # stored blocks of 65,535, 0 and the rest
        w = BitWriter()
        stored_block(w, filt[:65535], False)
        stored_block(w, b"", False)
        stored_block(w, filt[65535:], True)
        return [wrap(w.done(), filt)]
    out.append(Case("stored-65535-0-rest", make("rgba", big, [0] * 130, stored_blocks), 2))
    out.append(Case("stored-cut-by-idat", make("rgba", big, [1] * 130, lambda f: cut(stored_blocks(f)[0], [2, 30000, 0, 35539])), 2))

    def long_matches(filt):                                                  # fixed Huffman, matches zlib itself never emits
        w = BitWriter()
        m = {32768: (258, 32768), 40000: (258, 3), 41000: (3, 1), 42000: (258, 1)}
        fixed_block(w, filt, 0, len(filt), m, True)
        return [wrap(w.done(), filt)]
    img = pixels("rgba", 130, 129, 203).copy()
    flat = img.reshape(130, -1)
    stream = np.concatenate([np.zeros((130, 1), np.uint8), flat], 1).reshape(-1)   # filter 0 everywhere: the stream is the pixels
    stream[32768:33026] = stream[0:258]
    stream[39997:40258] = np.resize(np.array([9, 200, 31], np.uint8), 261)
    stream[40999:41003] = 77
    stream[41999:42258] = 5
    stream[::517] = 0
    img = stream.reshape(130, 517)[:, 1:].reshape(130, 129, 4)
    out.append(Case("match-258-at-32768-and-3", make("rgba", img, [0] * 130, long_matches), 2))
    period = np.resize(np.array([1, 2, 3], np.uint8), 130 * 129 * 4).reshape(130, 129, 4)
    out.append(Case("level9-period-3", make("rgba", period, [0] * 130, one_idat(9)), 2))
    # a skewed histogram: Fibonacci counts, shuffled, Huffman only -> codes of the maximum length, 15 bits
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    vals = np.repeat(np.arange(1, 22, dtype=np.uint8), fib)                  # 28,656 bytes
    np.random.default_rng(204).shuffle(vals)
    skew = np.resize(vals, 130 * 129 * 2).reshape(130, 129, 2)
    out.append(Case("skewed-15-bit-codes", make("greyalpha", skew, [0] * 130, one_idat(9, zlib.Z_HUFFMAN_ONLY)), 2))
    small = pixels("rgb", 5, 64, 205)
    out.append(Case("idat-1-byte-each", make("rgb", small, mixed_filters(5, 206), lambda f: [bytes([b]) for b in zlib_stream(f)]), 2))
    out.append(Case("idat-empty-between", make("rgb", small, mixed_filters(5, 206),
                                               lambda f: [x for p in cut(zlib_stream(f), [1, 1, 5, 100]) for x in (b"", p, b"")]), 2))
    # schedules
    for kind in KINDS:
        img = pixels(kind, 100, 120, 300)
        out.append(Case(f"project-like-{kind}", make(kind, img, mixed_filters(100, 301), lambda f: flushed_payloads(f, zlib.Z_FULL_FLUSH)), 1))
    out.append(Case("project-like-several-blocks", make("rgb", smooth, mixed_filters(100, 302),
                                                        lambda f: flushed_payloads(f, zlib.Z_FULL_FLUSH, pieces=4)), 1))
    out.append(Case("project-like-stored", make("rgb", smooth, mixed_filters(100, 303),
                                                lambda f: flushed_payloads(f, zlib.Z_FULL_FLUSH, level=0)), 1))
    out.append(Case("project-like-empty-idats", make("rgb", smooth, mixed_filters(100, 304),
                                                     lambda f: [x for p in flushed_payloads(f, zlib.Z_FULL_FLUSH) for x in (p, b"")]), 1))
    out.append(Case("project-like-one-segment", make("grey8", pixels("grey8", 7, 1, 305), [4] * 7,
                                                     lambda f: flushed_payloads(f, zlib.Z_FULL_FLUSH)), 1))
    out.append(Case("sync-flushed", make("rgb", smooth, mixed_filters(100, 306), lambda f: flushed_payloads(f, zlib.Z_SYNC_FLUSH)), 2))
    noise = np.random.default_rng(307).integers(0, 256, (260, 300, 3), np.uint8)
    out.append(Case("pil-several-idats", pil_file(noise), 2))                # PIL cuts at 65,536 bytes, not at block boundaries
    out.append(Case("pil-small", pil_file(pixels("rgb", 65, 63, 308)), 2))
    out.append(Case("pil-grey16", pil_file(pixels("grey16", 65, 63, 309)), 2))
    # ancillary chunks are skipped
    text = chunk(b"tEXt", b"Comment\x00by hand") + chunk(b"gAMA", struct.pack(">I", 45455))
    ct, depth, c = KINDS["rgb"]
    filt = filter_rows(row_bytes(small), 3, [2] * 5)
    out.append(Case("ancillary-chunks", png_file(64, 5, depth, ct, [zlib_stream(filt)], before=text), 2))
    return out


@functools.lru_cache(maxsize=None)
def malformed_cases() -> List[Bad]:
    """files the decoder rejects, each with the status bit it reports; PIL refuses them too, but for the three marked: a stream that
    inflates to more or fewer bytes than the image, and a wrong Adler-32 in an IDAT of its own, which PIL never reads"""
    out: List[Bad] = []
    img = pixels("rgb", 40, 30, 400)                                         # 40 * 91 = 3,640 filtered bytes
    filt = filter_rows(row_bytes(img), 3, mixed_filters(40, 401))
    file_of = lambda payloads: png_file(30, 40, 8, 2, payloads)
    good = zlib_stream(filt)
    out.append(Bad("truncated-mid-block", file_of([good[:len(good) // 2]]), ERR_END))
    out.append(Bad("truncated-project-like", file_of(flushed_payloads(filt, zlib.Z_FULL_FLUSH, seg=1024)[:3]), ERR_END))
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2)                                               # fixed block, first symbol a match of 3 at distance 1
    _fixed_symbol(w, 257); w.code(0, 5); _fixed_symbol(w, 256)
    out.append(Bad("distance-before-start", file_of([wrap(w.done(), filt)]), ERR_CODE))
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
    for k in range(19):
        w.bits(1 if k < 3 else 0, 3)                                         # three code-length codes of 1 bit
    w.bits(0, 32)
    out.append(Bad("table-over-subscribed", file_of([wrap(w.done(), filt)]), ERR_TABLE))
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(14, 4)
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1):
        w.bits({0: 1, 1: 2, 18: 2}.get(s, 0), 3)
    w.code(2, 2); w.code(2, 2)                                               # lengths 1, 1
    w.code(3, 2); w.bits(127, 7); w.code(3, 2); w.bits(106, 7)               # 138 + 117 zeros: symbol 256 has no code
    w.code(2, 2)                                                             # one distance code of 1 bit
    w.bits(0, 32)
    out.append(Bad("table-without-256", file_of([wrap(w.done(), filt)]), ERR_TABLE))
    w = BitWriter()
    stored_block(w, filt, True, nlen=0x1234)
    out.append(Bad("len-nlen-mismatch", file_of([wrap(w.done(), filt)]), ERR_BLOCK))
    out.append(Bad("inflates-longer", file_of([zlib_stream(filt + b"\x00" * 91)]), ERR_END, False))
    out.append(Bad("inflates-shorter", file_of([zlib_stream(filt[:-91])]), ERR_LENGTH, False))
    flipped = bytearray(good)
    flipped[-2] ^= 0x40
    out.append(Bad("adler-flipped", file_of([bytes(flipped)]), ERR_ADLER))
    payloads = flushed_payloads(filt, zlib.Z_FULL_FLUSH, seg=1024)
    payloads[-1] = bytes([payloads[-1][0] ^ 1]) + payloads[-1][1:]
    out.append(Bad("adler-flipped-project-like", file_of(payloads), ERR_ADLER, False))
    five = bytearray(filt)
    five[91 * 17] = 5
    out.append(Bad("filter-byte-5", file_of([zlib_stream(bytes(five))]), ERR_FILTER))
    out.append(Bad("filter-byte-5-project-like", file_of(flushed_payloads(bytes(five), zlib.Z_FULL_FLUSH, seg=1024)), ERR_FILTER))
    return out


def refused_cases() -> List[tuple]:
    """(name, file, a word of parse_png's reason): well-formed files the GPU decoder does not take"""
    from PIL import Image
    rng = np.random.default_rng(500)
    out = []

    def saved(im, **kw):
        b = io.BytesIO()
        im.save(b, "PNG", **kw)
        return b.getvalue()
    out.append(("palette", saved(Image.fromarray(rng.integers(0, 256, (9, 11, 3), np.uint8)).convert("P")), "palette"))
    out.append(("one-bit", saved(Image.fromarray(rng.integers(0, 2, (9, 11), np.uint8) * 255).convert("1")), "1-bit"))
    rows16 = rng.integers(0, 256, (4, 5 * 6), np.uint8)
    out.append(("rgb16", png_file(5, 4, 16, 2, [zlib_stream(filter_rows(rows16, 6, [0] * 4))]), "16-bit"))
    out.append(("greyalpha16", png_file(5, 4, 16, 4, [zlib_stream(filter_rows(rows16[:, :20], 4, [0] * 4))]), "16-bit"))
    out.append(("interlaced", png_file(5, 4, 8, 0, [zlib_stream(b"\x00" * 64)], interlace=1), "interlaced"))
    out.append(("four-bit", png_file(6, 4, 4, 0, [zlib_stream(filter_rows(rng.integers(0, 256, (4, 3), np.uint8), 1, [0] * 4))]), "4-bit"))
    return out
