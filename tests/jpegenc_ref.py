"""A numpy restatement of the baseline JPEG encoder behind topo4d_amd.jpeg (csrc/t4d_jpegenc.hip, csrc/t4d_jpeg_fdct.h): libjpeg's
arithmetic in plain Python loops, for small shapes only.  The reference of every test is PIL's own `save`; this module exists so
that the rules are written down once in a form that can be read, and so that the host build of the per-block arithmetic
(tests/native/jpegenc_host.cpp) has coefficients to be compared with.

    quant_tables(quality)                     the two Annex K tables scaled by jpeg_set_quality, natural order
    header(h, w, quality, subsampling)        the 623 bytes before the entropy-coded segment
    raw_blocks(img, subsampling)              jfdctint's output per block in scan order: all that does not depend on the quality
    blocks(img, quality, subsampling)         [(component, quantised coefficients in natural order [64], dummy)] in scan order
    encode(img, quality, subsampling)         (file bytes, census)

It reproduces PIL's bytes for every shape tried, the 4:2:0 images of even height that is no multiple of 16 included: there the last
partial MCU row repeats the last downsampled chroma row (`planes`).

census: {"zrl", "stuffed", "dummy_right", "dummy_bottom", "max_category", "eob_only": blocks per component that are one EOB,
"blocks": blocks per component}.
"""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
          80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
          95, 98, 112, 100, 103, 99]
CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
            99, 99] + [99] * 32

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]

SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2)}           # luma (h, v) sampling factors; chroma is 1 x 1


def quant_tables(quality):
    """jpeg_set_quality(quality, force_baseline=TRUE): jpeg_quality_scaling, then (base * scale + 50) / 100 clamped to 1..255."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (LUMA_Q, CHROMA_Q))


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def header(h, w, quality, subsampling):
    """SOI, JFIF APP0 (1.01, no units, density 1 x 1), a DQT per table, SOF0, the four Annex K DHTs, SOS."""
    hs, vs = SAMPLING[subsampling]
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, t in enumerate(quant_tables(quality)):
        out += _segment(0xDB, [i] + [t[ZIGZAG[k]] for k in range(64)])
    out += _segment(0xC0, [8] + list(h.to_bytes(2, "big")) + list(w.to_bytes(2, "big")) + [3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls_id, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                               (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _segment(0xC4, [cls_id] + bits + vals)
    out += _segment(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return out


def huff_codes(bits, vals):
    """{symbol: (code, length)} of a DHT table (jpeg_make_c_derived_tbl)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


FIX = lambda x: int(x * 65536 + 0.5)


def ycc(img):
    """libjpeg's rgb_ycc_convert: three int64 planes."""
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    half = 1 << 15
    off = (128 << 16) + half - 1
    y = (FIX(0.29900) * r + FIX(0.58700) * g + FIX(0.11400) * b + half) >> 16
    cb = (-FIX(0.16874) * r - FIX(0.33126) * g + FIX(0.50000) * b + off) >> 16
    cr = (FIX(0.50000) * r - FIX(0.41869) * g - FIX(0.08131) * b + off) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def planes(img, subsampling):
    """The three component planes padded to whole MCUs: luma at full size, chroma downsampled (h2v1 / h2v2_downsample).
    Columns are edge-replicated to whole MCUs at full size, before the downsampling (expand_right_edge).  Rows are replicated
    at full size only up to a whole row group (an even number of rows in 4:2:0: pre_process_data's conversion buffer); the rows
    from there to the MCU's end are copies of the last DOWNSAMPLED row (expand_bottom_edge on the output).  In 4:2:0 with an
    even height the two differ: the last chroma row is the mean of rows H-2 and H-1, and that mean is what is repeated, not
    the downsampling of row H-1 alone."""
    hs, vs = SAMPLING[subsampling]
    h, w = img.shape[:2]
    rows, cols = -(-h // (8 * vs)) * 8 * vs, -(-w // (8 * hs)) * 8 * hs
    group = -(-h // vs) * vs
    y, cb, cr = (_pad(p, group, cols) for p in ycc(img))
    out = [_pad(y, rows, cols)]
    for c in (cb, cr):
        if subsampling == 1:
            bias = np.arange(cols // 2) & 1
            c = (c[:, 0::2] + c[:, 1::2] + bias) >> 1
        elif subsampling == 2:
            bias = 1 + (np.arange(cols // 2) & 1)
            c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_pad(c, rows // vs, c.shape[1]))
    return out


C = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069,
         f2053=16819, f2562=20995, f3072=25172)


def _fdct_1d(d, first):
    """One pass of jfdctint's jpeg_fdct_islow over 8 values (CONST_BITS 13, PASS1_BITS 2)."""
    desc = lambda x, n: (x + (1 << (n - 1))) >> n
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [0] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = desc(t10 + t11, 2), desc(t10 - t11, 2)
    n = 11 if first else 15
    z1 = (t12 + t13) * C["f0541"]
    o[2] = desc(z1 + t13 * C["f0765"], n)
    o[6] = desc(z1 - t12 * C["f1847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C["f1175"]
    t4, t5, t6, t7 = t4 * C["f0298"], t5 * C["f2053"], t6 * C["f3072"], t7 * C["f1501"]
    z1, z2, z3, z4 = -z1 * C["f0899"], -z2 * C["f2562"], -z3 * C["f1961"] + z5, -z4 * C["f0390"] + z5
    o[7], o[5], o[3], o[1] = desc(t4 + z1 + z3, n), desc(t5 + z2 + z4, n), desc(t6 + z2 + z3, n), desc(t7 + z1 + z4, n)
    return o


def fdct(block):
    """jfdctint's output (natural order, 8 times the DCT) for an 8 x 8 block of samples: rows, then columns, on samples - 128."""
    d = [[int(v) - 128 for v in row] for row in block]
    d = [_fdct_1d(row, True) for row in d]
    cols = [_fdct_1d([d[r][c] for r in range(8)], False) for c in range(8)]
    return [cols[c][r] for r in range(8) for c in range(8)]


def quantize(coef, table):
    """sign(c) * ((|c| + (8q >> 1)) // 8q) per coefficient."""
    out = []
    for v, q in zip(coef, table):
        m = (abs(v) + (8 * q >> 1)) // (8 * q)
        out.append(-m if v < 0 else m)
    return out


def raw_blocks(img, subsampling):
    """[(component, jfdctint output [64] or None for a dummy, dummy: None | "right" | "bottom")] in scan order: everything of
    `blocks` that does not depend on the quality."""
    hs, vs = SAMPLING[subsampling]
    h, w = img.shape[:2]
    pl = planes(np.asarray(img), subsampling)
    yw, yh = -(-w // 8), -(-h // 8)                       # the luma component's own block grid
    out = []
    for my in range(pl[0].shape[0] // (8 * vs)):
        for mx in range(pl[0].shape[1] // (8 * hs)):
            for k in range(hs * vs):
                bx, by = mx * hs + k % hs, my * vs + k // hs
                if by >= yh or bx >= yw:
                    out.append((0, None, "bottom" if by >= yh else "right"))
                else:
                    out.append((0, fdct(pl[0][by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]), None))
            for c in (1, 2):
                out.append((c, fdct(pl[c][my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]), None))
    return out


def blocks(img, quality, subsampling, raw=None):
    """[(component, quantised coefficients [64] natural order, dummy: None | "right" | "bottom")] in scan order.  A dummy block
    has zero AC terms and the DC of the block before it in the MCU.  raw: raw_blocks(img, subsampling), if already made."""
    tabs = quant_tables(quality)
    out = []
    for comp, coef, dummy in (raw if raw is not None else raw_blocks(np.asarray(img), subsampling)):
        if dummy:
            out.append((comp, [out[-1][1][0]] + [0] * 63, dummy))
        else:
            out.append((comp, quantize(coef, tabs[0 if comp == 0 else 1]), None))
    return out


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.stuffed = bytearray(), 0, 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put(0x7F, 8 - self.n)


def encode(img, quality, subsampling, raw=None):
    img = np.asarray(img)
    h, w = img.shape[:2]
    dc = [huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS)]
    ac = [huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS)]
    bw = _Bits()
    census = {"zrl": 0, "stuffed": 0, "dummy_right": 0, "dummy_bottom": 0, "max_category": 0, "eob_only": [0, 0, 0],
              "blocks": [0, 0, 0]}
    last = [0, 0, 0]

    def value(v):
        n = abs(v).bit_length()
        census["max_category"] = max(census["max_category"], n)
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    for comp, coef, dummy in blocks(img, quality, subsampling, raw):
        t = 0 if comp == 0 else 1
        census["blocks"][comp] += 1
        if dummy:
            census["dummy_" + dummy] += 1
        n, low = value(coef[0] - last[comp])
        last[comp] = coef[0]
        bw.put(*dc[t][n])
        bw.put(low, n)
        run = 0
        for k in range(1, 64):
            v = coef[ZIGZAG[k]]
            if v == 0:
                run += 1
                continue
            while run > 15:
                bw.put(*ac[t][0xF0])
                census["zrl"] += 1
                run -= 16
            n, low = value(v)
            bw.put(*ac[t][(run << 4) | n])
            bw.put(low, n)
            run = 0
        if run:
            bw.put(*ac[t][0x00])
            census["eob_only"][comp] += run == 63
    bw.flush()
    census["stuffed"] = bw.stuffed
    return header(h, w, quality, subsampling) + bytes(bw.out) + b"\xff\xd9", census
