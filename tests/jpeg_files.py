"""A writer of baseline JPEG files from quantised coefficient blocks, for the decoder's tests (topo4d_amd.ingest, csrc/t4d_jpeg.h):
every table, id, slot, segment order, restart interval and padding bit is the caller's, and every file comes with a census of what
its entropy-coded segment holds, so that a test can assert that a file exercises what its name says.  Built from the pieces of
tests/jpegenc_ref.py; PIL is not used.

    write_jpeg(width, height, sampling, blocks, quant, ...) -> (file bytes, census)
    split(data) / join(parts)                  a file as (segments before the scan, scan bytes, tail) and back
    REWRITES: {name: f(data) -> data}          header rewrites of any baseline file that leave its pixels unchanged
    NOT_TAKEN: {name: (f, reason)}             rewrites after which parse_jpeg(...).gpu is False, for the stated reason
    make_table({symbol: code length})          (bits, vals) of a DHT table with those code lengths
    exact_idct(coef, q)                        float64 IDCT of one dequantised block (no level shift)
    block_count(width, height, sampling)       blocks of the scan, and block_components(...) their components in scan order

census: data_bits (coded bits before the final padding), pad_bits (0..7), stuffed, max_dc_category, max_ac_category, zrl,
max_zrl_run (most ZRLs before one term), eob_only, end_at_63 (blocks whose last term is index 63: no EOB), full_ac (blocks with 63
nonzero AC terms), max_code_length, code_lengths (set of code lengths used), len9, len10, max_dequant (largest |coefficient * q|),
sample_min / sample_max (exact float64 IDCT over all blocks), blocks.
"""
import math

import numpy as np

from tests.jpegenc_ref import (AC_CHROMA_BITS, AC_CHROMA_VALS, AC_LUMA_BITS, AC_LUMA_VALS, DC_CHROMA_BITS, DC_LUMA_BITS, DC_VALS,
                               ZIGZAG, _Bits, _segment, huff_codes, quant_tables)

ANNEX_K = {(0, 0): (DC_LUMA_BITS, DC_VALS), (1, 0): (AC_LUMA_BITS, AC_LUMA_VALS),
           (0, 1): (DC_CHROMA_BITS, DC_VALS), (1, 1): (AC_CHROMA_BITS, AC_CHROMA_VALS)}
JFIF = b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])

_M = np.array([[(math.sqrt(0.125) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16) for u in range(8)]
               for x in range(8)])


def exact_idct(coef, q):
    """The real-valued 8 x 8 IDCT of coef * q (both natural order), before the +128 level shift."""
    f = (np.asarray(coef, np.float64) * np.asarray(q, np.float64)).reshape(8, 8)
    return _M @ f @ _M.T


def block_count(width, height, sampling):
    hs, vs = sampling
    return -(-width // (8 * hs)) * -(-height // (8 * vs)) * (hs * vs + 2)


def block_components(width, height, sampling):
    hs, vs = sampling
    mcu = [0] * (hs * vs) + [1, 2]
    return mcu * (block_count(width, height, sampling) // len(mcu))


def make_table(lengths):
    """(bits[16], vals) of the DHT table that gives each symbol of {symbol: code length} a code of that length, symbols of one
    length in the dict's order.  The caller keeps the lengths within the code space (no all-ones code)."""
    bits, vals = [0] * 16, []
    for length in range(1, 17):
        for s, l in lengths.items():
            if l == length:
                bits[length - 1] += 1
                vals.append(s)
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        assert not bits[length - 1] or code < (1 << length), "the table over-fills its code space"
        code <<= 1
    return bits, vals


class _Writer(_Bits):
    def __init__(self):
        super().__init__()
        self.bits = 0

    def put(self, code, length):
        self.bits += length
        super().put(code, length)

    def pad(self, bit):
        n = (8 - self.n) % 8
        if n:
            super().put((1 << n) - 1 if bit else 0, n)
        return n


def dqt_body(tq, table, sixteen=False):
    zz = [int(table[ZIGZAG[k]]) for k in range(64)]
    if sixteen:
        return bytes([0x10 | tq]) + b"".join(v.to_bytes(2, "big") for v in zz)
    return bytes([tq] + zz)


def dht_body(cls, slot, bits, vals):
    return bytes([(cls << 4) | slot] + list(bits) + list(vals))


def write_jpeg(width, height, sampling, blocks, quant, huff=None, *, comp_quant=(0, 1, 1), comp_dc=(0, 1, 1), comp_ac=(0, 1, 1),
               comp_ids=(1, 2, 3), quant16=False, layout=("jfif", "dqt", "sof", "dht", "dri"), merged=False, sof=0xC0, restart=0,
               pad_bit=1):
    """A baseline file.  sampling: the luma (h, v) factors.  blocks: quantised coefficients [64] in natural order with absolute
    DC, one per block of the scan in scan order (block_components gives their components).  quant: {id: [64] natural order};
    huff: {(class, slot): (bits, vals)} (default: Annex K in slots 0 and 1); comp_*: table ids and component ids of Y, Cb, Cr.
    layout: the order of the segments before SOS ("jfif", "dqt", "sof", "dht", "dri"; "dri" is written only with restart > 0);
    merged: all tables of a kind in one segment.  restart: MCUs per restart interval.  pad_bit: the value of the padding bits."""
    hs, vs = sampling
    huff = dict(ANNEX_K if huff is None else huff)
    comps = block_components(width, height, sampling)
    assert len(blocks) == len(comps), (len(blocks), len(comps))
    codes = {k: huff_codes(*v) for k, v in huff.items()}
    bw = _Writer()
    cen = dict(data_bits=0, pad_bits=0, stuffed=0, max_dc_category=0, max_ac_category=0, zrl=0, max_zrl_run=0, eob_only=0,
               end_at_63=0, full_ac=0, max_code_length=0, code_lengths=set(), max_dequant=0, sample_min=0.0, sample_max=0.0,
               blocks=len(blocks))

    def symbol(cls, slot, s):
        code, length = codes[(cls, slot)][s]
        cen["code_lengths"].add(length)
        bw.put(code, length)

    def value(v, n):
        bw.put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)

    bpm = hs * vs + 2
    last = [0, 0, 0]
    n_rst = 0
    for b, (coef, c) in enumerate(zip(blocks, comps)):
        if restart and b and b % (restart * bpm) == 0:
            bw.pad(pad_bit)
            bw.out += bytes([0xFF, 0xD0 + (n_rst & 7)])
            n_rst += 1
            last = [0, 0, 0]
        q = quant[comp_quant[c]]
        cen["max_dequant"] = max(cen["max_dequant"], max(abs(int(v) * int(t)) for v, t in zip(coef, q)))
        s = exact_idct(coef, q)
        cen["sample_min"], cen["sample_max"] = min(cen["sample_min"], float(s.min())), max(cen["sample_max"], float(s.max()))
        d = int(coef[0]) - last[c]
        last[c] = int(coef[0])
        n = abs(d).bit_length()
        cen["max_dc_category"] = max(cen["max_dc_category"], n)
        symbol(0, comp_dc[c], n)
        value(d, n)
        run = zrls = terms = 0
        for k in range(1, 64):
            v = int(coef[ZIGZAG[k]])
            if v == 0:
                run += 1
                continue
            terms += 1
            cen["max_zrl_run"] = max(cen["max_zrl_run"], run // 16)
            while run > 15:
                symbol(1, comp_ac[c], 0xF0)
                cen["zrl"] += 1
                run -= 16
            n = abs(v).bit_length()
            cen["max_ac_category"] = max(cen["max_ac_category"], n)
            symbol(1, comp_ac[c], (run << 4) | n)
            value(v, n)
            run = 0
        if run:
            symbol(1, comp_ac[c], 0x00)
            cen["eob_only"] += run == 63
        else:
            cen["end_at_63"] += 1
        cen["full_ac"] += terms == 63
    cen["data_bits"] = bw.bits
    cen["pad_bits"] = bw.pad(pad_bit)
    cen["stuffed"] = bw.stuffed
    cen["max_code_length"] = max(cen["code_lengths"])
    cen["len9"], cen["len10"] = 9 in cen["code_lengths"], 10 in cen["code_lengths"]

    tq_ids = sorted(quant)
    sof_body = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3])
    for c in range(3):
        sof_body += bytes([comp_ids[c], ((hs << 4) | vs) if c == 0 else 0x11, comp_quant[c]])
    out = b"\xff\xd8"
    for part in layout:
        if part == "jfif":
            out += _segment(0xE0, JFIF)
        elif part == "dqt":
            bodies = [dqt_body(t, quant[t], quant16) for t in tq_ids]
            out += _segment(0xDB, b"".join(bodies)) if merged else b"".join(_segment(0xDB, x) for x in bodies)
        elif part == "dht":
            bodies = [dht_body(cls, slot, *huff[(cls, slot)]) for (cls, slot) in sorted(huff, key=lambda k: (k[1], k[0]))]
            out += _segment(0xC4, b"".join(bodies)) if merged else b"".join(_segment(0xC4, x) for x in bodies)
        elif part == "sof":
            out += _segment(sof, sof_body)
        elif part == "dri":
            if restart:
                out += _segment(0xDD, restart.to_bytes(2, "big"))
        else:
            raise ValueError(part)
    sos = bytes([3])
    for c in range(3):
        sos += bytes([comp_ids[c], (comp_dc[c] << 4) | comp_ac[c]])
    out += _segment(0xDA, sos + bytes([0, 63, 0]))
    return out + bytes(bw.out) + b"\xff\xd9", cen


# ---- header rewrites ---------------------------------------------------------------------------------------------------------
def split(data):
    """([(marker, body)] of the segments after SOI up to and including SOS, scan bytes up to the marker that ends them, tail)."""
    assert data[:2] == b"\xff\xd8"
    pos, segs = 2, []
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        n = (data[pos + 2] << 8) | data[pos + 3]
        segs.append((m, data[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if m == 0xDA:
            break
    end = pos
    while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
        end += 1
    return segs, data[pos:end], data[end:]


def join(segs, scan, tail, fill=b""):
    return b"\xff\xd8" + b"".join(fill + _segment(m, body) for m, body in segs) + scan + tail


def _tables(segs):
    """The DQT tables {id: body of one table} and DHT tables {(class, slot): body}, last definition winning, and the rest."""
    dqt, dht, rest = {}, {}, []
    for m, body in segs:
        if m == 0xDB:
            i = 0
            while i < len(body):
                n = 129 if body[i] >> 4 else 65
                dqt[body[i] & 15] = body[i:i + n]
                i += n
        elif m == 0xC4:
            i = 0
            while i < len(body):
                n = 17 + sum(body[i + 1:i + 17])
                dht[(body[i] >> 4, body[i] & 15)] = body[i:i + n]
                i += n
        else:
            rest.append((m, body))
    return dqt, dht, rest


def _before(rest, marker, new):
    """`rest` with the segments `new` put in front of the first segment `marker`."""
    i = [m for m, _ in rest].index(marker)
    return rest[:i] + list(new) + rest[i:]


def _retable(data, order="sof_first", merged=False, sixteen=False, reverse=False):
    segs, scan, tail = split(data)
    dqt, dht, rest = _tables(segs)
    if sixteen:
        dqt = {t: (bytes([0x10 | t]) + b"".join(bytes([0, v]) for v in b[1:]) if not b[0] >> 4 else b) for t, b in dqt.items()}
    qs, hs = [dqt[t] for t in sorted(dqt)], [dht[k] for k in sorted(dht)]
    if reverse:
        qs, hs = qs[::-1], hs[::-1]
    if merged:
        new = [(0xDB, b"".join(qs)), (0xC4, b"".join(hs))]
    else:
        new = [(0xDB, b) for b in qs] + [(0xC4, b) for b in hs]
    if reverse:
        new = new[::-1]
    return join(_before(rest, 0xDA if order == "sof_first" else [m for m, _ in rest if 0xC0 <= m <= 0xC3][0], new), scan, tail)


def _thumbnail():
    n = block_count(8, 8, (1, 1))
    return write_jpeg(8, 8, (1, 1), [[3] + [0] * 63] * n, dict(enumerate(quant_tables(50))))[0]


def exif_and_com(data):
    """An EXIF APP1 holding a whole thumbnail JPEG (its own SOI, SOS and EOI) and a COM segment holding FF D9 FF DA."""
    segs, scan, tail = split(data)
    new = [(0xE1, b"Exif\x00\x00MM\x00\x2a\x00\x00\x00\x08\x00\x00\x00\x00\x00\x00" + _thumbnail()), (0xFE, b"end \xff\xd9\xff\xda here")]
    return join(segs[:1] + new + segs[1:], scan, tail)


def dqt_16bit(data):
    return _retable(data, order="dqt_first", sixteen=True)


def split_reversed_after_sof(data):
    """One table per segment, in reverse order (DHT before DQT, high ids first), all after the SOF."""
    return _retable(data, reverse=True)


def tables_merged(data):
    return _retable(data, order="dqt_first", merged=True)


def _renumber(data, jfif):
    """Quantisation ids 0, 1 -> 3, 2; Huffman slots 0, 1 -> 2, 3; SOF1; component ids 7, 200, 0."""
    segs, scan, tail = split(data)
    dqt, dht, rest = _tables(segs)
    qmap, hmap, ids = {0: 3, 1: 2}, {0: 2, 1: 3}, (7, 200, 0)
    out = []
    for m, body in rest:
        b = bytearray(body)
        if m in (0xC0, 0xC1):
            for c in range(3):
                b[6 + 3 * c] = ids[c]
                b[8 + 3 * c] = qmap[b[8 + 3 * c]]
            m = 0xC1
        elif m == 0xDA:
            for c in range(3):
                b[1 + 2 * c] = ids[c]
                b[2 + 2 * c] = (hmap[b[2 + 2 * c] >> 4] << 4) | hmap[b[2 + 2 * c] & 15]
        elif m == 0xE0 and not jfif:
            continue
        out.append((m, bytes(b)))
    new = [(0xDB, bytes([(b[0] & 0xF0) | qmap[t]]) + b[1:]) for t, b in sorted(dqt.items())]
    new += [(0xC4, bytes([(cls << 4) | hmap[slot]]) + b[1:]) for (cls, slot), b in sorted(dht.items())]
    return join(_before(out, 0xC1, new), scan, tail)


def renumbered_sof1(data):
    return _renumber(data, True)


def renumbered_sof1_no_jfif(data):
    return _renumber(data, False)


def separate_cr_tables(data):
    """Cr reads copies of Cb's tables from a quantisation id and Huffman slots of its own."""
    segs, scan, tail = split(data)
    dqt, dht, rest = _tables(segs)
    out = []
    for m, body in segs:
        b = bytearray(body)
        if m in (0xC0, 0xC1):
            cb_q = b[8 + 3]
            b[8 + 6] = 2
            out.append((0xDB, bytes([(dqt[cb_q][0] & 0xF0) | 2]) + dqt[cb_q][1:]))
        elif m == 0xDA:
            td, ta = b[4] >> 4, b[4] & 15
            b[6] = 0x22
            out.append((0xC4, bytes([0x02]) + dht[(0, td)][1:]))
            out.append((0xC4, bytes([0x12]) + dht[(1, ta)][1:]))
        out.append((m, bytes(b)))
    return join(out, scan, tail)


def dht_redefined(data):
    """Wrong tables (the other component's) in every slot first; the right ones, defined later, must win."""
    segs, scan, tail = split(data)
    dqt, dht, rest = _tables(segs)
    wrong = []
    for (cls, slot), b in sorted(dht.items()):
        other = dht.get((cls, 1 - slot))
        if other is not None:
            wrong.append((0xC4, bytes([(cls << 4) | slot]) + other[1:]))
    return join(segs[:1] + wrong + segs[1:], scan, tail)


def _dri(value):
    def f(data):
        """DRI `value` early in the header; a file with a restart interval of its own defines it again later."""
        segs, scan, tail = split(data)
        return join(segs[:1] + [(0xDD, value.to_bytes(2, "big"))] + segs[1:], scan, tail)
    return f


ADOBE = b"Adobe\x00\x64\x00\x00\x00\x00"


def _adobe(transform, jfif):
    def f(data):
        segs, scan, tail = split(data)
        segs = [s for s in segs if jfif or s[0] != 0xE0]
        i = 1 if segs[0][0] == 0xE0 else 0
        return join(segs[:i] + [(0xEE, ADOBE + bytes([transform]))] + segs[i:], scan, tail)
    return f


def bytes_after_eoi(data):
    return data + b"\x00\xff\xd8\xff\xda trailing \xff\xd9"


def ff_fill(data):
    segs, scan, tail = split(data)
    return join(segs, scan, tail, fill=b"\xff\xff\xff")


REWRITES = {
    "exif_and_com": exif_and_com, "dqt_16bit": dqt_16bit, "split_reversed_after_sof": split_reversed_after_sof,
    "tables_merged": tables_merged, "renumbered_sof1": renumbered_sof1, "renumbered_sof1_no_jfif": renumbered_sof1_no_jfif,
    "separate_cr_tables": separate_cr_tables, "dht_redefined": dht_redefined, "dri_0": _dri(0), "dri_65535": _dri(65535),
    "adobe_1_no_jfif": _adobe(1, False), "adobe_1_jfif": _adobe(1, True), "bytes_after_eoi": bytes_after_eoi, "ff_fill": ff_fill,
}


def rgb_ids_no_jfif(data):
    segs, scan, tail = split(data)
    out = []
    for m, body in segs:
        b = bytearray(body)
        if m == 0xE0:
            continue
        if m in (0xC0, 0xC1):
            b[6], b[9], b[12] = b"RGB"
        elif m == 0xDA:
            b[1], b[3], b[5] = b"RGB"
        out.append((m, bytes(b)))
    return join(out, scan, tail)


def ff_before_eoi(data):
    segs, scan, tail = split(data)
    return join(segs, scan, b"\xff" + tail)


NOT_TAKEN = {
    "adobe_0": (_adobe(0, True), "Adobe transform flag: not YCbCr"),
    "rgb_ids_no_jfif": (rgb_ids_no_jfif, "RGB components"),
    "ff_ff_d9": (ff_before_eoi, "the scan ends with FFFF, not EOI"),
}
