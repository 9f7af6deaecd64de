"""Designed baseline JPEG files for the decoder's tests (tests/test_jpeg_files_host.py on the host build of csrc/t4d_jpeg.h,
tests/test_gpu_jpeg_files.py on the GPU), written by tests/jpeg_files.py.  Every image is at most 96 x 72.  Each case states the
census facts it claims as {census key: (op, value)}, op one of "eq", "ge", "le"; test_claims asserts them, so no case proves less
than its name says.  Every case but beyond_range() also keeps the range condition under which the decoder equals PIL (t4d_jpeg.h,
range_limit): exact IDCT samples within +-500 and |coefficient * q| below 32768.

    block_cases()       blocks: single coefficients, DC swings, AC category 10, ZRLs, EOB-only, full and dense blocks, each under
                        three samplings and four quantisation tables
    table_cases()       Huffman and quantisation tables, ids and slots
    padding_cases()     zero padding bits, and every padding length 0..7
    chunk_cases()       files with chunk sizes whose boundary falls strictly inside the padding bits
    fallback_cases()    (case, chunk_bits, whether the chunk lanes need the sequential fallback)
    header_cases()      the REWRITES and NOT_TAKEN variants of three designed base files and three from PIL's encoder
    beyond_range()      one file outside the range condition, where libjpeg's C wrap and PIL's saturation differ
    corrupted(seed)     corrupted entropy-coded segments and refused-table descriptors of valid files
"""
import functools
from collections import namedtuple

import numpy as np

from tests import jpeg_files as jf
from tests.jpegenc_ref import (AC_CHROMA_BITS, AC_CHROMA_VALS, AC_LUMA_BITS, AC_LUMA_VALS, DC_CHROMA_BITS, DC_LUMA_BITS, DC_VALS,
                               ZIGZAG, quant_tables)

Case = namedtuple("Case", "name data census claims")

SAMPLINGS = [(1, 1), (2, 1), (2, 2)]
RANGE = 500.0
QUANTS = {"ones": ([1] * 64, [1] * 64), "q50": quant_tables(50), "q10": quant_tables(10), "all255": ([255] * 64, [255] * 64)}
RANGE_CLAIMS = {"sample_min": ("ge", -RANGE), "sample_max": ("le", RANGE), "max_dequant": ("le", 32767)}


def in_range(block, q):
    s = jf.exact_idct(block, q)
    return max(-s.min(), s.max()) <= RANGE and np.abs(np.asarray(block, np.int64) * np.asarray(q, np.int64)).max() < 32768


def largest(unit, q, cap):
    """The largest m <= cap for which m * unit (one nonzero coefficient) keeps the range condition; at least 1."""
    k = int(np.flatnonzero(unit)[0])
    amp = np.abs(jf.exact_idct(unit, q)).max()
    m = max(1, min(cap, int(RANGE / amp), 32767 // q[k]))
    while m > 1 and not in_range([m * v for v in unit], q):
        m -= 1
    return m


# ---- block recipes: f(q of the block's component, index of the block within its component) -> coefficients [64], natural order
def single(pos, sign, big):
    def f(q, j):
        unit = [0] * 64
        unit[pos] = sign
        m = largest(unit, q, 1023) if big else 1
        return [m * v for v in unit]
    return f


def dc_swing(q, j):
    unit = [1] + [0] * 63
    m = largest(unit, q, 1023)
    return [m if j % 2 == 0 else -m] + [0] * 63


def ac_cat10(q, j):
    return single(ZIGZAG[1 + j % 63], 1 if j % 2 else -1, True)(q, j)


def at_zigzag(indices, dc=0):
    """+-1 at the given zig-zag indices (signs alternate with the block)."""
    def f(q, j):
        b = [0] * 64
        b[0] = dc
        for n, k in enumerate(indices):
            b[ZIGZAG[k]] = 1 if (n + j) % 2 else -1
        return b
    return f


def eob_only(q, j):
    return [0] * 64


def random_block(seed, terms, mag):
    """`terms` (None: 20..63 of them, (lo, hi): lo..hi-1, chosen per block) nonzero AC terms of magnitude up to `mag` and a DC,
    drawn again, with a halved magnitude every fourth time, until the range condition holds."""
    def f(q, j):
        rng = np.random.default_rng((seed, j, q[1], q[63]))
        m = mag
        for attempt in range(4000):
            n = terms if isinstance(terms, int) else int(rng.integers(*(terms or (20, 64))))
            b = np.zeros(64, np.int64)
            b[rng.permutation(63)[:n] + 1] = rng.integers(1, m + 1, n) * rng.choice((-1, 1), n)
            b[0] = int(rng.integers(-m, m + 1)) if q[0] * m <= 2000 else 0
            if in_range(b, q):
                return [int(v) for v in b]
            if attempt % 4 == 3 and m > 1:
                m //= 2
        raise AssertionError("no block within the range condition")
    return f


def build(name, recipes, sampling, quant, size=None, claims=None, fill=eob_only, **kw):
    """Files named name[i] holding the blocks of `recipes` in scan order (the rest of the last image: `fill`)."""
    comp_quant = kw.get("comp_quant", (0, 1, 1))
    out, at, i = [], 0, 0
    while at < len(recipes):
        w, h = size or (96, 72)
        comps = jf.block_components(w, h, sampling)
        seen = [0, 0, 0]
        blocks = []
        for c in comps:
            r = recipes[at] if at < len(recipes) else fill
            at += 1
            blocks.append(r(quant[comp_quant[c]], seen[c]))
            seen[c] += 1
        data, cen = jf.write_jpeg(w, h, sampling, blocks, quant, **kw)
        out.append(Case(f"{name}[{i}]", data, cen, dict(RANGE_CLAIMS, **(claims or {}))))
        i += 1
    return out


SMALL = {(1, 1): (41, 23), (2, 1): (41, 23), (2, 2): (41, 23)}     # 54, 36 and 36 blocks; no multiple of any MCU size


@functools.lru_cache(None)
def block_cases():
    out = []
    for sampling in SAMPLINGS:
        s = f"{sampling[0]}x{sampling[1]}"
        for qn, (ql, qc) in QUANTS.items():
            quant = {0: ql, 1: qc}
            ones = qn == "ones"
            tag = f"{s}-{qn}"
            n = jf.block_count(*SMALL[sampling], sampling)
            singles = [single(p, sg, big) for big in (False, True) for sg in (1, -1) for p in range(64)]
            out += build(f"single-{tag}", singles, sampling, quant, claims={"max_ac_category": ("ge", 10 if ones else 1)})
            out += build(f"dc_swing-{tag}", [dc_swing] * n, sampling, quant, SMALL[sampling],
                         {"max_dc_category": ("eq", 11) if ones else ("ge", 1), "eob_only": ("eq", n)})
            out += build(f"ac_cat10-{tag}", [ac_cat10] * n, sampling, quant, SMALL[sampling],
                         {"max_ac_category": ("eq", 10) if ones else ("ge", 1)})
            zr = [at_zigzag([17]), at_zigzag([33]), at_zigzag([49]), at_zigzag([63]), at_zigzag([14, 63]), at_zigzag([1, 18, 51]),
                  at_zigzag([16]), at_zigzag([15, 32]), at_zigzag([62])]
            out += build(f"zrl-{tag}", zr * (n // len(zr)), sampling, quant, SMALL[sampling],
                         {"zrl": ("ge", 10), "max_zrl_run": ("eq", 3), "end_at_63": ("ge", 2)})
            out += build(f"eob_only-{tag}", [eob_only] * n, sampling, quant, SMALL[sampling], {"eob_only": ("eq", n)})
            out += build(f"full_ac-{tag}", [random_block(11, 63, 3)] * n, sampling, quant, SMALL[sampling],
                         {"full_ac": ("eq", n), "end_at_63": ("eq", n)})
            out += build(f"dense-{tag}", [random_block(12, None, 40)] * n, sampling, quant, SMALL[sampling],
                         {"eob_only": ("eq", 0), "len9": ("eq", True), "len10": ("eq", True)})
    return out


# ---- tables -----------------------------------------------------------------------------------------------------------------
AC_9_10_16 = jf.make_table({0x02: 2, 0x03: 2, 0x04: 2, 0x00: 9, 0x01: 10, 0xF0: 16, 0x11: 16})
AC_EOB_ONLY = jf.make_table({0x00: 1})
DC_1BIT = jf.make_table({0: 1, 1: 3, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 8, 8: 9, 9: 10, 10: 11, 11: 12})
DC_9_10_16 = jf.make_table({0: 2, 1: 9, 2: 10, 3: 16, 4: 16})
FOUR = {(0, 0): (DC_LUMA_BITS, DC_VALS), (0, 1): (DC_CHROMA_BITS, DC_VALS), (0, 2): DC_1BIT, (0, 3): (DC_CHROMA_BITS, DC_VALS[::-1]),
        (1, 0): (AC_LUMA_BITS, AC_LUMA_VALS), (1, 1): (AC_CHROMA_BITS, AC_CHROMA_VALS),
        (1, 2): (AC_LUMA_BITS, AC_LUMA_VALS[40:] + AC_LUMA_VALS[:40]), (1, 3): (AC_CHROMA_BITS, AC_CHROMA_VALS[::-1])}


def small_dc(values):
    def f(q, j):
        return [values[j % len(values)] if q[0] * 7 <= 2000 else 0] + [0] * 63
    return f


@functools.lru_cache(None)
def table_cases():
    out = []
    q50 = dict(enumerate(quant_tables(50)))
    ones = {0: [1] * 64, 1: [1] * 64}
    for sampling in SAMPLINGS:
        s = f"{sampling[0]}x{sampling[1]}"
        size = SMALL[sampling]
        n = jf.block_count(*size, sampling)
        huff = {(0, 0): DC_9_10_16, (0, 1): DC_9_10_16, (1, 0): AC_9_10_16, (1, 1): AC_9_10_16}
        rec = [at_zigzag([1, 2]), at_zigzag([17, 18], dc=1), at_zigzag([1, 2, 19], dc=-2), at_zigzag([1], dc=5), eob_only]
        out += build(f"codes_9_10_16-{s}", rec * (n // len(rec)), sampling, ones, size,
                     {"len9": ("eq", True), "len10": ("eq", True), "max_code_length": ("eq", 16), "zrl": ("ge", 4)}, huff=huff)
        huff = dict(jf.ANNEX_K)
        huff[(1, 0)] = huff[(1, 1)] = AC_EOB_ONLY
        out += build(f"one_symbol_ac-{s}", [small_dc([3, -7, 0, 6, 1])] * n, sampling, q50, size, {"eob_only": ("eq", n)}, huff=huff)
        huff = dict(jf.ANNEX_K)
        huff[(0, 0)] = huff[(0, 1)] = DC_1BIT
        out += build(f"dc_1bit_flat-{s}", [small_dc([5])] * n, sampling, q50, size,
                     {"eob_only": ("eq", n), "max_dc_category": ("eq", 3), "data_bits": ("le", 7 * n)}, huff=huff)
        out += build(f"four_tables-{s}", [random_block(21, None, 12)] * n, sampling, q50, size, {"max_code_length": ("ge", 11)},
                     huff=FOUR, comp_dc=(3, 1, 2), comp_ac=(2, 3, 1))
        q3 = {0: quant_tables(50)[0], 1: quant_tables(75)[1], 2: quant_tables(10)[1]}
        out += build(f"three_quant-{s}", [random_block(22, None, 12)] * n, sampling, q3, size, comp_quant=(0, 1, 2))
        q16 = {0: [256 + 3 * k for k in range(64)], 1: [700 - 5 * k for k in range(64)]}
        out += build(f"dqt16_above_255-{s}", [random_block(23, (3, 10), 2)] * n, sampling, q16, size,
                     {"max_dequant": ("ge", 256)}, quant16=True)
        # the writer's own ids, slots and layout: SOF1, no JFIF, merged tables with the DHT first and the DQT after the SOF,
        # quantisation ids 3 and 2, Huffman slots 2 and 3, component ids 7, 200, 0, restart interval 3, zero padding bits
        k = jf.ANNEX_K
        out += build(f"writer_layout-{s}", [random_block(24, None, 12)] * n, sampling, {3: q50[0], 2: q50[1]}, size,
                     huff={(0, 2): k[(0, 0)], (1, 2): k[(1, 0)], (0, 3): k[(0, 1)], (1, 3): k[(1, 1)]}, comp_quant=(3, 2, 2),
                     comp_dc=(2, 3, 3), comp_ac=(2, 3, 3), comp_ids=(7, 200, 0), layout=("dht", "sof", "dqt", "dri"), merged=True,
                     sof=0xC1, restart=3, pad_bit=0)
    return out


# ---- padding -------------------------------------------------------------------------------------------------------------------
def _dense_file(seed, sampling=(1, 1), size=(24, 16), **kw):
    n = jf.block_count(*size, sampling)
    return build(f"dense_seed{seed}", [random_block(seed, None, 30)] * n, sampling, dict(enumerate(quant_tables(50))), size, **kw)[0]


@functools.lru_cache(None)
def padding_cases():
    """A file for every padding length 0..7 with one bits, and one with zero bits (found by varying the content)."""
    out = {}
    for seed in range(1000, 1400):
        for bit in (1, 0):
            c = _dense_file(seed, SAMPLINGS[seed % 3], pad_bit=bit)
            key = (c.census["pad_bits"], bit)
            if key not in out:
                out[key] = Case(f"pad{key[0]}_bit{bit}", c.data, c.census, dict(c.claims, pad_bits=("eq", key[0])))
        if len(out) == 16:
            break
    return [out[k] for k in sorted(out)]


# ---- chunk sizes ---------------------------------------------------------------------------------------------------------------
FIXED_CHUNKS = (65, 67, 101, 127, 250)


def boundary_in_padding(census, chunk_bits):
    """A multiple of chunk_bits lies strictly inside the padding bits: data_bits < m * chunk_bits < data_bits + pad_bits."""
    seg = census["data_bits"] + census["pad_bits"]
    return ((seg - 1) // chunk_bits) * chunk_bits > census["data_bits"]


def chunk_sizes(census):
    """data_bits + 1, its divisors >= 64, and the fixed sizes."""
    n = census["data_bits"] + 1
    return sorted({n} | {d for d in range(64, n) if n % d == 0} | set(FIXED_CHUNKS))


@functools.lru_cache(None)
def chunk_cases():
    """A small set of files in which, for each of the fixed sizes and for data_bits + 1, some file has a chunk boundary strictly
    inside its padding bits.  [(case, chunk sizes, those of them with a boundary inside the padding)]."""
    want, out = set(FIXED_CHUNKS), []
    for seed in range(2000, 2600):
        c = _dense_file(seed, SAMPLINGS[seed % 3])
        if c.census["pad_bits"] < 2:
            continue
        sizes = chunk_sizes(c.census)
        hit = [cb for cb in sizes if boundary_in_padding(c.census, cb)]
        if want & set(hit):
            want -= set(hit)
            out.append((c, sizes, hit))
        if not want:
            break
    assert not want, want
    return out


# ---- the sequential fallback ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def fallback_cases():
    """[(case, chunk_bits, fallback)]: whether the chunk lanes fail to reach their fixed point within t4d_jpeg::kRounds rounds.
    With: small chunks on dense blocks (a block is longer than several chunks, so a lane's guessed state stays wrong until its
    predecessor's true exit state arrives, one lane a round) and long flat runs (EOB-only blocks decode from any phase, so a
    guessed block-in-MCU phase never corrects itself).  Without: one lane, few lanes, and chunks long enough to re-synchronise."""
    q50 = dict(enumerate(quant_tables(50)))
    ones = {0: [1] * 64, 1: [1] * 64}
    n = jf.block_count(96, 72, (1, 1))
    dense = build("fallback_dense", [random_block(31, 63, 40)] * n, (1, 1), ones, (96, 72))[0]
    flat = build("fallback_flat", [small_dc([4])] * n, (2, 2), q50, (96, 72))[0]
    n = jf.block_count(96, 72, (2, 1))
    mild = build("fallback_mild", [random_block(32, None, 6)] * n, (2, 1), q50, (96, 72))[0]
    return [(dense, 64, True), (dense, 67, True), (flat, 64, True), (flat, 65, True),
            (dense, 0, False), (flat, 0, False), (mild, 0, False), (mild, 1000, False), (mild, 4096, False), (flat, 256, False),
            (dense, 1 << 20, False)]


# ---- headers -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def base_files():
    """Plain 4:2:0, 4:2:2 with optimised (non Annex K) tables, 4:4:4 with restart interval 2."""
    q = dict(enumerate(quant_tables(75)))
    out = []
    n = jf.block_count(47, 35, (2, 2))
    out += build("base_420", [random_block(41, None, 20)] * n, (2, 2), q, (47, 35))
    n = jf.block_count(52, 27, (2, 1))
    opt = {(0, 0): DC_1BIT, (0, 1): (DC_CHROMA_BITS, DC_VALS[::-1]), (1, 0): (AC_CHROMA_BITS, AC_CHROMA_VALS),
           (1, 1): (AC_LUMA_BITS, AC_LUMA_VALS)}
    out += build("base_422_opt", [random_block(42, None, 20)] * n, (2, 1), q, (52, 27), huff=opt)
    n = jf.block_count(33, 31, (1, 1))
    out += build("base_444_rst2", [random_block(43, None, 20)] * n, (1, 1), q, (33, 31), restart=2)
    return out


@functools.lru_cache(None)
def pil_base_files():
    """The same three kinds from PIL's encoder (no census): plain 4:2:0, optimize=True 4:2:2, 4:4:4 with restart interval 2."""
    import io
    from PIL import Image
    out = []
    for i, (name, (h, w), kw) in enumerate([("pil_420", (37, 53), dict(subsampling=2)),
                                            ("pil_422_opt", (29, 61), dict(subsampling=1, optimize=True)),
                                            ("pil_444_rst2", (33, 31), dict(subsampling=0, restart_marker_blocks=2))]):
        rng = np.random.default_rng(50 + i)
        y, x = np.mgrid[0:h, 0:w]
        img = np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (3 * x + 5 * y) % 256], -1) + rng.integers(-20, 21, (h, w, 3))
        b = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(b, "JPEG", quality=85, **kw)
        out.append(Case(name, b.getvalue(), None, {}))
    return out


@functools.lru_cache(None)
def header_cases():
    """([(name, data, base case)] the GPU path takes, [(name, data, base case, reason)] it does not)."""
    taken, not_taken = [], []
    for b in base_files() + pil_base_files():
        for name, f in jf.REWRITES.items():
            taken.append((f"{b.name}-{name}", f(b.data), b))
        for name, (f, reason) in jf.NOT_TAKEN.items():
            not_taken.append((f"{b.name}-{name}", f(b.data), b, reason))
    return taken, not_taken


# ---- beyond the range condition ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def beyond_range():
    """Blocks whose exact samples reach +-1000 and more (two large low-frequency terms against the DC): libjpeg's C range table
    wraps, SIMD builds saturate.  CPU only; no GPU test decodes it."""
    ones = {0: [1] * 64, 1: [1] * 64}

    def f(q, j):
        b = [0] * 64
        sign = 1 if j % 2 else -1
        b[0], b[1], b[8], b[9] = sign * 1000, sign * 1023, sign * 1023, sign * (900 + j)
        return b
    n = jf.block_count(16, 16, (1, 1))
    data, cen = jf.write_jpeg(16, 16, (1, 1), [f(None, j // 3) if j % 3 == 0 else [0] * 64 for j in range(n)], ones)
    return Case("beyond_range", data, cen, {"sample_max": ("ge", 512.0), "sample_min": ("le", -513.0)})


def all_cases():
    return block_cases() + table_cases() + padding_cases() + base_files()


# ---- corrupted input -----------------------------------------------------------------------------------------------------------
Corrupt = namedtuple("Corrupt", "name header segment tables")   # tables: {slot: bits[16]} written over the descriptor's tables


def _markers(seg):
    return [i for i in range(len(seg) - 1) if seg[i] == 0xFF and 0xD0 <= seg[i + 1] <= 0xD7]


@functools.lru_cache(None)
def corrupted(seed=7, per_kind=6):
    """Corrupted entropy-coded segments (bit flips, cuts, random bytes, FF / 00 runs, junk after the last block, restart markers
    dropped, doubled or out of order) and refused-table descriptors of valid files.  The segment goes to the decoder as it is,
    data_bytes its length: the C ABI promises defined behaviour whatever the bytes hold."""
    from topo4d_amd import ingest
    rng = np.random.default_rng(seed)
    bases = base_files() + [block_cases()[0], table_cases()[0]]
    out = []
    for b in bases:
        h = ingest.parse_jpeg(b.data)
        seg = b.data[h.scan_start:h.scan_end]
        n = len(seg)
        add = lambda kind, s, tables=None: out.append(Corrupt(f"{b.name}-{kind}{sum(1 for c in out if c.name.startswith(b.name + '-' + kind))}", h, bytes(s), tables))
        for _ in range(per_kind):
            s = bytearray(seg)
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(0, n))] ^= 1 << int(rng.integers(0, 8))
            add("flip", s)
            a = int(rng.integers(0, n))
            s = bytearray(seg)
            s[a:a + int(rng.integers(1, 40))] = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            add("random", s)
            a = int(rng.integers(0, n))
            add("ff_run", seg[:a] + b"\xff" * int(rng.integers(1, 20)) + seg[a:])
            add("zero_run", seg[:a] + b"\x00" * int(rng.integers(1, 20)) + seg[a + int(rng.integers(0, 8)):])
            add("junk", seg + rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8).tobytes())
        ffs = [i for i in range(n - 1) if seg[i] == 0xFF]
        cuts = {0, 1, n // 2, n - 1} | {i + 1 for i in ffs[:2]} | {i for i in ffs[:2]} | {i + 2 for i in _markers(seg)[:1]}
        for a in sorted(cuts):
            add("cut", seg[:a])
        ms = _markers(seg)
        if ms:
            m = ms[len(ms) // 2]
            add("rst_dropped", seg[:m] + seg[m + 2:])
            add("rst_doubled", seg[:m] + seg[m:m + 2] + seg[m:])
            s = bytearray(seg)
            s[ms[0] + 1], s[ms[1] + 1] = s[ms[1] + 1], s[ms[0] + 1]
            add("rst_swapped", s)
            add("rst_all_dropped", b"".join(seg[a + 2 if a >= 0 else 0:e] for a, e in zip([-1] + ms, ms + [n])))
        add("refused_overfull", seg, {0: [3] + [0] * 15})
        add("refused_all_ones", seg, {4: [0, 4] + [0] * 14})
        add("refused_too_many", seg, {5: [0] * 8 + [255, 255] + [0] * 6})
        add("refused_all_tables", seg, {s: [255] * 16 for s in range(8)})
    return out
