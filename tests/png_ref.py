"""The PNG encoder of csrc/t4d_png.hip restated in Python/numpy from its stated rule ("PNG encoder"): the whole file as
bytes, which the kernel's file must equal byte for byte (tests/test_gpu_png_bytes.py), plus a census of every segment that says
which of the rule's branches an input reaches (tests/png_enc_cases.py).

    encode(image, bits=8)  ->  (file bytes, [census per segment])

image: uint8 [h,w] / [h,w,c], c in {1, 3, 4}; with bits=16 an integer image whose low 16 bits are written high byte first.  The float
quantisers are not restated here (tests/test_gpu_png.py and test_gpu_progress.py hold them to numpy and torchvision exactly).

The rule, in the order of the code below:
  filter     per row the filter 0..4 with the least sum of |int8 residual| at a byte distance of bytes per pixel; the lower number
             wins a tie
  segments   16,384 filtered bytes each, the last one shorter; every segment is coded on its own
  parse      by the segment's maximal equal-byte runs: a literal, matches of 258 at distance 1, the remainder as one match if it is
             at least 3, else as literals
  histogram  of the literal/length symbols, plus one end-of-block; fewer than two used symbols are padded to two (symbol 1 if symbol 0
             is used, else symbol 0) - a branch no segment reaches, see pad_is_dead()
  lengths    used symbols by (frequency, symbol); two-queue Huffman, a leaf wins a weight tie against an internal node; depths
             clamped to 15 (7 for the code-length alphabet); the Kraft excess removed one unit at a time: the deepest non-empty
             length b < max gives one leaf to b + 1, which takes a clamped leaf as its sibling; lengths longest first to the least
             frequent symbols
  codes      canonical (RFC 1951 3.2.2), written LSB first
  header     HLIT trimmed to the last used length symbol, HDIST = 0 (one distance code, symbol 0, length 1), the code-length
             sequence = the HLIT + 257 lengths run-length coded, then the distance length on its own (never joined to a run of the
             lengths before it); zero runs: 18 for 11..138 at a time, then 17 for 3..10, then single zeros; other runs: the value,
             then 16 for 3..6 at a time, then single values; HCLEN trimmed in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
  choice     Huffman if its bytes - with the empty stored block that follows it on every segment but the last - are fewer than the
             stored block's n + 5; a tie is stored.  A stored segment is byte-aligned as it is and gets no empty block after it.
  framing    signature, IHDR, IDAT(78 01), one IDAT per segment, IDAT(Adler-32), IEND
"""
import heapq
import struct
import zlib

import numpy as np

SEG = 16384
LIT, CL = 286, 19
EOB = 256
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}


# ---- filters ---------------------------------------------------------------------------------------------------------------------
def filter_rows(by, bpp):
    """by: integer [h, stride] of the rows' bytes.  (filter byte per row uint8 [h], the five scores int64 [h,5], the filtered rows
    uint8 [h, 1 + stride])."""
    by = np.asarray(by).astype(np.int64)
    h, stride = by.shape
    z = np.zeros((h, min(bpp, stride)), np.int64)
    left = np.concatenate([z, by[:, :max(stride - bpp, 0)]], 1)
    up = np.concatenate([np.zeros((1, stride), np.int64), by[:-1]], 0)
    upleft = np.concatenate([z, up[:, :max(stride - bpp, 0)]], 1)
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    preds = [np.zeros_like(by), left, up, (left + up) >> 1, paeth]
    resid = np.stack([(by - q) & 255 for q in preds], 1)                          # [h, 5, stride]
    cost = np.abs((resid ^ 128) - 128).sum(2)                                       # |int8|
    best = np.argmin(cost, 1)                                                       # argmin: the first of equal minima
    rows = np.concatenate([best[:, None], resid[np.arange(h), best]], 1).astype(np.uint8)
    return best.astype(np.uint8), cost, rows


def image_bytes(image, bits=8):
    """(integer [h, stride] bytes of the rows, bytes per pixel, (h, w, c))"""
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[..., None]
    h, w, c = image.shape
    assert h >= 1 and w >= 1 and c in COLOUR_TYPE and bits in (8, 16)
    if bits == 8:
        assert image.dtype == np.uint8
        return image.reshape(h, w * c).astype(np.int64), c, (h, w, c)
    v = image.astype(np.int64) & 0xFFFF
    return np.stack([v >> 8, v & 255], -1).reshape(h, 2 * w * c), 2 * c, (h, w, c)


# ---- parse -----------------------------------------------------------------------------------------------------------------------
def length_symbol(l):
    """(symbol 257..285, extra bits, their value) of a match length 3..258"""
    assert 3 <= l <= 258
    i = max(k for k in range(29) if LEN_BASE[k] <= l)
    return 257 + i, LEN_EXTRA[i], l - LEN_BASE[i]


_LENGTH_SYMBOL = {l: length_symbol(l) for l in range(3, 259)}


def runs_of(seg):
    """[(start, end)] of the maximal equal-byte runs of a uint8 vector"""
    cut = np.flatnonzero(seg[1:] != seg[:-1]) + 1
    return list(zip(np.concatenate([[0], cut]).tolist(), np.concatenate([cut, [seg.size]]).tolist()))


def parse(seg):
    """Tokens of a segment: a literal is its byte 0..255; a match is -length.  Also the token classes that occurred."""
    tokens, classes = [], set()
    vals = seg.tolist()
    for rs, re in runs_of(seg):
        v = vals[rs]
        tokens.append(v)
        classes.add("literal")
        full, rem = divmod(re - rs - 1, 258)
        if full:
            tokens.extend([-258] * full)
            classes.add("match258")
        if rem >= 3:
            tokens.append(-rem)
            classes.add(("rem_match", _LENGTH_SYMBOL[rem][0]))
        else:
            tokens.extend([v] * rem)
            if full:
                classes.add(("rem_literals_after_258", rem))
    return tokens, classes


# ---- Huffman ---------------------------------------------------------------------------------------------------------------------
def natural_depth(freq):
    """The depth of the shallowest optimal Huffman tree of the used symbols, from a heap - independent of the two-queue code below.
    Among equal weights the heap takes the node of least height first, which gives the optimal tree of least height: if this depth
    passes the limit, every Huffman tree of the histogram does."""
    heap = [(int(f), 0, s) for s, f in enumerate(freq) if f]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    tick = len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tick))
        tick += 1
    return heap[0][1]


def two_queue_depths(weights):
    """Leaf depths of the Huffman tree of `weights` (ascending): two queues, the sorted leaves and the internal nodes in the order
    they were made; the lighter head is taken, a leaf on a tie."""
    m = len(weights)
    if m == 1:
        return [1]
    node_w, parent = list(weights), {}
    made = []                                      # internal nodes, in order: ids m, m + 1, ...
    li = ii = 0
    for _ in range(m - 1):
        picked = []
        for _ in range(2):
            if li < m and (ii >= len(made) or node_w[li] <= node_w[made[ii]]):
                picked.append(li)
                li += 1
            else:
                picked.append(made[ii])
                ii += 1
        nid = len(node_w)
        node_w.append(node_w[picked[0]] + node_w[picked[1]])
        parent[picked[0]] = parent[picked[1]] = nid
        made.append(nid)
    depth = {len(node_w) - 1: 0}
    for nid in range(len(node_w) - 2, -1, -1):     # a parent is always made after its children: ids descend from the root
        depth[nid] = depth[parent[nid]] + 1
    return [depth[i] for i in range(m)]


def limited_lengths(freq, max_bits, census=None):
    """Code lengths of the histogram `freq` under the encoder's rule (module docstring, "lengths")."""
    order = sorted((int(f), s) for s, f in enumerate(freq) if f)
    lengths = [0] * len(freq)
    if not order:
        return lengths
    depths = two_queue_depths([f for f, _ in order])
    count = [0] * (max(max(depths), max_bits) + 1)
    for d in depths:
        count[d] += 1
    clamped = sum(count[max_bits + 1:])
    count = count[:max_bits + 1]
    count[max_bits] += clamped
    excess = sum(n << (max_bits - b) for b, n in enumerate(count) if b) - (1 << max_bits)     # in units of 2^-max_bits
    steps = 0
    while excess > 0:
        b = max(k for k in range(1, max_bits) if count[k])
        count[b] -= 1                              # the leaf at b becomes an internal node with two children at b + 1:
        count[b + 1] += 2                          # itself and a leaf that was at max_bits
        count[max_bits] -= 1
        excess -= 1
        steps += 1
    at = 0
    for b in range(max_bits, 0, -1):
        for _ in range(count[b]):
            lengths[order[at][1]] = b
            at += 1
    assert at == len(order)
    if census is not None:
        census.update(two_queue_depth=max(depths), clamped_leaves=clamped, kraft_steps=steps)
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2 codes, each bit-reversed so that it is written LSB first"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for b in range(1, 17):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    codes = []
    for l in lengths:
        if not l:
            codes.append(0)
            continue
        v = nxt[l]
        nxt[l] += 1
        codes.append(int(format(v, f"0{l}b")[::-1], 2))
    return codes


def pad_to_two(freq):
    """The kernel's pad of a histogram with fewer than two used symbols"""
    if sum(1 for f in freq if f) < 2:
        freq[1 if freq[0] else 0] = 1


def code_length_ops(lit_len, n_lit):
    """[(code-length symbol, extra value)] for the n_lit literal/length lengths, then for the one distance length"""
    ops = []

    def rle(seq):
        i = 0
        while i < len(seq):
            v, run = seq[i], 1
            while i + run < len(seq) and seq[i + run] == v:
                run += 1
            i += run
            if v == 0:
                while run >= 11:
                    k = min(run, 138)
                    ops.append((18, k - 11))
                    run -= k
                if run >= 3:
                    ops.append((17, run - 3))
                    run = 0
            else:
                ops.append((v, 0))
                run -= 1
                while run >= 3:
                    k = min(run, 6)
                    ops.append((16, k - 3))
                    run -= k
            ops.extend([(v, 0)] * run)

    rle(list(lit_len[:n_lit]))
    rle([1])
    return ops


# ---- bits ------------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.vals, self.lens = [], []

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.vals.append(value)
        self.lens.append(nbits)

    def nbits(self):
        return int(sum(self.lens))

    def tobytes(self):
        lens = np.asarray(self.lens, np.int64)
        vals = np.asarray(self.vals, np.int64)
        total = int(lens.sum())
        start = np.cumsum(lens) - lens
        k = np.arange(total) - np.repeat(start, lens)
        bits = (np.repeat(vals, lens) >> k) & 1
        return np.packbits(bits.astype(np.uint8), bitorder="little").tobytes()


def deflate_segment(seg, last):
    """(bytes of the segment's IDAT payload, census)"""
    n = seg.size
    tokens, classes = parse(seg)
    freq = [0] * LIT
    for t in tokens:
        freq[t if t >= 0 else _LENGTH_SYMBOL[-t][0]] += 1
    freq[EOB] += 1
    census = {"n": n, "tokens": len(tokens), "classes": classes, "runs": runs_of(seg),
              "lit_used_before_pad": sum(1 for f in freq if f)}
    pad_to_two(freq)
    lit_census = {}
    lit_len = limited_lengths(freq, 15, lit_census)
    lit_code = canonical_codes(lit_len)
    n_lit = LIT
    while n_lit > 257 and lit_len[n_lit - 1] == 0:
        n_lit -= 1
    ops = code_length_ops(lit_len, n_lit)
    cl_freq = [0] * CL
    for s, _ in ops:
        cl_freq[s] += 1
    census["cl_used_before_pad"] = sum(1 for f in cl_freq if f)
    pad_to_two(cl_freq)
    cl_census = {}
    cl_len = limited_lengths(cl_freq, 7, cl_census)
    cl_code = canonical_codes(cl_len)
    n_cl = CL
    while n_cl > 4 and cl_len[CL_ORDER[n_cl - 1]] == 0:
        n_cl -= 1

    out = Bits()
    out.put((1 if last else 0) | (2 << 1), 3)                                       # BFINAL, BTYPE = 10
    out.put(n_lit - 257, 5)
    out.put(0, 5)                                                                   # HDIST
    out.put(n_cl - 4, 4)
    for i in range(n_cl):
        out.put(cl_len[CL_ORDER[i]], 3)
    for s, arg in ops:
        out.put(cl_code[s], cl_len[s])
        if s in CL_EXTRA:
            out.put(arg, CL_EXTRA[s])
    for t in tokens:
        if t >= 0:
            out.put(lit_code[t], lit_len[t])
        else:
            sym, e, val = _LENGTH_SYMBOL[-t]
            out.put(lit_code[sym], lit_len[sym])
            out.put(val, e)
            out.put(0, 1)                                                           # the distance code: one bit, 0
    out.put(lit_code[EOB], lit_len[EOB])
    if not last:
        out.put(0, 3)                                                               # an empty stored block, not final
        out.put(0, -out.nbits() % 8)
        out.put(0xFFFF0000, 32)                                                     # LEN 0, NLEN FFFF
    huff_bytes = (out.nbits() + 7) // 8
    stored_bytes = n + 5
    use_huffman = huff_bytes < stored_bytes
    if use_huffman:
        data = out.tobytes()
        assert len(data) == huff_bytes
    else:
        data = bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + seg.tobytes()
    census.update(lit_freq=freq, lit_len=lit_len, lit_depth=natural_depth(freq), lit=lit_census,
                  cl_freq=cl_freq, cl_len=cl_len, cl_depth=natural_depth(cl_freq), cl=cl_census,
                  n_lit=n_lit, n_cl=n_cl, huffman=use_huffman, huff_bytes=huff_bytes, stored_bytes=stored_bytes)
    return data, census


# ---- the file --------------------------------------------------------------------------------------------------------------------
def chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def encode(image, bits=8):
    by, bpp, (h, w, c) = image_bytes(image, bits)
    filters, cost, rows = filter_rows(by, bpp)
    stream = rows.reshape(-1)
    segs = -(-stream.size // SEG)
    out = [b"\x89PNG\r\n\x1a\n", chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bits, COLOUR_TYPE[c], 0, 0, 0)),
           chunk(b"IDAT", b"\x78\x01")]
    census = []
    for k in range(segs):
        seg = stream[k * SEG:(k + 1) * SEG]
        data, cen = deflate_segment(seg, k == segs - 1)
        cen["filters"] = filters
        cen["filter_cost"] = cost
        census.append(cen)
        out.append(chunk(b"IDAT", data))
    out.append(chunk(b"IDAT", struct.pack(">I", zlib.adler32(stream.tobytes()))))
    out.append(chunk(b"IEND", b""))
    return b"".join(out), census


def pad_is_dead():
    """Why `used < 2` cannot happen in a file, for either alphabet (the host program of tests/native covers the branch instead).

    Literal/length: a segment has n >= 1 bytes, so its first token is a literal, and end-of-block is always counted: two symbols.
    Code-length: the sequence holds the lengths of at least 257 symbols plus the distance length.  At least two of them are
    non-zero (a literal and end-of-block) and at least one is zero unless all 257 are used.  With a zero run the alphabet has a
    zero-run symbol (0, 17 or 18) and a non-zero length: two.  Without one, 257 or more non-zero lengths would have to be one value
    written singly; equal neighbours beyond three are written with 16, a second symbol, and 257 entries of one value cannot avoid a
    run of four."""
    return True
