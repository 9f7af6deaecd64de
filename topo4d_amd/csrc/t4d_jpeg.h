// t4d_jpeg.h — the per-symbol, per-block and per-pixel parts of a baseline JPEG decoder that reproduces libjpeg-turbo's output
// (ISLOW IDCT, fancy upsampling, table-driven YCbCr->RGB), as device functions and as host ones for the CPU tests
// (tests/native/jpeg_host.cpp).  csrc/t4d_ingest.hip runs them on the GPU.
//
// Entropy-coded data is read from the "compacted" stream: the scan's bytes with the FF 00 stuffing and the RSTn markers removed,
// so that a restart interval is a contiguous run of bits.  Past the end of a stream the reader sees zero bits (libjpeg inserts
// zeros once it meets a marker); a segment whose decode needs them is truncated.
//
// Decoding state between two symbols is (bit position, block within the MCU, coefficient index): k = 0 means the next symbol is
// a DC category, 1..63 an AC run/size.  Chunked decoding (Weissenberger & Schmidt, ICPP 2018) starts a lane at a guessed state
// and relies on these states re-synchronising; t4d_ingest.hip iterates the lanes' start states to a fixed point.
//
// Three rules ("View ingest"; tests/jpeg_dec_cases.py holds each):
//   - a chunk is any number of bits >= 64, byte multiple or not, and every such value decodes every valid file: a boundary inside
//     the 1..7 padding bits after the last block is handled in decode_lane;
//   - a DHT table build_huff refuses is still written in full, as a table that matches no code: the image reports kErrCode, every
//     later step reads defined values and always advances, the other images of a batch are unaffected;
//   - the output equals PIL's (libjpeg-turbo's SIMD IDCT) while a block's exact IDCT samples stay within +-500 and
//     |coefficient * q| below 32768; beyond that it is libjpeg's C range-table wrap (range_limit).
// Whatever the bytes hold, the arithmetic is defined (the IDCT wraps in 32 bits, `Wrap`) and no read or write leaves its arrays.
#pragma once

#include <stdint.h>

#include "../../include/topo4d_raster.h"

#if defined(__HIPCC__)
#define T4D_JPEG_HD __host__ __device__
#else
#define T4D_JPEG_HD
#endif
#define T4D_JPEG_FN T4D_JPEG_HD static inline

namespace t4d_jpeg {

constexpr int kLookBits = 9;
constexpr int kRounds = 12;       // start-state rounds of the chunk lanes before they are decoded one after another instead

// jpeg_make_d_derived_tbl: canonical codes of one DHT table
struct Huff {
    int32_t maxcode[18];          // largest code of length l (-1: none); maxcode[17] is a sentinel above every 16-bit code
    int32_t valoffset[18];        // symbol index = code + valoffset[l]
    uint16_t look[1 << kLookBits];  // codes of length <= kLookBits: (length << 8) | symbol; 0: longer
    uint8_t val[256];
};

// a table no code matches: every lookup is "bad" (symbol 0, 16 bits), so a decode that goes on over it reads defined values,
// always advances and reports kErrCode
T4D_JPEG_FN bool refuse_huff(Huff *h)
{
    for (int l = 0; l < 18; l++) {
        h->maxcode[l] = -1;
        h->valoffset[l] = 0;
    }
    h->maxcode[17] = 0xFFFFF;
    for (int i = 0; i < (1 << kLookBits); i++) h->look[i] = 0;
    for (int i = 0; i < 256; i++) h->val[i] = 0;
    return false;
}

// false: the BITS counts overflow the code space (an all-ones code included) or list more than 256 symbols, as libjpeg refuses.
// A refused table is still written in full (refuse_huff): the image's status gets kErrCode and nothing downstream reads an
// unwritten record.
T4D_JPEG_FN bool build_huff(const uint8_t *bits, const uint8_t *vals, Huff *h)
{
    uint8_t size[257];
    uint16_t code[257];
    int p = 0;
    for (int l = 1; l <= 16; l++)
        for (int i = 0; i < bits[l - 1]; i++) {
            if (p >= 256) return refuse_huff(h);
            size[p++] = (uint8_t)l;
        }
    size[p] = 0;
    const int n = p;
    uint32_t c = 0;
    int si = n ? size[0] : 0;
    p = 0;
    while (p < n) {
        while (p < n && size[p] == si) code[p++] = (uint16_t)c++;
        if (c >= (1u << si)) return refuse_huff(h);  // libjpeg: no all-ones code
        c <<= 1;
        si++;
    }
    p = 0;
    for (int l = 1; l <= 16; l++) {
        if (bits[l - 1]) {
            h->valoffset[l] = p - (int32_t)code[p];
            p += bits[l - 1];
            h->maxcode[l] = code[p - 1];
        } else {
            h->valoffset[l] = 0;
            h->maxcode[l] = -1;
        }
    }
    h->valoffset[0] = h->valoffset[17] = 0;
    h->maxcode[0] = -1;
    h->maxcode[17] = 0xFFFFF;
    for (int i = 0; i < (1 << kLookBits); i++) h->look[i] = 0;
    p = 0;
    for (int l = 1; l <= kLookBits; l++)
        for (int i = 0; i < bits[l - 1]; i++, p++) {
            const int lb = code[p] << (kLookBits - l);
            for (int j = 0; j < (1 << (kLookBits - l)); j++) h->look[lb + j] = (uint16_t)((l << 8) | vals[p]);
        }
    for (int i = 0; i < 256; i++) h->val[i] = i < n ? vals[i] : 0;
    return true;
}

// 32 bits of the stream from bit `pos`, most significant first; zeros past `nbytes`
T4D_JPEG_FN uint32_t peek32(const uint8_t *d, int64_t nbytes, int64_t pos)
{
    const int64_t b = pos >> 3;
    uint64_t w = 0;
    for (int i = 0; i < 5; i++) w = (w << 8) | (b + i < nbytes ? d[b + i] : 0u);
    return (uint32_t)((w << (pos & 7)) >> 8);
}

// decode one Huffman symbol at the top of `bits`: the symbol, its length in *len (a code no table holds: symbol 0, length 16,
// *bad set - libjpeg warns and also returns 0)
T4D_JPEG_FN int decode_symbol(const Huff &h, uint32_t bits, int *len, bool *bad)
{
    const uint16_t e = h.look[bits >> (32 - kLookBits)];
    if (e) {
        *len = e >> 8;
        return e & 0xFF;
    }
    for (int l = kLookBits + 1; l <= 16; l++) {
        const int32_t code = (int32_t)(bits >> (32 - l));
        if (code <= h.maxcode[l]) {
            *len = l;
            return h.val[(code + h.valoffset[l]) & 0xFF];
        }
    }
    *bad = true;
    *len = 16;
    return 0;
}

T4D_JPEG_FN int extend(uint32_t v, int s) { return (int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

struct State {
    int64_t pos;
    int32_t blk;                  // block within the MCU
    int32_t k;                    // next coefficient (zig-zag index): 0 = DC
};

T4D_JPEG_FN bool same(const State &a, const State &b) { return a.pos == b.pos && a.blk == b.blk && a.k == b.k; }

// one symbol (and its extra bits) from state s.  Returns the zig-zag index written (0 = DC, 1..63 = AC, -1 = none: ZRL/EOB) and
// its value in *value (a DC difference for index 0).  Indices past 63 (corrupt data) are clamped to 63 as libjpeg's padded
// natural-order table does.
T4D_JPEG_FN int step(const uint8_t *d, int64_t nbytes, const Huff *dc, const Huff *ac, State &s, int *value, bool *bad)
{
    const uint32_t bits = peek32(d, nbytes, s.pos);
    int len;
    if (s.k == 0) {
        const int t = decode_symbol(*dc, bits, &len, bad);
        const int cat = t > 15 ? 0 : t;
        if (t > 15) *bad = true;
        int v = 0;
        if (cat) v = extend((bits << len) >> (32 - cat), cat);
        s.pos += len + cat;
        s.k = 1;
        *value = v;
        return 0;
    }
    const int rs = decode_symbol(*ac, bits, &len, bad);
    const int r = rs >> 4, sz = rs & 15;
    int idx = -1;
    if (sz) {
        const int k = s.k + r;
        idx = k > 63 ? 63 : k;
        *value = extend((bits << len) >> (32 - sz), sz);
        s.k = k + 1;
    } else if (r == 15) {
        s.k += 16;
    } else {
        s.k = 64;
    }
    s.pos += len + sz;
    return idx;
}

T4D_JPEG_FN void next_block(State &s, int bpm)
{
    if (s.k >= 64) {
        s.k = 0;
        s.blk = s.blk + 1 == bpm ? 0 : s.blk + 1;
    }
}

// jpeg_natural_order: zig-zag index -> natural (row-major) index
T4D_JPEG_FN int natural(int k)
{
    const uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k];
}

// ---- jidctint.c (jpeg_idct_islow) -------------------------------------------------------------------------------------------
constexpr int kConstBits = 13, kPass1Bits = 2;

// IDCT_range_limit[x & 1023]: the 10-bit wrap of the descaled value, then clamp(x + 128, 0, 255).
// The table is a clamp for descaled values in [-512, 511] and wraps beyond, as libjpeg's C code does; libjpeg-turbo's SIMD IDCT,
// which PIL's builds run, saturates instead.  So "byte-identical to PIL" holds for blocks whose exact (real-valued) IDCT samples,
// before the +128 level shift, stay within +-500 (512 less ISLOW's error) and whose |coefficient * q| stays below 32768; no
// encoder writes others.  tests/jpeg_dec_cases.py keeps its designed blocks inside this range and records one outside it.
T4D_JPEG_FN uint8_t range_limit(int x)
{
    const int s = ((x + 512) & 1023) - 512 + 128;
    return (uint8_t)(s < 0 ? 0 : s > 255 ? 255 : s);
}

// libjpeg's `int` arithmetic as 32-bit two's complement that wraps: the same bits wherever `int` does not overflow, which covers
// every block of the documented range, and defined behaviour for the coefficients of a corrupt stream, which do overflow it
struct Wrap {
    uint32_t v;
    T4D_JPEG_HD Wrap(int x = 0) : v((uint32_t)x) {}
    T4D_JPEG_HD int i() const { return (int)v; }
};
T4D_JPEG_FN Wrap wrap_of(uint32_t v) { Wrap r; r.v = v; return r; }
T4D_JPEG_FN Wrap operator+(Wrap a, Wrap b) { return wrap_of(a.v + b.v); }
T4D_JPEG_FN Wrap operator-(Wrap a, Wrap b) { return wrap_of(a.v - b.v); }
T4D_JPEG_FN Wrap operator*(Wrap a, Wrap b) { return wrap_of(a.v * b.v); }
T4D_JPEG_FN Wrap &operator+=(Wrap &a, Wrap b) { a.v += b.v; return a; }
T4D_JPEG_FN Wrap &operator*=(Wrap &a, Wrap b) { a.v *= b.v; return a; }

T4D_JPEG_FN int descale(Wrap x, int n) { return (x + (1 << (n - 1))).i() >> n; }

// one 8x8 block: coef in natural order (dequantised by q, natural order) -> out[row * pitch + col]
T4D_JPEG_FN void idct_islow(const int16_t *coef, const uint16_t *q, uint8_t *out, int64_t pitch)
{
    int ws[64];
    for (int c = 0; c < 8; c++) {
        const int16_t *in = coef + c;
        const uint16_t *qq = q + c;
        bool ac0 = true;
        for (int r = 1; r < 8; r++) ac0 = ac0 && in[8 * r] == 0;
        if (ac0) {
            const int dc = (Wrap(in[0] * qq[0]) * (1 << kPass1Bits)).i();
            for (int r = 0; r < 8; r++) ws[8 * r + c] = dc;
            continue;
        }
        Wrap z2 = in[16] * qq[16], z3 = in[48] * qq[48];
        Wrap z1 = (z2 + z3) * 4433;
        Wrap tmp2 = z1 + z3 * -15137;
        Wrap tmp3 = z1 + z2 * 6270;
        z2 = in[0] * qq[0];
        z3 = in[32] * qq[32];
        Wrap tmp0 = (z2 + z3) * (1 << kConstBits);
        Wrap tmp1 = (z2 - z3) * (1 << kConstBits);
        const Wrap tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = in[56] * qq[56];
        tmp1 = in[40] * qq[40];
        tmp2 = in[24] * qq[24];
        tmp3 = in[8] * qq[8];
        z1 = tmp0 + tmp3;
        z2 = tmp1 + tmp2;
        z3 = tmp0 + tmp2;
        Wrap z4 = tmp1 + tmp3;
        const Wrap z5 = (z3 + z4) * 9633;
        tmp0 *= 2446;
        tmp1 *= 16819;
        tmp2 *= 25172;
        tmp3 *= 12299;
        z1 *= -7373;
        z2 *= -20995;
        z3 *= -16069;
        z4 *= -3196;
        z3 += z5;
        z4 += z5;
        tmp0 += z1 + z3;
        tmp1 += z2 + z4;
        tmp2 += z2 + z3;
        tmp3 += z1 + z4;
        const int n = kConstBits - kPass1Bits;
        ws[8 * 0 + c] = descale(tmp10 + tmp3, n);
        ws[8 * 7 + c] = descale(tmp10 - tmp3, n);
        ws[8 * 1 + c] = descale(tmp11 + tmp2, n);
        ws[8 * 6 + c] = descale(tmp11 - tmp2, n);
        ws[8 * 2 + c] = descale(tmp12 + tmp1, n);
        ws[8 * 5 + c] = descale(tmp12 - tmp1, n);
        ws[8 * 3 + c] = descale(tmp13 + tmp0, n);
        ws[8 * 4 + c] = descale(tmp13 - tmp0, n);
    }
    for (int r = 0; r < 8; r++) {
        const int *w = ws + 8 * r;
        uint8_t *o = out + r * pitch;
        if (w[1] == 0 && w[2] == 0 && w[3] == 0 && w[4] == 0 && w[5] == 0 && w[6] == 0 && w[7] == 0) {
            const uint8_t v = range_limit(descale(w[0], kPass1Bits + 3));
            for (int c = 0; c < 8; c++) o[c] = v;
            continue;
        }
        Wrap z2 = w[2], z3 = w[6];
        Wrap z1 = (z2 + z3) * 4433;
        Wrap tmp2 = z1 + z3 * -15137;
        Wrap tmp3 = z1 + z2 * 6270;
        Wrap tmp0 = (Wrap(w[0]) + w[4]) * (1 << kConstBits);
        Wrap tmp1 = (Wrap(w[0]) - w[4]) * (1 << kConstBits);
        const Wrap tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = w[7];
        tmp1 = w[5];
        tmp2 = w[3];
        tmp3 = w[1];
        z1 = tmp0 + tmp3;
        z2 = tmp1 + tmp2;
        z3 = tmp0 + tmp2;
        Wrap z4 = tmp1 + tmp3;
        const Wrap z5 = (z3 + z4) * 9633;
        tmp0 *= 2446;
        tmp1 *= 16819;
        tmp2 *= 25172;
        tmp3 *= 12299;
        z1 *= -7373;
        z2 *= -20995;
        z3 *= -16069;
        z4 *= -3196;
        z3 += z5;
        z4 += z5;
        tmp0 += z1 + z3;
        tmp1 += z2 + z4;
        tmp2 += z2 + z3;
        tmp3 += z1 + z4;
        const int n = kConstBits + kPass1Bits + 3;
        o[0] = range_limit(descale(tmp10 + tmp3, n));
        o[7] = range_limit(descale(tmp10 - tmp3, n));
        o[1] = range_limit(descale(tmp11 + tmp2, n));
        o[6] = range_limit(descale(tmp11 - tmp2, n));
        o[2] = range_limit(descale(tmp12 + tmp1, n));
        o[5] = range_limit(descale(tmp12 - tmp1, n));
        o[3] = range_limit(descale(tmp13 + tmp0, n));
        o[4] = range_limit(descale(tmp13 - tmp0, n));
    }
}

// ---- jdsample.c: one upsampled chroma sample --------------------------------------------------------------------------------
// plane: the component's samples, `pitch` bytes per row, cw x ch of them real (downsampled_width/height).  hs/vs: the luma
// sampling factors (the chroma ones are 1).  Fancy (triangular) upsampling when cw > 2, as jinit_upsampler picks it; rows above
// the first and below the last replicate the edge row (jdmainct's context pointers).
T4D_JPEG_FN int upsample(const uint8_t *plane, int64_t pitch, int cw, int ch, int hs, int vs, int x, int y)
{
    if (hs == 1) return plane[(int64_t)y * pitch + x];
    const int cx = x >> 1;
    if (cw <= 2) return plane[(int64_t)(vs == 2 ? y >> 1 : y) * pitch + cx];
    const bool odd = x & 1;
    if (vs == 1) {
        const uint8_t *p = plane + (int64_t)y * pitch;
        if (!odd) return cx == 0 ? p[0] : (p[cx] * 3 + p[cx - 1] + 1) >> 2;
        return cx == cw - 1 ? p[cx] : (p[cx] * 3 + p[cx + 1] + 2) >> 2;
    }
    const int r0 = y >> 1;
    int r1 = (y & 1) ? r0 + 1 : r0 - 1;
    r1 = r1 < 0 ? 0 : r1 > ch - 1 ? ch - 1 : r1;
    const uint8_t *p0 = plane + (int64_t)r0 * pitch, *p1 = plane + (int64_t)r1 * pitch;
    const int cs = p0[cx] * 3 + p1[cx];
    if (!odd) return cx == 0 ? (cs * 4 + 8) >> 4 : (cs * 3 + p0[cx - 1] * 3 + p1[cx - 1] + 8) >> 4;
    return cx == cw - 1 ? (cs * 4 + 7) >> 4 : (cs * 3 + p0[cx + 1] * 3 + p1[cx + 1] + 7) >> 4;
}

// ---- jdcolor.c ycc_rgb_convert (SCALEBITS 16, tables built with FIX(x) = x * 65536 + 0.5) ------------------------------------
T4D_JPEG_FN uint8_t clamp255(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

T4D_JPEG_FN void ycc_to_rgb(int y, int cb, int cr, uint8_t *rgb)
{
    const int xb = cb - 128, xr = cr - 128;
    const int64_t half = 1 << 15;
    const int cr_r = (int)((91881 * (int64_t)xr + half) >> 16);
    const int cb_b = (int)((116130 * (int64_t)xb + half) >> 16);
    const int g = (int)((-46802 * (int64_t)xr + (-22554 * (int64_t)xb + half)) >> 16);
    rgb[0] = clamp255(y + cr_r);
    rgb[1] = clamp255(y + g);
    rgb[2] = clamp255(y + cb_b);
}

// ---- geometry of one image --------------------------------------------------------------------------------------------------
struct Geom {
    int32_t hs, vs, bpm;          // luma sampling, blocks per MCU (hs*vs + 2)
    int32_t mcux, mcuy;           // MCUs per row / column
    int64_t n_mcu, n_blocks;
    int32_t pitch[3], rows[3];    // component planes (whole blocks)
    int32_t cw[3], ch[3];         // real samples per component (downsampled_width / height)
    int32_t n_seg;                // restart intervals (1 without DRI)
};

T4D_JPEG_FN Geom geometry(const T4DJpegImage &im)
{
    Geom g;
    g.hs = im.h_samp;
    g.vs = im.v_samp;
    g.bpm = g.hs * g.vs + 2;
    g.mcux = (im.width + 8 * g.hs - 1) / (8 * g.hs);
    g.mcuy = (im.height + 8 * g.vs - 1) / (8 * g.vs);
    g.n_mcu = (int64_t)g.mcux * g.mcuy;
    g.n_blocks = g.n_mcu * g.bpm;
    for (int c = 0; c < 3; c++) {
        const int h = c ? 1 : g.hs, v = c ? 1 : g.vs;
        g.pitch[c] = g.mcux * h * 8;
        g.rows[c] = g.mcuy * v * 8;
        g.cw[c] = (int)(((int64_t)im.width * h + g.hs - 1) / g.hs);
        g.ch[c] = (int)(((int64_t)im.height * v + g.vs - 1) / g.vs);
    }
    g.n_seg = im.restart_interval > 0 ? (int32_t)((g.n_mcu + im.restart_interval - 1) / im.restart_interval) : 1;
    return g;
}

// component of block b of an MCU
T4D_JPEG_FN int block_component(const Geom &g, int b) { return b < g.hs * g.vs ? 0 : b - g.hs * g.vs + 1; }

// (plane x, plane y) of the top-left sample of MCU-order block `blk`
T4D_JPEG_FN void block_origin(const Geom &g, int64_t blk, int *comp, int64_t *x, int64_t *y)
{
    const int64_t mcu = blk / g.bpm;
    const int b = (int)(blk - mcu * g.bpm);
    const int64_t mx = mcu % g.mcux, my = mcu / g.mcux;
    const int c = block_component(g, b);
    *comp = c;
    if (c == 0) {
        *x = (mx * g.hs + b % g.hs) * 8;
        *y = (my * g.vs + b / g.hs) * 8;
    } else {
        *x = mx * 8;
        *y = my * 8;
    }
}

// ---- a lane of the entropy decode ----------------------------------------------------------------------------------------------
enum : int32_t { kErrTruncated = 1, kErrOverrun = 2, kErrCode = 4, kErrRestart = 8 };  // the status bits (include/topo4d_raster.h)

struct Tables {
    const Huff *dc[3], *ac[3];    // per component
};

struct LaneCounts {
    int32_t blocks, dc[3];        // DC symbols met; their differences summed per component
};

// decode from s until the bit position reaches `end` (s becomes the lane's exit state), counting
T4D_JPEG_FN void run_counts(const uint8_t *d, int64_t nb, const Tables &tb, const Geom &g, State &s, int64_t end, LaneCounts &cnt)
{
    cnt = LaneCounts{0, {0, 0, 0}};
    bool bad = false;
    while (s.pos < end) {
        const int c = block_component(g, s.blk);
        int v;
        if (step(d, nb, tb.dc[c], tb.ac[c], s, &v, &bad) == 0) {
            cnt.blocks++;
            cnt.dc[c] = (int32_t)((uint32_t)cnt.dc[c] + (uint32_t)v);   // wraps, as the lanes' prefix sums do
        }
        next_block(s, g.bpm);
    }
}

// decode from s and write coefficients (natural order, DC predicted from pred[]) of MCU-order blocks into cf[blk * 64 ...]:
// blk is the block before the lane's first DC symbol.  A lane that is not the last of its segment stops at bit `end`; the last
// one stops when block blk_limit - 1 is complete, and the segment is truncated if that takes it past `end`.  A chunk boundary
// may fall inside the 1..7 padding bits after the last block: the lane before it is done once block blk_limit - 1 is complete
// and fewer than 8 bits of the segment are left (it does not read the padding as a symbol, though run_counts counted one), and
// the lane after it, whose first block would lie past blk_limit, has nothing to decode.  Eight or more bits after the last block
// are not padding: kErrOverrun.  Returns status bits.
T4D_JPEG_FN int decode_lane(const uint8_t *d, int64_t nb, const Tables &tb, const Geom &g, State s, int64_t end, bool last,
                            int64_t blk, int64_t blk_limit, int32_t *pred, int16_t *cf)
{
    bool bad = false;
    int err = 0;
    if (blk + 1 > blk_limit) return 0;
    for (;;) {
        if (last) {
            if (s.k == 0 && blk + 1 >= blk_limit) break;
            if (s.pos > end + 32) break;
        } else if (s.pos >= end || (s.k == 0 && blk + 1 >= blk_limit && nb * 8 - s.pos < 8)) {
            break;
        }
        const int c = block_component(g, s.blk);
        int v;
        const int idx = step(d, nb, tb.dc[c], tb.ac[c], s, &v, &bad);
        if (idx == 0) {
            if (++blk >= blk_limit) {
                err |= kErrOverrun;
                break;
            }
            pred[c] = (int32_t)((uint32_t)pred[c] + (uint32_t)v);
            cf[blk * 64] = (int16_t)pred[c];
        } else if (idx > 0 && blk >= 0 && blk < blk_limit) {
            cf[blk * 64 + natural(idx)] = (int16_t)v;
        }
        next_block(s, g.bpm);
    }
    if (last && s.pos > end) err |= kErrTruncated;
    if (bad) err |= kErrCode;
    return err;
}

T4D_JPEG_FN Tables tables(const T4DJpegImage &im, const Huff *hf)
{
    Tables t;
    for (int c = 0; c < 3; c++) {
        t.dc[c] = &hf[im.comp_dc[c]];
        t.ac[c] = &hf[4 + im.comp_ac[c]];
    }
    return t;
}

}  // namespace t4d_jpeg
