// t4d_png.hip — lossless PNG encoder for baked UV textures (write_texture(..., encoder="gpu")) and progress renders
// (progress.save_image), on the device.
//
// The file is a plain PNG: signature, IHDR (8-bit, or 16-bit from t4d_png_encode16; no interlace, colour type 0 / 2 / 6 for
// C = 1 / 3 / 4), a 2-byte IDAT with the zlib header, one IDAT per segment, a 4-byte IDAT with the Adler-32 trailer, IEND.  The
// IDAT payloads joined are one zlib stream.  Compression model ("PNG encoder"): every row is filtered with the PNG filter of least sum |int8 residual|,
// the filtered byte stream is cut into independent segments of kSeg bytes, and each segment is one dynamic-Huffman deflate block
// of literals and distance-1 runs (or one stored block where that is smaller), closed by an empty stored block so the next segment
// starts byte-aligned.  Four launches:
//
//  * k_png_filter   one workgroup per row: quantise (float32 [h,w,c] exactly as numpy's (x*255).astype(uint8) on x86-64, or a
//                   float32 [3,h,w] render exactly as torchvision's save_image; or the low 16 bits of an int32 [h,w,c] image as
//                   two bytes, high byte first), score the five filters at a byte distance of bytes per pixel, write filter
//                   byte + filtered row to scratch.  The later launches see filtered bytes only.
//  * k_png_encode   one workgroup per segment: segment into LDS; the parse into literals and distance-1 runs is fixed by the
//                   maximal equal-byte runs (every thread walks its own slice, with run bounds carried in by block scans);
//                   histograms by LDS integer atomics; length-limited Huffman codes (15 / 7 bits); bits OR'ed into LDS words at
//                   offsets from a block scan; CRC-32 of "IDAT" + the bytes and the segment's Adler-32 partial.
//  * k_png_finalize one workgroup: chunk offsets (exclusive scan of the segment sizes), the combined Adler-32, the header and
//                   trailer chunks and the total length.
//  * k_png_assemble one workgroup per segment: length, "IDAT", bytes and CRC of its chunk into the output.
//
// No float atomics, no cross-workgroup flags: kernel boundaries do the ordering.  Every byte the kernels read was written by an
// earlier one, so the file is a pure function of the pixels and the shape.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/topo4d_raster.h"
#include "t4d_block.h"
#include "t4d_host.h"
#include "t4d_png_huff.h"
#include "t4d_quant.h"

namespace {

constexpr int kBlock = 256;
constexpr int kSeg = 16384;                      // filtered bytes per segment (the last one shorter)
constexpr int kSegMaxOut = kSeg + 5;             // stored fallback: one 5-byte block header + the bytes
constexpr int kSlot = 16448;                     // scratch bytes per segment's encoded output (>= kSegMaxOut, 64-B multiple)
constexpr int kOutWords = kSlot / 4;
constexpr int kLit = kPngLit;                    // literal/length alphabet (t4d_png_huff.h)
constexpr int kCl = 19;                          // code-length alphabet
constexpr int kHeadBytes = 8 + 25 + 14;          // signature, IHDR chunk, IDAT(zlib header)
constexpr int kTailBytes = 16 + 12;              // IDAT(Adler-32), IEND
constexpr int kChunkBytes = 12;                  // length + type + CRC around every segment
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kAdlerMod = 65521u;
constexpr int64_t kMaxFiltered = (int64_t)1 << 38;

struct SegInfo {
    uint32_t bytes;                              // encoded bytes in the segment's slot
    uint32_t crc;                                // CRC-32 over "IDAT" + those bytes
    uint32_t adler_a;                            // sum of the filtered bytes, mod 65521
    uint32_t adler_b;                            // sum of (n - i) * byte_i, mod 65521
};

struct Shape {
    int32_t h, w, c;
    int32_t bps;                                 // bytes per sample: 1, or 2 (16-bit, big-endian)
    int64_t row;                                 // filtered bytes per row: 1 + w * c * bps
    int64_t n;                                   // filtered bytes in all: h * row
    int64_t segs;
};

__host__ __device__ inline Shape make_shape(int32_t h, int32_t w, int32_t c, int32_t bps = 1)
{
    Shape s;
    s.h = h; s.w = w; s.c = c; s.bps = bps;
    s.row = 1 + (int64_t)w * c * bps;
    s.n = (int64_t)h * s.row;
    s.segs = (s.n + kSeg - 1) / kSeg;
    return s;
}

__host__ __device__ inline int64_t max_bytes(const Shape &s)
{
    return kHeadBytes + kTailBytes + s.n + s.segs * (kChunkBytes + 5);
}

struct PngLayout {
    size_t filt, slots, info, offs, total;
};

PngLayout png_layout(const Shape &s)
{
    PngLayout L;
    size_t o = 0;
    L.filt = o;  o += align_up((size_t)s.n);
    L.slots = o; o += align_up((size_t)s.segs * kSlot);
    L.info = o;  o += align_up((size_t)s.segs * sizeof(SegInfo));
    L.offs = o;  o += align_up((size_t)s.segs * sizeof(int64_t));
    L.total = o;
    return L;
}

bool shape_ok(int32_t h, int32_t w, int32_t c, int32_t bps = 1)
{
    if (h < 1 || w < 1 || !(c == 1 || c == 3 || c == 4)) return false;
    return make_shape(h, w, c, bps).n <= kMaxFiltered;
}

// deflate length symbols 257..285 (RFC 1951 3.2.5)
__constant__ uint16_t c_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
                                        131, 163, 195, 227, 258};
__constant__ uint8_t c_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint8_t c_cl_order[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
// x^(8 * 2^j) mod the CRC-32 polynomial, j = 0..31, in the reflected form of gf_mul (bit 31 holds x^0)
__constant__ uint32_t c_crc_pw[32] = {
    0x00800000u, 0x00008000u, 0xEDB88320u, 0xB1E6B092u, 0xA06A2517u, 0xED627DAEu, 0x88D14467u, 0xD7BBFE6Au, 0xEC447F11u,
    0x8E7EA170u, 0x6427800Eu, 0x4D47BAE0u, 0x09FE548Fu, 0x83852D0Fu, 0x30362F1Au, 0x7B5A9CC3u, 0x31FEC169u, 0x9FEC022Au,
    0x6C8DEDC4u, 0x15D6874Du, 0x5FDE7A4Eu, 0xBAD90E37u, 0x2E4E5EEFu, 0x4EABA214u, 0xA8A472C0u, 0x429A969Eu, 0x148D302Au,
    0xC40BA6D0u, 0xC4E22C3Cu, 0x40000000u, 0x20000000u, 0x08000000u};

__device__ __forceinline__ int len_index(int l)                  // 3..258 -> 0..28
{
    if (l <= 10) return l - 3;
    if (l == 258) return 28;
    int i = 8;
    while (i < 27 && c_len_base[i + 1] <= l) ++i;
    return i;
}

// ---------------------------------------------------------------------------------------------------------------------------
// quantise + filter
// ---------------------------------------------------------------------------------------------------------------------------
// numpy's float32 -> uint8 cast on x86-64: t4d_quant_u8 (t4d_quant.h, shared with t4d_texture_quantize)

// torchvision's save_image: x.mul(255).add_(0.5).clamp_(0, 255) on the device, then .to("cpu", torch.uint8).  Two roundings, a
// clamp that keeps NaN, and ATen's x86-64 float -> uint8 conversion of the clamped value: truncation toward zero, NaN -> 0.
// hipcc contracts a*b+c into one v_fma_f32 (one rounding) by default, even through __fmul_rn / __fadd_rn: the pragma keeps the
// multiply and the add apart.  (A scan of every float32 in [-0.003, 1.003] found no byte the fused form changes; outside that range
// both clamp.  The pragma keeps the arithmetic torch's all the same.)
__device__ __forceinline__ uint32_t quant_tv(float x)
{
#pragma clang fp contract(off)
    const float m = x * 255.0f;
    const float y = m + 0.5f;
    if (!(y > 0.0f)) return 0u;                                       // also NaN
    if (y >= 255.0f) return 255u;
    return (uint32_t)y;
}

// input forms of k_png_filter
enum PixMode { kU8 = 0, kF32 = 1, kF32Chw = 2, kU16 = 3 };

// byte x of row r of the [h, w*c*bps] image: [h,w,c] uint8 or float32 (numpy's cast), a contiguous [3,h,w] float32 (torchvision's
// rounding), whose byte x is plane x % 3, column x / 3, or [h,w,c] int32 whose sample x / 2 gives its bits 15..8 for even x and its
// bits 7..0 for odd x
template <int MODE>
__device__ __forceinline__ uint32_t pix(const void *img, const Shape &s, int64_t r, int64_t x)
{
    if (MODE == kF32Chw) {
        const int64_t col = x / 3, plane = x - 3 * col;
        return quant_tv(((const float *)img)[(plane * s.h + r) * s.w + col]);
    }
    if (MODE == kU16) {
        const uint32_t v = (uint32_t)((const int32_t *)img)[r * ((int64_t)s.w * s.c) + (x >> 1)];
        return ((x & 1) ? v : v >> 8) & 0xFFu;
    }
    const int64_t i = r * ((int64_t)s.w * s.c) + x;
    if (MODE == kF32) return t4d_quant_u8(((const float *)img)[i]);
    return ((const uint8_t *)img)[i];
}

__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint32_t sabs8(uint32_t r)             // |(int8)r|
{
    const int v = (int)(int8_t)(uint8_t)r;
    return (uint32_t)(v < 0 ? -v : v);
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void k_png_filter(const void *img, Shape s, uint8_t *filt)
{
    __shared__ unsigned long long red[5][kBlock];
    const int64_t r = blockIdx.x;
    const int64_t wc = (int64_t)s.w * s.c * s.bps;               // bytes in the row
    const int c = s.c * s.bps;                                    // bytes per pixel: the filters' byte distance
    unsigned long long sum[5] = {0, 0, 0, 0, 0};
    for (int64_t x = threadIdx.x; x < wc; x += kBlock) {
        const uint32_t v = pix<MODE>(img, s, r, x);
        const uint32_t a = x >= c ? pix<MODE>(img, s, r, x - c) : 0u;
        const uint32_t b = r > 0 ? pix<MODE>(img, s, r - 1, x) : 0u;
        const uint32_t cc = (r > 0 && x >= c) ? pix<MODE>(img, s, r - 1, x - c) : 0u;
        sum[0] += sabs8(v);
        sum[1] += sabs8(v - a);
        sum[2] += sabs8(v - b);
        sum[3] += sabs8(v - ((a + b) >> 1));
        sum[4] += sabs8(v - paeth(a, b, cc));
    }
    for (int f = 0; f < 5; ++f) red[f][threadIdx.x] = sum[f];
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
            for (int f = 0; f < 5; ++f) red[f][threadIdx.x] += red[f][threadIdx.x + st];
        __syncthreads();
    }
    int best = 0;
    for (int f = 1; f < 5; ++f)
        if (red[f][0] < red[best][0]) best = f;                       // strict: the lowest filter number wins a tie
    uint8_t *out = filt + r * s.row;
    if (threadIdx.x == 0) out[0] = (uint8_t)best;
    for (int64_t x = threadIdx.x; x < wc; x += kBlock) {
        const uint32_t v = pix<MODE>(img, s, r, x);
        const uint32_t a = x >= c ? pix<MODE>(img, s, r, x - c) : 0u;
        const uint32_t b = r > 0 ? pix<MODE>(img, s, r - 1, x) : 0u;
        const uint32_t cc = (r > 0 && x >= c) ? pix<MODE>(img, s, r - 1, x - c) : 0u;
        const uint32_t pred = best == 0 ? 0u : best == 1 ? a : best == 2 ? b : best == 3 ? ((a + b) >> 1) : paeth(a, b, cc);
        out[1 + x] = (uint8_t)(v - pred);
    }
}

// reflected CRC-32 arithmetic: a * b mod P, bit 31 holds x^0
__device__ uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// x^(8 * nbytes) mod P from pw[j] = x^(8 * 2^j)
__device__ uint32_t gf_shift(uint64_t nbytes, const uint32_t *pw)
{
    uint32_t r = 0x80000000u;
    for (int j = 0; nbytes; ++j, nbytes >>= 1)
        if (nbytes & 1) r = gf_mul(r, pw[j]);
    return r;
}

__device__ uint32_t crc_bytes(uint32_t crc, const uint8_t *p, int n, const uint32_t *tab)
{
    for (int i = 0; i < n; ++i) crc = tab[(crc ^ p[i]) & 0xFFu] ^ (crc >> 8);
    return crc;
}

// CRC-32 one byte at a time without a table (the few header bytes of k_png_finalize)
__device__ uint32_t crc_slow(uint32_t crc, const uint8_t *p, int n)
{
    for (int i = 0; i < n; ++i) {
        crc ^= p[i];
        for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? (crc >> 1) ^ kCrcPoly : crc >> 1;
    }
    return crc;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Huffman code lengths
// ---------------------------------------------------------------------------------------------------------------------------
// Length-limited code lengths for freq[0..n) (max_bits), written to len[0..n).  A used set of fewer than two symbols is padded to two
// by the caller.  Huffman lengths from the two-queue method over the sorted leaves; leaves deeper than max_bits are clamped and the
// Kraft excess is removed one unit at a time (a leaf at depth b < max_bits moves to b + 1 and takes a clamped leaf as its sibling);
// then the lengths go to the symbols in frequency order.  Deterministic: every tie is broken by the symbol number.
__device__ void huff_lengths(const uint32_t *freq, int n, int max_bits, uint8_t *len, HuffScratch &hs)
{
    const int t = threadIdx.x;
    if (t == 0) hs.count = 0;
    __syncthreads();
    for (int s = t; s < n; s += kBlock) {
        len[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        int rank = 0;
        for (int u = 0; u < n; ++u) {
            const uint32_t g = freq[u];
            rank += (g && (g < f || (g == f && u < s))) ? 1 : 0;
        }
        hs.sorted[rank] = (uint16_t)s;
        hs.w_leaf[rank] = f;
        atomicAdd(&hs.count, 1);
    }
    __syncthreads();
    if (t == 0) t4d_png_huff_assign(max_bits, len, hs);                // t4d_png_huff.h
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------------
// segment encoder
// ---------------------------------------------------------------------------------------------------------------------------
struct EncShared {
    uint8_t in[kSeg];
    uint32_t out[kOutWords + 2];
    uint32_t crc_tab[256];
    uint32_t crc_pw[32];
    uint32_t lit_freq[kLit];
    uint32_t cl_freq[kCl];
    uint8_t lit_len[kLit];
    uint8_t cl_len[kCl];
    uint16_t lit_code[kLit];
    uint16_t cl_code[kCl];
    uint8_t ops_sym[kLit + 2];                   // the code-length sequence, run-length coded with 16 / 17 / 18
    uint8_t ops_arg[kLit + 2];
    int n_ops;
    int n_lit;                                   // HLIT + 257
    int n_cl;                                    // HCLEN + 4
    uint32_t head_bits;
    int use_huffman;
    unsigned long long scan_u64[kBlock];
    int scan_i32[kBlock];
    HuffScratch hs;
};

struct Slice {
    int c0, c1;                                  // this thread's positions [c0, c1)
    int prev_bnd;                                // last run start before c0 (from the threads before)
    int next_bnd;                                // first run start at or after c1, or n
};

__device__ __forceinline__ bool is_bnd(const uint8_t *in, int j) { return j == 0 || in[j] != in[j - 1]; }

// Calls lit(byte) / match(length) for every token whose first position lies in the thread's slice, in stream order.  A maximal run
// [rs, re) of equal bytes is: a literal at rs, matches of 258 (distance 1) over the rest, a last match of the remainder if it is at
// least 3, else that remainder as literals.
template <typename Lit, typename Match>
__device__ void walk_tokens(const uint8_t *in, const Slice &sl, Lit lit, Match match)
{
    int i = sl.c0;
    while (i < sl.c1) {
        const int rs = is_bnd(in, i) ? i : sl.prev_bnd;
        int j = i + 1;
        while (j < sl.c1 && !is_bnd(in, j)) ++j;
        const int re = j < sl.c1 ? j : sl.next_bnd;
        const int lo = i, hi = j;                                     // token starts taken here: [lo, hi)
        if (rs >= lo) lit(in[rs]);
        const int m = re - rs - 1, full = m / 258, rem = m % 258;
        int k = lo > rs + 1 ? (lo - rs - 1 + 257) / 258 : 0;
        for (; k < full; ++k) {
            if (rs + 1 + 258 * k >= hi) break;
            match(258);
        }
        const int p0 = rs + 1 + 258 * full;
        if (rem >= 3) {
            if (p0 >= lo && p0 < hi) match(rem);
        } else {
            for (int p = max(p0, lo); p < min(re, hi); ++p) lit(in[p]);
        }
        i = j;
    }
}

__device__ __forceinline__ void put_bits(uint32_t *out, uint64_t pos, uint32_t v)
{
    const uint64_t x = (uint64_t)v << (pos & 31);
    const uint64_t w = pos >> 5;
    if ((uint32_t)x) atomicOr(&out[w], (uint32_t)x);
    if ((uint32_t)(x >> 32)) atomicOr(&out[w + 1], (uint32_t)(x >> 32));
}

// thread 0: the code-length sequence of lit_len (n_lit entries) then the one distance length, run-length coded like zlib
__device__ void code_length_ops(EncShared &S)
{
    int n = 0;
    auto rle = [&](const uint8_t *l, int cnt) {
        int i = 0;
        while (i < cnt) {
            const uint8_t v = l[i];
            int run = 1;
            while (i + run < cnt && l[i + run] == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int k = min(run, 138); S.ops_sym[n] = 18; S.ops_arg[n++] = (uint8_t)(k - 11); run -= k; }
                if (run >= 3) { S.ops_sym[n] = 17; S.ops_arg[n++] = (uint8_t)(run - 3); run = 0; }
                while (run-- > 0) { S.ops_sym[n] = 0; S.ops_arg[n++] = 0; }
            } else {
                S.ops_sym[n] = v; S.ops_arg[n++] = 0; --run;
                while (run >= 3) { const int k = min(run, 6); S.ops_sym[n] = 16; S.ops_arg[n++] = (uint8_t)(k - 3); run -= k; }
                while (run-- > 0) { S.ops_sym[n] = v; S.ops_arg[n++] = 0; }
            }
        }
    };
    rle(S.lit_len, S.n_lit);
    const uint8_t one = 1;                                            // the single distance code: symbol 0 (distance 1), length 1
    rle(&one, 1);
    S.n_ops = n;
}

__device__ __forceinline__ int cl_extra(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

__global__ __launch_bounds__(kBlock) void k_png_encode(const uint8_t *filt, Shape s, uint8_t *slots, SegInfo *info)
{
    __shared__ EncShared S;
    const int t = threadIdx.x;
    const int64_t seg = blockIdx.x;
    const int64_t base = seg * kSeg;
    const int n = (int)min((int64_t)kSeg, s.n - base);
    const bool last = seg == s.segs - 1;

    // segment -> LDS; zero the output words and the histograms; CRC tables
    for (int i = t; i < n; i += kBlock) S.in[i] = filt[base + i];
    for (int i = t; i < kOutWords + 2; i += kBlock) S.out[i] = 0;
    for (int i = t; i < kLit; i += kBlock) S.lit_freq[i] = 0;
    if (t < kCl) S.cl_freq[t] = 0;
    {
        uint32_t c = (uint32_t)t;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        S.crc_tab[t] = c;
    }
    if (t < 32) S.crc_pw[t] = c_crc_pw[t];
    __syncthreads();

    // this thread's slice and the run bounds carried across slices
    const int K = (n + kBlock - 1) / kBlock;
    Slice sl;
    sl.c0 = min(t * K, n);
    sl.c1 = min(sl.c0 + K, n);
    int lmax = -1, lmin = n;
    for (int j = sl.c0; j < sl.c1; ++j)
        if (is_bnd(S.in, j)) { lmax = j; if (lmin == n) lmin = j; }
    sl.prev_bnd = block_exclusive_scan<kBlock, int>(lmax, -1, S.scan_i32, [](int a, int b) { return max(a, b); }, nullptr);
    {
        // suffix min: the exclusive prefix min over the reversed thread order
        S.scan_i32[t] = lmin;
        __syncthreads();
        const int rv = S.scan_i32[kBlock - 1 - t];
        __syncthreads();
        const int e = block_exclusive_scan<kBlock, int>(rv, n, S.scan_i32, [](int a, int b) { return min(a, b); }, nullptr);
        S.scan_i32[kBlock - 1 - t] = e;
        __syncthreads();
        sl.next_bnd = S.scan_i32[t];
        __syncthreads();
    }

    // histograms
    walk_tokens(S.in, sl, [&](uint32_t b) { atomicAdd(&S.lit_freq[b], 1u); },
                [&](int l) { atomicAdd(&S.lit_freq[257 + len_index(l)], 1u); });
    if (t == 0) S.lit_freq[256] += 1;                                 // end of block
    __syncthreads();
    if (t == 0) {
        int used = 0;
        for (int i = 0; i < kLit; ++i) used += S.lit_freq[i] ? 1 : 0;
        if (used < 2) S.lit_freq[S.lit_freq[0] ? 1 : 0] = 1;          // a complete code needs two symbols
    }
    __syncthreads();
    huff_lengths(S.lit_freq, kLit, 15, S.lit_len, S.hs);
    if (t == 0) {
        t4d_png_canonical_codes(S.lit_len, kLit, S.lit_code, S.hs);
        int nl = kLit;
        while (nl > 257 && S.lit_len[nl - 1] == 0) --nl;
        S.n_lit = nl;
        code_length_ops(S);
        for (int i = 0; i < S.n_ops; ++i) S.cl_freq[S.ops_sym[i]]++;
        int used = 0;
        for (int i = 0; i < kCl; ++i) used += S.cl_freq[i] ? 1 : 0;
        if (used < 2) S.cl_freq[S.cl_freq[0] ? 1 : 0] = 1;
    }
    __syncthreads();
    huff_lengths(S.cl_freq, kCl, 7, S.cl_len, S.hs);
    if (t == 0) {
        t4d_png_canonical_codes(S.cl_len, kCl, S.cl_code, S.hs);
        int nc = kCl;
        while (nc > 4 && S.cl_len[c_cl_order[nc - 1]] == 0) --nc;
        S.n_cl = nc;
        uint32_t bits = 3 + 5 + 5 + 4 + 3 * nc;
        for (int i = 0; i < S.n_ops; ++i) bits += S.cl_len[S.ops_sym[i]] + cl_extra(S.ops_sym[i]);
        S.head_bits = bits;
    }
    __syncthreads();

    // bits of this thread's tokens, their offsets, and the choice between Huffman and stored
    unsigned long long my_bits = 0;
    walk_tokens(S.in, sl, [&](uint32_t b) { my_bits += S.lit_len[b]; },
                [&](int l) { const int li = len_index(l); my_bits += S.lit_len[257 + li] + c_len_extra[li] + 1; });
    unsigned long long data_bits = 0;
    const unsigned long long my_off = block_exclusive_scan<kBlock>(my_bits, S.scan_u64, &data_bits);
    const uint64_t end_bits = S.head_bits + data_bits + S.lit_len[256];
    const uint64_t sync_at = last ? 0 : (end_bits + 3 + 7) / 8;       // byte of the empty stored block's LEN
    const uint64_t huff_bytes = last ? (end_bits + 7) / 8 : sync_at + 4;
    const bool huff = huff_bytes < (uint64_t)n + 5;

    uint8_t *ob = (uint8_t *)S.out;
    uint32_t out_bytes;
    if (huff) {
        if (t == 0) {
            uint64_t p = 0;
            put_bits(S.out, p, (last ? 1u : 0u) | (2u << 1)); p += 3;   // BFINAL, BTYPE = 10 (dynamic)
            put_bits(S.out, p, (uint32_t)(S.n_lit - 257)); p += 5;
            put_bits(S.out, p, 0u); p += 5;                              // HDIST + 1 = 1
            put_bits(S.out, p, (uint32_t)(S.n_cl - 4)); p += 4;
            for (int i = 0; i < S.n_cl; ++i) { put_bits(S.out, p, S.cl_len[c_cl_order[i]]); p += 3; }
            for (int i = 0; i < S.n_ops; ++i) {
                const int sym = S.ops_sym[i];
                put_bits(S.out, p, S.cl_code[sym]); p += S.cl_len[sym];
                const int e = cl_extra(sym);
                if (e) { put_bits(S.out, p, S.ops_arg[i]); p += e; }
            }
            put_bits(S.out, S.head_bits + data_bits, S.lit_code[256]);  // end of block
        }
        uint64_t p = S.head_bits + my_off;
        walk_tokens(S.in, sl,
                    [&](uint32_t b) { put_bits(S.out, p, S.lit_code[b]); p += S.lit_len[b]; },
                    [&](int l) {
                        const int li = len_index(l), sym = 257 + li;
                        const uint32_t ll = S.lit_len[sym], e = c_len_extra[li];
                        // length code, length extra bits, distance code 0 (one bit, 0), no distance extra bits
                        put_bits(S.out, p, (uint32_t)S.lit_code[sym] | ((uint32_t)(l - c_len_base[li]) << ll));
                        p += ll + e + 1;
                    });
        __syncthreads();
        if (t == 0 && !last) { ob[sync_at + 2] = 0xFF; ob[sync_at + 3] = 0xFF; }   // 00 00 FF FF after three zero bits
        out_bytes = (uint32_t)huff_bytes;
    } else {
        if (t == 0) {
            ob[0] = last ? 1 : 0;                                     // BFINAL, BTYPE = 00 (stored), padding
            ob[1] = (uint8_t)n; ob[2] = (uint8_t)(n >> 8);
            ob[3] = (uint8_t)~n; ob[4] = (uint8_t)(~n >> 8);
        }
        for (int i = t; i < n; i += kBlock) ob[5 + i] = S.in[i];
        out_bytes = (uint32_t)n + 5;
    }
    __syncthreads();

    // slot out, CRC-32 over "IDAT" + bytes (per-thread pieces combined by crc(A||B) = crc(A) x^(8|B|) + crc(B)), Adler partial
    uint32_t *slot = (uint32_t *)(slots + seg * (int64_t)kSlot);
    const int words = (int)((out_bytes + 3) / 4);
    for (int i = t; i < words; i += kBlock) slot[i] = S.out[i];
    const int KC = (int)((out_bytes + kBlock - 1) / kBlock);
    const int b0 = min(t * KC, (int)out_bytes), b1 = min(b0 + KC, (int)out_bytes);
    uint32_t crc = ~crc_bytes(0xFFFFFFFFu, ob + b0, b1 - b0, S.crc_tab);
    crc = gf_mul(crc, gf_shift(out_bytes - b1, S.crc_pw));
    if (t == 0) {
        const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
        const uint32_t c_idat = ~crc_bytes(0xFFFFFFFFu, idat, 4, S.crc_tab);
        crc ^= gf_mul(c_idat, gf_shift(out_bytes, S.crc_pw));
    }
    unsigned long long a = 0, b = 0;
    for (int i = t; i < n; i += kBlock) { a += S.in[i]; b += (unsigned long long)(n - i) * S.in[i]; }
    S.scan_i32[t] = (int)crc;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if (t < st) S.scan_i32[t] ^= S.scan_i32[t + st];
        __syncthreads();
    }
    unsigned long long sa = 0, sb = 0;
    block_exclusive_scan<kBlock>(a, S.scan_u64, &sa);
    block_exclusive_scan<kBlock>(b, S.scan_u64, &sb);
    if (t == 0) {
        SegInfo si;
        si.bytes = out_bytes;
        si.crc = (uint32_t)S.scan_i32[0];
        si.adler_a = (uint32_t)(sa % kAdlerMod);
        si.adler_b = (uint32_t)(sb % kAdlerMod);
        info[seg] = si;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// chunk offsets, header, trailer
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// a chunk of `len` data bytes already at p + 8: writes its length, type and CRC
__device__ void close_chunk(uint8_t *p, const char *type, uint32_t len)
{
    put_be32(p, len);
    for (int i = 0; i < 4; ++i) p[4 + i] = (uint8_t)type[i];
    put_be32(p + 8 + len, ~crc_slow(0xFFFFFFFFu, p + 4, 4 + (int)len));
}

__global__ __launch_bounds__(kBlock) void k_png_finalize(Shape s, const SegInfo *info, int64_t *offs, uint8_t *out, int64_t capacity,
                                                         int64_t *out_bytes)
{
    __shared__ unsigned long long tmp[kBlock];
    const int t = threadIdx.x;
    const int64_t per = (s.segs + kBlock - 1) / kBlock;
    const int64_t k0 = min((int64_t)t * per, s.segs), k1 = min(k0 + per, s.segs);
    unsigned long long sum = 0, a = 0, b = 0;
    const uint64_t N = (uint64_t)s.n;
    for (int64_t k = k0; k < k1; ++k) {
        const SegInfo si = info[k];
        sum += kChunkBytes + si.bytes;
        const uint64_t nk = (uint64_t)min((int64_t)kSeg, s.n - k * kSeg);
        const uint64_t after = (N - (uint64_t)k * kSeg - nk) % kAdlerMod;     // bytes after the segment
        a += si.adler_a;
        b += si.adler_b + after * si.adler_a % kAdlerMod;
    }
    unsigned long long total = 0, ta = 0, tb = 0;
    unsigned long long o = block_exclusive_scan<kBlock>(sum, tmp, &total);
    block_exclusive_scan<kBlock>(a % kAdlerMod, tmp, &ta);
    block_exclusive_scan<kBlock>(b % kAdlerMod, tmp, &tb);
    o += kHeadBytes;
    for (int64_t k = k0; k < k1; ++k) {
        offs[k] = (int64_t)o;
        o += kChunkBytes + info[k].bytes;
    }
    if (t != 0) return;
    const int64_t all = kHeadBytes + (int64_t)total + kTailBytes;
    if (all > capacity) { *out_bytes = -1; return; }                 // cannot happen: all <= max_bytes(s) <= capacity
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    for (int i = 0; i < 8; ++i) out[i] = sig[i];
    uint8_t *p = out + 8;
    put_be32(p + 8, (uint32_t)s.w);
    put_be32(p + 12, (uint32_t)s.h);
    p[16] = (uint8_t)(8 * s.bps);                                     // bit depth
    p[17] = s.c == 1 ? 0 : s.c == 3 ? 2 : 6;                          // grey, RGB, RGBA
    p[18] = 0; p[19] = 0; p[20] = 0;                                  // deflate, adaptive filtering, no interlace
    close_chunk(p, "IHDR", 13);
    p += 25;
    p[8] = 0x78; p[9] = 0x01;                                         // zlib: deflate, 32 KiB window; (0x7801 % 31) == 0
    close_chunk(p, "IDAT", 2);
    p = out + kHeadBytes + total;
    const uint32_t aa = (uint32_t)((1 + ta) % kAdlerMod);
    const uint32_t bb = (uint32_t)((N % kAdlerMod + tb) % kAdlerMod);
    put_be32(p + 8, (bb << 16) | aa);
    close_chunk(p, "IDAT", 4);
    close_chunk(p + 16, "IEND", 0);
    *out_bytes = all;
}

__global__ __launch_bounds__(kBlock) void k_png_assemble(Shape s, const uint8_t *slots, const SegInfo *info, const int64_t *offs,
                                                         uint8_t *out, int64_t capacity)
{
    const int64_t k = blockIdx.x;
    const SegInfo si = info[k];
    const int64_t o = offs[k];
    if (o < 0 || o + kChunkBytes + (int64_t)si.bytes > capacity || si.bytes > (uint32_t)kSegMaxOut) return;
    uint8_t *p = out + o;
    const uint8_t *src = slots + k * (int64_t)kSlot;
    const int t = threadIdx.x;
    if (t < 4) p[t] = (uint8_t)(si.bytes >> (24 - 8 * t));
    else if (t < 8) p[t] = (uint8_t)("IDAT"[t - 4]);
    else if (t < 12) p[8 + si.bytes + (t - 8)] = (uint8_t)(si.crc >> (24 - 8 * (t - 8)));
    for (uint32_t i = t; i < si.bytes; i += kBlock) p[8 + i] = src[i];
}

// the three launches after k_png_filter, on the filtered rows at scratch + L.filt
void launch_deflate(const Shape &s, const PngLayout &L, void *scratch, uint8_t *out, size_t out_capacity, int64_t *out_bytes,
                    hipStream_t stream)
{
    char *b = (char *)scratch;
    const uint8_t *filt = (const uint8_t *)(b + L.filt);
    uint8_t *slots = (uint8_t *)(b + L.slots);
    SegInfo *info = (SegInfo *)(b + L.info);
    int64_t *offs = (int64_t *)(b + L.offs);
    hipLaunchKernelGGL(k_png_encode, dim3((unsigned)s.segs), dim3(kBlock), 0, stream, filt, s, slots, info);
    hipLaunchKernelGGL(k_png_finalize, dim3(1), dim3(kBlock), 0, stream, s, info, offs, out, (int64_t)out_capacity, out_bytes);
    hipLaunchKernelGGL(k_png_assemble, dim3((unsigned)s.segs), dim3(kBlock), 0, stream, s, slots, info, offs, out,
                       (int64_t)out_capacity);
}

}  // namespace

T4D_EXPORT size_t t4d_png_max_bytes(int32_t h, int32_t w, int32_t c)
{
    if (!shape_ok(h, w, c)) {
        t4d_fail(T4D_ERR_ARG, "t4d_png_max_bytes: need h, w >= 1, c in {1, 3, 4} and h*(1+w*c) <= 2^38");
        return 0;
    }
    return (size_t)max_bytes(make_shape(h, w, c));
}

T4D_EXPORT size_t t4d_png_scratch_bytes(int32_t h, int32_t w, int32_t c)
{
    if (!shape_ok(h, w, c)) {
        t4d_fail(T4D_ERR_ARG, "t4d_png_scratch_bytes: need h, w >= 1, c in {1, 3, 4} and h*(1+w*c) <= 2^38");
        return 0;
    }
    return png_layout(make_shape(h, w, c)).total;
}

T4D_EXPORT int t4d_png_encode(const void *image, int32_t is_float32, int32_t h, int32_t w, int32_t c, uint8_t *out, size_t out_capacity,
                              int64_t *out_bytes, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!image || !out || !out_bytes || !scratch || (is_float32 != 0 && is_float32 != 1) || !shape_ok(h, w, c))
        return t4d_fail(T4D_ERR_ARG, "t4d_png_encode: bad arguments");
    const Shape s = make_shape(h, w, c);
    if (out_capacity < (size_t)max_bytes(s))
        return t4d_fail(T4D_ERR_ARG, "t4d_png_encode: out_capacity below t4d_png_max_bytes");
    const PngLayout L = png_layout(s);
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_png_encode: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    uint8_t *filt = (uint8_t *)((char *)scratch + L.filt);
    if (is_float32) hipLaunchKernelGGL(k_png_filter<kF32>, dim3((unsigned)h), dim3(kBlock), 0, stream, image, s, filt);
    else hipLaunchKernelGGL(k_png_filter<kU8>, dim3((unsigned)h), dim3(kBlock), 0, stream, image, s, filt);
    launch_deflate(s, L, scratch, out, out_capacity, out_bytes, stream);
    return t4d_launch_status("t4d_png_encode");
}

T4D_EXPORT int t4d_png_encode_chw(const float *image, int32_t h, int32_t w, uint8_t *out, size_t out_capacity, int64_t *out_bytes,
                                  void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!image || !out || !out_bytes || !scratch || !shape_ok(h, w, 3))
        return t4d_fail(T4D_ERR_ARG, "t4d_png_encode_chw: bad arguments (NULL buffer, or h, w < 1 or h*(1+3w) > 2^38)");
    const Shape s = make_shape(h, w, 3);
    if (out_capacity < (size_t)max_bytes(s))
        return t4d_fail(T4D_ERR_ARG, "t4d_png_encode_chw: out_capacity below t4d_png_max_bytes(h, w, 3)");
    const PngLayout L = png_layout(s);
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_png_encode_chw: scratch below t4d_png_scratch_bytes(h, w, 3)");
    hipStream_t stream = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_png_filter<kF32Chw>, dim3((unsigned)h), dim3(kBlock), 0, stream, (const void *)image, s,
                       (uint8_t *)((char *)scratch + L.filt));
    launch_deflate(s, L, scratch, out, out_capacity, out_bytes, stream);
    return t4d_launch_status("t4d_png_encode_chw");
}

T4D_EXPORT size_t t4d_png_max_bytes16(int32_t h, int32_t w, int32_t c)
{
    if (!shape_ok(h, w, c, 2)) {
        t4d_fail(T4D_ERR_ARG, "t4d_png_max_bytes16: need h, w >= 1, c in {1, 3, 4} and h*(1+2*w*c) <= 2^38");
        return 0;
    }
    return (size_t)max_bytes(make_shape(h, w, c, 2));
}

T4D_EXPORT size_t t4d_png_scratch_bytes16(int32_t h, int32_t w, int32_t c)
{
    if (!shape_ok(h, w, c, 2)) {
        t4d_fail(T4D_ERR_ARG, "t4d_png_scratch_bytes16: need h, w >= 1, c in {1, 3, 4} and h*(1+2*w*c) <= 2^38");
        return 0;
    }
    return png_layout(make_shape(h, w, c, 2)).total;
}

T4D_EXPORT int t4d_png_encode16(const int32_t *image, int32_t h, int32_t w, int32_t c, uint8_t *out, size_t out_capacity,
                                int64_t *out_bytes, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!image || !out || !out_bytes || !scratch || !shape_ok(h, w, c, 2))
        return t4d_fail(T4D_ERR_ARG, "t4d_png_encode16: bad arguments (NULL buffer, or h, w < 1, c not in {1, 3, 4} or h*(1+2*w*c) > 2^38)");
    const Shape s = make_shape(h, w, c, 2);
    if (out_capacity < (size_t)max_bytes(s))
        return t4d_fail(T4D_ERR_ARG, "t4d_png_encode16: out_capacity below t4d_png_max_bytes16");
    const PngLayout L = png_layout(s);
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_png_encode16: scratch below t4d_png_scratch_bytes16");
    hipStream_t stream = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_png_filter<kU16>, dim3((unsigned)h), dim3(kBlock), 0, stream, (const void *)image, s,
                       (uint8_t *)((char *)scratch + L.filt));
    launch_deflate(s, L, scratch, out, out_capacity, out_bytes, stream);
    return t4d_launch_status("t4d_png_encode16");
}
