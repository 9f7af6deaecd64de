// t4d_jpeg_fdct.h — the per-block arithmetic of the baseline JPEG encoder (csrc/t4d_jpegenc.hip), shared with a host build
// (tests/native/jpegenc_host.cpp): libjpeg's RGB -> YCbCr, its edge rules and h2v1 / h2v2 downsampling, jfdctint's two passes,
// the quantiser, and the tables of a file written with jpeg_set_quality and the Annex K Huffman tables.  It is the arithmetic of
// csrc/t4d_jpeg.h (the decoder) run forwards.  Nothing here launches anything; every function is plain integer C++.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define T4D_JE_HD __host__ __device__ inline
#else
#define T4D_JE_HD inline
#endif

constexpr int kJpegEncHeaderBytes = 623;              // SOI .. SOS of a three-component file with two DQT and four DHT segments
constexpr int kJpegEncSofAt = 2 + 18 + 2 * 69;        // offset of the SOF0 marker; height is at +5, width at +7, luma sampling at +11
// bits of one block, at most: a DC code of <= 11 bits + 11 value bits, 63 AC codes of <= 16 bits + 10 value bits
constexpr int kJpegEncBlockMaxBits = 22 + 63 * 26;
constexpr int kJpegEncBlockWords = (kJpegEncBlockMaxBits + 31) / 32;

// jpeg_natural_order: zig-zag position -> natural index
constexpr uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1 / K.2
constexpr uint8_t kJpegLumaQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                    14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kJpegChromaQ[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                      99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: DC luma, DC chroma (12 values each), AC luma, AC chroma (162 values each)
constexpr uint8_t kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                        {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kJpegAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// the codes an encoder looks up (jpeg_make_c_derived_tbl): length << 16 | code; table 0 luma, 1 chroma
struct T4DJpegHuffEnc {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
    uint8_t zz_of[64];                                // natural index -> zig-zag position
};

constexpr T4DJpegHuffEnc t4d_jpeg_make_huff()
{
    T4DJpegHuffEnc t = {};
    for (int tab = 0; tab < 2; ++tab) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kJpegDcBits[tab][len - 1]; ++i) t.dc[tab][k++] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kJpegAcBits[tab][len - 1]; ++i) t.ac[tab][kJpegAcVals[tab][k++]] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
    }
    for (int z = 0; z < 64; ++z) t.zz_of[kJpegZigzag[z]] = (uint8_t)z;
    return t;
}

// luma sampling factors of subsampling 0 (4:4:4), 1 (4:2:2), 2 (4:2:0); chroma is 1 x 1
T4D_JE_HD int t4d_jpeg_hs(int subsampling) { return subsampling == 0 ? 1 : 2; }
T4D_JE_HD int t4d_jpeg_vs(int subsampling) { return subsampling == 2 ? 2 : 1; }

// jpeg_set_quality(quality, force_baseline = TRUE): both tables in natural order
inline void t4d_jpeg_quant_tables(int quality, uint16_t luma[64], uint16_t chroma[64])
{
    const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; ++i) {
        const int a = (kJpegLumaQ[i] * scale + 50) / 100, b = (kJpegChromaQ[i] * scale + 50) / 100;
        luma[i] = (uint16_t)(a < 1 ? 1 : a > 255 ? 255 : a);
        chroma[i] = (uint16_t)(b < 1 ? 1 : b > 255 ? 255 : b);
    }
}

// The kJpegEncHeaderBytes bytes before the entropy-coded segment: SOI, JFIF APP0 (1.01, no units, density 1 x 1), one DQT per
// table, SOF0, the Annex K DHTs (DC 0, AC 0, DC 1, AC 1), SOS.
inline void t4d_jpeg_header(uint8_t *out, int height, int width, int quality, int subsampling)
{
    uint16_t qt[2][64];
    t4d_jpeg_quant_tables(quality, qt[0], qt[1]);
    uint8_t *p = out;
    auto put = [&](int v) { *p++ = (uint8_t)v; };
    auto marker = [&](int m, int len) { put(0xFF); put(m); put(len >> 8); put(len); };
    put(0xFF); put(0xD8);
    marker(0xE0, 16);
    for (char c : {'J', 'F', 'I', 'F'}) put(c);
    for (int v : {0, 1, 1, 0, 0, 1, 0, 1, 0, 0}) put(v);
    for (int t = 0; t < 2; ++t) {
        marker(0xDB, 67);
        put(t);
        for (int z = 0; z < 64; ++z) put(qt[t][kJpegZigzag[z]]);
    }
    marker(0xC0, 17);
    put(8); put(height >> 8); put(height); put(width >> 8); put(width); put(3);
    put(1); put((t4d_jpeg_hs(subsampling) << 4) | t4d_jpeg_vs(subsampling)); put(0);
    put(2); put(0x11); put(1);
    put(3); put(0x11); put(1);
    for (int t = 0; t < 2; ++t) {
        marker(0xC4, 31);
        put(t);
        for (int i = 0; i < 16; ++i) put(kJpegDcBits[t][i]);
        for (int i = 0; i < 12; ++i) put(i);
        marker(0xC4, 181);
        put(0x10 | t);
        for (int i = 0; i < 16; ++i) put(kJpegAcBits[t][i]);
        for (int i = 0; i < 162; ++i) put(kJpegAcVals[t][i]);
    }
    marker(0xDA, 12);
    for (int v : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) put(v);
}

// ---- samples -----------------------------------------------------------------------------------------------------------------
// rgb_ycc_convert: FIX(x) = int(x * 65536 + 0.5); component 0 Y, 1 Cb, 2 Cr
T4D_JE_HD int t4d_jpeg_ycc(int comp, int r, int g, int b)
{
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    const int off = (128 << 16) + 32768 - 1;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + off) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + off) >> 16;
}

T4D_JE_HD int t4d_jpeg_pixel(const uint8_t *src, int64_t pitch, int comp, int x, int y)
{
    const uint8_t *p = src + (int64_t)y * pitch + 3 * (int64_t)x;
    return t4d_jpeg_ycc(comp, p[0], p[1], p[2]);
}

// Sample (x, y) of component `comp`'s plane padded to whole MCUs (x, y in the component's own, downsampled grid).
// Columns: the full-size row is edge-replicated, then downsampled (expand_right_edge before h2v*_downsample).  Rows: the full-size
// image is replicated only to a whole row group; below the last downsampled row that row is repeated (expand_bottom_edge of the
// output) - in 4:2:0 with an even height that is the mean of the last two rows, not the last row alone.
// h2v1: (a + b + bias) >> 1, bias 0, 1, 0, 1.. along x; h2v2: (sum of 4 + bias) >> 2, bias 1, 2, 1, 2..
T4D_JE_HD int t4d_jpeg_sample(const uint8_t *src, int64_t pitch, int width, int height, int subsampling, int comp, int x, int y)
{
    if (comp == 0 || subsampling == 0) {
        x = x < width ? x : width - 1;
        y = y < height ? y : height - 1;
        return t4d_jpeg_pixel(src, pitch, comp, x, y);
    }
    const int x0 = 2 * x < width ? 2 * x : width - 1, x1 = 2 * x + 1 < width ? 2 * x + 1 : width - 1;
    if (subsampling == 1) {
        y = y < height ? y : height - 1;
        return (t4d_jpeg_pixel(src, pitch, comp, x0, y) + t4d_jpeg_pixel(src, pitch, comp, x1, y) + (x & 1)) >> 1;
    }
    const int last = (height + 1) / 2 - 1;
    y = y < last ? y : last;
    const int y0 = 2 * y, y1 = 2 * y + 1 < height ? 2 * y + 1 : height - 1;
    return (t4d_jpeg_pixel(src, pitch, comp, x0, y0) + t4d_jpeg_pixel(src, pitch, comp, x1, y0) + t4d_jpeg_pixel(src, pitch, comp, x0, y1)
            + t4d_jpeg_pixel(src, pitch, comp, x1, y1) + 1 + (x & 1)) >> 2;
}

// ---- jfdctint (ISLOW): CONST_BITS 13, PASS1_BITS 2 -----------------------------------------------------------------------------
// One pass over 8 values in place.  FIRST: the row pass (results scaled up by 4); otherwise the column pass (the scaling of the
// row pass removed; the result stays 8 times the true DCT, which the quantiser divides out).  int32 is enough: samples are
// -128..127, so the row pass stays under 2^23 before its shift and the column pass under 2^31.
template <bool FIRST>
T4D_JE_HD void t4d_fdct_pass(int d[8])
{
    constexpr int n = FIRST ? 11 : 15;
    const int round = 1 << (n - 1);
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) * 4;
        d[4] = (t10 - t11) * 4;
    } else {
        d[0] = (t10 + t11 + 2) >> 2;
        d[4] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    d[2] = (z1 + t13 * 6270 + round) >> n;
    d[6] = (z1 - t12 * 15137 + round) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = (t4 + z1 + z3 + round) >> n;
    d[5] = (t5 + z2 + z4 + round) >> n;
    d[3] = (t6 + z2 + z3 + round) >> n;
    d[1] = (t7 + z1 + z4 + round) >> n;
}

// libjpeg's quantiser on jfdctint's output (8 times the DCT): sign(c) * ((|c| + (8q >> 1)) / 8q)
T4D_JE_HD int t4d_jpeg_quantize(int c, int q)
{
    const int q8 = 8 * q, m = ((c < 0 ? -c : c) + (q8 >> 1)) / q8;
    return c < 0 ? -m : m;
}

// Quantised coefficients, natural order, of block (bx, by) of component `comp`'s own grid; q: that component's table in natural
// order.  The whole-block form of what the kernel spreads over eight lanes.
T4D_JE_HD void t4d_jpeg_block(const uint8_t *src, int64_t pitch, int width, int height, int subsampling, int comp, int bx, int by,
                              const uint16_t *q, int16_t out[64])
{
    int v[64];
    for (int r = 0; r < 8; ++r) {
        int d[8];
        for (int c = 0; c < 8; ++c) d[c] = t4d_jpeg_sample(src, pitch, width, height, subsampling, comp, bx * 8 + c, by * 8 + r) - 128;
        t4d_fdct_pass<true>(d);
        for (int c = 0; c < 8; ++c) v[r * 8 + c] = d[c];
    }
    for (int c = 0; c < 8; ++c) {
        int d[8];
        for (int r = 0; r < 8; ++r) d[r] = v[r * 8 + c];
        t4d_fdct_pass<false>(d);
        for (int r = 0; r < 8; ++r) out[r * 8 + c] = (int16_t)t4d_jpeg_quantize(d[r], q[r * 8 + c]);
    }
}

// bits in the magnitude of v (libjpeg's nbits), 0 for 0
T4D_JE_HD int t4d_jpeg_category(int v)
{
    unsigned m = (unsigned)(v < 0 ? -v : v);
    int n = 0;
    while (m) { ++n; m >>= 1; }
    return n;
}
