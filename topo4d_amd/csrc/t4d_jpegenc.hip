// t4d_jpegenc.hip — baseline JPEG encoder for prepared capture trees (topo4d_amd/jpeg.py, topo4d_amd/prepare.py), on the device.
//
// A batch of n uint8 [H,W,3] RGB images of mixed sizes becomes n complete JFIF files, each byte-identical to what libjpeg-turbo
// writes for jpeg_set_quality(quality) with the Annex K Huffman tables (PIL's save(..., quality=q, subsampling=s)): csrc/
// t4d_jpeg_fdct.h holds the arithmetic and the rules, this file the schedule.  Blocks are numbered in scan order, MCU by MCU,
// per image; images follow each other.  Launches, all on the caller's stream, none synchronising:
//
//  * k_enc_plan     one thread: per-image geometry and the prefix sums every later launch finds its image by; quantisation tables
//                   and the file header template into scratch.
//  * k_enc_dct      eight lanes per 8 x 8 block, one row each; a workgroup takes whole MCUs.  Colour conversion, edge replication and
//                   chroma downsampling on load, the row pass in registers, the transpose through LDS, the column pass, the
//                   quantiser.  Dummy blocks (luma blocks of the last MCU column / row outside the component's own block grid) get
//                   zero AC terms and the DC of the block before them in the MCU.  int16 coefficients out, zig-zag order.
//  * k_enc_size     one thread per block: the bits of its codes from its coefficients and the DC of its component's previous block
//                   in scan order (a lookup, not a chain); the sum of each 256-block chunk.
//  * k_enc_scan     one workgroup per image: exclusive int64 scan of the chunk sums; the image's bit count.
//  * k_enc_zero     clears the words of each image's bit buffer that the emit will touch.
//  * k_enc_emit     one thread per block: its codes at its bit offset, MSB first, into big-endian 32-bit words.  A block's first and
//                   last words may be shared with its neighbours and take a vector atomic OR; the words between are its own.
//                   OR is commutative, so the words are the same for every launch shape and order.
//  * k_enc_count    per 4096-byte chunk of the stream (its last byte padded with 1-bits): the 0xFF bytes.
//  * k_enc_scan     again, over those counts.
//  * k_enc_scatter  header, the stream with a 0x00 after every 0xFF, EOI; the file's length to out_bytes[i].
//
// No float arithmetic, no cross-workgroup flags: kernel boundaries do the ordering, and every byte a kernel reads was written by an
// earlier one (scratch may hold anything on entry).  Nothing is written to `out` beyond a file's length.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_block.h"
#include "t4d_host.h"
#include "t4d_jpeg_fdct.h"

namespace {

constexpr int kBlock = 256;
constexpr int kStuffPer = 16;                       // stream bytes per thread of k_enc_count / k_enc_scatter (four words)
constexpr int kStuffChunk = kBlock * kStuffPer;
constexpr int kMaxImages = 1 << 16;
constexpr int64_t kMaxGrid = (int64_t)1 << 22;      // workgroups of one launch
constexpr int kBlockBytes = kJpegEncBlockWords * 4; // stream bytes of one block, at most (before stuffing)

__constant__ T4DJpegHuffEnc c_huff = t4d_jpeg_make_huff();

struct Geom {
    int32_t mx, my;                                 // MCUs across and down
    int32_t yw, yh;                                 // the luma component's own block grid
    int64_t mcus, blocks;
    int64_t wgs;                                    // workgroups of k_enc_dct
    int64_t chunks;                                 // 256-block chunks (k_enc_size, k_enc_emit)
    int64_t words;                                  // words of the bit buffer
    int64_t schunks;                                // kStuffChunk-byte chunks of the stream, at most
};

__host__ __device__ inline int mcus_per_group(int ss) { return kBlock / (8 * (t4d_jpeg_hs(ss) * t4d_jpeg_vs(ss) + 2)); }

__host__ __device__ inline Geom make_geom(int32_t w, int32_t h, int32_t ss)
{
    const int hs = t4d_jpeg_hs(ss), vs = t4d_jpeg_vs(ss);
    Geom g;
    g.mx = (w + 8 * hs - 1) / (8 * hs);
    g.my = (h + 8 * vs - 1) / (8 * vs);
    g.yw = (w + 7) / 8;
    g.yh = (h + 7) / 8;
    g.mcus = (int64_t)g.mx * g.my;
    g.blocks = g.mcus * (hs * vs + 2);
    const int mpg = mcus_per_group(ss);
    g.wgs = (g.mcus + mpg - 1) / mpg;
    g.chunks = (g.blocks + kBlock - 1) / kBlock;
    g.words = g.blocks * kJpegEncBlockWords + 4;
    g.schunks = (g.words * 4 + kStuffChunk - 1) / kStuffChunk;
    return g;
}

__host__ __device__ inline int64_t max_bytes(const Geom &g)
{
    return kJpegEncHeaderBytes + 2 * g.blocks * kBlockBytes + 2;      // every stream byte stuffed: a bound, never reached
}

struct EncImage {
    const uint8_t *src;
    int64_t pitch;
    int32_t w, h;
    Geom g;
    int64_t blk0;                                   // first block
    int64_t word0;                                  // first word of the bit buffer
    int64_t out_offset;
};

struct EncTables {
    uint16_t q[2][64];
    uint8_t header[kJpegEncHeaderBytes + 1];
};

struct EncLayout {
    size_t plan, wg0, chunk0, schunk0, tables, img_bits, img_ff, coef, bits, chunk_sum, chunk_off, words, ff_cnt, ff_off, total;
    int64_t wgs, blocks, chunks, n_words, schunks;
};

// false: an image the encoder does not take, or a batch beyond one launch
bool enc_layout(const T4DJpegEncImage *images, int32_t n, int32_t ss, EncLayout &L)
{
    L.wgs = L.blocks = L.chunks = L.n_words = L.schunks = 0;
    for (int32_t i = 0; i < n; ++i) {
        const T4DJpegEncImage &im = images[i];
        if (im.width < 1 || im.height < 1 || im.width > 65535 || im.height > 65535) return false;
        const Geom g = make_geom(im.width, im.height, ss);
        L.wgs += g.wgs; L.blocks += g.blocks; L.chunks += g.chunks; L.n_words += g.words; L.schunks += g.schunks;
    }
    if (L.wgs > kMaxGrid || L.chunks > kMaxGrid || L.schunks > kMaxGrid) return false;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
    L.plan = take((size_t)n * sizeof(EncImage));
    L.wg0 = take((size_t)(n + 1) * 8);
    L.chunk0 = take((size_t)(n + 1) * 8);
    L.schunk0 = take((size_t)(n + 1) * 8);
    L.tables = take(sizeof(EncTables));
    L.img_bits = take((size_t)n * 8);
    L.img_ff = take((size_t)n * 8);
    L.coef = take((size_t)L.blocks * 128);
    L.bits = take((size_t)L.chunks * kBlock * 2);
    L.chunk_sum = take((size_t)L.chunks * 4);
    L.chunk_off = take((size_t)L.chunks * 8);
    L.words = take((size_t)L.n_words * 4);
    L.ff_cnt = take((size_t)L.schunks * 4);
    L.ff_off = take((size_t)L.schunks * 8);
    L.total = o;
    return true;
}

// the image whose range [first[i], first[i + 1]) holds `key` (first[0] = 0, first[n] > key)
__device__ __forceinline__ int find_image(const int64_t *first, int n, int64_t key)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= key) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void k_enc_plan(const T4DJpegEncImage *images, int n, int ss, EncTables tables, EncImage *plan, int64_t *wg0,
                           int64_t *chunk0, int64_t *schunk0, EncTables *d_tables)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t wg = 0, chunk = 0, schunk = 0, blk = 0, word = 0;
    for (int i = 0; i < n; ++i) {
        EncImage e;
        e.src = images[i].src;
        e.pitch = images[i].src_pitch;
        e.w = images[i].width;
        e.h = images[i].height;
        e.g = make_geom(e.w, e.h, ss);
        e.blk0 = blk;
        e.word0 = word;
        e.out_offset = images[i].out_offset;
        plan[i] = e;
        wg0[i] = wg; chunk0[i] = chunk; schunk0[i] = schunk;
        wg += e.g.wgs; chunk += e.g.chunks; schunk += e.g.schunks; blk += e.g.blocks; word += e.g.words;
    }
    wg0[n] = wg; chunk0[n] = chunk; schunk0[n] = schunk;
    *d_tables = tables;
}

// ---------------------------------------------------------------------------------------------------------------------------
// samples -> quantised coefficients
// ---------------------------------------------------------------------------------------------------------------------------
template <int SS>
__global__ __launch_bounds__(kBlock) void k_enc_dct(const EncImage *plan, const int64_t *wg0, int n, const EncTables *tables,
                                                    int16_t *coef)
{
    constexpr int HS = SS == 0 ? 1 : 2, VS = SS == 2 ? 2 : 1, NL = HS * VS, BPM = NL + 2, LPM = 8 * BPM, MPG = kBlock / LPM;
    __shared__ int s_row[MPG * BPM][8][8];
    __shared__ __attribute__((aligned(16))) int16_t s_out[MPG * BPM][64];
    __shared__ uint16_t s_q[2][64];
    const int t = threadIdx.x;
    if (t < 128) s_q[t >> 6][t & 63] = tables->q[t >> 6][t & 63];
    const int i = find_image(wg0, n, blockIdx.x);
    const EncImage &im = plan[i];
    const int ml = t / LPM, lane = t % LPM, k = lane / 8, r = lane % 8;
    const int64_t m = ((int64_t)blockIdx.x - wg0[i]) * MPG + ml;
    const bool active = t < MPG * LPM && m < im.g.mcus;
    const int blk = ml * BPM + k;
    const int comp = k < NL ? 0 : k - NL + 1;
    const int mcx = active ? (int)(m % im.g.mx) : 0, mcy = active ? (int)(m / im.g.mx) : 0;
    const int bx = comp == 0 ? mcx * HS + k % HS : mcx, by = comp == 0 ? mcy * VS + k / HS : mcy;
    const bool dummy = comp == 0 && (bx >= im.g.yw || by >= im.g.yh);
    const bool work = active && !dummy;
    if (work) {
        int d[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) d[c] = t4d_jpeg_sample(im.src, im.pitch, im.w, im.h, SS, comp, bx * 8 + c, by * 8 + r) - 128;
        t4d_fdct_pass<true>(d);
#pragma unroll
        for (int c = 0; c < 8; ++c) s_row[blk][r][c] = d[c];
    }
    __syncthreads();
    if (work) {
        int d[8];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) d[rr] = s_row[blk][rr][r];             // this lane's column is its row number
        t4d_fdct_pass<false>(d);
        const int tab = comp ? 1 : 0;
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const int nat = rr * 8 + r;
            s_out[blk][c_huff.zz_of[nat]] = (int16_t)t4d_jpeg_quantize(d[rr], s_q[tab][nat]);
        }
    }
    __syncthreads();
    if (!active) return;
    int4 v = make_int4(0, 0, 0, 0);
    if (!dummy) {
        v = *(const int4 *)&s_out[blk][r * 8];
    } else if (r == 0) {
        // the last real block before this one in the MCU (block 0 is always real)
        int j = k - 1;
        while (j > 0 && (mcx * HS + j % HS >= im.g.yw || mcy * VS + j / HS >= im.g.yh)) --j;
        v.x = (int)(uint16_t)s_out[ml * BPM + j][0];
    }
    *(int4 *)(coef + ((im.blk0 + m * BPM + k) * 64 + r * 8)) = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// entropy coding
// ---------------------------------------------------------------------------------------------------------------------------
struct HuffShared {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

__device__ __forceinline__ void load_huff(HuffShared &S)
{
    const int t = threadIdx.x;
    S.ac[0][t] = c_huff.ac[0][t];
    S.ac[1][t] = c_huff.ac[1][t];
    if (t < 32) S.dc[t >> 4][t & 15] = c_huff.dc[t >> 4][t & 15];
    __syncthreads();
}

// index of the block whose DC predicts block (m, k)'s, relative to it; 0: none (the component's first block of the image)
template <int SS>
__device__ __forceinline__ int dc_pred_back(int64_t m, int k)
{
    constexpr int NL = (SS == 0 ? 1 : 2) * (SS == 2 ? 2 : 1), BPM = NL + 2;
    if (k < NL && k > 0) return 1;
    if (m == 0) return 0;
    return k < NL ? BPM - (NL - 1) : BPM;
}

__device__ __forceinline__ uint32_t value_bits(int v, int n) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }
__device__ __forceinline__ int category(int v) { return 32 - __clz(v < 0 ? -v : v); }

// put(code, length) for every code of a block in stream order (a Huffman code and its value bits as one put of <= 27 bits).
// c: the block's coefficients in zig-zag order; pred: the DC it is predicted from.
template <typename Put>
__device__ __forceinline__ void walk_block(const int16_t *c, int pred, const uint32_t *dc, const uint32_t *ac, Put put)
{
    const int4 *p = (const int4 *)c;
    int run = 0;
    for (int j = 0; j < 8; ++j) {
        const int4 q = p[j];
        const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int v = (int)(int16_t)(e & 1 ? (uint32_t)w[e >> 1] >> 16 : (uint32_t)w[e >> 1] & 0xFFFFu);
            if (j == 0 && e == 0) {
                const int diff = v - pred, nb = category(diff);
                const uint32_t h = dc[nb];
                put(((h & 0xFFFFu) << nb) | value_bits(diff, nb), (int)(h >> 16) + nb);
                continue;
            }
            if (v == 0) { ++run; continue; }
            while (run > 15) {
                const uint32_t z = ac[0xF0];
                put(z & 0xFFFFu, (int)(z >> 16));
                run -= 16;
            }
            const int nb = category(v);
            const uint32_t h = ac[(run << 4) | nb];
            put(((h & 0xFFFFu) << nb) | value_bits(v, nb), (int)(h >> 16) + nb);
            run = 0;
        }
    }
    if (run) put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}

template <int SS>
__global__ __launch_bounds__(kBlock) void k_enc_size(const EncImage *plan, const int64_t *chunk0, int n, const int16_t *coef,
                                                     uint16_t *bits, int32_t *chunk_sum)
{
    constexpr int BPM = (SS == 0 ? 1 : 2) * (SS == 2 ? 2 : 1) + 2;
    __shared__ HuffShared S;
    __shared__ int tmp[kBlock];
    load_huff(S);
    const int i = find_image(chunk0, n, blockIdx.x);
    const EncImage &im = plan[i];
    const int64_t b = ((int64_t)blockIdx.x - chunk0[i]) * kBlock + threadIdx.x;
    int nbits = 0;
    if (b < im.g.blocks) {
        const int64_t m = b / BPM;
        const int k = (int)(b - m * BPM);
        const int16_t *c = coef + (im.blk0 + b) * 64;
        const int back = dc_pred_back<SS>(m, k);
        const int pred = back ? c[-64 * back] : 0;
        const int tab = k < BPM - 2 ? 0 : 1;
        walk_block(c, pred, S.dc[tab], S.ac[tab], [&](uint32_t, int len) { nbits += len; });
    }
    bits[(int64_t)blockIdx.x * kBlock + threadIdx.x] = (uint16_t)nbits;
    const int all = block_sum<kBlock>(nbits, tmp);
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = all;
}

// One workgroup per image: off[c] = the sum of sums[first .. c) over the image's chunks, total[image] = the sum of all of them.
// STREAM: the chunks are those of the stuffing kernels and only the ones the image's stream reaches count.
template <bool STREAM>
__global__ __launch_bounds__(kBlock) void k_enc_scan(const int64_t *first, const int64_t *img_bits, const int32_t *sums, int64_t *off,
                                                     int64_t *total)
{
    __shared__ int64_t tmp[kBlock];
    const int i = blockIdx.x, t = threadIdx.x;
    const int64_t c0 = first[i];
    int64_t cnt = first[i + 1] - c0;
    if (STREAM) cnt = ((img_bits[i] + 7) / 8 + kStuffChunk - 1) / kStuffChunk;
    const int64_t per = (cnt + kBlock - 1) / kBlock;
    const int64_t k0 = min((int64_t)t * per, cnt), k1 = min(k0 + per, cnt);
    int64_t sum = 0;
    for (int64_t k = k0; k < k1; ++k) sum += sums[c0 + k];
    int64_t all = 0;
    int64_t o = block_exclusive_scan<kBlock>(sum, tmp, &all);
    for (int64_t k = k0; k < k1; ++k) {
        off[c0 + k] = o;
        o += sums[c0 + k];
    }
    if (t == 0) total[i] = all;
}

__global__ __launch_bounds__(kBlock) void k_enc_zero(const EncImage *plan, const int64_t *img_bits, uint32_t *words)
{
    const EncImage &im = plan[blockIdx.y];
    const int64_t cnt = min(img_bits[blockIdx.y] / 32 + 2, im.g.words);
    uint32_t *w = words + im.word0;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < cnt; k += (int64_t)gridDim.x * kBlock) w[k] = 0u;
}

template <int SS>
__global__ __launch_bounds__(kBlock) void k_enc_emit(const EncImage *plan, const int64_t *chunk0, int n, const int16_t *coef,
                                                     const uint16_t *bits, const int64_t *chunk_off, uint32_t *words)
{
    constexpr int BPM = (SS == 0 ? 1 : 2) * (SS == 2 ? 2 : 1) + 2;
    __shared__ HuffShared S;
    __shared__ int tmp[kBlock];
    load_huff(S);
    const int i = find_image(chunk0, n, blockIdx.x);
    const EncImage &im = plan[i];
    const int64_t b = ((int64_t)blockIdx.x - chunk0[i]) * kBlock + threadIdx.x;
    const int mine = bits[(int64_t)blockIdx.x * kBlock + threadIdx.x];
    const int64_t at = chunk_off[blockIdx.x] + block_exclusive_scan<kBlock, int>(mine, tmp, nullptr);
    if (b >= im.g.blocks) return;
    const int64_t m = b / BPM;
    const int k = (int)(b - m * BPM);
    const int16_t *c = coef + (im.blk0 + b) * 64;
    const int back = dc_pred_back<SS>(m, k);
    const int pred = back ? c[-64 * back] : 0;
    const int tab = k < BPM - 2 ? 0 : 1;
    uint32_t *w = words + im.word0 + (at >> 5);
    uint64_t acc = 0;                                  // the low `cnt` bits are pending; the first at & 31 of them are not ours (zero)
    int cnt = (int)(at & 31);
    bool first = true;
    walk_block(c, pred, S.dc[tab], S.ac[tab], [&](uint32_t code, int len) {
        acc = (acc << len) | code;
        cnt += len;
        if (cnt >= 32) {
            cnt -= 32;
            const uint32_t word = (uint32_t)(acc >> cnt);
            if (first) atomicOr(w, word); else *w = word;
            first = false;
            ++w;
        }
    });
    if (cnt > 0) atomicOr(w, (uint32_t)(acc << (32 - cnt)));
}

// ---------------------------------------------------------------------------------------------------------------------------
// byte stuffing and the file around the stream
// ---------------------------------------------------------------------------------------------------------------------------
// Stream bytes [j0, j0 + 16) of an image as this thread sees them: n of them exist (0..16); the stream's last byte has its unused
// low bits set.  Bytes are big-endian in the words.
__device__ __forceinline__ int stream_bytes16(const uint32_t *w, int64_t j0, int64_t nbits, uint8_t out[kStuffPer])
{
    const int64_t total = (nbits + 7) / 8;
    const int n = (int)max((int64_t)0, min((int64_t)kStuffPer, total - j0));
    if (n == 0) return 0;
    const uint4 q = *(const uint4 *)(w + (j0 >> 2));
    const uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < kStuffPer; ++e) out[e] = (uint8_t)(v[e >> 2] >> (24 - 8 * (e & 3)));
    const int pad = (int)(total * 8 - nbits);
    if (pad && j0 + n == total) {
#pragma unroll
        for (int e = 0; e < kStuffPer; ++e)
            if (e == n - 1) out[e] |= (uint8_t)((1u << pad) - 1u);
    }
    return n;
}

__global__ __launch_bounds__(kBlock) void k_enc_count(const EncImage *plan, const int64_t *schunk0, int n, const int64_t *img_bits,
                                                      const uint32_t *words, int32_t *ff_cnt)
{
    __shared__ int tmp[kBlock];
    const int i = find_image(schunk0, n, blockIdx.x);
    const int64_t cl = (int64_t)blockIdx.x - schunk0[i];
    const int64_t nbits = img_bits[i];
    if (cl * kStuffChunk >= (nbits + 7) / 8) return;
    uint8_t by[kStuffPer];
    const int cnt = stream_bytes16(words + plan[i].word0, cl * kStuffChunk + threadIdx.x * kStuffPer, nbits, by);
    int ff = 0;
#pragma unroll
    for (int e = 0; e < kStuffPer; ++e) ff += (e < cnt && by[e] == 0xFF) ? 1 : 0;
    const int all = block_sum<kBlock>(ff, tmp);
    if (threadIdx.x == 0) ff_cnt[blockIdx.x] = all;
}

__global__ __launch_bounds__(kBlock) void k_enc_scatter(const EncImage *plan, const int64_t *schunk0, int n, int ss,
                                                        const int64_t *img_bits, const int64_t *img_ff, const uint32_t *words,
                                                        const int64_t *ff_off, const EncTables *tables, uint8_t *out,
                                                        int64_t *out_bytes)
{
    __shared__ int tmp[kBlock];
    const int t = threadIdx.x;
    const int i = find_image(schunk0, n, blockIdx.x);
    const EncImage &im = plan[i];
    const int64_t cl = (int64_t)blockIdx.x - schunk0[i];
    const int64_t nbits = img_bits[i], sbytes = (nbits + 7) / 8;
    if (cl * kStuffChunk >= sbytes) return;
    const int64_t length = kJpegEncHeaderBytes + sbytes + img_ff[i] + 2;
    if (length > max_bytes(im.g)) {                                       // cannot happen: max_bytes bounds every stream
        if (cl == 0 && t == 0) out_bytes[i] = -1;
        return;
    }
    uint8_t *file = out + im.out_offset;
    if (cl == 0) {
        for (int k = t; k < kJpegEncHeaderBytes; k += kBlock) {
            uint8_t b = tables->header[k];
            const int f = k - kJpegEncSofAt;
            if (f == 5) b = (uint8_t)(im.h >> 8);
            if (f == 6) b = (uint8_t)im.h;
            if (f == 7) b = (uint8_t)(im.w >> 8);
            if (f == 8) b = (uint8_t)im.w;
            file[k] = b;
        }
        if (t == 0) {
            file[length - 2] = 0xFF;
            file[length - 1] = 0xD9;
            out_bytes[i] = length;
        }
    }
    uint8_t by[kStuffPer];
    const int64_t j0 = cl * kStuffChunk + t * kStuffPer;
    const int cnt = stream_bytes16(words + im.word0, j0, nbits, by);
    int ff = 0;
#pragma unroll
    for (int e = 0; e < kStuffPer; ++e) ff += (e < cnt && by[e] == 0xFF) ? 1 : 0;
    const int before = block_exclusive_scan<kBlock, int>(ff, tmp, nullptr);
    uint8_t *p = file + kJpegEncHeaderBytes + j0 + ff_off[blockIdx.x] + before;
#pragma unroll
    for (int e = 0; e < kStuffPer; ++e) {
        if (e < cnt) {
            *p++ = by[e];
            if (by[e] == 0xFF) *p++ = 0;
        }
    }
}

// float32 [C,H,W] -> uint8 [H,W,C]: clip(floor(float64(x) * 255 + 0.5), 0, 255); NaN gives 0
__global__ __launch_bounds__(kBlock) void k_views_to_u8(const float *src, int c, int64_t hw, uint8_t *dst)
{
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= hw) return;
    for (int ch = 0; ch < c; ++ch) {
        const double v = floor((double)src[ch * hw + p] * 255.0 + 0.5);
        dst[p * c + ch] = (uint8_t)(v >= 255.0 ? 255 : v > 0.0 ? (int)v : 0);
    }
}

template <int SS>
void launch_encode(const EncLayout &L, int32_t n, char *b, uint8_t *out, int64_t *out_bytes, hipStream_t stream)
{
    EncImage *plan = (EncImage *)(b + L.plan);
    int64_t *wg0 = (int64_t *)(b + L.wg0), *chunk0 = (int64_t *)(b + L.chunk0), *schunk0 = (int64_t *)(b + L.schunk0);
    EncTables *tables = (EncTables *)(b + L.tables);
    int64_t *img_bits = (int64_t *)(b + L.img_bits), *img_ff = (int64_t *)(b + L.img_ff);
    int16_t *coef = (int16_t *)(b + L.coef);
    uint16_t *bits = (uint16_t *)(b + L.bits);
    int32_t *chunk_sum = (int32_t *)(b + L.chunk_sum), *ff_cnt = (int32_t *)(b + L.ff_cnt);
    int64_t *chunk_off = (int64_t *)(b + L.chunk_off), *ff_off = (int64_t *)(b + L.ff_off);
    uint32_t *words = (uint32_t *)(b + L.words);
    hipLaunchKernelGGL(k_enc_dct<SS>, dim3((unsigned)L.wgs), dim3(kBlock), 0, stream, plan, wg0, n, tables, coef);
    hipLaunchKernelGGL(k_enc_size<SS>, dim3((unsigned)L.chunks), dim3(kBlock), 0, stream, plan, chunk0, n, coef, bits, chunk_sum);
    hipLaunchKernelGGL(k_enc_scan<false>, dim3((unsigned)n), dim3(kBlock), 0, stream, chunk0, img_bits, chunk_sum, chunk_off, img_bits);
    const unsigned zero_wgs = (unsigned)min((int64_t)1024, (L.n_words / n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_enc_zero, dim3(zero_wgs, (unsigned)n), dim3(kBlock), 0, stream, plan, img_bits, words);
    hipLaunchKernelGGL(k_enc_emit<SS>, dim3((unsigned)L.chunks), dim3(kBlock), 0, stream, plan, chunk0, n, coef, bits, chunk_off, words);
    hipLaunchKernelGGL(k_enc_count, dim3((unsigned)L.schunks), dim3(kBlock), 0, stream, plan, schunk0, n, img_bits, words, ff_cnt);
    hipLaunchKernelGGL(k_enc_scan<true>, dim3((unsigned)n), dim3(kBlock), 0, stream, schunk0, img_bits, ff_cnt, ff_off, img_ff);
    hipLaunchKernelGGL(k_enc_scatter, dim3((unsigned)L.schunks), dim3(kBlock), 0, stream, plan, schunk0, n, SS, img_bits, img_ff, words,
                       ff_off, tables, out, out_bytes);
}

bool ss_ok(int32_t ss) { return ss >= 0 && ss <= 2; }

}  // namespace

T4D_EXPORT size_t t4d_jpeg_enc_max_bytes(int32_t height, int32_t width, int32_t subsampling)
{
    if (height < 1 || width < 1 || height > 65535 || width > 65535 || !ss_ok(subsampling)) {
        t4d_fail(T4D_ERR_ARG, "t4d_jpeg_enc_max_bytes: need height, width in 1..65535 and subsampling in {0, 1, 2}");
        return 0;
    }
    return (size_t)max_bytes(make_geom(width, height, subsampling));
}

T4D_EXPORT size_t t4d_jpeg_enc_scratch_bytes(const T4DJpegEncImage *images, int32_t n, int32_t subsampling)
{
    EncLayout L;
    if (!images || n < 1 || n > kMaxImages || !ss_ok(subsampling) || !enc_layout(images, n, subsampling, L)) {
        t4d_fail(T4D_ERR_ARG, "t4d_jpeg_enc_scratch_bytes: need 1..65536 images of 1..65535 pixels a side, subsampling in {0, 1, 2} "
                              "and a batch within one launch (2^22 workgroups: split a larger one)");
        return 0;
    }
    return L.total;
}

T4D_EXPORT int t4d_jpeg_encode(const T4DJpegEncImage *images, const T4DJpegEncImage *d_images, int32_t n, int32_t quality,
                               int32_t subsampling, uint8_t *out, size_t out_capacity, int64_t *out_bytes, void *scratch,
                               size_t scratch_bytes, void *hip_stream)
{
    if (!images || !d_images || !out || !out_bytes || !scratch || n < 1 || n > kMaxImages)
        return t4d_fail(T4D_ERR_ARG, "t4d_jpeg_encode: bad arguments (NULL buffer, or n outside 1..65536)");
    if (quality < 1 || quality > 100 || !ss_ok(subsampling))
        return t4d_fail(T4D_ERR_ARG, "t4d_jpeg_encode: quality must be 1..100 and subsampling 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)");
    EncLayout L;
    if (!enc_layout(images, n, subsampling, L))
        return t4d_fail(T4D_ERR_ARG, "t4d_jpeg_encode: an image outside 1..65535 pixels a side, or a batch beyond one launch (split it)");
    for (int32_t i = 0; i < n; ++i) {
        const T4DJpegEncImage &im = images[i];
        if (!im.src || (int64_t)im.src_pitch < 3 * (int64_t)im.width)
            return t4d_fail(T4D_ERR_ARG, "t4d_jpeg_encode: image %d: NULL src or src_pitch below 3 * width", i);
        const int64_t need = max_bytes(make_geom(im.width, im.height, subsampling));
        if (im.out_offset < 0 || (uint64_t)im.out_offset + (uint64_t)need > (uint64_t)out_capacity)
            return t4d_fail(T4D_ERR_ARG, "t4d_jpeg_encode: image %d: out_offset + t4d_jpeg_enc_max_bytes exceeds out_capacity", i);
    }
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_jpeg_encode: scratch below t4d_jpeg_enc_scratch_bytes");
    hipStream_t stream = (hipStream_t)hip_stream;
    char *b = (char *)scratch;
    EncTables tables;
    t4d_jpeg_quant_tables(quality, tables.q[0], tables.q[1]);
    t4d_jpeg_header(tables.header, 0, 0, quality, subsampling);
    tables.header[kJpegEncHeaderBytes] = 0;
    hipLaunchKernelGGL(k_enc_plan, dim3(1), dim3(1), 0, stream, d_images, n, subsampling, tables, (EncImage *)(b + L.plan),
                       (int64_t *)(b + L.wg0), (int64_t *)(b + L.chunk0), (int64_t *)(b + L.schunk0), (EncTables *)(b + L.tables));
    if (subsampling == 0) launch_encode<0>(L, n, b, out, out_bytes, stream);
    else if (subsampling == 1) launch_encode<1>(L, n, b, out, out_bytes, stream);
    else launch_encode<2>(L, n, b, out, out_bytes, stream);
    return t4d_launch_status("t4d_jpeg_encode");
}

T4D_EXPORT int t4d_views_to_u8(const float *src, int32_t channels, int32_t height, int32_t width, uint8_t *dst, void *hip_stream)
{
    if (!src || !dst || channels < 1 || channels > 4 || height < 1 || width < 1)
        return t4d_fail(T4D_ERR_ARG, "t4d_views_to_u8: bad arguments (NULL buffer, channels outside 1..4, or an empty image)");
    const int64_t hw = (int64_t)height * width;
    if (hw > ((int64_t)1 << 31)) return t4d_fail(T4D_ERR_ARG, "t4d_views_to_u8: image too large");
    hipLaunchKernelGGL(k_views_to_u8, dim3((unsigned)((hw + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)hip_stream, src,
                       (int)channels, hw, dst);
    return t4d_launch_status("t4d_views_to_u8");
}
