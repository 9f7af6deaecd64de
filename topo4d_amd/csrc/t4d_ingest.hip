// t4d_ingest.hip — a frame's views from file bytes to float32 targets: baseline JPEG decoding that reproduces libjpeg-turbo's
// output (the block/pixel maths is csrc/t4d_jpeg.h) and skimage.transform.rotate(..., resize=True)'s order-1 warp, bit for bit.
//
// JPEG, for a batch of images packed back to back in one device buffer (each image's entropy-coded segment, stuffed, RSTn
// included; include/topo4d_raster.h T4DJpegImage):
//   k_jpeg_plan          one thread: per-image geometry and the offsets of its arrays in scratch
//   k_jpeg_huff          the derived Huffman tables, one thread per (image, table)
//   k_stuff_count/scan/write   remove FF00 stuffing and RSTn markers (parallel scan + compaction) and record where each
//                        restart interval starts
//   k_jpeg_sync (rounds) chunked self-synchronising decode of images without restart intervals: every lane decodes its chunk
//                        from the exit state of the lane before it, until no start state changes (at most t4d_jpeg::kRounds launches;
//                        k_jpeg_sync_fallback decodes the chunks of an image that did not converge one after another)
//   k_jpeg_lane_scan     per image: exclusive prefix of the lanes' block counts and DC-difference sums
//   k_jpeg_decode        every lane (a chunk, or a restart interval) decodes again from its synchronised state and writes its
//                        coefficients, DC predicted (prefix of the differences, reset at every restart interval)
//   k_jpeg_idct          ISLOW IDCT per block into the component planes
//   k_jpeg_color         fancy upsampling + YCbCr->RGB per pixel, uint8 HWC
//
// Warp: k_warp_in_range (input min/max), k_warp_out_range (warped min/max, only for views whose cval lies outside the input's
// range: _clip_warp_output), k_warp (order-1 warp in float64 through an LDS-staged source tile, clip, round to float32).
#include <hip/hip_runtime.h>

#include "t4d_block.h"
#include "t4d_host.h"
#include "t4d_jpeg.h"

using t4d_jpeg::Geom;
using t4d_jpeg::Huff;
using t4d_jpeg::LaneCounts;
using t4d_jpeg::State;
using namespace t4d_jpeg;  // the status bits

namespace {

constexpr int kBlock = 256;
constexpr int kTileBytes = kBlock * 16;  // bytes per stuffing tile (16 per thread)
constexpr int kMinChunkBits = 64;
constexpr int kDefaultChunkBits = 4096;

struct ImgPlan {
    Geom g;
    int64_t data_offset, data_bytes;     // raw segment; the compacted one is written at the same offset
    int64_t tile_base, lane_base, seg_base, blk_base, px_base;
    int64_t plane_off[3];
    int64_t out_offset;
    int32_t n_tiles, n_lanes, restart, width, height;
};

struct Layout {
    size_t plans, huff, tiles, clen, nrst, compact, rst, S, E0, E1, counts, prefix, changed, coef, planes, total;
    int64_t n_tiles, n_lanes, n_segs, n_blocks, n_px, data_bytes, plane_bytes;
};

// the plans (may be NULL) and the totals; false: an image the decoder does not take
__host__ __device__ inline bool make_plans(const T4DJpegImage *im, int n, int chunk_bits, ImgPlan *plans, Layout *L)
{
    int64_t tiles = 0, lanes = 0, segs = 0, blocks = 0, px = 0, data = 0, planes = 0;
    for (int i = 0; i < n; i++) {
        const T4DJpegImage &m = im[i];
        if (m.width < 1 || m.height < 1 || m.width > 65535 || m.height > 65535 || m.restart_interval < 0 || m.data_bytes < 0 ||
            m.data_offset != data)
            return false;
        if (!((m.h_samp == 1 && m.v_samp == 1) || (m.h_samp == 2 && m.v_samp == 1) || (m.h_samp == 2 && m.v_samp == 2)))
            return false;
        for (int c = 0; c < 3; c++)
            if (m.comp_quant[c] > 3 || m.comp_dc[c] > 3 || m.comp_ac[c] > 3) return false;
        ImgPlan p;
        p.g = t4d_jpeg::geometry(m);
        p.data_offset = m.data_offset;
        p.data_bytes = m.data_bytes;
        p.n_tiles = (int32_t)div_up(m.data_bytes, kTileBytes);
        p.restart = m.restart_interval;
        p.n_lanes = m.restart_interval > 0 ? p.g.n_seg : (int32_t)(div_up(m.data_bytes * 8, chunk_bits) > 0 ? div_up(m.data_bytes * 8, chunk_bits) : 1);
        p.tile_base = tiles;
        p.lane_base = lanes;
        p.seg_base = segs;
        p.blk_base = blocks;
        p.px_base = px;
        for (int c = 0; c < 3; c++) {
            p.plane_off[c] = planes;
            planes += (int64_t)p.g.pitch[c] * p.g.rows[c];
        }
        p.out_offset = m.out_offset;
        p.width = m.width;
        p.height = m.height;
        tiles += p.n_tiles;
        lanes += p.n_lanes;
        segs += p.g.n_seg;
        blocks += p.g.n_blocks;
        px += (int64_t)m.width * m.height;
        data += m.data_bytes;
        if (plans) plans[i] = p;
    }
    L->n_tiles = tiles;
    L->n_lanes = lanes;
    L->n_segs = segs;
    L->n_blocks = blocks;
    L->n_px = px;
    L->data_bytes = data;
    L->plane_bytes = planes;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    L->plans = take(sizeof(ImgPlan) * n);
    L->huff = take(sizeof(Huff) * 8 * n);
    L->tiles = take(8 * (size_t)tiles);
    L->clen = take(8 * (size_t)n);
    L->nrst = take(8 * (size_t)n);
    L->compact = take((size_t)data + 8);
    L->rst = take(8 * (size_t)segs);
    L->S = take(sizeof(State) * (size_t)lanes);
    L->E0 = take(sizeof(State) * (size_t)lanes);
    L->E1 = take(sizeof(State) * (size_t)lanes);
    L->counts = take(16 * (size_t)lanes);
    L->prefix = take(16 * (size_t)lanes);
    L->changed = take(4 * (size_t)kRounds * n);
    L->coef = take(128 * (size_t)blocks);
    L->planes = take((size_t)planes);
    L->total = o;
    return true;
}

// the plan whose [base, base + count) holds global index x (plans sorted by base)
template <typename F>
__device__ inline int find_plan(const ImgPlan *P, int n, int64_t x, F base)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base(P[mid]) <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void k_jpeg_plan(const T4DJpegImage *im, int n, int chunk_bits, ImgPlan *plans)
{
    Layout L;
    make_plans(im, n, chunk_bits, plans, &L);
}

__global__ void k_jpeg_huff(const T4DJpegImage *im, int n, Huff *huff, int32_t *status)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * 8) return;
    const int i = t >> 3, s = t & 7;
    if (!t4d_jpeg::build_huff(im[i].huff_bits[s], im[i].huff_vals[s], &huff[t])) atomicOr(&status[i], kErrCode);
}

__device__ inline bool is_rst(uint8_t b) { return b >= 0xD0 && b <= 0xD7; }

// byte j of an image's raw segment d[0, nb): kept (1) or dropped (stuffing 00, or one of the two bytes of an RSTn marker);
// *rst: j is the FF of an RSTn marker
__device__ inline int keep_byte(const uint8_t *d, int64_t nb, int64_t j, int *rst)
{
    const uint8_t b = d[j];
    const bool prev_ff = j > 0 && d[j - 1] == 0xFF;
    *rst = b == 0xFF && j + 1 < nb && is_rst(d[j + 1]);
    if (*rst) return 0;
    if (prev_ff && (b == 0x00 || is_rst(b))) return 0;
    return 1;
}

constexpr uint64_t kRstOne = 1ull << 40;

__global__ void k_stuff_count(const ImgPlan *P, int n, const uint8_t *data, uint64_t *tiles)
{
    __shared__ uint64_t tmp[kBlock];
    const int64_t tile = blockIdx.x;
    const int i = find_plan(P, n, tile, [](const ImgPlan &p) { return p.tile_base; });
    const ImgPlan &p = P[i];
    const uint8_t *d = data + p.data_offset;
    const int64_t j0 = (tile - p.tile_base) * kTileBytes + threadIdx.x * 16;
    uint64_t v = 0;
    for (int64_t j = j0; j < j0 + 16 && j < p.data_bytes; j++) {
        int rst;
        v += keep_byte(d, p.data_bytes, j, &rst);
        v += rst ? kRstOne : 0;
    }
    uint64_t total;
    block_exclusive_scan<kBlock>(v, tmp, &total);
    if (threadIdx.x == 0) tiles[tile] = total;
}

__global__ void k_stuff_scan(const ImgPlan *P, uint64_t *tiles, int64_t *clen, int64_t *nrst, int32_t *status)
{
    __shared__ uint64_t tmp[kBlock];
    const ImgPlan &p = P[blockIdx.x];
    uint64_t carry = 0;
    for (int64_t b = 0; b < p.n_tiles; b += kBlock) {
        const int64_t t = b + threadIdx.x;
        const uint64_t v = t < p.n_tiles ? tiles[p.tile_base + t] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan<kBlock>(v, tmp, &total);
        if (t < p.n_tiles) tiles[p.tile_base + t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        clen[blockIdx.x] = (int64_t)(carry & (kRstOne - 1));
        nrst[blockIdx.x] = (int64_t)(carry >> 40);
        if (nrst[blockIdx.x] != p.g.n_seg - 1) atomicOr(&status[blockIdx.x], kErrRestart);
    }
}

__global__ void k_stuff_write(const ImgPlan *P, int n, const uint8_t *data, const uint64_t *tiles, uint8_t *compact,
                              int64_t *rst_pos, int32_t *status)
{
    __shared__ uint64_t tmp[kBlock];
    const int64_t tile = blockIdx.x;
    const int i = find_plan(P, n, tile, [](const ImgPlan &p) { return p.tile_base; });
    const ImgPlan &p = P[i];
    const uint8_t *d = data + p.data_offset;
    uint8_t *out = compact + p.data_offset;
    const int64_t j0 = (tile - p.tile_base) * kTileBytes + threadIdx.x * 16;
    uint64_t v = 0;
    for (int64_t j = j0; j < j0 + 16 && j < p.data_bytes; j++) {
        int rst;
        v += keep_byte(d, p.data_bytes, j, &rst);
        v += rst ? kRstOne : 0;
    }
    uint64_t total;
    uint64_t at = tiles[tile] + block_exclusive_scan<kBlock>(v, tmp, &total);
    for (int64_t j = j0; j < j0 + 16 && j < p.data_bytes; j++) {
        int rst;
        const int k = keep_byte(d, p.data_bytes, j, &rst);
        const int64_t pos = (int64_t)(at & (kRstOne - 1)), r = (int64_t)(at >> 40);
        if (k) out[pos] = d[j];
        if (rst) {
            if (r < p.g.n_seg - 1) rst_pos[p.seg_base + r] = pos;
            if (d[j + 1] - 0xD0 != (int)(r & 7)) atomicOr(&status[i], kErrRestart);
        }
        at += k + (rst ? kRstOne : 0);
    }
}

struct LaneGeom {
    int64_t start, end;          // the chunk's bits
    int64_t seg_bits;
    bool live;
};

__device__ inline LaneGeom lane_geom(const ImgPlan &p, int64_t clen, int64_t t, int chunk_bits)
{
    LaneGeom l;
    l.seg_bits = clen * 8;
    l.start = t * chunk_bits;
    l.end = l.start + chunk_bits < l.seg_bits ? l.start + chunk_bits : l.seg_bits;
    const int64_t last = l.seg_bits > 0 ? (l.seg_bits - 1) / chunk_bits : 0;
    l.live = t <= last;
    return l;
}

__global__ void k_jpeg_sync(const ImgPlan *P, int n, const T4DJpegImage *im, const Huff *huff, const uint8_t *compact,
                            const int64_t *clen, int chunk_bits, int round, State *S, const State *Ein, State *Eout,
                            LaneCounts *counts, int32_t *changed, int64_t n_lanes)
{
    const int64_t gl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gl >= n_lanes) return;
    const int i = find_plan(P, n, gl, [](const ImgPlan &p) { return p.lane_base; });
    const ImgPlan &p = P[i];
    if (p.restart > 0) return;
    if (round > 0 && changed[(round - 1) * n + i] == 0) return;
    const int64_t t = gl - p.lane_base;
    const LaneGeom l = lane_geom(p, clen[i], t, chunk_bits);
    if (!l.live) {                       // past the compacted data (the lanes are counted on the stuffed bytes): no chunk
        if (round == 0) counts[gl] = LaneCounts{0, {0, 0, 0}};
        return;
    }
    const uint8_t *d = compact + p.data_offset;
    State s;
    if (round == 0) {
        s = State{l.start, 0, 0};
        S[gl] = s;
        if (p.n_lanes > 1 && t == 0) changed[i] = 1;
    } else {
        if (t == 0) {
            Eout[gl] = Ein[gl];
            return;
        }
        s = Ein[gl - 1];
        if (t4d_jpeg::same(s, S[gl])) {
            Eout[gl] = Ein[gl];
            return;
        }
        S[gl] = s;
        changed[round * n + i] = 1;
    }
    LaneCounts c;
    run_counts(d, clen[i], tables(im[i], huff + 8 * i), p.g, s, l.end, c);
    Eout[gl] = s;
    counts[gl] = c;
}

// an image whose lanes did not reach a fixed point within kRounds: its chunks' start states one after another
__global__ void k_jpeg_sync_fallback(const ImgPlan *P, int n, const T4DJpegImage *im, const Huff *huff, const uint8_t *compact,
                                     const int64_t *clen, int chunk_bits, State *S, LaneCounts *counts, const int32_t *changed)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ImgPlan &p = P[i];
    if (p.restart > 0 || changed[(kRounds - 1) * n + i] == 0) return;
    State s{0, 0, 0};
    for (int64_t t = 0; t < p.n_lanes; t++) {
        const LaneGeom l = lane_geom(p, clen[i], t, chunk_bits);
        S[p.lane_base + t] = s;
        LaneCounts c;
        run_counts(compact + p.data_offset, clen[i], tables(im[i], huff + 8 * i), p.g, s, l.end, c);
        counts[p.lane_base + t] = c;
    }
}

// exclusive prefix of the lanes' counts: the global index of a lane's first DC symbol and its DC predictors at entry
__global__ void k_jpeg_lane_scan(const ImgPlan *P, const LaneCounts *counts, LaneCounts *prefix)
{
    __shared__ uint32_t tmp[kBlock];
    const ImgPlan &p = P[blockIdx.x];
    if (p.restart > 0) return;
    uint32_t carry[4] = {0, 0, 0, 0};                               // 32-bit two's-complement sums
    for (int64_t b = 0; b < p.n_lanes; b += kBlock) {
        const int64_t t = b + threadIdx.x;
        LaneCounts c = t < p.n_lanes ? counts[p.lane_base + t] : LaneCounts{0, {0, 0, 0}};
        const int32_t v[4] = {c.blocks, c.dc[0], c.dc[1], c.dc[2]};
        int32_t ex[4];
        for (int q = 0; q < 4; q++) {
            uint32_t total;
            ex[q] = (int32_t)(carry[q] + block_exclusive_scan<kBlock>((uint32_t)v[q], tmp, &total));
            carry[q] += total;
        }
        if (t < p.n_lanes) prefix[p.lane_base + t] = LaneCounts{ex[0], {ex[1], ex[2], ex[3]}};
    }
}

__global__ void k_jpeg_decode(const ImgPlan *P, int n, const T4DJpegImage *im, const Huff *huff, const uint8_t *compact,
                              const int64_t *clen, const int64_t *rst_pos, int chunk_bits, const State *S, const LaneCounts *prefix,
                              int16_t *coef, int32_t *status, int64_t n_lanes)
{
    const int64_t gl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gl >= n_lanes) return;
    const int i = find_plan(P, n, gl, [](const ImgPlan &p) { return p.lane_base; });
    const ImgPlan &p = P[i];
    const Geom &g = p.g;
    const int64_t t = gl - p.lane_base;
    const Huff *hf = huff + 8 * i;
    const T4DJpegImage &m = im[i];
    const uint8_t *d;
    int64_t nb, end, blk, blk_limit;
    int32_t pred[3] = {0, 0, 0};
    bool last;
    State s;
    if (p.restart > 0) {
        if (status[i] & kErrRestart) return;
        const int64_t a = t == 0 ? 0 : rst_pos[p.seg_base + t - 1];
        const int64_t b = t + 1 < g.n_seg ? rst_pos[p.seg_base + t] : clen[i];
        if (a < 0 || b < a || b > clen[i]) {
            atomicOr(&status[i], kErrRestart);
            return;
        }
        d = compact + p.data_offset + a;
        nb = b - a;
        end = nb * 8;
        s = State{0, 0, 0};
        blk = t * p.restart * g.bpm - 1;
        const int64_t lim = (t + 1) * p.restart < g.n_mcu ? (t + 1) * p.restart : g.n_mcu;
        blk_limit = lim * g.bpm;
        last = true;
    } else {
        const LaneGeom l = lane_geom(p, clen[i], t, chunk_bits);
        if (!l.live) return;
        d = compact + p.data_offset;
        nb = clen[i];
        end = l.end;
        s = S[gl];
        const LaneCounts pre = prefix[gl];
        blk = (int64_t)pre.blocks - 1;
        for (int c = 0; c < 3; c++) pred[c] = pre.dc[c];
        blk_limit = g.n_blocks;
        last = l.end >= l.seg_bits;
    }
    const int err = decode_lane(d, nb, tables(m, hf), g, s, end, last, blk, blk_limit, pred, coef + p.blk_base * 64);
    if (err) atomicOr(&status[i], err);
}

__global__ void k_jpeg_idct(const ImgPlan *P, int n, const T4DJpegImage *im, const int16_t *coef, uint8_t *planes, int64_t n_blocks)
{
    const int64_t gb = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gb >= n_blocks) return;
    const int i = find_plan(P, n, gb, [](const ImgPlan &p) { return p.blk_base; });
    const ImgPlan &p = P[i];
    const int64_t blk = gb - p.blk_base;
    int c;
    int64_t x, y;
    t4d_jpeg::block_origin(p.g, blk, &c, &x, &y);
    alignas(16) int16_t cf[64];
    const int4 *src = (const int4 *)(coef + gb * 64);
    for (int q = 0; q < 8; q++) ((int4 *)cf)[q] = src[q];
    t4d_jpeg::idct_islow(cf, im[i].quant[im[i].comp_quant[c]], planes + p.plane_off[c] + y * p.g.pitch[c] + x, p.g.pitch[c]);
}

__global__ void k_jpeg_color(const ImgPlan *P, int n, const uint8_t *planes, const int32_t *status, uint8_t *out, int64_t n_px)
{
    const int64_t gp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gp >= n_px) return;
    const int i = find_plan(P, n, gp, [](const ImgPlan &p) { return p.px_base; });
    const ImgPlan &p = P[i];
    const Geom &g = p.g;
    const int64_t q = gp - p.px_base;
    const int y = (int)(q / p.width), x = (int)(q - (int64_t)y * p.width);
    const int Y = planes[p.plane_off[0] + (int64_t)y * g.pitch[0] + x];
    const int cb = t4d_jpeg::upsample(planes + p.plane_off[1], g.pitch[1], g.cw[1], g.ch[1], g.hs, g.vs, x, y);
    const int cr = t4d_jpeg::upsample(planes + p.plane_off[2], g.pitch[2], g.cw[2], g.ch[2], g.hs, g.vs, x, y);
    uint8_t rgb[3];
    t4d_jpeg::ycc_to_rgb(Y, cb, cr, rgb);
    uint8_t *o = out + p.out_offset + q * 3;
    o[0] = rgb[0];
    o[1] = rgb[1];
    o[2] = rgb[2];
}

// ---- warp ------------------------------------------------------------------------------------------------------------------
constexpr int kWarpTile = 32;                 // output tile side; 256 threads, 4 rows each
constexpr int kWarpLds = 16384;               // staged source bytes per tile
constexpr int kRangeBytes = kBlock * 16;      // source bytes per block of k_warp_in_range

struct WarpRange {
    uint32_t in_min, in_max;
    unsigned long long out_min, out_max;       // order-preserving encodings of the warped values' min / max
};

__host__ __device__ inline int64_t warp_tiles(const T4DWarpView &v)
{
    return div_up(v.out_rows, kWarpTile) * div_up(v.out_cols, kWarpTile);
}

__host__ __device__ inline int64_t range_blocks(const T4DWarpView &v)
{
    return div_up((int64_t)v.rows * v.cols * v.channels, kRangeBytes);
}

__device__ inline unsigned long long order_key(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : u | (1ull << 63);
}

__device__ inline double order_val(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? k & ~(1ull << 63) : ~k));
}

__global__ void k_warp_init(WarpRange *R, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) R[i] = WarpRange{255u, 0u, ~0ull, 0ull};
}

__global__ void k_warp_in_range(const T4DWarpView *V, int n, WarpRange *R)
{
    int64_t lb;
    const int vi = find_view(V, n, blockIdx.x, &lb, [](const T4DWarpView &w) { return range_blocks(w); });
    if (vi < 0) return;
    const T4DWarpView &v = V[vi];
    const int64_t row_bytes = (int64_t)v.cols * v.channels, total = row_bytes * v.rows;
    uint32_t mn = 255, mx = 0;
    for (int64_t e = lb * kRangeBytes + threadIdx.x; e < (lb + 1) * kRangeBytes && e < total; e += kBlock) {
        const int64_t r = e / row_bytes;
        const uint32_t b = v.src[r * v.src_pitch + (e - r * row_bytes)];
        mn = b < mn ? b : mn;
        mx = b > mx ? b : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&R[vi].in_min, mn);
        atomicMax(&R[vi].in_max, mx);
    }
}

#pragma clang fp contract(off)      // skimage's Cython: every product and every sum rounded
// skimage's get_pixel2d (mode constant) of a u8 source as float64
__device__ inline double tap(const T4DWarpView &v, const uint8_t *lds, int64_t br, int64_t bc, int bh, int bw, int64_t r, int64_t c,
                             int ch)
{
    if (r < 0 || r >= v.rows || c < 0 || c >= v.cols) return v.cval;
    const int64_t lr = r - br, lc = c - bc;
    const uint8_t b = (lds && lr >= 0 && lr < bh && lc >= 0 && lc < bw) ? lds[(lr * bw + lc) * v.channels + ch]
                                                                          : v.src[r * v.src_pitch + c * v.channels + ch];
    return (double)b / 255.0;
}

// skimage _warp_fast: _transform_affine then bilinear_interpolation
__device__ inline double warp_sample(const T4DWarpView &v, const uint8_t *lds, int64_t br, int64_t bc, int bh, int bw, double r,
                                     double c, int ch)
{
    const double fr = floor(r), fc = floor(c), cr = ceil(r), cc = ceil(c);
    const int64_t minr = (int64_t)fr, minc = (int64_t)fc, maxr = (int64_t)cr, maxc = (int64_t)cc;
    const double dr = r - (double)minr, dc = c - (double)minc;
    const double tl = tap(v, lds, br, bc, bh, bw, minr, minc, ch), tr = tap(v, lds, br, bc, bh, bw, minr, maxc, ch);
    const double bl = tap(v, lds, br, bc, bh, bw, maxr, minc, ch), bt = tap(v, lds, br, bc, bh, bw, maxr, maxc, ch);
    const double top = (1 - dc) * tl + dc * tr;
    const double bottom = (1 - dc) * bl + dc * bt;
    return (1 - dr) * top + dr * bottom;
}

__device__ inline void source_rc(const T4DWarpView &v, int64_t ro, int64_t co, double *r, double *c)
{
    const double x = (double)co, y = (double)ro;
    *c = v.matrix[0] * x + v.matrix[1] * y + v.matrix[2];
    *r = v.matrix[3] * x + v.matrix[4] * y + v.matrix[5];
}

__device__ inline bool needs_out_range(const T4DWarpView &v, const WarpRange &R)
{
    const double lo = (double)R.in_min / 255.0, hi = (double)R.in_max / 255.0;
    return !(lo <= v.cval && v.cval <= hi);
}

__global__ void k_warp_out_range(const T4DWarpView *V, int n, WarpRange *R)
{
    int64_t lt;
    const int vi = find_view(V, n, blockIdx.x, &lt, [](const T4DWarpView &w) { return warp_tiles(w); });
    if (vi < 0) return;
    const T4DWarpView &v = V[vi];
    if (!needs_out_range(v, R[vi])) return;
    const int64_t tc = div_up(v.out_cols, kWarpTile);
    const int64_t r0 = lt / tc * kWarpTile, c0 = lt % tc * kWarpTile;
    const int64_t co = c0 + (threadIdx.x & 31);
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t ro = r0 + (threadIdx.x >> 5); ro < r0 + kWarpTile; ro += 8) {
        if (ro >= v.out_rows || co >= v.out_cols) continue;
        double r, c;
        source_rc(v, ro, co, &r, &c);
        for (int ch = 0; ch < v.channels; ch++) {
            const double x = warp_sample(v, nullptr, 0, 0, 0, 0, r, c, ch);
            mn = x < mn ? x : mn;
            mx = x > mx ? x : mx;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0 && mn <= mx) {
        atomicMin(&R[vi].out_min, order_key(mn));
        atomicMax(&R[vi].out_max, order_key(mx));
    }
}

__global__ void __launch_bounds__(kBlock) k_warp(const T4DWarpView *V, int n, const WarpRange *R)
{
    __shared__ uint8_t lds[kWarpLds];
    int64_t lt;
    const int vi = find_view(V, n, blockIdx.x, &lt, [](const T4DWarpView &w) { return warp_tiles(w); });
    if (vi < 0) return;
    const T4DWarpView &v = V[vi];
    // _clip_warp_output
    double lo = (double)R[vi].in_min / 255.0, hi = (double)R[vi].in_max / 255.0;
    if (needs_out_range(v, R[vi])) {
        const double omin = order_val(R[vi].out_min), omax = order_val(R[vi].out_max);
        if (omin <= v.cval && v.cval <= omax) {
            lo = lo < v.cval ? lo : v.cval;
            hi = hi > v.cval ? hi : v.cval;
        }
    }
    const int64_t tc = div_up(v.out_cols, kWarpTile);
    const int64_t r0 = lt / tc * kWarpTile, c0 = lt % tc * kWarpTile;
    const int64_t r1 = (r0 + kWarpTile < v.out_rows ? r0 + kWarpTile : v.out_rows) - 1;
    const int64_t c1 = (c0 + kWarpTile < v.out_cols ? c0 + kWarpTile : v.out_cols) - 1;
    // the source footprint of the tile (an affine map: its corners bound it), one sample of margin, clipped to the source
    double rmin = INFINITY, rmax = -INFINITY, cmin = INFINITY, cmax = -INFINITY;
    for (int q = 0; q < 4; q++) {
        double r, c;
        source_rc(v, q & 1 ? r1 : r0, q & 2 ? c1 : c0, &r, &c);
        rmin = fmin(rmin, r);
        rmax = fmax(rmax, r);
        cmin = fmin(cmin, c);
        cmax = fmax(cmax, c);
    }
    const bool finite = rmin > -1e9 && rmax < 1e9 && cmin > -1e9 && cmax < 1e9;
    int64_t br = finite ? (int64_t)floor(rmin) - 1 : 0, bc = finite ? (int64_t)floor(cmin) - 1 : 0;
    int64_t er = finite ? (int64_t)ceil(rmax) + 1 : -1, ec = finite ? (int64_t)ceil(cmax) + 1 : -1;
    br = br < 0 ? 0 : br;
    bc = bc < 0 ? 0 : bc;
    er = er > v.rows - 1 ? v.rows - 1 : er;
    ec = ec > v.cols - 1 ? v.cols - 1 : ec;
    const int64_t bh = er - br + 1, bw = ec - bc + 1;
    const bool staged = finite && bh > 0 && bw > 0 && bh * bw * v.channels <= kWarpLds;
    if (staged) {
        const int64_t row_bytes = bw * v.channels;
        for (int64_t e = threadIdx.x; e < bh * row_bytes; e += kBlock) {
            const int64_t lr = e / row_bytes;
            lds[e] = v.src[(br + lr) * v.src_pitch + bc * v.channels + (e - lr * row_bytes)];
        }
    }
    __syncthreads();
    const int64_t co = c0 + (threadIdx.x & 31);
    const int64_t plane = (int64_t)v.out_rows * v.out_cols;
    for (int64_t ro = r0 + (threadIdx.x >> 5); ro <= r1; ro += 8) {
        if (co > c1) break;
        double r, c;
        source_rc(v, ro, co, &r, &c);
        for (int ch = 0; ch < v.channels; ch++) {
            double x = staged ? warp_sample(v, lds, br, bc, (int)bh, (int)bw, r, c, ch) : warp_sample(v, nullptr, 0, 0, 0, 0, r, c, ch);
            x = x > lo ? x : lo;                 // np.clip: minimum(maximum(x, lo), hi)
            x = x < hi ? x : hi;
            v.dst[ch * plane + ro * v.out_cols + co] = (float)x;
        }
    }
}

}  // namespace

T4D_EXPORT size_t t4d_jpeg_scratch_bytes(const T4DJpegImage *images, int32_t n, int32_t chunk_bits)
{
    Layout L;
    if (!images || n < 1 || (chunk_bits != 0 && chunk_bits < kMinChunkBits) ||
        !make_plans(images, n, chunk_bits ? chunk_bits : kDefaultChunkBits, nullptr, &L)) {
        t4d_fail(T4D_ERR_ARG, "t4d_jpeg_scratch_bytes: bad image descriptors (packed data, size, sampling or table slots) or chunk_bits < %d", kMinChunkBits);
        return 0;
    }
    return L.total;
}

T4D_EXPORT int t4d_jpeg_decode(const T4DJpegImage *images, const T4DJpegImage *d_images, int32_t n, const uint8_t *data,
                               int32_t chunk_bits, uint8_t *out, size_t out_capacity, int32_t *status, void *scratch,
                               size_t scratch_bytes, void *hip_stream)
{
    if (!images || !d_images || n < 1 || !data || !out || !status || !scratch || (chunk_bits != 0 && chunk_bits < kMinChunkBits))
        return t4d_fail(T4D_ERR_ARG, "t4d_jpeg_decode: bad arguments");
    const int cb = chunk_bits ? chunk_bits : kDefaultChunkBits;
    Layout L;
    if (!make_plans(images, n, cb, nullptr, &L)) return t4d_fail(T4D_ERR_ARG, "t4d_jpeg_decode: bad image descriptors");
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_jpeg_decode: scratch too small");
    for (int i = 0; i < n; i++)
        if (images[i].out_offset < 0 || (size_t)images[i].out_offset + (size_t)images[i].width * images[i].height * 3 > out_capacity)
            return t4d_fail(T4D_ERR_ARG, "t4d_jpeg_decode: image %d does not fit the output buffer", i);
    hipStream_t stream = (hipStream_t)hip_stream;
    char *b = (char *)scratch;
    ImgPlan *plans = (ImgPlan *)(b + L.plans);
    Huff *huff = (Huff *)(b + L.huff);
    uint64_t *tiles = (uint64_t *)(b + L.tiles);
    int64_t *clen = (int64_t *)(b + L.clen), *nrst = (int64_t *)(b + L.nrst), *rst = (int64_t *)(b + L.rst);
    uint8_t *compact = (uint8_t *)(b + L.compact), *planes = (uint8_t *)(b + L.planes);
    State *S = (State *)(b + L.S), *E[2] = {(State *)(b + L.E0), (State *)(b + L.E1)};
    LaneCounts *counts = (LaneCounts *)(b + L.counts), *prefix = (LaneCounts *)(b + L.prefix);
    int32_t *changed = (int32_t *)(b + L.changed);
    int16_t *coef = (int16_t *)(b + L.coef);
    const unsigned lane_grid = (unsigned)div_up(L.n_lanes, kBlock);
    T4D_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t) * n, stream));
    T4D_HIP_CHECK(hipMemsetAsync(changed, 0, sizeof(int32_t) * kRounds * n, stream));
    T4D_HIP_CHECK(hipMemsetAsync(coef, 0, 128 * (size_t)L.n_blocks, stream));
    hipLaunchKernelGGL(k_jpeg_plan, dim3(1), dim3(1), 0, stream, d_images, n, cb, plans);
    hipLaunchKernelGGL(k_jpeg_huff, dim3((unsigned)div_up(8 * n, kBlock)), dim3(kBlock), 0, stream, d_images, n, huff, status);
    if (L.n_tiles > 0) {
        hipLaunchKernelGGL(k_stuff_count, dim3((unsigned)L.n_tiles), dim3(kBlock), 0, stream, plans, n, data, tiles);
        hipLaunchKernelGGL(k_stuff_scan, dim3((unsigned)n), dim3(kBlock), 0, stream, plans, tiles, clen, nrst, status);
        hipLaunchKernelGGL(k_stuff_write, dim3((unsigned)L.n_tiles), dim3(kBlock), 0, stream, plans, n, data, tiles, compact, rst,
                           status);
    } else {
        T4D_HIP_CHECK(hipMemsetAsync(clen, 0, 8 * (size_t)n, stream));
        hipLaunchKernelGGL(k_stuff_scan, dim3((unsigned)n), dim3(kBlock), 0, stream, plans, tiles, clen, nrst, status);
    }
    for (int r = 0; r < kRounds; r++)
        hipLaunchKernelGGL(k_jpeg_sync, dim3(lane_grid), dim3(kBlock), 0, stream, plans, n, d_images, huff, compact, clen, cb, r, S,
                           E[(r + 1) & 1], E[r & 1], counts, changed, L.n_lanes);
    hipLaunchKernelGGL(k_jpeg_sync_fallback, dim3((unsigned)div_up(n, 64)), dim3(64), 0, stream, plans, n, d_images, huff, compact,
                       clen, cb, S, counts, changed);
    hipLaunchKernelGGL(k_jpeg_lane_scan, dim3((unsigned)n), dim3(kBlock), 0, stream, plans, counts, prefix);
    hipLaunchKernelGGL(k_jpeg_decode, dim3(lane_grid), dim3(kBlock), 0, stream, plans, n, d_images, huff, compact, clen, rst, cb, S,
                       prefix, coef, status, L.n_lanes);
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)div_up(L.n_blocks, kBlock)), dim3(kBlock), 0, stream, plans, n, d_images, coef,
                       planes, L.n_blocks);
    hipLaunchKernelGGL(k_jpeg_color, dim3((unsigned)div_up(L.n_px, kBlock)), dim3(kBlock), 0, stream, plans, n, planes, status, out,
                       L.n_px);
    return t4d_launch_status("t4d_jpeg_decode");
}

T4D_EXPORT size_t t4d_warp_scratch_bytes(int32_t n_views)
{
    if (n_views < 1) {
        t4d_fail(T4D_ERR_ARG, "t4d_warp_scratch_bytes: n_views < 1");
        return 0;
    }
    return align_up(sizeof(WarpRange) * (size_t)n_views);
}

T4D_EXPORT int t4d_warp_views(const T4DWarpView *views, const T4DWarpView *d_views, int32_t n_views, void *scratch,
                              size_t scratch_bytes, void *hip_stream)
{
    if (!views || !d_views || n_views < 1 || !scratch) return t4d_fail(T4D_ERR_ARG, "t4d_warp_views: bad arguments");
    if (scratch_bytes < sizeof(WarpRange) * (size_t)n_views) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_warp_views: scratch too small");
    int64_t tiles = 0, blocks = 0;
    for (int i = 0; i < n_views; i++) {
        const T4DWarpView &v = views[i];
        if (!v.src || !v.dst || v.rows < 1 || v.cols < 1 || v.channels < 1 || v.channels > 4 || v.out_rows < 1 || v.out_cols < 1 ||
            v.src_pitch < v.cols * v.channels)
            return t4d_fail(T4D_ERR_ARG, "t4d_warp_views: bad view descriptor");
        tiles += warp_tiles(v);
        blocks += range_blocks(v);
    }
    if (tiles > 0x7fffffff || blocks > 0x7fffffff) return t4d_fail(T4D_ERR_ARG, "t4d_warp_views: too many tiles");
    hipStream_t stream = (hipStream_t)hip_stream;
    WarpRange *R = (WarpRange *)scratch;
    hipLaunchKernelGGL(k_warp_init, dim3((unsigned)div_up(n_views, 64)), dim3(64), 0, stream, R, n_views);
    hipLaunchKernelGGL(k_warp_in_range, dim3((unsigned)blocks), dim3(kBlock), 0, stream, d_views, n_views, R);
    hipLaunchKernelGGL(k_warp_out_range, dim3((unsigned)tiles), dim3(kBlock), 0, stream, d_views, n_views, R);
    hipLaunchKernelGGL(k_warp, dim3((unsigned)tiles), dim3(kBlock), 0, stream, d_views, n_views, R);
    return t4d_launch_status("t4d_warp_views");
}
