// t4d_texfill.hip — the push-pull hole fill of a UV texture on the device (topo4d_amd/texfinish.py: fill, fill_islands).  The rule
// is stated in include/topo4d_raster.h; everything is integer arithmetic, so the result is a pure function of the inputs and does
// not depend on the launch shape.  tests/texfill_ref.py restates the rule in whole-level numpy operations.
//
// The pyramid lives in the scratch: level k (1 .. top, the 1x1 level) is uint16 [h_k, w_k, c] with h_k = ceil(h / 2^k), colours in
// units of 1/256 (at most 255 * 256 = 0xFF00); a texel without a valid descendant holds kHole = 0xFFFF in channel 0.
//
//  * k_fill_pull       one 64x64 tile of level `base` per workgroup: its levels base+1 .. base+6 through LDS, each written once.
//                      base = 0 reads the image and the valid map (staged in LDS with vector loads), base = 6, 12 read the level
//                      the launch before wrote: at most three launches for the 16 levels of a 65536^2 image.
//  * k_fill_push_coarse  the mirror for base = 12, 6: per tile the regions of levels base+6 .. base+1 that the tile's texels
//                      interpolate from (the tile's share of the level and a halo of one texel) are completed in LDS, coarse to
//                      fine, then every hole of level `base` in the tile is filled in place.  Only level `base` is written: no
//                      workgroup reads what another writes in the same launch.
//  * k_fill_push       base = 0: the same, ending in the output.  A tile without a texel to fill (none invalid, or none in the
//                      domain) reads no pyramid level at all and is copied through.
//
// t4d_texture_fill16 is the same rule on 16-bit samples held in int32 (a quantised displacement map): the kernels are templated on
// the pyramid's word T, uint16 for 8-bit samples and uint32 for 16-bit ones (colours up to 65535 * 256, a hole is all ones in
// channel 0; the push sum reaches 16 * 65535 * 256 + 8 < 2^32, so it is taken in uint32).  Its level-0 kernels read and write the
// int32 image in global memory (k_fill_pull with kSrcI32, k_fill_push16): four bytes per sample leave no room to stage a tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxDim = 65536;                   // h, w: 16 levels above level 0
constexpr int kLevels = 17;
constexpr int kTile = 64;                        // texels per tile side
constexpr int kSpan = 6;                         // levels a workgroup fuses: 64 = 2^6
template <typename T> struct Hole { static constexpr uint32_t v = (uint32_t)(T) ~(T)0; };   // 0xFFFF / 0xFFFFFFFF in channel 0
enum PullSrc { kSrcLevel = 0, kSrcU8 = 1, kSrcI32 = 2 };   // what k_fill_pull's first level reads: the pyramid, or the image
constexpr int kPullTexels = 1365;                // 32^2 + 16^2 + ... + 1: a tile's levels 1 .. 6
constexpr int kPushTexels = 1641;                // 34^2 + 18^2 + 10^2 + 6^2 + 4^2 + 3^2: the same with a halo of one texel

template <typename T>
struct FillLevels {
    T *p[kLevels];                        // p[0] unused: level 0 is the image
    int32_t h[kLevels], w[kLevels];
    int32_t top;                                 // the 1x1 level
};

__device__ inline int pull_off(int j) { return (4096 - (4096 >> (2 * (j - 1)))) / 3; }     // texels before a tile's level j

__device__ inline int push_side(int j) { return (kTile >> j) + 2; }

__device__ inline int push_off(int j)
{
    int o = 0;
    for (int i = 1; i < j; ++i) o += push_side(i) * push_side(i);
    return o;
}

template <typename W> __device__ inline W zero_word();
template <> __device__ inline uint8_t zero_word<uint8_t>() { return 0; }
template <> __device__ inline uint32_t zero_word<uint32_t>() { return 0; }
template <> __device__ inline uint4 zero_word<uint4>() { return make_uint4(0, 0, 0, 0); }

// a tile's rows of B bytes per texel between global memory and LDS (64 * B bytes per LDS row), as words of type W: the host picks
// W so that every row of the image starts on a word (w * B a multiple of sizeof(W), the buffer aligned); the tile's rows then do
// too, since x0 * B is a multiple of 64.  Texels outside the image load as 0 and are not stored.
template <typename W>
__device__ inline void tile_load(const uint8_t *g, int h, int w, int B, int x0, int y0, W *s)
{
    const int row_words = kTile * B / (int)sizeof(W);
    const int row_bytes = (w - x0 < kTile ? w - x0 : kTile) * B;
    for (int i = threadIdx.x; i < kTile * row_words; i += kBlock) {
        const int r = i / row_words, k = i % row_words;
        const int64_t y = y0 + r;
        const bool ok = y < h && k * (int)sizeof(W) < row_bytes;
        s[i] = ok ? ((const W *)(g + (y * w + x0) * B))[k] : zero_word<W>();
    }
}

template <typename W>
__device__ inline void tile_store(uint8_t *g, int h, int w, int B, int x0, int y0, const W *s)
{
    const int row_words = kTile * B / (int)sizeof(W);
    const int row_bytes = (w - x0 < kTile ? w - x0 : kTile) * B;
    for (int i = threadIdx.x; i < kTile * row_words; i += kBlock) {
        const int r = i / row_words, k = i % row_words;
        const int64_t y = y0 + r;
        if (y < h && k * (int)sizeof(W) < row_bytes) ((W *)(g + (y * w + x0) * B))[k] = s[i];
    }
}

// the mean of n valid children with channel sums `sum`, round half up; kHole without any
template <int C, typename T>
__device__ inline void pull_store(T *t, uint32_t n, const uint32_t *sum)
{
    for (int c = 0; c < C; ++c) t[c] = n ? (T)((2 * sum[c] + n) / (2 * n)) : (T)0;
    if (!n) t[0] = (T)Hole<T>::v;
}

template <int C, int SRC, typename W, typename T>
__global__ __launch_bounds__(kBlock) void k_fill_pull(const void *image, const uint8_t *valid, FillLevels<T> L, int base, int jmax,
                                                      int tiles_x)
{
    constexpr bool IMG = SRC == kSrcU8;
    constexpr uint32_t kHole = Hole<T>::v;
    __shared__ T s[kPullTexels * C];
    __shared__ W simg[IMG ? kTile * kTile * C / sizeof(W) : 1];
    __shared__ W sval[IMG ? kTile * kTile / sizeof(W) : 1];
    const int x0 = (int)(blockIdx.x % tiles_x) * kTile, y0 = (int)(blockIdx.x / tiles_x) * kTile;
    const int bh = L.h[base], bw = L.w[base];
    if (IMG) {
        tile_load<W>((const uint8_t *)image, bh, bw, C, x0, y0, simg);
        tile_load<W>(valid, bh, bw, 1, x0, y0, sval);
        __syncthreads();
    }
    const uint8_t *si = (const uint8_t *)simg, *sv = (const uint8_t *)sval;
    for (int j = 1; j <= jmax; ++j) {
        const int side = kTile >> j;
        T *cur = s + pull_off(j) * C;
        const T *prev = s + (j > 1 ? pull_off(j - 1) : 0) * C;
        const int lev = base + j, lh = L.h[lev], lw = L.w[lev];
        for (int i = threadIdx.x; i < side * side; i += kBlock) {
            const int lx = i % side, ly = i / side;
            uint32_t n = 0, sum[C];
            for (int c = 0; c < C; ++c) sum[c] = 0;
            for (int k = 0; k < 4; ++k) {
                const int cx = 2 * lx + (k & 1), cy = 2 * ly + (k >> 1);
                if (j > 1) {                                              // texels outside the level are holes in LDS
                    const T *q = prev + (cy * 2 * side + cx) * C;
                    if (q[0] == kHole) continue;
                    ++n;
                    for (int c = 0; c < C; ++c) sum[c] += q[c];
                } else if (IMG) {                                         // texels outside the image were staged as not valid
                    const int at = cy * kTile + cx;
                    if (sv[at] == 0) continue;
                    ++n;
                    for (int c = 0; c < C; ++c) sum[c] += 256u * si[at * C + c];
                } else if (SRC == kSrcI32) {                              // the low 16 bits of an int32 image, from global memory
                    const int gx = x0 + cx, gy = y0 + cy;
                    if (gx >= bw || gy >= bh) continue;
                    const int64_t at = (int64_t)gy * bw + gx;
                    if (valid[at] == 0) continue;
                    ++n;
                    for (int c = 0; c < C; ++c) sum[c] += 256u * ((uint32_t)((const int32_t *)image)[at * C + c] & 0xFFFFu);
                } else {
                    const int gx = x0 + cx, gy = y0 + cy;
                    if (gx >= bw || gy >= bh) continue;
                    const T *q = L.p[base] + ((int64_t)gy * bw + gx) * C;
                    if (q[0] == kHole) continue;
                    ++n;
                    for (int c = 0; c < C; ++c) sum[c] += q[c];
                }
            }
            pull_store<C, T>(cur + i * C, n, sum);
            const int gx = (x0 >> j) + lx, gy = (y0 >> j) + ly;
            if (gx < lw && gy < lh) pull_store<C, T>(L.p[lev] + ((int64_t)gy * lw + gx) * C, n, sum);
        }
        __syncthreads();
    }
}

// texel (x, y) of a level from the completed level above, P: an LDS region of side n whose texel (0, 0) is the level's (ox, oy);
// pw, ph: that level's size
template <int C, typename T>
__device__ inline void fill_up(const T *P, int n, int ox, int oy, int pw, int ph, int x, int y, uint32_t *out)
{
    const int px = x >> 1, py = y >> 1;
    int nx = px + ((x & 1) ? 1 : -1), ny = py + ((y & 1) ? 1 : -1);
    nx = nx < 0 ? 0 : (nx > pw - 1 ? pw - 1 : nx);
    ny = ny < 0 ? 0 : (ny > ph - 1 ? ph - 1 : ny);
    const T *a = P + ((py - oy) * n + (px - ox)) * C, *b = P + ((py - oy) * n + (nx - ox)) * C;
    const T *d = P + ((ny - oy) * n + (px - ox)) * C, *e = P + ((ny - oy) * n + (nx - ox)) * C;
    for (int c = 0; c < C; ++c) out[c] = (9u * a[c] + 3u * b[c] + 3u * d[c] + e[c] + 8u) >> 4;
}

// The completed regions of levels base+jstart .. base+1 for the tile of level `base` at (x0, y0), into s.  The region of level
// base+j is the tile's share [x0 >> j, (x0 >> j) + (64 >> j)) and one texel round it: a texel of that region at level j has its
// parent and the parent's neighbour towards it inside the region of level j+1 (x0 >> j is even for j <= 5).  Level base+jstart is
// complete in global memory (the top, or the level the launch before completed); the others are read as pulled and their holes
// interpolated.  Texels outside a level are left alone: the clamp of the rule never names them.
template <int C, typename T>
__device__ inline void fill_regions(const FillLevels<T> &L, int base, int jstart, int x0, int y0, T *s)
{
    constexpr uint32_t kHole = Hole<T>::v;
    for (int j = jstart; j >= 1; --j) {
        const int lev = base + j, n = push_side(j), ox = (x0 >> j) - 1, oy = (y0 >> j) - 1, lh = L.h[lev], lw = L.w[lev];
        T *cur = s + push_off(j) * C;
        const T *P = s + push_off(j + 1) * C;
        for (int i = threadIdx.x; i < n * n; i += kBlock) {
            const int x = ox + i % n, y = oy + i / n;
            if (x < 0 || y < 0 || x >= lw || y >= lh) continue;
            const T *q = L.p[lev] + ((int64_t)y * lw + x) * C;
            uint32_t v[C];
            if (j < jstart && q[0] == kHole)
                fill_up<C, T>(P, push_side(j + 1), (x0 >> (j + 1)) - 1, (y0 >> (j + 1)) - 1, L.w[lev + 1], L.h[lev + 1], x, y, v);
            else
                for (int c = 0; c < C; ++c) v[c] = q[c];
            for (int c = 0; c < C; ++c) cur[i * C + c] = (T)v[c];
        }
        __syncthreads();
    }
}

template <int C, typename T>
__global__ __launch_bounds__(kBlock) void k_fill_push_coarse(FillLevels<T> L, int base, int jstart, int tiles_x)
{
    constexpr uint32_t kHole = Hole<T>::v;
    __shared__ T s[kPushTexels * C];
    if (L.p[L.top][0] == kHole) return;                                   // no valid texel at all: nothing will be read
    const int x0 = (int)(blockIdx.x % tiles_x) * kTile, y0 = (int)(blockIdx.x / tiles_x) * kTile;
    fill_regions<C, T>(L, base, jstart, x0, y0, s);
    const int bh = L.h[base], bw = L.w[base];
    for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {
        const int x = x0 + i % kTile, y = y0 + i / kTile;
        if (x >= bw || y >= bh) continue;
        T *q = L.p[base] + ((int64_t)y * bw + x) * C;
        if (q[0] != kHole) continue;
        uint32_t v[C];
        fill_up<C, T>(s, push_side(1), (x0 >> 1) - 1, (y0 >> 1) - 1, L.w[base + 1], L.h[base + 1], x, y, v);
        for (int c = 0; c < C; ++c) q[c] = (T)v[c];
    }
}

template <int C, typename W>
__global__ __launch_bounds__(kBlock) void k_fill_push(const uint8_t *image, const uint8_t *valid, const uint8_t *domain,
                                                      FillLevels<uint16_t> L, int jstart, int tiles_x, uint8_t *out, uint8_t *out_filled)
{
    constexpr uint32_t kHole = Hole<uint16_t>::v;
    __shared__ uint16_t s[kPushTexels * C];
    __shared__ W simg[kTile * kTile * C / sizeof(W)];
    __shared__ W sval[kTile * kTile / sizeof(W)];
    __shared__ W sdom[kTile * kTile / sizeof(W)];
    const int x0 = (int)(blockIdx.x % tiles_x) * kTile, y0 = (int)(blockIdx.x / tiles_x) * kTile;
    const int h = L.h[0], w = L.w[0];
    const bool any = L.top > 0 && L.p[L.top][0] != kHole;                 // (a 1x1 image has nothing to fill from)
    tile_load<W>(image, h, w, C, x0, y0, simg);
    tile_load<W>(valid, h, w, 1, x0, y0, sval);
    if (domain) tile_load<W>(domain, h, w, 1, x0, y0, sdom);
    __syncthreads();
    uint8_t *si = (uint8_t *)simg, *sv = (uint8_t *)sval;
    const uint8_t *sd = (const uint8_t *)sdom;
    int mine = 0;
    for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {           // sv: valid -> "to fill", which is out_filled
        const bool inside = x0 + i % kTile < w && y0 + i / kTile < h;
        const int need = any && inside && sv[i] == 0 && (!domain || sd[i] != 0);
        sv[i] = (uint8_t)need;
        mine |= need;
    }
    if (__syncthreads_or(mine)) {
        fill_regions<C, uint16_t>(L, 0, jstart, x0, y0, s);
        for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {
            if (!sv[i]) continue;
            uint32_t v[C];
            fill_up<C, uint16_t>(s, push_side(1), (x0 >> 1) - 1, (y0 >> 1) - 1, L.w[1], L.h[1], x0 + i % kTile, y0 + i / kTile, v);
            for (int c = 0; c < C; ++c) si[i * C + c] = (uint8_t)((v[c] + 128u) >> 8);
        }
        __syncthreads();
    }
    tile_store<W>(out, h, w, C, x0, y0, simg);
    tile_store<W>(out_filled, h, w, 1, x0, y0, sval);
}

// k_fill_push for the int32 image of 16-bit samples: the same rule, with the image, the masks and the outputs in global memory.
// Every texel of the tile is written exactly once: a copy (the low 16 bits) or its fill.
template <int C>
__global__ __launch_bounds__(kBlock) void k_fill_push16(const int32_t *image, const uint8_t *valid, const uint8_t *domain,
                                                        FillLevels<uint32_t> L, int jstart, int tiles_x, int32_t *out, uint8_t *out_filled)
{
    constexpr uint32_t kHole = Hole<uint32_t>::v;
    __shared__ uint32_t s[kPushTexels * C];
    __shared__ uint8_t sneed[kTile * kTile];
    const int x0 = (int)(blockIdx.x % tiles_x) * kTile, y0 = (int)(blockIdx.x / tiles_x) * kTile;
    const int h = L.h[0], w = L.w[0];
    const bool any = L.top > 0 && L.p[L.top][0] != kHole;                 // (a 1x1 image has nothing to fill from)
    int mine = 0;
    for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {
        const int x = x0 + i % kTile, y = y0 + i / kTile;
        int need = 0;
        if (x < w && y < h) {
            const int64_t at = (int64_t)y * w + x;
            need = any && valid[at] == 0 && (!domain || domain[at] != 0);
            out_filled[at] = (uint8_t)need;
            if (!need)
                for (int c = 0; c < C; ++c) out[at * C + c] = (int32_t)((uint32_t)image[at * C + c] & 0xFFFFu);
        }
        sneed[i] = (uint8_t)need;
        mine |= need;
    }
    if (!__syncthreads_or(mine)) return;
    fill_regions<C, uint32_t>(L, 0, jstart, x0, y0, s);
    for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {
        if (!sneed[i]) continue;
        const int x = x0 + i % kTile, y = y0 + i / kTile;
        uint32_t v[C];
        fill_up<C, uint32_t>(s, push_side(1), (x0 >> 1) - 1, (y0 >> 1) - 1, L.w[1], L.h[1], x, y, v);
        for (int c = 0; c < C; ++c) out[((int64_t)y * w + x) * C + c] = (int32_t)((v[c] + 128u) >> 8);
    }
}

bool dims_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= kMaxDim && w <= kMaxDim; }
bool channels_ok(int32_t c) { return c == 1 || c == 3 || c == 4; }
bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int level_dim(int32_t n, int k) { return ((n - 1) >> k) + 1; }            // ceil(n / 2^k)

int top_level(int32_t h, int32_t w)
{
    int t = 0;
    while (level_dim(h, t) > 1 || level_dim(w, t) > 1) ++t;
    return t;
}

size_t level_bytes(int32_t h, int32_t w, int32_t c, int k, size_t word = sizeof(uint16_t))
{
    return align_up((size_t)level_dim(h, k) * (size_t)level_dim(w, k) * (size_t)c * word);
}

size_t fill_scratch(int32_t h, int32_t w, int32_t c, size_t word = sizeof(uint16_t))
{
    size_t n = 256;                                                       // never 0: 0 is the size query's refusal
    for (int k = 1; k <= top_level(h, w); ++k) n += level_bytes(h, w, c, k, word);
    return n;
}

template <typename T>
FillLevels<T> make_levels(int32_t h, int32_t w, int32_t c, void *scratch)
{
    FillLevels<T> L = {};
    L.top = top_level(h, w);
    uint8_t *at = (uint8_t *)scratch;
    for (int k = 0; k <= L.top; ++k) {
        L.h[k] = level_dim(h, k);
        L.w[k] = level_dim(w, k);
        if (k == 0) continue;
        L.p[k] = (T *)at;
        at += level_bytes(h, w, c, k, sizeof(T));
    }
    return L;
}

unsigned tiles(int n) { return (unsigned)((n + kTile - 1) / kTile); }

template <int C, typename W>
void launch(const uint8_t *image, const uint8_t *valid, const uint8_t *domain, const FillLevels<uint16_t> &L, uint8_t *out,
            uint8_t *out_filled, hipStream_t stream)
{
    const int top = L.top;
    int base = 0;
    for (; base < top; base += kSpan) {
        const int jmax = top - base < kSpan ? top - base : kSpan;
        const int tiles_x = (int)tiles(L.w[base]);
        const dim3 grid((unsigned)tiles_x * tiles(L.h[base]));
        if (base == 0)
            hipLaunchKernelGGL((k_fill_pull<C, kSrcU8, W, uint16_t>), grid, dim3(kBlock), 0, stream, (const void *)image, valid, L, base,
                               jmax, tiles_x);
        else
            hipLaunchKernelGGL((k_fill_pull<C, kSrcLevel, uint8_t, uint16_t>), grid, dim3(kBlock), 0, stream, (const void *)image, valid,
                               L, base, jmax, tiles_x);
    }
    for (base -= kSpan; base > 0; base -= kSpan) {
        const int jstart = top - base < kSpan ? top - base : kSpan;
        const int tiles_x = (int)tiles(L.w[base]);
        hipLaunchKernelGGL((k_fill_push_coarse<C, uint16_t>), dim3((unsigned)tiles_x * tiles(L.h[base])), dim3(kBlock), 0, stream, L,
                           base, jstart, tiles_x);
    }
    const int tiles_x = (int)tiles(L.w[0]);
    hipLaunchKernelGGL((k_fill_push<C, W>), dim3((unsigned)tiles_x * tiles(L.h[0])), dim3(kBlock), 0, stream, image, valid, domain, L,
                       top < kSpan ? top : kSpan, tiles_x, out, out_filled);
}

// the same launch sequence for the int32 image of 16-bit samples
template <int C>
void launch16(const int32_t *image, const uint8_t *valid, const uint8_t *domain, const FillLevels<uint32_t> &L, int32_t *out,
              uint8_t *out_filled, hipStream_t stream)
{
    const int top = L.top;
    int base = 0;
    for (; base < top; base += kSpan) {
        const int jmax = top - base < kSpan ? top - base : kSpan;
        const int tiles_x = (int)tiles(L.w[base]);
        const dim3 grid((unsigned)tiles_x * tiles(L.h[base]));
        if (base == 0)
            hipLaunchKernelGGL((k_fill_pull<C, kSrcI32, uint8_t, uint32_t>), grid, dim3(kBlock), 0, stream, (const void *)image, valid, L,
                               base, jmax, tiles_x);
        else
            hipLaunchKernelGGL((k_fill_pull<C, kSrcLevel, uint8_t, uint32_t>), grid, dim3(kBlock), 0, stream, (const void *)image, valid,
                               L, base, jmax, tiles_x);
    }
    for (base -= kSpan; base > 0; base -= kSpan) {
        const int jstart = top - base < kSpan ? top - base : kSpan;
        const int tiles_x = (int)tiles(L.w[base]);
        hipLaunchKernelGGL((k_fill_push_coarse<C, uint32_t>), dim3((unsigned)tiles_x * tiles(L.h[base])), dim3(kBlock), 0, stream, L,
                           base, jstart, tiles_x);
    }
    const int tiles_x = (int)tiles(L.w[0]);
    hipLaunchKernelGGL((k_fill_push16<C>), dim3((unsigned)tiles_x * tiles(L.h[0])), dim3(kBlock), 0, stream, image, valid, domain, L,
                       top < kSpan ? top : kSpan, tiles_x, out, out_filled);
}

template <int C>
void launch_words(size_t word, const uint8_t *image, const uint8_t *valid, const uint8_t *domain, const FillLevels<uint16_t> &L, uint8_t *out,
                  uint8_t *out_filled, hipStream_t stream)
{
    if (word == 16) launch<C, uint4>(image, valid, domain, L, out, out_filled, stream);
    else if (word == 4) launch<C, uint32_t>(image, valid, domain, L, out, out_filled, stream);
    else launch<C, uint8_t>(image, valid, domain, L, out, out_filled, stream);
}

}  // namespace

T4D_EXPORT size_t t4d_texture_fill_scratch_bytes(int32_t h, int32_t w, int32_t c)
{
    if (!dims_ok(h, w) || !channels_ok(c)) {
        t4d_fail(T4D_ERR_ARG, "t4d_texture_fill_scratch_bytes: need 1 <= h, w <= %d and c in {1, 3, 4}, got %d x %d x %d", kMaxDim, h, w, c);
        return 0;
    }
    return fill_scratch(h, w, c);
}

T4D_EXPORT int t4d_texture_fill(const uint8_t *image, const uint8_t *valid, const uint8_t *domain, int32_t h, int32_t w, int32_t c,
                                uint8_t *out_image, uint8_t *out_filled, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!image || !valid || !out_image || !out_filled || !scratch || image == out_image || valid == out_filled || domain == out_filled)
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_fill: NULL buffer, or input and output are one buffer");
    if (!dims_ok(h, w) || !channels_ok(c))
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_fill: need 1 <= h, w <= %d and c in {1, 3, 4}, got %d x %d x %d", kMaxDim, h, w, c);
    if (scratch_bytes < fill_scratch(h, w, c))
        return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_texture_fill: scratch below t4d_texture_fill_scratch_bytes(h, w, c)");
    if (!aligned(scratch, 2)) return t4d_fail(T4D_ERR_ARG, "t4d_texture_fill: the scratch must be aligned to 2 bytes");
    const FillLevels<uint16_t> L = make_levels<uint16_t>(h, w, c, scratch);
    // the widest word every row of every byte image starts on
    size_t word = 1;
    for (size_t cand : {(size_t)16, (size_t)4}) {
        if (w % (int)cand == 0 && aligned(image, cand) && aligned(valid, cand) && aligned(out_image, cand) && aligned(out_filled, cand) &&
            (!domain || aligned(domain, cand))) {
            word = cand;
            break;
        }
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    if (c == 1) launch_words<1>(word, image, valid, domain, L, out_image, out_filled, stream);
    else if (c == 3) launch_words<3>(word, image, valid, domain, L, out_image, out_filled, stream);
    else launch_words<4>(word, image, valid, domain, L, out_image, out_filled, stream);
    return t4d_launch_status("t4d_texture_fill");
}

T4D_EXPORT size_t t4d_texture_fill16_scratch_bytes(int32_t h, int32_t w, int32_t c)
{
    if (!dims_ok(h, w) || !channels_ok(c)) {
        t4d_fail(T4D_ERR_ARG, "t4d_texture_fill16_scratch_bytes: need 1 <= h, w <= %d and c in {1, 3, 4}, got %d x %d x %d", kMaxDim, h, w, c);
        return 0;
    }
    return fill_scratch(h, w, c, sizeof(uint32_t));
}

T4D_EXPORT int t4d_texture_fill16(const int32_t *image, const uint8_t *valid, const uint8_t *domain, int32_t h, int32_t w, int32_t c,
                                  int32_t *out_image, uint8_t *out_filled, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!image || !valid || !out_image || !out_filled || !scratch || image == out_image || valid == out_filled || domain == out_filled)
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_fill16: NULL buffer, or input and output are one buffer");
    if (!dims_ok(h, w) || !channels_ok(c))
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_fill16: need 1 <= h, w <= %d and c in {1, 3, 4}, got %d x %d x %d", kMaxDim, h, w, c);
    if (scratch_bytes < fill_scratch(h, w, c, sizeof(uint32_t)))
        return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_texture_fill16: scratch below t4d_texture_fill16_scratch_bytes(h, w, c)");
    if (!aligned(scratch, 4) || !aligned(image, 4) || !aligned(out_image, 4))
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_fill16: the images and the scratch must be aligned to 4 bytes");
    const FillLevels<uint32_t> L = make_levels<uint32_t>(h, w, c, scratch);
    hipStream_t stream = (hipStream_t)hip_stream;
    if (c == 1) launch16<1>(image, valid, domain, L, out_image, out_filled, stream);
    else if (c == 3) launch16<3>(image, valid, domain, L, out_image, out_filled, stream);
    else launch16<4>(image, valid, domain, L, out_image, out_filled, stream);
    return t4d_launch_status("t4d_texture_fill16");
}
