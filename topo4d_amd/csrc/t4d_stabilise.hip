// t4d_stabilise.hip — what topo4d_amd/drift.py makes of the matcher's measurement: the dense flow of every texel from the block
// nodes, and frame b's texture resampled through it.  The rule is stated in include/topo4d_raster.h; everything is integer
// arithmetic in a fixed order, so both results are pure functions of the inputs and do not depend on the launch shape.
// tests/stabilise_ref.py restates the rule in numpy.
//
//  * k_drift_dense   one workgroup per tile of 64 x 16 texels, one lane per texel column and four rows.  The nodes within reach
//                    of the tile, at most (16 + 2 reach) x (64 + 2 reach) of them, are staged in LDS once: q and the label under
//                    which the node takes part (0: not kept, or no island).  Every lane then walks the at most (2 reach)^2 nodes
//                    with a positive weight for its texel; a wave's 64 lanes read neighbouring or identical LDS words.  A row of
//                    a wave's flow is one coalesced store of 64 int32x2.  The node ranges come from a float reciprocal of the
//                    node spacing with an exact integer correction, not from integer divisions; a weight is one 32-bit product
//                    (the entry point refuses T^2 >= 2^31), and the two rounded divisions run in 32 bits whenever numerator
//                    and denominator fit and in 64 bits otherwise.
//  * k_drift_warp    streaming, one workgroup per 256 texels of one row, one texel per lane, so no lane divides by the width.
//                    The four taps of neighbouring lanes lie on the same two rows next to each other, so they share cache
//                    lines; the two taps of a row are neighbours in memory, so where both lie inside the image one 2-byte
//                    load fetches both validities, one both labels and one 2 C-byte copy both colours (the load
//                    instructions, not the bytes, bound this kernel).  The workgroup's output bytes meet in LDS and leave as whole dwords when the width is a multiple
//                    of 4 (every row then starts on a dword), as bytes otherwise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxDim = 65536;
constexpr int kMinB = 8, kMaxB = 64, kMaxLevel = 8, kMaxReach = 4;
constexpr int kTileW = 64, kTileH = 16;
constexpr int kNodesY = kTileH + 2 * kMaxReach, kNodesX = kTileW + 2 * kMaxReach;    // a tile's nodes: see nodes_of
constexpr int kRowsPerLane = kTileH * kTileW / kBlock;
constexpr int kMaxT = 46340;                                   // T^2 < 2^31: a weight wy wx fits 32 bits
// nodes_of: the nodes within reach of n texels in a row span at most 2 (n - 1) + 2 (T - 1) doubled indices, P >= 2 apart with
// T = reach P, so there are at most n + 2 reach - 1 of them; the staging arrays and the lane layout rest on these
static_assert(kNodesY >= kTileH + 2 * kMaxReach - 1 && kNodesX >= kTileW + 2 * kMaxReach - 1, "a tile's nodes must fit the LDS arrays");
static_assert(kBlock % kTileW == 0 && kRowsPerLane * kBlock == kTileH * kTileW, "a lane owns one column and kRowsPerLane rows");
static_assert(3 * kNodesY * kNodesX * sizeof(int) <= 65536, "the staged nodes fit the static LDS limit");

struct DenseGrid {
    int nby, nbx;          // nodes
    int P, c0, T;          // doubled texel indices: node k lies at P k + c0, and the weight reaches T
    float inv_p;           // 1 / P
    int lab0, lab_step;    // the texel of node k's label: lab0 + k lab_step
};

// floor(a / P) for |a| < 2^23: a is exact in float and the product is within one of the quotient, which the remainder corrects
__device__ inline int floor_div(int a, int P, float inv_p)
{
    int q = (int)floorf((float)a * inv_p);
    const int r = a - q * P;
    if (r < 0) --q;
    else if (r >= P) ++q;
    return q;
}

// the nodes k with |v - (P k + c0)| < T for some doubled index v in [lo2, hi2], clamped to 0..n-1.  P >= 2 and T = reach P, so
// there are at most (hi2 - lo2) / 2 + 2 reach of them.
__device__ inline void nodes_of(const DenseGrid &g, int lo2, int hi2, int n, int &first, int &last)
{
    first = max(0, floor_div(lo2 - g.T - g.c0 + g.P, g.P, g.inv_p));
    last = min(n - 1, floor_div(hi2 + g.T - 1 - g.c0, g.P, g.inv_p));
}

// floor((2 num + den) / (2 den)) with den > 0
__device__ inline int32_t rounded_div(int64_t num, int64_t den)
{
    const int64_t n = 2 * num + den, d = 2 * den;
    const uint64_t a = (uint64_t)(n < 0 ? -n : n);
    if (((a | (uint64_t)d) >> 32) == 0) {
        const uint32_t a32 = (uint32_t)a, d32 = (uint32_t)d;
        const uint32_t q = a32 / d32;
        return n < 0 ? -(int32_t)q - (int32_t)(q * d32 != a32) : (int32_t)q;
    }
    int64_t q = n / d;
    if (n < 0 && q * d != n) --q;
    return (int32_t)q;
}

__global__ __launch_bounds__(kBlock) void k_drift_dense(const int32_t *nodes, const uint8_t *kept, const uint8_t *labels, int H, int W,
                                                        DenseGrid g, int32_t *flow, uint8_t *support)
{
    __shared__ int s_qy[kNodesY * kNodesX], s_qx[kNodesY * kNodesX], s_part[kNodesY * kNodesX];
    const int x0 = (int)blockIdx.x * kTileW, y0 = (int)blockIdx.y * kTileH;
    const int x1 = min(x0 + kTileW, W) - 1, y1 = min(y0 + kTileH, H) - 1;
    int by0, by1, bx0, bx1;
    nodes_of(g, 2 * y0, 2 * y1, g.nby, by0, by1);
    nodes_of(g, 2 * x0, 2 * x1, g.nbx, bx0, bx1);
    const int cy = min(max(by1 - by0 + 1, 0), kNodesY), cx = min(max(bx1 - bx0 + 1, 0), kNodesX);
    for (int i = threadIdx.x; i < cy * cx; i += kBlock) {
        const int j = i / cx, k = i - j * cx;
        const int by = by0 + j, bx = bx0 + k;
        const int64_t node = (int64_t)by * g.nbx + bx;
        const int lab = labels[(int64_t)(g.lab0 + by * g.lab_step) * W + (g.lab0 + bx * g.lab_step)];
        s_qy[i] = nodes[2 * node];
        s_qx[i] = nodes[2 * node + 1];
        s_part[i] = kept[node] ? lab : 0;
    }
    __syncthreads();
    const int x = x0 + (int)(threadIdx.x % kTileW);
    if (x >= W) return;
    int kx0, kx1;
    nodes_of(g, 2 * x, 2 * x, g.nbx, kx0, kx1);
    kx0 = max(kx0, bx0), kx1 = min(kx1, bx0 + cx - 1);
    for (int r = 0; r < kRowsPerLane; ++r) {
        const int y = y0 + (int)(threadIdx.x / kTileW) + r * (kBlock / kTileW);
        if (y >= H) break;
        const int64_t texel = (int64_t)y * W + x;
        const int l = labels[texel];
        int64_t num_y = 0, num_x = 0, den = 0;
        if (l != 0) {
            int ky0, ky1;
            nodes_of(g, 2 * y, 2 * y, g.nby, ky0, ky1);
            ky0 = max(ky0, by0), ky1 = min(ky1, by0 + cy - 1);
            for (int by = ky0; by <= ky1; ++by) {
                const int wy = g.T - abs(2 * y - (g.P * by + g.c0));
                const int row = (by - by0) * cx - bx0;
                for (int bx = kx0; bx <= kx1; ++bx) {
                    const int wx = g.T - abs(2 * x - (g.P * bx + g.c0));
                    if (s_part[row + bx] != l) continue;
                    const int wgt = wy * wx;                   // T <= kMaxT
                    den += wgt;
                    num_y += (int64_t)wgt * s_qy[row + bx];
                    num_x += (int64_t)wgt * s_qx[row + bx];
                }
            }
        }
        int2 f = make_int2(0, 0);
        if (den > 0) f = make_int2(rounded_div(num_y, den), rounded_div(num_x, den));
        reinterpret_cast<int2 *>(flow)[texel] = f;
        support[texel] = den > 0 ? 1 : 0;
    }
}

template <int C, bool Wide>                                    // Wide: W % 4 == 0, every row of both outputs starts on a dword
__global__ __launch_bounds__(kBlock) void k_drift_warp(const uint8_t *image, const uint8_t *valid, const uint8_t *labels,
                                                       const int32_t *flow, int H, int W, uint8_t *out, uint8_t *out_valid)
{
    __shared__ uint32_t s_out[kBlock * C / 4], s_valid[kBlock / 4];
    uint8_t *so = reinterpret_cast<uint8_t *>(s_out), *sv = reinterpret_cast<uint8_t *>(s_valid);
    const int y = (int)blockIdx.x, x0 = (int)blockIdx.y * kBlock, x = x0 + (int)threadIdx.x;
    const int64_t first = (int64_t)y * W + x0;                 // the workgroup's first texel
    uint32_t sum[C], total = 0;
    for (int ch = 0; ch < C; ++ch) sum[ch] = 0;
    if (x < W) {
        const int64_t i = first + threadIdx.x;
        const int l = labels[i];
        const int2 f = reinterpret_cast<const int2 *>(flow)[i];
        const int64_t Y = 256 * (int64_t)y + f.x, X = 256 * (int64_t)x + f.y;
        const int64_t ty0 = Y >> 8, tx0 = X >> 8;
        const uint32_t ty = (uint32_t)(Y & 255), tx = (uint32_t)(X & 255);
        if (l != 0) {
            const bool pair = tx0 >= 0 && tx0 + 1 < W;         // both taps of a row inside: they are neighbours in memory
            for (int a = 0; a < 2; ++a) {
                const int64_t yy = ty0 + a;
                if (yy < 0 || yy >= H) continue;
                const uint32_t wy = a ? ty : 256 - ty;
                if (pair) {                                    // one load each for the two validities, labels and colours
                    const int64_t j = yy * W + tx0;
                    uint16_t v2, l2;
                    uint8_t px[2 * C];
                    __builtin_memcpy(&v2, valid + j, 2);
                    __builtin_memcpy(&l2, labels + j, 2);
                    __builtin_memcpy(px, image + j * C, 2 * C);
                    for (int b = 0; b < 2; ++b) {
                        if (((v2 >> (8 * b)) & 255) == 0 || (int)((l2 >> (8 * b)) & 255) != l) continue;
                        const uint32_t wgt = wy * (b ? tx : 256 - tx);
                        total += wgt;
                        for (int ch = 0; ch < C; ++ch) sum[ch] += wgt * px[b * C + ch];
                    }
                    continue;
                }
                for (int b = 0; b < 2; ++b) {
                    const int64_t xx = tx0 + b;
                    if (xx < 0 || xx >= W) continue;
                    const int64_t j = yy * W + xx;
                    if (valid[j] == 0 || labels[j] != l) continue;
                    const uint32_t wgt = wy * (b ? tx : 256 - tx);
                    total += wgt;
                    for (int ch = 0; ch < C; ++ch) sum[ch] += wgt * image[j * C + ch];
                }
            }
        }
    }
    for (int ch = 0; ch < C; ++ch) so[threadIdx.x * C + ch] = total ? (uint8_t)((2 * sum[ch] + total) / (2 * total)) : 0;
    sv[threadIdx.x] = total ? 1 : 0;
    __syncthreads();
    const int n = min(kBlock, W - x0);                         // the workgroup's texels; with Wide a multiple of 4, as first is
    if (Wide) {
        for (int k = threadIdx.x; 4 * k < n * C; k += kBlock) reinterpret_cast<uint32_t *>(out + first * C)[k] = s_out[k];
        if (4 * (int)threadIdx.x < n) reinterpret_cast<uint32_t *>(out_valid + first)[threadIdx.x] = s_valid[threadIdx.x];
    } else {
        for (int k = threadIdx.x; k < n * C; k += kBlock) out[first * C + k] = so[k];
        if ((int)threadIdx.x < n) out_valid[first + threadIdx.x] = sv[threadIdx.x];
    }
}

template <int C>
void launch_warp(hipStream_t stream, const uint8_t *image, const uint8_t *valid, const uint8_t *labels, const int32_t *flow, int h, int w,
                 uint8_t *out, uint8_t *out_valid)
{
    const dim3 grid((unsigned)h, (unsigned)((w + kBlock - 1) / kBlock));
    if (w % 4 == 0)
        hipLaunchKernelGGL((k_drift_warp<C, true>), grid, dim3(kBlock), 0, stream, image, valid, labels, flow, h, w, out, out_valid);
    else
        hipLaunchKernelGGL((k_drift_warp<C, false>), grid, dim3(kBlock), 0, stream, image, valid, labels, flow, h, w, out, out_valid);
}

bool dims_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= kMaxDim && w <= kMaxDim; }

}  // namespace

T4D_EXPORT int t4d_drift_dense(const int32_t *nodes, const uint8_t *kept, const uint8_t *labels, int32_t h, int32_t w, int32_t block,
                               int32_t stride, int32_t level, int32_t reach, int32_t *flow, uint8_t *support, void *hip_stream)
{
    if (!labels || !flow || !support) return t4d_fail(T4D_ERR_ARG, "t4d_drift_dense: NULL buffer");
    if (!dims_ok(h, w) || block < kMinB || block > kMaxB || block % 2 || stride < 1 || stride > block || level < 0 || level > kMaxLevel ||
        reach < 1 || reach > kMaxReach)
        return t4d_fail(T4D_ERR_ARG,
                        "t4d_drift_dense: need 1 <= h, w <= %d, block even in %d..%d, stride in 1..block, level in 0..%d and reach in "
                        "1..%d, got %d x %d, block %d, stride %d, level %d, reach %d", kMaxDim, kMinB, kMaxB, kMaxLevel, kMaxReach, h, w,
                        block, stride, level, reach);
    if (h % (1 << level) || w % (1 << level))
        return t4d_fail(T4D_ERR_ARG, "t4d_drift_dense: %d x %d is not divisible by 2^level = %d", h, w, 1 << level);
    if (((uintptr_t)flow & 7) != 0 || ((uintptr_t)nodes & 3) != 0)
        return t4d_fail(T4D_ERR_ARG, "t4d_drift_dense: flow must be aligned to 8 bytes and nodes to 4");
    const int lh = h >> level, lw = w >> level;
    DenseGrid g;
    g.nby = lh >= block ? (lh - block) / stride + 1 : 0;
    g.nbx = lw >= block ? (lw - block) / stride + 1 : 0;
    if (g.nby == 0 || g.nbx == 0) g.nby = g.nbx = 0;                     // no block: every texel gets f = 0 and support = 0
    if (g.nby != 0 && (!nodes || !kept)) return t4d_fail(T4D_ERR_ARG, "t4d_drift_dense: NULL buffer");
    g.P = stride << (level + 1);
    g.c0 = ((block / 2) << (level + 1)) - 1;
    g.T = reach * g.P;
    if (g.T > kMaxT)
        return t4d_fail(T4D_ERR_ARG, "t4d_drift_dense: reach 2 stride 2^level must be at most %d, got %d", kMaxT, g.T);
    g.inv_p = 1.0f / (float)g.P;
    g.lab0 = (block / 2) << level;
    g.lab_step = stride << level;
    const dim3 grid((unsigned)((w + kTileW - 1) / kTileW), (unsigned)((h + kTileH - 1) / kTileH));
    hipStream_t stream = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_drift_dense, grid, dim3(kBlock), 0, stream, nodes, kept, labels, h, w, g, flow, support);
    return t4d_launch_status("t4d_drift_dense");
}

T4D_EXPORT int t4d_drift_warp(const uint8_t *image, const uint8_t *valid, const uint8_t *labels, const int32_t *flow, int32_t h, int32_t w,
                              int32_t c, uint8_t *out_image, uint8_t *out_valid, void *hip_stream)
{
    if (!image || !valid || !labels || !flow || !out_image || !out_valid) return t4d_fail(T4D_ERR_ARG, "t4d_drift_warp: NULL buffer");
    if (!dims_ok(h, w) || (c != 1 && c != 3 && c != 4))
        return t4d_fail(T4D_ERR_ARG, "t4d_drift_warp: need 1 <= h, w <= %d and c in (1, 3, 4), got %d x %d x %d", kMaxDim, h, w, c);
    if (((uintptr_t)flow & 7) != 0 || ((uintptr_t)out_image & 3) != 0 || ((uintptr_t)out_valid & 3) != 0)
        return t4d_fail(T4D_ERR_ARG, "t4d_drift_warp: flow must be aligned to 8 bytes, out_image and out_valid to 4");
    if (out_image == image || out_valid == valid) return t4d_fail(T4D_ERR_ARG, "t4d_drift_warp: the outputs must not be the inputs");
    hipStream_t stream = (hipStream_t)hip_stream;
    if (c == 1)
        launch_warp<1>(stream, image, valid, labels, flow, h, w, out_image, out_valid);
    else if (c == 3)
        launch_warp<3>(stream, image, valid, labels, flow, h, w, out_image, out_valid);
    else
        launch_warp<4>(stream, image, valid, labels, flow, h, w, out_image, out_valid);
    return t4d_launch_status("t4d_drift_warp");
}
