// t4d_dispmap.hip — finishing a baked displacement map on the device (topo4d_amd/dispmap.py): quantise to 16-bit codes, smooth the
// codes within their UV island, derive the tangent-space normal map.  include/topo4d_raster.h states the rules; everything is integer
// or float64 arithmetic in a fixed order without contraction, so every output is a pure function of the inputs and does not depend on
// the launch shape.  tests/dispmap_ref.py restates the rules in numpy.
//
//  * k_disp_quantize  one texel per thread.
//  * k_disp_smooth    one round: a workgroup owns a 64x16 tile and stages it with a halo of 2 in LDS, one word per texel: the code
//                     in the low half and, above it, the texel's key: its label where it has a value, 0 elsewhere and outside the
//                     image.  A tap counts when its key equals the centre's label, which is never 0.  Rounds ping-pong between
//                     `out` and one scratch image so that the last lands in `out`; a kernel boundary orders them.
//  * k_disp_normals   one texel per thread; the four neighbours come from global memory (each is read by four texels, the caches
//                     serve them).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxDim = 65536;
constexpr int kMaxRounds = 8;
constexpr int kTileW = 64, kTileH = 16;          // texels a workgroup smooths: 4 per thread
constexpr int kHalo = 2;
constexpr int kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo;

__global__ __launch_bounds__(kBlock) void k_disp_quantize(const float *disp, const uint8_t *hit, double dist, int64_t n, int32_t *code,
                                                          uint8_t *has)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float d = disp[i];
    const bool ok = hit[i] != 0 && isfinite(d);
    int32_t v = 32768;
    if (ok) {
        double q = rint(((double)d / dist) * 32767.0);                 // round half to even
        q = q < -32767.0 ? -32767.0 : (q > 32767.0 ? 32767.0 : q);
        v += (int32_t)q;
    }
    code[i] = v;
    has[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_disp_copy(const int32_t *code, int64_t n, int32_t *out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = code[i] & 0xFFFF;
}

__global__ __launch_bounds__(kBlock) void k_disp_smooth(const int32_t *code, const uint8_t *has, const uint8_t *labels, int h, int w,
                                                        int tiles_x, int32_t *out)
{
    __shared__ uint32_t s[kLdsH * kLdsW];
    const int x0 = (int)(blockIdx.x % tiles_x) * kTileW, y0 = (int)(blockIdx.x / tiles_x) * kTileH;
    for (int i = threadIdx.x; i < kLdsH * kLdsW; i += kBlock) {
        const int x = x0 - kHalo + i % kLdsW, y = y0 - kHalo + i / kLdsW;
        uint32_t v = 0;
        if (x >= 0 && y >= 0 && x < w && y < h) {
            const int64_t at = (int64_t)y * w + x;
            const uint32_t key = has[at] ? labels[at] : 0u;
            v = ((uint32_t)code[at] & 0xFFFFu) | (key << 16);
        }
        s[i] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTileH * kTileW; i += kBlock) {
        const int lx = i % kTileW, ly = i / kTileW;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= w || y >= h) continue;
        const uint32_t *c = s + (ly + kHalo) * kLdsW + (lx + kHalo);
        const uint32_t key = c[0] >> 16;
        uint32_t r = c[0] & 0xFFFFu;
        if (key != 0) {
            uint32_t S = 0, Wt = 0;
            for (int j = -2; j <= 2; ++j) {
                const uint32_t wj = j == 0 ? 6u : (j == -1 || j == 1) ? 4u : 1u;
                for (int k = -2; k <= 2; ++k) {
                    const uint32_t wk = k == 0 ? 6u : (k == -1 || k == 1) ? 4u : 1u;
                    const uint32_t t = c[j * kLdsW + k];
                    if ((t >> 16) != key) continue;
                    S += wj * wk * (t & 0xFFFFu);
                    Wt += wj * wk;
                }
            }
            r = (2u * S + Wt) / (2u * Wt);                            // S <= 256 * 65535: no overflow
        }
        out[(int64_t)y * w + x] = (int32_t)r;
    }
}

// does texel (x, y) count as a neighbour of a texel with label L?
__device__ __forceinline__ bool same_island(const uint8_t *has, const uint8_t *labels, int h, int w, int x, int y, uint32_t L)
{
    if (x < 0 || y < 0 || x >= w || y >= h) return false;
    const int64_t at = (int64_t)y * w + x;
    return has[at] != 0 && labels[at] == L;
}

// the slope between texels p and m (indices into the maps): code difference in scan units over the distance of their surface points
__device__ __forceinline__ double slope(const int32_t *code, const float *pos, int64_t p, int64_t m, double unit)
{
#pragma clang fp contract(off)
    if (p == m) return 0.0;
    const double t0 = (double)pos[3 * p] - (double)pos[3 * m];
    const double t1 = (double)pos[3 * p + 1] - (double)pos[3 * m + 1];
    const double t2 = (double)pos[3 * p + 2] - (double)pos[3 * m + 2];
    const double a = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
    if (a == 0.0) return 0.0;
    return ((double)((code[p] & 0xFFFF) - (code[m] & 0xFFFF)) * unit) / a;
}

__device__ __forceinline__ int32_t encode_unit(double v)
{
#pragma clang fp contract(off)
    const double q = rint((v * 0.5 + 0.5) * 65535.0);
    if (!(q >= 0.0)) return 0;                                        // also NaN (non-finite positions)
    return (int32_t)(q > 65535.0 ? 65535.0 : q);
}

__global__ __launch_bounds__(kBlock) void k_disp_normals(const int32_t *code, const uint8_t *has, const uint8_t *labels, const float *pos,
                                                         double unit, int h, int w, int32_t *normal)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)h * w) return;
    const int x = (int)(i % w), y = (int)(i / w);
    double sx = 0.0, sy = 0.0;
    const uint32_t L = labels[i];
    if (has[i] != 0 && L != 0) {
        const int xp = same_island(has, labels, h, w, x + 1, y, L) ? x + 1 : x;
        const int xm = same_island(has, labels, h, w, x - 1, y, L) ? x - 1 : x;
        const int yp = same_island(has, labels, h, w, x, y + 1, L) ? y + 1 : y;
        const int ym = same_island(has, labels, h, w, x, y - 1, L) ? y - 1 : y;
        sx = slope(code, pos, (int64_t)y * w + xp, (int64_t)y * w + xm, unit);
        sy = slope(code, pos, (int64_t)yp * w + x, (int64_t)ym * w + x, unit);
    }
    const double len = sqrt((sx * sx + sy * sy) + 1.0);
    normal[3 * i] = encode_unit(-sx / len);
    normal[3 * i + 1] = encode_unit(sy / len);
    normal[3 * i + 2] = encode_unit(1.0 / len);
}

bool dims_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= kMaxDim && w <= kMaxDim; }
unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }
size_t smooth_scratch(int32_t h, int32_t w) { return 256 + align_up((size_t)h * (size_t)w * sizeof(int32_t)); }

}  // namespace

T4D_EXPORT int t4d_disp_quantize(const float *disp, const uint8_t *hit, int32_t h, int32_t w, double dist, int32_t *code, uint8_t *has,
                                 void *hip_stream)
{
    if (!disp || !hit || !code || !has) return t4d_fail(T4D_ERR_ARG, "t4d_disp_quantize: NULL buffer");
    if (!dims_ok(h, w)) return t4d_fail(T4D_ERR_ARG, "t4d_disp_quantize: need 1 <= h, w <= %d, got %d x %d", kMaxDim, h, w);
    if (!(isfinite(dist) && dist > 0.0)) return t4d_fail(T4D_ERR_ARG, "t4d_disp_quantize: dist must be finite and > 0, got %g", dist);
    const int64_t n = (int64_t)h * w;
    hipLaunchKernelGGL(k_disp_quantize, dim3(blocks(n)), dim3(kBlock), 0, (hipStream_t)hip_stream, disp, hit, dist, n, code, has);
    return t4d_launch_status("t4d_disp_quantize");
}

T4D_EXPORT size_t t4d_disp_smooth_scratch_bytes(int32_t h, int32_t w)
{
    if (!dims_ok(h, w)) {
        t4d_fail(T4D_ERR_ARG, "t4d_disp_smooth_scratch_bytes: need 1 <= h, w <= %d, got %d x %d", kMaxDim, h, w);
        return 0;
    }
    return smooth_scratch(h, w);
}

T4D_EXPORT int t4d_disp_smooth(const int32_t *code, const uint8_t *has, const uint8_t *labels, int32_t h, int32_t w, int32_t rounds,
                               int32_t *out, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!code || !has || !labels || !out || !scratch || code == out)
        return t4d_fail(T4D_ERR_ARG, "t4d_disp_smooth: NULL buffer, or input and output are one buffer");
    if (!dims_ok(h, w)) return t4d_fail(T4D_ERR_ARG, "t4d_disp_smooth: need 1 <= h, w <= %d, got %d x %d", kMaxDim, h, w);
    if (rounds < 0 || rounds > kMaxRounds) return t4d_fail(T4D_ERR_ARG, "t4d_disp_smooth: rounds must be in 0..%d, got %d", kMaxRounds, rounds);
    if (scratch_bytes < smooth_scratch(h, w))
        return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_disp_smooth: scratch below t4d_disp_smooth_scratch_bytes(h, w)");
    if (((uintptr_t)scratch & 3) != 0) return t4d_fail(T4D_ERR_ARG, "t4d_disp_smooth: the scratch must be aligned to 4 bytes");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t n = (int64_t)h * w;
    if (rounds == 0) {
        hipLaunchKernelGGL(k_disp_copy, dim3(blocks(n)), dim3(kBlock), 0, stream, code, n, out);
        return t4d_launch_status("t4d_disp_smooth");
    }
    const int tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;
    int32_t *tmp = (int32_t *)scratch;
    const int32_t *src = code;
    for (int r = 0; r < rounds; ++r) {
        int32_t *dst = ((rounds - 1 - r) % 2 == 0) ? out : tmp;           // the last round writes `out`
        hipLaunchKernelGGL(k_disp_smooth, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(kBlock), 0, stream, src, has, labels, (int)h,
                           (int)w, tiles_x, dst);
        src = dst;
    }
    return t4d_launch_status("t4d_disp_smooth");
}

T4D_EXPORT int t4d_disp_normals(const int32_t *code, const uint8_t *has, const uint8_t *labels, const float *pos, int32_t h, int32_t w,
                                double unit, int32_t *normal, void *hip_stream)
{
    if (!code || !has || !labels || !pos || !normal) return t4d_fail(T4D_ERR_ARG, "t4d_disp_normals: NULL buffer");
    if (!dims_ok(h, w)) return t4d_fail(T4D_ERR_ARG, "t4d_disp_normals: need 1 <= h, w <= %d, got %d x %d", kMaxDim, h, w);
    if (!(isfinite(unit) && unit > 0.0)) return t4d_fail(T4D_ERR_ARG, "t4d_disp_normals: unit must be finite and > 0, got %g", unit);
    const int64_t n = (int64_t)h * w;
    hipLaunchKernelGGL(k_disp_normals, dim3(blocks(n)), dim3(kBlock), 0, (hipStream_t)hip_stream, code, has, labels, pos, unit, (int)h,
                       (int)w, normal);
    return t4d_launch_status("t4d_disp_normals");
}
