// t4d_texfinish.hip — finishing a baked UV texture on the device (topo4d_amd/texfinish.py): coverage from the bake's depth buffer,
// the encoder's quantisation as a kernel of its own, erosion of the coverage, an exact nearest-texel gutter round the UV islands
// and coverage-weighted halving.  The rules are stated in include/topo4d_raster.h; everything after the quantisation is integer
// arithmetic, so every result is a pure function of its inputs and does not depend on the launch shape.
//
//  * k_tf_coverage  depth > -999999 per texel.
//  * k_tf_quantize  t4d_quant_u8 per value (t4d_quant.h: the rule k_png_filter applies to a float32 image).
//  * k_tf_erode     E rounds of "a texel stays if it and its 4-neighbours inside the image are covered" in one launch: in a
//                   rectangle that is "every texel of the image within |dx| + |dy| <= E is covered"; the diamond is read from an
//                   LDS tile with a 4-texel halo (texels outside the image staged as covered).
//  * k_tf_pad_rows  per texel the signed offset to the nearest covered texel of its own row within R (int8; kNone when there is
//                   none; the left one on equal |dx|), from a row segment staged in LDS with an R-texel halo.
//  * k_tf_pad_cols  one 64x64 tile per workgroup, the offset rows [y0 - R, y0 + 64 + R) of its 64 columns in LDS.  An uncovered
//                   texel walks |dy| = 0, 1, ... and keeps the smallest key (d^2, dy, dx) packed into one integer, stopping once
//                   dy^2 exceeds the best d^2; a row's nearest texel (left on ties) is that row's smallest key, so the minimum
//                   over rows is the minimum over the disc.  Then the winner's texel is gathered.  Covered texels copy through.
//  * k_tf_halve     2x2 blocks: per channel (2 s + cnt) / (2 cnt) over the covered texels, 0 when there are none.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"
#include "t4d_quant.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxDim = 65536;                   // h, w: keeps every grid below 2^31 workgroups and every index in int64
constexpr int kMaxErode = 4;
constexpr int kMaxPad = 64;
constexpr int kNone = -128;                      // "no covered texel of this row within R" (offsets span [-64, 64])
constexpr int kTile = 64;                        // k_tf_pad_cols: texels per tile side
constexpr int kErodeW = 64, kErodeH = 16;        // k_tf_erode: tile

__global__ __launch_bounds__(kBlock) void k_tf_coverage(const float *depth, int64_t n, uint8_t *cov)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) cov[i] = depth[i] > -999999.0f ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_tf_quantize(const float *img, int64_t n, uint8_t *out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = (uint8_t)t4d_quant_u8(img[i]);
}

// four values per thread (both pointers 16 / 4-byte aligned, n4 = n / 4); the tail goes through the scalar kernels
__global__ __launch_bounds__(kBlock) void k_tf_coverage4(const float4 *depth, int64_t n4, uchar4 *cov)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n4) return;
    const float4 d = depth[i];
    cov[i] = make_uchar4(d.x > -999999.0f ? 1 : 0, d.y > -999999.0f ? 1 : 0, d.z > -999999.0f ? 1 : 0, d.w > -999999.0f ? 1 : 0);
}

__global__ __launch_bounds__(kBlock) void k_tf_quantize4(const float4 *img, int64_t n4, uchar4 *out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n4) return;
    const float4 v = img[i];
    out[i] = make_uchar4((uint8_t)t4d_quant_u8(v.x), (uint8_t)t4d_quant_u8(v.y), (uint8_t)t4d_quant_u8(v.z), (uint8_t)t4d_quant_u8(v.w));
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

__global__ __launch_bounds__(kBlock) void k_tf_erode(const uint8_t *cov, int h, int w, int rounds, int tiles_x, uint8_t *out)
{
    constexpr int LW = kErodeW + 2 * kMaxErode, LH = kErodeH + 2 * kMaxErode;
    __shared__ uint8_t s[LH * LW];
    const int x0 = (int)(blockIdx.x % tiles_x) * kErodeW, y0 = (int)(blockIdx.x / tiles_x) * kErodeH;
    for (int i = threadIdx.x; i < LH * LW; i += kBlock) {
        const int y = y0 - kMaxErode + i / LW, x = x0 - kMaxErode + i % LW;
        s[i] = (y < 0 || y >= h || x < 0 || x >= w) ? 1 : (cov[(int64_t)y * w + x] != 0 ? 1 : 0);
    }
    __syncthreads();
    const int tx = threadIdx.x % kErodeW, x = x0 + tx;
    if (x >= w) return;
    for (int ty = threadIdx.x / kErodeW; ty < kErodeH; ty += kBlock / kErodeW) {
        const int y = y0 + ty;
        if (y >= h) break;
        int keep = 1;
        for (int dy = -rounds; dy <= rounds; ++dy) {
            const int span = rounds - (dy < 0 ? -dy : dy);
            const uint8_t *row = s + (ty + kMaxErode + dy) * LW + tx + kMaxErode;
            for (int dx = -span; dx <= span; ++dx) keep &= row[dx];
        }
        out[(int64_t)y * w + x] = (uint8_t)keep;
    }
}

__global__ __launch_bounds__(kBlock) void k_tf_pad_rows(const uint8_t *cov, int w, int R, int segs_x, int8_t *off)
{
    __shared__ uint8_t s[kBlock + 2 * kMaxPad];
    const int64_t y = blockIdx.x / segs_x;
    const int x0 = (int)(blockIdx.x % segs_x) * kBlock;
    const uint8_t *row = cov + y * w;
    for (int i = threadIdx.x; i < kBlock + 2 * R; i += kBlock) {
        const int x = x0 - R + i;
        s[i] = (x >= 0 && x < w && row[x] != 0) ? 1 : 0;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    const uint8_t *p = s + threadIdx.x + R;
    int o = kNone;
    if (p[0]) o = 0;
    else
        for (int d = 1; d <= R; ++d) {
            if (p[-d]) { o = -d; break; }                              // the left texel wins on equal |dx|
            if (p[d]) { o = d; break; }
        }
    off[y * w + x] = (int8_t)o;
}

template <int C>
__global__ __launch_bounds__(kBlock) void k_tf_pad_cols(const uint8_t *img, const int8_t *off, int h, int w, int R, int tiles_x,
                                                        uint8_t *out, uint8_t *out_cov)
{
    __shared__ int8_t s[(kTile + 2 * kMaxPad) * kTile];
    const int x0 = (int)(blockIdx.x % tiles_x) * kTile, y0 = (int)(blockIdx.x / tiles_x) * kTile;
    const int rows = kTile + 2 * R;
    for (int i = threadIdx.x; i < rows * kTile; i += kBlock) {
        const int y = y0 - R + i / kTile, x = x0 + i % kTile;
        s[i] = (y >= 0 && y < h && x < w) ? off[(int64_t)y * w + x] : (int8_t)kNone;
    }
    __syncthreads();
    const int tx = threadIdx.x % kTile, x = x0 + tx;
    if (x >= w) return;
    const uint32_t none = (uint32_t)(R * R + 1) << 16;                // above every key of the disc
    for (int ty = threadIdx.x / kTile; ty < kTile; ty += kBlock / kTile) {
        const int y = y0 + ty;
        if (y >= h) break;
        const int8_t *col = s + (ty + R) * kTile + tx;
        const int64_t at = (int64_t)y * w + x;
        if (col[0] == 0) {                                             // covered: copied through
            for (int c = 0; c < C; ++c) out[at * C + c] = img[at * C + c];
            out_cov[at] = 1;
            continue;
        }
        uint32_t best = none;
        for (int k = 0; k <= R; ++k) {
            if ((uint32_t)(k * k) > (best >> 16)) break;              // no texel of these rows can be nearer, nor tie
            for (int sgn = -1; sgn <= (k ? 1 : -1); sgn += 2) {
                const int dy = sgn * k;
                const int o = col[dy * kTile];
                if (o == kNone) continue;
                const uint32_t key = ((uint32_t)(o * o + k * k) << 16) | ((uint32_t)(dy + kMaxPad) << 8) | (uint32_t)(o + kMaxPad);
                best = key < best ? key : best;
            }
        }
        if (best < none) {
            const int dy = (int)((best >> 8) & 0xFFu) - kMaxPad, dx = (int)(best & 0xFFu) - kMaxPad;
            const int64_t from = (int64_t)(y + dy) * w + (x + dx);
            for (int c = 0; c < C; ++c) out[at * C + c] = img[from * C + c];
            out_cov[at] = 1;
        } else {
            for (int c = 0; c < C; ++c) out[at * C + c] = img[at * C + c];
            out_cov[at] = 0;
        }
    }
}

template <int C>
__global__ __launch_bounds__(kBlock) void k_tf_halve(const uint8_t *img, const uint8_t *cov, int h2, int w2, uint8_t *out,
                                                     uint8_t *out_cov)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)h2 * w2) return;
    const int64_t y = i / w2, x = i % w2;
    const int64_t w = 2 * (int64_t)w2;
    uint32_t cnt = 0, sum[C];
    for (int c = 0; c < C; ++c) sum[c] = 0;
    for (int k = 0; k < 4; ++k) {
        const int64_t at = (2 * y + (k >> 1)) * w + 2 * x + (k & 1);
        if (cov[at] == 0) continue;
        ++cnt;
        for (int c = 0; c < C; ++c) sum[c] += img[at * C + c];
    }
    for (int c = 0; c < C; ++c) out[i * C + c] = cnt ? (uint8_t)((2 * sum[c] + cnt) / (2 * cnt)) : 0;   // round half up
    out_cov[i] = cnt ? 1 : 0;
}

bool dims_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= kMaxDim && w <= kMaxDim; }
bool channels_ok(int32_t c) { return c == 1 || c == 3 || c == 4; }

size_t pad_scratch(int32_t h, int32_t w) { return align_up((size_t)h * (size_t)w); }

}  // namespace

T4D_EXPORT int t4d_texture_coverage(const float *depth, int32_t h, int32_t w, uint8_t *coverage, void *hip_stream)
{
    if (!depth || !coverage) return t4d_fail(T4D_ERR_ARG, "t4d_texture_coverage: NULL buffer");
    if (!dims_ok(h, w)) return t4d_fail(T4D_ERR_ARG, "t4d_texture_coverage: need 1 <= h, w <= %d, got %d x %d", kMaxDim, h, w);
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t n = (int64_t)h * w;
    int64_t done = 0;
    if (aligned(depth, 16) && aligned(coverage, 4) && n >= 4) {
        done = n / 4 * 4;
        hipLaunchKernelGGL(k_tf_coverage4, dim3(blocks_for(n / 4)), dim3(kBlock), 0, stream, (const float4 *)depth, n / 4,
                           (uchar4 *)coverage);
    }
    if (done < n)
        hipLaunchKernelGGL(k_tf_coverage, dim3(blocks_for(n - done)), dim3(kBlock), 0, stream, depth + done, n - done, coverage + done);
    return t4d_launch_status("t4d_texture_coverage");
}

T4D_EXPORT int t4d_texture_quantize(const float *image, int32_t h, int32_t w, int32_t c, uint8_t *out, void *hip_stream)
{
    if (!image || !out) return t4d_fail(T4D_ERR_ARG, "t4d_texture_quantize: NULL buffer");
    if (!dims_ok(h, w) || !channels_ok(c))
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_quantize: need 1 <= h, w <= %d and c in {1, 3, 4}, got %d x %d x %d", kMaxDim, h, w, c);
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t n = (int64_t)h * w * c;
    int64_t done = 0;
    if (aligned(image, 16) && aligned(out, 4) && n >= 4) {
        done = n / 4 * 4;
        hipLaunchKernelGGL(k_tf_quantize4, dim3(blocks_for(n / 4)), dim3(kBlock), 0, stream, (const float4 *)image, n / 4, (uchar4 *)out);
    }
    if (done < n)
        hipLaunchKernelGGL(k_tf_quantize, dim3(blocks_for(n - done)), dim3(kBlock), 0, stream, image + done, n - done, out + done);
    return t4d_launch_status("t4d_texture_quantize");
}

T4D_EXPORT int t4d_texture_erode(const uint8_t *coverage, int32_t h, int32_t w, int32_t rounds, uint8_t *out, void *hip_stream)
{
    if (!coverage || !out || coverage == out) return t4d_fail(T4D_ERR_ARG, "t4d_texture_erode: NULL buffer, or input and output are one buffer");
    if (!dims_ok(h, w)) return t4d_fail(T4D_ERR_ARG, "t4d_texture_erode: need 1 <= h, w <= %d, got %d x %d", kMaxDim, h, w);
    if (rounds < 0 || rounds > kMaxErode) return t4d_fail(T4D_ERR_ARG, "t4d_texture_erode: rounds must be in [0, %d], got %d", kMaxErode, rounds);
    const int tiles_x = (w + kErodeW - 1) / kErodeW, tiles_y = (h + kErodeH - 1) / kErodeH;
    hipLaunchKernelGGL(k_tf_erode, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(kBlock), 0, (hipStream_t)hip_stream, coverage, h, w,
                       rounds, tiles_x, out);
    return t4d_launch_status("t4d_texture_erode");
}

T4D_EXPORT size_t t4d_texture_pad_scratch_bytes(int32_t h, int32_t w)
{
    if (!dims_ok(h, w)) {
        t4d_fail(T4D_ERR_ARG, "t4d_texture_pad_scratch_bytes: need 1 <= h, w <= %d, got %d x %d", kMaxDim, h, w);
        return 0;
    }
    return pad_scratch(h, w);
}

T4D_EXPORT int t4d_texture_pad(const uint8_t *image, const uint8_t *coverage, int32_t h, int32_t w, int32_t c, int32_t radius,
                               uint8_t *out_image, uint8_t *out_coverage, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!image || !coverage || !out_image || !out_coverage || !scratch || image == out_image || coverage == out_coverage)
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_pad: NULL buffer, or input and output are one buffer");
    if (!dims_ok(h, w) || !channels_ok(c))
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_pad: need 1 <= h, w <= %d and c in {1, 3, 4}, got %d x %d x %d", kMaxDim, h, w, c);
    if (radius < 0 || radius > kMaxPad) return t4d_fail(T4D_ERR_ARG, "t4d_texture_pad: radius must be in [0, %d], got %d", kMaxPad, radius);
    if (scratch_bytes < pad_scratch(h, w)) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_texture_pad: scratch below t4d_texture_pad_scratch_bytes(h, w)");
    hipStream_t stream = (hipStream_t)hip_stream;
    int8_t *off = (int8_t *)scratch;
    const int segs_x = (w + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_tf_pad_rows, dim3((unsigned)segs_x * (unsigned)h), dim3(kBlock), 0, stream, coverage, w, radius, segs_x, off);
    const int tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y);
    if (c == 1)
        hipLaunchKernelGGL(k_tf_pad_cols<1>, grid, dim3(kBlock), 0, stream, image, off, h, w, radius, tiles_x, out_image, out_coverage);
    else if (c == 3)
        hipLaunchKernelGGL(k_tf_pad_cols<3>, grid, dim3(kBlock), 0, stream, image, off, h, w, radius, tiles_x, out_image, out_coverage);
    else
        hipLaunchKernelGGL(k_tf_pad_cols<4>, grid, dim3(kBlock), 0, stream, image, off, h, w, radius, tiles_x, out_image, out_coverage);
    return t4d_launch_status("t4d_texture_pad");
}

T4D_EXPORT int t4d_texture_halve(const uint8_t *image, const uint8_t *coverage, int32_t h, int32_t w, int32_t c, uint8_t *out_image,
                                 uint8_t *out_coverage, void *hip_stream)
{
    if (!image || !coverage || !out_image || !out_coverage) return t4d_fail(T4D_ERR_ARG, "t4d_texture_halve: NULL buffer");
    if (!dims_ok(h, w) || !channels_ok(c))
        return t4d_fail(T4D_ERR_ARG, "t4d_texture_halve: need 1 <= h, w <= %d and c in {1, 3, 4}, got %d x %d x %d", kMaxDim, h, w, c);
    if ((h & 1) || (w & 1)) return t4d_fail(T4D_ERR_ARG, "t4d_texture_halve: h and w must be even, got %d x %d", h, w);
    hipStream_t stream = (hipStream_t)hip_stream;
    const int h2 = h / 2, w2 = w / 2;
    const dim3 grid(blocks_for((int64_t)h2 * w2));
    if (c == 1) hipLaunchKernelGGL(k_tf_halve<1>, grid, dim3(kBlock), 0, stream, image, coverage, h2, w2, out_image, out_coverage);
    else if (c == 3) hipLaunchKernelGGL(k_tf_halve<3>, grid, dim3(kBlock), 0, stream, image, coverage, h2, w2, out_image, out_coverage);
    else hipLaunchKernelGGL(k_tf_halve<4>, grid, dim3(kBlock), 0, stream, image, coverage, h2, w2, out_image, out_coverage);
    return t4d_launch_status("t4d_texture_halve");
}
