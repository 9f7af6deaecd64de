// t4d_seqtex.hip — a sequence's stabilised textures fused over time (topo4d_amd/seqtex.py): per texel and channel the sample of
// a given rank among the frames that photographed the texel, and one frame completed from that base.  The rule is stated in
// include/topo4d_raster.h; everything is integer arithmetic, so both results are pure functions of the inputs and do not depend
// on the launch shape.  tests/seqtex_ref.py restates the rule in numpy.
//
//  * k_seqtex_select    streaming, one workgroup per 256 texels of one row, one texel per lane, so no lane divides by the width.
//                       The frame pointers travel as kernel arguments (scalar registers), and the loop over the frames is
//                       uniform and unrolled, so a lane's samples stay in registers, packed four to a dword: CAP / 4 dwords per
//                       channel, and one bit per frame that holds a photograph.  The frames are read in groups of eight under
//                       one uniform branch, so that eight frames' loads are in flight at a time; the host pads the tables to a
//                       multiple of eight with frame 0's pointers, whose validity the kernel masks.  The copies are C bytes and
//                       1 byte wide, which the hardware takes at any address: no input alignment is assumed.  The rank comes
//                       from an 8-step radix select from the top bit.  Channel by channel the packed samples are first turned
//                       into eight bit planes (an 8 x 8 bit transpose per eight frames, then 4 x 4 byte transposes with
//                       v_perm_b32: about 30 vector instructions per eight frames), so that a step of the select is a handful
//                       of instructions on a 64-bit mask: the candidates whose bit is 0 are cand & ~plane, their number is a
//                       population count, and one side is kept.  Selecting on the packed bytes themselves, five instructions
//                       per dword, bit and channel (1920 per texel at 64 frames and three channels), measured 1.5 times this
//                       kernel's time at 64 frames.  CAP in (8, 16, 32, 64), so that a short sequence does not pay for 64.
//  * k_seqtex_complete  elementwise, the same launch shape.
//  Both stage the workgroup's output bytes in LDS and store whole dwords when the width is a multiple of 4 (every row of the
//  outputs then starts on a dword), and bytes otherwise, as k_drift_warp does.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxDim = 65536;
constexpr int kGroup = 8;                                      // frames read under one uniform branch
static_assert(T4D_SEQTEX_MAX_FRAMES == 64 && T4D_SEQTEX_MAX_FRAMES % kGroup == 0, "the largest capacity is 64 frames, whole groups");

template <int CAP>
struct Frames {
    const uint8_t *image[CAP];
    const uint8_t *valid[CAP];
};

// (hi : lo) as an 8 x 8 bit matrix, byte i = row i: transposed in place, so that bit i of byte j is what bit j of byte i was
// (three rounds of swaps of 1 x 1, 2 x 2 and 4 x 4 blocks; the first two stay inside a dword)
__device__ inline void transpose_bits(uint32_t &lo, uint32_t &hi)
{
    uint32_t t;
    t = (lo ^ (lo >> 7)) & 0x00AA00AAu, lo ^= t ^ (t << 7);
    t = (hi ^ (hi >> 7)) & 0x00AA00AAu, hi ^= t ^ (t << 7);
    t = (lo ^ (lo >> 14)) & 0x0000CCCCu, lo ^= t ^ (t << 14);
    t = (hi ^ (hi >> 14)) & 0x0000CCCCu, hi ^= t ^ (t << 14);
    t = (lo ^ (hi << 4)) & 0xF0F0F0F0u, lo ^= t, hi ^= t >> 4;
}

// four dwords as a 4 x 4 byte matrix, transposed in place: afterwards `a` holds the bytes 0 of a, b, c, d in that order, `b` the
// bytes 1, and so on.  v_perm_b32 picks byte k of its result from the eight bytes (second operand: 0..3, first operand: 4..7).
__device__ inline void transpose_bytes(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d)
{
    const uint32_t u0 = __builtin_amdgcn_perm(b, a, 0x05010400u), u1 = __builtin_amdgcn_perm(b, a, 0x07030602u);
    const uint32_t v0 = __builtin_amdgcn_perm(d, c, 0x05010400u), v1 = __builtin_amdgcn_perm(d, c, 0x07030602u);
    a = __builtin_amdgcn_perm(v0, u0, 0x05040100u), b = __builtin_amdgcn_perm(v0, u0, 0x07060302u);
    c = __builtin_amdgcn_perm(v1, u1, 0x05040100u), d = __builtin_amdgcn_perm(v1, u1, 0x07060302u);
}

// the workgroup's n texels (C bytes each in `bytes`, one in `flags`) from LDS to the two outputs, whose first texel is `first`
template <int C, bool Wide>
__device__ inline void store_staged(const uint32_t *s_bytes, const uint32_t *s_flags, int n, int64_t first, uint8_t *out, uint8_t *out_flag)
{
    if (Wide) {                                                // n and first are multiples of 4
        for (int k = threadIdx.x; 4 * k < n * C; k += kBlock) reinterpret_cast<uint32_t *>(out + first * C)[k] = s_bytes[k];
        if (4 * (int)threadIdx.x < n) reinterpret_cast<uint32_t *>(out_flag + first)[threadIdx.x] = s_flags[threadIdx.x];
    } else {
        const uint8_t *sb = reinterpret_cast<const uint8_t *>(s_bytes), *sf = reinterpret_cast<const uint8_t *>(s_flags);
        for (int k = threadIdx.x; k < n * C; k += kBlock) out[first * C + k] = sb[k];
        if ((int)threadIdx.x < n) out_flag[first + threadIdx.x] = sf[threadIdx.x];
    }
}

template <int CAP, int C, bool Wide>
__global__ __launch_bounds__(kBlock) void k_seqtex_select(Frames<CAP> f, int n_frames, int W, uint32_t num, uint32_t den, uint8_t *out,
                                                          uint8_t *out_count)
{
    constexpr int D = CAP / 4;                                 // dwords of packed samples per channel
    constexpr int NW = CAP > 32 ? 2 : 1;                       // dwords of a mask over the frames
    __shared__ uint32_t s_out[kBlock * C / 4], s_count[kBlock / 4];
    uint8_t *so = reinterpret_cast<uint8_t *>(s_out), *sc = reinterpret_cast<uint8_t *>(s_count);
    const int y = (int)blockIdx.x, x0 = (int)blockIdx.y * kBlock, x = x0 + (int)threadIdx.x;
    const int64_t first = (int64_t)y * W + x0;                 // the workgroup's first texel
    uint32_t smp[C][D], held[NW];                              // held: bit t % 32 of word t / 32 says that frame t holds the texel
#pragma unroll
    for (int j = 0; j < D; ++j) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) smp[ch][j] = 0;
    }
#pragma unroll
    for (int w = 0; w < NW; ++w) held[w] = 0;
    if (x < W) {
        const int64_t i = first + threadIdx.x;
#pragma unroll
        for (int g = 0; g < CAP; g += kGroup) {
            if (g < n_frames) {                                // uniform: the tables are padded to whole groups
#pragma unroll
                for (int t = g; t < g + kGroup; ++t) {
                    uint8_t px[C];
                    __builtin_memcpy(px, f.image[t] + i * C, C);
                    const uint32_t v = (f.valid[t][i] != 0 && t < n_frames) ? 1u : 0u;
                    held[t / 32] |= v << (t % 32);
#pragma unroll
                    for (int ch = 0; ch < C; ++ch) smp[ch][t / 4] |= (uint32_t)px[ch] << (8 * (t % 4));
                }
            }
        }
    }
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) n += __popc(held[w]);
    const uint32_t k0 = n ? ((n - 1) * num) / den : 0;         // n - 1 <= 63 and num <= 64
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        // the channel's samples as bit planes: bit t % 32 of plane[b][t / 32] is bit b of frame t's sample.  A group of eight
        // frames (two dwords) is an 8 x 8 bit matrix, frame by bit; transposed, its byte b holds bit b of the eight frames, and
        // a 4 x 4 byte transpose over four groups puts the bytes b of 32 frames into one dword.
        uint32_t plane[8][NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            uint32_t lo[4], hi[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int g = 4 * w + q;
                lo[q] = hi[q] = 0;
                if (g < CAP / 8) {                             // a constant once unrolled; the index is clamped for the compiler
                    lo[q] = smp[ch][2 * (g % (CAP / 8))], hi[q] = smp[ch][2 * (g % (CAP / 8)) + 1];
                    transpose_bits(lo[q], hi[q]);
                }
            }
            transpose_bytes(lo[0], lo[1], lo[2], lo[3]);
            transpose_bytes(hi[0], hi[1], hi[2], hi[3]);
#pragma unroll
            for (int q = 0; q < 4; ++q) plane[q][w] = lo[q], plane[4 + q][w] = hi[q];
        }
        uint32_t cand[NW], k = k0, res = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) cand[w] = held[w];
#pragma unroll
        for (int b = 7; b >= 0; --b) {
            uint32_t z[NW], zeros = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {                     // the candidates whose bit b is 0
                z[w] = cand[w] & ~plane[b][w];
                zeros += __popc(z[w]);
            }
            const bool low = k < zeros;                        // the rank lies among them
#pragma unroll
            for (int w = 0; w < NW; ++w) cand[w] = low ? z[w] : cand[w] ^ z[w];
            if (!low) {
                k -= zeros;
                res |= 1u << b;
            }
        }
        so[threadIdx.x * C + ch] = n ? (uint8_t)res : 0;
    }
    sc[threadIdx.x] = (uint8_t)n;
    __syncthreads();
    store_staged<C, Wide>(s_out, s_count, min(kBlock, W - x0), first, out, out_count);
}

template <int C, bool Wide>
__global__ __launch_bounds__(kBlock) void k_seqtex_complete(const uint8_t *image, const uint8_t *valid, const uint8_t *base, const uint8_t *count,
                                                            int W, int min_count, int min_votes, int tol, uint8_t *out, uint8_t *out_source)
{
    __shared__ uint32_t s_out[kBlock * C / 4], s_source[kBlock / 4];
    uint8_t *so = reinterpret_cast<uint8_t *>(s_out), *ss = reinterpret_cast<uint8_t *>(s_source);
    const int y = (int)blockIdx.x, x0 = (int)blockIdx.y * kBlock, x = x0 + (int)threadIdx.x;
    const int64_t first = (int64_t)y * W + x0;
    uint8_t px[C], bs[C];
    for (int ch = 0; ch < C; ++ch) px[ch] = bs[ch] = 0;
    int source = 0;
    if (x < W) {
        const int64_t i = first + threadIdx.x;
        __builtin_memcpy(px, image + i * C, C);
        __builtin_memcpy(bs, base + i * C, C);
        const bool v = valid[i] != 0;
        const int n = count[i];
        int far = 0;
        for (int ch = 0; ch < C; ++ch) far = max(far, abs((int)px[ch] - (int)bs[ch]));
        const bool outlier = v && n >= min_votes && far > tol;
        if (v && !outlier)
            source = 1;
        else if (n >= min_count)
            source = v ? 3 : 2;
    }
    for (int ch = 0; ch < C; ++ch) so[threadIdx.x * C + ch] = source == 1 ? px[ch] : source ? bs[ch] : 0;
    ss[threadIdx.x] = (uint8_t)source;
    __syncthreads();
    store_staged<C, Wide>(s_out, s_source, min(kBlock, W - x0), first, out, out_source);
}

template <int CAP, int C>
void launch_select(hipStream_t stream, const uint8_t *const *images, const uint8_t *const *valids, int n_frames, int h, int w, int num, int den,
                   uint8_t *out, uint8_t *out_count)
{
    Frames<CAP> f;
    for (int t = 0; t < CAP; ++t) {                            // beyond n_frames: frame 0's, read in the last group and masked
        f.image[t] = images[t < n_frames ? t : 0];
        f.valid[t] = valids[t < n_frames ? t : 0];
    }
    const dim3 grid((unsigned)h, (unsigned)((w + kBlock - 1) / kBlock));
    if (w % 4 == 0)
        hipLaunchKernelGGL((k_seqtex_select<CAP, C, true>), grid, dim3(kBlock), 0, stream, f, n_frames, w, (uint32_t)num, (uint32_t)den, out,
                           out_count);
    else
        hipLaunchKernelGGL((k_seqtex_select<CAP, C, false>), grid, dim3(kBlock), 0, stream, f, n_frames, w, (uint32_t)num, (uint32_t)den, out,
                           out_count);
}

template <int C>
void launch_select_frames(hipStream_t stream, const uint8_t *const *images, const uint8_t *const *valids, int n_frames, int h, int w, int num,
                          int den, uint8_t *out, uint8_t *out_count)
{
    if (n_frames <= 8)
        launch_select<8, C>(stream, images, valids, n_frames, h, w, num, den, out, out_count);
    else if (n_frames <= 16)
        launch_select<16, C>(stream, images, valids, n_frames, h, w, num, den, out, out_count);
    else if (n_frames <= 32)
        launch_select<32, C>(stream, images, valids, n_frames, h, w, num, den, out, out_count);
    else
        launch_select<64, C>(stream, images, valids, n_frames, h, w, num, den, out, out_count);
}

template <int C>
void launch_complete(hipStream_t stream, const uint8_t *image, const uint8_t *valid, const uint8_t *base, const uint8_t *count, int h, int w,
                     int min_count, int min_votes, int tol, uint8_t *out, uint8_t *out_source)
{
    const dim3 grid((unsigned)h, (unsigned)((w + kBlock - 1) / kBlock));
    if (w % 4 == 0)
        hipLaunchKernelGGL((k_seqtex_complete<C, true>), grid, dim3(kBlock), 0, stream, image, valid, base, count, w, min_count, min_votes, tol,
                           out, out_source);
    else
        hipLaunchKernelGGL((k_seqtex_complete<C, false>), grid, dim3(kBlock), 0, stream, image, valid, base, count, w, min_count, min_votes, tol,
                           out, out_source);
}

bool shape_ok(int32_t h, int32_t w, int32_t c) { return h >= 1 && w >= 1 && h <= kMaxDim && w <= kMaxDim && (c == 1 || c == 3 || c == 4); }

}  // namespace

T4D_EXPORT int t4d_seqtex_select(const uint8_t *const *images, const uint8_t *const *valids, int32_t n_frames, int32_t h, int32_t w, int32_t c,
                                 int32_t num, int32_t den, uint8_t *out_image, uint8_t *out_count, void *hip_stream)
{
    if (!images || !valids || !out_image || !out_count) return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_select: NULL buffer");
    if (n_frames < 1 || n_frames > T4D_SEQTEX_MAX_FRAMES || !shape_ok(h, w, c) || den < 1 || den > T4D_SEQTEX_MAX_FRAMES || num < 0 || num > den)
        return t4d_fail(T4D_ERR_ARG,
                        "t4d_seqtex_select: need 1 <= n_frames <= %d, 1 <= h, w <= %d, c in (1, 3, 4) and 0 <= num <= den with den in "
                        "1..%d, got %d frames of %d x %d x %d, quantile %d / %d", T4D_SEQTEX_MAX_FRAMES, kMaxDim, T4D_SEQTEX_MAX_FRAMES,
                        n_frames, h, w, c, num, den);
    if (((uintptr_t)out_image & 3) != 0 || ((uintptr_t)out_count & 3) != 0)
        return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_select: out_image and out_count must be aligned to 4 bytes");
    if (out_image == out_count) return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_select: out_image and out_count must be two buffers");
    for (int t = 0; t < n_frames; ++t) {
        if (!images[t] || !valids[t]) return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_select: NULL entry %d of images or valids", t);
        if (images[t] == out_image || images[t] == out_count || valids[t] == out_image || valids[t] == out_count)
            return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_select: the outputs must not be inputs (frame %d)", t);
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    if (c == 1)
        launch_select_frames<1>(stream, images, valids, n_frames, h, w, num, den, out_image, out_count);
    else if (c == 3)
        launch_select_frames<3>(stream, images, valids, n_frames, h, w, num, den, out_image, out_count);
    else
        launch_select_frames<4>(stream, images, valids, n_frames, h, w, num, den, out_image, out_count);
    return t4d_launch_status("t4d_seqtex_select");
}

T4D_EXPORT int t4d_seqtex_complete(const uint8_t *image, const uint8_t *valid, const uint8_t *base, const uint8_t *count, int32_t h, int32_t w,
                                   int32_t c, int32_t min_count, int32_t min_votes, int32_t tol, uint8_t *out_image, uint8_t *out_source,
                                   void *hip_stream)
{
    if (!image || !valid || !base || !count || !out_image || !out_source) return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_complete: NULL buffer");
    if (!shape_ok(h, w, c) || min_count < 1 || min_count > T4D_SEQTEX_MAX_FRAMES || min_votes < 1 || min_votes > T4D_SEQTEX_MAX_FRAMES ||
        tol < 0 || tol > 255)
        return t4d_fail(T4D_ERR_ARG,
                        "t4d_seqtex_complete: need 1 <= h, w <= %d, c in (1, 3, 4), min_count and min_votes in 1..%d and tol in 0..255, got "
                        "%d x %d x %d, min_count %d, min_votes %d, tol %d", kMaxDim, T4D_SEQTEX_MAX_FRAMES, h, w, c, min_count, min_votes, tol);
    if (((uintptr_t)out_image & 3) != 0 || ((uintptr_t)out_source & 3) != 0)
        return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_complete: out_image and out_source must be aligned to 4 bytes");
    const uint8_t *inputs[4] = {image, valid, base, count};
    for (const uint8_t *p : inputs)
        if (p == out_image || p == out_source) return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_complete: the outputs must not be inputs");
    if (out_image == out_source) return t4d_fail(T4D_ERR_ARG, "t4d_seqtex_complete: out_image and out_source must be two buffers");
    hipStream_t stream = (hipStream_t)hip_stream;
    if (c == 1)
        launch_complete<1>(stream, image, valid, base, count, h, w, min_count, min_votes, tol, out_image, out_source);
    else if (c == 3)
        launch_complete<3>(stream, image, valid, base, count, h, w, min_count, min_votes, tol, out_image, out_source);
    else
        launch_complete<4>(stream, image, valid, base, count, h, w, min_count, min_votes, tol, out_image, out_source);
    return t4d_launch_status("t4d_seqtex_complete");
}
