// t4d_drift.hip — the census block matcher behind topo4d_amd/drift.py: the displacement of every block of frame a's UV texture in
// frame b's.  The rule is stated in include/topo4d_raster.h; everything is integer arithmetic, so the table is a pure function of
// the inputs and does not depend on the launch shape.  tests/drift_ref.py restates the rule in whole-image numpy operations.
//
//  * k_drift_census   one texel per lane, both frames in one launch (blockIdx.y): the 64-bit word of every texel into the scratch.
//                     Bits 0..47 hold the census, bits 48..55 the label and bit 63 says "census-valid"; a texel that is not
//                     census-valid holds kNoA in frame a and kNoB in frame b.  For a pair of words x = Wa ^ Wb, x >> 48 == 0
//                     exactly when both texels are census-valid and carry one label, and popcount(x) is then the pair's cost.
//  * k_drift_match    one block per workgroup.  LDS: the block's B x B words of a, the (B + 2R)^2 window of b round it (texels
//                     outside the image hold kNoB) and (c, n) of the (2R + 1)^2 candidates.  The window's rows are `pitch` words
//                     apart with pitch = B + 2R + ((1 - B) mod 32), so that pitch = 2R + 1 (mod 32): the lanes of a wave hold
//                     consecutive candidates (dy, dx) in row-major order, their words of b are then consecutive modulo 32 words,
//                     and the 32 lanes of a ds_read_b64 group cover the 64 banks once; the word of a is one address for all of
//                     them, a broadcast.  The work is dealt as (candidate, slice of the block's rows) items, so that there are
//                     enough items for 256 lanes at a small radius; the partial sums meet in LDS by integer atomic adds, whose
//                     order does not matter.  Wave 0 then picks the best and the second: every lane scans its share of the
//                     candidates and a butterfly of __shfl_xor takes the minimum under the rule's total order, so the result
//                     does not depend on which lane held which candidate.
//                     Neighbouring blocks overlap by B - S and every workgroup stages and sums its own block: nothing is shared
//                     between workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxDim = 65536;
constexpr int kCensus = 3;                       // the census window reaches this far
constexpr int kMinB = 8, kMaxB = 64, kMaxR = 16;
constexpr int kRowSlices = 8;                    // a candidate's sum is dealt as this many slices of the block's rows
constexpr uint64_t kValid = 1ull << 63, kNoA = 1ull << 62, kNoB = 1ull << 61;

struct CensusFrames {
    const uint8_t *luma[2], *valid[2];
    uint64_t *words[2];
};

__global__ __launch_bounds__(kBlock) void k_drift_census(CensusFrames F, const uint8_t *labels, int h, int w)
{
    const int f = (int)blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)h * w) return;
    const int y = (int)(i / w), x = (int)(i % w);
    const uint8_t *L = F.luma[f], *V = F.valid[f];
    const uint32_t lab = labels[i];
    uint64_t word = f ? kNoB : kNoA;
    if (lab != 0 && y >= kCensus && y < h - kCensus && x >= kCensus && x < w - kCensus) {
        const uint32_t centre = L[i];
        uint64_t bits = 0;
        bool ok = true;
        int k = 0;
        for (int j = -kCensus; j <= kCensus; ++j) {
            const int64_t row = i + (int64_t)j * w;
            for (int d = -kCensus; d <= kCensus; ++d) {
                ok = ok && V[row + d] != 0;
                if (j == 0 && d == 0) continue;
                bits |= (uint64_t)(L[row + d] < centre) << k;
                ++k;
            }
        }
        if (ok) word = kValid | ((uint64_t)lab << 48) | bits;
    }
    F.words[f][i] = word;
}

struct Pick {
    int c, n, idx;                               // n == 0: none
};

// the rule's order; idx = (dy + R) (2R + 1) + (dx + R), so "smaller dy, then smaller dx" is the smaller idx
__device__ inline bool better(const Pick &a, const Pick &b, int R)
{
    if (a.n == 0) return false;
    if (b.n == 0) return true;
    const int64_t l = (int64_t)a.c * b.n, r = (int64_t)b.c * a.n;
    if (l != r) return l < r;
    const int D = 2 * R + 1;
    const int ay = a.idx / D - R, ax = a.idx % D - R, by = b.idx / D - R, bx = b.idx % D - R;
    const int ar = ay * ay + ax * ax, br = by * by + bx * bx;
    if (ar != br) return ar < br;
    return a.idx < b.idx;
}

// wave 0: the first admissible candidate of the order; away_from >= 0: among those farther than 1 (Chebyshev) from that candidate
__device__ inline Pick pick(const int *acc, int R, int min_count, int away_from)
{
    const int D = 2 * R + 1, ncand = D * D;
    const int fy = away_from >= 0 ? away_from / D : 0, fx = away_from >= 0 ? away_from % D : 0;
    Pick mine = {0, 0, 0};
    for (int i = (int)threadIdx.x; i < ncand; i += 64) {
        const int n = acc[2 * i + 1];
        if (n < min_count) continue;
        if (away_from >= 0) {
            const int ey = i / D - fy, ex = i % D - fx;
            if (ey >= -1 && ey <= 1 && ex >= -1 && ex <= 1) continue;
        }
        const Pick p = {acc[2 * i], n, i};
        if (better(p, mine, R)) mine = p;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const Pick o = {__shfl_xor(mine.c, off, 64), __shfl_xor(mine.n, off, 64), __shfl_xor(mine.idx, off, 64)};
        if (better(o, mine, R)) mine = o;
    }
    return mine;
}

__global__ __launch_bounds__(kBlock) void k_drift_match(const uint64_t *wa, const uint64_t *wb, int h, int w, int B, int S, int R,
                                                        int min_count, int nbx, int pitch, int32_t *out)
{
    extern __shared__ uint64_t lds[];
    const int D = 2 * R + 1, ncand = D * D, win = B + 2 * R;
    uint64_t *sa = lds, *sb = lds + B * B;
    int *acc = (int *)(sb + win * pitch);
    const int by = (int)(blockIdx.x / (unsigned)nbx), bx = (int)(blockIdx.x % (unsigned)nbx);
    const int y0 = by * S, x0 = bx * S;
    for (int i = threadIdx.x; i < B * B; i += kBlock) {
        const int y = i / B, x = i % B;
        sa[i] = wa[(int64_t)(y0 + y) * w + (x0 + x)];
    }
    for (int i = threadIdx.x; i < win * win; i += kBlock) {
        const int wy = i / win, wx = i % win;
        const int gy = y0 - R + wy, gx = x0 - R + wx;
        sb[wy * pitch + wx] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? wb[(int64_t)gy * w + gx] : kNoB;
    }
    for (int i = threadIdx.x; i < 2 * ncand; i += kBlock) acc[i] = 0;
    __syncthreads();
    for (int it = threadIdx.x; it < ncand * kRowSlices; it += kBlock) {
        const int slice = it / ncand, cand = it - slice * ncand;
        const int dyi = cand / D, dxi = cand - dyi * D;
        const int r0 = slice * B / kRowSlices, r1 = (slice + 1) * B / kRowSlices;
        int c = 0, n = 0;
        for (int y = r0; y < r1; ++y) {
            const uint64_t *pa = sa + y * B, *pb = sb + (y + dyi) * pitch + dxi;
#pragma unroll 4
            for (int x = 0; x < B; ++x) {
                const uint64_t v = pa[x] ^ pb[x];
                const bool ok = (v >> 48) == 0;
                c += ok ? __popcll(v) : 0;
                n += ok ? 1 : 0;
            }
        }
        if (n) {
            atomicAdd(&acc[2 * cand], c);
            atomicAdd(&acc[2 * cand + 1], n);
        }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const Pick best = pick(acc, R, min_count, -1);
    const Pick second = best.n ? pick(acc, R, min_count, best.idx) : best;
    if (threadIdx.x != 0) return;
    int32_t *o = out + (int64_t)blockIdx.x * 16;
    for (int k = 0; k < 16; ++k) o[k] = 0;
    if (best.n == 0) return;
    const int dyi = best.idx / D, dxi = best.idx % D;
    o[0] = dyi - R;
    o[1] = dxi - R;
    o[2] = best.c;
    o[3] = best.n;
    const int ny[4] = {dyi - 1, dyi + 1, dyi, dyi}, nx[4] = {dxi, dxi, dxi - 1, dxi + 1};
    for (int k = 0; k < 4; ++k) {
        if (ny[k] < 0 || ny[k] >= D || nx[k] < 0 || nx[k] >= D) continue;
        const int i = ny[k] * D + nx[k];
        if (acc[2 * i + 1] < min_count) continue;
        o[4 + 2 * k] = acc[2 * i];
        o[5 + 2 * k] = acc[2 * i + 1];
    }
    o[12] = second.n ? second.c : 0;
    o[13] = second.n;
}

bool dims_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && h <= kMaxDim && w <= kMaxDim; }

bool options_ok(int32_t B, int32_t S, int32_t R)
{
    return B >= kMinB && B <= kMaxB && B % 2 == 0 && S >= 1 && S <= B && R >= 0 && R <= kMaxR;
}

size_t words_bytes(int32_t h, int32_t w) { return align_up((size_t)h * (size_t)w * sizeof(uint64_t)); }

int fail_options(const char *entry, int32_t h, int32_t w, int32_t B, int32_t S, int32_t R)
{
    return t4d_fail(T4D_ERR_ARG,
                    "%s: need 1 <= h, w <= %d, block even in %d..%d, stride in 1..block and radius in 0..%d, got %d x %d, block %d, "
                    "stride %d, radius %d", entry, kMaxDim, kMinB, kMaxB, kMaxR, h, w, B, S, R);
}

}  // namespace

T4D_EXPORT size_t t4d_drift_scratch_bytes(int32_t h, int32_t w, int32_t block, int32_t stride, int32_t radius)
{
    if (!dims_ok(h, w) || !options_ok(block, stride, radius)) {
        fail_options("t4d_drift_scratch_bytes", h, w, block, stride, radius);
        return 0;
    }
    return 2 * words_bytes(h, w);
}

T4D_EXPORT int t4d_drift_match(const uint8_t *luma_a, const uint8_t *valid_a, const uint8_t *luma_b, const uint8_t *valid_b,
                               const uint8_t *labels, int32_t h, int32_t w, int32_t block, int32_t stride, int32_t radius,
                               int32_t min_count, int32_t *out, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!luma_a || !valid_a || !luma_b || !valid_b || !labels || !out || !scratch)
        return t4d_fail(T4D_ERR_ARG, "t4d_drift_match: NULL buffer");
    if (!dims_ok(h, w) || !options_ok(block, stride, radius)) return fail_options("t4d_drift_match", h, w, block, stride, radius);
    if (min_count < 1 || min_count > block * block)
        return t4d_fail(T4D_ERR_ARG, "t4d_drift_match: min_count must be in 1..block^2 = %d, got %d", block * block, min_count);
    if (scratch_bytes < 2 * words_bytes(h, w))
        return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_drift_match: scratch below t4d_drift_scratch_bytes(h, w, block, stride, radius)");
    if (((uintptr_t)scratch & 7) != 0) return t4d_fail(T4D_ERR_ARG, "t4d_drift_match: the scratch must be aligned to 8 bytes");
    if (h < block || w < block) return T4D_OK;                           // no block: nothing to write
    const int nby = (h - block) / stride + 1, nbx = (w - block) / stride + 1;
    if ((int64_t)nby * nbx > 0x7fffffff)
        return t4d_fail(T4D_ERR_ARG, "t4d_drift_match: %d x %d blocks are more than one launch holds (2^31 - 1)", nby, nbx);
    hipStream_t stream = (hipStream_t)hip_stream;
    CensusFrames F;
    F.luma[0] = luma_a, F.luma[1] = luma_b, F.valid[0] = valid_a, F.valid[1] = valid_b;
    F.words[0] = (uint64_t *)scratch;
    F.words[1] = (uint64_t *)((uint8_t *)scratch + words_bytes(h, w));
    const int win = block + 2 * radius, D = 2 * radius + 1;
    const int pitch = win + ((1 - block) % 32 + 32) % 32;
    const size_t lds = ((size_t)block * block + (size_t)win * pitch) * sizeof(uint64_t) + (size_t)2 * D * D * sizeof(int);
    if (lds > 65536)                                                     // before anything is queued: a refusal leaves no launch behind
        T4D_HIP_CHECK(hipFuncSetAttribute((const void *)k_drift_match, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t texels = (int64_t)h * w;
    hipLaunchKernelGGL(k_drift_census, dim3((unsigned)((texels + kBlock - 1) / kBlock), 2), dim3(kBlock), 0, stream, F, labels, h, w);
    hipLaunchKernelGGL(k_drift_match, dim3((unsigned)nby * (unsigned)nbx), dim3(kBlock), lds, stream, F.words[0], F.words[1], h, w, block,
                       stride, radius, min_count, nbx, pitch, out);
    return t4d_launch_status("t4d_drift_match");
}
