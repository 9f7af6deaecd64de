// The two device-wide exclusive scans of the count -> scan -> fill passes (declared in t4d_host.h; hidden, not part of the ABI).
//
// t4d_scan_i32 (closest-point index, kNN table): int32 words, any count.  Per-workgroup scans of 1024 words, one workgroup over
// the workgroups' sums (1024 a trip, a carry between trips), then each workgroup's offset added.
//
// t4d_scan_bins (texture bake, mesh render): uint32 bin counts, offsets saturated at 0xffffffff and a 64-bit total for the
// host's capacity retry.  One workgroup per chunk of 1024 bins; its wave 0 adds up the totals of the chunks before it.
#include "t4d_block.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 1024;
static_assert(kBlock == kScanI32Block && kBlock == kScanBinsChunk, "t4d_host.h sizes the callers' scratch");

__global__ __launch_bounds__(kBlock) void k_scan_i32_blocks(const int32_t *in, int32_t *out, int32_t *bsum, int64_t words)
{
    __shared__ int32_t s[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t total;
    const int32_t excl = block_exclusive_scan<kBlock>(i < words ? in[i] : 0, s, &total);
    if (i < words) out[i] = excl;
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_scan_i32_sums(int32_t *bsum, int64_t nb)
{
    __shared__ int32_t s[kBlock];
    int32_t carry = 0;
    for (int64_t base = 0; base < nb; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        int32_t total;
        const int32_t excl = block_exclusive_scan<kBlock>(i < nb ? bsum[i] : 0, s, &total);
        if (i < nb) bsum[i] = carry + excl;
        carry += total;
    }
}

__global__ __launch_bounds__(kBlock) void k_scan_i32_add(int32_t *out, int32_t *copy, const int32_t *bsum, int64_t words)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < words) {
        out[i] += bsum[blockIdx.x];
        if (copy) copy[i] = out[i];
    }
}

__global__ __launch_bounds__(kBlock) void k_scan_bins_chunk_sums(const uint32_t *count, int nb, uint32_t *chunk_sum)
{
    __shared__ uint32_t s_w[kBlock / 64];
    const int c = blockIdx.x, tid = threadIdx.x, b = c * kBlock + tid;
    const uint32_t x = wave_sum(b < nb ? count[b] : 0u);
    if ((tid & 63) == 0) s_w[tid >> 6] = x;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) tot += s_w[w];
        chunk_sum[c] = tot;
    }
}

__global__ __launch_bounds__(kBlock) void k_scan_bins(const uint32_t *count, int nb, const uint32_t *chunk_sum, uint32_t *off,
                                                      unsigned long long *total)
{
    __shared__ uint32_t s_w[kBlock / 64];
    __shared__ unsigned long long s_carry;
    const int chunk = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (wave == 0) {                                                // pairs in the chunks before this one
        unsigned long long part = 0;
        for (int i = lane; i < chunk; i += 64) part += chunk_sum[i];
        part = wave_sum(part);
        if (lane == 0) s_carry = part;
    }
    const int b = chunk * kBlock + tid;
    const uint32_t c = b < nb ? count[b] : 0u;
    const uint32_t incl = wave_inclusive_scan(c);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kBlock / 64; k++) {
        const uint32_t x = s_w[k];
        if (k < wave) woff += x;
        tot += x;
    }
    const unsigned long long carry = s_carry;
    const unsigned long long o = carry + woff + incl - c;
    if (b < nb) off[b] = o > 0xffffffffull ? 0xffffffffu : (uint32_t)o;
    if (tid == 0 && chunk == (int)gridDim.x - 1) *total = carry + tot;
}

}  // namespace

void t4d_scan_i32(const int32_t *in, int32_t *out, int32_t *copy, int32_t *bsum, int64_t words, hipStream_t stream)
{
    const unsigned nb = (unsigned)div_up(words, kBlock);
    hipLaunchKernelGGL(k_scan_i32_blocks, dim3(nb), dim3(kBlock), 0, stream, in, out, bsum, words);
    hipLaunchKernelGGL(k_scan_i32_sums, dim3(1), dim3(kBlock), 0, stream, bsum, (int64_t)nb);
    hipLaunchKernelGGL(k_scan_i32_add, dim3(nb), dim3(kBlock), 0, stream, out, copy, bsum, words);
}

void t4d_scan_bins(const uint32_t *count, int nb, uint32_t *off, uint32_t *chunk_sum, unsigned long long *total, hipStream_t stream)
{
    const unsigned chunks = (unsigned)t4d_scan_bins_chunks(nb);
    if (chunks > 1) hipLaunchKernelGGL(k_scan_bins_chunk_sums, dim3(chunks), dim3(kBlock), 0, stream, count, nb, chunk_sum);
    hipLaunchKernelGGL(k_scan_bins, dim3(chunks), dim3(kBlock), 0, stream, count, nb, chunk_sum, off, total);
}
