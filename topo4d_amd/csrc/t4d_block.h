// Device-side scans and sums shared by the count -> scan -> fill passes of every translation unit outside the rasterizer (whose
// DPP-tuned forms stay in t4d_raster_*.h) and t4d_photometric.hip.  Wave size 64.  Integer results are exact; the floating-point
// wave_sum adds in the fixed butterfly order 32, 16, ..., 1, which the references of its callers restate.
//
// The workgroup forms (block_exclusive_scan, block_sum) share one contract:
//   - `tmp` points to N entries of LDS;
//   - all N threads of the workgroup call, with blockDim.x == N;
//   - `tmp` may be reused by the caller as soon as the call returns (the call ends on a barrier), and whatever the caller
//     last did with `tmp` must be behind a barrier of its own;
//   - `total` may be null.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

__host__ __device__ inline int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the view that holds block b when view i takes count(views[i]) consecutive blocks, and b's rank inside it; -1 past the last
template <typename V, typename F>
__device__ inline int find_view(const V *views, int n, int64_t b, int64_t *local, F count)
{
    int64_t base = 0;
    for (int i = 0; i < n; i++) {
        const int64_t c = count(views[i]);
        if (b < base + c) {
            *local = b - base;
            return i;
        }
        base += c;
    }
    *local = 0;
    return -1;
}

// the sum of x over the wave's 64 lanes, in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        if constexpr (std::is_integral<T>::value && sizeof(T) == 8) {           // two 32-bit shuffles
            const unsigned long long u = (unsigned long long)x;
            x += (T)(((unsigned long long)(uint32_t)__shfl_xor((int)(u >> 32), d, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)u, d, 64));
        } else if constexpr (std::is_integral<T>::value) {
            x += (T)__shfl_xor((int)x, d, 64);
        } else {
            x += __shfl_xor(x, d, 64);
        }
    }
    return x;
}

// lane l: the sum of x over lanes 0..l
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(x, d, 64);
        if (lane >= d) x += o;
    }
    return x;
}

// thread t: op over the values of threads 0..t-1 (`identity` for thread 0); *total: op over all N (Hillis-Steele in LDS)
template <int N, typename T, typename Op>
__device__ __forceinline__ T block_exclusive_scan(T v, T identity, T *tmp, Op op, T *total)
{
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (int d = 1; d < N; d <<= 1) {
        const T o = t >= d ? tmp[t - d] : identity;
        __syncthreads();
        tmp[t] = op(tmp[t], o);
        __syncthreads();
    }
    const T excl = t > 0 ? tmp[t - 1] : identity;
    if (total) *total = tmp[N - 1];
    __syncthreads();
    return excl;
}

template <int N, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *tmp, T *total)
{
    return block_exclusive_scan<N>(v, (T)0, tmp, [](T a, T b) { return a + b; }, total);
}

// the sum of v over the workgroup's N threads, in every thread (a tree in LDS)
template <int N, typename T>
__device__ __forceinline__ T block_sum(T v, T *tmp)
{
    const int t = threadIdx.x;
    tmp[t] = v;
    __syncthreads();
    for (int st = N / 2; st > 0; st >>= 1) {
        if (t < st) tmp[t] += tmp[t + st];
        __syncthreads();
    }
    const T all = tmp[0];
    __syncthreads();
    return all;
}
