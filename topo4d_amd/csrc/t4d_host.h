// Host-side helpers shared by the library's translation units other than t4d_raster.hip, which owns the error message
// (g_err) and defines t4d_internal_fail.  Nothing here is part of the ABI or runs on the device.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/topo4d_raster.h"

#define T4D_EXPORT extern "C" __attribute__((visibility("default")))

// t4d_raster.hip: stores the message t4d_last_error() returns and gives back `code` (hidden: not exported)
int t4d_internal_fail(int code, const char *fmt, const char *a);

// t4d_internal_fail with a printf-style message (the same 512-byte limit)
__attribute__((format(printf, 2, 3))) static inline int t4d_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return t4d_internal_fail(code, "%s", buf);
}

// the return value of entry point `entry` after its launches: T4D_OK, or T4D_ERR_HIP with "<entry> launch: <HIP error>"
static inline int t4d_launch_status(const char *entry)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? T4D_OK : t4d_fail(T4D_ERR_HIP, "%s launch: %s", entry, hipGetErrorString(e));
}

// return T4D_ERR_HIP with "<call>: <HIP error>" from the enclosing function when a HIP runtime call fails
#define T4D_HIP_CHECK(call)                                                                          \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return t4d_fail(T4D_ERR_HIP, #call ": %s", hipGetErrorString(e_));    \
    } while (0)

// t4d_closest.hip: where a finished closest-point index keeps its primitives (device float64, nine coordinates a b c per
// triangle, or three per point), after one small copy of the index's header to the host; T4D_OK or the refusal of `entry`
int t4d_closest_index_records(const char *entry, const void *index, size_t index_bytes, void *hip_stream, const double **records,
                              int64_t *n_prims, int *is_tri);

// t4d_scan.hip: exclusive scan of `words` int32 from `in` to `out` (in == out allowed), also written to `copy` unless that is
// NULL.  With a zero in the last word of `in`, the last word of `out` holds the total.  `bsum` is scratch of
// t4d_scan_i32_sum_words(words) int32.
constexpr int kScanI32Block = 1024;
static inline int64_t t4d_scan_i32_sum_words(int64_t words) { return (words + kScanI32Block - 1) / kScanI32Block + 1; }
void t4d_scan_i32(const int32_t *in, int32_t *out, int32_t *copy, int32_t *bsum, int64_t words, hipStream_t stream);

// t4d_scan.hip: off[b] = count[0] + ... + count[b - 1] for nb >= 1 bins, saturated at 0xffffffff, and *total = the sum of all
// counts in 64 bits.  `chunk_sum` is scratch of t4d_scan_bins_chunks(nb) uint32.
constexpr int kScanBinsChunk = 1024;
static inline int t4d_scan_bins_chunks(int nb) { return (nb + kScanBinsChunk - 1) / kScanBinsChunk; }
void t4d_scan_bins(const uint32_t *count, int nb, uint32_t *off, uint32_t *chunk_sum, unsigned long long *total, hipStream_t stream);

static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
