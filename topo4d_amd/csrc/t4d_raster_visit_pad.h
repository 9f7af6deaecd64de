// t4d_raster_visit_pad.h - where the wave-wide stores of a visit-list prefill go.
//
// A wave of a render kernel keeps four row lists in one contiguous LDS block of BYTES bytes.  Before the lists are built the block
// is filled with the null entry by wave-wide stores of VEC bytes per lane (prefill_visit_lists, t4d_raster_render_fwd.h), so that
// every row reads null wherever no entry is written - what used to be padded row by row.  Store k covers the bytes
// [k 64 VEC, (k + 1) 64 VEC) of the block; the last store of a block that is no multiple of 64 VEC bytes is moved back so that it
// ends with the block (it overlaps the store before it: same value), and a block shorter than one store takes a single store by
// its first BYTES / VEC lanes.  Nothing is written outside [0, BYTES).
// Plain C++: included by t4d_raster.hip and by the host test program tests/native/visit_pad_host.cpp.
#pragma once

#ifndef T4D_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define T4D_HD __host__ __device__
#else
#define T4D_HD
#endif
#endif

template <int BYTES, int VEC>
T4D_HD constexpr int visit_prefill_stores()
{
    static_assert(VEC > 0 && BYTES > 0 && BYTES % VEC == 0, "the block is a whole number of stores per lane");
    return (BYTES + 64 * VEC - 1) / (64 * VEC);
}

// does `lane` take part in store k of the prefill, and at which byte offset of the block?
template <int BYTES, int VEC>
T4D_HD constexpr bool visit_prefill_store(const int k, const int lane, int &offset)
{
    constexpr int kStore = 64 * VEC;
    if (BYTES < kStore) {
        offset = lane * VEC;
        return lane < BYTES / VEC;
    }
    offset = ((k + 1) * kStore <= BYTES ? k * kStore : BYTES - kStore) + lane * VEC;
    return true;
}
