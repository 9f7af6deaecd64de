// t4d_tile_div.h - division of a wave-uniform index by a launch constant as a multiply-high and a shift.
//
// The render kernels decode work-item indices with a divisor that is fixed for the launch (tile index / gx, spare workgroup /
// spans, fill workgroup / gy).  The scalar unit has no divide: `t / d` on a scalar value is compiled to a reciprocal on the
// VECTOR unit (v_cvt, v_rcp_iflag_f32, v_mul, v_cvt, v_readfirstlane - hoisted to the workgroup's entry where d is loop-invariant)
// and about fifteen scalar instructions of correction per quotient.  Here the host derives, once per launch, a multiplier and a
// shift (round-up method):
//     m = ceil(2^(32+s) / d),     t / d == (t * m) >> (32 + s)   for every t < limit,
// which the kernels evaluate as ONE scalar multiply-high and a shift.  With e = m d - 2^(32+s) (0 <= e < d) the quotient of
// t = q d + r is exact iff t e < 2^(32+s) in the worst case r = d - 1, so the host takes the largest s whose m fits 32 bits and
// for which (limit - 1) e < 2^(32+s) holds.  For d >= 2 and limit <= 2^31 that always exists (s = ceil(log2 d) - 1: e < d <= 2 2^s),
// and every index the rasterizer divides is below 2^30 (check_problem).  d = 1 has no 32-bit multiplier (m = 2^32) and needs
// none: it is marked by mul == 0 and the quotient is t itself.  Where neither holds - limits beyond 2^31 with awkward divisors -
// t4d_div_make reports failure and the caller must not launch with it.
// Plain C++: included by t4d_raster.hip and by the host test program tests/native/tile_div_host.cpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define T4D_HD __host__ __device__
#else
#define T4D_HD
#endif

struct T4DDiv {
    uint32_t mul;        // 0: the divisor is 1
    uint32_t shift;      // quotient = mulhi(t, mul) >> shift
};

// multiplier and shift for t / d, exact for every t < limit (limit <= 2^32); false: none exists (or d == 0)
inline bool t4d_div_make(const uint32_t d, const uint64_t limit, T4DDiv &r)
{
    r.mul = 0u; r.shift = 0u;
    if (d == 1u) return true;
    if (d == 0u || limit > (1ull << 32)) return false;
    bool found = false;
    const uint64_t tmax = limit ? limit - 1u : 0u;               // < 2^32
    for (uint32_t s = 0; s < 32u; s++) {
        const uint64_t pow = 1ull << (32u + s);                  // <= 2^63
        const uint64_t m = (pow + d - 1u) / d;
        if (m >> 32) break;                                      // m only grows with s: no later s fits either
        const uint64_t e = m * d - pow;                          // < d < 2^32, so tmax * e < 2^64
        if (tmax * e < pow) { r.mul = (uint32_t)m; r.shift = s; found = true; }      // keeps the LARGEST s that fits
    }
    return found;
}

T4D_HD inline uint32_t t4d_div_mulhi(const uint32_t a, const uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// t / d for t below the limit `dv` was made for
T4D_HD inline uint32_t t4d_div(const uint32_t t, const T4DDiv dv) { return dv.mul ? (t4d_div_mulhi(t, dv.mul) >> dv.shift) : t; }
