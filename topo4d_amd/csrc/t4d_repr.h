// t4d_repr.h — Python's repr(float) of a float64, as a device function (and a host one, for the CPU tests).
//
// Digits: the shortest decimal that reads back as the same double, and of those the one closest to it (ties to an even last
// digit) - Ryu (U. Adams, "Ryu: fast float-to-string conversion", PLDI 2018, section 3).  The interval of decimals that round
// to x is [4*m2 - 1 - mm_shift, 4*m2 + 2] * 2^(e2 - 2) (endpoints included when m2 is even: round-half-even on input);
// multiplying its three points by 10^-q, with q just below the number of digits to drop, needs one 64x125-bit product each
// against the tables of t4d_repr_tables.h (tools/gen_repr_tables.py), after which digits are removed while the interval still
// holds two distinct truncations.  The exact-remainder flags (vm/vr "is trailing zeros") are only needed when the product can be
// exact, i.e. q small, and are found by counting factors of 5 or 2 of the integer operand.
//
// Notation: CPython's float_repr_style 'short' (format code 'r'): with decpt the position of the decimal point in
// 0.d1d2...dn x 10^decpt, fixed notation when -4 < decpt <= 16 (an integer value keeps a ".0"), otherwise d1[.d2...dn]e<sign>XX
// with at least two exponent digits.  Specials: "nan" (any sign), "inf", "-inf", "0.0", "-0.0".  At most 24 characters
// ("-1.2345678901234567e-308").
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define T4D_REPR_FN __host__ __device__ static inline
#define T4D_REPR_TABLE static __device__
#else
#define T4D_REPR_FN static inline
#define T4D_REPR_TABLE static
#endif

#include "t4d_repr_tables.h"

#define T4D_REPR_MAX_CHARS 24                   // = T4D_OBJ_FLOAT_CHARS (include/topo4d_raster.h)

namespace t4d_repr {

struct Decimal {
    uint64_t digits;                            // 1..17 decimal digits, no trailing zero unless the value is exact
    int32_t exp10;                              // value = digits * 10^exp10
};

T4D_REPR_FN uint32_t pow5_bits(int32_t e) { return (uint32_t)(((uint32_t)e * 1217359u) >> 19) + 1; }  // ceil(log2(5^e)), 1 at e = 0
T4D_REPR_FN uint32_t log10_pow2(int32_t e) { return ((uint32_t)e * 78913u) >> 18; }                    // floor(e * log10(2))
T4D_REPR_FN uint32_t log10_pow5(int32_t e) { return ((uint32_t)e * 732923u) >> 20; }                   // floor(e * log10(5))

T4D_REPR_FN uint64_t umulh(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// floor(m * mul / 2^j), mul = {lo, hi} a 125-bit integer, m < 2^55, j >= 64 (the result fits 64 bits by the choice of j)
T4D_REPR_FN uint64_t mul_shift(uint64_t m, const uint64_t *mul, int32_t j)
{
    const uint64_t mid = umulh(m, mul[0]);
    const uint64_t lo = m * mul[1];
    const uint64_t hi = umulh(m, mul[1]);
    const uint64_t sum = mid + lo;              // bits 64..127 of the product
    const uint64_t top = hi + (sum < mid);      // bits 128..191
    const int32_t s = j - 64;
    if (s == 0) return sum;
    if (s < 64) return (sum >> s) | (top << (64 - s));
    return top >> (s - 64);
}

T4D_REPR_FN uint32_t pow5_factor(uint64_t v)
{
    uint32_t n = 0;
    while (v != 0 && v % 5 == 0) {
        v /= 5;
        ++n;
    }
    return n;
}

T4D_REPR_FN bool multiple_of_pow5(uint64_t v, uint32_t p) { return pow5_factor(v) >= p; }
T4D_REPR_FN bool multiple_of_pow2(uint64_t v, uint32_t p) { return p >= 64 ? v == 0 : (v & ((1ull << p) - 1)) == 0; }

// the shortest, closest decimal of a finite, non-zero double with raw fields (ieee_m, ieee_e)
T4D_REPR_FN Decimal shortest(uint64_t ieee_m, uint32_t ieee_e)
{
    int32_t e2;
    uint64_t m2;
    if (ieee_e == 0) {
        e2 = 1 - 1023 - 52 - 2;
        m2 = ieee_m;
    } else {
        e2 = (int32_t)ieee_e - 1023 - 52 - 2;
        m2 = (1ull << 52) | ieee_m;
    }
    const bool even = (m2 & 1) == 0;
    const bool accept_bounds = even;
    const uint64_t mv = 4 * m2;                                   // the value, scaled by 4
    const uint32_t mm_shift = (ieee_m != 0 || ieee_e <= 1) ? 1 : 0;  // the gap below is half as wide at a power of two

    uint64_t vr, vp, vm;
    int32_t e10;
    bool vm_tz = false, vr_tz = false;                            // the dropped part of vm / vr is exactly zero
    if (e2 >= 0) {
        const uint32_t q = log10_pow2(e2) - (e2 > 3);
        e10 = (int32_t)q;
        const int32_t k = T4D_REPR_POW5_INV_BITS + (int32_t)pow5_bits((int32_t)q) - 1;
        const int32_t i = -e2 + (int32_t)q + k;
        vr = mul_shift(4 * m2, t4d_pow5_inv[q], i);
        vp = mul_shift(4 * m2 + 2, t4d_pow5_inv[q], i);
        vm = mul_shift(4 * m2 - 1 - mm_shift, t4d_pow5_inv[q], i);
        if (q <= 21) {                                            // only then can 5^q divide one of the three
            if (mv % 5 == 0) vr_tz = multiple_of_pow5(mv, q);
            else if (accept_bounds) vm_tz = multiple_of_pow5(mv - 1 - mm_shift, q);
            else vp -= multiple_of_pow5(mv + 2, q);
        }
    } else {
        const uint32_t q = log10_pow5(-e2) - (-e2 > 1);
        e10 = (int32_t)q + e2;
        const int32_t i = -e2 - (int32_t)q;
        const int32_t k = (int32_t)pow5_bits(i) - T4D_REPR_POW5_BITS;
        const int32_t j = (int32_t)q - k;
        vr = mul_shift(4 * m2, t4d_pow5[i], j);
        vp = mul_shift(4 * m2 + 2, t4d_pow5[i], j);
        vm = mul_shift(4 * m2 - 1 - mm_shift, t4d_pow5[i], j);
        if (q <= 1) {                                             // mv * 5^i / 2^q with q <= 1: every point is exact
            vr_tz = true;
            if (accept_bounds) vm_tz = mm_shift == 1;             // vm = mv - 2 is even, so exact too
            else --vp;                                            // vp = mv + 2 is exact and excluded
        } else if (q < 63) {
            vr_tz = multiple_of_pow2(mv, q);
        }
    }

    int32_t removed = 0;
    uint8_t last = 0;                                             // the last digit dropped from vr
    uint64_t out;
    if (vm_tz || vr_tz) {                                         // the general case (rare)
        while (vp / 10 > vm / 10) {
            vm_tz &= vm % 10 == 0;
            vr_tz &= last == 0;
            last = (uint8_t)(vr % 10);
            vr /= 10;
            vp /= 10;
            vm /= 10;
            ++removed;
        }
        if (vm_tz) {
            while (vm % 10 == 0) {
                vr_tz &= last == 0;
                last = (uint8_t)(vr % 10);
                vr /= 10;
                vp /= 10;
                vm /= 10;
                ++removed;
            }
        }
        if (vr_tz && last == 5 && vr % 2 == 0) last = 4;          // an exact tie: round half to even
        out = vr + ((vr == vm && (!accept_bounds || !vm_tz)) || last >= 5);
    } else {
        bool round_up = false;
        while (vp / 10 > vm / 10) {
            round_up = vr % 10 >= 5;
            vr /= 10;
            vp /= 10;
            vm /= 10;
            ++removed;
        }
        out = vr + (vr == vm || round_up);
    }
    Decimal d;
    d.digits = out;
    d.exp10 = e10 + removed;
    return d;
}

// repr(float(x)) into out[0..23]; returns the number of characters
template <typename Out>
T4D_REPR_FN int format(double x, Out *out)
{
    const uint64_t bits = (uint64_t)__builtin_bit_cast(uint64_t, x);
    const bool neg = (bits >> 63) != 0;
    const uint64_t ieee_m = bits & ((1ull << 52) - 1);
    const uint32_t ieee_e = (uint32_t)((bits >> 52) & 0x7ff);
    int n = 0;
    if (ieee_e == 0x7ff) {
        if (ieee_m != 0) {
            out[0] = 'n'; out[1] = 'a'; out[2] = 'n';
            return 3;
        }
        if (neg) out[n++] = '-';
        out[n++] = 'i'; out[n++] = 'n'; out[n++] = 'f';
        return n;
    }
    if (neg) out[n++] = '-';
    if (ieee_e == 0 && ieee_m == 0) {
        out[n++] = '0'; out[n++] = '.'; out[n++] = '0';
        return n;
    }
    const Decimal d = shortest(ieee_m, ieee_e);
    char dig[17];
    int len = 0;
    for (uint64_t v = d.digits; v != 0; v /= 10) dig[len++] = (char)('0' + v % 10);  // least significant first
    const int decpt = d.exp10 + len;
    if (decpt > -4 && decpt <= 16) {
        if (decpt <= 0) {
            out[n++] = '0';
            out[n++] = '.';
            for (int i = 0; i < -decpt; ++i) out[n++] = '0';
            for (int i = len - 1; i >= 0; --i) out[n++] = dig[i];
        } else if (decpt >= len) {
            for (int i = len - 1; i >= 0; --i) out[n++] = dig[i];
            for (int i = len; i < decpt; ++i) out[n++] = '0';
            out[n++] = '.';
            out[n++] = '0';
        } else {
            for (int i = 0; i < decpt; ++i) out[n++] = dig[len - 1 - i];
            out[n++] = '.';
            for (int i = decpt; i < len; ++i) out[n++] = dig[len - 1 - i];
        }
        return n;
    }
    out[n++] = dig[len - 1];
    if (len > 1) {
        out[n++] = '.';
        for (int i = len - 2; i >= 0; --i) out[n++] = dig[i];
    }
    int e = decpt - 1;
    out[n++] = 'e';
    out[n++] = e < 0 ? '-' : '+';
    if (e < 0) e = -e;
    if (e >= 100) out[n++] = (char)('0' + e / 100);
    out[n++] = (char)('0' + e / 10 % 10);
    out[n++] = (char)('0' + e % 10);
    return n;
}

}  // namespace t4d_repr
