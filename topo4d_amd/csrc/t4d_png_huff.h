// t4d_png_huff.h — the single-thread part of the PNG encoder's Huffman construction (csrc/t4d_png.hip): length-limited code lengths
// from the sorted leaves, and canonical codes.  __host__ __device__, so that tests/native/png_huff_host.cpp runs the same arithmetic
// on the CPU (under the address and undefined-behaviour sanitizers) on histograms no image of a few segments reaches.  The parallel
// rank computation that fills `sorted` / `w_leaf` / `count` stays in the kernel; the host program does it with a plain loop.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define T4D_PH_HD __host__ __device__ inline
#else
#define T4D_PH_HD inline
#endif

constexpr int kPngLit = 286;                     // literal/length alphabet: the largest alphabet the scratch holds

struct HuffScratch {
    uint16_t sorted[kPngLit];                    // used symbols by (freq, symbol) ascending
    uint32_t w_leaf[kPngLit];                    // their frequencies
    uint32_t bl[32];                             // leaves per code length
    uint32_t next[16];                           // canonical_codes: next code per length
    uint32_t w_int[kPngLit];                     // internal-node weights
    uint16_t par_leaf[kPngLit], par_int[kPngLit];
    uint8_t depth_int[kPngLit];
    int count;
};

T4D_PH_HD int t4d_png_min(int a, int b) { return a < b ? a : b; }

T4D_PH_HD uint32_t t4d_png_brev(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
    return (v >> 16) | (v << 16);
#endif
}

// One thread.  hs.sorted / hs.w_leaf hold the hs.count used symbols by (frequency, symbol) ascending; len[] is zero for every
// unused symbol already.  Huffman depths from the two-queue method (a leaf wins a weight tie against an internal node); leaves
// deeper than max_bits are clamped and the Kraft excess is removed one unit at a time (the deepest non-empty length b < max_bits
// gives one leaf to b + 1, which takes a clamped leaf as its sibling); then the lengths go to the symbols longest first, least
// frequent first.
T4D_PH_HD void t4d_png_huff_assign(int max_bits, uint8_t *len, HuffScratch &hs)
{
    const int m = hs.count;
    int i = 0, j = 0;
    for (int k = 0; k < m - 1; ++k) {
        uint32_t w = 0;
        for (int pick = 0; pick < 2; ++pick) {
            const bool leaf = i < m && (j >= k || hs.w_leaf[i] <= hs.w_int[j]);
            if (leaf) { w += hs.w_leaf[i]; hs.par_leaf[i++] = (uint16_t)k; }
            else { w += hs.w_int[j]; hs.par_int[j++] = (uint16_t)k; }
        }
        hs.w_int[k] = w;
    }
    uint32_t *bl = hs.bl;                                         // LDS: a private array here would live in scratch memory
    for (int b = 0; b < 32; ++b) bl[b] = 0;
    if (m >= 2) {
        hs.depth_int[m - 2] = 0;
        for (int k = m - 3; k >= 0; --k) hs.depth_int[k] = (uint8_t)t4d_png_min(hs.depth_int[hs.par_int[k]] + 1, 31);
        for (int q = 0; q < m; ++q) bl[t4d_png_min(hs.depth_int[hs.par_leaf[q]] + 1, 31)]++;
    } else if (m == 1) {
        bl[1] = 1;
    }
    for (int b = max_bits + 1; b < 32; ++b) { bl[max_bits] += bl[b]; bl[b] = 0; }
    uint64_t kraft = 0;
    for (int b = 1; b <= max_bits; ++b) kraft += (uint64_t)bl[b] << (max_bits - b);
    const uint64_t one = (uint64_t)1 << max_bits;
    while (kraft > one) {
        int b = max_bits - 1;
        while (b > 0 && bl[b] == 0) --b;
        if (b == 0) break;                                        // cannot happen for n <= 2^max_bits
        bl[b]--; bl[b + 1] += 2; bl[max_bits]--;
        kraft -= 1;
    }
    int q = 0;                                                    // least frequent first: the longest lengths
    for (int b = max_bits; b >= 1; --b)
        for (uint32_t k = 0; k < bl[b] && q < m; ++k) len[hs.sorted[q++]] = (uint8_t)b;
}

// canonical codes, bit-reversed for LSB-first output (RFC 1951 3.2.2); one thread
T4D_PH_HD void t4d_png_canonical_codes(const uint8_t *len, int n, uint16_t *code, HuffScratch &hs)
{
    uint32_t *bl = hs.bl, *next = hs.next;
    for (int b = 0; b < 16; ++b) bl[b] = next[b] = 0;
    for (int s = 0; s < n; ++s) bl[len[s]]++;
    bl[0] = 0;
    uint32_t c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + bl[b - 1]) << 1; next[b] = c; }
    for (int s = 0; s < n; ++s) {
        const int l = len[s];
        if (!l) { code[s] = 0; continue; }
        const uint32_t v = next[l]++;
        code[s] = (uint16_t)(t4d_png_brev(v) >> (32 - l));
    }
}
