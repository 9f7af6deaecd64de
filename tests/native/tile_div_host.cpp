// Host build of csrc/t4d_tile_div.h for the CPU tests: the multiplier the host derives for the render kernels' index divisions,
// checked against the plain division.  Prints "ok <checks>" and exits 0, or prints the first failure and exits 1.
#include <stdio.h>

#include "../../topo4d_amd/csrc/t4d_tile_div.h"

static unsigned long long g_checks = 0;

static int fail(const char *what, unsigned long long d, unsigned long long limit, unsigned long long t)
{
    printf("FAIL %s: d=%llu limit=%llu t=%llu\n", what, d, limit, t);
    return 1;
}

static int check_one(const T4DDiv dv, const uint32_t d, const uint64_t limit, const uint32_t t)
{
    const uint32_t q = t4d_div(t, dv);
    g_checks++;
    if (q != t / d || t - q * d != t % d) return fail("quotient", d, limit, t);
    return 0;
}

// the values where a round-up multiplier goes wrong first: the top of the range and the neighbours of the multiples of d below it
static int check_edges(const T4DDiv dv, const uint32_t d, const uint64_t limit)
{
    if (limit == 0) return 0;
    const uint64_t top = limit - 1;
    for (uint64_t k = 0; k < 4; k++) {
        const uint64_t m = (top / d - (top / d >= k ? k : 0)) * d;
        for (int o = -1; o <= 1; o++) {
            const uint64_t t = m + (uint64_t)(int64_t)o;
            if (t <= top && check_one(dv, d, limit, (uint32_t)t)) return 1;
        }
    }
    return check_one(dv, d, limit, (uint32_t)top) || check_one(dv, d, limit, 0u);
}

int main()
{
    T4DDiv dv;
    // tile / gx: every grid width up to 1024, every tile index of up to 1024 rows of tiles (at most 2^20 tiles: check_problem)
    for (uint32_t gx = 1; gx <= 1024; gx++) {
        const uint64_t limit = (uint64_t)gx * 1024 < (1ull << 20) ? (uint64_t)gx * 1024 : (1ull << 20);
        if (!t4d_div_make(gx, limit, dv)) return fail("no multiplier", gx, limit, 0);
        if ((gx == 1) != (dv.mul == 0u)) return fail("mul == 0 must mean d == 1", gx, limit, 0);
        for (uint32_t t = 0; t < (uint32_t)limit; t++)
            if (check_one(dv, gx, limit, t)) return 1;
    }
    // every divisor a launch can have (up to 2^20 tiles per row, spans, rows) over every index it can have (V T <= 2^30): always a
    // multiplier, exact at the edges
    for (uint32_t d = 1; d <= (1u << 20); d++) {
        if (!t4d_div_make(d, 1ull << 31, dv)) return fail("no multiplier below 2^31", d, 1ull << 31, 0);
        if (check_edges(dv, d, 1ull << 31)) return 1;
    }
    // the forward's spreading of F fill workgroups over G workgroups: floor(b F / G) for b = 0 .. G, as the kernel forms it
    const uint32_t shapes[][2] = { { 12288 + 768, 768 }, { 32768 + 3072, 3072 }, { 48128 + 188, 188 }, { 5, 1 }, { 2, 1 }, { 100003, 4095 } };
    for (const auto &sh : shapes) {
        const uint32_t G = sh[0], F = sh[1];
        const uint64_t top = (uint64_t)G * F;
        if (top >= (1ull << 32)) return fail("shape too large for the test", G, top, 0);
        if (!t4d_div_make(G, top + 1, dv)) return fail("no multiplier for a launch shape", G, top + 1, 0);
        for (uint32_t b = 0; b <= G; b++) {
            g_checks++;
            if (t4d_div(b * F, dv) != (uint32_t)(((unsigned long long)b * F) / G)) return fail("fill spreading", G, top + 1, b);
        }
    }
    // a range no 32-bit multiplier serves must be REPORTED: d = 7 over all of 2^32 needs 33 bits; d = 0 is never served; and
    // whatever IS accepted over the full 32-bit range must be exact at its edges
    if (t4d_div_make(7u, 1ull << 32, dv)) return fail("d = 7 over 2^32 accepted", 7, 1ull << 32, 0);
    if (t4d_div_make(0u, 16, dv)) return fail("d = 0 accepted", 0, 16, 0);
    if (t4d_div_make(3u, (1ull << 32) + 1, dv)) return fail("limit beyond 2^32 accepted", 3, (1ull << 32) + 1, 0);
    unsigned refused = 0;
    for (uint32_t d = 1; d <= 4096; d++) {
        if (!t4d_div_make(d, 1ull << 32, dv)) { refused++; continue; }
        if (check_edges(dv, d, 1ull << 32)) return 1;
    }
    if (refused == 0) return fail("nothing refused over 2^32", 0, 1ull << 32, 0);
    printf("ok %llu\n", g_checks);
    return 0;
}
