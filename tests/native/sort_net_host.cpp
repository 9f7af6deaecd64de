// Host model of the one-wave bin sort (csrc/t4d_raster_sort_net.h): 64 lanes of K keys each, K = 1, 2, 4, 8, run through the
// header's stage list exactly as sort_bin_wave unrolls it (in-lane stages on a lane's own keys, cross-lane stages against the
// lane at the stage's lane distance, the header's direction rule) and compared with std::sort.  Also: the plans of the launch
// shapes that run the 256-thread sorter sort their short bins one per wave, T4D_NO_WAVE_SORT restores the old path and changes
// nothing else, and no other shape's plan knows of it (csrc/t4d_raster_plan.h).
// Prints "ok <checks>" and exits 0, or prints every failure and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../topo4d_amd/csrc/t4d_raster_plan.h"
#include "../../topo4d_amd/csrc/t4d_raster_sort_net.h"

namespace sn = t4d_sort_net;
typedef unsigned long long u64;

static unsigned long long g_checks = 0;
static int g_failed = 0;

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        g_checks++;                                                                       \
        if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); g_failed++; }      \
    } while (0)

// the kernel's sort_bin_wave<K>: lane l holds keys[l K ... l K + K), +inf beyond n
template <int K>
static std::vector<u64> model_sort(const std::vector<u64> &in)
{
    const uint32_t n = (uint32_t)in.size();
    u64 key[sn::kLanes][K];
    for (int lane = 0; lane < sn::kLanes; lane++)
        for (int e = 0; e < K; e++) {
            const uint32_t i = (uint32_t)lane * K + e;
            key[lane][e] = i < n ? in[i] : ~0ull;
        }
    for (int s = 0; s < sn::stage_count(sn::elements(K)); s++) {
        const sn::Stage st = sn::stage_at(s);
        if (sn::in_lane(st, K)) {
            for (int lane = 0; lane < sn::kLanes; lane++)
                for (int e = 0; e < K; e++) {
                    if ((e & st.j) != 0) continue;
                    const u64 a = key[lane][e], b = key[lane][e | st.j];
                    const bool swap = (b < a) == sn::keeps_min(st, K, lane, e);
                    key[lane][e] = swap ? b : a;
                    key[lane][e | st.j] = swap ? a : b;
                }
        } else {
            const int J = sn::lane_distance(st, K);
            u64 next[sn::kLanes][K];
            for (int lane = 0; lane < sn::kLanes; lane++) {
                const bool keep_min = sn::keeps_min(st, K, lane, 0);
                for (int e = 0; e < K; e++) {
                    // (the direction is the same for all keys of a lane: the kernel computes it once)
                    if (sn::keeps_min(st, K, lane, e) != keep_min) { printf("FAIL: direction differs inside a lane\n"); g_failed++; }
                    const u64 other = key[lane ^ J][e];
                    next[lane][e] = ((other < key[lane][e]) == keep_min) ? other : key[lane][e];
                }
            }
            memcpy(key, next, sizeof(key));
        }
    }
    std::vector<u64> out(n);
    for (int lane = 0; lane < sn::kLanes; lane++)
        for (int e = 0; e < K; e++) {
            const uint32_t i = (uint32_t)lane * K + e;
            if (i < n) out[i] = key[lane][e];
            else CHECK(key[lane][e] == ~0ull);          // the padding stays behind every real key
        }
    return out;
}

template <int K>
static void check_input(const std::vector<u64> &in)
{
    std::vector<u64> want = in;
    std::sort(want.begin(), want.end());
    const std::vector<u64> got = model_sort<K>(in);
    g_checks++;
    if (got != want) { printf("FAIL: K = %d, n = %zu: not sorted\n", K, in.size()); g_failed++; }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static u64 make_key(const uint32_t depth_bits, const uint32_t index) { return ((u64)depth_bits << 32) | index; }

template <int K>
static void check_K()
{
    const uint32_t N = 64 * K;
    const uint32_t lens[] = { 1, 2, N / 2, N / 2 + 1, N - 1, N };
    for (const uint32_t n : lens) {
        if (n == 0) continue;
        std::vector<u64> v(n);
        for (uint32_t i = 0; i < n; i++) v[i] = make_key(0x3f000000u + 7u * i, i);                    // sorted
        check_input<K>(v);
        std::reverse(v.begin(), v.end());                                                              // reversed
        check_input<K>(v);
        for (uint32_t i = 0; i < n; i++) v[i] = make_key(0x3f800000u, (uint32_t)((i * 2654435761u) % 100003u));   // one depth: the index word orders
        check_input<K>(v);
        for (uint32_t i = 0; i < n; i++) v[i] = make_key(0x3f000000u + (uint32_t)(rnd() % 5u), (uint32_t)(rnd() % 9u));   // runs of duplicates
        check_input<K>(v);
        for (uint32_t i = 0; i < n; i++) v[i] = make_key(0x3f000000u + (uint32_t)((n - i) / 7u), n - i);          // groups of equal depth, descending
        check_input<K>(v);
    }
    for (int t = 0; t < 3000; t++) {
        const uint32_t n = 1u + (uint32_t)(rnd() % N);
        std::vector<u64> v(n);
        const int kind = t % 3;
        for (uint32_t i = 0; i < n; i++)
            v[i] = kind == 0 ? (rnd() >> 1) : kind == 1 ? make_key((uint32_t)(rnd() % 16u), (uint32_t)(rnd() % 64u)) : make_key((uint32_t)rnd(), i);
        check_input<K>(v);
    }
}

static void check_header()
{
    CHECK(sn::stage_count(64) == 21 && sn::stage_count(128) == 28 && sn::stage_count(256) == 36 && sn::stage_count(512) == 45);
    CHECK(sn::in_lane_stages(1) == 0 && sn::in_lane_stages(2) == 7 && sn::in_lane_stages(4) == 15 && sn::in_lane_stages(8) == 24);
    for (int K = 1; K <= 8; K *= 2) {
        int cross = 0;
        for (int s = 0; s < sn::stage_count(64 * K); s++) {
            const sn::Stage st = sn::stage_at(s);
            CHECK(st.j >= 1 && st.j < st.k && st.k <= 64 * K && (st.k & (st.k - 1)) == 0 && (st.j & (st.j - 1)) == 0);
            if (!sn::in_lane(st, K)) { cross++; CHECK(sn::lane_distance(st, K) >= 1 && sn::lane_distance(st, K) <= 32); }
        }
        CHECK(cross == 21);                                      // every K pays the 21 cross-lane stages of wave_sort64, per key
    }
    CHECK(sn::keys_per_lane(1) == 1 && sn::keys_per_lane(64) == 1 && sn::keys_per_lane(65) == 2 && sn::keys_per_lane(128) == 2);
    CHECK(sn::keys_per_lane(129) == 4 && sn::keys_per_lane(256) == 4 && sn::keys_per_lane(257) == 8 && sn::keys_per_lane(511) == 8);
}

// the plans: who takes the wave sort
static T4DProblem problem(const int P, const int W, const int H, const int V, const uint32_t flags)
{
    T4DProblem p;
    memset(&p, 0, sizeof(p));
    p.P = P; p.W = W; p.H = H; p.n_views = V; p.flags = flags;
    p.pair_capacity = 1 << 20;
    return p;
}

static void check_plans()
{
    const DeviceFacts dev = { 256, 0u };
    Overrides ov, off;
    off.no_wave_sort = true;
    setenv("T4D_NO_WAVE_SORT", "1", 1);
    CHECK(read_overrides().no_wave_sort);
    unsetenv("T4D_NO_WAVE_SORT");
    CHECK(!read_overrides().no_wave_sort);
    // BASELINE config 2 and config 4: the 256-thread sorter, so the wave sort in front of it
    const T4DProblem shapes[] = { problem(30000, 512, 512, 24, T4D_FLAG_NO_LONG_BINS), problem(120000, 2048, 2048, 24, T4D_FLAG_NO_LONG_BINS),
                                  problem(30000, 512, 512, 24, 0) };
    for (const T4DProblem &p : shapes) {
        const ForwardPlan f = plan_forward(p, dev, ov, true), g = plan_forward(p, dev, off, true);
        const int n_tiles = f.regime.T * p.n_views;
        CHECK(f.sorter == Sorter::Block256 && f.wave_bins);
        // the override restores the old sort and touches nothing else: same launch, same grid
        CHECK(g.sorter == Sorter::Block256 && !g.wave_bins && g.sort_grid == f.sort_grid && g.sort_grid == (unsigned)tile_grid(n_tiles, 5, 2, dev, ov));
        CHECK(memcmp(&g.regime, &f.regime, sizeof(Regime)) == 0 && g.tile_blocks == f.tile_blocks && g.fused_sort == f.fused_sort &&
              g.long_bins == f.long_bins && g.long_bins_grid == f.long_bins_grid && g.fill_blocks == f.fill_blocks &&
              build_key(g.render) == build_key(f.render));
    }
    // a small launch on the 256-thread sorter (the caller's word that the bins are short; T4D_SORT_256): the same
    {
        const ForwardPlan f = plan_forward(problem(8280, 512, 375, 4, T4D_FLAG_NO_LONG_BINS | T4D_FLAG_SHORT_BINS), dev, ov, true);
        CHECK(f.sorter != Sorter::Block1024);
        CHECK((f.sorter == Sorter::Block256) == f.wave_bins);
        Overrides s256; s256.sort_256 = true; s256.has_latency_tiles = true; s256.latency_tiles = 0;
        const ForwardPlan h = plan_forward(problem(600, 64, 64, 24, 0), dev, s256, true);
        CHECK(h.sorter == Sorter::Block256 && h.wave_bins);
    }
    // everybody else: no wave sort, whatever the switch says
    const T4DProblem others[] = { problem(8280, 512, 375, 1, 0),                          /* Topo4D's own call: Block1024 or fused */
                                  problem(30000, 512, 512, 3, 0),                         /* a view-sharded rank */
                                  problem(1000000, 4096, 3008, 1, 0) };                  /* the dense one-view pass: fused */
    for (const T4DProblem &p : others)
        for (const Overrides &o : { ov, off }) {
            const ForwardPlan f = plan_forward(p, dev, o, true);
            CHECK(f.sorter != Sorter::Block256 && !f.wave_bins);
        }
}

int main()
{
    check_header();
    check_K<1>();
    check_K<2>();
    check_K<4>();
    check_K<8>();
    check_plans();
    if (g_failed) { printf("%d failed of %llu\n", g_failed, g_checks); return 1; }
    printf("ok %llu\n", g_checks);
    return 0;
}
