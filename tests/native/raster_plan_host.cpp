// Host build of csrc/t4d_raster_plan.h for the CPU tests: the launch plans of the shapes the project is about, against literals -
// at default and under every environment switch that applies, each of which must flip the decision INTEGRATION.md §7 documents
// and nothing else in the plan - and the agreement of forward and backward over all of them.
// Prints "ok <checks>" and exits 0, or prints every failure and exits 1.
#include <stdio.h>

#include <string>
#include <vector>

#include "../../topo4d_amd/csrc/t4d_raster_plan.h"

static unsigned long long g_checks = 0;
static int g_failed = 0;

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        g_checks++;                                                                       \
        if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); g_failed++; }      \
    } while (0)

// every field of a plan, so that "nothing else changed" is one comparison (and a failure shows what did)
static std::string str(const Regime &r)
{
    char b[1024];
    snprintf(b, sizeof(b), "g=%dx%d T=%d mode=%d slots=%u shift=%u by_off=%u min=%u vps=%u nseg=%u seg_cap=%u chunks=%d long_bins=%d segn=%d",
             r.gx, r.gy, r.T, r.seg_mode, r.slots_per_view, r.seg_shift, r.slots_by_offset, r.seg_min_pairs, r.views_per_set, r.nseg,
             r.seg_cap, r.n_chunks, r.long_bins_elsewhere, r.segn);
    return b;
}
static std::string str(const ForwardPlan &f)
{
    char b[1024];
    snprintf(b, sizeof(b), " | front=%d pre=%u small=%u sums=%d scan=%ux%u scatter=%u status_by_kernel=%d | sorter=%d@%u fused=%u long_bins=%d@%u"
             " | fwd{%d,%d,%d,%d,%d} tile=%u fill=%u vec=%u long_fwd=%d@%u,%u",
             (int)f.front, f.preprocess_grid, f.small_grid, (int)f.chunk_sums, f.scan_grid_x, f.scan_grid_y, f.scatter_grid,
             (int)f.status_by_kernel, (int)f.sorter, f.sort_grid, f.fused_sort, (int)f.long_bins, f.long_bins_grid, (int)f.render.lat,
             f.render.fb, f.render.segn, (int)f.render.prune, (int)f.render.long_elsewhere, f.tile_blocks, f.fill_blocks, f.fill_vec,
             (int)f.long_fwd, f.long_seg_grid, f.long_prefix_grid);
    return str(f.regime) + b;
}
static std::string str(const BackwardPlan &p)
{
    std::string s = str(p.regime);
    char b[1024];
    for (int i = 0; i < p.n_render; i++) {
        const BwdLaunch &l = p.render[i];
        snprintf(b, sizeof(b), " | bwd{%d,%d,%d,%d} tile=%u grid=%u", (int)l.build.da, (int)l.build.lat, l.build.segn,
                 (int)l.build.long_elsewhere, l.tile_blocks, l.grid);
        s += b;
    }
    snprintf(b, sizeof(b), " | gaussians=%u sh=%d@%u", p.gaussian_grid, (int)p.sh, p.sh_grid);
    return s + b;
}
#define CHECK_SAME(plan, expected)                                                                                          \
    do {                                                                                                                    \
        g_checks++;                                                                                                         \
        const std::string is_ = str(plan), expected_ = str(expected);                                                       \
        if (is_ != expected_) {                                                                                             \
            printf("FAIL line %d: %s\n  is       %s\n  expected %s\n", __LINE__, #plan, is_.c_str(), expected_.c_str());       \
            g_failed++;                                                                                                     \
        }                                                                                                                   \
    } while (0)

static T4DProblem problem(int V, int W, int H, int P, uint32_t flags, int64_t cap, int deg = 0, int coeffs = 0, uint32_t views_per_set = 0)
{
    T4DProblem p = {};
    p.abi_version = T4D_ABI_VERSION;
    p.n_views = V; p.W = W; p.H = H; p.P = P; p.flags = flags; p.pair_capacity = cap;
    p.sh_degree = deg; p.sh_coeffs = coeffs; p.scale_modifier = 1.f; p.views_per_param_set = views_per_set;
    return p;
}
static Overrides with(void (*set)(Overrides &))
{
    Overrides o;
    set(o);
    return o;
}

// every (problem, device, switches) the rows below plan, for the agreement check at the end
struct Case { T4DProblem p; DeviceFacts dev; Overrides ov; };
static std::vector<Case> g_cases;
static ForwardPlan fwd(const T4DProblem &p, const DeviceFacts &dev, const Overrides &ov)
{
    g_cases.push_back({ p, dev, ov });
    return plan_forward(p, dev, ov, true);
}
static BackwardPlan bwd(const T4DProblem &p, const DeviceFacts &dev, const Overrides &ov, bool dot = false)
{
    g_cases.push_back({ p, dev, ov });
    return plan_backward(p, dev, ov, false, dot, p.sh_coeffs > 0);
}
static bool is(const FwdBuild a, const FwdBuild b) { return build_key(a) == build_key(b); }
static bool is(const BwdBuild a, const BwdBuild b) { return build_key(a) == build_key(b); }

int main()
{
    const DeviceFacts mi355x = { 256, 2048 };       // 256 CUs, ample residency for k_front_small
    const DeviceFacts half = { 128, 2048 };
    const Overrides none;
    const Overrides no_front_fusion = with([](Overrides &o) { o.no_front_fusion = true; });
    const Overrides no_small_view = with([](Overrides &o) { o.no_small_view = true; });
    const Overrides status_by_copy = with([](Overrides &o) { o.status_by_copy = true; });
    const Overrides no_fused_sort = with([](Overrides &o) { o.no_fused_sort = true; });
    const Overrides sort_256 = with([](Overrides &o) { o.sort_256 = true; });
    const Overrides never_latency = with([](Overrides &o) { o.has_latency_tiles = true; o.latency_tiles = 0; });
    const Overrides always_latency = with([](Overrides &o) { o.has_latency_tiles = true; o.latency_tiles = 1000000000; });
    const Overrides no_segments = with([](Overrides &o) { o.no_segments = true; });
    const Overrides no_prune = with([](Overrides &o) { o.no_prune = true; });
    const Overrides no_long_fwd = with([](Overrides &o) { o.no_long_fwd = true; });
    const Overrides sh_bwd_plain = with([](Overrides &o) { o.sh_bwd_plain = true; });
    const Overrides fill_scalar = with([](Overrides &o) { o.fill_scalar = true; });
    const Overrides tile_div_4 = with([](Overrides &o) { o.tile_div = 4; });
    const uint32_t topo_flags = T4D_FLAG_NO_LONG_BINS | T4D_FLAG_SHORT_BINS | T4D_FLAG_ASYNC_STATUS;

    // ---- row 1: Topo4D's call: one 512 x 375 view of 8,280 Gaussians
    {
        const int64_t cap = 200000;
        const T4DProblem p = problem(1, 512, 375, 8280, topo_flags, cap);
        const ForwardPlan f = fwd(p, mi355x, none);
        CHECK(f.regime.T == 768 && f.regime.gx == 32 && f.regime.gy == 24);
        CHECK(f.regime.seg_mode == 1 && f.regime.segn == 64 && f.regime.seg_shift == 6u && f.regime.seg_min_pairs == 0u);
        CHECK(f.regime.slots_per_view == (uint32_t)(cap / 64 + 768 + 1));
        CHECK(f.regime.nseg == 4u && f.regime.seg_cap == 50000u && f.regime.n_chunks == 1 && f.regime.long_bins_elsewhere == 0);
        CHECK(f.front == FrontEnd::Fused && f.preprocess_grid == 41u);
        CHECK(f.status_by_kernel);
        CHECK(f.sorter == Sorter::Fused && f.fused_sort == 1u);
        CHECK(!f.long_bins && !f.long_fwd);
        CHECK(is(f.render, { true, 256, 64, true, false }));
        CHECK(f.tile_blocks == 768u && f.fill_blocks == 24u && f.fill_vec == 1u);
        const BackwardPlan b = bwd(p, mi355x, none);
        CHECK(b.n_render == 1 && is(b.render[0].build, { false, false, 64, false }));
        CHECK(b.render[0].tile_blocks == f.regime.slots_per_view && b.render[0].grid == f.regime.slots_per_view);
        CHECK(b.gaussian_grid == 40u && b.sh == ShBackward::None);
        CHECK(is(plan_backward(p, mi355x, none, true, false, false).render[0].build, { true, false, 64, false }));

        ForwardPlan e = f;                                   // T4D_NO_FRONT_FUSION: k_preprocess + k_scan_scatter_small
        e.front = FrontEnd::SmallView; e.preprocess_grid = 40;
        CHECK(e.small_grid == 41u);
        CHECK_SAME(fwd(p, mi355x, no_front_fusion), e);
        CHECK_SAME(fwd(p, DeviceFacts{ 256, 40 }, none), e);   // 41 workgroups do not fit 40 resident ones: not fused either
        CHECK_SAME(fwd(p, DeviceFacts{ 256, 41 }, none), f);
        e = f;                                               // T4D_NO_SMALL_VIEW: the general front end, one scan chunk, status by copy
        e.front = FrontEnd::General; e.preprocess_grid = 40; e.status_by_kernel = false;
        CHECK(!e.chunk_sums && e.scan_grid_x == 1u && e.scan_grid_y == 1u && e.scatter_grid == 43u);
        CHECK_SAME(fwd(p, mi355x, no_small_view), e);
        e = f; e.status_by_kernel = false;                   // T4D_STATUS_BY_COPY
        CHECK_SAME(fwd(p, mi355x, status_by_copy), e);
        e = f; e.status_by_kernel = false;                   // ... and so do T4D_FLAG_CHECKED and a call without T4D_FLAG_ASYNC_STATUS
        CHECK_SAME(fwd(problem(1, 512, 375, 8280, topo_flags | T4D_FLAG_CHECKED, cap), mi355x, none), e);
        CHECK_SAME(fwd(problem(1, 512, 375, 8280, topo_flags & ~T4D_FLAG_ASYNC_STATUS, cap), mi355x, none), e);
        e = f; e.sorter = Sorter::Block256; e.sort_grid = 768; e.fused_sort = 0;      // T4D_NO_FUSED_SORT: k_sort_tiles<256>
        CHECK_SAME(fwd(p, mi355x, no_fused_sort), e);
        e = f; e.fill_vec = 0;                               // T4D_FILL_SCALAR
        CHECK_SAME(fwd(p, mi355x, fill_scalar), e);
        CHECK(plan_forward(p, mi355x, none, false).fill_vec == 0u);                   // ... as for output planes off 16 bytes
        CHECK(plan_forward(problem(1, 510, 375, 8280, topo_flags, cap), mi355x, none, true).fill_vec == 0u);        // ... and W % 4 != 0
        // the same call without T4D_FLAG_SHORT_BINS: k_sort_tiles<1024>, or <256> under T4D_SORT_256
        const T4DProblem q = problem(1, 512, 375, 8280, topo_flags & ~T4D_FLAG_SHORT_BINS, cap);
        e = f; e.sorter = Sorter::Block1024; e.sort_grid = 768; e.fused_sort = 0;
        CHECK_SAME(fwd(q, mi355x, none), e);
        e.sorter = Sorter::Block256;
        CHECK_SAME(fwd(q, mi355x, sort_256), e);
        CHECK_SAME(fwd(p, mi355x, sort_256), f);             // (nothing to switch when the sort is fused)
        e = f;                                               // T4D_LATENCY_TILES=0: throughput forward and a sort launch
        e.render = { false, 256, 64, true, false }; e.sorter = Sorter::Block256; e.sort_grid = 768; e.fused_sort = 0;
        CHECK(e.tile_blocks == 768u);
        CHECK_SAME(fwd(p, mi355x, never_latency), e);
        CHECK_SAME(fwd(p, mi355x, with([](Overrides &o) { o.has_fwd_latency_tiles = true; o.fwd_latency_tiles = 0; })), e);
        // ... T4D_FWD_LATENCY_TILES goes before T4D_LATENCY_TILES in the forward
        CHECK_SAME(fwd(p, mi355x, with([](Overrides &o) { o.has_fwd_latency_tiles = o.has_latency_tiles = true; o.fwd_latency_tiles = 768; o.latency_tiles = 0; })), f);
        CHECK_SAME(fwd(p, mi355x, no_segments), f);          // the backward's switches leave the forward alone, and the other way round
        CHECK_SAME(fwd(p, mi355x, no_prune), f);
        CHECK_SAME(fwd(p, mi355x, no_long_fwd), f);
        CHECK_SAME(bwd(p, mi355x, never_latency), b);
        CHECK_SAME(bwd(p, mi355x, no_front_fusion), b);
        BackwardPlan eb = b;                                 // T4D_NO_SEGMENTS: whole tiles, latency build (768 <= 4 x 256)
        eb.render[0] = { { false, true, 0, false }, 768, 768 };
        CHECK_SAME(bwd(p, mi355x, no_segments), eb);
        eb.render[0].build.lat = false;                      // ... throughput build with T4D_LATENCY_TILES=0, or on 128 CUs (768 > 4 x 128)
        CHECK_SAME(bwd(p, mi355x, with([](Overrides &o) { o.no_segments = true; o.has_latency_tiles = true; o.latency_tiles = 0; })), eb);
        eb.render[0].tile_blocks = eb.render[0].grid = 512;
        CHECK_SAME(bwd(p, half, no_segments), eb);
    }
    // ---- row 2: the fused front end's bound of 128 workgroups, the scan's included
    {
        const ForwardPlan a = fwd(problem(1, 512, 375, 30720, topo_flags, 200000), mi355x, none);
        CHECK(a.front == FrontEnd::Fused && a.preprocess_grid == 121u);
        const ForwardPlan b = fwd(problem(1, 512, 375, 30721, topo_flags, 200000), mi355x, none);
        CHECK(b.front == FrontEnd::SmallView && b.preprocess_grid == 128u && b.small_grid == 129u);
        CHECK(front_small_candidate(problem(1, 512, 375, 30720, topo_flags, 200000), none));
        CHECK(!front_small_candidate(problem(1, 512, 375, 30721, topo_flags, 200000), none));      // no occupancy query for these
        CHECK(!front_small_candidate(problem(1, 512, 375, 8280, topo_flags, 200000), no_front_fusion));
        CHECK(!front_small_candidate(problem(2, 512, 375, 8280, topo_flags, 200000), none));
    }
    // ---- row 3: one 1024 x 750 view
    {
        const T4DProblem p = problem(1, 1024, 750, 8280, topo_flags, 400000);
        const ForwardPlan f = fwd(p, mi355x, none);
        CHECK(f.regime.T == 3008 && f.regime.n_chunks == 3);
        CHECK(f.front == FrontEnd::General && f.chunk_sums && f.scan_grid_x == 3u && f.scan_grid_y == 1u && !f.status_by_kernel);
        CHECK(f.regime.seg_mode == 1 && f.regime.segn == 64 && f.regime.slots_per_view == 400000u / 64u + 3008u + 1u);
        CHECK(is(f.render, { true, 256, 64, true, false }) && f.sorter == Sorter::Fused);       // 3,008 <= 12 x 256
        CHECK(f.tile_blocks == 3008u && f.fill_blocks == 47u);
        CHECK(is(fwd(p, half, none).render, { false, 256, 64, true, false }));
        CHECK(is(fwd(problem(1, 1024, 750, 8280, topo_flags | T4D_FLAG_LONG_LISTS, 400000), half, none).render, { true, 256, 64, true, false }));
        CHECK(is(bwd(p, mi355x, none).render[0].build, { false, false, 64, false }));
        CHECK(is(bwd(p, mi355x, no_segments).render[0].build, { false, false, 0, false }));     // 3,008 > 4 x 256
    }
    // ---- row 4: a view-sharded rank: three 512 x 512 views
    {
        const T4DProblem p = problem(3, 512, 512, 30000, T4D_FLAG_NO_LONG_BINS, 300000);
        const ForwardPlan f = fwd(p, mi355x, none);
        CHECK(f.regime.T == 1024 && f.regime.seg_mode == 1 && f.regime.segn == 128 && f.regime.seg_shift == 7u);
        CHECK(f.regime.slots_per_view == 300000u / 128u + 1024u + 1u);
        CHECK(f.front == FrontEnd::General && !f.chunk_sums);
        CHECK(is(f.render, { true, 256, 128, true, false }) && f.tile_blocks == 3072u);          // exactly on the bound of 12 x 256
        CHECK(f.sorter == Sorter::Block1024 && f.sort_grid == 1024u);
        const BackwardPlan b = bwd(p, mi355x, none, true);
        CHECK(b.n_render == 1 && is(b.render[0].build, { false, false, 128, false }));
        CHECK(b.render[0].tile_blocks == 3u * f.regime.slots_per_view && b.render[0].grid == b.render[0].tile_blocks + 3u * 16u);
        const T4DProblem p4 = problem(4, 512, 512, 30000, T4D_FLAG_NO_LONG_BINS, 300000);
        CHECK(is(fwd(p4, mi355x, none).render, { false, 256, 128, true, false }));
        CHECK(is(fwd(problem(4, 512, 512, 30000, T4D_FLAG_NO_LONG_BINS | T4D_FLAG_LONG_LISTS, 300000), mi355x, none).render, { true, 256, 128, true, false }));
        CHECK(is(bwd(p4, mi355x, none).render[0].build, { false, false, 128, false }));
    }
    // ---- row 5: the segmenting bound of 8,192 tiles
    {
        const T4DProblem p8 = problem(8, 512, 512, 30000, T4D_FLAG_NO_LONG_BINS, 300000);
        const T4DProblem p9 = problem(9, 512, 512, 30000, T4D_FLAG_NO_LONG_BINS, 300000);
        CHECK(regime_of(p8).seg_mode == 1 && regime_of(p8).segn == 128 && regime_of(p8).slots_per_view != 0u);
        CHECK(regime_of(p9).seg_mode == 0 && regime_of(p9).segn == 0 && regime_of(p9).slots_per_view == 0u);
        CHECK(is(fwd(p8, mi355x, none).render, { false, 256, 128, true, false }));
        CHECK(is(fwd(p9, mi355x, none).render, { false, kFwdBatch, 0, false, false }));
        CHECK(is(bwd(p8, mi355x, none).render[0].build, { false, false, 128, false }));
        CHECK(is(bwd(p9, mi355x, none).render[0].build, { false, false, 0, false }));
    }
    // ---- row 6: BASELINE config 2: 24 views 512 x 512, 30,000 Gaussians
    {
        const T4DProblem p = problem(24, 512, 512, 30000, T4D_FLAG_NO_LONG_BINS, 300000);
        const ForwardPlan f = fwd(p, mi355x, none);
        CHECK(f.regime.seg_mode == 0 && f.regime.slots_per_view == 0u && f.regime.nseg == 8u);
        CHECK(f.front == FrontEnd::General && f.preprocess_grid == 2880u && !f.chunk_sums);
        CHECK(f.scan_grid_x == 1u && f.scan_grid_y == 24u && f.scatter_grid == 2976u);
        CHECK(f.sorter == Sorter::Block256 && f.sort_grid == 12288u && f.fused_sort == 0u);
        CHECK(!f.long_bins && !f.long_fwd);
        CHECK(is(f.render, { false, kFwdBatch, 0, false, false }) && f.tile_blocks == 12288u && f.fill_blocks == 768u);
        const BackwardPlan b = bwd(p, mi355x, none);
        CHECK(b.n_render == 1 && is(b.render[0].build, { false, false, 0, false }));
        CHECK(b.render[0].tile_blocks == 12288u && b.render[0].grid == 12288u && b.gaussian_grid == 2880u);
        BackwardPlan eb = b;
        eb.render[0].grid = 12288 + 384; eb.gaussian_grid = 2880 + 24;                          // the cotangent dot is asked for
        CHECK_SAME(bwd(p, mi355x, none, true), eb);
        CHECK_SAME(bwd(p, mi355x, no_segments), b);
        // without the caller's word that no bin is long: the long-bin launches run and the PRUNE build is used
        const T4DProblem q = problem(24, 512, 512, 30000, 0u, 300000);
        ForwardPlan e = f;
        e.regime.long_bins_elsewhere = 1; e.long_bins = true; e.render.prune = true;
        CHECK(e.long_bins_grid == 512u);
        CHECK_SAME(fwd(q, mi355x, none), e);
        e.render.prune = false;
        CHECK_SAME(fwd(q, mi355x, no_prune), e);
        CHECK_SAME(fwd(p, mi355x, no_prune), f);
        e = f; e.sort_grid = 6144; e.tile_blocks = 6144;                                         // T4D_TILE_DIV=4
        CHECK_SAME(fwd(p, mi355x, tile_div_4), e);
        CHECK(bwd(p, mi355x, tile_div_4).render[0].tile_blocks == 6144u);
    }
    // ---- row 7: BASELINE config 4: 24 views 2048 x 2048, 120,000 Gaussians, SH degree 3 with 16 coefficients
    {
        const T4DProblem p = problem(24, 2048, 2048, 120000, 0u, 4000000, 3, 16);
        const ForwardPlan f = fwd(p, mi355x, none);
        CHECK(f.regime.T == 16384 && f.regime.n_chunks == 16 && f.chunk_sums && f.regime.nseg == 32u);
        CHECK(f.sort_grid == 24576u && f.tile_blocks == 24576u);                                 // capped at 96 per CU
        const BackwardPlan b = bwd(p, mi355x, none);
        CHECK(b.render[0].tile_blocks == 24576u);
        CHECK(b.sh == ShBackward::Degree3x16 && b.sh_grid == 472u * 3u);
        BackwardPlan eb = b;
        eb.sh = ShBackward::General; eb.sh_grid = 472 * 24;
        CHECK_SAME(bwd(p, mi355x, sh_bwd_plain), eb);
        eb.regime.views_per_set = 3;
        CHECK_SAME(bwd(problem(24, 2048, 2048, 120000, 0u, 4000000, 3, 16, 3), mi355x, none), eb);
        CHECK(bwd(problem(24, 2048, 2048, 120000, 0u, 4000000, 3, 16, 8), mi355x, none).sh == ShBackward::Degree3x16);
        CHECK(bwd(problem(24, 2048, 2048, 120000, 0u, 4000000, 2, 16), mi355x, none).sh == ShBackward::General);
        CHECK(bwd(problem(24, 2048, 2048, 120000, 0u, 4000000), mi355x, none).sh == ShBackward::None);
    }
    // ---- row 8: the texture pass: one 4096 x 3008 view of 10^6 Gaussians
    {
        const int64_t cap = 16000000;
        const T4DProblem p = problem(1, 4096, 3008, 1000000, 0u, cap);
        const ForwardPlan f = fwd(p, mi355x, none);
        CHECK(f.regime.T == 48128 && f.regime.seg_mode == 2 && f.regime.segn == 128 && f.regime.nseg == 64u);
        CHECK(f.regime.slots_by_offset == 1u && f.regime.seg_min_pairs == (uint32_t)kSegLongMin);
        CHECK(f.regime.slots_per_view == (uint32_t)(cap / 128 + cap / 2048 + 2));
        CHECK(f.sorter == Sorter::Fused && f.fused_sort == 1u);                                  // the throughput forward sorts its own bins
        CHECK(f.long_bins && f.long_bins_grid == 512u);
        CHECK(is(f.render, { false, kFwdBatch, 0, true, true }) && f.tile_blocks == 24064u && f.fill_blocks == 188u);
        CHECK(f.long_fwd && f.long_seg_grid == 2048u && f.long_prefix_grid == 1024u);
        const BackwardPlan b = bwd(p, mi355x, none);
        CHECK(b.n_render == 2);
        CHECK(is(b.render[0].build, { false, false, 0, true }) && b.render[0].tile_blocks == 24064u && b.render[0].grid == 24064u);
        CHECK(is(b.render[1].build, { false, false, 128, true }) && b.render[1].tile_blocks == 2048u && b.render[1].grid == 2048u);
        CHECK(bwd(p, mi355x, none, true).render[0].grid == 24064u + 752u && bwd(p, mi355x, none, true).render[1].grid == 2048u);

        ForwardPlan e = f;                                   // T4D_NO_LONG_FWD: one pass that keeps the snapshots itself, and a sort launch
        e.long_fwd = false; e.render = { false, 256, 128, true, false }; e.sorter = Sorter::Block256; e.sort_grid = 24064; e.fused_sort = 0;
        CHECK_SAME(fwd(p, mi355x, no_long_fwd), e);
        CHECK_SAME(bwd(p, mi355x, no_long_fwd), b);
        e = f; e.sorter = Sorter::Block256; e.sort_grid = 24064; e.fused_sort = 0;                // T4D_NO_FUSED_SORT
        CHECK_SAME(fwd(p, mi355x, no_fused_sort), e);
        e = f;                                               // T4D_LATENCY_TILES=1000000000: latency forward, no depth-parallel launches
        e.long_fwd = false; e.render = { true, 256, 128, true, false }; e.sorter = Sorter::Block256; e.sort_grid = 24064; e.fused_sort = 0;
        e.tile_blocks = 48128;
        CHECK_SAME(fwd(p, mi355x, always_latency), e);
        BackwardPlan eb = b;                                 // ... and the backward keeps its two throughput launches, one workgroup per tile
        eb.render[0].tile_blocks = eb.render[0].grid = 48128;
        CHECK_SAME(bwd(p, mi355x, always_latency), eb);
        eb = b;                                              // T4D_NO_SEGMENTS: one whole-tile backward, not the LONG build
        eb.n_render = 1; eb.render[0].build = { false, false, 0, false };
        CHECK_SAME(bwd(p, mi355x, no_segments), eb);
        CHECK_SAME(fwd(p, mi355x, no_segments), f);
        // T4D_FLAG_NO_LONG_BINS: no snapshots used, plain throughput forward, one backward launch
        const T4DProblem q = problem(1, 4096, 3008, 1000000, T4D_FLAG_NO_LONG_BINS, cap);
        e = f;
        e.regime.seg_min_pairs = 0xffffffffu; e.regime.segn = 0; e.regime.long_bins_elsewhere = 0;
        e.long_fwd = false; e.long_bins = false; e.render = { false, kFwdBatch, 0, false, false };
        e.sorter = Sorter::Block256; e.sort_grid = 24064; e.fused_sort = 0;
        CHECK_SAME(fwd(q, mi355x, none), e);
        eb.regime = e.regime;
        CHECK_SAME(bwd(q, mi355x, none), eb);
        CHECK_SAME(bwd(q, mi355x, no_segments), eb);
    }
    // ---- the switches' names: each sets its own field of Overrides and no other, read anew at every call
    {
        const struct { const char *name; bool Overrides::*field; } flags[] = {
            { "T4D_NO_SEGMENTS", &Overrides::no_segments }, { "T4D_NO_LONG_FWD", &Overrides::no_long_fwd },
            { "T4D_NO_FUSED_SORT", &Overrides::no_fused_sort }, { "T4D_SORT_256", &Overrides::sort_256 },
            { "T4D_NO_FRONT_FUSION", &Overrides::no_front_fusion }, { "T4D_STATUS_BY_COPY", &Overrides::status_by_copy },
            { "T4D_NO_PRUNE", &Overrides::no_prune }, { "T4D_NO_SMALL_VIEW", &Overrides::no_small_view },
            { "T4D_FILL_SCALAR", &Overrides::fill_scalar }, { "T4D_SH_BWD_PLAIN", &Overrides::sh_bwd_plain },
        };
        const char *const numbers[] = { "T4D_LATENCY_TILES", "T4D_FWD_LATENCY_TILES", "T4D_TILE_DIV" };
        for (const auto &f : flags) unsetenv(f.name);
        for (const char *n : numbers) unsetenv(n);
        auto fields = [&](const Overrides &o) {
            std::string s;
            for (const auto &f : flags) s += o.*(f.field) ? '1' : '0';
            char b[128];
            snprintf(b, sizeof(b), " %d:%d %d:%d %d", (int)o.has_latency_tiles, o.latency_tiles, (int)o.has_fwd_latency_tiles, o.fwd_latency_tiles, o.tile_div);
            return s + b;
        };
        CHECK(fields(read_overrides()) == "0000000000 0:0 0:0 0");
        for (size_t i = 0; i < sizeof(flags) / sizeof(flags[0]); i++) {
            setenv(flags[i].name, "1", 1);
            std::string expected = "0000000000 0:0 0:0 0";
            expected[i] = '1';
            CHECK(fields(read_overrides()) == expected);
            unsetenv(flags[i].name);
        }
        setenv("T4D_LATENCY_TILES", "0", 1);
        CHECK(fields(read_overrides()) == "0000000000 1:0 0:0 0");
        setenv("T4D_FWD_LATENCY_TILES", "1000000000", 1);
        CHECK(fields(read_overrides()) == "0000000000 1:0 1:1000000000 0");
        unsetenv("T4D_LATENCY_TILES"); unsetenv("T4D_FWD_LATENCY_TILES");
        setenv("T4D_TILE_DIV", "4", 1);
        CHECK(fields(read_overrides()) == "0000000000 0:0 0:0 4");
        unsetenv("T4D_TILE_DIV");
        setenv("T4D_LIB", "somewhere", 1);                   // (a T4D_ variable that is no switch)
        CHECK(fields(read_overrides()) == "0000000000 0:0 0:0 0");
        unsetenv("T4D_LIB");
    }
    // ---- row 9: forward and backward agree, over every launch planned above
    for (const Case &c : g_cases) {
        const ForwardPlan f = plan_forward(c.p, c.dev, c.ov, true);
        const BackwardPlan b = plan_backward(c.p, c.dev, c.ov, false, false, c.p.sh_coeffs > 0);
        CHECK(str(f.regime) == str(b.regime));
        // the positions per snapshot the forward kept: its render kernel's, or the depth-parallel kernels' (kSeg)
        const int kept = f.long_fwd ? kSeg : f.render.segn;
        CHECK(kept == f.regime.segn);
        const int replayed = b.render[b.n_render - 1].build.segn;
        CHECK(replayed == (c.ov.no_segments ? 0 : kept));
        CHECK(b.n_render == 1 || (b.n_render == 2 && f.regime.seg_min_pairs == (uint32_t)kSegLongMin && !c.ov.no_segments));
        CHECK((b.n_render == 2) == (b.render[0].build.long_elsewhere && b.render[1].build.long_elsewhere));
        CHECK(f.long_fwd == f.render.long_elsewhere);
        // a forward that leaves its long bins to k_sort_long launches it; one that sorts in the render workgroups launches no sort
        CHECK(f.long_bins == (f.regime.long_bins_elsewhere != 0) && (f.sorter == Sorter::Fused) == (f.fused_sort != 0u));
    }
    if (g_failed) { printf("%d of %llu checks failed\n", g_failed, g_checks); return 1; }
    printf("ok %llu\n", g_checks);
    return 0;
}
