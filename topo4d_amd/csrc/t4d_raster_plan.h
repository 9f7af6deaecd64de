// t4d_raster_plan.h - which regime a rasterizer launch is in: decided once, here, as a value.
//
// The render path has several builds of most of its kernels (a latency and a throughput build, whole tiles or depth segments of
// 64 / 128 list positions, a fused or a separate bin sort, a front end of one, two or three-four launches) and which of them run
// depends on the launch's dimensions, the caller's flags, the device's size and the environment switches of INTEGRATION.md §7.
// t4d_state_bytes, the forward and the backward of a call must reach the SAME answer - a forward that kept snapshots feeds a
// segmented backward, a forward that left its long tiles out relies on three more launches - so the answer is computed by the
// pure functions below and nowhere else: regime_of (what the problem alone decides: the state layout and the kernel parameter
// block take it from there), plan_forward and plan_backward (what each entry point launches, with every grid size).  A plan is a
// value: it decides and launches nothing.  tests/native/raster_plan_host.cpp pins the plans of the launch shapes the project is
// about, switch by switch, and asserts that the two directions agree.
//
// CONTRACT: the backward must be given the T4DProblem of its forward, FLAGS INCLUDED (topo4d_amd/rasterizer.py keeps the forward's
// problem for that).  The regime is re-derived from it, not read from the state buffer: a forward with T4D_FLAG_NO_LONG_BINS on a
// big one-view launch keeps no slot table, and a backward WITHOUT the flag would leave the long tiles out of its whole-tile launch
// expecting segments that were never written.
//
// Plain C++17: no HIP, nothing __device__ (T4D_HD only lets the kernels call gaussian_grid).  Included first by t4d_raster.hip and
// by the host test program.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <unistd.h>

#include <algorithm>

#include "../../include/t4d_config.h"
#include "../../include/topo4d_raster.h"

#ifndef T4D_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define T4D_HD __host__ __device__
#else
#define T4D_HD
#endif
#endif

// ---------------------------------------------------------------------------------------------------------
// regime constants
// ---------------------------------------------------------------------------------------------------------
constexpr int kBlock = 256;          // threads per workgroup everywhere (4 wave64)
#ifndef T4D_FWD_BATCH
#define T4D_FWD_BATCH 192
#endif
constexpr int kFwdBatch = T4D_FWD_BATCH;   // splats staged in LDS per round of the forward blend (one per thread: <= 256; sweep of round 3 with 7 waves per SIMD, config 2 / config 4: 128: 106 / 1,197 us, 192: 101.5 / 1,113, 256: 102 / 1,134)
constexpr int kSortLdsCap = 2048;    // keys sorted in LDS by k_sort_tiles (16 KiB: 8 workgroups per CU); longer bins go to k_sort_long
constexpr int kLongBlock = 1024;     // k_sort_long_chunks, k_merge_long (bins beyond kSortLdsCap keys) and small launches' k_sort_tiles: threads per workgroup
constexpr int kScanChunk = 1024;     // tiles scanned per workgroup of k_scan_tiles
// pair-slot cursors per view, at most (same-address returning atomics are serial: see k_preprocess).  A view gets one cursor per 16
// workgroups of Gaussians up to this many: 8 at config 2 (118 workgroups per view), 32 at config 4, 64 for ONE view of 10^6 Gaussians -
// 3,907 workgroups on 8 cursors were 488 serial atomics each: k_preprocess 60.4 -> 37.8 us there (round 5; 256 cursors: 33.5, but the
// scan's walk over them costs what that saves)
constexpr int kCursorSegs = 64;
// Small launches (the reference's own call shape: ONE view per call, train.py:661-673; a view-sharded rank: three views) cannot
// fill the chip with whole tiles: a kernel lasts as long as its LONGEST tile list is walked by one workgroup.  For launches of
// at most kSegMaxTiles tiles the backward is therefore cut along DEPTH: a tile list of n pairs becomes ceil(n / kSeg)
// independent work items.  What makes them independent is kept by the forward: the per-pixel blend state (T, C, D) at every
// kSeg-th list position (a "snapshot", 20 bytes per pixel and boundary) - the backward's replay of positions [j kSeg, (j+1) kSeg)
// starts from the transmittance in front of position (j+1) kSeg and from the suffix colour (C_final - C_prefix) / T, both taken
// from the snapshots instead of from the replay of everything behind.  No running value of the replay feeds a discrete
// decision, so the segments take the decisions of the whole-list replay; sums differ by rounding only.
#ifndef T4D_SEG
#define T4D_SEG 128
#endif
constexpr int kSeg = T4D_SEG;        // list positions per backward segment of a 2-8 view launch; a ONE-view launch takes kSegOne (seg_positions)
constexpr int kSegOne = 64;          // round 4 measured it with a compile-time switch: one view of Topo4D's size 85.4 -> 81.3 us (half the walk per
                                     // work item, twice the list rounds in the forward), three views of the config-2 scene 176 -> 183: hence per launch
constexpr int kSegMaxTiles = 8192;   // launches of at most this many tiles (V * T) run the segmented backward
// A ONE-view launch of more tiles than that (the texture pass: one 4096 x 3008 view = 48,128 tiles of 10^6 Gaussians) fills the chip
// with whole tiles - until the short tiles run out and a few workgroups are still walking lists of thousands of pairs: the SAME
// number of wave-steps (counting build) took the backward 343 us on a scene whose longest list held 1,459 pairs and 400 / 906 us
// (two cameras) on one with lists of 9,000 - 12,000.  There the tiles of at least kSegLongMin pairs - and only those - are cut into
// segments (kSeg positions each, their own launch behind the whole-tile one, which skips them): same box, whole tiles / threshold
// 1,024 / 2,048 / 4,096: 400 / 406 / 403 / 382 us and 906 / 414 / 398 / 529 us.  (Segments for EVERY tile of such a launch, the
// small launches' way: 488 / 506 us and 50 us more in the forward, which then keeps 40,000 snapshots.)
#ifndef T4D_SEG_LONG_MIN
#define T4D_SEG_LONG_MIN 2048
#endif
constexpr int kSegLongMin = T4D_SEG_LONG_MIN;
static_assert((kSegLongMin & (kSegLongMin - 1)) == 0, "k_fwd_long_prefix stops at the first work item of a shorter length CLASS (powers of two)");
static_assert(kSegOne == 64 && kSeg == 128, "seg_shift assumes segment lengths of 64 and 128");
constexpr int kSmallTiles = 4 * kBlock;  // ONE view of at most this many tiles: scan and scatter are one launch (k_scan_scatter_small: four tile counts per thread)
constexpr int kEmptySpan = 64;           // tiles per spare workgroup of the empty-tile share of cotangent_dot
#ifndef T4D_SHB_VIEWS
#define T4D_SHB_VIEWS 8                  // views k_sh_bwd16 serves from one fetch of its 256 coefficient rows
#endif
// Grids of the per-tile kernels: at most this many workgroups per CU.  Beyond that (config 4: 393k tiles per launch) more workgroups
// only add prologues - the best div measured there was 12-16 (24-33k workgroups: 5.13 -> 4.79 ms per step), at config 2 (24.6k
// tiles) it is 2
constexpr int kMaxGridPerCu = 96;

// ---------------------------------------------------------------------------------------------------------
// what the problem alone decides
// ---------------------------------------------------------------------------------------------------------
// the tile grid of a W x H image: the one place that divides by the tile size
struct TileDims { int gx, gy; int64_t T; };
inline TileDims tile_dims(const int W, const int H)
{
    TileDims d;
    d.gx = (W + T4D_TILE_X - 1) / T4D_TILE_X;
    d.gy = (H + T4D_TILE_Y - 1) / T4D_TILE_Y;
    d.T = (int64_t)d.gx * (int64_t)d.gy;
    return d;
}

// segmented backward (see kSeg): decided by the problem's dimensions alone, so that t4d_state_bytes, the forward and the
// backward of a call agree without talking to each other
// 0: whole tiles only; 1: every tile is segmented (small launch); 2: the long tiles of a big one-view launch are
inline int seg_mode(const T4DProblem &p)
{
    if ((long long)p.n_views * tile_dims(p.W, p.H).T <= kSegMaxTiles) return 1;
    return p.n_views == 1 ? 2 : 0;
}
// Segment slots of a view.  Tile t (arena offset off, n pairs) owns the slots floor(off / kSeg) + t ... + ceil(n / kSeg) - 1:
// disjoint from tile to tile ((off + n) / kSeg - off / kSeg >= floor(n / kSeg)) without a prefix sum over the tiles.
// seg_mode 2 (only the tiles of at least kSegLongMin pairs own slots): floor(off / kSeg) + floor(off / kSegLongMin) instead - the
// second term grows by at least one from a long tile to the next ((off + n) / kSegLongMin - off / kSegLongMin >= 1 for n >=
// kSegLongMin), which is all the "+ t" was for: cap / kSeg + cap / kSegLongMin slots instead of cap / kSeg + T (one
// 4096 x 3008 view carried 48,128 x 6 KB = 290 MB of snapshot slots for tiles that can never own one).
inline int seg_positions(const T4DProblem &p) { return (p.n_views == 1 && seg_mode(p) == 1) ? kSegOne : kSeg; }
inline size_t seg_slots_per_view(const T4DProblem &p, size_t T)
{
    if (seg_mode(p) == 2) return (size_t)p.pair_capacity / (size_t)kSeg + (size_t)p.pair_capacity / (size_t)kSegLongMin + 2;
    return (size_t)p.pair_capacity / (size_t)seg_positions(p) + T + 1;
}

// grid of the per-Gaussian kernels: blocks of 256 Gaussians in groups of eight (one per XCD), times the views (block_and_view)
T4D_HD inline unsigned gaussian_grid(const int P, const int V) { return (unsigned)((((P + kBlock - 1) / kBlock + 7) / 8) * 8 * V); }

// The regime-dependent fields of the kernel parameter block (KP, same names) and the tile grid they follow from.  Forward and
// backward of a call get the same ones because both derive them from the same T4DProblem (the contract above).
struct Regime {
    int gx, gy, T;
    int seg_mode;
    uint32_t slots_per_view;         // 0: this launch is not segmented
    uint32_t seg_shift;              // log2 of the backward's segment length of this launch (seg_positions: 6 or 7)
    uint32_t slots_by_offset;        // seg_mode 2: a long tile's first slot is off / kSeg + off / kSegLongMin, not off / kSeg + tile
    uint32_t seg_min_pairs;          // tiles of fewer pairs are not segmented (0: every tile is; kSegLongMin: seg_mode 2; ~0: none is)
    uint32_t views_per_set;          // 0: one parameter set for all views
    uint32_t nseg, seg_cap;          // pair-slot cursors per view and the slots each hands out
    int n_chunks;                    // scan chunks per view = ceil(T / kScanChunk)
    int long_bins_elsewhere;         // 1: k_sort_long runs behind k_sort_tiles and takes the bins longer than kSortLdsCap
    int segn;                        // list positions per snapshot the forward keeps = per segment of the backward (0: none)
};
inline Regime regime_of(const T4DProblem &p)
{
    Regime r;
    const TileDims d = tile_dims(p.W, p.H);
    r.gx = d.gx; r.gy = d.gy; r.T = (int)d.T;                  // (check_problem: at most 2^20 tiles)
    r.seg_mode = seg_mode(p);
    r.slots_per_view = r.seg_mode != 0 ? (uint32_t)seg_slots_per_view(p, (size_t)r.T) : 0u;
    r.seg_shift = seg_positions(p) == 64 ? 6u : 7u;
    r.slots_by_offset = r.seg_mode == 2 ? 1u : 0u;
    // seg_mode 2: the caller's word that no list is long (T4D_FLAG_NO_LONG_BINS) keeps every tile whole
    r.seg_min_pairs = r.seg_mode == 2 ? ((p.flags & T4D_FLAG_NO_LONG_BINS) ? 0xffffffffu : (uint32_t)kSegLongMin) : 0u;
    r.views_per_set = (p.views_per_param_set != 0u && p.views_per_param_set < (uint32_t)p.n_views) ? p.views_per_param_set : 0u;
    const uint32_t n_wg = (uint32_t)((p.P + kBlock - 1) / kBlock);
    r.nseg = 1;
    while (r.nseg < (uint32_t)kCursorSegs && n_wg >= 16u * r.nseg) r.nseg <<= 1;       // >= 8 workgroups per cursor
    r.seg_cap = (uint32_t)p.pair_capacity / r.nseg;
    r.n_chunks = (r.T + kScanChunk - 1) / kScanChunk;
    r.long_bins_elsewhere = (p.flags & T4D_FLAG_NO_LONG_BINS) ? 0 : 1;
    // small launch, or a big one-view launch that may hold long lists: snapshots for the segmented backward (kSeg)
    r.segn = (r.slots_per_view != 0u && r.seg_min_pairs != 0xffffffffu) ? seg_positions(p) : 0;
    return r;
}

// ---------------------------------------------------------------------------------------------------------
// what the environment and the device add
// ---------------------------------------------------------------------------------------------------------
// The switches of INTEGRATION.md §7 that the rasterizer reads; read once per entry-point call (the tests switch them at run time
// inside one process).
struct Overrides {
    bool has_latency_tiles = false, has_fwd_latency_tiles = false;
    int latency_tiles = 0;           // T4D_LATENCY_TILES: launches of at most this many tiles run the latency builds (0 = never)
    int fwd_latency_tiles = 0;       // T4D_FWD_LATENCY_TILES: the same for the forward alone (goes before T4D_LATENCY_TILES there)
    int tile_div = 0;                // T4D_TILE_DIV > 0: tiles per workgroup of the per-tile kernels' grids
    bool no_segments = false;        // T4D_NO_SEGMENTS: whole-tile backward (the forward's state serves both)
    bool no_long_fwd = false;        // T4D_NO_LONG_FWD: no depth-parallel forward of a big one-view launch's long tiles
    bool no_fused_sort = false;      // T4D_NO_FUSED_SORT: the bins are sorted by k_sort_tiles, never by the render workgroups
    bool sort_256 = false;           // T4D_SORT_256: small launches keep the 256-thread k_sort_tiles
    bool no_front_fusion = false;    // T4D_NO_FRONT_FUSION: no k_front_small
    bool status_by_copy = false;     // T4D_STATUS_BY_COPY: the async status block is copied, not written by the binning kernel
    bool no_prune = false;           // T4D_NO_PRUNE: big launches that may hold long lists run the plain throughput forward
    bool no_small_view = false;      // T4D_NO_SMALL_VIEW: one small view takes the general front end
    bool fill_scalar = false;        // T4D_FILL_SCALAR: empty tiles written with 4-byte stores
    bool sh_bwd_plain = false;       // T4D_SH_BWD_PLAIN: the general SH backward also for degree 3
    bool no_wave_sort = false;       // T4D_NO_WAVE_SORT: the 256-thread k_sort_tiles sorts bins of 64 keys and more through LDS, one per workgroup
};
inline Overrides read_overrides()
{
    Overrides o;
    // (every getenv is a walk over the whole environment and this runs in every call, where a one-view iteration is a few hundred
    // microseconds of host time: one walk of its own first - a process without any T4D_ variable, the normal case, is done after it)
    bool any = false;
    for (char **e = environ; e && *e && !any; e++) any = (*e)[0] == 'T' && (*e)[1] == '4' && (*e)[2] == 'D' && (*e)[3] == '_';
    if (!any) return o;
    if (const char *e = getenv("T4D_LATENCY_TILES")) { o.has_latency_tiles = true; o.latency_tiles = atoi(e); }
    if (const char *e = getenv("T4D_FWD_LATENCY_TILES")) { o.has_fwd_latency_tiles = true; o.fwd_latency_tiles = atoi(e); }
    if (const char *e = getenv("T4D_TILE_DIV")) o.tile_div = atoi(e);
    o.no_segments = getenv("T4D_NO_SEGMENTS") != nullptr;
    o.no_long_fwd = getenv("T4D_NO_LONG_FWD") != nullptr;
    o.no_fused_sort = getenv("T4D_NO_FUSED_SORT") != nullptr;
    o.sort_256 = getenv("T4D_SORT_256") != nullptr;
    o.no_front_fusion = getenv("T4D_NO_FRONT_FUSION") != nullptr;
    o.status_by_copy = getenv("T4D_STATUS_BY_COPY") != nullptr;
    o.no_prune = getenv("T4D_NO_PRUNE") != nullptr;
    o.no_small_view = getenv("T4D_NO_SMALL_VIEW") != nullptr;
    o.fill_scalar = getenv("T4D_FILL_SCALAR") != nullptr;
    o.sh_bwd_plain = getenv("T4D_SH_BWD_PLAIN") != nullptr;
    o.no_wave_sort = getenv("T4D_NO_WAVE_SORT") != nullptr;
    return o;
}

struct DeviceFacts {
    int cus;                         // compute units of the current device
    unsigned front_resident_blocks;  // workgroups of k_front_small the device holds at once (only asked for when front_small_candidate)
};

// Grid of the per-tile kernels.  They are grid-stride loops over the length-ordered work items, so the grid size is a
// free choice.  Measured on MI355X (config 2): a RESIDENT grid (CUs x 4-6 workgroups; the switch is gone) loses 1.3x to
// the hardware dispatcher's dynamic balancing; one workgroup per tile pays ~25k workgroup launches of which two
// thirds only find an empty tile; V*T / div workgroups, each taking items b, b+G, b+2G, ... (one from every length
// class, heavy first), keeps the dynamic balancing and divides the launch overhead.  T4D_TILE_DIV overrides div.
inline int tile_grid(const int n_tiles, const int per_cu, const int div, const DeviceFacts &dev, const Overrides &ov)
{
    if (ov.tile_div > 0) return std::max(std::min(n_tiles, dev.cus * per_cu), (n_tiles + ov.tile_div - 1) / ov.tile_div);
    return std::max(std::min(n_tiles, dev.cus * per_cu), std::min((n_tiles + div - 1) / div, dev.cus * kMaxGridPerCu));
}

// A launch of at most this many tiles runs the LATENCY build of the backward render kernel: with <= 4 workgroups per CU in total
// nothing queues behind anything, and a kernel lasts as long as its longest tile (T4D_LATENCY_TILES overrides; 0 = never).
inline bool latency_launch(const int n_tiles, const DeviceFacts &dev, const Overrides &ov)
{
    return n_tiles <= (ov.has_latency_tiles ? ov.latency_tiles : 4 * dev.cus);
}
// The FORWARD's latency build (registers for instruction-level parallelism, its own tile's bin sorted in the workgroup, records
// of the next batch in flight during the walk) stays ahead of the throughput build for much larger launches than the
// backward's did (which needs 82 KiB of LDS per workgroup): T4D_FWD_LATENCY_TILES overrides, T4D_LATENCY_TILES too (tests).
// Where the two builds cross depends on the scene: a launch that waits for one long list (the config-2 scene: 1,400 pairs in a
// tile) is better off in the latency build up to ~6 views (4 views: 67 against 82 us), a launch of many short lists (Topo4D's
// scene, longest 470) only up to 4 (5 views: 48 against 35 us).  The caller's T4D_FLAG_LONG_LISTS says which it is.
inline bool latency_launch_fwd(const int n_tiles, const uint32_t flags, const DeviceFacts &dev, const Overrides &ov)
{
    if (ov.has_fwd_latency_tiles) return n_tiles <= ov.fwd_latency_tiles;
    if (ov.has_latency_tiles) return n_tiles <= ov.latency_tiles;
    return n_tiles <= ((flags & T4D_FLAG_LONG_LISTS) ? 24 : 12) * dev.cus;
}

// one view of at most 1,024 tiles (Topo4D's own call shape): scan and scatter are ONE launch (k_scan_scatter_small) ...
inline bool small_view(const T4DProblem &p, const Overrides &ov)
{
    return p.n_views == 1 && tile_dims(p.W, p.H).T <= kSmallTiles && !ov.no_small_view;
}
// ... and with at most 128 workgroups of Gaussians preprocess could join them behind a grid-wide barrier (k_front_small): the
// launches for which the caller must fill DeviceFacts::front_resident_blocks
inline bool front_small_candidate(const T4DProblem &p, const Overrides &ov)
{
    return small_view(p, ov) && gaussian_grid(p.P, 1) + 1u <= 128u && !ov.no_front_fusion;
}

// ---------------------------------------------------------------------------------------------------------
// the forward's plan
// ---------------------------------------------------------------------------------------------------------
enum class FrontEnd {
    Fused,          // k_front_small
    SmallView,      // k_preprocess, k_scan_scatter_small
    General         // k_preprocess, (k_tile_chunk_sums,) k_scan_tiles, k_scatter
};
enum class Sorter { Fused /* no launch: the render workgroups sort */, Block1024 /* k_sort_tiles<kLongBlock> */, Block256 /* k_sort_tiles<kBlock> */ };
struct FwdBuild { bool lat; int fb; int segn; bool prune; bool long_elsewhere; };       // k_render_fwd<LAT, FB, SEGN, PRUNE, LONG>
constexpr uint32_t build_key(const FwdBuild b)
{
    return (uint32_t)b.lat | (uint32_t)b.prune << 1 | (uint32_t)b.long_elsewhere << 2 | (uint32_t)b.fb << 4 | (uint32_t)b.segn << 16;
}

struct ForwardPlan {
    Regime regime;
    FrontEnd front;
    unsigned preprocess_grid;        // k_front_small (its scan workgroup included) or k_preprocess
    unsigned small_grid;             // k_scan_scatter_small
    bool chunk_sums;                 // General: k_tile_chunk_sums runs (a view has more than one scan chunk)
    unsigned scan_grid_x, scan_grid_y, scatter_grid;
    bool status_by_kernel;           // the binning kernel writes the caller's pinned status block itself (publish_status), if it can be mapped
    Sorter sorter;
    unsigned sort_grid;
    bool wave_bins;                  // KP field: Block256 sorts the bins of fewer than 512 keys one per wave, in registers
    bool long_bins;                  // k_sort_long_chunks + k_merge_long
    unsigned long_bins_grid;
    FwdBuild render;
    uint32_t tile_blocks, fill_blocks, fill_vec;      // KP fields of the same names; the render grid is tile_blocks + fill_blocks
    bool long_fwd;                   // the three depth-parallel launches follow (k_fwd_long_seg<false>, k_fwd_long_prefix, k_fwd_long_seg<true>)
    unsigned long_seg_grid, long_prefix_grid;
    uint32_t fused_sort;             // KP field
};

inline ForwardPlan plan_forward(const T4DProblem &p, const DeviceFacts &dev, const Overrides &ov, const bool planes_aligned16)
{
    ForwardPlan f = {};
    const Regime &r = f.regime = regime_of(p);
    const int n_tiles = r.T * p.n_views;
    const bool checked = (p.flags & (T4D_FLAG_DEBUG_SYNC | T4D_FLAG_CHECKED)) != 0;

    // (the grid barrier of k_front_small is only safe when every workgroup of the launch is resident at once: checked against what
    // the DEVICE can hold - a CU mask or a compute partition of 32 CUs shows up there - not assumed from the workgroup count)
    f.front = !small_view(p, ov) ? FrontEnd::General
            : (front_small_candidate(p, ov) && gaussian_grid(p.P, 1) + 1u <= dev.front_resident_blocks) ? FrontEnd::Fused : FrontEnd::SmallView;
    f.preprocess_grid = f.front == FrontEnd::Fused ? gaussian_grid(p.P, 1) + 1u : gaussian_grid(p.P, p.n_views);
    f.small_grid = gaussian_grid(p.P, 1) + 1u;
    f.chunk_sums = r.n_chunks > 1;
    f.scan_grid_x = (unsigned)r.n_chunks; f.scan_grid_y = (unsigned)p.n_views;
    f.scatter_grid = gaussian_grid(p.P, p.n_views) + (unsigned)(((size_t)r.T * p.n_views + kBlock - 1) / kBlock);
    // un-synchronised one-view call with a pinned status block
    f.status_by_kernel = !checked && (p.flags & T4D_FLAG_ASYNC_STATUS) != 0 && small_view(p, ov) && !ov.status_by_copy;

    // Who sorts the bins.  A big launch: k_sort_tiles on 256 threads.  A small launch (at most kSegMaxTiles tiles) waits for its
    // longest bin: 1024 threads per bin - unless the forward runs its latency build AND the caller knows that every bin fits the
    // one-pass ranking sort (T4D_FLAG_SHORT_BINS): then the render workgroup of a tile sorts its own bin (no launch at all).
    const bool lat = latency_launch_fwd(n_tiles, p.flags, dev, ov);
    // a big one-view launch that may hold long lists: its long tiles go through the depth-parallel kernels (three launches over the
    // slot table, t4d_raster_render_fwd_long.h), and the throughput forward that renders the others leaves the long ones out and
    // sorts its own tiles' bins first (k_render_fwd, FUSE): no k_sort_tiles launch
    f.long_fwd = r.seg_mode == 2 && r.segn != 0 && !lat && !ov.no_long_fwd;
    f.fused_sort = (!ov.no_fused_sort && (f.long_fwd || (lat && (p.flags & T4D_FLAG_SHORT_BINS) != 0))) ? 1u : 0u;
    // (1024 threads per bin only pay when some bin is long: with the caller's word that every bin fits the ranking sort, a
    // small launch of several views keeps the 256-thread kernel - 4 views of Topo4D's size: 9.7 against 12.6 us)
    if (f.fused_sort) { f.sorter = Sorter::Fused; f.sort_grid = 0; }
    else if (r.seg_mode == 1 && (p.flags & T4D_FLAG_SHORT_BINS) == 0 && !ov.sort_256) { f.sorter = Sorter::Block1024; f.sort_grid = (unsigned)std::min(n_tiles, 4 * dev.cus); }
    else { f.sorter = Sorter::Block256; f.sort_grid = (unsigned)tile_grid(n_tiles, 5, 2, dev, ov); }
    // (the 256-thread sorter takes bins of fewer than 512 keys one per wave: same launch, same grid - t4d_raster_sort.h)
    f.wave_bins = f.sorter == Sorter::Block256 && !ov.no_wave_sort;
    // bins beyond the LDS sort buffer (the caller has not said that there are none): their chunks, then the merges
    f.long_bins = r.long_bins_elsewhere != 0;
    f.long_bins_grid = (unsigned)std::min(n_tiles, 2 * dev.cus);

    f.tile_blocks = (uint32_t)(lat ? n_tiles : tile_grid(n_tiles, 6, 2, dev, ov));
    f.fill_blocks = (uint32_t)(r.gy * p.n_views);
    f.fill_vec = (p.W % 4 == 0 && planes_aligned16 && !ov.fill_scalar) ? 1u : 0u;
    if (f.long_fwd) f.render = { false, kFwdBatch, 0, true, true };
    else if (lat || r.segn != 0) f.render = { lat, kBlock, r.segn, true, false };
    // a big launch that may hold long lists (the caller has not passed T4D_FLAG_NO_LONG_BINS): a dense pass
    else f.render = { false, kFwdBatch, 0, r.long_bins_elsewhere != 0 && !ov.no_prune, false };
    f.long_seg_grid = std::min(r.slots_per_view, (uint32_t)(8 * dev.cus));
    f.long_prefix_grid = std::min((uint32_t)r.T, (uint32_t)(4 * dev.cus));
    return f;
}

// ---------------------------------------------------------------------------------------------------------
// the backward's plan
// ---------------------------------------------------------------------------------------------------------
struct BwdBuild { bool da, lat; int segn; bool long_elsewhere; };                       // k_render_bwd<DA, LAT, SEGN, LONG>
constexpr uint32_t build_key(const BwdBuild b)
{
    return (uint32_t)b.da | (uint32_t)b.lat << 1 | (uint32_t)b.long_elsewhere << 2 | (uint32_t)b.segn << 16;
}
struct BwdLaunch { BwdBuild build; uint32_t tile_blocks; unsigned grid; };                // tile_blocks: the KP field of this launch
enum class ShBackward { None, Degree3x16 /* k_sh_bwd16 */, General /* k_sh_bwd */ };

struct BackwardPlan {
    Regime regime;
    int n_render;                    // 1, or 2: whole tiles, then the segments of the long tiles of a big one-view launch
    BwdLaunch render[2];
    unsigned gaussian_grid;          // k_preprocess_bwd
    ShBackward sh;
    unsigned sh_grid;
};

inline BackwardPlan plan_backward(const T4DProblem &p, const DeviceFacts &dev, const Overrides &ov, const bool da,
                                  const bool wants_tile_dot, const bool has_shs)
{
    BackwardPlan b = {};
    const Regime &r = b.regime = regime_of(p);
    const int n_tiles = r.T * p.n_views;
    const bool lat = latency_launch(n_tiles, dev, ov);
    // small launches: one workgroup per segment slot (kSeg; T4D_NO_SEGMENTS=1: whole tiles, for tests and experiments - the
    // forward's state serves both)
    // (seg_mode 2 - the long tiles of a big one-view launch - only when the caller has not said that there are none: the forward
    // of a call that says so keeps no snapshots, and a forward that kept them is simply not used)
    const bool seg = r.seg_mode == 1 && !ov.no_segments;
    const bool seg_long = r.seg_mode == 2 && r.segn != 0 && !ov.no_segments;
    const uint32_t tile_blocks = seg ? (uint32_t)p.n_views * r.slots_per_view : (uint32_t)(lat ? n_tiles : tile_grid(n_tiles, 4, 2, dev, ov));
    const unsigned grid = tile_blocks + (wants_tile_dot ? (uint32_t)p.n_views * (uint32_t)((r.T + kEmptySpan - 1) / kEmptySpan) : 0u);
    b.n_render = 1;
    if (seg_long) {
        // two launches: the whole-tile throughput build leaves out the tiles that own segments (the forward wrote their slot-table
        // entries), then the segmented build walks the slot table with a fixed number of workgroups (most of its cap / kSeg + T
        // slots are empty: one workgroup per slot would be 79,000 launches for a few thousand segments)
        b.n_render = 2;
        b.render[0] = { { da, false, 0, true }, tile_blocks, grid };
        const uint32_t walkers = std::min(r.slots_per_view, (uint32_t)(8 * dev.cus));
        b.render[1] = { { da, false, kSeg, true }, walkers, walkers };
    } else if (seg) {
        // Segments always run the throughput build: the latency build's one slab per DPP row is 82 KiB of LDS, ONE workgroup per
        // CU, and a one-view launch has more segments than CUs (432 at Topo4D's size: two rounds, 47 us against 29 us measured)
        b.render[0] = { { da, false, r.segn, false }, tile_blocks, grid };
    } else {
        b.render[0] = { { da, lat, 0, false }, tile_blocks, grid };
    }
    b.gaussian_grid = gaussian_grid(p.P, p.n_views) + (wants_tile_dot ? (unsigned)p.n_views : 0u);
    // (k_sh_bwd16 serves T4D_SHB_VIEWS views from one fetch of the coefficient rows: they must belong to one parameter set)
    if (!has_shs) { b.sh = ShBackward::None; b.sh_grid = 0; }
    else if (p.sh_coeffs == 16 && p.sh_degree == 3 && !ov.sh_bwd_plain && (r.views_per_set == 0u || r.views_per_set % T4D_SHB_VIEWS == 0u)) {
        b.sh = ShBackward::Degree3x16;
        b.sh_grid = gaussian_grid(p.P, (p.n_views + T4D_SHB_VIEWS - 1) / T4D_SHB_VIEWS);
    } else {
        b.sh = ShBackward::General;
        b.sh_grid = gaussian_grid(p.P, p.n_views);
    }
    return b;
}
