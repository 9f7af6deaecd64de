// t4d_raster_sort_net.h - the bitonic network of the one-wave bin sort, as data.
//
// N = 64 K elements (K = 1, 2, 4, 8 keys per lane of a wave64), element index i = lane K + e: a lane owns K CONSECUTIVE keys.
// The network is the classic one: for every block size k = 2, 4, ..., N the distances j = k/2, k/4, ..., 1; a stage compares
// element i with element i ^ j, and i keeps the smaller of the two iff (bit j of i is clear) == (bit k of i is clear) - the
// blocks of size k alternate between ascending and descending, the last one (k = N, whose bit no index has) is ascending.
// A stage with j < K exchanges inside a lane (compare + selects on the lane's own registers), one with j >= K between lanes
// at distance j / K (lane_xor).  Equal elements may end in either order: the keys are unique where the order matters (the
// Gaussian index is the low word), and padding or stale duplicates are bit-equal, so the sorted sequence is unique.
//
// Plain C++17, nothing __device__ (T4D_HD only lets the kernels call it): sort_bin_wave (t4d_raster_sort.h) unrolls the
// stage list at compile time, tests/native/sort_net_host.cpp runs the same list on a host model of 64 lanes.
#pragma once

#ifndef T4D_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define T4D_HD __host__ __device__
#else
#define T4D_HD
#endif
#endif

namespace t4d_sort_net {

constexpr int kLanes = 64;
constexpr int kMaxKeysPerLane = 8;

struct Stage { int k, j; };          // block size and distance, in elements

T4D_HD constexpr int log2i(const int n) { return n <= 1 ? 0 : 1 + log2i(n / 2); }
T4D_HD constexpr int elements(const int K) { return kLanes * K; }
// stages of the network over N elements: 1 + 2 + ... + log2 N
T4D_HD constexpr int stage_count(const int N) { return log2i(N) * (log2i(N) + 1) / 2; }
// the s-th stage (0 <= s < stage_count(N)); the answer does not depend on N, which only bounds s
T4D_HD constexpr Stage stage_at(const int s, const int level = 1)
{
    return s < level ? Stage{ 1 << level, (1 << level) >> (s + 1) } : stage_at(s - level, level + 1);
}
T4D_HD constexpr bool in_lane(const Stage st, const int K) { return st.j < K; }
// in-lane stages among the first stage_count(64 K) (the table of DESIGN 6.3)
T4D_HD constexpr int in_lane_stages(const int K, const int s = 0)
{
    return s >= stage_count(elements(K)) ? 0 : (in_lane(stage_at(s), K) ? 1 : 0) + in_lane_stages(K, s + 1);
}
// lane distance of a cross-lane stage
T4D_HD constexpr int lane_distance(const Stage st, const int K) { return st.j / K; }

// is bit `bit` (a power of two) of element index lane K + e clear?  Split so that the half that a kernel knows at compile time
// (e) and the half it holds per lane stay apart.
T4D_HD constexpr bool bit_clear(const int K, const int lane, const int e, const int bit)
{
    return bit < K ? (e & bit) == 0 : (lane & (bit / K)) == 0;
}
// the direction rule: does element lane K + e keep the SMALLER of itself and its partner (element index ^ st.j)?
T4D_HD constexpr bool keeps_min(const Stage st, const int K, const int lane, const int e)
{
    return bit_clear(K, lane, e, st.j) == bit_clear(K, lane, e, st.k);
}

// keys per lane for a bin of n keys (1 <= n <= 64 kMaxKeysPerLane): the smallest network that holds it
T4D_HD constexpr int keys_per_lane(const unsigned n) { return n <= 64u ? 1 : n <= 128u ? 2 : n <= 256u ? 4 : 8; }

static_assert(stage_count(64) == 21 && stage_count(512) == 45, "21 cross-lane stages, 0 / 7 / 15 / 24 in-lane ones");
static_assert(in_lane_stages(1) == 0 && in_lane_stages(2) == 7 && in_lane_stages(4) == 15 && in_lane_stages(8) == 24, "");
static_assert(stage_at(0).k == 2 && stage_at(0).j == 1 && stage_at(2).k == 4 && stage_at(2).j == 1 && stage_at(20).k == 64 && stage_at(20).j == 1, "");

}   // namespace t4d_sort_net
