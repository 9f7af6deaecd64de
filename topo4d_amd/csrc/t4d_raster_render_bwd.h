// t4d_raster_render_bwd.h - part of the translation unit t4d_raster.hip (included there, inside its anonymous namespace; not a
// stand-alone header).  A.4: the separable moment reduction over a DPP row and the backward render kernel (whole tiles or depth segments).
// See t4d_raster.hip for the overview, the constants, the state layout and the kernel parameter block.
// ---------------------------------------------------------------------------------------------------------
// The backward's pixel map.  Waves, DPP rows and sub-blocks are the forward's (tile_pixel); only the place of a pixel INSIDE its
// 4x4 sub-block differs: lane i of a row takes pixel (x, y) = (i >> 2, i & 3), so that the four x of one y sit in the four
// banks of the row (bank = four consecutive lanes = bits b3 b2 of i) and the four y of one x inside one bank (bits b1 b0).
// Everything per pixel is read by pixel address; what the forward leaves BY THREAD (the snapshots of the segmented builds) is
// read through fwd_thread_of.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_pixel_bwd(int tid, int tx, int ty, int &px, int &py)
{
    const int w = tid >> 6, r = (tid >> 4) & 3, i = tid & 15;
    px = tx * T4D_TILE_X + ((w & 1) << 3) + ((r & 1) << 2) + (i >> 2);
    py = ty * T4D_TILE_Y + ((w >> 1) << 3) + ((r >> 1) << 2) + (i & 3);
}

// the forward's thread of the pixel this backward thread holds (same wave, same row, x and y swapped inside the row)
__device__ __forceinline__ int fwd_thread_of(int tid) { return (tid & ~15) | ((tid & 3) << 2) | ((tid >> 2) & 3); }

// ---------------------------------------------------------------------------------------------------------
// Reduction of a step's sums over each 16-lane DPP row, SEPARABLY: x first, then y.
// A lane holds e = G dL/dalpha and w = alpha T of its pixel.  Six of the ten sums of a record are moments of e about the splat
// centre; about a FIXED origin (the centre of the wave's 8x8 block: pixel = origin + (X, Y), |X|, |Y| <= 3.5, lane constants)
// they are linear in the raw moments  M_ab = sum e X^a Y^b, a + b <= 2, and a raw moment separates: sum e X^a over x, times Y^b,
// summed over y.  So only SIX values per lane enter the x stage - e, e X, e X^2 and the three w dL/dC - instead of ten products,
// and the y weights are applied to x-sums.  The slabs accumulate raw moments; the shift to the splat centre is done once per
// staged splat and wave where the record is written (moments_about_centre).
//   x stage (banks): "transpose-reduce" - at every butterfly level two partial-sum vectors are folded into one, each half of the
//     banks keeping a different value.  xor8 by row_ror:8: (e X^2 | c0) -> a, (c1 | c2) -> b, (e | e X) -> c, the second of each
//     pair in banks 2,3.  xor4 by bank-masked row shifts: a and b fold into ONE register (bank (b3 b2): e X^2, c1, c0, c2), c folds
//     into itself: banks 0,1 hold the x-sum of e, banks 2,3 that of e X - every bank one more copy than the fold needs, which
//     is what the y stage wants: the x-sum of e is needed under three weights (1, Y, Y^2), that of e X under two (1, Y).
//   y stage (inside a bank, quad_perm): the xor2 fold of the weighted copies needs no selects - "keep Ka on lanes with b1 = 0 and
//     Kb on the others, send the opposite" is a multiply by a lane constant (ks) and a DPP multiply-add by another (kg), the
//     weights folded in:  bank 0: (1 | Y) -> M00, M01   bank 1: (Y^2 | -) -> M02   bank 2: (1 | Y) -> M10, M11.  The other register
//     takes a plain xor2 add; xor1 folds the two with selects on the constant lane mask b0.
// Per step: 1 truncation of e (moment_e) + 4 products + 10 banked adds + 6 in the y stage (a plain xor2 add, the weight multiply
// and multiply-add, two selects, the xor1 add) = 21 vector instructions against 5 + 22 for ten products reduced one by one
// (config 2, 24 views: 252 -> 240 us); with a depth cotangent the seventh value (w dL/dD) is summed over x on its own (2) and
// folded in at xor2 with selects (+2).
// Written as one asm block: the instruction order keeps every DPP read at least two instructions behind the write of its source
// (the gfx9 VALU->DPP hazard), so no s_nop is needed between the levels; the leading s_nop covers inputs produced just before the
// block.  All inputs are read-only, the three temporaries are fresh registers (tying halves of packed products to in/out operands
// costs a v_mov each).
// Returns, in lane i = (b3 b2 b1 b0) of a row, the sum row10_index(i) names.
// ---------------------------------------------------------------------------------------------------------
struct RowWeights { float X, ks, kg; };   // lane constants: x about the wave's block centre, and the y-weight patterns (see above)

__device__ __forceinline__ RowWeights row_weights(const int lane)
{
    const int r = lane >> 4, i = lane & 15, bank = i >> 2, b1 = (i >> 1) & 1;
    RowWeights k;
    k.X = (float)(((r & 1) << 2) + (i >> 2)) - 3.5f;
    const float y0 = (float)((r >> 1) << 2) - 3.5f;
    const float Y = y0 + (float)(i & 3), Yp = y0 + (float)((i & 3) ^ 2);      // own y and that of the xor2 partner
    auto Ka = [&](float y) { return bank == 1 ? y * y : (bank == 3 ? 0.f : 1.f); };      // weights of the sums kept on b1 = 0
    auto Kb = [&](float y) { return (bank & 1) ? 0.f : y; };                              // ... on b1 = 1
    k.ks = b1 ? Kb(Y) : Ka(Y);
    k.kg = b1 ? Kb(Yp) : Ka(Yp);           // applied to the PARTNER's value where it arrives
    return k;
}

template <bool NINE>          // NINE: no depth cotangent - the seventh value is not reduced
__device__ __forceinline__ float reduce_moments_row(const float e, const float ex, const float exx, const float c0, const float c1,
                                                    const float c2, const float cd, const RowWeights &k)
{
    float a, b, c;
#define T4D_RED_X                                                                                     \
        "s_nop 1\n\t"                                                                                 \
        "v_add_f32_dpp %[a], %[v0], %[v0] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"                   \
        "v_add_f32_dpp %[b], %[v2], %[v2] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"                   \
        "v_add_f32_dpp %[c], %[v4], %[v4] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"                   \
        "v_add_f32_dpp %[a], %[v1], %[v1] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                   \
        "v_add_f32_dpp %[b], %[v3], %[v3] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"                   \
        "v_add_f32_dpp %[c], %[v5], %[v5] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
#define T4D_RED_X4                                                                                    \
        "v_add_f32_dpp %[a], %[a], %[a] row_shl:4 row_mask:0xf bank_mask:0x5\n\t"                     \
        "v_add_f32_dpp %[a], %[b], %[b] row_shr:4 row_mask:0xf bank_mask:0xa\n\t"                     \
        "v_add_f32_dpp %[b], %[c], %[c] row_shl:4 row_mask:0xf bank_mask:0x5\n\t"                     \
        "v_add_f32_dpp %[b], %[c], %[c] row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
#define T4D_RED_OUT [a] "=&v"(a), [b] "=&v"(b), [c] "=&v"(c)
#define T4D_RED_IN [v0] "v"(exx), [v1] "v"(c0), [v2] "v"(c1), [v3] "v"(c2), [v4] "v"(e), [v5] "v"(ex), [ks] "v"(k.ks), [kg] "v"(k.kg), \
                   [m0] "s"(0xaaaaaaaaaaaaaaaaull)
    if (NINE) {
        asm(T4D_RED_X T4D_RED_X4
            "v_add_f32_dpp %[a], %[a], %[a] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_mul_f32_e32 %[c], %[b], %[ks]\n\t"
            "v_fmac_f32_dpp %[c], %[b], %[kg] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_e64 %[b], %[a], %[c], %[m0]\n\t"             /* b0 ? moments : others  (goes to the partner) */
            "v_cndmask_b32_e64 %[c], %[c], %[a], %[m0]\n\t"             /* b0 ? others : moments  (stays)               */
            "s_nop 0\n\t"
            "v_add_f32_dpp %[c], %[b], %[c] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
            : T4D_RED_OUT : T4D_RED_IN);
        return c;
    } else {
        float d;                // the x-sum of w dL/dD, in every bank; folded in at xor2 with selects: the lanes with b1 = 1 keep it
        asm(T4D_RED_X
            "v_add_f32_dpp %[d], %[v6], %[v6] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
            T4D_RED_X4
            "v_add_f32_dpp %[d], %[d], %[d] row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_e64 %[c], %[d], %[a], %[m1]\n\t"             /* b1 ? others : depth  (goes to the partner) */
            "v_cndmask_b32_e64 %[d], %[a], %[d], %[m1]\n\t"             /* b1 ? depth : others  (stays)               */
            "v_mul_f32_e32 %[a], %[b], %[ks]\n\t"
            "v_fmac_f32_dpp %[a], %[b], %[kg] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_add_f32_dpp %[d], %[c], %[d] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_cndmask_b32_e64 %[b], %[d], %[a], %[m0]\n\t"             /* b0 ? moments : others  (goes to the partner) */
            "v_cndmask_b32_e64 %[a], %[a], %[d], %[m0]\n\t"             /* b0 ? others : moments  (stays)               */
            "s_nop 0\n\t"
            "v_add_f32_dpp %[a], %[b], %[a] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
            : T4D_RED_OUT, [d] "=&v"(d) : T4D_RED_IN, [v6] "v"(cd), [m1] "s"(0xccccccccccccccccull));
        return a;
    }
#undef T4D_RED_X
#undef T4D_RED_X4
#undef T4D_RED_OUT
#undef T4D_RED_IN
}

// which of the ten sums (slab entry / record order) lane i of a row holds after reduce_moments_row; -1 = none (or a duplicate)
constexpr int row10_index(const int lane)
{
    const int b0 = lane & 1, b1 = (lane >> 1) & 1, bank = (lane >> 2) & 3;
    if (!b0) {
        if (bank == 0) return b1 ? 2 : 0;        // M01 : M00
        if (bank == 1) return b1 ? -1 : 5;       //       M02
        if (bank == 2) return b1 ? 4 : 1;        // M11 : M10
        return -1;
    }
    if (!b1) return bank == 0 ? 3 : (bank == 1 ? 7 : (bank == 2 ? 6 : 8));      // M20, sum w dL/dC1, C0, C2
    return bank == 0 ? 9 : -1;                                                  // sum w dL/dD (with a depth cotangent only)
}

// row10_index of the sixteen lanes of a row as a table of 4-bit entries (index + 1; 0 = none): what a lane reads at kernel entry.
// Evaluated there as nested conditions it was forty vector instructions under exec masks, once per workgroup.
template <bool NINE>          // NINE: as reduce_moments_row - the lane that would hold sum 9 holds nothing
constexpr unsigned long long row10_table()
{
    unsigned long long t = 0ull;
    for (int i = 0; i < 16; i++) {
        const int s = row10_index(i);
        t |= (unsigned long long)((NINE && s == 9) ? 0 : s + 1) << (4 * i);
    }
    return t;
}

// A slab entry's raw moments about the origin o become the record's sums about the splat centre; p = centre - o.
//   sum e dx = p.x M00 - M10    sum e dx dx = p.x^2 M00 - 2 p.x M10 + M20    sum e dx dy = p.x p.y M00 - p.x M01 - p.y M10 + M11
// The shift cancels, and a record must stay accurate RELATIVE TO ITSELF where everything in it is tiny: a splat whose opacity is
// within a few ulp of 1/255 is drawn on the one pixel its centre sits on, |d| ~ 1e-6, and every gradient of such a scene is made
// of sums like e d.  Two things keep those exact: e enters the moments with 18 significant bits (moment_e), so that its products
// with X, X^2, Y, Y^2, X Y (at most 6 bits) are exact floats and a sum with a single contributing pixel IS e X^a Y^b; and the
// shift is evaluated in double precision, factored so that every step but the last fused multiply-add is exact for such a sum:
// p.x M00 - M10 = e dx, p.x M10 - M20 = e X dx, and p.x (e dx) - (e X dx) = e dx dx rounds once.  Sums over many pixels carry
// float rounding of the moments instead, about 1e-5 of the largest entry at worst (tools/experiments/model_bwd_moment_numerics.py).
// Once per staged splat and wave: noise in the instruction count.
__device__ __forceinline__ void moments_about_centre(float (&m)[10], const float pxf, const float pyf)
{
    const double px = pxf, py = pyf, M00 = m[0], M10 = m[1], M01 = m[2], M20 = m[3], M11 = m[4], M02 = m[5];
    const double sx = fma(px, M00, -M10), sy = fma(py, M00, -M01);
    m[1] = (float)sx; m[2] = (float)sy;
    m[3] = (float)fma(px, sx, -fma(px, M10, -M20));
    m[4] = (float)fma(px, sy, -fma(py, M10, -M11));
    m[5] = (float)fma(py, sy, -fma(py, M01, -M02));
}

// e as the moments take it: 18 significant bits (truncated), see moments_about_centre
__device__ __forceinline__ float moment_e(const float e) { return __uint_as_float(__float_as_uint(e) & 0xffffffc0u); }

__device__ __forceinline__ uint32_t row_max_u32(uint32_t v)      // every lane gets the maximum over its 16-lane row
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true));   // row_half_mirror
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true));   // row_mirror
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// A.4 backward replay.  No global atomics: one kGP-float record per (Gaussian,tile) pair.
// record (raw sums over the tile's pixels, e = G * dL/dalpha, d = splat centre - pixel):
//   [0] sum e   [1,2] sum e*d   [3,4,5] sum e*dx*dx, e*dx*dy, e*dy*dy   [6,7,8] sum alpha*T*dL/dC   [9] sum alpha*T*dL/dD
// Inside the workgroup every wave owns an LDS slab of ten sums per staged splat - [1..5] there as RAW moments about the centre of
// the wave's 8x8 block (reduce_moments_row), shifted to the splat centre when the record is written; a row's reduced sums are added to it
// by plain read-add-write (no LDS float atomics: they retire ~3 cycles per lane here), rows that hold the same splat
// in the same step taking turns, and the slabs of the four waves are summed in wave order when the batch is written
// out.  Every addition order is fixed, so the gradients are bit-reproducible.
// ---------------------------------------------------------------------------------------------------------
// DA = the caller supplied dL/ddepth and/or dL/dalpha.  Topo4D discards depth and alpha (train.py:307), so its backward
// runs the DA = false instantiation, which carries neither the two extra suffix accumulators nor their products.
#ifndef T4D_BWD_WAVES
#define T4D_BWD_WAVES 5                  // = workgroups per CU (30.8 KB of LDS each); 4 is 14 % slower, 6 spills (round-3 sweep)
#endif
#ifndef T4D_SEG_WAVES
#define T4D_SEG_WAVES 5          // (4 = 128 registers, no spills: config-2 scene 1 view 36.3 us, 3 views 64.4; 5: 37.4 / 59.3, 6 views 104.7 -> 95.6)
#endif
#ifndef T4D_BWD_DA_WAVES
#define T4D_BWD_DA_WAVES T4D_BWD_WAVES
#endif
#define T4D_BWD_NW (LAT ? 2 : (SEGN != 0 ? T4D_SEG_WAVES : (DA ? T4D_BWD_DA_WAVES : T4D_BWD_WAVES)))
#define T4D_BWD_ATTR __attribute__((amdgpu_waves_per_eu(LAT ? 1 : T4D_BWD_NW, T4D_BWD_NW)))
constexpr int kAcc = 10;                 // sums per (wave, staged splat) slab entry
// (kEmptySpan, the tiles per spare workgroup of the empty-tile share of cotangent_dot: t4d_raster_plan.h)
__host__ __device__ inline uint32_t empty_spans(const int T) { return (uint32_t)(T + kEmptySpan - 1) / kEmptySpan; }      // spare workgroups per view
// LAT: the latency build (see k_render_fwd): one slab per DPP ROW instead of one per wave (82 KB of LDS: one workgroup per CU
// is all such a launch has anyway), so two rows holding the same splat in the same step never meet and the conflict
// detection and its branches disappear; the gradient arithmetic is predicated with selects instead of an exec-masked region,
// which lets the compiler interleave the four steps of a group.
// SEG: the segmented backward of small launches (kSeg): a work item is ONE segment of a tile list - workgroup b takes slot b of
// the slot table - and the replay starts from the forward's snapshot at the segment's far end instead of from the list's end.
// LONG: the two launches of a big one-view launch (seg_mode 2) - the whole-tile build (SEGN == 0) leaves out the tiles that own
// segments, the segmented build (SEGN != 0) walks the mostly empty slot table with a fixed number of workgroups.  A template
// parameter so that every other launch shape runs the code it always ran (a one-view launch of Topo4D's size lasts 23 us: the same
// tests at run time in its prologue cost 0.8-1.6 us).
template <bool DA, bool LAT, int SEGN, bool LONG = false>
__global__ __launch_bounds__(kBlock) T4D_BWD_ATTR void k_render_bwd(const KP kp)
{
    // T4D_REGION entry
    constexpr bool SEG = SEGN != 0;
    // a segment is ONE staged batch: the segmented build stages SEGN splats per round (128, or 64 for a one-view launch), the
    // whole-tile builds kBwdBatch (these shadow the globals inside the kernel)
    constexpr int kSeg = SEG ? SEGN : ::kSeg;
    constexpr int kBwdBatch = SEG ? SEGN : ::kBwdBatch;
    constexpr int kSlabs = LAT ? 16 : 4;
    constexpr int kChunks = (kBwdBatch + 63) / 64;
    constexpr int kListStride = kBwdBatch + 4;
    // A staged splat is ONE 40-byte record - scaled conic + opacity (16) | rgb + depth (16) | xy (8) - exactly as long as a slab
    // entry (ten floats), and list entries are slot * 40: the byte offset of BOTH, so a step spends no vector instruction on
    // addresses (records are read as 8-byte words: a 40-byte stride keeps them 8- but not 16-byte aligned).
    constexpr int kEnt = 40;
    static_assert(kBwdBatch % 64 == 0, "staged slots come in chunks of one per lane");
    static_assert(kGP == kAcc, "the slab entry and the scratch record hold the same ten sums");
    static_assert(kAcc * 4 == kEnt, "a slab entry and a staged record must have the same stride");
    // One struct, so that the layout is ours: the staged records sit at LDS offset 0 and the replay's paired 8-byte reads reach
    // them with immediate offsets (behind the slabs, at 20 KiB, every step paid a vector add for the address).
    struct __attribute__((aligned(16))) Shared {
        unsigned char rec[(kBwdBatch + 1) * kEnt];
        float acc[kSlabs][kBwdBatch + 1][kAcc];                 // + the null splat's (never read) row
        unsigned short list[4][4][kListStride];
        float cut_r2[kChunks * 64];                             // cut-off of every staged splat (< 0: none in this slot)
        uint32_t pair[kBwdBatch];
        uint32_t wmax[4];
    };
    static_assert(((kBwdBatch + 1) * kEnt) % 8 == 0 && (sizeof(float) * kSlabs * (kBwdBatch + 1) * kAcc) % 8 == 0 &&
                  (sizeof(unsigned short) * 16 * kListStride) % 8 == 0, "8-byte members must stay 8-byte aligned");
    __shared__ Shared sh;
    auto &s_rec = sh.rec;
    auto &s_pair = sh.pair;
    auto &s_acc = sh.acc;
    auto &s_r2 = sh.cut_r2;
    auto &s_wmax = sh.wmax;
    auto &s_list = sh.list;
    constexpr int kNull = kBwdBatch;
    // PF (the throughput build on whole tiles): a batch is staged by the waves that write no records - waves kStageWave0 and up
    // request batch bi - 1 while the waves below them write batch bi out, and commit it to LDS behind the barrier that ends
    // the write-out (which reads the centres and pair slots of batch bi).  Staged one after the other on the same two waves,
    // the new batch's loads queued behind the record stores (one in-order counter for both), the other two waves idled
    // through both phases, and all of the per-batch vector work sat on the SIMDs of waves 0 and 1.  The latency and the
    // segmented builds stage one batch per item or have the chip's LDS to themselves: they stage where they always did.
    constexpr bool PF = !LAT && !SEG;
    constexpr int kStageWave0 = kBlock / 64 - kChunks;          // first staging wave of the PF build
    static_assert(!PF || (kStageWave0 >= kChunks && kBwdBatch == kChunks * 64), "staging and write-out waves are disjoint, one lane per slot");
    // what a staging lane holds of its splat between request and commit
    struct Staged { unsigned long long key; float r2; float2 p; int rad; uint32_t po; float4 c; float c0, c1, c2; };

    // Whole tiles: the items are ordered by length, so a tile workgroup whose FIRST item is empty has nothing to do at all (a
    // quarter of a config-2 launch, two thirds of config 4's): it leaves here, before the slab clear and before the kernel's
    // wave-uniform state is set up.  The item is kept for the first round of the tile loop.
    uint4 it = make_uint4(0u, 0u, 0u, 0u);
    if (!SEG && blockIdx.x < kp.tile_blocks) {           // (tile_blocks <= V T: tile_grid)
        it = kp.items[blockIdx.x];
        if (it.z == 0u) return;
    }
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, row = lane >> 4;      // wave: a scalar
    // without a depth cotangent the seventh value is not reduced (reduce_moments_row<true>): the lane that would hold sum 9 holds a
    // second copy of sum 3 and must stay out
    constexpr unsigned long long kSlotTable = row10_table<!DA>();
    const int my_slot = (int)((uint32_t)(kSlotTable >> (4 * (lane & 15))) & 15u) - 1;
    const RowWeights rw = row_weights(lane);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < kEnt / 8; k++) reinterpret_cast<float2 *>(s_rec + kNull * kEnt)[k] = make_float2(0.f, 0.f);
    }
    if (blockIdx.x >= kp.tile_blocks) {
        // Spare workgroups behind the tile workgroups, launched only when the caller asked for <outputs, cotangents>: the EMPTY
        // tiles' share.  An empty tile shows the background at T = 1, so on black (Topo4D: helpers.py setup_camera, bg = 0)
        // there is nothing to add and the workgroup leaves at once; otherwise it sums bg . dL/dC over its kEmptySpan tiles.
        const uint32_t spans = empty_spans(kp.T);
        const uint32_t j = blockIdx.x - kp.tile_blocks;
        const int v = (int)t4d_div(j, kp.div_spans), t0 = (int)(j - (uint32_t)v * spans) * kEmptySpan;
        const float *vb = kp.views + (size_t)v * T4D_VIEW_FLOATS + 35;
        const float b0 = vb[0], b1 = vb[1], b2 = vb[2];
        if (b0 == 0.f && b1 == 0.f && b2 == 0.f) return;
        const size_t HWe = (size_t)kp.H * kp.W;
        const float *dc = kp.dL_dcolor + (size_t)v * 3 * HWe;
        for (int t = t0; t < min(t0 + kEmptySpan, kp.T); t++) {
            if (kp.tile_count[(size_t)v * kp.T + t] != 0u) continue;           // workgroup-uniform
            const int ty = (int)t4d_div((uint32_t)t, kp.div_gx), tx = t - ty * kp.gx;
            int ex, ey;
            tile_pixel(tid, tx, ty, ex, ey);
            float d = 0.f;
            if (ex < kp.W && ey < kp.H) {
                const size_t pe = (size_t)ey * kp.W + ex;
                d = fmaf(b0, dc[pe], fmaf(b1, dc[HWe + pe], b2 * dc[2 * HWe + pe]));
            }
            d = wave_sum_to_lane63(d);
            if (lane == 63) kp.tile_dot[((size_t)v * kp.T + t) * 4 + wave] = d;
        }
        return;
    }
    if (SEG && !LONG) {
        it = kp.slot_tab[blockIdx.x];                // one slot per workgroup; most slots hold no segment
        if (it.w == 0u) return;
    }
    {
        // slabs are all-zero between batches.  8 bytes per store at compile-time offsets: the counted loop over single floats was
        // 20 stores and 60 vector instructions of index arithmetic per thread, once per workgroup - which is once per tile
        constexpr int kPairs = kSlabs * (kBwdBatch + 1) * kAcc / 2;
        static_assert(kAcc % 2 == 0, "slab entries are cleared as float2");
        float2 *a2 = reinterpret_cast<float2 *>(&s_acc[0][0][0]);
#pragma unroll
        for (int i = 0; i < kPairs / kBlock; i++) a2[i * kBlock + tid] = make_float2(0.f, 0.f);
        if (tid < kPairs % kBlock) a2[(kPairs / kBlock) * kBlock + tid] = make_float2(0.f, 0.f);
    }
    // work items: the length-ordered tile list (whole tiles), ONE slot of the slot table (segments of a small launch), or a strided
    // walk over the mostly empty table of a big one-view launch (LONG)
    // (LONG segments: entries k, k + grid, ... of the compact list of live segments - the table itself is mostly empty, and a
    // strided walk over it, even with one gather per 64 slots, cost 20-40 us and dealt the segments out unevenly)
    // T4D_REGION tile prologue
    for (uint32_t item = blockIdx.x; item < (SEG ? (LONG ? kp.status->live_segments : blockIdx.x + 1u) : (uint32_t)(kp.V * kp.T)); item += kp.tile_blocks) {
    if (SEG && LONG) it = kp.slot_tab[kp.live[item]];
    if (!SEG && item != blockIdx.x) it = kp.items[item];
    const int seg_j = SEG ? (int)(it.w & 0x7fffffffu) : 0;           // this item's segment: list positions [seg_j kSeg, (seg_j + 1) kSeg)
    const int v = (int)(it.x >> 20), t_ = (int)(it.x & 0xfffffu);
    const int ty = (int)t4d_div((uint32_t)t_, kp.div_gx), tx = t_ - ty * kp.gx;
    const uint32_t off = it.y, n = it.z;
    if (n == 0) break;                                             // ordered by length: only empty tiles remain
    // a big one-view launch: the tiles the forward cut into segments (it wrote their slot-table entries with their snapshots) are
    // the segmented launch's
    if (!SEG && LONG && n >= kp.seg_min_pairs &&
        kp.slot_tab[(size_t)v * kp.slots_per_view + seg_slot0(kp, off, (uint32_t)t_)].w != 0u) continue;
    const kp_kernarg_p kt = kernarg_kp();          // this tile's reads of the parameter block: scalar loads here, nothing kept across tiles
    const unsigned long long *keys = kt->keys + (size_t)v * kt->cap + off;
    const float *r2_in = kt->cut_r2 + (size_t)v * kt->cap + off;
    const float2 *xy = kt->xy + (size_t)v * kt->P;
    const float4 *co = kt->conic_opacity + (size_t)v * kt->P;
    const float *rgb = kt->shs ? kt->rgb + (size_t)v * kt->P * 3 : kt->colors_precomp + 3 * param_row0(kp, v);
    const int32_t *radii = kt->radii + (size_t)v * kt->P;
    const uint32_t *pair_off = kt->pair_off + (size_t)v * kt->P;
    float2 *grad_pair = reinterpret_cast<float2 *>(kt->grad_pair) + (size_t)v * kt->cap * (kGP / 2);
    const float *vr = kt->views + (size_t)v * T4D_VIEW_FLOATS;

    // Staging in two halves.  stage_request_key + stage_request: lane t asks for everything slot t of the batch at list position
    // lo needs - the key and the kept cut-off, and behind the key ONE level of dependent loads: everything a splat needs is
    // requested before any of it is used (centre and radius, then the pair slot, then conic and colour were four dependent
    // round trips per batch while the other waves waited at the barrier).  stage_commit: the same lane turns what arrived
    // into the staged record, the cut-off and the pair slot in LDS.  `want` = the batch will be walked (or may be: the tile's
    // first batch is requested before that is known); conic, colour and cut-off are loaded only then, and used only if the
    // batch is live.
    // stage_commit reads of a Staged exactly what stage_request loaded under the same conditions; nothing else is set.  A
    // Staged starts out as stage_none leaves it: every member defined by an empty asm statement - no instruction, but a
    // definition on every path.  Left uninitialised, a member keeps "whatever it held in the previous tile or batch" on the
    // waves that request nothing, and those fourteen registers stay allocated across the walk (84 bytes of scratch).
    auto stage_none = [](Staged &s) __attribute__((always_inline)) {
        asm("" : "=v"(s.key), "=v"(s.r2), "=v"(s.p.x), "=v"(s.p.y), "=v"(s.rad), "=v"(s.po));
        asm("" : "=v"(s.c.x), "=v"(s.c.y), "=v"(s.c.z), "=v"(s.c.w), "=v"(s.c0), "=v"(s.c1), "=v"(s.c2));
    };
    // (the array bases are read from the parameter block again, scalar loads on the requesting waves: held in scalar
    // registers from the tile's prologue to the last request they pushed five other scalars out into vector lanes)
    auto stage_request_key = [&](Staged &s, const int t, const uint32_t lo, const int cnt, const bool want) __attribute__((always_inline)) {
        const kp_kernarg_p kq = kernarg_kp();
        const size_t at = (size_t)v * kq->cap + off + lo;
        if (t < cnt) {
            s.key = kq->keys[at + t];
            if (want) s.r2 = kq->cut_r2[at + t];                               // = cutoff_radius2(c), kept by the forward
        }
    };
    auto stage_request = [&](Staged &s, const int t, const int cnt, const bool want) __attribute__((always_inline)) {
        const kp_kernarg_p kq = kernarg_kp();
        const size_t vP = (size_t)v * kq->P;
        if (t < cnt) {
            const uint32_t g = (uint32_t)s.key;
            if (g < (uint32_t)kp.P) {                                          // stale entries after an overflow are skipped
                s.p = kq->xy[vP + g];
                s.rad = kq->radii[vP + g];
                s.po = kq->pair_off[vP + g];
                if (want) { s.c = kq->conic_opacity[vP + g]; s.c0 = rgb[3 * (size_t)g]; s.c1 = rgb[3 * (size_t)g + 1]; s.c2 = rgb[3 * (size_t)g + 2]; }
            }
        }
    };
    auto stage_commit = [&](const Staged &s, const int t, const int cnt, const bool live) __attribute__((always_inline)) {
        if (t < cnt) s_pair[t] = 0xffffffffu;
        float r2 = -1.f;                                 // a slot without a splat touches nothing ...
        float2 p = make_float2(0.f, 0.f);                // ... and holds a finite centre
        if (t < cnt && (uint32_t)s.key < (uint32_t)kp.P) {
            p = s.p;
            int x0, y0, x1, y1;
            tile_rect(s.p.x, s.p.y, s.rad, kp.gx, kp.gy, x0, y0, x1, y1);
            const int local = (ty - y0) * (x1 - x0) + (tx - x0);
            s_pair[t] = (tx >= x0 && tx < x1 && ty >= y0 && ty < y1) ? s.po + (uint32_t)local : 0xffffffffu;
            if (live) {
                const float4 q4 = scale_conic(s.c);
                float2 *rec = reinterpret_cast<float2 *>(s_rec + t * kEnt);
                rec[0] = make_float2(q4.x, q4.y); rec[1] = make_float2(q4.z, q4.w);
                rec[2] = make_float2(s.c0, s.c1);
                rec[3] = make_float2(s.c2, __uint_as_float((uint32_t)(s.key >> 32)));
                r2 = s.r2;
            }
        }
        if (live) {
            reinterpret_cast<float2 *>(s_rec + t * kEnt)[4] = p;
            s_r2[t] = r2;
        }
    };
    const int nb = (int)((n + kBwdBatch - 1) / kBwdBatch);
    const int stage_t = tid - kStageWave0 * 64;          // PF: the slot a lane of the staging waves stages
    Staged st_first;
    if (PF) stage_none(st_first);
    // T4D_REGION staging
    if (PF && wave >= kStageWave0) {
        // the tile's first batch (its last): the keys go out ahead of the pixel-state loads below, what hangs on the keys
        // behind them, so that the gathers are in flight under the row maxima and the barrier that follow.  (The memory counter
        // is in order, and as compiled the wait for the keys also takes in the pixel loads - they sit in a divergent branch,
        // and the wait count at the join is the conservative one: keys and pixel state share one round trip, the gathers are
        // the second.)  Whether the batch is live is known only behind that barrier.
        const uint32_t lo0 = (uint32_t)(nb - 1) * kBwdBatch;
        stage_request_key(st_first, stage_t, lo0, (int)(n - lo0), true);
    }
    // T4D_REGION tile prologue

    int px, py;
    tile_pixel_bwd(tid, tx, ty, px, py);
    const bool inside = px < kt->W && py < kt->H;
    const v2f pix_f = { (float)px, (float)py };
    const size_t HW = (size_t)kt->H * kt->W, pix = (size_t)py * kt->W + px;

    float T_final = 0.f, dp0 = 0.f, dp1 = 0.f, dp2 = 0.f, ddep = 0.f, dalp = 0.f;
    uint32_t last_contributor = 0;
    if (inside) {
        T_final = kt->final_T[(size_t)v * HW + pix];
        last_contributor = kt->n_contrib[(size_t)v * HW + pix];
        const float *dc = kt->dL_dcolor + (size_t)v * 3 * HW;
        dp0 = dc[pix]; dp1 = dc[HW + pix]; dp2 = dc[2 * HW + pix];
        if (DA && kt->dL_ddepth) ddep = kt->dL_ddepth[(size_t)v * HW + pix];
        if (DA && kt->dL_dalpha) dalp = kt->dL_dalpha[(size_t)v * HW + pix];
    }
    // T4D_REGION staging
    if (PF && wave >= kStageWave0) stage_request(st_first, stage_t, (int)(n - (uint32_t)(nb - 1) * kBwdBatch), true);
    // T4D_REGION tile prologue
    const v2f dp01 = { dp0, dp1 };
    float T = T_final;
    // Suffix state of the replay.  Upstream keeps one running "colour behind me" per channel (+ depth, + alpha) and dots
    // it with dL/dpixel afterwards; the recursion is linear, so the dot product is taken FIRST and a single scalar is
    // carried:  q_i = c_i . dL/dC (+ depth_i dL/dD + dL/dAlpha),  acc <- alpha_i q_i + (1 - alpha_i) acc  once splat i is done
    // (upstream applies the same update lazily, at the next contributor).
    // The BACKGROUND is the splat behind all others (colour bg, alpha 1): the recursion starts from its q = bg . dL/dC instead of
    // from zero.  Upstream starts from zero and subtracts T_final / (1 - alpha_i) * (bg . dL/dC) from every dL/dalpha_i; with
    // acc' = acc + T_final (bg . dL/dC) / T_i (T_i = transmittance in front of splat i) both the update acc' <- alpha q + (1 - alpha) acc'
    // and dL/dalpha_i = (q_i - acc') T_i hold exactly - one multiply and one fused multiply-add less per step, and for a black
    // background (Topo4D: helpers.py setup_camera, bg = 0) the same bits as before.
    float acc = vr[35] * dp0 + vr[36] * dp1 + vr[37] * dp2;
    if (SEG && seg_j + 1 < nb) {
        // A segment that does not end at the list's end starts from the forward's snapshot at position p = (seg_j + 1) kSeg:
        // T = the transmittance in front of p, acc = the colour behind p as the recursion would hold it there,
        // ((C_final - C_prefix(p)) . dL/dC (+ depth and alpha terms) + T_final bg . dL/dC) / T(p).  A pixel whose last contributor
        // lies before p has its final state at p: exactly the start values above (the forward writes no snapshot for a
        // finished wave, so nothing is read for such a pixel).
        const uint32_t p = (uint32_t)(seg_j + 1) * kSeg;
        if (last_contributor > p) {
            const float *sb = kp.snap + ((size_t)v * kp.slots_per_view + seg_slot0(kp, off, (uint32_t)t_)) * (kSnapFloats * kBlock) + fwd_thread_of(tid);
            const float *sp = sb + (size_t)seg_j * (kSnapFloats * kBlock), *sf = sb + (size_t)(nb - 1) * (kSnapFloats * kBlock);
            const float Tp = sp[0];
            float suf = fmaf(sf[kBlock] - sp[kBlock], dp0, fmaf(sf[2 * kBlock] - sp[2 * kBlock], dp1, (sf[3 * kBlock] - sp[3 * kBlock]) * dp2));
            if (DA) suf = fmaf(sf[4 * kBlock] - sp[4 * kBlock], ddep, suf) + (Tp - T_final) * dalp;
            acc = fmaf(T_final, acc, suf) / Tp;
            T = Tp;
        }
    }

    const uint32_t rmax_v = row_max_u32(last_contributor);
    uint32_t row_max[4];
#pragma unroll
    for (int r = 0; r < 4; r++) row_max[r] = lane_value(rmax_v, 16 * r);
    const uint32_t wave_max = max(max(row_max[0], row_max[1]), max(row_max[2], row_max[3]));
    if (lane == 0) s_wmax[wave] = wave_max;
    __syncthreads();
    const uint32_t tile_max = max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3]));
    // T4D_REGION staging
    if (PF && wave >= kStageWave0) {
        const uint32_t lo0 = (uint32_t)(nb - 1) * kBwdBatch;
        stage_commit(st_first, stage_t, (int)(n - lo0), lo0 < tile_max);
    }

    for (int bi = SEG ? seg_j : nb - 1; bi >= (SEG ? seg_j : 0); bi--) {
        const uint32_t lo = (uint32_t)bi * kBwdBatch;
        const int cnt = (int)min((uint32_t)kBwdBatch, n - lo);
        const bool live = lo < tile_max;      // workgroup-uniform
        // T4D_REGION staging
        // ---- stage ----
        // (PF: this batch was staged behind the previous write-out, or in the tile's prologue)
        if (!PF && tid < cnt) s_pair[tid] = 0xffffffffu;
        if (!PF && tid < kChunks * 64) {
            float r2 = -1.f;                                 // a slot without a splat touches nothing ...
            float2 p = make_float2(0.f, 0.f);                // ... and holds a finite centre
            if (tid < cnt) {
                // ONE level of dependent loads behind the key: everything a splat needs is requested before any of it is used
                // (as the code was written - centre and radius, then the pair slot, then conic and colour - the staging waves went
                // through four dependent round trips per batch while the other waves waited at the barrier)
                const unsigned long long key = keys[lo + tid];
                const float r2_kept = live ? r2_in[lo + tid] : -1.f;               // = cutoff_radius2(c), kept by the forward
                const uint32_t g = (uint32_t)key;
                if (g < (uint32_t)kp.P) {                                          // stale entries after an overflow are skipped
                    const float2 pg = xy[g];
                    const int rad = radii[g];
                    const uint32_t po = pair_off[g];
                    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
                    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
                    if (live) { c = co[g]; c0 = rgb[3 * (size_t)g]; c1 = rgb[3 * (size_t)g + 1]; c2 = rgb[3 * (size_t)g + 2]; }
                    p = pg;
                    int x0, y0, x1, y1;
                    tile_rect(pg.x, pg.y, rad, kp.gx, kp.gy, x0, y0, x1, y1);
                    const int local = (ty - y0) * (x1 - x0) + (tx - x0);
                    s_pair[tid] = (tx >= x0 && tx < x1 && ty >= y0 && ty < y1) ? po + (uint32_t)local : 0xffffffffu;
                    if (live) {
                        const float4 q4 = scale_conic(c);
                        float2 *rec = reinterpret_cast<float2 *>(s_rec + tid * kEnt);
                        rec[0] = make_float2(q4.x, q4.y); rec[1] = make_float2(q4.z, q4.w);
                        rec[2] = make_float2(c0, c1);
                        rec[3] = make_float2(c2, __uint_as_float((uint32_t)(key >> 32)));
                        r2 = r2_kept;
                    }
                }
            }
            if (live) {
                reinterpret_cast<float2 *>(s_rec + tid * kEnt)[4] = p;
                s_r2[tid] = r2;
            }
        }
        __syncthreads();
        if (live) {
            // T4D_REGION masks + lists
            // which of the staged splats can touch which of this wave's four sub-blocks: the forward's test, on the forward's numbers
            unsigned long long mt[4][kChunks];
#pragma unroll
            for (int c2 = 0; c2 < kChunks; c2++) {
                const int slot = (c2 << 6) + lane;
                unsigned long long mc[4] = { 0ull, 0ull, 0ull, 0ull };
                if ((c2 << 6) < cnt)                         // wave-uniform
                    wave_touch_masks(reinterpret_cast<const float2 *>(s_rec + slot * kEnt)[4], s_r2[slot], tx, ty, wave, mc);
#pragma unroll
                for (int r = 0; r < 4; r++) mt[r][c2] = mc[r];
            }
            // every row walks as many steps as the wave's longest list, four at a time (and the walk fetches one group ahead): the
            // lists are null wherever no entry is written.  The block sits 8 bytes off a 16-byte boundary: 8-byte stores.
            static_assert(offsetof(Shared, list) % 8 == 0 && (sizeof(unsigned short) * 4 * kListStride) % 8 == 0, "8-byte stores");
            prefill_visit_lists<4 * kListStride * 2, uint2>(&s_list[wave][0][0], lane, (unsigned short)(kNull * kEnt));
            int nsteps = 0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                unsigned long long m[kChunks];
#pragma unroll
                for (int c2 = 0; c2 < kChunks; c2++) {
                    m[c2] = mt[r][c2];
                    // positions at or beyond the row's last contributor cannot matter: drop them from the mask
                    const uint32_t base = lo + ((uint32_t)c2 << 6);
                    if (row_max[r] <= base) m[c2] = 0;
                    else if (row_max[r] - base < 64u) m[c2] &= (1ull << (row_max[r] - base)) - 1ull;
                }
                build_visit_list<kChunks, true, kEnt>(m, s_list[wave][r], lane);   // back to front
                nsteps = uniform_max(nsteps, visit_count(m));
            }
            __builtin_amdgcn_wave_barrier();
            // Steps in which two rows of this wave hold the SAME splat (about one in five) must not do their slab updates in
            // one instruction; they are found here, 64 steps per pass, so that the replay only tests a scalar bit.
            unsigned long long conflict[kChunks];
#pragma unroll
            for (int c2 = 0; c2 < kChunks; c2++) {
                conflict[c2] = 0ull;
                if (!LAT && (c2 << 6) < nsteps) {
                    const int st = (c2 << 6) + lane;
                    const unsigned short *l0 = s_list[wave][0];
                    const uint32_t e0 = l0[st], e1 = l0[kListStride + st], e2 = l0[2 * kListStride + st], e3 = l0[3 * kListStride + st];
                    const uint32_t nul = (uint32_t)(kNull * kEnt);
                    const bool same = st < nsteps && ((e0 == e1 && e0 != nul) || (e0 == e2 && e0 != nul) || (e0 == e3 && e0 != nul) ||
                                                      (e1 == e2 && e1 != nul) || (e1 == e3 && e1 != nul) || (e2 == e3 && e2 != nul));
                    conflict[c2] = __ballot(same);
                }
            }
            unsigned long long conflict_s[kChunks];           // the same masks, pinned to scalar registers
#pragma unroll
            for (int c2 = 0; c2 < kChunks; c2++) conflict_s[c2] = uniform_u64(conflict[c2]);
            const unsigned short *list = s_list[wave][row];
            const unsigned char *rec_b = s_rec;
            // LAT: lanes that keep no sum write (zeros plus whatever) into distinct floats of the null splat's row of their slab
            unsigned char *slab = LAT ? reinterpret_cast<unsigned char *>(my_slot >= 0 ? &s_acc[wave * 4 + row][0][my_slot]
                                                                                      : &s_acc[wave * 4 + row][kNull][(lane & 15) % kAcc])
                                      : reinterpret_cast<unsigned char *>(&s_acc[wave][0][0] + (my_slot >= 0 ? my_slot : 0));
            const uint32_t slab_and = (!LAT || my_slot >= 0) ? 0xffffffffu : 0u;       // slot-less lanes of the latency build stay on their dummy float
            // entry of the first staged splat this pixel did NOT see in the forward pass (entries are slot * kEnt)
            const int lc_rel = (int)min(last_contributor - min(last_contributor, lo), (uint32_t)kBwdBatch) * kEnt;
            // The loop is arranged so that no LDS round trip sits between dependent instructions: the list entries of the
            // NEXT group are fetched while this group is processed, the colour records are fetched together with the
            // geometry records, and a step's slab value is read BEFORE its arithmetic and written back after it
            // (same wave, program order: the previous step's write is already ahead of the read in the LDS queue).
            // T4D_REGION walk
            uint2 pk = *reinterpret_cast<const uint2 *>(list);
            for (int k = 0; k < nsteps; k += 4) {
                const uint32_t ee[4] = { pk.x & 0xffffu, pk.x >> 16, pk.y & 0xffffu, pk.y >> 16 };
                pk = *reinterpret_cast<const uint2 *>(list + k + 4);          // the lists are padded: always readable
                float Gs[4], alphas[4];
                float4 cds[4];
                bool contribs[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {            // four independent evaluations (ILP)
                    const float2 *rec = reinterpret_cast<const float2 *>(rec_b + ee[u]);
                    const float2 q01 = rec[0], q23 = rec[1], c01 = rec[2], c23 = rec[3];
                    const v2f d = *reinterpret_cast<const v2f *>(rec + 4) - pix_f;
                    cds[u] = make_float4(c01.x, c01.y, c23.x, c23.y);
                    float p2;
                    eval_splat(make_float4(q01.x, q01.y, q23.x, q23.y), d, p2, Gs[u], alphas[u]);
                    contribs[u] = (int)ee[u] < lc_rel && !(p2 > 0.0f) && !(alphas[u] < T4D_ALPHA_MIN);
                }
                const uint32_t cbits = (uint32_t)(conflict_s[kChunks == 1 ? 0 : (k >> 6)] >> (k & 63));
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const bool contrib = contribs[u];
                    const float G = Gs[u], alpha = alphas[u];
                    float *dst = reinterpret_cast<float *>(slab + (LAT ? (ee[u] & slab_and) : ee[u]));
                    const float old = *dst;              // early read of the slab value this step adds to
                    float e = 0.f, w = 0.f;
                    if (LAT) {
                        // the same operations in the same order as the exec-masked region below, on every lane; the selects keep
                        // the state of the lanes that do not contribute
                        const float4 cd = cds[u];
                        const float om = 1.f - alpha;
                        const float inv = __builtin_amdgcn_rcpf(om);
                        const float Tn = T * inv;
                        float q = fmaf(cd.x, dp01.x, fmaf(cd.y, dp01.y, cd.z * dp2));
                        if (DA) q = fmaf(cd.w, ddep, q) + dalp;
                        const float qma = q - acc;
                        const float dL_dalpha = qma * Tn;
                        T = contrib ? Tn : T;
                        w = contrib ? alpha * Tn : 0.f;
                        e = contrib ? G * dL_dalpha : 0.f;
                        acc = contrib ? fmaf(alpha, qma, acc) : acc;
                    } else if (contrib) {
                        // Per lane only what depends on the pixel: e = G * dL/dalpha and its first/second moments about
                        // the splat centre, and w * dL/dC.  Everything that is constant per splat (opacity, conic,
                        // 0.5*W, -0.5 ...) is applied ONCE per Gaussian after all tiles are summed (k_preprocess_bwd).
                        const float4 cd = cds[u];
                        const float om = 1.f - alpha;                              // >= 0.01
                        const float inv = __builtin_amdgcn_rcpf(om);          // (a Newton step on it: +1.9 % of the kernel, no decision depends on it - tools/experiments/README.md)
                        T = T * inv;
                        w = alpha * T;
                        float q = fmaf(cd.x, dp01.x, fmaf(cd.y, dp01.y, cd.z * dp2));
                        if (DA) q = fmaf(cd.w, ddep, q) + dalp;
                        const float qma = q - acc;                                 // acc = the colour behind THIS splat (background included)
                        const float dL_dalpha = qma * T;
                        e = G * dL_dalpha;
                        // ... and now behind the next one towards the eye: alpha q + (1 - alpha) acc as acc + alpha (q - acc), the
                        // difference being at hand (one instruction instead of two; upstream's two-product form rounds differently
                        // in the last bit)
                        acc = fmaf(alpha, qma, acc);
                    }
                    // lanes that do not contribute carry e = w = 0, so their products are exact zeros
                    e = moment_e(e);
                    const float ex = e * rw.X;
                    const v2f wdp = w * dp01;
                    const float tot = reduce_moments_row<!DA>(e, ex, ex * rw.X, wdp.x, wdp.y, w * dp2, DA ? w * ddep : 0.f, rw);
                    // Plain read-add-write into the wave's slab (ds_add_f32 retires ~3 cycles per LANE on this part).  Idle
                    // rows add their zeros to the null splat's row, which nobody reads.
                    const bool add = my_slot >= 0;
                    if (LAT) {
                        *dst = old + tot;                // own slab per row: never a conflict; slot-less lanes hit their dummy float
                    } else if (!((cbits >> u) & 1u)) {
                        if (add) *dst = old + tot;
                    } else {
#pragma unroll
                        for (int rr = 0; rr < 4; rr++) {                 // two rows hold the same splat: one after the other
                            if (add && row == rr) *dst += tot;
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                }
            }
        }
        __syncthreads();
        // the next batch of the tile (always a full one; none behind the tile's first)
        const uint32_t lo_n = lo - (uint32_t)(bi > 0 ? kBwdBatch : 0);
        const int cnt_n = bi > 0 ? kBwdBatch : 0;
        const bool live_n = lo_n < tile_max;
        Staged st;
        if (PF) stage_none(st);
        // T4D_REGION staging
        if (PF && wave >= kStageWave0) {
            // while the other waves write this batch out, the waves that have no record to write request the next one.  Its
            // loads stay in flight across the barrier below - the compiler waits for them where stage_commit uses them - and
            // queue behind no record store: those are the other waves'.
            stage_request_key(st, stage_t, lo_n, cnt_n, live_n);
            stage_request(st, stage_t, cnt_n, live_n);
        } else
        // T4D_REGION write-out
        // ---- write one record per pair (zeros when no wave touched it); fixed wave order => deterministic ----
        if (tid < cnt) {
            float a[10];
#pragma unroll
            for (int k = 0; k < 10; k++) a[k] = 0.f;
            // a batch nobody walked staged nothing: its slabs are zero and stay zero under any (finite) shift
            const float2 pc = live ? reinterpret_cast<const float2 *>(s_rec + tid * kEnt)[4] : make_float2(0.f, 0.f);
#pragma unroll 1
            for (int w = 0; w < 4; w++) {
                // the wave's raw moments (the latency build: of its four rows' slabs), then their shift from the centre of the
                // wave's 8x8 block to the splat centre; both differences below are exact
                // (the first slab is taken as it is, not added to zero: 0 + x is an instruction the compiler must keep for x = -0,
                // ten per wave and trip.  A slab starts at +0 and only ever has sums added to it, so it never holds -0; and a
                // zero's sign could not reach a record anyway: everything below is added to a[], which starts at +0)
                float m[10];
#pragma unroll
                for (int s = 0; s < kSlabs / 4; s++) {
                    float2 *src = reinterpret_cast<float2 *>(&s_acc[w * (kSlabs / 4) + s][tid][0]);
#pragma unroll
                    for (int k = 0; k < 5; k++) {
                        const float2 b2 = src[k];
                        if (s == 0) { m[2 * k] = b2.x; m[2 * k + 1] = b2.y; }
                        else { m[2 * k] += b2.x; m[2 * k + 1] += b2.y; }
                        src[k] = make_float2(0.f, 0.f);              // leave the slab zeroed for the next batch
                    }
                }
                moments_about_centre(m, pc.x - ((float)(tx * T4D_TILE_X + ((w & 1) << 3)) + 3.5f),
                                        pc.y - ((float)(ty * T4D_TILE_Y + ((w >> 1) << 3)) + 3.5f));
#pragma unroll
                for (int k = 0; k < 10; k++) a[k] += m[k];
            }
            const uint32_t pr = s_pair[tid];
            if (pr < kp.cap) {
#pragma unroll
                for (int k = 0; k < kGP / 2; k++) grad_pair[(size_t)pr * (kGP / 2) + k] = make_float2(a[2 * k], a[2 * k + 1]);
            }
        }
        __syncthreads();
        // T4D_REGION staging
        // (behind the barrier: the write-out read the centres and pair slots of the batch these stores replace)
        if (PF && wave >= kStageWave0 && bi > 0) stage_commit(st, stage_t, cnt_n, live_n);
    }
    // T4D_REGION tile epilogue
    const kp_kernarg_p ke = kernarg_kp();
    if (ke->tile_dot && seg_j == 0) {
        // The suffix recursion has reached the eye: acc = sum_i T_i alpha_i q_i + T_final bg . dL/dC = <colour, dL/dC> (+ <depth, dL/dD> +
        // <alpha, dL/dA>), this pixel's <outputs, cotangents> - the per-view sum costs one reduction per tile.
        // One float per wave, no barrier: a workgroup's lifetime is what this launch is made of.
        const float d = wave_sum_to_lane63(acc);
        if (lane == 63) ke->tile_dot[((size_t)v * ke->T + t_) * 4 + wave] = d;
    }
    }
}

