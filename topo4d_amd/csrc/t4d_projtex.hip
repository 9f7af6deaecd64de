// t4d_projtex.hip — the capture photographs projected into a frame's UV texture on MI355X (topo4d_amd/projtex.py).
//
// Every texel of the UV image knows its point on the surface (pos) and its normal (nrm): the maps projtex.surface_maps bakes.
// k_projtex colours it from the views that see it: one thread per texel, 16x16 texel tiles (neighbouring lanes gather neighbouring
// pixels), the view loop inside; a texel outside the coverage reads its coverage byte, writes zeros and is done, so the waves of
// an empty tile retire at once (there is no separate whole-tile test: every lane of such a wave takes this exit).  No atomics, no shared memory: every texel is a pure function of its inputs.
//
// The arithmetic is float64 with FP contraction off, every product and sum rounded, in this order, so that the numpy
// restatement tests/projtex_ref.py reproduces every output bit.  With P = (X, Y, Z) = pos and n = nrm as float64, once per texel:
//   nl = sqrt((n.x n.x + n.y n.y) + n.z n.z); the texel is skipped unless nl > 0;  nh = n / nl (per component)
// and for the views v = 0, 1, ... in ascending order, with vm / pm the column-major view and projection matrices of the record:
//   1. cx = ((pm(0,0) X + pm(0,1) Y) + pm(0,2) Z) + pm(0,3), cy and cw likewise from rows 1 and 3;  px = ((cx / cw + 1) W - 1) 0.5,
//      py = ((cy / cw + 1) H - 1) 0.5;  z = ((vm(2,0) X + vm(2,1) Y) + vm(2,2) Z) + vm(2,3)   (t4d_mesh_render's projection);
//      the view is rejected unless z > 0.01
//   2. x0 = floor(px), y0 = floor(py); rejected unless 0 <= x0, x0 + 1 <= W - 1, 0 <= y0, y0 + 1 <= H - 1
//   3. every tap d of depth at (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1) must satisfy d > 0 and z <= d (1 + depth_tol)
//   4. centre c_j = -((vm(0,j) t0 + vm(1,j) t1) + vm(2,j) t2), t_i = vm(i,3) (never the record's campos);  e = c - P,
//      el = sqrt((e.x e.x + e.y e.y) + e.z e.z), eh = e / el;  cos = (nh.x eh.x + nh.y eh.y) + nh.z eh.z;  rejected unless cos >= cos_min
//   5. w = 1, then `power` times w = w cos;  with fade_px > 0: m = min(min(px, (W - 1) - px), min(py, (H - 1) - py)),
//      f = m / fade_px, and w = w f when f < 1;  a view whose w is not > 0 contributes nothing and is rejected
//   6. fx = px - x0, fy = py - y0;  per channel s = (1 - fy) ((1 - fx) t00 + fx t01) + fy ((1 - fx) t10 + fx t11)
//   7. weighted: sw = sw + w, sc = sc + w s, at the end color = float32(sc / sw), weight = float32(sw);
//      best: the view replaces the kept one when w > the kept w (ties stay with the lower view), color = float32(s), weight = float32(w)
// count is the number of views that passed 1..5.  A texel nobody sees gets color 0, weight 0, count 0.
// t4d_project_texture_gains multiplies the sample of step 6 by the view's gain, s = s gains[v][c] (one rounded product), before
// step 7; k_pair_stats (below) gathers what these gains are solved from.
//
// Two bands (t4d_projtex_low_band, t4d_project_texture_bands; the rule is restated in tests/projtex_bands_ref.py): the views never
// register to the pixel, so "weighted" smears the detail and "best" shows a step where the best view changes.  The low band of
// every photograph is blended over all views, the detail above it comes from the best view alone.
// k_low_band, per view and channel, with I the photograph, M = depth > 0 and R the radius (0..32), in float64:
//   A[r][c] = +0, then for k = -R .. R ascending A = A + I[r][c + k] where 0 <= c + k < W and M[r][c + k]; N1[r][c] counts these taps
//   (a tap outside M or outside the image is skipped, never multiplied by 0: a NaN there stays out)
//   B[r][c] = +0, then for k = -R .. R ascending B = B + A[r + k][c] where 0 <= r + k < H; N likewise from N1
//   low = N > 0 ? float32(B / N) : 0
// A box over the mesh pixels only, so the background never bleeds into the face at its silhouette; across a self-occlusion edge
// (nose over cheek) it does mix the two surfaces.  R is in pixels of the photograph.  A workgroup owns a tile of 64 x 32 pixels
// of one view and channel: it forms A and N1 of the tile's rows -R .. 32 + R in LDS (at R = 32: 96 x 64 doubles, 48 KB), four
// rows per step through a staged copy of their pixels -R .. 64 + R, then every lane sums its column of A.  The sums are formed
// tap by tap, never as a running window: that would round differently (the integer counts do slide).
// k_projtex_bands, per covered texel with a non-zero normal and the views in ascending order: steps 1..6 as above (every accepted
// view is sampled), then
//   6b. l = the bilinear mix of step 6 over the same four taps of low, times gains[v][c] when given (one rounded product)
//   7.  sw = sw + w, sl = sl + w l;  where w > bw (the kept best weight, 0 at first): bw = w, hb = s - l (one rounded subtraction;
//       ties stay with the lower view)
// and at the end low_color = float32(sl / sw), weight = float32(sw), high = float32(hb), best_weight = float32(bw), count as
// above; every other texel gets zeros.  The caller adds the bands: color = low_color + high.
//
// Registration (t4d_project_texture_flow / t4d_project_texture_bands_flow; the rule is restated in tests/projtex_flow_ref.py):
// calibration, the tracked mesh and the lens model are never exact to the pixel, so each view carries a small 2D flow against the
// consensus of all views, flows [V,H,W,2] int16 = (f_y, f_x) in 1/256 px (projtex.view_flows), and the photograph is sampled
// through it (Eisemann et al., "Floating Textures").  Geometry decides visibility and weight; the flow only moves the colour
// sample.  Per texel and view:
//   F.1. steps 1..5 and the skip bit at the unshifted pixel (px, py), exactly as they stand
//   F.2. for an accepted view: ix = (int)floor(px + 0.5), iy = (int)floor(py + 0.5), each clamped to the image; (f_y, f_x) =
//        flows[v][iy][ix], one 32-bit load
//   F.3. px' = px + f_x / 256.0, py' = py + f_y / 256.0
//   F.4. x0' = floor(px'), y0' = floor(py'); the view is rejected, as one that failed step 5, unless 0 <= x0', x0' + 1 <= W - 1,
//        0 <= y0', y0' + 1 <= H - 1: it does not count, cannot be the best view and enters no blend
//   F.5. steps 6 (and 6b) with fx = px' - x0', fy = py' - y0' over the taps at (y0', x0'); step 7 as it stands
// The flow is a template flag of the two kernels (kFlow), so that the instances without it are what they were.
//
// Photo-consistency (t4d_projtex_consistency; the rule is restated in tests/projtex_consist_ref.py): a specular highlight, a
// leak of the occlusion test (hair, lashes, a nose rim the mesh does not model) and transient content in one camera are no gain per
// camera and no registration error; what they share is that one view disagrees with a consensus of the others (Waechter et al.,
// "Let There Be Color!").  The rule is in integers, so no order of evaluation changes a bit.  Per covered texel with a non-zero
// normal, over all V <= 32 views of the call, of mixed image sizes, numbered as t4d_projtex_pair_stats numbers them:
//   A.1. each view is taken through steps 1..6 as they stand, the sample times gains[v] when given
//   A.2. for every accepted view, with s' = s >= 0 ? (s <= 4 ? s : 4) : 0 (a NaN becomes 0): q[c] = llrint(s'[c] 65536)
//   A.3. a voter is an accepted view with cos >= vote_cos_min; n = the number of voters; if n < min_votes nothing is rejected here
//   A.4. per channel m[c] = the lower median of the voters' q[c]: the value of the voter of rank (n - 1) / 2 (integer division)
//        in the order by (q[c], view index) ascending
//   A.5. an accepted view, voter or not, is an outlier when max_c |q[c] - m[c]| > qt, qt = llrint(reject_tol 65536)
//   A.6. if every accepted view is an outlier there is no consensus and nothing is rejected; otherwise bit v of the texel's skip
//        word is set for every outlier v, so at least one accepted view is always kept
// skip [h,w] uint32 is 0 for every texel that is not live; votes [h,w] uint8 holds n.  The blends take the mask (kSkip below): view
// v of a launch is left out at a texel, exactly as a view that failed step 5, when bit skip_base + v of skip[texel] is set.
// k_projtex_consist: one lane per texel, one wave per workgroup, a tile of 16 x 4 texels (a wave's four rows of the 16 x 16 tile
// of the other texel kernels, so neighbouring lanes still gather neighbouring pixels).  The view loop runs once; the accepted and
// the voter mask stay in registers, and the packed q of every accepted view (three fields of 21 bits: q <= 2^18) goes to LDS as
// one 64-bit word at [v][lane], V x 512 bytes per wave, sized by the call's V: 16 KiB at V = 32, so 10 waves per CU of the 160
// KiB, 13 at the 24 views of a capture rig.  A 256-lane workgroup would take 64 KiB at V = 32 and leave 2 workgroups = 8 waves per
// CU, with 32 KiB idle; the single wave keeps every 16 KiB in use, needs no barrier (a lane reads only its own column) and lets the
// waves of an empty tile retire at once.  The median is found by rank counting over the voters, O(n^2) compares of words the lane
// reads back from its column (consecutive lanes, consecutive 64-bit words: no bank conflict), all three channels per pair.  No
// global scratch, no atomics: every texel is a pure function of its inputs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_block.h"
#include "t4d_host.h"

namespace {

constexpr int kTile = 16;                    // 16x16 texels per workgroup: a wave holds 4 rows of 16 neighbouring texels
constexpr int kMaxDim = 65536;               // texture and image sides: every grid stays below 2^31 workgroups
constexpr int kMaxViews = 255;               // count is a uint8
constexpr int kMaxPower = 8;
constexpr double kNear = 0.01;               // the mesh renderer's near plane

struct Rule {                                 // what accepts and weighs a view, the same in every kernel
    int power;
    double cos_min, fade_px, depth_lim;      // depth_lim = 1 + depth_tol
};

struct Tex {                                  // what every texel kernel takes: the texel maps, the views' records, the rule
    const float *pos, *nrm, *views;
    const uint8_t *coverage;
    const double *gains;                     // [V,3] or NULL
    int th, tw, V;
    Rule rule;
};

struct PTP {
    Tex T;
    const float *photos, *depth;
    int H, W, mode;
    float *color, *weight;
    uint8_t *count;
    const uint32_t *skip;                    // [th,tw] the consistency mask or NULL; view v is bit skip_base + v
    int skip_base;
    const int16_t *flows;                    // [V,H,W,2] (f_y, f_x) in 1/256 px, or NULL
};

// The texel (tx, ty), and through texel_load the lane's texel of the 16x16 tile (tile_x, tile_y): whether it lies inside the texture, and there `at`; whether it is live (inside,
// covered, with a non-zero normal), and then its point and its normalised normal.  A texel outside the coverage costs one byte read.
struct Texel {
    bool inside, live;
    size_t at;
    double X, Y, Z, nhx, nhy, nhz;
};

__device__ __forceinline__ Texel texel_at(const Tex &T, int tx, int ty)
{
#pragma clang fp contract(off)
    Texel t = {};
    t.inside = tx < T.tw && ty < T.th;
    t.at = (size_t)ty * (size_t)T.tw + (size_t)tx;
    if (!t.inside || T.coverage[t.at] == 0) return t;
    const double nx = (double)T.nrm[3 * t.at], ny = (double)T.nrm[3 * t.at + 1], nz = (double)T.nrm[3 * t.at + 2];
    const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
    t.live = nl > 0.0;
    t.X = (double)T.pos[3 * t.at]; t.Y = (double)T.pos[3 * t.at + 1]; t.Z = (double)T.pos[3 * t.at + 2];
    t.nhx = nx / nl; t.nhy = ny / nl; t.nhz = nz / nl;
    return t;
}

__device__ __forceinline__ Texel texel_load(const Tex &T, int tile_x, int tile_y)
{
    return texel_at(T, tile_x * kTile + (int)(threadIdx.x % kTile), tile_y * kTile + (int)(threadIdx.x / kTile));
}

struct View {                                 // one view of size H x W: its record (vm, then pm) and its depth [H,W]
    const float *vm, *depth;
    int H, W;
};

struct Hit {                                  // an accepted view at a texel: weight, cosine, the first of its four taps and the bilinear fractions
    double w, cs, fx, fy;
    double px, py;                           // the pixel of step 1, for view_flow
    size_t tap;
};

// Steps 1..5 of the rule above for one view at a live texel: whether the view is accepted, and then `h`.
__device__ __forceinline__ bool view_accept(const View &v, const Rule &r, const Texel &t, Hit &h)
{
#pragma clang fp contract(off)
    const float *vm = v.vm, *pm = vm + 16;
    const int W = v.W;
    const double X = t.X, Y = t.Y, Z = t.Z;
    const double Wd = (double)W, Hd = (double)v.H, xmax = (double)(W - 1), ymax = (double)(v.H - 1);
    // 1. projection
    const double cx = (((double)pm[0] * X + (double)pm[4] * Y) + (double)pm[8] * Z) + (double)pm[12];
    const double cy = (((double)pm[1] * X + (double)pm[5] * Y) + (double)pm[9] * Z) + (double)pm[13];
    const double cw = (((double)pm[3] * X + (double)pm[7] * Y) + (double)pm[11] * Z) + (double)pm[15];
    const double px = ((cx / cw + 1.0) * Wd - 1.0) * 0.5;
    const double py = ((cy / cw + 1.0) * Hd - 1.0) * 0.5;
    const double z = (((double)vm[2] * X + (double)vm[6] * Y) + (double)vm[10] * Z) + (double)vm[14];
    if (!(z > kNear)) return false;
    // 2. the four taps inside the image (a NaN fails the comparisons)
    const double fx0 = floor(px), fy0 = floor(py);
    if (!(fx0 >= 0.0 && fx0 + 1.0 <= xmax && fy0 >= 0.0 && fy0 + 1.0 <= ymax)) return false;
    // 4. facing (before the gathers: it needs no memory)
    const double t0 = (double)vm[12], t1 = (double)vm[13], t2 = (double)vm[14];
    const double ex = -(((double)vm[0] * t0 + (double)vm[1] * t1) + (double)vm[2] * t2) - X;
    const double ey = -(((double)vm[4] * t0 + (double)vm[5] * t1) + (double)vm[6] * t2) - Y;
    const double ez = -(((double)vm[8] * t0 + (double)vm[9] * t1) + (double)vm[10] * t2) - Z;
    const double el = sqrt((ex * ex + ey * ey) + ez * ez);
    const double cs = (t.nhx * (ex / el) + t.nhy * (ey / el)) + t.nhz * (ez / el);
    if (!(cs >= r.cos_min)) return false;
    // 3. visibility
    h.tap = (size_t)(int)fy0 * (size_t)W + (size_t)(int)fx0;
    const float *dp = v.depth + h.tap;
    const double d00 = (double)dp[0], d01 = (double)dp[1], d10 = (double)dp[W], d11 = (double)dp[W + 1];
    if (!(d00 > 0.0 && d01 > 0.0 && d10 > 0.0 && d11 > 0.0)) return false;
    if (!(z <= d00 * r.depth_lim && z <= d01 * r.depth_lim && z <= d10 * r.depth_lim && z <= d11 * r.depth_lim)) return false;
    // 5. weight
    double w = 1.0;
    for (int k = 0; k < r.power; ++k) w = w * cs;
    if (r.fade_px > 0.0) {
        const double m = fmin(fmin(px, xmax - px), fmin(py, ymax - py));
        const double f = m / r.fade_px;
        if (f < 1.0) w = w * f;
    }
    if (!(w > 0.0)) return false;
    h.w = w;
    h.cs = cs;
    h.fx = px - fx0;
    h.fy = py - fy0;
    h.px = px;
    h.py = py;
    return true;
}

// Steps F.2..F.4 of the registration rule for an accepted view: the flow ([H,W,2] int16: (f_y, f_x) in 1/256 px) read at the
// pixel nearest to (px, py) moves the taps and the fractions of `h`; false when a moved tap leaves the image.
__device__ __forceinline__ bool view_flow(const int16_t *flow, const View &v, Hit &h)
{
#pragma clang fp contract(off)
    const int W = v.W, H = v.H;
    int ix = (int)floor(h.px + 0.5), iy = (int)floor(h.py + 0.5);
    ix = ix < 0 ? 0 : (ix > W - 1 ? W - 1 : ix);
    iy = iy < 0 ? 0 : (iy > H - 1 ? H - 1 : iy);
    const uint32_t f = reinterpret_cast<const uint32_t *>(flow)[(size_t)iy * (size_t)W + (size_t)ix];     // f_y low, f_x high
    const double px = h.px + (double)(int16_t)(f >> 16) / 256.0, py = h.py + (double)(int16_t)(f & 0xffffu) / 256.0;
    const double fx0 = floor(px), fy0 = floor(py);
    if (!(fx0 >= 0.0 && fx0 + 1.0 <= (double)(W - 1) && fy0 >= 0.0 && fy0 + 1.0 <= (double)(H - 1))) return false;
    h.tap = (size_t)(int)fy0 * (size_t)W + (size_t)(int)fx0;
    h.fx = px - fx0;
    h.fy = py - fy0;
    return true;
}

// Step 6 under an accepted view's taps: s = the bilinear mix of img ([3,H,W]: the photograph, or its low band), times gain[c] when
// gain is given (one rounded product).
__device__ __forceinline__ void view_sample(const float *img, const View &v, const Hit &h, const double *gain, double s[3])
{
#pragma clang fp contract(off)
    const int W = v.W;
    const size_t plane = (size_t)v.H * (size_t)W;
    const double fx = h.fx, fy = h.fy, gx = 1.0 - fx, gy = 1.0 - fy;
    for (int c = 0; c < 3; ++c) {
        const float *q = img + h.tap + (size_t)c * plane;
        const double a = gx * (double)q[0] + fx * (double)q[1], b = gx * (double)q[W] + fx * (double)q[W + 1];
        s[c] = gy * a + fy * b;
        if (gain) s[c] = s[c] * gain[c];
    }
}

// (an instance per flag, so that the kernel without gains, without a mask and without flows is the one it was before they existed)
template <bool kGains, bool kSkip, bool kFlow>
__global__ __launch_bounds__(kTile * kTile) void k_projtex(const PTP P)
{
#pragma clang fp contract(off)
    const Texel t = texel_load(P.T, (int)blockIdx.x, (int)blockIdx.y);
    if (!t.inside) return;
    const size_t at = t.at;
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int cnt = 0;
    if (t.live) {                                                           // (else, most of a face's UV layout: one byte read, zeros out)
        const size_t plane = (size_t)P.H * (size_t)P.W;
        const bool best = P.mode == T4D_PROJTEX_BEST;
        const uint32_t skip = kSkip ? P.skip[at] >> P.skip_base : 0u;       // (skip_base + V <= 32: the entry point checks)
        for (int v = 0; v < P.T.V; ++v) {
            if (kSkip && ((skip >> v) & 1u)) continue;                      // a rejected view: as one that failed step 5
            const View view = {P.T.views + (size_t)v * T4D_VIEW_FLOATS, P.depth + (size_t)v * plane, P.H, P.W};
            Hit h;
            if (!view_accept(view, P.T.rule, t, h)) continue;
            if (kFlow && !view_flow(P.flows + (size_t)v * 2 * plane, view, h)) continue;         // F.4: as one that failed step 5
            ++cnt;
            if (best && !(h.w > sw)) continue;                              // a view that cannot win is counted but not gathered (ties stay with the lower view)
            double s[3];
            view_sample(P.photos + (size_t)v * 3 * plane, view, h, kGains ? P.T.gains + 3 * v : nullptr, s);
            // 7. accumulate
            if (best) {
                sw = h.w; s0 = s[0]; s1 = s[1]; s2 = s[2];
            } else {
                sw = sw + h.w;
                s0 = s0 + h.w * s[0]; s1 = s1 + h.w * s[1]; s2 = s2 + h.w * s[2];
            }
        }
        if (cnt && !best) { s0 = s0 / sw; s1 = s1 / sw; s2 = s2 / sw; }
    }
    P.color[3 * at] = (float)s0;
    P.color[3 * at + 1] = (float)s1;
    P.color[3 * at + 2] = (float)s2;
    P.weight[at] = (float)sw;
    P.count[at] = (uint8_t)cnt;
}

// ---- pair statistics: what projtex.solve_gains equalises the cameras from ----------------------------------------------------
// A view takes part at a texel when it is accepted (steps 1..5), cos >= stat_cos_min and every channel of its sample s (step 6,
// times its gain) lies in [stat_lo, stat_hi]; q[c] = llrint(s[c] 65536).  For every ordered pair (i, j) of views that both take part
// at a texel, pair_count[i][j] += 1 and pair_sum[i][j][c] += q_i[c].  Everything summed is an integer, so no order of accumulation
// changes a bit.
//
// One lane per texel, 16x16 tiles as k_projtex, so a wave holds 4 rows of 16 neighbouring texels; a workgroup walks the tiles
// blockIdx.x, blockIdx.x + gridDim.x, ... and keeps a [V,V,4] int64 table (count, three sums) in LDS that it adds to global memory
// once at its end, entry by entry with 64-bit vector atomics, the zero entries left out.
// Per wave and tile, first the view loop: each lane keeps a 32-bit mask of its taking-part views; a ballot gives the view's lane set
// and a butterfly the sum of its q over that set; lane v of the wave keeps both for view v (V <= 32 < 64).  Then the pairs: for view
// i lane j sees set_i & set_j; where that equals set_i (neighbouring texels mostly share their view sets) the sum over the pair is
// the sum over set_i, so lanes j = 0..V-1 add their entries (i, j) in one step with no further cross-lane work.  Only for a view i
// that has a partner covering part of its set is q_i evaluated again (nothing per lane and view is stored: at 12 bytes per view
// and lane that would take the LDS the occupancy needs for the gathers), followed by a masked butterfly per such partner.
constexpr int kStatViews = 32;               // the lane's mask has 32 bits
constexpr int kStatGrid = 4096;              // workgroups at most: 16 per CU, each flushing its table once
constexpr double kStatRange = 1024.0;        // |stat_lo|, |stat_hi| at most: q < 2^26, so an int64 holds the sum over 2^37 texels
constexpr double kStatScale = 65536.0;

struct PSP {
    Tex T;
    const int32_t *sizes;                    // [V,2] (h, w)
    const float *const *photos, *const *depth;
    int tiles_x, tiles;
    double stat_cos_min, stat_lo, stat_hi;
    unsigned long long *pair_count, *pair_sum;
};

// whether view v takes part at the lane's texel, and its q
__device__ __forceinline__ bool stat_eval(const PSP &P, int v, const Texel &t, long long q[3])
{
#pragma clang fp contract(off)
    const View view = {P.T.views + (size_t)v * T4D_VIEW_FLOATS, P.depth[v], P.sizes[2 * v], P.sizes[2 * v + 1]};
    if (view.H < 1 || view.W < 1 || view.H > kMaxDim || view.W > kMaxDim) return false;
    Hit h;
    double s[3];
    if (!view_accept(view, P.T.rule, t, h) || !(h.cs >= P.stat_cos_min)) return false;
    view_sample(P.photos[v], view, h, P.T.gains ? P.T.gains + 3 * v : nullptr, s);
    for (int c = 0; c < 3; ++c)
        if (!(s[c] >= P.stat_lo && s[c] <= P.stat_hi)) return false;
    for (int c = 0; c < 3; ++c) q[c] = llrint(s[c] * kStatScale);
    return true;
}

__global__ __launch_bounds__(kTile * kTile) void k_pair_stats(const PSP P)
{
    __shared__ unsigned long long tab[kStatViews * kStatViews * 4];
    const int V = P.T.V, lane = (int)(threadIdx.x & 63);
    for (int e = (int)threadIdx.x; e < V * V * 4; e += kTile * kTile) tab[e] = 0;
    __syncthreads();
    for (int t = (int)blockIdx.x; t < P.tiles; t += (int)gridDim.x) {
        const Texel tex = texel_load(P.T, t % P.tiles_x, t / P.tiles_x);
        const bool live = tex.live;
        if (__ballot(live) == 0) continue;                                  // the whole wave, so every lane reaches the shuffles below
        // the views: the lane's mask; lane v keeps the lane set of view v and the sums of q over it
        uint32_t mask = 0;
        unsigned long long set = 0;
        long long tot0 = 0, tot1 = 0, tot2 = 0;
        for (int v = 0; v < V; ++v) {
            long long q[3] = {0, 0, 0};
            const bool part = live && stat_eval(P, v, tex, q);
            const unsigned long long b = __ballot(part);
            if (b == 0) continue;
            if (part) mask |= 1u << v;
            const long long a0 = wave_sum(part ? q[0] : 0), a1 = wave_sum(part ? q[1] : 0), a2 = wave_sum(part ? q[2] : 0);
            if (lane == v) { set = b; tot0 = a0; tot1 = a1; tot2 = a2; }
        }
        // the pairs
        for (int i = 0; i < V; ++i) {
            const unsigned long long si = __shfl(set, i, 64);
            if (si == 0) continue;
            const long long t0 = __shfl(tot0, i, 64), t1 = __shfl(tot1, i, 64), t2 = __shfl(tot2, i, 64);
            const unsigned long long both = si & set;                       // lane j: texels of the wave where i and j take part
            const bool whole = both == si;
            if (both != 0 && whole) {                                       // (only lanes j < V hold a set)
                unsigned long long *e = tab + (size_t)(i * V + lane) * 4;
                atomicAdd(e, (unsigned long long)__popcll(both));
                atomicAdd(e + 1, (unsigned long long)t0); atomicAdd(e + 2, (unsigned long long)t1); atomicAdd(e + 3, (unsigned long long)t2);
            }
            unsigned long long partial = __ballot(both != 0 && !whole);     // partners j that share only a part of set_i
            if (partial == 0) continue;
            long long q[3] = {0, 0, 0};
            const bool has_i = (mask >> i) & 1u;
            if (has_i) stat_eval(P, i, tex, q);         // the same operations again: the same q
            while (partial) {
                const int j = __builtin_ctzll(partial);
                partial &= partial - 1;
                const bool in = has_i && ((mask >> j) & 1u);
                const unsigned long long n = (unsigned long long)__popcll(__ballot(in));
                const long long a0 = wave_sum(in ? q[0] : 0), a1 = wave_sum(in ? q[1] : 0), a2 = wave_sum(in ? q[2] : 0);
                if (lane == 0) {
                    unsigned long long *e = tab + (size_t)(i * V + j) * 4;
                    atomicAdd(e, n);
                    atomicAdd(e + 1, (unsigned long long)a0); atomicAdd(e + 2, (unsigned long long)a1); atomicAdd(e + 3, (unsigned long long)a2);
                }
            }
        }
    }
    __syncthreads();
    for (int e = (int)threadIdx.x; e < V * V; e += kTile * kTile) {
        if (tab[4 * e] == 0) continue;
        atomicAdd(P.pair_count + e, tab[4 * e]);
        for (int c = 0; c < 3; ++c)
            if (tab[4 * e + 1 + c] != 0) atomicAdd(P.pair_sum + 3 * (size_t)e + c, tab[4 * e + 1 + c]);
    }
}

// ---- photo-consistency: the views that disagree with the median of the facing ones (rule A.1..A.6 at the top) -------------------
constexpr int kConsW = kTile, kConsH = 4;    // texels per workgroup of k_projtex_consist: one wave
constexpr int kConsLanes = kConsW * kConsH;
constexpr int kConsBits = 21;                // a field of the packed q: q <= 4 * 65536 = 2^18
constexpr double kConsMax = 4.0;             // samples are clamped to [0, kConsMax] before they are rounded; reject_tol at most this

struct PCP {
    Tex T;
    const int32_t *sizes;                    // [V,2] (h, w)
    const float *const *photos, *const *depth;
    double vote_cos_min;
    int qt, min_votes;
    uint32_t *skip;
    uint8_t *votes;
};

__device__ __forceinline__ int cons_field(unsigned long long word, int c)
{
    return (int)((word >> (c * kConsBits)) & ((1ull << kConsBits) - 1));
}

__global__ __launch_bounds__(kConsLanes) void k_projtex_consist(const PCP P)
{
#pragma clang fp contract(off)
    extern __shared__ unsigned long long cons_q[];                          // [V][64]: the packed q of the lane's accepted views
    const int lane = (int)threadIdx.x, V = P.T.V;
    const Texel t = texel_at(P.T, (int)blockIdx.x * kConsW + lane % kConsW, (int)blockIdx.y * kConsH + lane / kConsW);
    if (!t.inside) return;
    uint32_t accepted = 0, voters = 0, out = 0;
    if (t.live) {
        for (int v = 0; v < V; ++v) {
            const View view = {P.T.views + (size_t)v * T4D_VIEW_FLOATS, P.depth[v], P.sizes[2 * v], P.sizes[2 * v + 1]};
            if (view.H < 1 || view.W < 1 || view.H > kMaxDim || view.W > kMaxDim) continue;
            Hit h;
            if (!view_accept(view, P.T.rule, t, h)) continue;
            double s[3];
            view_sample(P.photos[v], view, h, P.T.gains ? P.T.gains + 3 * v : nullptr, s);
            unsigned long long word = 0;
            for (int c = 0; c < 3; ++c) {
                const double sc = s[c] >= 0.0 ? (s[c] <= kConsMax ? s[c] : kConsMax) : 0.0;         // (a NaN fails the first comparison)
                word |= (unsigned long long)llrint(sc * kStatScale) << (c * kConsBits);
            }
            cons_q[v * kConsLanes + lane] = word;
            accepted |= 1u << v;
            if (h.cs >= P.vote_cos_min) voters |= 1u << v;
        }
    }
    const int n = __popc(voters);
    if (n >= P.min_votes) {                                                 // (min_votes >= 2: never with n = 0)
        // A.4: the voter that exactly (n - 1) / 2 voters precede in the order by (q[c], view index) holds the median of channel c
        const int want = (n - 1) / 2;
        int m[3] = {0, 0, 0};
        int found = 0;
        for (uint32_t bi = voters; bi && found < 3; bi &= bi - 1) {
            const int i = __builtin_ctz(bi);
            const unsigned long long wi = cons_q[i * kConsLanes + lane];
            int rank[3] = {0, 0, 0};
            for (uint32_t bj = voters; bj; bj &= bj - 1) {
                const int j = __builtin_ctz(bj);
                const unsigned long long wj = cons_q[j * kConsLanes + lane];
                for (int c = 0; c < 3; ++c) {
                    const int qi = cons_field(wi, c), qj = cons_field(wj, c);
                    rank[c] += (qj < qi || (qj == qi && j < i)) ? 1 : 0;
                }
            }
            for (int c = 0; c < 3; ++c)
                if (rank[c] == want) { m[c] = cons_field(wi, c); ++found; }
        }
        // A.5, A.6
        for (uint32_t b = accepted; b; b &= b - 1) {
            const int v = __builtin_ctz(b);
            const unsigned long long w = cons_q[v * kConsLanes + lane];
            int worst = 0;
            for (int c = 0; c < 3; ++c) {
                const int d = cons_field(w, c) - m[c];
                const int ad = d < 0 ? -d : d;
                if (ad > worst) worst = ad;
            }
            if (worst > P.qt) out |= 1u << v;
        }
        if (out == accepted) out = 0;                                       // no consensus: every accepted view is kept
    }
    P.skip[t.at] = out;
    P.votes[t.at] = (uint8_t)n;
}

// ---- two bands: the low band of the photographs, and the projection that blends it and keeps the best view's detail -----------
constexpr int kLowW = 64, kLowH = 32;        // pixels per workgroup of k_low_band: a wave per row, 256 lanes
constexpr int kLowStep = 4;                  // rows of A formed per step, one per wave
constexpr int kMaxRadius = 32;
constexpr int kLowSeg = kLowW + 2 * kMaxRadius;

struct LBP {
    const float *photos, *depth;
    float *low;
    int H, W, R;
};

static size_t low_band_lds(int R)
{
    const size_t rows = (size_t)(kLowH + 2 * R);
    return rows * kLowW * (sizeof(double) + 1) + (size_t)kLowStep * kLowSeg * sizeof(float);
}

__global__ __launch_bounds__(kLowW * kLowStep) void k_low_band(const LBP P)
{
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    const int R = P.R, H = P.H, W = P.W, rows = kLowH + 2 * R, seg = kLowW + 2 * R;
    double *A = lds;                                                        // [rows][64]: the horizontal sums
    float *sv = (float *)(A + (size_t)rows * kLowW);                        // [4][128]: the staged pixels of four rows, 0 off the mesh
    uint8_t *N1 = (uint8_t *)(sv + kLowStep * kLowSeg);                     // [rows][64]: the taps in A (at most 65)
    const int tid = (int)threadIdx.x, lane = tid % kLowW, wv = tid / kLowW;
    const int x0 = (int)blockIdx.x * kLowW, y0 = (int)blockIdx.y * kLowH;
    const size_t plane = (size_t)H * (size_t)W;
    const float *photo = P.photos + (size_t)blockIdx.z * plane;             // blockIdx.z = 3 view + channel
    const float *depth = P.depth + (size_t)(blockIdx.z / 3) * plane;
    const unsigned long long window = 2 * R + 1 >= 64 ? ~0ull : (1ull << (2 * R + 1)) - 1;
    // A wave forms its row of A from the row's pixels -R .. 64 + R, which it stages itself.  A pixel off the mesh or outside the
    // image is staged as +0: A starts at +0 and is never -0, so adding +0 leaves every bit as skipping the tap does, and the
    // pixel itself is not read.  The number of taps is the population of the mask's bits lane .. lane + 2 R.
    for (int r0 = 0; r0 < rows; r0 += kLowStep) {
        const int y = y0 - R + r0 + wv;
        unsigned long long mask[2] = {0ull, 0ull};
        for (int half = 0; half < 2; ++half) {
            const int j = lane + half * kLowW, x = x0 - R + j;
            bool m = false;
            float val = 0.0f;
            if (j < seg && y >= 0 && y < H && x >= 0 && x < W) {
                const size_t at = (size_t)y * (size_t)W + (size_t)x;
                m = depth[at] > 0.0f;
                if (m) val = photo[at];
            }
            sv[wv * kLowSeg + j] = val;
            mask[half] = __ballot(m);
        }
        const unsigned long long mlo = mask[0], mhi = mask[1];
        __syncthreads();
        if (r0 + wv < rows) {
            const float *pv = sv + wv * kLowSeg + lane;
            double a = 0.0;
            for (int k = 0; k <= 2 * R; ++k) a = a + (double)pv[k];
            const unsigned long long bits = (mlo >> lane) | (lane ? mhi << (64 - lane) : 0ull);      // the mask from pixel `lane` on
            const int n = __popcll(bits & window) + (R == kMaxRadius ? (int)((mhi >> lane) & 1ull) : 0);
            A[(size_t)(r0 + wv) * kLowW + lane] = a;
            N1[(size_t)(r0 + wv) * kLowW + lane] = (uint8_t)n;
        }
        __syncthreads();
    }
    const int x = x0 + lane;
    if (x >= W) return;
    // the vertical pass: a lane sums its column over eight consecutive rows; rows outside the image hold A = +0 and N1 = 0, and
    // the count, an integer, slides from row to row
    float *out = P.low + (size_t)blockIdx.z * plane;
    const int i0 = wv * (kLowH / kLowStep);
    int n = 0;
    for (int k = 0; k <= 2 * R; ++k) n += N1[(size_t)(i0 + k) * kLowW + lane];
    for (int i = i0; i < i0 + kLowH / kLowStep && y0 + i < H; ++i) {
        const int y = y0 + i;
        const int klo = R < y ? -R : -y, khi = R < H - 1 - y ? R : H - 1 - y;   // the rows inside the image
        double b = 0.0;
        for (int k = klo; k <= khi; ++k) b = b + A[(size_t)(i + k + R) * kLowW + lane];
        out[(size_t)y * (size_t)W + (size_t)x] = n > 0 ? (float)(b / (double)n) : 0.0f;
        if (i + 1 < kLowH) n += (int)N1[(size_t)(i + 1 + 2 * R) * kLowW + lane] - (int)N1[(size_t)i * kLowW + lane];
    }
}

struct PBP {
    Tex T;
    const float *photos, *low, *depth;
    int H, W;
    float *low_color, *weight, *high, *best_weight;
    uint8_t *count;
    const uint32_t *skip;                    // as PTP's
    int skip_base;
    const int16_t *flows;                    // as PTP's
};

template <bool kGains, bool kSkip, bool kFlow>
__global__ __launch_bounds__(kTile * kTile) void k_projtex_bands(const PBP P)
{
#pragma clang fp contract(off)
    const Texel t = texel_load(P.T, (int)blockIdx.x, (int)blockIdx.y);
    if (!t.inside) return;
    const size_t at = t.at;
    double sw = 0.0, bw = 0.0, sl[3] = {0.0, 0.0, 0.0}, hb[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    if (t.live) {
        const size_t plane = (size_t)P.H * (size_t)P.W;
        const uint32_t skip = kSkip ? P.skip[at] >> P.skip_base : 0u;
        for (int v = 0; v < P.T.V; ++v) {
            if (kSkip && ((skip >> v) & 1u)) continue;
            const View view = {P.T.views + (size_t)v * T4D_VIEW_FLOATS, P.depth + (size_t)v * plane, P.H, P.W};
            const double *gain = kGains ? P.T.gains + 3 * v : nullptr;
            Hit h;
            if (!view_accept(view, P.T.rule, t, h)) continue;
            if (kFlow && !view_flow(P.flows + (size_t)v * 2 * plane, view, h)) continue;
            ++cnt;
            double s[3], l[3];
            view_sample(P.photos + (size_t)v * 3 * plane, view, h, gain, s);
            view_sample(P.low + (size_t)v * 3 * plane, view, h, gain, l);    // 6b. the low band under the same taps
            // 7. the low band of every view, the detail of the best one
            sw = sw + h.w;
            for (int c = 0; c < 3; ++c) sl[c] = sl[c] + h.w * l[c];
            if (h.w > bw) {
                bw = h.w;
                for (int c = 0; c < 3; ++c) hb[c] = s[c] - l[c];
            }
        }
        if (cnt)
            for (int c = 0; c < 3; ++c) sl[c] = sl[c] / sw;
    }
    for (int c = 0; c < 3; ++c) {
        P.low_color[3 * at + c] = (float)sl[c];
        P.high[3 * at + c] = (float)hb[c];
    }
    P.weight[at] = (float)sw;
    P.best_weight[at] = (float)bw;
    P.count[at] = (uint8_t)cnt;
}

}  // namespace

// What the entry points check alike: the buffers (`buffers`: none of them NULL), the image sides and the number of views.
static int views_check(const char *name, bool buffers, int32_t n_views, int max_views, int32_t h, int32_t w)
{
    if (!buffers) return t4d_fail(T4D_ERR_ARG, "%s: NULL buffer", name);
    if (h < 1 || w < 1 || h > kMaxDim || w > kMaxDim)
        return t4d_fail(T4D_ERR_ARG, "%s: need 1 <= sides <= %d, got %d x %d images", name, kMaxDim, h, w);
    if (n_views < 1 || n_views > max_views) return t4d_fail(T4D_ERR_ARG, "%s: n_views must be in [1, %d], got %d", name, max_views, n_views);
    return T4D_OK;
}

static int projtex_check(const char *name, int32_t tex_h, int32_t tex_w, int32_t power, double cos_min, double fade_px, double depth_tol)
{
    if (tex_h < 1 || tex_w < 1 || tex_h > kMaxDim || tex_w > kMaxDim)
        return t4d_fail(T4D_ERR_ARG, "%s: need 1 <= sides <= %d, got a %d x %d texture", name, kMaxDim, tex_h, tex_w);
    if (power < 0 || power > kMaxPower) return t4d_fail(T4D_ERR_ARG, "%s: power must be in [0, %d], got %d", name, kMaxPower, power);
    if (!(cos_min >= -1.0 && cos_min <= 1.0) || !(fade_px >= 0.0 && fade_px <= (double)kMaxDim) || !(depth_tol >= 0.0 && depth_tol <= 1.0))
        return t4d_fail(T4D_ERR_ARG, "%s: need cos_min in [-1, 1], fade_px in [0, %d] and depth_tol in [0, 1]", name, kMaxDim);
    return T4D_OK;
}

static Tex tex_block(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w, const float *views,
                     int32_t n_views, const double *gains, int32_t power, double cos_min, double fade_px, double depth_tol)
{
    return Tex{pos, nrm, views, coverage, gains, tex_h, tex_w, n_views, Rule{power, cos_min, fade_px, 1.0 + depth_tol}};
}

static dim3 tile_grid(int32_t tex_h, int32_t tex_w)
{
    return dim3((unsigned)((tex_w + kTile - 1) / kTile), (unsigned)((tex_h + kTile - 1) / kTile));
}

// the mask of a blend: with skip given, its bits skip_base .. skip_base + n_views - 1 are the launch's views
static int skip_check(const char *name, const uint32_t *skip, int32_t skip_base, int32_t n_views)
{
    if (skip && (skip_base < 0 || skip_base > kStatViews || skip_base + n_views > kStatViews))
        return t4d_fail(T4D_ERR_ARG, "%s: with skip, need skip_base >= 0 and skip_base + n_views <= %d, got %d + %d", name, kStatViews,
                        skip_base, n_views);
    return T4D_OK;
}

// the flows of a blend: int16 pairs read as one 32-bit word
static int flows_check(const char *name, const int16_t *flows)
{
    if (flows && (uintptr_t)flows % sizeof(uint32_t) != 0) return t4d_fail(T4D_ERR_ARG, "%s: flows must be aligned to 4 bytes", name);
    return T4D_OK;
}

// the instance of a texel kernel for what a launch is given: K<gains, skip, flows>
#define T4D_PROJTEX_INSTANCE(K, gains, skip, flows)                                                                              \
    ((flows) ? ((skip) ? ((gains) ? K<true, true, true> : K<false, true, true>) : ((gains) ? K<true, false, true> : K<false, false, true>))   \
             : ((skip) ? ((gains) ? K<true, true, false> : K<false, true, false>) : ((gains) ? K<true, false, false> : K<false, false, false>)))

T4D_EXPORT int t4d_project_texture_flow(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                        const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos,
                                        const float *depth, const double *gains, int32_t power, double cos_min, double fade_px,
                                        double depth_tol, int32_t mode, float *color, float *weight, uint8_t *count,
                                        const uint32_t *skip, int32_t skip_base, void *hip_stream, const int16_t *flows)
{
    const char *name = "t4d_project_texture";
    if (const int rc = views_check(name, pos && nrm && coverage && views && photos && depth && color && weight && count, n_views, kMaxViews, h, w))
        return rc;
    if (mode != T4D_PROJTEX_WEIGHTED && mode != T4D_PROJTEX_BEST)
        return t4d_fail(T4D_ERR_ARG, "%s: mode must be T4D_PROJTEX_WEIGHTED or T4D_PROJTEX_BEST, got %d", name, mode);
    if (const int rc = projtex_check(name, tex_h, tex_w, power, cos_min, fade_px, depth_tol)) return rc;
    if (const int rc = skip_check(name, skip, skip_base, n_views)) return rc;
    if (const int rc = flows_check(name, flows)) return rc;
    const PTP P = {tex_block(pos, nrm, coverage, tex_h, tex_w, views, n_views, gains, power, cos_min, fade_px, depth_tol),
                   photos, depth, h, w, mode, color, weight, count, skip, skip_base, flows};
    const auto kernel = T4D_PROJTEX_INSTANCE(k_projtex, gains, skip, flows);
    hipLaunchKernelGGL(kernel, tile_grid(tex_h, tex_w), dim3(kTile * kTile), 0, (hipStream_t)hip_stream, P);
    return t4d_launch_status(name);
}

T4D_EXPORT int t4d_project_texture_skip(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                        const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos,
                                        const float *depth, const double *gains, int32_t power, double cos_min, double fade_px,
                                        double depth_tol, int32_t mode, float *color, float *weight, uint8_t *count,
                                        const uint32_t *skip, int32_t skip_base, void *hip_stream)
{
    return t4d_project_texture_flow(pos, nrm, coverage, tex_h, tex_w, views, n_views, h, w, photos, depth, gains, power, cos_min,
                                    fade_px, depth_tol, mode, color, weight, count, skip, skip_base, hip_stream, nullptr);
}

T4D_EXPORT int t4d_project_texture_gains(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                         const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos,
                                         const float *depth, const double *gains, int32_t power, double cos_min, double fade_px,
                                         double depth_tol, int32_t mode, float *color, float *weight, uint8_t *count, void *hip_stream)
{
    return t4d_project_texture_skip(pos, nrm, coverage, tex_h, tex_w, views, n_views, h, w, photos, depth, gains, power, cos_min,
                                    fade_px, depth_tol, mode, color, weight, count, nullptr, 0, hip_stream);
}

T4D_EXPORT int t4d_project_texture(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                   const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos, const float *depth,
                                   int32_t power, double cos_min, double fade_px, double depth_tol, int32_t mode, float *color,
                                   float *weight, uint8_t *count, void *hip_stream)
{
    return t4d_project_texture_gains(pos, nrm, coverage, tex_h, tex_w, views, n_views, h, w, photos, depth, nullptr, power, cos_min,
                                     fade_px, depth_tol, mode, color, weight, count, hip_stream);
}

T4D_EXPORT int t4d_projtex_pair_stats(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                      const float *views, int32_t n_views, const int32_t *sizes, const float *const *photos,
                                      const float *const *depth, int32_t power, double cos_min, double fade_px, double depth_tol,
                                      double stat_cos_min, double stat_lo, double stat_hi, const double *gains, int64_t *pair_count,
                                      int64_t *pair_sum, void *hip_stream)
{
    const char *name = "t4d_projtex_pair_stats";             // (the image sides are per view, in `sizes` on the device: the kernel looks at them)
    if (const int rc = views_check(name, pos && nrm && coverage && views && sizes && photos && depth && pair_count && pair_sum, n_views, kStatViews, 1, 1))
        return rc;
    if (const int rc = projtex_check(name, tex_h, tex_w, power, cos_min, fade_px, depth_tol)) return rc;
    if (!(stat_cos_min >= -1.0 && stat_cos_min <= 1.0) || !(stat_lo >= -kStatRange && stat_lo <= stat_hi && stat_hi <= kStatRange))
        return t4d_fail(T4D_ERR_ARG, "%s: need stat_cos_min in [-1, 1] and -%g <= stat_lo <= stat_hi <= %g", name, kStatRange, kStatRange);
    const int tiles_x = (tex_w + kTile - 1) / kTile, tiles = tiles_x * ((tex_h + kTile - 1) / kTile);      // at most 4096^2
    const PSP P = {tex_block(pos, nrm, coverage, tex_h, tex_w, views, n_views, gains, power, cos_min, fade_px, depth_tol),
                   sizes, photos, depth, tiles_x, tiles, stat_cos_min, stat_lo, stat_hi,
                   (unsigned long long *)pair_count, (unsigned long long *)pair_sum};
    const int blocks = tiles < kStatGrid ? tiles : kStatGrid;
    hipLaunchKernelGGL(k_pair_stats, dim3((unsigned)blocks), dim3(kTile * kTile), 0, (hipStream_t)hip_stream, P);
    return t4d_launch_status(name);
}

T4D_EXPORT int t4d_projtex_consistency(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                       const float *views, int32_t n_views, const int32_t *sizes, const float *const *photos,
                                       const float *const *depth, int32_t power, double cos_min, double fade_px, double depth_tol,
                                       const double *gains, double reject_tol, double vote_cos_min, int32_t min_votes, uint32_t *skip,
                                       uint8_t *votes, void *hip_stream)
{
    const char *name = "t4d_projtex_consistency";            // (the image sides are per view, in `sizes` on the device: the kernel looks at them)
    if (const int rc = views_check(name, pos && nrm && coverage && views && sizes && photos && depth && skip && votes, n_views, kStatViews, 1, 1))
        return rc;
    if (const int rc = projtex_check(name, tex_h, tex_w, power, cos_min, fade_px, depth_tol)) return rc;
    if (!(reject_tol >= 0.0 && reject_tol <= kConsMax) || !(vote_cos_min >= -1.0 && vote_cos_min <= 1.0) || min_votes < 2 || min_votes > kStatViews)
        return t4d_fail(T4D_ERR_ARG, "%s: need reject_tol in [0, %g], vote_cos_min in [-1, 1] and min_votes in [2, %d]", name, kConsMax, kStatViews);
    const PCP P = {tex_block(pos, nrm, coverage, tex_h, tex_w, views, n_views, gains, power, cos_min, fade_px, depth_tol),
                   sizes, photos, depth, vote_cos_min, (int)llrint(reject_tol * kStatScale), min_votes, skip, votes};
    const dim3 grid((unsigned)((tex_w + kConsW - 1) / kConsW), (unsigned)((tex_h + kConsH - 1) / kConsH));
    hipLaunchKernelGGL(k_projtex_consist, grid, dim3(kConsLanes), (size_t)n_views * kConsLanes * sizeof(unsigned long long),
                       (hipStream_t)hip_stream, P);
    return t4d_launch_status(name);
}

T4D_EXPORT int t4d_projtex_low_band(const float *photos, const float *depth, int32_t n_views, int32_t h, int32_t w, int32_t radius,
                                    float *low, void *hip_stream)
{
    const char *name = "t4d_projtex_low_band";
    if (const int rc = views_check(name, photos && depth && low, n_views, kMaxViews, h, w)) return rc;
    if (radius < 0 || radius > kMaxRadius) return t4d_fail(T4D_ERR_ARG, "%s: radius must be in [0, %d], got %d", name, kMaxRadius, radius);
    if (low == photos) return t4d_fail(T4D_ERR_ARG, "%s: low must not be the photographs themselves", name);
    LBP P;
    P.photos = photos; P.depth = depth; P.low = low; P.H = h; P.W = w; P.R = radius;
    const dim3 grid((unsigned)((w + kLowW - 1) / kLowW), (unsigned)((h + kLowH - 1) / kLowH), (unsigned)(3 * n_views));
    hipLaunchKernelGGL(k_low_band, grid, dim3(kLowW * kLowStep), low_band_lds(radius), (hipStream_t)hip_stream, P);
    return t4d_launch_status(name);
}

T4D_EXPORT int t4d_project_texture_bands_flow(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                              const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos,
                                              const float *low, const float *depth, const double *gains, int32_t power, double cos_min,
                                              double fade_px, double depth_tol, float *low_color, float *weight, uint8_t *count,
                                              float *high, float *best_weight, const uint32_t *skip, int32_t skip_base, void *hip_stream,
                                              const int16_t *flows)
{
    const char *name = "t4d_project_texture_bands";
    if (const int rc = views_check(name, pos && nrm && coverage && views && photos && low && depth && low_color && weight && count && high && best_weight,
                                   n_views, kMaxViews, h, w))
        return rc;
    if (const int rc = projtex_check(name, tex_h, tex_w, power, cos_min, fade_px, depth_tol)) return rc;
    if (const int rc = skip_check(name, skip, skip_base, n_views)) return rc;
    if (const int rc = flows_check(name, flows)) return rc;
    const PBP P = {tex_block(pos, nrm, coverage, tex_h, tex_w, views, n_views, gains, power, cos_min, fade_px, depth_tol),
                   photos, low, depth, h, w, low_color, weight, high, best_weight, count, skip, skip_base, flows};
    const auto kernel = T4D_PROJTEX_INSTANCE(k_projtex_bands, gains, skip, flows);
    hipLaunchKernelGGL(kernel, tile_grid(tex_h, tex_w), dim3(kTile * kTile), 0, (hipStream_t)hip_stream, P);
    return t4d_launch_status(name);
}

T4D_EXPORT int t4d_project_texture_bands_skip(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                              const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos,
                                              const float *low, const float *depth, const double *gains, int32_t power, double cos_min,
                                              double fade_px, double depth_tol, float *low_color, float *weight, uint8_t *count,
                                              float *high, float *best_weight, const uint32_t *skip, int32_t skip_base, void *hip_stream)
{
    return t4d_project_texture_bands_flow(pos, nrm, coverage, tex_h, tex_w, views, n_views, h, w, photos, low, depth, gains, power,
                                          cos_min, fade_px, depth_tol, low_color, weight, count, high, best_weight, skip, skip_base,
                                          hip_stream, nullptr);
}

T4D_EXPORT int t4d_project_texture_bands(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                         const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos,
                                         const float *low, const float *depth, const double *gains, int32_t power, double cos_min,
                                         double fade_px, double depth_tol, float *low_color, float *weight, uint8_t *count,
                                         float *high, float *best_weight, void *hip_stream)
{
    return t4d_project_texture_bands_skip(pos, nrm, coverage, tex_h, tex_w, views, n_views, h, w, photos, low, depth, gains, power,
                                          cos_min, fade_px, depth_tol, low_color, weight, count, high, best_weight, nullptr, 0, hip_stream);
}
