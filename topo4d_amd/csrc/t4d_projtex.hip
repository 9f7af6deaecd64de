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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"

namespace {

constexpr int kTile = 16;                    // 16x16 texels per workgroup: a wave holds 4 rows of 16 neighbouring texels
constexpr int kMaxDim = 65536;               // texture and image sides: every grid stays below 2^31 workgroups
constexpr int kMaxViews = 255;               // count is a uint8
constexpr int kMaxPower = 8;
constexpr double kNear = 0.01;               // the mesh renderer's near plane

struct PTP {
    const float *pos, *nrm, *views, *photos, *depth;
    const uint8_t *coverage;
    int th, tw, V, H, W, power, mode;
    double cos_min, fade_px, depth_lim;      // depth_lim = 1 + depth_tol
    float *color, *weight;
    uint8_t *count;
};

__global__ __launch_bounds__(kTile * kTile) void k_projtex(const PTP P)
{
#pragma clang fp contract(off)
    const int tx = (int)blockIdx.x * kTile + (int)(threadIdx.x % kTile), ty = (int)blockIdx.y * kTile + (int)(threadIdx.x / kTile);
    if (tx >= P.tw || ty >= P.th) return;
    const size_t at = (size_t)ty * (size_t)P.tw + (size_t)tx;
    if (P.coverage[at] == 0) {                                              // most of a face's UV layout: one byte read, zeros out
        P.color[3 * at] = 0.0f; P.color[3 * at + 1] = 0.0f; P.color[3 * at + 2] = 0.0f;
        P.weight[at] = 0.0f;
        P.count[at] = 0;
        return;
    }
    double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int cnt = 0;
    const double nx = (double)P.nrm[3 * at], ny = (double)P.nrm[3 * at + 1], nz = (double)P.nrm[3 * at + 2];
    const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
    if (nl > 0.0) {
        const double X = (double)P.pos[3 * at], Y = (double)P.pos[3 * at + 1], Z = (double)P.pos[3 * at + 2];
        const double nhx = nx / nl, nhy = ny / nl, nhz = nz / nl;
        const double Wd = (double)P.W, Hd = (double)P.H, xmax = (double)(P.W - 1), ymax = (double)(P.H - 1);
        const size_t plane = (size_t)P.H * (size_t)P.W;
        for (int v = 0; v < P.V; ++v) {
            const float *vm = P.views + (size_t)v * T4D_VIEW_FLOATS, *pm = vm + 16;
            // 1. projection
            const double cx = (((double)pm[0] * X + (double)pm[4] * Y) + (double)pm[8] * Z) + (double)pm[12];
            const double cy = (((double)pm[1] * X + (double)pm[5] * Y) + (double)pm[9] * Z) + (double)pm[13];
            const double cw = (((double)pm[3] * X + (double)pm[7] * Y) + (double)pm[11] * Z) + (double)pm[15];
            const double px = ((cx / cw + 1.0) * Wd - 1.0) * 0.5;
            const double py = ((cy / cw + 1.0) * Hd - 1.0) * 0.5;
            const double z = (((double)vm[2] * X + (double)vm[6] * Y) + (double)vm[10] * Z) + (double)vm[14];
            if (!(z > kNear)) continue;
            // 2. the four taps inside the image (a NaN fails the comparisons)
            const double fx0 = floor(px), fy0 = floor(py);
            if (!(fx0 >= 0.0 && fx0 + 1.0 <= xmax && fy0 >= 0.0 && fy0 + 1.0 <= ymax)) continue;
            // 4. facing (before the gathers: it needs no memory)
            const double t0 = (double)vm[12], t1 = (double)vm[13], t2 = (double)vm[14];
            const double ex = -(((double)vm[0] * t0 + (double)vm[1] * t1) + (double)vm[2] * t2) - X;
            const double ey = -(((double)vm[4] * t0 + (double)vm[5] * t1) + (double)vm[6] * t2) - Y;
            const double ez = -(((double)vm[8] * t0 + (double)vm[9] * t1) + (double)vm[10] * t2) - Z;
            const double el = sqrt((ex * ex + ey * ey) + ez * ez);
            const double cs = (nhx * (ex / el) + nhy * (ey / el)) + nhz * (ez / el);
            if (!(cs >= P.cos_min)) continue;
            // 3. visibility
            const size_t tap = (size_t)(int)fy0 * (size_t)P.W + (size_t)(int)fx0;
            const float *dp = P.depth + (size_t)v * plane + tap;
            const double d00 = (double)dp[0], d01 = (double)dp[1], d10 = (double)dp[P.W], d11 = (double)dp[P.W + 1];
            if (!(d00 > 0.0 && d01 > 0.0 && d10 > 0.0 && d11 > 0.0)) continue;
            if (!(z <= d00 * P.depth_lim && z <= d01 * P.depth_lim && z <= d10 * P.depth_lim && z <= d11 * P.depth_lim)) continue;
            // 5. weight
            double w = 1.0;
            for (int k = 0; k < P.power; ++k) w = w * cs;
            if (P.fade_px > 0.0) {
                const double m = fmin(fmin(px, xmax - px), fmin(py, ymax - py));
                const double f = m / P.fade_px;
                if (f < 1.0) w = w * f;
            }
            if (!(w > 0.0)) continue;
            ++cnt;
            if (P.mode == T4D_PROJTEX_BEST && !(w > sw)) continue;
            // 6. sample
            const double fx = px - fx0, fy = py - fy0, gx = 1.0 - fx, gy = 1.0 - fy;
            const float *ph = P.photos + (size_t)v * 3 * plane + tap;
            double s[3];
            for (int c = 0; c < 3; ++c) {
                const float *q = ph + (size_t)c * plane;
                const double a = gx * (double)q[0] + fx * (double)q[1], b = gx * (double)q[P.W] + fx * (double)q[P.W + 1];
                s[c] = gy * a + fy * b;
            }
            // 7. accumulate
            if (P.mode == T4D_PROJTEX_BEST) {
                sw = w; s0 = s[0]; s1 = s[1]; s2 = s[2];
            } else {
                sw = sw + w;
                s0 = s0 + w * s[0]; s1 = s1 + w * s[1]; s2 = s2 + w * s[2];
            }
        }
        if (cnt && P.mode != T4D_PROJTEX_BEST) { s0 = s0 / sw; s1 = s1 / sw; s2 = s2 / sw; }
    }
    P.color[3 * at] = (float)s0;
    P.color[3 * at + 1] = (float)s1;
    P.color[3 * at + 2] = (float)s2;
    P.weight[at] = (float)sw;
    P.count[at] = (uint8_t)cnt;
}

}  // namespace

T4D_EXPORT int t4d_project_texture(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                   const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos, const float *depth,
                                   int32_t power, double cos_min, double fade_px, double depth_tol, int32_t mode, float *color,
                                   float *weight, uint8_t *count, void *hip_stream)
{
    if (!pos || !nrm || !coverage || !views || !photos || !depth || !color || !weight || !count)
        return t4d_fail(T4D_ERR_ARG, "t4d_project_texture: NULL buffer");
    if (tex_h < 1 || tex_w < 1 || tex_h > kMaxDim || tex_w > kMaxDim || h < 1 || w < 1 || h > kMaxDim || w > kMaxDim)
        return t4d_fail(T4D_ERR_ARG, "t4d_project_texture: need 1 <= sides <= %d, got a %d x %d texture and %d x %d images", kMaxDim,
                        tex_h, tex_w, h, w);
    if (n_views < 1 || n_views > kMaxViews)
        return t4d_fail(T4D_ERR_ARG, "t4d_project_texture: n_views must be in [1, %d], got %d", kMaxViews, n_views);
    if (power < 0 || power > kMaxPower) return t4d_fail(T4D_ERR_ARG, "t4d_project_texture: power must be in [0, %d], got %d", kMaxPower, power);
    if (mode != T4D_PROJTEX_WEIGHTED && mode != T4D_PROJTEX_BEST)
        return t4d_fail(T4D_ERR_ARG, "t4d_project_texture: mode must be T4D_PROJTEX_WEIGHTED or T4D_PROJTEX_BEST, got %d", mode);
    if (!(cos_min >= -1.0 && cos_min <= 1.0) || !(fade_px >= 0.0 && fade_px <= (double)kMaxDim) || !(depth_tol >= 0.0 && depth_tol <= 1.0))
        return t4d_fail(T4D_ERR_ARG, "t4d_project_texture: need cos_min in [-1, 1], fade_px in [0, %d] and depth_tol in [0, 1]", kMaxDim);
    PTP P;
    P.pos = pos; P.nrm = nrm; P.views = views; P.photos = photos; P.depth = depth; P.coverage = coverage;
    P.th = tex_h; P.tw = tex_w; P.V = n_views; P.H = h; P.W = w; P.power = power; P.mode = mode;
    P.cos_min = cos_min; P.fade_px = fade_px; P.depth_lim = 1.0 + depth_tol;
    P.color = color; P.weight = weight; P.count = count;
    const dim3 grid((unsigned)((tex_w + kTile - 1) / kTile), (unsigned)((tex_h + kTile - 1) / kTile));
    hipLaunchKernelGGL(k_projtex, grid, dim3(kTile * kTile), 0, (hipStream_t)hip_stream, P);
    return t4d_launch_status("t4d_project_texture");
}
