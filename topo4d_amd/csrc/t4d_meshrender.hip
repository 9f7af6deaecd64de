// t4d_meshrender.hip — z-buffered textured-mesh render into calibrated views, and per-view image metrics, on MI355X.
//
// What a finished run is scored with (topo4d_amd/meshrender.py, topo4d_amd/evaluate.py): each frame's face.obj + face.png
// rendered into every camera of the frame and compared with the photograph.  The render's rules are fixed so that a numpy
// float64 restatement (tests/meshrender_ref.py) reproduces every output bit:
//   projection   clip = proj (x,y,z,1), ndc = clip.xyz / clip.w, pixel = ((ndc + 1) S - 1) / 2 (the splat rasterizer's preprocess),
//                view z = (view (x,y,z,1)).z; a triangle with a corner at view z <= 0.01 (setup_camera's near plane) is dropped
//   coverage     pixel (x, y) samples the point (x, y); float64 edge functions of the positively oriented triangle, every edge
//                evaluated from its lexicographically smaller end point (a shared edge gives its two triangles exactly opposite
//                values), inside when all three are >= 0 with the top-left rule for exact zeros; zero-area triangles skipped
//   depth        1 / sum(b_i / z_i); a pixel keeps the lexicographic minimum of (float32 bits of the depth, triangle index)
//   texture      uv = sum beta_i uv_i, beta_i = (b_i / z_i) / sum; texel x = u (Wt - 1), y = (Ht - v (Ht - 1)) - 1 (process_uv),
//                clamped; bilinear, or nearest with round-half-even; a uint8 texel reads as x / 255.0
// Everything is float64 with FP contraction off; outputs are rounded to float32 once.  The launch set follows the UV bake of
// t4d_texture.hip:
//   k_mr_setup<count> / t4d_scan_bins / k_mr_setup<fill>   per-(view, triangle) record, then (triangle, 16x16 tile)
//                pairs binned with a count / scan / fill; on a pair-capacity overflow the host learns the size and retries
//   k_mr_tile    one workgroup per (view, tile): a triangle visits the pixels of its box inside the tile (16 lanes per record),
//                a covered pixel enters an LDS 64-bit minimum with its key; then every pixel re-evaluates its winner with the very
//                same operations and shades it.  No float atomics: the result does not depend on the order of arrival.
// k_im_tile / k_im_final: the metrics of a render against its target (SSIM map in float32 as external.calc_ssim computes it,
// every sum in float64 in a fixed order).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/topo4d_raster.h"
#include "t4d_block.h"
#include "t4d_host.h"

namespace {

constexpr int kTile = 16;                    // 16x16 pixels per bin and per workgroup: one pixel per thread in the write-out
constexpr int kBlock = 256;
constexpr int kStage = 64;                   // records staged in LDS per round (96 B each)
constexpr int kGroup = 16;                   // lanes per record in the coverage loop
constexpr double kNear = 0.01;               // setup_camera's near plane
constexpr unsigned long long kNoKey = ~0ull;

// Per (view, triangle): the projected corners, their view depths, the signed doubled area and the pixel box.  96 bytes.
struct MRec {
    double x0, y0, x1, y1, x2, y2;
    double z0, z1, z2;
    double A;                                // edge function of (p0, p1) at p2; 0 marks a dropped triangle
    uint32_t bx;                             // x_min | x_max << 16 (pixels); x_min > x_max: no pixel
    uint32_t by;                             // y_min | y_max << 16
    uint32_t owns;                           // bit i: edge i (opposite corner i) owns the points where its edge function is 0
    uint32_t pad;
};
static_assert(sizeof(MRec) == 96, "MRec must stay 96 bytes");

struct MRP {
    const float *vertices, *uvs, *views, *texf;
    const int32_t *tri, *uvtri;
    const uint8_t *texb;
    int nvert, ntri, nuv, th, tw, V, H, W, mapping;
    int tx, ty, tpv, nb;                     // tiles in x, in y, per view; bins
    uint32_t cap;
    float bg0, bg1, bg2;
    MRec *recs;
    uint32_t *bin_count, *bin_cursor, *bin_off, *list;
    float *color, *depth;
    int32_t *index;
};

// edge function of the segment a-b at p, always evaluated from the lexicographically smaller end point: E(a,b,p) = -E(b,a,p) exactly
__device__ __forceinline__ double edge_fn(const double ax, const double ay, const double bx, const double by, const double px,
                                          const double py)
{
#pragma clang fp contract(off)
    if (ax < bx || (ax == bx && ay < by)) return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
    return -((ax - bx) * (py - by) - (ay - by) * (px - bx));
}

// the directed edge a -> b of the positively oriented triangle owns its zero points when it points up, or right along a row
__device__ __forceinline__ bool edge_owns(const double ax, const double ay, const double bx, const double by)
{
    const double dx = bx - ax, dy = by - ay;
    return dy < 0 || (dy == 0 && dx > 0);
}

// pixel -> screen, view depth of one vertex through one packed view record (include/topo4d_raster.h: column-major matrices)
__device__ __forceinline__ void project(const float *vr, const int H, const int W, const double X, const double Y, const double Z,
                                        double &px, double &py, double &vz)
{
#pragma clang fp contract(off)
    const float *vm = vr, *pm = vr + 16;
    const double cx = (double)pm[0] * X + (double)pm[4] * Y + (double)pm[8] * Z + (double)pm[12];
    const double cy = (double)pm[1] * X + (double)pm[5] * Y + (double)pm[9] * Z + (double)pm[13];
    const double cw = (double)pm[3] * X + (double)pm[7] * Y + (double)pm[11] * Z + (double)pm[15];
    const double nx = cx / cw, ny = cy / cw;
    px = ((nx + 1.0) * (double)W - 1.0) * 0.5;
    py = ((ny + 1.0) * (double)H - 1.0) * 0.5;
    vz = (double)vm[2] * X + (double)vm[6] * Y + (double)vm[10] * Z + (double)vm[14];
}

__device__ void setup_record(const MRP &P, const int v, const int f, MRec &r)
{
#pragma clang fp contract(off)
    memset(&r, 0, sizeof(r));
    r.bx = 1u; r.by = 1u;                                                    // x_min 1 > x_max 0: no pixel
    const int i0 = P.tri[3 * (size_t)f], i1 = P.tri[3 * (size_t)f + 1], i2 = P.tri[3 * (size_t)f + 2];
    const int u0 = P.uvtri[3 * (size_t)f], u1 = P.uvtri[3 * (size_t)f + 1], u2 = P.uvtri[3 * (size_t)f + 2];
    if (min(i0, min(i1, i2)) < 0 || max(i0, max(i1, i2)) >= P.nvert || min(u0, min(u1, u2)) < 0 || max(u0, max(u1, u2)) >= P.nuv)
        return;                                                              // (the host checks the indices; nothing is read out of range)
    const float *vr = P.views + (size_t)v * T4D_VIEW_FLOATS;
    project(vr, P.H, P.W, P.vertices[3 * (size_t)i0], P.vertices[3 * (size_t)i0 + 1], P.vertices[3 * (size_t)i0 + 2], r.x0, r.y0, r.z0);
    project(vr, P.H, P.W, P.vertices[3 * (size_t)i1], P.vertices[3 * (size_t)i1 + 1], P.vertices[3 * (size_t)i1 + 2], r.x1, r.y1, r.z1);
    project(vr, P.H, P.W, P.vertices[3 * (size_t)i2], P.vertices[3 * (size_t)i2 + 1], P.vertices[3 * (size_t)i2 + 2], r.x2, r.y2, r.z2);
    if (!(r.z0 > kNear && r.z1 > kNear && r.z2 > kNear)) return;
    const double A = edge_fn(r.x0, r.y0, r.x1, r.y1, r.x2, r.y2);
    if (!(A > 0 || A < 0)) return;                                           // zero area (or NaN)
    const double lo_x = ceil(fmin(r.x0, fmin(r.x1, r.x2))), hi_x = floor(fmax(r.x0, fmax(r.x1, r.x2)));
    const double lo_y = ceil(fmin(r.y0, fmin(r.y1, r.y2))), hi_y = floor(fmax(r.y0, fmax(r.y1, r.y2)));
    if (!(isfinite(lo_x) && isfinite(hi_x) && isfinite(lo_y) && isfinite(hi_y))) return;
    const double cx0 = fmax(lo_x, 0.0), cx1 = fmin(hi_x, (double)(P.W - 1)), cy0 = fmax(lo_y, 0.0), cy1 = fmin(hi_y, (double)(P.H - 1));
    if (cx0 > cx1 || cy0 > cy1) return;
    r.A = A;
    r.bx = (uint32_t)cx0 | (uint32_t)cx1 << 16;
    r.by = (uint32_t)cy0 | (uint32_t)cy1 << 16;
    const bool pos = A > 0;                                                  // edge i runs p(i+1) -> p(i+2), reversed when A < 0
    const bool o0 = pos ? edge_owns(r.x1, r.y1, r.x2, r.y2) : edge_owns(r.x2, r.y2, r.x1, r.y1);
    const bool o1 = pos ? edge_owns(r.x2, r.y2, r.x0, r.y0) : edge_owns(r.x0, r.y0, r.x2, r.y2);
    const bool o2 = pos ? edge_owns(r.x0, r.y0, r.x1, r.y1) : edge_owns(r.x1, r.y1, r.x0, r.y0);
    r.owns = (o0 ? 1u : 0u) | (o1 ? 2u : 0u) | (o2 ? 4u : 0u);
}

struct Hit { double q0, q1, q2, S; };

// coverage and perspective terms of record r at pixel (px, py): false when the pixel is outside (or the sum is not positive)
__device__ __forceinline__ bool eval_pixel(const MRec &r, const double px, const double py, Hit &h)
{
#pragma clang fp contract(off)
    const bool pos = r.A > 0;
    double e0 = edge_fn(r.x1, r.y1, r.x2, r.y2, px, py);
    double e1 = edge_fn(r.x2, r.y2, r.x0, r.y0, px, py);
    double e2 = edge_fn(r.x0, r.y0, r.x1, r.y1, px, py);
    if (!pos) { e0 = -e0; e1 = -e1; e2 = -e2; }
    const bool in = (e0 > 0 || (e0 == 0 && (r.owns & 1u))) && (e1 > 0 || (e1 == 0 && (r.owns & 2u))) &&
                    (e2 > 0 || (e2 == 0 && (r.owns & 4u)));
    if (!in) return false;
    const double aA = fabs(r.A);
    h.q0 = (e0 / aA) / r.z0;
    h.q1 = (e1 / aA) / r.z1;
    h.q2 = (e2 / aA) / r.z2;
    h.S = h.q0 + h.q1 + h.q2;
    return h.S > 0;
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_mr_setup(const MRP P)
{
    const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= (size_t)P.V * P.ntri) return;
    const int v = (int)(g / P.ntri), f = (int)(g % P.ntri);
    MRec r;
    if (FILL) r = P.recs[g];
    else {
        setup_record(P, v, f, r);
        P.recs[g] = r;
    }
    const int x0 = (int)(r.bx & 0xffffu), x1 = (int)(r.bx >> 16), y0 = (int)(r.by & 0xffffu), y1 = (int)(r.by >> 16);
    if (x0 > x1 || y0 > y1) return;
    for (int ty = y0 / kTile; ty <= y1 / kTile; ty++)
        for (int tx = x0 / kTile; tx <= x1 / kTile; tx++) {
            const int b = v * P.tpv + ty * P.tx + tx;
            if (FILL) {
                const uint32_t pos = P.bin_off[b] + atomicAdd(&P.bin_cursor[b], 1u);
                if (pos < P.cap) P.list[pos] = (uint32_t)f;
            } else {
                atomicAdd(&P.bin_count[b], 1u);
            }
        }
}

__device__ __forceinline__ double texel(const MRP &P, const int iy, const int ix, const int c)
{
    const size_t o = ((size_t)iy * P.tw + ix) * 3 + c;
    return P.texf ? (double)P.texf[o] : (double)P.texb[o] / 255.0;
}

// shade the winner of a pixel: uv from the perspective-correct weights, then the texture
__device__ __forceinline__ void shade(const MRP &P, const int f, const Hit &h, double col[3])
{
#pragma clang fp contract(off)
    const double b0 = h.q0 / h.S, b1 = h.q1 / h.S, b2 = h.q2 / h.S;
    const int u0 = P.uvtri[3 * (size_t)f], u1 = P.uvtri[3 * (size_t)f + 1], u2 = P.uvtri[3 * (size_t)f + 2];
    const double u = b0 * (double)P.uvs[2 * (size_t)u0] + b1 * (double)P.uvs[2 * (size_t)u1] + b2 * (double)P.uvs[2 * (size_t)u2];
    const double v = b0 * (double)P.uvs[2 * (size_t)u0 + 1] + b1 * (double)P.uvs[2 * (size_t)u1 + 1] + b2 * (double)P.uvs[2 * (size_t)u2 + 1];
    const double wm = (double)(P.tw - 1), hm = (double)(P.th - 1);
    double tx = u * wm;
    double ty = ((double)P.th - v * hm) - 1.0;
    if (!(tx > 0)) tx = 0;
    if (tx > wm) tx = wm;
    if (!(ty > 0)) ty = 0;
    if (ty > hm) ty = hm;
    if (P.mapping == 1) {                                          // nearest, numpy's round (half to even)
        const int ix = (int)rint(tx), iy = (int)rint(ty);
        for (int c = 0; c < 3; c++) col[c] = texel(P, iy, ix, c);
        return;
    }
    const double fx0 = floor(tx), fy0 = floor(ty);
    const double fx = tx - fx0, fy = ty - fy0;
    const int ix0 = (int)fx0, iy0 = (int)fy0, ix1 = min(ix0 + 1, P.tw - 1), iy1 = min(iy0 + 1, P.th - 1);
    for (int c = 0; c < 3; c++) {
        const double t00 = texel(P, iy0, ix0, c), t01 = texel(P, iy0, ix1, c), t10 = texel(P, iy1, ix0, c), t11 = texel(P, iy1, ix1, c);
        col[c] = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t01) + fy * ((1.0 - fx) * t10 + fx * t11);
    }
}

__global__ __launch_bounds__(kBlock) void k_mr_tile(const MRP P)
{
#pragma clang fp contract(off)
    __shared__ MRec s_rec[kStage];
    __shared__ uint32_t s_idx[kStage], s_box[kStage];
    __shared__ unsigned long long s_key[kTile * kTile];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int b = blockIdx.x, v = b / P.tpv, t = b % P.tpv;
    const int tx0 = (t % P.tx) * kTile, ty0 = (t / P.tx) * kTile;
    const uint32_t n = P.bin_count[b], off = P.bin_off[b];
    s_key[tid] = kNoKey;
    for (uint32_t base = 0; base < n; base += kStage) {
        const int cnt = (int)min((uint32_t)kStage, n - base);
        __syncthreads();
        if (tid < cnt) {
            const uint32_t f = P.list[off + base + tid];
            const MRec r = P.recs[(size_t)v * P.ntri + f];
            s_rec[tid] = r;
            s_idx[tid] = f;
            const int x_lo = max((int)(r.bx & 0xffffu), tx0) - tx0, x_hi = min((int)(r.bx >> 16), tx0 + kTile - 1) - tx0;
            const int y_lo = max((int)(r.by & 0xffffu), ty0) - ty0, y_hi = min((int)(r.by >> 16), ty0 + kTile - 1) - ty0;
            s_box[tid] = (x_hi < x_lo || y_hi < y_lo) ? 1u : (uint32_t)x_lo | (uint32_t)x_hi << 8 | (uint32_t)y_lo << 16 | (uint32_t)y_hi << 24;
        }
        __syncthreads();
        constexpr int kPerWave = 64 / kGroup;
        const int grp = lane / kGroup, hl = lane % kGroup;
        for (int k0 = kPerWave * wave; k0 < cnt; k0 += kPerWave * (kBlock / 64)) {
            const int k = k0 + grp;
            if (k >= cnt) continue;
            const uint32_t box = s_box[k];
            const int bx_lo = (int)(box & 0xffu), bx_hi = (int)((box >> 8) & 0xffu), by_lo = (int)((box >> 16) & 0xffu), by_hi = (int)(box >> 24);
            const int rw = bx_hi - bx_lo + 1, rh = by_hi - by_lo + 1;
            const int npx = rw > 0 ? rw * rh : 0;
            const MRec &r = s_rec[k];
            const unsigned long long low = s_idx[k];
            for (int p = hl; p < npx; p += kGroup) {
                const int lx = bx_lo + p % rw, ly = by_lo + p / rw;
                Hit h;
                if (eval_pixel(r, (double)(tx0 + lx), (double)(ty0 + ly), h)) {
                    const float d = (float)(1.0 / h.S);
                    atomicMin(&s_key[ly * kTile + lx], ((unsigned long long)__float_as_uint(d) << 32) | low);
                }
            }
        }
    }
    __syncthreads();
    const int x = tx0 + (tid % kTile), y = ty0 + tid / kTile;
    if (x >= P.W || y >= P.H) return;
    const size_t plane = (size_t)P.H * P.W, o = (size_t)y * P.W + x;
    const unsigned long long key = s_key[tid];
    float *col = P.color + (size_t)v * 3 * plane + o;
    if (key == kNoKey) {
        col[0] = P.bg0; col[plane] = P.bg1; col[2 * plane] = P.bg2;
        P.depth[(size_t)v * plane + o] = 0.f;
        P.index[(size_t)v * plane + o] = -1;
        return;
    }
    const int f = (int)(uint32_t)key;
    const MRec r = P.recs[(size_t)v * P.ntri + f];
    Hit h;
    eval_pixel(r, (double)x, (double)y, h);                        // the same record and operations as the loop above: covered
    double c[3];
    shade(P, f, h, c);
    col[0] = (float)c[0]; col[plane] = (float)c[1]; col[2 * plane] = (float)c[2];
    P.depth[(size_t)v * plane + o] = (float)(1.0 / h.S);
    P.index[(size_t)v * plane + o] = f;
}

struct MRLayout { size_t total_, bin_count, bin_cursor, zero_end, bin_off, chunk_sum, recs, list, bytes; };

MRLayout mr_layout(int V, int ntri, int h, int w, int64_t cap)
{
    const size_t nb = (size_t)V * ((w + kTile - 1) / kTile) * ((h + kTile - 1) / kTile);
    MRLayout L;
    size_t o = 0;
    L.total_ = o;     o = align_up(o + 8);
    L.bin_count = o;  o = align_up(o + nb * 4);
    L.bin_cursor = o; o = align_up(o + nb * 4);
    L.zero_end = o;
    L.bin_off = o;    o = align_up(o + nb * 4);
    L.chunk_sum = o;  o = align_up(o + ((nb + kScanBinsChunk - 1) / kScanBinsChunk) * 4);
    L.recs = o;       o = align_up(o + (size_t)V * ntri * sizeof(MRec));
    L.list = o;       o = align_up(o + (size_t)cap * 4);
    L.bytes = o;
    return L;
}

constexpr int kMaxSide = 32768;

bool mr_shape_ok(int V, int ntri, int h, int w)
{
    return V >= 1 && ntri >= 0 && h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide &&
           (size_t)V * ((w + kTile - 1) / kTile) * ((h + kTile - 1) / kTile) < 0x7fffffffull && (size_t)V * ntri < 0x7fffffffull;
}

// ---- metrics -----------------------------------------------------------------------------------------------------------------------
constexpr int kR = 5, kWin = 11, kPatch = kTile + 2 * kR;          // 26 x 26 input patch per 16 x 16 output tile
constexpr int kParts = 7;                                          // per tile: sum d^2 of channels 0..2 (all pixels); masked sum |d|, sum d^2, count, sum SSIM
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct IMP {
    int V, H, W, tx, tpv;
    const float *render, *target, *mask;
    const int32_t *coverage;
    double *part, *out;
    float win[kWin];
};

__global__ __launch_bounds__(kBlock) void k_im_tile(const IMP P)
{
#pragma clang fp contract(off)
    __shared__ float s_x[kPatch][kPatch], s_y[kPatch][kPatch];
    __shared__ float s_h[5][kPatch][kTile];
    __shared__ double s_red[kBlock / 64][kParts];
    const int tid = threadIdx.x, b = blockIdx.x, v = b / P.tpv, t = b % P.tpv;
    const int tx0 = (t % P.tx) * kTile, ty0 = (t / P.tx) * kTile;
    const int lx = tid % kTile, ly = tid / kTile, x = tx0 + lx, y = ty0 + ly;
    const bool inside = x < P.W && y < P.H;
    const size_t plane = (size_t)P.H * P.W, o = (size_t)y * P.W + x;
    bool sel = false;
    if (inside) {
        sel = P.coverage ? P.coverage[(size_t)v * plane + o] >= 0 : true;
        if (P.mask && !(P.mask[(size_t)v * plane + o] > 0.5f)) sel = false;
    }
    double acc[kParts] = {0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < 3; c++) {
        const float *X = P.render + ((size_t)v * 3 + c) * plane, *Y = P.target + ((size_t)v * 3 + c) * plane;
        __syncthreads();
        for (int e = tid; e < kPatch * kPatch; e += kBlock) {      // zero padding outside the image
            const int py = ty0 - kR + e / kPatch, px = tx0 - kR + e % kPatch;
            const bool ok = px >= 0 && px < P.W && py >= 0 && py < P.H;
            s_x[e / kPatch][e % kPatch] = ok ? X[(size_t)py * P.W + px] : 0.f;
            s_y[e / kPatch][e % kPatch] = ok ? Y[(size_t)py * P.W + px] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < kPatch * kTile; e += kBlock) {        // horizontal pass of x, y, x^2, y^2, x y
            const int r = e / kTile, j = e % kTile;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int k = 0; k < kWin; k++) {
                const float xv = s_x[r][j + k], yv = s_y[r][j + k], w = P.win[k];
                a0 += w * xv; a1 += w * yv; a2 += w * (xv * xv); a3 += w * (yv * yv); a4 += w * (xv * yv);
            }
            s_h[0][r][j] = a0; s_h[1][r][j] = a1; s_h[2][r][j] = a2; s_h[3][r][j] = a3; s_h[4][r][j] = a4;
        }
        __syncthreads();
        if (!inside) continue;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kWin; k++)
#pragma unroll
            for (int q = 0; q < 5; q++) m[q] += P.win[k] * s_h[q][ly + k][lx];
        const double d = (double)s_x[ly + kR][lx + kR] - (double)s_y[ly + kR][lx + kR];
        acc[c] += d * d;
        if (!sel) continue;
        // external.py:100-111, float32 element-wise
        const float mu1_sq = m[0] * m[0], mu2_sq = m[1] * m[1], mu1_mu2 = m[0] * m[1];
        const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu1_mu2;
        const float ssim = ((2.f * mu1_mu2 + kC1) * (2.f * s12 + kC2)) / ((mu1_sq + mu2_sq + kC1) * (s1 + s2 + kC2));
        acc[3] += fabs(d);
        acc[4] += d * d;
        if (c == 0) acc[5] += 1.0;
        acc[6] += (double)ssim;
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int q = 0; q < kParts; q++) {
        const double s = wave_sum(acc[q]);
        if (lane == 0) s_red[wave][q] = s;
    }
    __syncthreads();
    if (tid < kParts) {
        double s = 0;
        for (int w = 0; w < kBlock / 64; w++) s += s_red[w][tid];
        P.part[(size_t)b * kParts + tid] = s;
    }
}

__global__ __launch_bounds__(kBlock) void k_im_final(const IMP P)
{
    __shared__ double s_red[kBlock / 64][kParts];
    const int v = blockIdx.x, tid = threadIdx.x;
    double acc[kParts] = {0, 0, 0, 0, 0, 0, 0};
    for (int t = tid; t < P.tpv; t += kBlock)
#pragma unroll
        for (int q = 0; q < kParts; q++) acc[q] += P.part[((size_t)v * P.tpv + t) * kParts + q];
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int q = 0; q < kParts; q++) {
        const double s = wave_sum(acc[q]);
        if (lane == 0) s_red[wave][q] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    double s[kParts];
    for (int q = 0; q < kParts; q++) {
        s[q] = 0;
        for (int w = 0; w < kBlock / 64; w++) s[q] += s_red[w][q];
    }
    const double npix = (double)P.H * (double)P.W;
    double psnr_full = 0;
    for (int c = 0; c < 3; c++) psnr_full += 20.0 * log10(1.0 / sqrt(s[c] / npix));
    psnr_full /= 3.0;
    const double cnt = s[5], nval = 3.0 * cnt;
    const double mse = s[4] / nval;
    double *out = P.out + (size_t)v * T4D_METRICS_FIELDS;
    out[0] = psnr_full;
    out[1] = cnt;
    out[2] = s[3] / nval;
    out[3] = mse;
    out[4] = 20.0 * log10(1.0 / sqrt(mse));
    out[5] = s[6] / nval;
}

}  // namespace

T4D_EXPORT size_t t4d_mesh_render_scratch_bytes(int32_t n_views, int32_t n_tri, int32_t h, int32_t w, int64_t pair_capacity)
{
    if (!mr_shape_ok(n_views, n_tri, h, w) || pair_capacity < 1 || pair_capacity > 0x7fffffffLL) return 0;
    return mr_layout(n_views, n_tri, h, w, pair_capacity).bytes;
}

T4D_EXPORT int t4d_mesh_render(const float *vertices, int32_t n_vert, const int32_t *triangles, const int32_t *uv_triangles, int32_t n_tri,
                               const float *uvs, int32_t n_uv, const void *texture, int32_t tex_is_float32, int32_t tex_h, int32_t tex_w,
                               const float *views, int32_t n_views, int32_t h, int32_t w, const float *background, int32_t mapping,
                               float *color, float *depth, int32_t *tri_index, void *scratch, size_t scratch_bytes,
                               int64_t pair_capacity, int64_t *pairs_needed, void *hip_stream)
{
    if (!vertices || !triangles || !uv_triangles || !uvs || !texture || !views || !background || !color || !depth || !tri_index ||
        !scratch || n_vert < 1 || n_uv < 1 || tex_h < 1 || tex_w < 1 || (tex_is_float32 != 0 && tex_is_float32 != 1))
        return t4d_fail(T4D_ERR_ARG, "t4d_mesh_render: bad arguments");
    if (!mr_shape_ok(n_views, n_tri, h, w))
        return t4d_fail(T4D_ERR_ARG, "t4d_mesh_render: views/triangles/size out of range (1 <= h, w <= %d)", kMaxSide);
    if (mapping != T4D_MESH_BILINEAR && mapping != T4D_MESH_NEAREST)
        return t4d_fail(T4D_ERR_ARG, "t4d_mesh_render: mapping must be T4D_MESH_BILINEAR or T4D_MESH_NEAREST");
    if (pair_capacity < 1 || pair_capacity > 0x7fffffffLL) return t4d_fail(T4D_ERR_ARG, "t4d_mesh_render: pair_capacity out of range");
    const MRLayout L = mr_layout(n_views, n_tri, h, w, pair_capacity);
    if (scratch_bytes < L.bytes) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_mesh_render: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    char *sc = (char *)scratch;
    MRP P;
    memset(&P, 0, sizeof(P));
    P.vertices = vertices; P.uvs = uvs; P.views = views;
    P.texf = tex_is_float32 ? (const float *)texture : nullptr;
    P.texb = tex_is_float32 ? nullptr : (const uint8_t *)texture;
    P.tri = triangles; P.uvtri = uv_triangles;
    P.nvert = n_vert; P.ntri = n_tri; P.nuv = n_uv; P.th = tex_h; P.tw = tex_w; P.V = n_views; P.H = h; P.W = w; P.mapping = mapping;
    P.tx = (w + kTile - 1) / kTile; P.ty = (h + kTile - 1) / kTile; P.tpv = P.tx * P.ty; P.nb = n_views * P.tpv;
    P.cap = (uint32_t)pair_capacity;
    P.bg0 = background[0]; P.bg1 = background[1]; P.bg2 = background[2];
    P.bin_count = (uint32_t *)(sc + L.bin_count);
    P.bin_cursor = (uint32_t *)(sc + L.bin_cursor);
    P.bin_off = (uint32_t *)(sc + L.bin_off);
    P.recs = (MRec *)(sc + L.recs);
    P.list = (uint32_t *)(sc + L.list);
    P.color = color; P.depth = depth; P.index = tri_index;
    if (pairs_needed) *pairs_needed = 0;
    T4D_HIP_CHECK(hipMemsetAsync(sc, 0, L.zero_end, stream));
    if (n_tri > 0) {
        const int gt = (int)(((size_t)n_views * n_tri + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_mr_setup<false>, dim3(gt), dim3(kBlock), 0, stream, P);
        unsigned long long *d_total = (unsigned long long *)(sc + L.total_);
        t4d_scan_bins(P.bin_count, P.nb, P.bin_off, (uint32_t *)(sc + L.chunk_sum), d_total, stream);
        unsigned long long total = 0;
        T4D_HIP_CHECK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, stream));
        T4D_HIP_CHECK(hipStreamSynchronize(stream));          // once per frame: the pair count decides the fill
        if (pairs_needed) *pairs_needed = (int64_t)total;
        if (total > (unsigned long long)pair_capacity)
            return t4d_fail(T4D_ERR_PAIR_OVERFLOW, "t4d_mesh_render: pair_capacity too small");
        hipLaunchKernelGGL(k_mr_setup<true>, dim3(gt), dim3(kBlock), 0, stream, P);
    }
    hipLaunchKernelGGL(k_mr_tile, dim3(P.nb), dim3(kBlock), 0, stream, P);
    return t4d_launch_status("t4d_mesh_render");
}

T4D_EXPORT size_t t4d_image_metrics_scratch_bytes(int32_t n_views, int32_t h, int32_t w)
{
    if (!mr_shape_ok(n_views, 0, h, w)) return 0;
    return align_up((size_t)n_views * ((w + kTile - 1) / kTile) * ((h + kTile - 1) / kTile) * kParts * sizeof(double));
}

T4D_EXPORT int t4d_image_metrics(int32_t n_views, int32_t h, int32_t w, const float *render, const float *target, const float *mask,
                                 const int32_t *coverage, double *out, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!render || !target || !out || !scratch) return t4d_fail(T4D_ERR_ARG, "t4d_image_metrics: bad arguments");
    if (!mr_shape_ok(n_views, 0, h, w))
        return t4d_fail(T4D_ERR_ARG, "t4d_image_metrics: views/size out of range (1 <= h, w <= %d)", kMaxSide);
    if (scratch_bytes < t4d_image_metrics_scratch_bytes(n_views, h, w))
        return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_image_metrics: scratch too small");
    IMP P;
    memset(&P, 0, sizeof(P));
    P.V = n_views; P.H = h; P.W = w; P.tx = (w + kTile - 1) / kTile; P.tpv = P.tx * ((h + kTile - 1) / kTile);
    P.render = render; P.target = target; P.mask = mask; P.coverage = coverage;
    P.part = (double *)scratch; P.out = out;
    {   // external.gaussian(11, 1.5) as torch builds it: float32 taps, then divided by their float32 sum
        float g[kWin], sum = 0.f;
        for (int k = 0; k < kWin; k++) {
            const double dx = (double)(k - kWin / 2);
            g[k] = (float)exp(-(dx * dx) / (2.0 * 1.5 * 1.5));
        }
        for (int k = 0; k < kWin; k++) sum += g[k];
        for (int k = 0; k < kWin; k++) P.win[k] = g[k] / sum;
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_im_tile, dim3(n_views * P.tpv), dim3(kBlock), 0, stream, P);
    hipLaunchKernelGGL(k_im_final, dim3(n_views), dim3(kBlock), 0, stream, P);
    return t4d_launch_status("t4d_image_metrics");
}
