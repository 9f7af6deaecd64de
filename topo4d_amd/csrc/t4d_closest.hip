// Exact closest point on a triangle soup (or a bare point cloud) for many query points: what scores a frame's exported mesh
// against its multi-view-stereo scan (topo4d_amd/scanscore.py).  It replaces the host route of trimesh.proximity.closest_point /
// open3d's RaycastingScene.compute_closest_points; the reference project computes no such quantity.
//
// Index: a uniform grid over the primitives' bounding box, padded by half a cell.  A primitive is listed in every cell its
// axis-aligned box overlaps (count -> scan -> fill, then each cell's list sorted ascending).  closest_grid() chooses the cell
// edge: 2 sqrt(A / n) with A the surface of the bounding box (n primitives on a surface are about sqrt(A / n) apart), at least
// the mean extent of a primitive's box (so that a primitive is listed about 8 times, not hundreds), at least 2^-10 of the largest
// extent, and grown by steps of 1.25 until the grid has at most 2^22 cells (a 16 MiB offset table, whatever the input).
//
// Query: one lane per query point, the queries counted and scattered by cell first so that neighbouring lanes walk the same
// lists.  Cube shells of growing Chebyshev radius r around the point's clamped cell; after shell r every primitive not yet seen
// lies beyond one of the six planes bounding the visited block (its listed cells are disjoint from the block on some axis).  The
// walk stops once best d2 <= face^2, with face the distance to the nearest such plane that is not the grid's border, less a
// margin of 2^-40 of the coordinates' magnitude: the rounding of the cell coordinates and of d2 is some 2^-52 of it, so an unseen
// primitive's computed d2 is strictly larger and the result equals a brute-force search.  With max_dist the walk also stops once
// face > max_dist.  Queries still open after kMaxShells shells go to k_closest_brute, one block per query over all primitives.
//
// The arithmetic (tests/scanscore_ref.py states it in numpy, bit for bit): float64, no contraction, dot(u,v) = (u0 v0 + u1 v1) +
// u2 v2; Ericson's region walk (Real-Time Collision Detection, 5.1.5) with quotients instead of a reciprocal; a triangle whose
// unnormalised normal is exactly zero, or whose interior weights do not come out >= 0 with a positive sum, is the nearest of its
// edges ab, bc, ca (the first wins a tie); an edge of zero length is its first end.  Equal d2: the lowest primitive index wins.
//
// Ray query (t4d_closest_raycast, what topo4d_amd/scanbake.py bakes a displacement map with): on a triangle index, per ray the
// triangle met at the smallest |t| within [t_lo, t_hi], by the hit rule of include/topo4d_raster.h; tests/scanray_ref.py applies
// it to every (ray, triangle) pair and the walk of k_closest_raycast equals that bit for bit.
#include <stdint.h>
#include <math.h>
#include <string.h>

#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxShells = 8;
constexpr int64_t kMaxCells = (int64_t)1 << 22;
constexpr int kBruteBlocks = 1024;

struct CGrid {
    double lo[3];
    double cell;
    double margin;
    int32_t dim[3];
    int32_t is_tri;
    int64_t n_prims;
    int64_t n_cells;
    uint64_t magic;
};
constexpr uint64_t kMagic = 0x7434645f636c6f73ull;

struct CLayout {
    size_t head, rec, start, work, bsum, entries, total;
};

unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

bool bbox_ok(const double *bbox)
{
    if (!bbox) return false;
    for (int a = 0; a < 3; a++)
        if (!isfinite(bbox[a]) || !isfinite(bbox[3 + a]) || bbox[a] > bbox[3 + a] || !isfinite(bbox[3 + a] - bbox[a])) return false;
    return true;
}

// the grid of a primitive set: a function of the bounding box, the count and the mean box extent only
CGrid closest_grid(const double *bbox, int64_t n, double mean_extent, int is_tri)
{
    CGrid g;
    memset(&g, 0, sizeof(g));
    const double e0 = bbox[3] - bbox[0], e1 = bbox[4] - bbox[1], e2 = bbox[5] - bbox[2];
    const double emax = fmax(e0, fmax(e1, e2));
    const double area = 2.0 * (e0 * e1 + e1 * e2 + e0 * e2);
    double cell = area > 0.0 ? 2.0 * sqrt(area / (double)n) : 2.0 * emax / (double)n;
    if (mean_extent > cell) cell = mean_extent;
    cell = fmax(cell, emax * 0x1p-10);
    if (!(cell > 0.0) || !isfinite(cell)) cell = 1.0;
    for (;;) {
        int64_t cells = 1;
        for (int a = 0; a < 3; a++) {
            const double d = floor(((bbox[3 + a] - bbox[a]) + cell) / cell) + 1.0;
            g.dim[a] = d > 4096.0 ? 4096 : (int32_t)d;
            cells *= g.dim[a];
        }
        if (cells <= kMaxCells && g.dim[0] < 4096 && g.dim[1] < 4096 && g.dim[2] < 4096) {
            g.n_cells = cells;
            break;
        }
        cell *= 1.25;
    }
    double mag = 0.0;
    for (int a = 0; a < 3; a++) {
        g.lo[a] = bbox[a] - 0.5 * cell;
        mag = fmax(mag, fmax(fabs(g.lo[a]), fabs(g.lo[a] + (double)(g.dim[a] + 1) * cell)));
    }
    g.cell = cell;
    g.margin = 0x1p-40 * (mag + cell);
    g.is_tri = is_tri;
    g.n_prims = n;
    g.magic = kMagic;
    return g;
}

CLayout closest_layout(const CGrid &g, int64_t entry_capacity)
{
    CLayout L;
    const int64_t words = g.n_cells + 1;
    size_t o = 0;
    L.head = o;    o += 256;
    L.rec = o;     o += align_up(sizeof(double) * (g.is_tri ? 9 : 3) * (size_t)g.n_prims);
    L.start = o;   o += align_up(sizeof(int32_t) * (size_t)words);
    L.work = o;    o += align_up(sizeof(int32_t) * (size_t)words);
    L.bsum = o;    o += align_up(sizeof(int32_t) * (size_t)t4d_scan_i32_sum_words(words));
    L.entries = o; o += align_up(sizeof(int32_t) * (size_t)entry_capacity);
    L.total = o;
    return L;
}

struct QLayout {
    size_t order, qcell, fall, total;
};

QLayout query_layout(int64_t nq)
{
    QLayout L;
    size_t o = 0;
    L.order = o; o += align_up(sizeof(int32_t) * (size_t)nq);
    L.qcell = o; o += align_up(sizeof(int32_t) * (size_t)nq);
    L.fall = o;  o += align_up(sizeof(int32_t) * (size_t)(nq + 1));  // [0]: count, then the open queries
    L.total = o;
    return L;
}

__device__ __forceinline__ int32_t cell_coord(double x, double lo, double cell, int32_t dim)
{
#pragma clang fp contract(off)
    const double f = floor((x - lo) / cell);
    return !(f > 0.0) ? 0 : f >= (double)dim ? dim - 1 : (int32_t)f;      // (a NaN goes to cell 0)
}

__device__ __forceinline__ int64_t cell_id(const CGrid &g, int32_t x, int32_t y, int32_t z)
{
    return x + (int64_t)g.dim[0] * (y + (int64_t)g.dim[1] * z);
}

// ---- build ----------------------------------------------------------------------------------------------------------------
// the primitive records in primitive order (a triangle's nine coordinates, or the point), so that the query reads one record
// per list entry instead of a face and three vertices
__global__ __launch_bounds__(kBlock) void k_closest_records(const double *v, const int32_t *faces, const CGrid *gp, double *rec)
{
    const CGrid g = *gp;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= g.n_prims) return;
    if (g.is_tri) {
        for (int k = 0; k < 3; k++) {
            const int64_t vi = faces[3 * i + k];
            for (int c = 0; c < 3; c++) rec[9 * i + 3 * k + c] = v[3 * vi + c];
        }
    } else {
        for (int c = 0; c < 3; c++) rec[3 * i + c] = v[3 * i + c];
    }
}

__device__ __forceinline__ void prim_cells(const CGrid &g, const double *rec, int64_t i, int32_t lo[3], int32_t hi[3])
{
    const int nv = g.is_tri ? 3 : 1;
    const double *r = rec + (g.is_tri ? 9 : 3) * i;
    for (int a = 0; a < 3; a++) {
        double mn = r[a], mx = r[a];
        for (int k = 1; k < nv; k++) {
            mn = fmin(mn, r[3 * k + a]);
            mx = fmax(mx, r[3 * k + a]);
        }
        lo[a] = cell_coord(mn, g.lo[a], g.cell, g.dim[a]);
        hi[a] = cell_coord(mx, g.lo[a], g.cell, g.dim[a]);
    }
}

// fill == 0: count a primitive into every cell its box overlaps; fill == 1: write it at the cell's cursor
__global__ __launch_bounds__(kBlock) void k_closest_bin(const CGrid *gp, const double *rec, int32_t *cnt_or_cursor, int32_t *entries,
                                                        int64_t capacity, int fill)
{
    const CGrid g = *gp;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= g.n_prims) return;
    int32_t lo[3], hi[3];
    prim_cells(g, rec, i, lo, hi);
    for (int32_t z = lo[2]; z <= hi[2]; z++)
        for (int32_t y = lo[1]; y <= hi[1]; y++)
            for (int32_t x = lo[0]; x <= hi[0]; x++) {
                const int32_t pos = atomicAdd(&cnt_or_cursor[cell_id(g, x, y, z)], 1);
                if (fill && (int64_t)pos < capacity) entries[pos] = (int32_t)i;
            }
}

// each cell's list in ascending primitive index (the atomics of the fill leave it in schedule order): heap sort, one lane a cell
__global__ __launch_bounds__(kBlock) void k_closest_sort_cells(const CGrid *gp, const int32_t *start, int32_t *entries)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= gp->n_cells) return;
    int32_t *a = entries + start[c];
    const int32_t n = start[c + 1] - start[c];
    if (n < 2) return;
    auto sift = [&](int32_t root, int32_t end) {
        for (;;) {
            int32_t child = 2 * root + 1;
            if (child >= end) return;
            if (child + 1 < end && a[child] < a[child + 1]) child++;
            if (a[root] >= a[child]) return;
            const int32_t t = a[root]; a[root] = a[child]; a[child] = t;
            root = child;
        }
    };
    for (int32_t i = n / 2 - 1; i >= 0; i--) sift(i, n);
    for (int32_t end = n - 1; end > 0; end--) {
        const int32_t t = a[0]; a[0] = a[end]; a[end] = t;
        sift(0, end);
    }
}

// ---- the closest point of one primitive -------------------------------------------------------------------------------------
struct Best {
    double d2;
    int32_t idx;
    double c[3];
};

__device__ __forceinline__ double dot3(const double *u, const double *v)
{
#pragma clang fp contract(off)
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

__device__ __forceinline__ double dist2(const double *p, const double *c)
{
#pragma clang fp contract(off)
    const double d[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    return dot3(d, d);
}

// closest point of segment a-b: a for a zero-length edge or t <= 0, b for t >= 1
__device__ __forceinline__ double seg_closest(const double *p, const double *a, const double *b, double *c)
{
#pragma clang fp contract(off)
    const double e[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const double ee = dot3(e, e);
    const double t = ee > 0.0 ? dot3(ap, e) / ee : 0.0;
    if (!(t > 0.0)) { c[0] = a[0]; c[1] = a[1]; c[2] = a[2]; }
    else if (t >= 1.0) { c[0] = b[0]; c[1] = b[1]; c[2] = b[2]; }
    else { c[0] = a[0] + t * e[0]; c[1] = a[1] + t * e[1]; c[2] = a[2] + t * e[2]; }
    return dist2(p, c);
}

__device__ __forceinline__ double edges_closest(const double *p, const double *a, const double *b, const double *c, double *out)
{
    double q[3];
    double best = seg_closest(p, a, b, out);
    double d = seg_closest(p, b, c, q);
    if (d < best) { best = d; out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; }
    d = seg_closest(p, c, a, q);
    if (d < best) { best = d; out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; }
    return best;
}

__device__ __forceinline__ double tri_closest(const double *p, const double *t, double *out)
{
#pragma clang fp contract(off)
    const double *a = t, *b = t + 3, *c = t + 6;
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    if (nx == 0.0 && ny == 0.0 && nz == 0.0) return edges_closest(p, a, b, c, out);
    const double ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; return dist2(p, out); }
    const double bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) { out[0] = b[0]; out[1] = b[1]; out[2] = b[2]; return dist2(p, out); }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
        const double v = d1 / (d1 - d3);
        out[0] = a[0] + v * ab[0]; out[1] = a[1] + v * ab[1]; out[2] = a[2] + v * ab[2];
        return dist2(p, out);
    }
    const double cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; return dist2(p, out); }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
        const double w = d2 / (d2 - d6);
        out[0] = a[0] + w * ac[0]; out[1] = a[1] + w * ac[1]; out[2] = a[2] + w * ac[2];
        return dist2(p, out);
    }
    const double va = d3 * d6 - d5 * d4;
    const double g43 = d4 - d3, g56 = d5 - d6;
    if (va <= 0.0 && g43 >= 0.0 && g56 >= 0.0) {
        const double w = g43 / (g43 + g56);
        out[0] = b[0] + w * (c[0] - b[0]); out[1] = b[1] + w * (c[1] - b[1]); out[2] = b[2] + w * (c[2] - b[2]);
        return dist2(p, out);
    }
    const double s = (va + vb) + vc;
    if (!(s > 0.0) || !(va >= 0.0) || !(vb >= 0.0) || !(vc >= 0.0)) return edges_closest(p, a, b, c, out);
    const double v = vb / s, w = vc / s;
    out[0] = (a[0] + ab[0] * v) + ac[0] * w; out[1] = (a[1] + ab[1] * v) + ac[1] * w; out[2] = (a[2] + ab[2] * v) + ac[2] * w;
    return dist2(p, out);
}

__device__ __forceinline__ void consider(const double *rec, int is_tri, int32_t prim, const double *p, Best &best)
{
    double c[3], d;
    if (is_tri) {
        d = tri_closest(p, rec + 9 * (int64_t)prim, c);
    } else {
        const double *r = rec + 3 * (int64_t)prim;
        c[0] = r[0]; c[1] = r[1]; c[2] = r[2];
        d = dist2(p, c);
    }
    if (d < best.d2 || (d == best.d2 && prim < best.idx)) {
        best.d2 = d; best.idx = prim; best.c[0] = c[0]; best.c[1] = c[1]; best.c[2] = c[2];
    }
}

// matched iff d2 <= max_dist^2; has_max == 0: every query is matched
__device__ __forceinline__ void write_result(const Best &best, int has_max, double max_dist, int64_t qi, double *out_d2,
                                             int32_t *out_idx, double *out_c)
{
#pragma clang fp contract(off)
    const bool ok = best.idx >= 0 && (!has_max || best.d2 <= max_dist * max_dist);
    out_d2[qi] = ok ? best.d2 : INFINITY;
    out_idx[qi] = ok ? best.idx : -1;
    for (int a = 0; a < 3; a++) out_c[3 * qi + a] = ok ? best.c[a] : 0.0;
}

// ---- query ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_closest_query_cells(const CGrid *gp, const double *q, int64_t nq, int32_t *qcell, int32_t *cnt)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nq) return;
    const CGrid g = *gp;
    const int64_t c = cell_id(g, cell_coord(q[3 * i], g.lo[0], g.cell, g.dim[0]), cell_coord(q[3 * i + 1], g.lo[1], g.cell, g.dim[1]),
                              cell_coord(q[3 * i + 2], g.lo[2], g.cell, g.dim[2]));
    qcell[i] = (int32_t)c;
    atomicAdd(&cnt[c], 1);
}

// queries grouped by cell (the order inside a cell depends on the schedule; no result does)
__global__ __launch_bounds__(kBlock) void k_closest_query_order(const int32_t *qcell, int64_t nq, int32_t *cursor, int32_t *order)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nq) return;
    order[atomicAdd(&cursor[qcell[i]], 1)] = (int32_t)i;
}

// one lane per query (order != NULL: in cell order); see the head of the file for the stop rule
__global__ __launch_bounds__(kBlock) void k_closest_grid(const CGrid *gp, const double *rec, const int32_t *start, const int32_t *entries,
                                                         const double *q, int64_t nq, const int32_t *order, int has_max,
                                                         double max_dist, double *out_d2, int32_t *out_idx, double *out_c, int32_t *fall)
{
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= nq) return;
    const int64_t qi = order ? order[s] : s;
    const CGrid g = *gp;
    const double p[3] = {q[3 * qi], q[3 * qi + 1], q[3 * qi + 2]};
    int32_t c[3];
    for (int a = 0; a < 3; a++) c[a] = cell_coord(p[a], g.lo[a], g.cell, g.dim[a]);
    Best best;
    best.d2 = INFINITY; best.idx = -1; best.c[0] = best.c[1] = best.c[2] = 0.0;
    for (int r = 0; r <= kMaxShells; r++) {
        for (int dz = -r; dz <= r; dz++) {
            const int z = c[2] + dz;
            if (z < 0 || z >= g.dim[2]) continue;
            for (int dy = -r; dy <= r; dy++) {
                const int y = c[1] + dy;
                if (y < 0 || y >= g.dim[1]) continue;
                const bool full = (dz == -r || dz == r || dy == -r || dy == r);
                for (int dx = -r; dx <= r; dx += (full || r == 0) ? 1 : 2 * r) {
                    const int x = c[0] + dx;
                    if (x < 0 || x >= g.dim[0]) continue;
                    const int64_t id = cell_id(g, x, y, z);
                    const int32_t b = start[id], e = start[id + 1];
                    for (int32_t j = b; j < e; j++) consider(rec, g.is_tri, entries[j], p, best);
                }
            }
        }
        double face = INFINITY;
        for (int a = 0; a < 3; a++) {
            if (c[a] - r > 0) face = fmin(face, p[a] - (g.lo[a] + (double)(c[a] - r) * g.cell));
            if (c[a] + r < g.dim[a] - 1) face = fmin(face, (g.lo[a] + (double)(c[a] + r + 1) * g.cell) - p[a]);
        }
        if (face == INFINITY) break;                                 // the block covers the whole grid: every primitive was seen
        face -= g.margin;
        if (face > 0.0 && best.idx >= 0 && best.d2 <= face * face) break;
        if (has_max && face > max_dist) break;                       // nothing unseen is within max_dist
        if (r == kMaxShells) {
            fall[1 + atomicAdd(&fall[0], 1)] = (int32_t)qi;
            return;
        }
    }
    write_result(best, has_max, max_dist, qi, out_d2, out_idx, out_c);
}

// one block per open query (grid-stride over the open list): every lane keeps the best of a strided share of all primitives,
// then a fixed tree over the block picks the lexicographic minimum of (d2, index)
__global__ __launch_bounds__(kBlock) void k_closest_brute(const CGrid *gp, const double *rec, const double *q, const int32_t *fall,
                                                          int has_max, double max_dist, double *out_d2, int32_t *out_idx, double *out_c)
{
    __shared__ double sd[kBlock];
    __shared__ int32_t si[kBlock];
    __shared__ double sc[kBlock][3];
    const CGrid g = *gp;
    const int nf = fall[0];
    for (int f = blockIdx.x; f < nf; f += gridDim.x) {
        const int64_t qi = fall[1 + f];
        const double p[3] = {q[3 * qi], q[3 * qi + 1], q[3 * qi + 2]};
        Best best;
        best.d2 = INFINITY; best.idx = -1; best.c[0] = best.c[1] = best.c[2] = 0.0;
        for (int64_t j = threadIdx.x; j < g.n_prims; j += kBlock) consider(rec, g.is_tri, (int32_t)j, p, best);
        sd[threadIdx.x] = best.d2; si[threadIdx.x] = best.idx;
        for (int a = 0; a < 3; a++) sc[threadIdx.x][a] = best.c[a];
        __syncthreads();
        for (int w = kBlock / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                const int o = threadIdx.x + w;
                if (si[o] >= 0 && (si[threadIdx.x] < 0 || sd[o] < sd[threadIdx.x] || (sd[o] == sd[threadIdx.x] && si[o] < si[threadIdx.x]))) {
                    sd[threadIdx.x] = sd[o]; si[threadIdx.x] = si[o];
                    for (int a = 0; a < 3; a++) sc[threadIdx.x][a] = sc[o][a];
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            best.d2 = sd[0]; best.idx = si[0];
            for (int a = 0; a < 3; a++) best.c[a] = sc[0][a];
            write_result(best, has_max, max_dist, qi, out_d2, out_idx, out_c);
        }
        __syncthreads();
    }
}

// signed distance of a matched query: sqrt(d2) with the sign of (p - closest) . n, n = (b - a) x (c - a) of the chosen triangle
// (0 where that product is 0, for point primitives and for unmatched queries)
__global__ __launch_bounds__(kBlock) void k_closest_signed(const CGrid *gp, const double *rec, const double *q, int64_t nq,
                                                           const double *d2, const int32_t *idx, const double *closest, double *out)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= nq) return;
    const int32_t k = idx[i];
    double r = 0.0;
    if (k >= 0 && gp->is_tri && (int64_t)k < gp->n_prims) {
        const double *a = rec + 9 * (int64_t)k, *b = a + 3, *c = a + 6;
        const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const double ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const double n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
        const double d[3] = {q[3 * i] - closest[3 * i], q[3 * i + 1] - closest[3 * i + 1], q[3 * i + 2] - closest[3 * i + 2]};
        const double s = dot3(d, n);
        const double dist = sqrt(d2[i]);
        r = s > 0.0 ? dist : s < 0.0 ? -dist : 0.0;
    }
    out[i] = r;
}

// ---- ray cast ---------------------------------------------------------------------------------------------------------------
// The hit rule of include/topo4d_raster.h (t4d_closest_raycast), which tests/scanray_ref.py applies to every (ray, triangle)
// pair: a hit's computed point lies in the triangle's box grown by the margin, hence in cells that list the triangle, and that
// is what lets a walk over the cells along the ray equal the all-pairs search bit for bit.
struct Hit {
    double t, u, v;
    int32_t prim;
};

__device__ __forceinline__ void ray_consider(const double *rec, int32_t prim, const double *o, const double *d, double t_lo, double t_hi,
                                             int same_side, double margin, Hit &best)
{
#pragma clang fp contract(off)
    const double *a = rec + 9 * (int64_t)prim, *b = a + 3, *c = a + 6;
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
    const double det = dot3(e1, pv);
    if (det == 0.0 || (same_side && det >= 0.0)) return;
    const double tv[3] = {o[0] - a[0], o[1] - a[1], o[2] - a[2]};
    const double u = dot3(tv, pv) / det;
    if (!(u >= 0.0 && u <= 1.0)) return;
    const double qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    const double v = dot3(d, qv) / det;
    if (!(v >= 0.0 && u + v <= 1.0)) return;
    const double t = dot3(e2, qv) / det;
    if (!(t >= t_lo && t <= t_hi)) return;
    for (int k = 0; k < 3; k++) {                                   // the box condition
        const double p = o[k] + t * d[k];
        const double mn = fmin(a[k], fmin(b[k], c[k])), mx = fmax(a[k], fmax(b[k], c[k]));
        if (!(p >= mn - margin && p <= mx + margin)) return;
    }
    const double at = fabs(t), bt = fabs(best.t);
    const bool fwd = t >= 0.0, best_fwd = best.t >= 0.0;
    if (best.prim < 0 || at < bt || (at == bt && ((fwd && !best_fwd) || (fwd == best_fwd && prim < best.prim)))) {
        best.t = t; best.u = u; best.v = v; best.prim = prim;
    }
}

// one lane per ray (order != NULL: grouped by the cell of the origin).  [t_lo, t_hi] is cut into pieces of at most one cell
// along the ray's longest axis (1024 at the most); o + t d is monotone in t under rounding, so a piece's computed points lie in
// the box of its two ends, and the cells of that box grown by twice the margin (once for the box condition, once for the
// rounding of the sums that undo it) list every triangle the piece can hit.  The pieces are walked outward from the one next to
// t = 0 until every piece left begins beyond the best |t|; a piece outside the grid is passed over.
__global__ __launch_bounds__(kBlock) void k_closest_raycast(const CGrid *gp, const double *rec, const int32_t *start, const int32_t *entries,
                                                            const double *org, const double *dir, int64_t n_rays, const int32_t *order,
                                                            double t_lo, double t_hi, int same_side, double *out_t, int32_t *out_prim,
                                                            double *out_uv)
{
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_rays) return;
    const int64_t ri = order ? order[s] : s;
    const CGrid g = *gp;
    const double o[3] = {org[3 * ri], org[3 * ri + 1], org[3 * ri + 2]};
    const double d[3] = {dir[3 * ri], dir[3 * ri + 1], dir[3 * ri + 2]};
    Hit best;
    best.t = best.u = best.v = 0.0; best.prim = -1;
    bool ok = t_lo <= t_hi && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0);
    for (int a = 0; a < 3; a++) ok = ok && isfinite(o[a]) && isfinite(d[a]);
    if (ok) {
        const double span = t_hi - t_lo;
        const double want = ceil(span * fmax(fabs(d[0]), fmax(fabs(d[1]), fabs(d[2]))) / g.cell);
        const int np = !(want >= 1.0) ? 1 : want >= 1024.0 ? 1024 : (int)want;
        const double h = span / (double)np;
        auto cut = [&](int i) { return i >= np ? t_hi : t_lo + (double)i * h; };
        auto nearest = [&](int k) {                                 // min |t| over piece k
            const double lo = cut(k), hi = cut(k + 1);
            return lo > 0.0 ? lo : hi < 0.0 ? -hi : 0.0;
        };
        int k = 0;
        if (t_hi <= 0.0) k = np - 1;
        else if (t_lo < 0.0) {
            const double f = floor(-t_lo / h);
            k = !(f > 0.0) ? 0 : f >= (double)np ? np - 1 : (int)f;
        }
        int down = k - 1, up = k + 1;
        for (;;) {
            const double lo = cut(k), hi = cut(k + 1);
            int32_t c0[3], c1[3];
            bool inside = true;
            for (int a = 0; a < 3; a++) {
                const double pa = o[a] + lo * d[a], pb = o[a] + hi * d[a];
                const double mn = fmin(pa, pb) - 2.0 * g.margin, mx = fmax(pa, pb) + 2.0 * g.margin;
                inside = inside && !(mx < g.lo[a]) && !(mn > g.lo[a] + (double)g.dim[a] * g.cell);
                c0[a] = cell_coord(mn, g.lo[a], g.cell, g.dim[a]);
                c1[a] = cell_coord(mx, g.lo[a], g.cell, g.dim[a]);
            }
            if (inside)
                for (int32_t z = c0[2]; z <= c1[2]; z++)
                    for (int32_t y = c0[1]; y <= c1[1]; y++)
                        for (int32_t x = c0[0]; x <= c1[0]; x++) {
                            const int64_t id = cell_id(g, x, y, z);
                            const int32_t b = start[id], e = start[id + 1];
                            for (int32_t j = b; j < e; j++) ray_consider(rec, entries[j], o, d, t_lo, t_hi, same_side, g.margin, best);
                        }
            const double nd = down >= 0 ? nearest(down) : INFINITY, nu = up < np ? nearest(up) : INFINITY;
            if (down < 0 && up >= np) break;
            if (best.prim >= 0 && fmin(nd, nu) > fabs(best.t)) break;
            if (nd <= nu) k = down--;
            else k = up++;
        }
    }
    out_t[ri] = best.t;
    out_prim[ri] = best.prim;
    out_uv[2 * ri] = best.u;
    out_uv[2 * ri + 1] = best.v;
}

bool build_args_ok(int64_t n_vert, int64_t n_faces, const double *bbox, double mean_extent, int64_t entry_capacity)
{
    const int64_t n = n_faces > 0 ? n_faces : n_vert;
    return n_vert >= 1 && n_faces >= 0 && n <= INT32_MAX / 16 && n_vert <= INT32_MAX / 16 && bbox_ok(bbox) && mean_extent >= 0.0 &&
           isfinite(mean_extent) && entry_capacity >= 1 && entry_capacity <= INT32_MAX;
}

}  // namespace

// replaces trimesh.proximity.ProximityQuery's r-tree / open3d's RaycastingScene on the host: see include/topo4d_raster.h
T4D_EXPORT size_t t4d_closest_index_bytes(int64_t n_vert, int64_t n_faces, const double *bbox, double mean_extent, int64_t entry_capacity)
{
    if (!build_args_ok(n_vert, n_faces, bbox, mean_extent, entry_capacity)) {
        t4d_fail(T4D_ERR_ARG, "t4d_closest_index_bytes: need n_vert >= 1, n_faces >= 0, a finite ordered bbox, mean_extent >= 0 and 1 <= entry_capacity < 2^31");
        return 0;
    }
    const int is_tri = n_faces > 0;
    return closest_layout(closest_grid(bbox, is_tri ? n_faces : n_vert, mean_extent, is_tri), entry_capacity).total;
}

T4D_EXPORT int t4d_closest_build(const double *vertices, int64_t n_vert, const int32_t *faces, int64_t n_faces, const double *bbox,
                                 double mean_extent, void *index, size_t index_bytes, int64_t entry_capacity, int64_t *entries_needed,
                                 void *hip_stream)
{
    if (!vertices || !index || !entries_needed || (n_faces > 0 && !faces) || !build_args_ok(n_vert, n_faces, bbox, mean_extent, entry_capacity))
        return t4d_fail(T4D_ERR_ARG, "t4d_closest_build: bad arguments (NULL buffer, empty set, bad bbox or entry_capacity)");
    const int is_tri = n_faces > 0;
    const CGrid g = closest_grid(bbox, is_tri ? n_faces : n_vert, mean_extent, is_tri);
    const CLayout L = closest_layout(g, entry_capacity);
    if (index_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_closest_build: index buffer too small (%zu < %zu)", index_bytes, L.total);
    hipStream_t stream = (hipStream_t)hip_stream;
    char *b = (char *)index;
    CGrid *gd = (CGrid *)(b + L.head);
    double *rec = (double *)(b + L.rec);
    int32_t *start = (int32_t *)(b + L.start), *work = (int32_t *)(b + L.work), *bsum = (int32_t *)(b + L.bsum);
    int32_t *entries = (int32_t *)(b + L.entries);
    CGrid staged = g;
    staged.magic = 0;                                               // valid only once the lists are complete
    T4D_HIP_CHECK(hipMemcpyAsync(gd, &staged, sizeof(CGrid), hipMemcpyHostToDevice, stream));
    T4D_HIP_CHECK(hipStreamSynchronize(stream));                    // `staged` leaves scope
    T4D_HIP_CHECK(hipMemsetAsync(start, 0, sizeof(int32_t) * (size_t)(g.n_cells + 1), stream));
    hipLaunchKernelGGL(k_closest_records, dim3(blocks(g.n_prims, kBlock)), dim3(kBlock), 0, stream, vertices, faces, gd, rec);
    hipLaunchKernelGGL(k_closest_bin, dim3(blocks(g.n_prims, kBlock)), dim3(kBlock), 0, stream, gd, rec, start, entries, entry_capacity, 0);
    t4d_scan_i32(start, start, work, bsum, g.n_cells + 1, stream);
    int32_t total = 0;
    T4D_HIP_CHECK(hipMemcpyAsync(&total, start + g.n_cells, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    T4D_HIP_CHECK(hipStreamSynchronize(stream));
    *entries_needed = total;
    if (total < 0 || (int64_t)total > entry_capacity)
        return t4d_fail(T4D_ERR_PAIR_OVERFLOW, "t4d_closest_build: %d list entries, capacity %lld", total, (long long)entry_capacity);
    hipLaunchKernelGGL(k_closest_bin, dim3(blocks(g.n_prims, kBlock)), dim3(kBlock), 0, stream, gd, rec, work, entries, entry_capacity, 1);
    hipLaunchKernelGGL(k_closest_sort_cells, dim3(blocks(g.n_cells, kBlock)), dim3(kBlock), 0, stream, gd, start, entries);
    T4D_HIP_CHECK(hipMemcpyAsync(&gd->magic, &kMagic, sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    T4D_HIP_CHECK(hipStreamSynchronize(stream));
    return t4d_launch_status("t4d_closest_build");
}

T4D_EXPORT size_t t4d_closest_query_scratch_bytes(int64_t n_queries)
{
    if (n_queries < 1 || n_queries > INT32_MAX / 2) {
        t4d_fail(T4D_ERR_ARG, "t4d_closest_query_scratch_bytes: need 1 <= n_queries < 2^30");
        return 0;
    }
    return query_layout(n_queries).total;
}

namespace {
// the index's header back on the host (one small copy: the launch sizes and the layout follow from it)
int read_index(const char *entry, const void *index, size_t index_bytes, hipStream_t stream, CGrid *g, CLayout *L)
{
    T4D_HIP_CHECK(hipMemcpyAsync(g, index, sizeof(CGrid), hipMemcpyDeviceToHost, stream));
    T4D_HIP_CHECK(hipStreamSynchronize(stream));
    if (g->magic != kMagic || g->n_prims < 1 || g->n_cells < 1 || g->n_cells > kMaxCells)
        return t4d_fail(T4D_ERR_ARG, "%s: the index buffer holds no finished t4d_closest_build", entry);
    *L = closest_layout(*g, 1);
    if (index_bytes < L->total) return t4d_fail(T4D_ERR_STATE_SIZE, "%s: index buffer smaller than its own layout", entry);
    return T4D_OK;
}
}  // namespace

// t4d_align.hip reads the triangles of a finished index through this (hidden: declared in t4d_host.h, not part of the ABI)
int t4d_closest_index_records(const char *entry, const void *index, size_t index_bytes, void *hip_stream, const double **records,
                              int64_t *n_prims, int *is_tri)
{
    CGrid g;
    CLayout L;
    const int rc = read_index(entry, index, index_bytes, (hipStream_t)hip_stream, &g, &L);
    if (rc != T4D_OK) return rc;
    *records = (const double *)((const char *)index + L.rec);
    *n_prims = g.n_prims;
    *is_tri = g.is_tri;
    return T4D_OK;
}

T4D_EXPORT int t4d_closest_query(void *index, size_t index_bytes, const double *points, int64_t n_queries, double max_dist,
                                 int32_t flags, double *d2, int32_t *prim_index, double *closest, void *scratch, size_t scratch_bytes,
                                 void *hip_stream)
{
    if (!index || !points || !d2 || !prim_index || !closest || !scratch || n_queries < 1 || n_queries > INT32_MAX / 2 ||
        index_bytes < 256 || (flags & ~T4D_CLOSEST_INPUT_ORDER) || max_dist != max_dist)
        return t4d_fail(T4D_ERR_ARG, "t4d_closest_query: bad arguments (NULL buffer, no queries, unknown flag or NaN max_dist)");
    const QLayout Q = query_layout(n_queries);
    if (scratch_bytes < Q.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_closest_query: scratch too small (%zu < %zu)", scratch_bytes, Q.total);
    hipStream_t stream = (hipStream_t)hip_stream;
    CGrid g;
    CLayout L;
    const int rc = read_index("t4d_closest_query", index, index_bytes, stream, &g, &L);
    if (rc != T4D_OK) return rc;
    char *b = (char *)index, *s = (char *)scratch;
    const CGrid *gd = (const CGrid *)(b + L.head);
    const double *rec = (const double *)(b + L.rec);
    const int32_t *start = (const int32_t *)(b + L.start), *entries = (const int32_t *)(b + L.entries);
    int32_t *work = (int32_t *)(b + L.work), *bsum = (int32_t *)(b + L.bsum);
    int32_t *order = (int32_t *)(s + Q.order), *qcell = (int32_t *)(s + Q.qcell), *fall = (int32_t *)(s + Q.fall);
    const int has_max = max_dist >= 0.0 && max_dist < INFINITY;
    const bool sorted = !(flags & T4D_CLOSEST_INPUT_ORDER);
    if (sorted) {
        T4D_HIP_CHECK(hipMemsetAsync(work, 0, sizeof(int32_t) * (size_t)(g.n_cells + 1), stream));
        hipLaunchKernelGGL(k_closest_query_cells, dim3(blocks(n_queries, kBlock)), dim3(kBlock), 0, stream, gd, points, n_queries, qcell, work);
        t4d_scan_i32(work, work, nullptr, bsum, g.n_cells + 1, stream);
        hipLaunchKernelGGL(k_closest_query_order, dim3(blocks(n_queries, kBlock)), dim3(kBlock), 0, stream, qcell, n_queries, work, order);
    }
    T4D_HIP_CHECK(hipMemsetAsync(fall, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_closest_grid, dim3(blocks(n_queries, kBlock)), dim3(kBlock), 0, stream, gd, rec, start, entries, points, n_queries,
                       sorted ? order : (const int32_t *)nullptr, has_max, max_dist, d2, prim_index, closest, fall);
    hipLaunchKernelGGL(k_closest_brute, dim3(kBruteBlocks), dim3(kBlock), 0, stream, gd, rec, points, fall, has_max, max_dist, d2,
                       prim_index, closest);
    return t4d_launch_status("t4d_closest_query");
}

T4D_EXPORT int t4d_closest_signed(const void *index, size_t index_bytes, const double *points, int64_t n_queries, const double *d2,
                                  const int32_t *prim_index, const double *closest, double *signed_dist, void *hip_stream)
{
    if (!index || !points || !d2 || !prim_index || !closest || !signed_dist || n_queries < 1 || n_queries > INT32_MAX / 2 || index_bytes < 256)
        return t4d_fail(T4D_ERR_ARG, "t4d_closest_signed: bad arguments (NULL buffer or no queries)");
    hipStream_t stream = (hipStream_t)hip_stream;
    CGrid g;
    CLayout L;
    const int rc = read_index("t4d_closest_signed", index, index_bytes, stream, &g, &L);
    if (rc != T4D_OK) return rc;
    const char *b = (const char *)index;
    hipLaunchKernelGGL(k_closest_signed, dim3(blocks(n_queries, kBlock)), dim3(kBlock), 0, stream, (const CGrid *)(b + L.head),
                       (const double *)(b + L.rec), points, n_queries, d2, prim_index, closest, signed_dist);
    return t4d_launch_status("t4d_closest_signed");
}

T4D_EXPORT int t4d_closest_raycast(void *index, size_t index_bytes, const double *origins, const double *dirs, int64_t n_rays, double t_lo,
                                   double t_hi, int32_t flags, double *out_t, int32_t *out_prim, double *out_uv, void *scratch,
                                   size_t scratch_bytes, void *hip_stream)
{
    if (!index || !origins || !dirs || !out_t || !out_prim || !out_uv || !scratch || n_rays < 1 || n_rays > INT32_MAX / 2 ||
        index_bytes < 256 || (flags & ~(T4D_CLOSEST_INPUT_ORDER | T4D_RAY_SAME_SIDE)) || !isfinite(t_lo) || !isfinite(t_hi) ||
        !isfinite(t_hi - t_lo))
        return t4d_fail(T4D_ERR_ARG, "t4d_closest_raycast: bad arguments (NULL buffer, no rays, unknown flag, or limits that are not finite with a finite difference)");
    const QLayout Q = query_layout(n_rays);
    if (scratch_bytes < Q.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_closest_raycast: scratch too small (%zu < %zu)", scratch_bytes, Q.total);
    hipStream_t stream = (hipStream_t)hip_stream;
    CGrid g;
    CLayout L;
    const int rc = read_index("t4d_closest_raycast", index, index_bytes, stream, &g, &L);
    if (rc != T4D_OK) return rc;
    if (!g.is_tri) return t4d_fail(T4D_ERR_ARG, "t4d_closest_raycast: the index holds points, and a ray meets only triangles");
    char *b = (char *)index, *s = (char *)scratch;
    const CGrid *gd = (const CGrid *)(b + L.head);
    const double *rec = (const double *)(b + L.rec);
    const int32_t *start = (const int32_t *)(b + L.start), *entries = (const int32_t *)(b + L.entries);
    int32_t *work = (int32_t *)(b + L.work), *bsum = (int32_t *)(b + L.bsum);
    int32_t *order = (int32_t *)(s + Q.order), *qcell = (int32_t *)(s + Q.qcell);
    const bool sorted = !(flags & T4D_CLOSEST_INPUT_ORDER);
    if (sorted) {                                                   // the rays grouped by the cell of their origin
        T4D_HIP_CHECK(hipMemsetAsync(work, 0, sizeof(int32_t) * (size_t)(g.n_cells + 1), stream));
        hipLaunchKernelGGL(k_closest_query_cells, dim3(blocks(n_rays, kBlock)), dim3(kBlock), 0, stream, gd, origins, n_rays, qcell, work);
        t4d_scan_i32(work, work, nullptr, bsum, g.n_cells + 1, stream);
        hipLaunchKernelGGL(k_closest_query_order, dim3(blocks(n_rays, kBlock)), dim3(kBlock), 0, stream, qcell, n_rays, work, order);
    }
    hipLaunchKernelGGL(k_closest_raycast, dim3(blocks(n_rays, kBlock)), dim3(kBlock), 0, stream, gd, rec, start, entries, origins, dirs, n_rays,
                       sorted ? order : (const int32_t *)nullptr, t_lo, t_hi, (flags & T4D_RAY_SAME_SIDE) ? 1 : 0, out_t, out_prim, out_uv);
    return t4d_launch_status("t4d_closest_raycast");
}
