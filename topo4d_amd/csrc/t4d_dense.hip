// t4d_dense.hip — the UV-densified Gaussian mesh of the texture pass (train.py:213-269) and its exact kNN scales, on the device.
//
//  * k_dense_grid: one thread per (frontal quad, i, j), 0 <= i, j <= d+1, of helpers.bilinear_interpolate_2 (helpers.py:421-599).
//    The reference's sequential `edge_dict` is replaced by a host pre-pass (topo4d_amd/densify.py:plan_dense_mesh) that gives each
//    quad its four "borrowed edge" flags, the owner (quad, slot) of every borrowed edge and its prefix offset; every index then
//    follows in closed form (dense_index below).  A thread writes its point (position, weights, father, UV) if it generates one,
//    and sub-quad (i-1, j-1)'s two vertex and two UV triangles (triangulate_faces) if i, j >= 1.
//  * k_dense_copy: the coarse rows of dense_vertex / dense_uvs, and the triangles and non-frontal quads of train.py:236-240.
//  * kNN (o3d_knn + .mean(-1), helpers.py:147-157): a hashed uniform grid over the occupied cells only (count, scan, scatter
//    passes), then one thread per point searching cube shells of growing radius; queries still open after kMaxShells shells go
//    to a block-parallel brute-force pass.
//
// Every index the kernels read is checked against its array (a violation sets a status word in the scratch, and the read is
// skipped); results are bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kKnnMax = T4D_KNN_MAX_K + 1;      // candidates held per query: k nearest + the point itself
constexpr int kMaxShells = 4;                   // shells searched before a query goes to the brute-force pass
constexpr uint64_t kEmpty = ~0ull;

struct DenseStatus {
    int bad;                                    // 0: every index was in range; otherwise a bit per kind of violation
};

// ---------------------------------------------------------------------------------------------------------------------------
// dense mesh
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int slot_start(int s) { return s == 0 ? 0 : s == 1 ? 0 : s == 2 ? 1 : 3; }
__device__ __forceinline__ int slot_end(int s) { return s == 0 ? 3 : s == 1 ? 1 : 2; }

// row-major rank of generated position (i, j) among the quad's generated positions
__device__ __forceinline__ int local_index(int flags, int i, int j, int d)
{
    const int b0 = flags & 1, b1 = (flags >> 1) & 1, b3 = (flags >> 3) & 1;
    const int r0 = b0 ? 0 : d;
    const int m = d + (1 - b1) + (1 - b3);
    if (i == 0) return j - 1;
    if (i == d + 1) return r0 + d * m + j - 1;
    return r0 + (i - 1) * m + (j == 0 ? 0 : (1 - b1) + min(j - 1, d));
}

// slot of a non-corner border position, -1 inside; the i == 0 / j == 0 / i == d+1 / j == d+1 order of the reference
__device__ __forceinline__ int border_slot(int i, int j, int d)
{
    return i == 0 ? 0 : j == 0 ? 1 : i == d + 1 ? 2 : j == d + 1 ? 3 : -1;
}

// Vertex index (uv = 0) or UV index (uv = 1) of grid position (i, j) of quad q: pts_idx / pts_idx_uv of the reference.
// *gen = 1 when the quad generates the point there itself.
__device__ int dense_index(const T4DDenseMesh &m, int q, int i, int j, int uv, int *gen, DenseStatus *st)
{
    const int d = m.density;
    const int32_t *f = m.quads + 4 * (int64_t)q;
    const int32_t *fu = m.uv_quads + 4 * (int64_t)q;
    const int base = uv ? m.n_uv : m.n_vert;
    *gen = 0;
    if ((i == 0 || i == d + 1) && (j == 0 || j == d + 1)) {
        const int k = i == 0 ? (j == 0 ? 0 : 3) : (j == 0 ? 1 : 2);
        return uv ? fu[k] : f[k];
    }
    const int flags = m.plan[2 * (int64_t)q];
    const int s = border_slot(i, j, d);
    if (s >= 0 && ((flags >> s) & 1)) {
        const int p = (s == 0 || s == 2) ? j : i;                                 // 1..d along the slot from its start corner
        const int k = f[slot_start(s)] > f[slot_end(s)] ? d - p : p - 1;          // rank from the smaller vertex index
        const int so = m.src[4 * (int64_t)q + s];
        const int oq = so >> 2, os = so & 3;
        if (so < 0 || oq >= m.n_quads) {
            atomicOr(&st->bad, 1);
            return 0;
        }
        const int32_t *of = m.quads + 4 * (int64_t)oq;
        const int op = of[slot_start(os)] > of[slot_end(os)] ? d - k : k + 1;
        const int oi = os == 0 ? 0 : os == 2 ? d + 1 : op;
        const int oj = os == 1 ? 0 : os == 3 ? d + 1 : op;
        return base + m.plan[2 * (int64_t)oq + 1] + local_index(m.plan[2 * (int64_t)oq], oi, oj, d);
    }
    *gen = 1;
    return base + m.plan[2 * (int64_t)q + 1] + local_index(flags, i, j, d);
}

__global__ __launch_bounds__(kBlock) void k_dense_grid(const T4DDenseMesh m, DenseStatus *st)
{
#pragma clang fp contract(off)      // numpy rounds every product and every partial sum
    const int d = m.density, g = d + 2;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)m.n_quads * g * g) return;
    const int q = (int)(t / (g * g));
    const int rem = (int)(t - (int64_t)q * g * g);
    const int i = rem / g, j = rem - (rem / g) * g;
    const int32_t *f = m.quads + 4 * (int64_t)q;
    const int32_t *fu = m.uv_quads + 4 * (int64_t)q;
    for (int k = 0; k < 4; k++)
        if (f[k] < 0 || f[k] >= m.n_vert || fu[k] < 0 || fu[k] >= m.n_uv) {
            atomicOr(&st->bad, 2);
            return;
        }
    int gen;
    const int v = dense_index(m, q, i, j, 0, &gen, st);
    if (gen) {
        const int64_t r = (int64_t)v - m.n_vert;
        if (r < 0 || r >= m.n_points) {
            atomicOr(&st->bad, 4);
            return;
        }
        const double tt = (double)i / (double)(d + 1), u = (double)j / (double)(d + 1);
        const double w[4] = {(1 - tt) * (1 - u), tt * (1 - u), tt * u, (1 - tt) * u};
        for (int c = 0; c < 3; c++) {
            // float32 vertices times Python floats: each weight rounded to float, products added left to right in float
            float s = (float)w[0] * m.vertices[3 * (int64_t)f[0] + c];
            s = s + (float)w[1] * m.vertices[3 * (int64_t)f[1] + c];
            s = s + (float)w[2] * m.vertices[3 * (int64_t)f[2] + c];
            s = s + (float)w[3] * m.vertices[3 * (int64_t)f[3] + c];
            m.dense_vertex[3 * (int64_t)v + c] = (double)s;
        }
        for (int k = 0; k < 4; k++) m.vertex_weight[4 * r + k] = w[k];
        m.vertex_father[r] = q;
        for (int c = 0; c < 2; c++) {                                          // np.sum(uvs * weight, axis=1): left to right
            double a = m.uvs[2 * (int64_t)fu[0] + c] * w[0];
            a = a + m.uvs[2 * (int64_t)fu[1] + c] * w[1];
            a = a + m.uvs[2 * (int64_t)fu[2] + c] * w[2];
            a = a + m.uvs[2 * (int64_t)fu[3] + c] * w[3];
            m.dense_uvs[2 * ((int64_t)m.n_uv + r) + c] = a;
        }
    }
    if (i >= 1 && j >= 1) {
        int idx[4], uvi[4], dummy;
        const int pi[4] = {i - 1, i, i, i - 1}, pj[4] = {j - 1, j - 1, j, j};   // new_faces[cnt_f, 0..3]
        for (int k = 0; k < 4; k++) {
            idx[k] = dense_index(m, q, pi[k], pj[k], 0, &dummy, st);
            uvi[k] = dense_index(m, q, pi[k], pj[k], 1, &dummy, st);
        }
        const int64_t row = (int64_t)m.n_tri + 2 * ((int64_t)q * (d + 1) * (d + 1) + (int64_t)(i - 1) * (d + 1) + (j - 1));
        const int tri[2][3] = {{0, 1, 2}, {0, 2, 3}};                           // triangulate_faces
        for (int h = 0; h < 2; h++)
            for (int c = 0; c < 3; c++) {
                m.faces[3 * (row + h) + c] = idx[tri[h][c]];
                m.uv_faces[3 * (row + h) + c] = uvi[tri[h][c]];
            }
    }
}

// the rows that are copies: coarse dense_vertex / dense_uvs rows, triangles, non-frontal quads (triangulated)
__global__ __launch_bounds__(kBlock) void k_dense_copy(const T4DDenseMesh m, DenseStatus *st)
{
    int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t < m.n_vert) {
        for (int c = 0; c < 3; c++) m.dense_vertex[3 * t + c] = (double)m.vertices[3 * t + c];
        return;
    }
    t -= m.n_vert;
    if (t < m.n_uv) {
        for (int c = 0; c < 2; c++) m.dense_uvs[2 * t + c] = m.uvs[2 * t + c];
        return;
    }
    t -= m.n_uv;
    if (t < m.n_tri) {
        for (int c = 0; c < 3; c++) {
            const int a = m.tri[3 * t + c], b = m.uv_tri[3 * t + c];
            if (a < 0 || a >= m.n_vert || b < 0 || b >= m.n_uv) atomicOr(&st->bad, 8);
            m.faces[3 * t + c] = a;
            m.uv_faces[3 * t + c] = b;
        }
        return;
    }
    t -= m.n_tri;
    if (t < m.n_rest) {
        const int64_t row = (int64_t)m.n_tri + 2 * ((int64_t)m.n_quads * (m.density + 1) * (m.density + 1) + t);
        const int tri[2][3] = {{0, 1, 2}, {0, 2, 3}};
        for (int h = 0; h < 2; h++)
            for (int c = 0; c < 3; c++) {
                const int a = m.rest[4 * t + tri[h][c]], b = m.uv_rest[4 * t + tri[h][c]];
                if (a < 0 || a >= m.n_vert || b < 0 || b >= m.n_uv) atomicOr(&st->bad, 8);
                m.faces[3 * (row + h) + c] = a;
                m.uv_faces[3 * (row + h) + c] = b;
            }
    }
}

__global__ void k_zero_status(DenseStatus *st) { st->bad = 0; }

bool dense_valid(const T4DDenseMesh *m)
{
    if (!m || m->n_vert < 0 || m->n_uv < 0 || m->n_quads < 0 || m->n_tri < 0 || m->n_rest < 0 || m->density < 1 ||
        m->density > 1024 || m->n_points < 0)
        return false;
    const int64_t g = (int64_t)m->density + 2;
    const int64_t d1 = (int64_t)m->density + 1;
    // n_points lies between "every edge borrowed" and "none borrowed"; the face count is what train.py:236-240 builds
    if (m->n_points > (int64_t)m->n_quads * (g * g - 4) || m->n_points < (int64_t)m->n_quads * (g * g - 4 - 4 * m->density)) return false;
    if (m->n_faces != (int64_t)m->n_tri + 2 * ((int64_t)m->n_quads * d1 * d1 + m->n_rest)) return false;
    if ((int64_t)m->n_vert + m->n_points > INT32_MAX || (int64_t)m->n_uv + m->n_points > INT32_MAX) return false;
    if ((int64_t)m->n_quads * g * g > ((int64_t)1 << 40)) return false;
    if ((m->n_vert > 0 && !m->vertices) || (m->n_uv > 0 && !m->uvs) || !m->dense_vertex || !m->dense_uvs) return false;
    if (m->n_quads > 0 && (!m->quads || !m->uv_quads || !m->plan || !m->src)) return false;
    if (m->n_points > 0 && (!m->vertex_father || !m->vertex_weight)) return false;
    if (m->n_tri > 0 && (!m->tri || !m->uv_tri)) return false;
    if (m->n_rest > 0 && (!m->rest || !m->uv_rest)) return false;
    if (m->n_faces > 0 && (!m->faces || !m->uv_faces)) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// kNN
// ---------------------------------------------------------------------------------------------------------------------------
struct Grid {
    double lo[3];
    double cell;
    int64_t dim[3];
};

struct KnnLayout {
    size_t bbox, keys, cnt, start, cursor, slot, spts, sidx, bsum, fall, total;
    int64_t table;
};

KnnLayout knn_layout(int64_t n)
{
    KnnLayout L;
    int64_t t = 1;
    while (t < 2 * n) t <<= 1;                                      // at most n occupied cells: load factor <= 1/2
    L.table = t;
    size_t o = 0;
    L.bbox = o;   o += align_up(sizeof(double) * 6 * 1024);         // per-block min / max partials, then the grid
    L.keys = o;   o += align_up(sizeof(uint64_t) * t);
    L.cnt = o;    o += align_up(sizeof(int32_t) * t);
    L.start = o;  o += align_up(sizeof(int32_t) * t);
    L.cursor = o; o += align_up(sizeof(int32_t) * t);
    L.slot = o;   o += align_up(sizeof(int32_t) * n);
    L.spts = o;   o += align_up(sizeof(double) * 3 * n);
    L.sidx = o;   o += align_up(sizeof(int32_t) * n);
    L.bsum = o;   o += align_up(sizeof(int32_t) * t4d_scan_i32_sum_words(t));
    L.fall = o;   o += align_up(sizeof(int32_t) * (n + 1));         // [0]: count, then the open queries
    L.total = o + 256;                                              // + the Grid record
    return L;
}

constexpr int kBboxBlocks = 1024;

// per-block min / max of the coordinates (order-independent: the result does not depend on the schedule)
__global__ __launch_bounds__(kBlock) void k_bbox_partial(const double *p, int64_t n, double *part)
{
    __shared__ double s[6][kBlock];
    double v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        for (int c = 0; c < 3; c++) {
            v[c] = fmin(v[c], p[3 * i + c]);
            v[3 + c] = fmax(v[3 + c], p[3 * i + c]);
        }
    for (int c = 0; c < 6; c++) s[c][threadIdx.x] = v[c];
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int c = 0; c < 6; c++)
                s[c][threadIdx.x] = c < 3 ? fmin(s[c][threadIdx.x], s[c][threadIdx.x + w]) : fmax(s[c][threadIdx.x], s[c][threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int c = 0; c < 6; c++) part[6 * blockIdx.x + c] = s[c][0];
}

// The cell size assumes the points lie on a surface (the dense Gaussians sit on the face mesh): with A the area of the bounding
// box's surface, n points are about sqrt(A / n) apart, and a cell edge of 2 sqrt(A / n) holds about four of them where the surface
// crosses it flat - about what a k = 4 query needs from its own cell and the first shell.  The cell is kept >= 2^-20 of the
// largest extent (at most 2^20 + 1 cells per axis, so a cell key fits 63 bits) and > 0.
__global__ void k_grid(const double *part, int nparts, int64_t n, Grid *g)
{
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = 0; b < nparts; b++)
        for (int c = 0; c < 3; c++) {
            lo[c] = fmin(lo[c], part[6 * b + c]);
            hi[c] = fmax(hi[c], part[6 * b + 3 + c]);
        }
    const double e0 = hi[0] - lo[0], e1 = hi[1] - lo[1], e2 = hi[2] - lo[2];
    const double emax = fmax(e0, fmax(e1, e2));
    const double area = 2.0 * (e0 * e1 + e1 * e2 + e0 * e2);
    double cell = 2.0 * sqrt(area / (double)n);
    cell = fmax(cell, emax * 0x1p-20);
    if (!(cell > 0.0)) cell = 1.0;
    for (int c = 0; c < 3; c++) {
        g->lo[c] = lo[c];
        g->dim[c] = (int64_t)floor((hi[c] - lo[c]) / cell) + 1;
    }
    g->cell = cell;
}

__device__ __forceinline__ int64_t cell_coord(double x, double lo, double cell, int64_t dim)
{
    int64_t c = (int64_t)floor((x - lo) / cell);
    return c < 0 ? 0 : c >= dim ? dim - 1 : c;
}

__device__ __forceinline__ uint64_t cell_key(const Grid &g, int64_t cx, int64_t cy, int64_t cz)
{
    return (uint64_t)(cx + g.dim[0] * (cy + g.dim[1] * cz));
}

__device__ __forceinline__ uint64_t hash64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

__global__ __launch_bounds__(kBlock) void k_fill(uint64_t *keys, int32_t *cnt, int64_t t)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < t) { keys[i] = kEmpty; cnt[i] = 0; }
}

__global__ __launch_bounds__(kBlock) void k_insert(const double *p, int64_t n, const Grid *gp, uint64_t *keys, int32_t *cnt,
                                                   int32_t *slot, int64_t mask)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const Grid g = *gp;
    const uint64_t key = cell_key(g, cell_coord(p[3 * i], g.lo[0], g.cell, g.dim[0]), cell_coord(p[3 * i + 1], g.lo[1], g.cell, g.dim[1]),
                                  cell_coord(p[3 * i + 2], g.lo[2], g.cell, g.dim[2]));
    int64_t h = (int64_t)(hash64(key) & (uint64_t)mask);
    for (;;) {                                                      // the table has >= 2n slots: a free one exists
        const uint64_t prev = atomicCAS((unsigned long long *)&keys[h], (unsigned long long)kEmpty, (unsigned long long)key);
        if (prev == kEmpty || prev == key) break;
        h = (h + 1) & mask;
    }
    atomicAdd(&cnt[h], 1);
    slot[i] = (int32_t)h;
}

// points grouped by cell (the order inside a cell depends on the schedule; the query result does not)
__global__ __launch_bounds__(kBlock) void k_scatter(const double *p, int64_t n, const int32_t *slot, int32_t *cursor, double *spts,
                                                    int32_t *sidx)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t pos = atomicAdd(&cursor[slot[i]], 1);
    for (int c = 0; c < 3; c++) spts[3 * (int64_t)pos + c] = p[3 * i + c];
    sidx[pos] = (int32_t)i;
}

// ascending list of the K smallest squared distances seen
struct TopK {
    double d[kKnnMax];
    int n;
    __device__ void init() { n = 0; }
    __device__ __forceinline__ void push(double v, int K)
    {
        if (n == K && !(v < d[K - 1])) return;
        int m = n < K ? n++ : K - 1;
        while (m > 0 && d[m - 1] > v) {
            d[m] = d[m - 1];
            m--;
        }
        d[m] = v;
    }
};

__device__ __forceinline__ double sq_dist(const double *a, const double *b)
{
#pragma clang fp contract(off)      // nanoflann's L2 adaptor for dim 3: ((dx*dx + dy*dy) + dz*dz)
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double finish(const TopK &t, int k)
{
#pragma clang fp contract(off)
    double s = 0.0;                                                 // the point's own zero included: ascending order
    for (int m = 0; m <= k; m++) s = s + t.d[m];
    return s / (double)k;
}

__device__ void scan_cell(const Grid &g, const uint64_t *keys, const int32_t *start, const int32_t *cnt, int64_t mask,
                          const double *spts, int64_t cx, int64_t cy, int64_t cz, const double *q, TopK &best, int K)
{
    const uint64_t key = cell_key(g, cx, cy, cz);
    int64_t h = (int64_t)(hash64(key) & (uint64_t)mask);
    for (;;) {
        const uint64_t k = keys[h];
        if (k == kEmpty) return;
        if (k == key) break;
        h = (h + 1) & mask;
    }
    const int32_t b = start[h], e = b + cnt[h];
    for (int32_t j = b; j < e; j++) best.push(sq_dist(q, spts + 3 * (int64_t)j), K);
}

// one thread per point, in cell order (neighbouring threads share cells): shells of growing Chebyshev radius r around the point's
// cell; stop once K candidates are held and the worst is no farther than the nearest face of the searched cube that does not lie
// on the grid's border (a small margin covers the rounding of the cell coordinates); after kMaxShells shells hand over.
__global__ __launch_bounds__(kBlock) void k_knn_grid(const Grid *gp, const uint64_t *keys, const int32_t *start, const int32_t *cnt,
                                                     int64_t mask, const double *spts, const int32_t *sidx, int64_t n, int k,
                                                     double *out, int32_t *fall)
{
#pragma clang fp contract(off)
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n) return;
    const Grid g = *gp;
    const int K = k + 1;
    const double q[3] = {spts[3 * s], spts[3 * s + 1], spts[3 * s + 2]};
    int64_t c[3];
    for (int a = 0; a < 3; a++) c[a] = cell_coord(q[a], g.lo[a], g.cell, g.dim[a]);
    const double margin = 1e-9 * (g.cell + (double)max(g.dim[0], max(g.dim[1], g.dim[2])) * g.cell);
    TopK best;
    best.init();
    for (int r = 0; r <= kMaxShells; r++) {
        for (int64_t dz = -r; dz <= r; dz++) {
            const int64_t z = c[2] + dz;
            if (z < 0 || z >= g.dim[2]) continue;
            for (int64_t dy = -r; dy <= r; dy++) {
                const int64_t y = c[1] + dy;
                if (y < 0 || y >= g.dim[1]) continue;
                const bool full = (dz == -r || dz == r || dy == -r || dy == r);
                for (int64_t dx = -r; dx <= r; dx += (full || r == 0) ? 1 : 2 * r) {
                    const int64_t x = c[0] + dx;
                    if (x < 0 || x >= g.dim[0]) continue;
                    scan_cell(g, keys, start, cnt, mask, spts, x, y, z, q, best, K);
                }
            }
        }
        double face = INFINITY;
        for (int a = 0; a < 3; a++) {
            if (c[a] - r > 0) face = fmin(face, q[a] - (g.lo[a] + (double)(c[a] - r) * g.cell));
            if (c[a] + r < g.dim[a] - 1) face = fmin(face, (g.lo[a] + (double)(c[a] + r + 1) * g.cell) - q[a]);
        }
        if (face == INFINITY) break;                                 // the cube covers the whole grid: every point was seen
        face -= margin;
        if (best.n == K && face > 0.0 && best.d[K - 1] <= face * face) break;
        if (r == kMaxShells) {                                        // still open: the brute-force pass answers it
            fall[1 + atomicAdd(&fall[0], 1)] = (int32_t)s;
            return;
        }
    }
    out[sidx[s]] = finish(best, k);
}

// one block per open query (grid-stride over the open list): every thread keeps the K smallest of a strided share of all points,
// thread 0 merges the per-thread lists
__global__ __launch_bounds__(kBlock) void k_knn_brute(const double *spts, const int32_t *sidx, int64_t n, int k, const int32_t *fall,
                                                      double *out)
{
    __shared__ double s[kBlock * kKnnMax];
    __shared__ int sn[kBlock];
    const int K = k + 1;
    const int nf = fall[0];
    for (int f = blockIdx.x; f < nf; f += gridDim.x) {
        const int64_t qs = fall[1 + f];
        const double q[3] = {spts[3 * qs], spts[3 * qs + 1], spts[3 * qs + 2]};
        TopK best;
        best.init();
        for (int64_t j = threadIdx.x; j < n; j += kBlock) best.push(sq_dist(q, spts + 3 * j), K);
        for (int m = 0; m < best.n; m++) s[threadIdx.x * kKnnMax + m] = best.d[m];
        sn[threadIdx.x] = best.n;
        __syncthreads();
        if (threadIdx.x == 0) {
            TopK all;
            all.init();
            for (int t = 0; t < kBlock; t++)
                for (int m = 0; m < sn[t]; m++) all.push(s[t * kKnnMax + m], K);
            out[sidx[qs]] = finish(all, k);
        }
        __syncthreads();
    }
}

// dense_log_scales (train.py:245-246, :262): np.tile(np.log(np.sqrt(mean.clip(min=1e-7))), 3) in float64, then .float()
__global__ __launch_bounds__(kBlock) void k_log_scales(const double *mean, int64_t n, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float v = (float)log(sqrt(fmax(mean[i], 0.0000001)));
    out[3 * i] = v; out[3 * i + 1] = v; out[3 * i + 2] = v;
}

unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

}  // namespace

// train.py:214-243 (helpers.build_dense_vertices_2 / bilinear_interpolate_2, helpers.py:421-654, and the face lists of train.py:233-240
// with triangulate_faces, helpers.py:657-667): see include/topo4d_raster.h
T4D_EXPORT size_t t4d_dense_scratch_bytes(const T4DDenseMesh *m)
{
    if (!dense_valid(m)) {
        t4d_fail(T4D_ERR_ARG, "t4d_dense_scratch_bytes: bad mesh descriptor");
        return 0;
    }
    return 256;
}

T4D_EXPORT int t4d_dense_build(const T4DDenseMesh *m, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!dense_valid(m) || !scratch) return t4d_fail(T4D_ERR_ARG, "t4d_dense_build: bad arguments");
    if (scratch_bytes < 256) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_dense_build: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    DenseStatus *st = (DenseStatus *)scratch;
    hipLaunchKernelGGL(k_zero_status, dim3(1), dim3(1), 0, stream, st);
    const int64_t g = (int64_t)m->density + 2;
    const int64_t cells = (int64_t)m->n_quads * g * g;
    if (cells > 0) hipLaunchKernelGGL(k_dense_grid, dim3(blocks(cells, kBlock)), dim3(kBlock), 0, stream, *m, st);
    const int64_t copies = (int64_t)m->n_vert + m->n_uv + m->n_tri + m->n_rest;
    if (copies > 0) hipLaunchKernelGGL(k_dense_copy, dim3(blocks(copies, kBlock)), dim3(kBlock), 0, stream, *m, st);
    return t4d_launch_status("t4d_dense_build");
}

// helpers.py:147-157 (o3d_knn) followed by `.mean(-1)` (train.py:131-132, :245-246): see include/topo4d_raster.h
T4D_EXPORT size_t t4d_knn_scratch_bytes(int64_t n, int32_t k)
{
    if (k < 1 || k > T4D_KNN_MAX_K || n < (int64_t)k + 1 || n > INT32_MAX / 2) {
        t4d_fail(T4D_ERR_ARG, "t4d_knn_scratch_bytes: need 1 <= k <= T4D_KNN_MAX_K and k < n < 2^30");
        return 0;
    }
    return knn_layout(n).total;
}

T4D_EXPORT int t4d_knn_mean_sq_dist(const double *points, int64_t n, int32_t k, double *mean, float *log_scales, void *scratch,
                                    size_t scratch_bytes, void *hip_stream)
{
    if (!points || !mean || !scratch || k < 1 || k > T4D_KNN_MAX_K || n < (int64_t)k + 1 || n > INT32_MAX / 2)
        return t4d_fail(T4D_ERR_ARG, "t4d_knn_mean_sq_dist: bad arguments");
    const KnnLayout L = knn_layout(n);
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_knn_mean_sq_dist: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    char *b = (char *)scratch;
    double *part = (double *)(b + L.bbox);
    Grid *grid = (Grid *)(b + L.total - 256);
    uint64_t *keys = (uint64_t *)(b + L.keys);
    int32_t *cnt = (int32_t *)(b + L.cnt), *start = (int32_t *)(b + L.start), *cursor = (int32_t *)(b + L.cursor);
    int32_t *slot = (int32_t *)(b + L.slot), *sidx = (int32_t *)(b + L.sidx), *bsum = (int32_t *)(b + L.bsum);
    int32_t *fall = (int32_t *)(b + L.fall);
    double *spts = (double *)(b + L.spts);
    const int64_t mask = L.table - 1;
    const int nb = (int)(n < (int64_t)kBboxBlocks * kBlock ? blocks(n, kBlock) : kBboxBlocks);
    hipLaunchKernelGGL(k_bbox_partial, dim3(nb), dim3(kBlock), 0, stream, points, n, part);
    hipLaunchKernelGGL(k_grid, dim3(1), dim3(1), 0, stream, part, nb, n, grid);
    hipLaunchKernelGGL(k_fill, dim3(blocks(L.table, kBlock)), dim3(kBlock), 0, stream, keys, cnt, L.table);
    hipLaunchKernelGGL(k_insert, dim3(blocks(n, kBlock)), dim3(kBlock), 0, stream, points, n, grid, keys, cnt, slot, mask);
    t4d_scan_i32(cnt, start, cursor, bsum, L.table, stream);
    hipLaunchKernelGGL(k_scatter, dim3(blocks(n, kBlock)), dim3(kBlock), 0, stream, points, n, slot, cursor, spts, sidx);
    hipError_t e = hipMemsetAsync(fall, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return t4d_fail(T4D_ERR_HIP, "t4d_knn_mean_sq_dist memset: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_knn_grid, dim3(blocks(n, kBlock)), dim3(kBlock), 0, stream, grid, keys, start, cnt, mask, spts, sidx, n,
                       (int)k, mean, fall);
    hipLaunchKernelGGL(k_knn_brute, dim3(256), dim3(kBlock), 0, stream, spts, sidx, n, (int)k, fall, mean);
    if (log_scales) hipLaunchKernelGGL(k_log_scales, dim3(blocks(n, kBlock)), dim3(kBlock), 0, stream, mean, n, log_scales);
    return t4d_launch_status("t4d_knn_mean_sq_dist");
}
