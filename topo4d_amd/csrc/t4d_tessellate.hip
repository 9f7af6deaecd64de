// t4d_tessellate.hip — applying a finished displacement map on the device (topo4d_amd/tessellate.py): the index lists of the flat
// level-N tessellation, its points, and the fine vertices pushed along the interpolated normal by the sampled code map.
// include/topo4d_raster.h states the rules; everything is integer or float64 arithmetic in a fixed order without contraction, so
// every output is a pure function of the inputs and does not depend on the launch shape.  tests/tessellate_ref.py restates the rules
// in numpy.
//
//  * k_tess_faces     one fine triangle per thread: its coarse triangle, row and place from the id, three lattice points to ids.
//  * k_tess_points    one fine vertex per thread: (kind, edge or triangle, lattice point) from the id, then the interpolation.
//  * k_tess_displace  one fine vertex per thread, a gather: consecutive ids lie on one edge or in one triangle, so a wave reads the
//                     same few coarse corners and neighbouring texels; the owner, its UV corners and its island come from three small
//                     tables (corner owner, edges, triangles), no per-vertex record is stored anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/topo4d_raster.h"
#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxDim = 65536;
constexpr int kMaxLevel = 64;

// where a fine vertex lies: kind 0 a corner (at = its id), 1 on edge `at` at step s from lo, 2 inside triangle `at` at (i, j, k)
struct Place {
    int kind, at, s, i, j, k;
};

__device__ __forceinline__ Place place_of(int64_t id, int n_corner, int n_edges, int N)
{
    Place p = {0, (int)id, 0, 0, 0, 0};
    if (id < n_corner) return p;
    int64_t r = id - n_corner;
    const int64_t on_edges = (int64_t)n_edges * (N - 1);
    if (r < on_edges) {
        p.kind = 1;
        p.at = (int)(r / (N - 1));
        p.s = (int)(r % (N - 1)) + 1;
        return p;
    }
    r -= on_edges;
    const int I = (N - 1) * (N - 2) / 2;
    p.kind = 2;
    p.at = (int)(r / I);
    int idx = (int)(r % I), j = 1, row = N - 2;                // row j holds k = 1..N-1-j
    while (idx >= row) {
        idx -= row;
        ++j;
        --row;
    }
    p.j = j;
    p.k = idx + 1;
    p.i = N - j - p.k;
    return p;
}

__device__ __forceinline__ double mix2(double lo, double hi, int s, int N)
{
#pragma clang fp contract(off)
    const double a = (double)(N - s) * lo, b = (double)s * hi;
    return (a + b) / (double)N;
}

__device__ __forceinline__ double mix3(double a, double b, double c, int i, int j, int k, int N)
{
#pragma clang fp contract(off)
    const double x = (double)i * a, y = (double)j * b, z = (double)k * c;
    return ((x + y) + z) / (double)N;
}

// the corner of triangle `t3` (three vertex ids) that is vertex v
__device__ __forceinline__ int corner_of(const int32_t *t3, int v) { return t3[1] == v ? 1 : (t3[2] == v ? 2 : 0); }

// the id of lattice point (i, j, k) of triangle t = (a, b, c) with the edges e0 = (a, b), e1 = (b, c), e2 = (c, a)
__device__ __forceinline__ int32_t lattice_id(int a, int b, int c, int e0, int e1, int e2, int i, int j, int k, int N, int n_corner,
                                              int64_t inner_base)
{
    if (i == N) return a;
    if (j == N) return b;
    if (k == N) return c;
    if (k == 0) return (int32_t)(n_corner + (int64_t)e0 * (N - 1) + ((a < b ? j : N - j) - 1));
    if (i == 0) return (int32_t)(n_corner + (int64_t)e1 * (N - 1) + ((b < c ? k : N - k) - 1));
    if (j == 0) return (int32_t)(n_corner + (int64_t)e2 * (N - 1) + ((c < a ? i : N - i) - 1));
    return (int32_t)(inner_base + ((j - 1) * (N - 1) - (j - 1) * j / 2 + (k - 1)));
}

__global__ __launch_bounds__(kBlock) void k_tess_faces(const int32_t *tri, const int32_t *tri_edge, int64_t n_fine_tri, int n_corner,
                                                       int n_edges, int N, int32_t *out)
{
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_fine_tri) return;
    const int t = (int)(f / (N * N)), q = (int)(f % (N * N));
    int r = 0;                                                  // row r starts at r^2 and holds 2 r + 1 triangles
    for (int bit = 32; bit; bit >>= 1) {
        const int c = r | bit;
        if (c * c <= q) r = c;
    }
    const int p = q - r * r, s = p >> 1;
    const int i = N - r, j = r - s, k = s;
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    const int e0 = tri_edge[3 * t], e1 = tri_edge[3 * t + 1], e2 = tri_edge[3 * t + 2];
    const int I = (N - 1) * (N - 2) / 2;
    const int64_t inner = (int64_t)n_corner + (int64_t)n_edges * (N - 1) + (int64_t)t * I;
    int32_t v0 = lattice_id(a, b, c, e0, e1, e2, i, j, k, N, n_corner, inner), v1, v2;
    if ((p & 1) == 0) {
        v1 = lattice_id(a, b, c, e0, e1, e2, i - 1, j + 1, k, N, n_corner, inner);
        v2 = lattice_id(a, b, c, e0, e1, e2, i - 1, j, k + 1, N, n_corner, inner);
    } else {
        v1 = lattice_id(a, b, c, e0, e1, e2, i - 1, j, k + 1, N, n_corner, inner);
        v2 = lattice_id(a, b, c, e0, e1, e2, i, j - 1, k + 1, N, n_corner, inner);
    }
    out[3 * f] = v0;
    out[3 * f + 1] = v1;
    out[3 * f + 2] = v2;
}

template <int D>
__global__ __launch_bounds__(kBlock) void k_tess_points(const double *values, const int32_t *edges, const int32_t *tri, int64_t n_fine,
                                                        int n_corner, int n_edges, int N, double *out)
{
    const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (id >= n_fine) return;
    const Place p = place_of(id, n_corner, n_edges, N);
    if (p.kind == 0) {
        for (int c = 0; c < D; ++c) out[D * id + c] = values[D * id + c];
    } else if (p.kind == 1) {
        const int64_t lo = edges[3 * p.at], hi = edges[3 * p.at + 1];
        for (int c = 0; c < D; ++c) out[D * id + c] = mix2(values[D * lo + c], values[D * hi + c], p.s, N);
    } else {
        const int64_t a = tri[3 * p.at], b = tri[3 * p.at + 1], cc = tri[3 * p.at + 2];
        for (int c = 0; c < D; ++c) out[D * id + c] = mix3(values[D * a + c], values[D * b + c], values[D * cc + c], p.i, p.j, p.k, N);
    }
}

struct Tap {
    double weight;
    int64_t at;
};

__global__ __launch_bounds__(kBlock) void k_tess_displace(const double *X, const double *Nv, const double *uvs, const int32_t *corner_owner,
                                                          const int32_t *edges, const int32_t *tri, const int32_t *uv_tri,
                                                          const int32_t *tri_island, int64_t n_fine, int n_vert, int n_edges, int N,
                                                          const int32_t *code, const uint8_t *has, const uint8_t *labels, int h, int w,
                                                          double unit, double *out, uint8_t *sampled)
{
#pragma clang fp contract(off)
    const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (id >= n_fine) return;
    const Place p = place_of(id, n_vert, n_edges, N);
    double P[3], n[3], u, v;
    int owner;
    if (p.kind == 0) {
        const int co = corner_owner[id];
        for (int c = 0; c < 3; ++c) P[c] = X[3 * id + c];
        if (co < 0) {                                           // in no triangle: copied through
            for (int c = 0; c < 3; ++c) out[3 * id + c] = P[c];
            sampled[id] = 0;
            return;
        }
        owner = co / 3;
        const int64_t t = uv_tri[co];
        for (int c = 0; c < 3; ++c) n[c] = Nv[3 * id + c];
        u = uvs[2 * t];
        v = uvs[2 * t + 1];
    } else if (p.kind == 1) {
        const int64_t lo = edges[3 * p.at], hi = edges[3 * p.at + 1];
        owner = edges[3 * p.at + 2];
        const int64_t tl = uv_tri[3 * owner + corner_of(tri + 3 * owner, (int)lo)];
        const int64_t th = uv_tri[3 * owner + corner_of(tri + 3 * owner, (int)hi)];
        for (int c = 0; c < 3; ++c) {
            P[c] = mix2(X[3 * lo + c], X[3 * hi + c], p.s, N);
            n[c] = mix2(Nv[3 * lo + c], Nv[3 * hi + c], p.s, N);
        }
        u = mix2(uvs[2 * tl], uvs[2 * th], p.s, N);
        v = mix2(uvs[2 * tl + 1], uvs[2 * th + 1], p.s, N);
    } else {
        owner = p.at;
        const int64_t a = tri[3 * owner], b = tri[3 * owner + 1], cc = tri[3 * owner + 2];
        const int64_t ta = uv_tri[3 * owner], tb = uv_tri[3 * owner + 1], tc = uv_tri[3 * owner + 2];
        for (int c = 0; c < 3; ++c) {
            P[c] = mix3(X[3 * a + c], X[3 * b + c], X[3 * cc + c], p.i, p.j, p.k, N);
            n[c] = mix3(Nv[3 * a + c], Nv[3 * b + c], Nv[3 * cc + c], p.i, p.j, p.k, N);
        }
        u = mix3(uvs[2 * ta], uvs[2 * tb], uvs[2 * tc], p.i, p.j, p.k, N);
        v = mix3(uvs[2 * ta + 1], uvs[2 * tb + 1], uvs[2 * tc + 1], p.i, p.j, p.k, N);
    }
    const uint32_t L = (uint32_t)tri_island[owner];
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    bool ok = len != 0.0 && isfinite(len) && isfinite(u) && isfinite(v);
    for (int c = 0; c < 3; ++c) ok = ok && isfinite(P[c]) && isfinite(n[c]);
    double d = 0.0;
    bool any = false;
    if (ok) {
        const double x = u * (double)(w - 1), y = ((double)h - v * (double)(h - 1)) - 1.0;
        const double xmax = (double)(w >= 2 ? w - 2 : 0), ymax = (double)(h >= 2 ? h - 2 : 0);
        double xf = floor(x), yf = floor(y);
        xf = xf < 0.0 ? 0.0 : (xf > xmax ? xmax : xf);            // clamped as a double: x may be far outside an int
        yf = yf < 0.0 ? 0.0 : (yf > ymax ? ymax : yf);
        const int x0 = (int)xf, y0 = (int)yf;
        const int x1 = x0 + 1 < w ? x0 + 1 : w - 1, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
        double fx = x - xf, fy = y - yf;
        fx = fx < 0.0 ? 0.0 : (fx > 1.0 ? 1.0 : fx);
        fy = fy < 0.0 ? 0.0 : (fy > 1.0 ? 1.0 : fy);
        const Tap taps[4] = {{(1.0 - fx) * (1.0 - fy), (int64_t)y0 * w + x0}, {fx * (1.0 - fy), (int64_t)y0 * w + x1},
                             {(1.0 - fx) * fy, (int64_t)y1 * w + x0}, {fx * fy, (int64_t)y1 * w + x1}};
        double S = 0.0, W = 0.0;
        int sum = 0, count = 0;
        for (int k = 0; k < 4; ++k) {
            const int64_t at = taps[k].at;
            const bool counts = has[at] != 0 && labels[at] == L;
            const int cv = (code[at] & 0xFFFF) - 32768;
            S = S + (counts ? taps[k].weight * (double)cv : 0.0);
            W = W + (counts ? taps[k].weight : 0.0);
            sum += counts ? cv : 0;
            count += counts ? 1 : 0;
        }
        any = count > 0;
        if (W > 0.0)
            d = (S / W) * unit;
        else if (any)
            d = ((double)sum / (double)count) * unit;
    }
    if (ok)
        for (int c = 0; c < 3; ++c) out[3 * id + c] = P[c] + d * (n[c] / len);
    else
        for (int c = 0; c < 3; ++c) out[3 * id + c] = P[c];
    sampled[id] = any ? 1 : 0;
}

unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// the sizes of a level-N tessellation, or the refusal: *n_fine vertices and *n_fine_tri triangles, both below 2^31
int sizes(const char *entry, int32_t n_corner, int32_t n_edges, int32_t n_tri, int32_t level, int64_t *n_fine, int64_t *n_fine_tri)
{
    if (n_corner < 1 || n_edges < 1 || n_tri < 1)
        return t4d_fail(T4D_ERR_ARG, "%s: need at least one vertex, edge and triangle, got %d, %d and %d", entry, n_corner, n_edges, n_tri);
    if (level < 1 || level > kMaxLevel) return t4d_fail(T4D_ERR_ARG, "%s: level must be in 1..%d, got %d", entry, kMaxLevel, level);
    const int64_t N = level, I = (N - 1) * (N - 2) / 2;
    *n_fine_tri = N * N * (int64_t)n_tri;
    *n_fine = (int64_t)n_corner + (int64_t)n_edges * (N - 1) + (int64_t)n_tri * I;
    if (*n_fine_tri >= (int64_t)1 << 31 || *n_fine >= (int64_t)1 << 31)
        return t4d_fail(T4D_ERR_STATE_SIZE, "%s: level %d gives %lld triangles and %lld vertices; both must be below 2^31", entry, level,
                        (long long)*n_fine_tri, (long long)*n_fine);
    return T4D_OK;
}

}  // namespace

T4D_EXPORT int t4d_tess_faces(const int32_t *tri, const int32_t *tri_edge, int32_t n_tri, int32_t n_corner, int32_t n_edges, int32_t level,
                              int32_t *out, void *hip_stream)
{
    if (!tri || !tri_edge || !out) return t4d_fail(T4D_ERR_ARG, "t4d_tess_faces: NULL buffer");
    int64_t n_fine, n_fine_tri;
    const int rc = sizes("t4d_tess_faces", n_corner, n_edges, n_tri, level, &n_fine, &n_fine_tri);
    if (rc != T4D_OK) return rc;
    hipLaunchKernelGGL(k_tess_faces, dim3(blocks(n_fine_tri)), dim3(kBlock), 0, (hipStream_t)hip_stream, tri, tri_edge, n_fine_tri,
                       (int)n_corner, (int)n_edges, (int)level, out);
    return t4d_launch_status("t4d_tess_faces");
}

T4D_EXPORT int t4d_tess_points(const double *values, int32_t dim, int32_t n_corner, const int32_t *edges, int32_t n_edges,
                               const int32_t *tri, int32_t n_tri, int32_t level, double *out, void *hip_stream)
{
    if (!values || !edges || !tri || !out || values == out)
        return t4d_fail(T4D_ERR_ARG, "t4d_tess_points: NULL buffer, or input and output are one buffer");
    if (dim != 2 && dim != 3) return t4d_fail(T4D_ERR_ARG, "t4d_tess_points: dim must be 2 or 3, got %d", dim);
    int64_t n_fine, n_fine_tri;
    const int rc = sizes("t4d_tess_points", n_corner, n_edges, n_tri, level, &n_fine, &n_fine_tri);
    if (rc != T4D_OK) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (dim == 2)
        hipLaunchKernelGGL(k_tess_points<2>, dim3(blocks(n_fine)), dim3(kBlock), 0, stream, values, edges, tri, n_fine, (int)n_corner,
                           (int)n_edges, (int)level, out);
    else
        hipLaunchKernelGGL(k_tess_points<3>, dim3(blocks(n_fine)), dim3(kBlock), 0, stream, values, edges, tri, n_fine, (int)n_corner,
                           (int)n_edges, (int)level, out);
    return t4d_launch_status("t4d_tess_points");
}

T4D_EXPORT int t4d_tess_displace(const double *vertices, const double *normals, const double *uvs, const int32_t *corner_owner,
                                 const int32_t *edges, const int32_t *tri, const int32_t *uv_tri, const int32_t *tri_island,
                                 int32_t n_vert, int32_t n_uv, int32_t n_edges, int32_t n_tri, int32_t level, const int32_t *code,
                                 const uint8_t *has, const uint8_t *labels, int32_t h, int32_t w, double unit, double *out,
                                 uint8_t *sampled, void *hip_stream)
{
    if (!vertices || !normals || !uvs || !corner_owner || !edges || !tri || !uv_tri || !tri_island || !code || !has || !labels || !out ||
        !sampled || vertices == out)
        return t4d_fail(T4D_ERR_ARG, "t4d_tess_displace: NULL buffer, or input and output are one buffer");
    if (n_uv < 1) return t4d_fail(T4D_ERR_ARG, "t4d_tess_displace: need at least one UV vertex, got %d", n_uv);
    if (h < 1 || w < 1 || h > kMaxDim || w > kMaxDim)
        return t4d_fail(T4D_ERR_ARG, "t4d_tess_displace: need 1 <= h, w <= %d, got %d x %d", kMaxDim, h, w);
    if (!isfinite(unit)) return t4d_fail(T4D_ERR_ARG, "t4d_tess_displace: unit must be finite, got %g", unit);
    int64_t n_fine, n_fine_tri;
    const int rc = sizes("t4d_tess_displace", n_vert, n_edges, n_tri, level, &n_fine, &n_fine_tri);
    if (rc != T4D_OK) return rc;
    hipLaunchKernelGGL(k_tess_displace, dim3(blocks(n_fine)), dim3(kBlock), 0, (hipStream_t)hip_stream, vertices, normals, uvs,
                       corner_owner, edges, tri, uv_tri, tri_island, n_fine, (int)n_vert, (int)n_edges, (int)level, code, has, labels,
                       (int)h, (int)w, unit, out, sampled);
    return t4d_launch_status("t4d_tess_displace");
}
