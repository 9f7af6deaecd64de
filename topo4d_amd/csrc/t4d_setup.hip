// t4d_setup.hip — the coarse half of initialize_params (train.py:115-206) and the topology of initialize_losses
// (train.py:511-581, loss_util.py:114-170, 223-255, 262-318) on the device, once per run.
//
//  * t4d_setup_vertex_colors    compute_vertex_colors + get_color_from_texture (helpers.py:181-209, 300-333): one thread per
//                               triangle corner does the reference's float64 bilinear sample with Python's `% 1` and int()
//                               truncation; one thread per vertex averages its corners (vertex -> corner CSR of
//                               t4d_obj_vertex_faces), integer division as `np.mean(...).astype(int)`, and rgb = c / 255.0.
//  * t4d_setup_quaternions      external.build_quaterion (external.py:45-61) on float32(vertex normals).
//  * t4d_setup_one_ring         the neighbour loop of train.py:177-200: squared distances, the x1000 eye rule, exp(-2000 wh)
//                               with 1 -> 0, sqrt; float64, then float32.
//  * t4d_setup_region_weights   one of the iso_w / rig_w / rot_w blocks of train.py:545-581: per row a membership bit per mask,
//                               then the set masks' float32 factors applied in list order.
//  * t4d_setup_flatten_edges    the FlattenLoss / SoftFlattenLoss constructors: per candidate edge the faces holding both ends
//                               (vertex -> face CSR), then one workgroup scans and compacts the 2-face edges in order.
//  * t4d_setup_neighbor_mask    FlattenLoss_v2's [P,K,3] int64 mask from neighbor_num.
//
// Arithmetic the reference does in float64 is written operation by operation with FP contraction off.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/topo4d_raster.h"
#include "t4d_block.h"
#include "t4d_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;

unsigned grid_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// One rounded operation each, compiled under the pragma above.  The headers' __dmul_rn / __dadd_rn / __fmul_rn / __fadd_rn are
// defined before it: their operations keep the contract flag and, once inlined, a product and the sum it feeds become one fma
// (a sum of squares was one v_mul_f64 and two v_fmac_f64), which the float32 casts hid on the golden scene.
__device__ __forceinline__ double dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double dadd(double a, double b) { return a + b; }
__device__ __forceinline__ float fmul(float a, float b) { return a * b; }
__device__ __forceinline__ float fadd(float a, float b) { return a + b; }

// Python's float `x % 1.0` (Objects/floatobject.c float_rem): fmod, shifted into [0, 1) when the signs differ, +0 for 0
__device__ double py_mod1(double x)
{
    double m = fmod(x, 1.0);
    if (m != 0.0) {
        if (m < 0.0) m = dadd(m, 1.0);
    } else {
        m = 0.0;
    }
    return m;
}

// ---- a. corner colours, vertex colours --------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_corner_colors(const uint8_t *__restrict__ image, int32_t width, int32_t height,
                                                          int32_t channels, const double *__restrict__ uv, int64_t n_corners,
                                                          int32_t *__restrict__ rgb, int32_t *__restrict__ status)
{
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_corners) return;
    const double u = py_mod1(uv[2 * c]), v = py_mod1(uv[2 * c + 1]);
    const double x = dmul(u, (double)width);
    const double y = dmul(dadd(1.0, -v), (double)height);
    // int(x), int(y); getpixel raises for a column >= width or a row >= height (and int() for NaN): counted, nothing read
    if (!(x >= 0.0 && x < (double)width && y >= 0.0 && y < (double)height)) {
        for (int k = 0; k < 3; ++k) rgb[3 * c + k] = 0;
        atomicAdd(&status[0], 1);
        atomicMin(&status[1], (int32_t)c);
        return;
    }
    const int x1 = (int)x, y1 = (int)y;
    const int x2 = min(x1 + 1, width - 1), y2 = min(y1 + 1, height - 1);
    const uint8_t *q11 = image + ((int64_t)y1 * width + x1) * channels;
    const uint8_t *q21 = image + ((int64_t)y1 * width + x2) * channels;
    const uint8_t *q12 = image + ((int64_t)y2 * width + x1) * channels;
    const uint8_t *q22 = image + ((int64_t)y2 * width + x2) * channels;
    const double ax = dadd((double)x2, -x), bx = dadd(x, -(double)x1);
    const double ay = dadd((double)y2, -y), by = dadd(y, -(double)y1);
    for (int k = 0; k < 3; ++k) {
        const double r1 = dadd(dmul(ax, (double)q11[k]), dmul(bx, (double)q21[k]));
        const double r2 = dadd(dmul(ax, (double)q12[k]), dmul(bx, (double)q22[k]));
        const double p = dadd(dmul(ay, r1), dmul(by, r2));
        rgb[3 * c + k] = (int32_t)p;                                     // int(): truncation toward zero
    }
}

__global__ void __launch_bounds__(kBlock) k_vertex_colors(const int32_t *__restrict__ corner_rgb, const int32_t *__restrict__ offsets,
                                                          const int32_t *__restrict__ entries, int32_t n_vert,
                                                          int32_t *__restrict__ colors, float *__restrict__ rgb_colors,
                                                          int32_t *__restrict__ status)
{
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_vert) return;
    const int b = offsets[v], e = offsets[v + 1];
    if (e <= b) {                                                       // a vertex no corner lists: the reference's array is shorter
        atomicAdd(&status[2], 1);
        for (int k = 0; k < 3; ++k) colors[3 * v + k] = 0, rgb_colors[3 * v + k] = 0.f;
        return;
    }
    int64_t s[3] = {0, 0, 0};
    for (int i = b; i < e; ++i)
        for (int k = 0; k < 3; ++k) s[k] += corner_rgb[3 * (int64_t)entries[i] + k];
    for (int k = 0; k < 3; ++k) {
        // np.mean of integers is sum / count rounded once; astype(int) truncates: an exact integer division (|sum| < 2^53)
        const int32_t col = (int32_t)(s[k] / (int64_t)(e - b));
        colors[3 * v + k] = col;
        rgb_colors[3 * v + k] = (float)__ddiv_rn((double)col, 255.0);
    }
}

// ---- b. build_quaterion in float32 ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_quaternions(const double *__restrict__ normals, int32_t n, float *__restrict__ quat)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float d0 = (float)normals[3 * i], d1 = (float)normals[3 * i + 1], d2 = (float)normals[3 * i + 2];
    const float nrm = sqrtf(fadd(fadd(fmul(d0, d0), fmul(d1, d1)), fmul(d2, d2)));
    const float u0 = __fdiv_rn(d0, nrm), u1 = __fdiv_rn(d1, nrm), u2 = __fdiv_rn(d2, nrm);
    // cross((1,0,0), u) = (0*u2 - 0*u1, 0*u0 - 1*u2, 1*u1 - 0*u0); angle = acos(1*u0 + 0*u1 + 0*u2)
    const float ax = fadd(fmul(0.f, u2), -fmul(0.f, u1));
    const float ay = fadd(fmul(0.f, u0), -u2);
    const float az = fadd(u1, -fmul(0.f, u0));
    const float ang = acosf(fadd(fadd(u0, fmul(0.f, u1)), fmul(0.f, u2)));
    const float h = fmul(ang, 0.5f);                               // angle / 2 (exact)
    const float s = sinf(h);
    quat[4 * i] = cosf(h);
    quat[4 * i + 1] = fmul(ax, s);
    quat[4 * i + 2] = fmul(ay, s);
    quat[4 * i + 3] = fmul(az, s);
}

// ---- c. one-ring distances and weights --------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_one_ring(const float *__restrict__ means3D, int32_t n_vert, int32_t K,
                                                     const int64_t *__restrict__ nbr, const uint8_t *__restrict__ eye_del,
                                                     float *__restrict__ weight, float *__restrict__ dist, int32_t *__restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)n_vert * K) return;
    const int v = (int)(t / K);
    const int64_t j = nbr[t];
    if (j < 0 || j >= n_vert) {
        atomicAdd(&status[0], 1);
        weight[t] = 0.f, dist[t] = 0.f;
        return;
    }
    double d[3], sq = 0.0, wh = 0.0;
    for (int k = 0; k < 3; ++k) d[k] = dadd((double)means3D[3 * v + k], -(double)means3D[3 * j + k]);
    sq = dadd(dadd(dmul(d[0], d[0]), dmul(d[1], d[1])), dmul(d[2], d[2]));
    if (eye_del[j] && !eye_del[v]) {                                  // ((a - b) * 1000) ** 2, summed
        double e[3];
        for (int k = 0; k < 3; ++k) e[k] = dmul(d[k], 1000.0);
        wh = dadd(dadd(dmul(e[0], e[0]), dmul(e[1], e[1])), dmul(e[2], e[2]));
    } else {
        wh = sq;
    }
    double w = exp(dmul(-2000.0, wh));
    if (w == 1.0) w = 0.0;
    weight[t] = (float)w;
    dist[t] = (float)__dsqrt_rn(sq);
}

// ---- d. region weights ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_region_bits(const int32_t *__restrict__ rows, const int32_t *__restrict__ mask_off,
                                                        int32_t n_masks, int32_t n_vert, uint32_t *__restrict__ bits)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= mask_off[n_masks]) return;
    int m = 0;
    while (m + 1 < n_masks && mask_off[m + 1] <= t) ++m;
    const int r = rows[t];
    if (r >= 0 && r < n_vert) atomicOr(&bits[r], 1u << m);
}

__global__ void __launch_bounds__(kBlock) k_region_apply(const float *__restrict__ in, int32_t n_vert, int32_t K,
                                                         const uint32_t *__restrict__ bits, const float *__restrict__ factors,
                                                         int32_t n_masks, float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)n_vert * K) return;
    const uint32_t b = bits[t / K];
    float w = in[t];
    for (int m = 0; m < n_masks; ++m)
        if (b >> m & 1u) w = fmul(w, factors[m]);
    out[t] = w;
}

// ---- e. flatten-edge topology -----------------------------------------------------------------------------------------
// per edge: count of distinct faces holding both ends (face ids ascending: the CSR lists corners 3*face+k ascending), the
// opposite corner of the first two.  status[0]: an endpoint out of range; status[1]: a face with no corner besides the ends, on
// an edge of at most two faces
__global__ void __launch_bounds__(kBlock) k_edge_faces(const int32_t *__restrict__ faces, int32_t n_vert, const int32_t *__restrict__ offsets,
                                                       const int32_t *__restrict__ entries, const int32_t *__restrict__ edges,
                                                       int64_t n_edges, int32_t *__restrict__ info, int32_t *__restrict__ status)
{
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_edges) return;
    const int a = edges[2 * e], b = edges[2 * e + 1];
    int count = 0, opp[2] = {-1, -1}, last = -1, no_third = 0;
    if (a < 0 || a >= n_vert || b < 0 || b >= n_vert) {
        atomicAdd(&status[0], 1);
    } else {
        for (int i = offsets[a]; i < offsets[a + 1]; ++i) {
            const int f = entries[i] / 3;
            if (f == last) continue;                                   // a face listing the vertex twice (set() keeps it once)
            last = f;
            const int c0 = faces[3 * f], c1 = faces[3 * f + 1], c2 = faces[3 * f + 2];
            if (c0 != b && c1 != b && c2 != b) continue;
            if (count < 2) {
                // np.copy(face)[v != v0][v != v1][0]: the first corner that is neither end
                const int o = (c0 != a && c0 != b) ? c0 : (c1 != a && c1 != b) ? c1 : (c2 != a && c2 != b) ? c2 : -1;
                if (o < 0) ++no_third;
                opp[count] = o;
            }
            ++count;
        }
        // the reference skips an edge of more than two faces before it looks at their corners: only a kept edge can fail
        if (count <= 2 && no_third) atomicAdd(&status[1], no_third);
    }
    info[3 * e] = count;
    info[3 * e + 1] = opp[0];
    info[3 * e + 2] = opp[1];
}

// one workgroup: keep = count <= 2 ranks an edge among the kept ones (the reference's idx), two = count == 2 its output slot j.
// v0s[j], v1s[j] are read at the edge list's position idx (the reference indexes its full v0s / v1s with nosin_list, which counts
// kept edges only), v2s[j], v3s[j] are the edge's own.  out: [4, n_edges] int64; n_out: the number of slots written.
__global__ void __launch_bounds__(kBlock) k_edge_compact(const int32_t *__restrict__ edges, int64_t n_edges,
                                                         const int32_t *__restrict__ info, int64_t *__restrict__ out,
                                                         int64_t *__restrict__ n_out)
{
    __shared__ int2 tmp[kBlock];                                       // x: kept edges, y: edges with two faces
    const int t = threadIdx.x;
    int64_t keep_base = 0, two_base = 0;
    for (int64_t base = 0; base < n_edges; base += kBlock) {
        const int64_t e = base + t;
        const int cnt = e < n_edges ? info[3 * e] : 3;
        const int keep = cnt <= 2, two = cnt == 2;
        int2 all;
        const int2 before = block_exclusive_scan<kBlock>(make_int2(keep, two), make_int2(0, 0), tmp,
                                                         [](int2 a, int2 b) { return make_int2(a.x + b.x, a.y + b.y); }, &all);
        if (two) {
            const int64_t idx = keep_base + before.x, j = two_base + before.y;     // keep holds wherever two does
            out[j] = edges[2 * idx];
            out[n_edges + j] = edges[2 * idx + 1];
            out[2 * n_edges + j] = info[3 * e + 1];
            out[3 * n_edges + j] = info[3 * e + 2];
        }
        keep_base += all.x;
        two_base += all.y;
    }
    if (t == 0) *n_out = two_base;
}

// ---- f. FlattenLoss_v2's mask -----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_neighbor_mask(const int64_t *__restrict__ neighbor_num, int32_t n_vert, int32_t K,
                                                          int64_t *__restrict__ mask)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)n_vert * K * 3) return;
    const int64_t pk = t / 3;
    mask[t] = (pk % K) < neighbor_num[pk / K] ? 1 : 0;
}

}  // namespace

// =====================================================================================================================
T4D_EXPORT size_t t4d_setup_colors_scratch_bytes(int64_t n_corners)
{
    if (n_corners < 1 || n_corners > INT32_MAX) {
        t4d_fail(T4D_ERR_ARG, "t4d_setup_colors_scratch_bytes: need 1 <= n_corners < 2^31");
        return 0;
    }
    return align_up((size_t)n_corners * 3 * sizeof(int32_t));
}

T4D_EXPORT int t4d_setup_vertex_colors(const uint8_t *image, int32_t width, int32_t height, int32_t channels, const double *corner_uv,
                                       int64_t n_corners, const int32_t *offsets, const int32_t *entries, int32_t n_vert,
                                       int32_t *colors, float *rgb_colors, int32_t *status, void *scratch, size_t scratch_bytes,
                                       void *hip_stream)
{
    if (!image || !corner_uv || !offsets || !entries || !colors || !rgb_colors || !status || !scratch || width < 1 || height < 1 ||
        (channels != 3 && channels != 4) || n_corners < 1 || n_corners > INT32_MAX || n_vert < 1)
        return t4d_fail(T4D_ERR_ARG, "t4d_setup_vertex_colors: bad arguments (need an RGB / RGBA image, n_corners >= 1, n_vert >= 1)");
    if (scratch_bytes < (size_t)n_corners * 3 * sizeof(int32_t))
        return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_setup_vertex_colors: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    int32_t *corner_rgb = (int32_t *)scratch;
    const int32_t init[3] = {0, INT32_MAX, 0};
    T4D_HIP_CHECK(hipMemcpyAsync(status, init, sizeof(init), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_corner_colors, dim3(grid_of(n_corners)), dim3(kBlock), 0, stream, image, width, height, channels, corner_uv,
                       n_corners, corner_rgb, status);
    hipLaunchKernelGGL(k_vertex_colors, dim3(grid_of(n_vert)), dim3(kBlock), 0, stream, (const int32_t *)corner_rgb, offsets, entries,
                       n_vert, colors, rgb_colors, status);
    return t4d_launch_status("t4d_setup_vertex_colors");
}

T4D_EXPORT int t4d_setup_quaternions(const double *normals, int32_t n, float *quaternions, void *hip_stream)
{
    if (!normals || !quaternions || n < 1) return t4d_fail(T4D_ERR_ARG, "t4d_setup_quaternions: bad arguments (need n >= 1)");
    hipLaunchKernelGGL(k_quaternions, dim3(grid_of(n)), dim3(kBlock), 0, (hipStream_t)hip_stream, normals, n, quaternions);
    return t4d_launch_status("t4d_setup_quaternions");
}

T4D_EXPORT int t4d_setup_one_ring(const float *means3D, int32_t n_vert, int32_t K, const int64_t *neighbor_indices,
                                  const uint8_t *eye_del, float *neighbor_weight, float *neighbor_dist, int32_t *status,
                                  void *hip_stream)
{
    if (!means3D || !neighbor_indices || !eye_del || !neighbor_weight || !neighbor_dist || !status || n_vert < 1 || K < 1 ||
        (int64_t)n_vert * K > INT32_MAX)
        return t4d_fail(T4D_ERR_ARG, "t4d_setup_one_ring: bad arguments (need n_vert >= 1, K >= 1, n_vert * K < 2^31)");
    hipStream_t stream = (hipStream_t)hip_stream;
    T4D_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_one_ring, dim3(grid_of((int64_t)n_vert * K)), dim3(kBlock), 0, stream, means3D, n_vert, K, neighbor_indices,
                       eye_del, neighbor_weight, neighbor_dist, status);
    return t4d_launch_status("t4d_setup_one_ring");
}

T4D_EXPORT size_t t4d_setup_region_scratch_bytes(int32_t n_vert)
{
    if (n_vert < 1) {
        t4d_fail(T4D_ERR_ARG, "t4d_setup_region_scratch_bytes: need n_vert >= 1");
        return 0;
    }
    return align_up((size_t)n_vert * sizeof(uint32_t));
}

T4D_EXPORT int t4d_setup_region_weights(const float *neighbor_weight, int32_t n_vert, int32_t K, const int32_t *rows,
                                        const int32_t *d_mask_off, const int32_t *mask_off, int32_t n_masks, const float *factors,
                                        float *out, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!neighbor_weight || !out || !scratch || !d_mask_off || !mask_off || !factors || n_vert < 1 || K < 1 ||
        (int64_t)n_vert * K > INT32_MAX || n_masks < 0 || n_masks > T4D_SETUP_MAX_MASKS)
        return t4d_fail(T4D_ERR_ARG, "t4d_setup_region_weights: bad arguments (need n_vert, K >= 1 and 0 <= n_masks <= %d)",
                        T4D_SETUP_MAX_MASKS);
    const int32_t n_rows = mask_off[n_masks];
    if (mask_off[0] != 0 || n_rows < 0 || (n_rows > 0 && !rows))
        return t4d_fail(T4D_ERR_ARG, "t4d_setup_region_weights: mask_off must start at 0 (and rows be given when it ends above 0)");
    for (int m = 0; m < n_masks; ++m)
        if (mask_off[m + 1] < mask_off[m]) return t4d_fail(T4D_ERR_ARG, "t4d_setup_region_weights: mask_off must not decrease");
    if (scratch_bytes < (size_t)n_vert * sizeof(uint32_t)) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_setup_region_weights: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    uint32_t *bits = (uint32_t *)scratch;
    T4D_HIP_CHECK(hipMemsetAsync(bits, 0, (size_t)n_vert * sizeof(uint32_t), stream));
    if (n_rows > 0)
        hipLaunchKernelGGL(k_region_bits, dim3(grid_of(n_rows)), dim3(kBlock), 0, stream, rows, d_mask_off, n_masks, n_vert, bits);
    hipLaunchKernelGGL(k_region_apply, dim3(grid_of((int64_t)n_vert * K)), dim3(kBlock), 0, stream, neighbor_weight, n_vert, K,
                       (const uint32_t *)bits, factors, n_masks, out);
    return t4d_launch_status("t4d_setup_region_weights");
}

T4D_EXPORT size_t t4d_setup_edges_scratch_bytes(int64_t n_edges)
{
    if (n_edges < 1 || n_edges > INT32_MAX / 3) {
        t4d_fail(T4D_ERR_ARG, "t4d_setup_edges_scratch_bytes: need 1 <= n_edges < 2^31 / 3");
        return 0;
    }
    return align_up((size_t)n_edges * 3 * sizeof(int32_t));
}

T4D_EXPORT int t4d_setup_flatten_edges(const int32_t *faces, int32_t n_vert, const int32_t *offsets, const int32_t *entries,
                                       const int32_t *edges, int64_t n_edges, int64_t *out, int64_t *n_out, int32_t *status,
                                       void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!faces || !offsets || !entries || !edges || !out || !n_out || !status || !scratch || n_vert < 1 || n_edges < 1 ||
        n_edges > INT32_MAX / 3)
        return t4d_fail(T4D_ERR_ARG, "t4d_setup_flatten_edges: bad arguments (need n_vert >= 1 and 1 <= n_edges < 2^31 / 3)");
    if (scratch_bytes < (size_t)n_edges * 3 * sizeof(int32_t))
        return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_setup_flatten_edges: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    int32_t *info = (int32_t *)scratch;
    T4D_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_edge_faces, dim3(grid_of(n_edges)), dim3(kBlock), 0, stream, faces, n_vert, offsets, entries, edges, n_edges,
                       info, status);
    hipLaunchKernelGGL(k_edge_compact, dim3(1), dim3(kBlock), 0, stream, edges, n_edges, (const int32_t *)info, out, n_out);
    return t4d_launch_status("t4d_setup_flatten_edges");
}

T4D_EXPORT int t4d_setup_neighbor_mask(const int64_t *neighbor_num, int32_t n_vert, int32_t K, int64_t *mask, void *hip_stream)
{
    if (!neighbor_num || !mask || n_vert < 1 || K < 1 || (int64_t)n_vert * K * 3 > INT32_MAX)
        return t4d_fail(T4D_ERR_ARG, "t4d_setup_neighbor_mask: bad arguments (need n_vert >= 1, K >= 1, 3 * n_vert * K < 2^31)");
    hipLaunchKernelGGL(k_neighbor_mask, dim3(grid_of((int64_t)n_vert * K * 3)), dim3(kBlock), 0, (hipStream_t)hip_stream,
                       neighbor_num, n_vert, K, mask);
    return t4d_launch_status("t4d_setup_neighbor_mask");
}
