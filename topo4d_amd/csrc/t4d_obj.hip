// t4d_obj.hip — the face.obj of helpers.save_mesh (helpers.py:963-990) on the device: trimesh's vertex normals, the frame's
// vertices, and the OBJ text with Python's float formatting.
//
//  * t4d_obj_vertex_faces    vertex -> corner CSR of a triangle list, once per topology: integer-atomic counts, one exclusive
//                            scan, an atomic fill and a per-vertex insertion sort, so every vertex lists its corners in
//                            ascending face order whatever order the fill ran in.  Counts bad indices and unreferenced vertices.
//  * t4d_obj_vertex_normals  trimesh 4.4.1 Trimesh.vertex_normals: per face its unit normal and three corner
//                            angles; per vertex sum(angle x face normal) over its CSR row in that order, unitised.  float64.
//  * t4d_obj_frame_vertices  save_mesh's vertices in one launch: the "cast scale" push along the normal in float32 (frame != 1)
//                            and the float64 global transform.
//  * t4d_obj_format_doubles  repr(float(x)) of every value into fixed 24-byte slots (csrc/t4d_repr.h), for tests.
//  * t4d_obj_float_lines     "v x y z\n" / "vt u v\n" blocks, and t4d_obj_face_lines "f a/b c/d ...\n": per row its line length
//                            and a block sum, one exclusive scan of the block sums, then per block an in-block scan and the
//                            line's bytes written at its offset - one contiguous buffer, the length to a device int64.
//
// Element-wise arithmetic is written operation by operation as numpy / torch evaluate it, with FP contraction off.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/topo4d_raster.h"
#include "t4d_block.h"
#include "t4d_host.h"
#include "t4d_repr.h"

namespace {

constexpr int kBlock = 256;
constexpr int kFaceDoubles = 6;                  // per face: unit normal xyz, corner angles 0..2
constexpr double kTolZero = 1e-13;               // trimesh tol.zero: np.finfo(np.float64).resolution * 100
constexpr double kTolMerge = 1e-8;               // trimesh tol.merge
constexpr double kPi = 3.141592653589793;
constexpr int kIntChars = 20;                    // "-9223372036854775808" (the face indices + 1 are int64)

struct GlobalTransform {
    double r[9];                                 // row-major 3x3
    double t[3];
};

// ---- one-workgroup exclusive scan ----------------------------------------------------------------------------------------
// in[0..n) -> out[0..n] exclusive (out[n] = the sum); in == out allowed
template <typename T>
__global__ void __launch_bounds__(kBlock) k_obj_scan(const T *in, int64_t n, T *out, int64_t *total_out)
{
    __shared__ T sh[kBlock];
    T carry = 0;
    for (int64_t base = 0; base < n; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const T x = i < n ? in[i] : (T)0;
        T tot;
        const T ex = block_exclusive_scan<kBlock>(x, sh, &tot);
        if (i < n) out[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        out[n] = carry;
        if (total_out) *total_out = (int64_t)carry;
    }
}

// ---- vertex -> corner CSR ------------------------------------------------------------------------------------------------
__global__ void k_obj_count(const int32_t *faces, int64_t n_corners, int32_t n_vert, int32_t *cnt, int32_t *status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_corners) return;
    const int32_t v = faces[i];
    if (v < 0 || v >= n_vert) atomicAdd(&status[0], 1);
    else atomicAdd(&cnt[v], 1);
}

__global__ void k_obj_fill(const int32_t *faces, int64_t n_corners, int32_t n_vert, const int32_t *offsets, int32_t *cursor,
                           int32_t *entries)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_corners) return;
    const int32_t v = faces[i];
    if (v < 0 || v >= n_vert) return;
    entries[offsets[v] + atomicAdd(&cursor[v], 1)] = (int32_t)i;
}

// per vertex: its corners in ascending order (= ascending face, then corner); an empty row counts as unreferenced
__global__ void k_obj_sort_rows(const int32_t *offsets, int32_t n_vert, int32_t *entries, int32_t *status)
{
    const int32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_vert) return;
    const int32_t b = offsets[v], e = offsets[v + 1];
    if (b == e) atomicAdd(&status[1], 1);
    for (int32_t i = b + 1; i < e; ++i) {
        const int32_t x = entries[i];
        int32_t j = i - 1;
        while (j >= b && entries[j] > x) {
            entries[j + 1] = entries[j];
            --j;
        }
        entries[j + 1] = x;
    }
}

// ---- trimesh vertex normals ----------------------------------------------------------------------------------------------
struct D3 {
    double x, y, z;
};

__device__ inline D3 sub(D3 a, D3 b)
{
#pragma clang fp contract(off)
    return {a.x - b.x, a.y - b.y, a.z - b.z};
}

__device__ inline double dot3(D3 a, D3 b)
{
#pragma clang fp contract(off)
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
}

// trimesh.util.unitize without check_valid: rows with norm <= tol.zero are multiplied by their norm instead of its reciprocal
__device__ inline D3 unitize(D3 a, bool *valid)
{
#pragma clang fp contract(off)
    const double n = sqrt(dot3(a, a));
    *valid = n > kTolZero;
    const double s = *valid ? 1.0 / n : n;
    return {a.x * s, a.y * s, a.z * s};
}

template <typename T>
__device__ inline D3 load3(const T *p, int64_t i)
{
    return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]};
}

// per face: trimesh.triangles.normals (a zero normal where the cross product's norm is <= tol.zero) and triangles.angles
template <typename T>
__global__ void k_obj_face_terms(const T *vertices, int32_t n_vert, const int32_t *faces, int64_t n_faces, double *face_data)
{
#pragma clang fp contract(off)
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    double *o = face_data + kFaceDoubles * f;
    if (i0 < 0 || i0 >= n_vert || i1 < 0 || i1 >= n_vert || i2 < 0 || i2 >= n_vert) {   // refused by the CSR build already
        for (int k = 0; k < kFaceDoubles; ++k) o[k] = 0.0;
        return;
    }
    const D3 a = load3(vertices, i0), b = load3(vertices, i1), c = load3(vertices, i2);
    const D3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b);
    const D3 cr = {ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x};   // np.cross
    bool valid;
    D3 n = unitize(cr, &valid);
    if (!valid) n = {0.0, 0.0, 0.0};
    bool unused;
    const D3 u = unitize(ab, &unused), v = unitize(ac, &unused), w = unitize(bc, &unused);
    const D3 mu = {-u.x, -u.y, -u.z};
    const double a0 = acos(fmin(fmax(dot3(u, v), -1.0), 1.0));
    const double a1 = acos(fmin(fmax(dot3(mu, w), -1.0), 1.0));
    const double a2 = kPi - a0 - a1;
    const bool degenerate = a0 < kTolMerge || a1 < kTolMerge || a2 < kTolMerge;
    o[0] = n.x;
    o[1] = n.y;
    o[2] = n.z;
    o[3] = degenerate ? 0.0 : a0;
    o[4] = degenerate ? 0.0 : a1;
    o[5] = degenerate ? 0.0 : a2;
}

// per vertex: scipy's CSR product of the (vertex, face) angle matrix - a face's angles at the vertex summed first - with the
// face normals, in ascending face order, then unitised
__global__ void k_obj_vertex_normals(const int32_t *offsets, const int32_t *entries, int32_t n_vert, int64_t n_faces,
                                     const double *face_data, double *normals)
{
#pragma clang fp contract(off)
    const int32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= n_vert) return;
    D3 s = {0.0, 0.0, 0.0};
    const int32_t b = offsets[v], e = offsets[v + 1];
    for (int32_t i = b; i < e;) {
        const int32_t f = entries[i] / 3;
        if (f >= n_faces) break;                                      // a CSR of other faces (refused on the host)
        double w = face_data[kFaceDoubles * (int64_t)f + 3 + entries[i] % 3];
        for (++i; i < e && entries[i] / 3 == f; ++i) w += face_data[kFaceDoubles * (int64_t)f + 3 + entries[i] % 3];
        const double *n = face_data + kFaceDoubles * (int64_t)f;
        s.x += w * n[0];
        s.y += w * n[1];
        s.z += w * n[2];
    }
    bool unused;
    const D3 u = unitize(s, &unused);
    normals[3 * (int64_t)v] = u.x;
    normals[3 * (int64_t)v + 1] = u.y;
    normals[3 * (int64_t)v + 2] = u.z;
}

// ---- the frame's vertices ------------------------------------------------------------------------------------------------
// frame != 1 (normals != NULL): v = float64(means3D) + float64(cast) * normal, cast from external.build_rotation, an inverse
// and the clamp in float32; then every frame: v @ Rg.T + tg in float64
__global__ void k_obj_frame_vertices(const float *means3D, const float *log_scales, const float *rotations, const double *normals,
                                     int32_t n_vert, GlobalTransform g, double *out)
{
#pragma clang fp contract(off)
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_vert) return;
    const int64_t k = i;
    double v[3] = {(double)means3D[3 * k], (double)means3D[3 * k + 1], (double)means3D[3 * k + 2]};
    if (normals) {
        const double nd[3] = {normals[3 * k], normals[3 * k + 1], normals[3 * k + 2]};
        float r = rotations[4 * k], x = rotations[4 * k + 1], y = rotations[4 * k + 2], z = rotations[4 * k + 3];
        const float qn = sqrtf(r * r + x * x + y * y + z * z);
        r = r / qn;
        x = x / qn;
        y = y / qn;
        z = z / qn;
        const float R[9] = {1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - r * z), 2.0f * (x * z + r * y),
                            2.0f * (x * y + r * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - r * x),
                            2.0f * (x * z - r * y), 2.0f * (y * z + r * x), 1.0f - 2.0f * (x * x + y * y)};
        // R^-1 = adj(R) / det(R)
        const float c00 = R[4] * R[8] - R[5] * R[7], c01 = R[5] * R[6] - R[3] * R[8], c02 = R[3] * R[7] - R[4] * R[6];
        const float det = R[0] * c00 + R[1] * c01 + R[2] * c02;
        const float Ri[9] = {c00 / det, (R[2] * R[7] - R[1] * R[8]) / det, (R[1] * R[5] - R[2] * R[4]) / det,
                             c01 / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[2] * R[3] - R[0] * R[5]) / det,
                             c02 / det, (R[1] * R[6] - R[0] * R[7]) / det, (R[0] * R[4] - R[1] * R[3]) / det};
        const float nf[3] = {(float)nd[0], (float)nd[1], (float)nd[2]};
        float acc = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const float nr = Ri[3 * a] * nf[0] + Ri[3 * a + 1] * nf[1] + Ri[3 * a + 2] * nf[2];
            const float s = expf(log_scales[3 * k + a]);
            acc += (nr * nr) / (s * s);
        }
        float cast = sqrtf(1.0f / acc);                  // a zero normal: 1/0 = inf -> clamped to 1e-3, times 0
        if (!isnan(cast)) cast = fminf(fmaxf(cast, 0.0f), 0.001f);
        const double cd = (double)cast;
        for (int a = 0; a < 3; ++a) v[a] = v[a] + cd * nd[a];
    }
    for (int a = 0; a < 3; ++a)
        out[3 * k + a] = ((v[0] * g.r[3 * a] + v[1] * g.r[3 * a + 1]) + v[2] * g.r[3 * a + 2]) + g.t[a];
}

// ---- text ----------------------------------------------------------------------------------------------------------------
__device__ inline int int_chars(int64_t v)
{
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    int n = v < 0 ? 2 : 1;
    while (u >= 10) {
        u /= 10;
        ++n;
    }
    return n;
}

__device__ inline int write_int(int64_t v, uint8_t *out)
{
    const int n = int_chars(v);
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    if (v < 0) out[0] = '-';
    for (int i = n - 1; i >= (v < 0 ? 1 : 0); --i) {
        out[i] = (uint8_t)('0' + u % 10);
        u /= 10;
    }
    return n;
}

__global__ void k_obj_format(const double *values, int64_t n, uint8_t *chars, uint8_t *lengths)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    lengths[i] = (uint8_t)t4d_repr::format(values[i], chars + T4D_REPR_MAX_CHARS * i);
}

// per row: its values formatted into slots, its line length ("v" / "vt", a space before every value, '\n'), the block's sum
template <int Cols>
__global__ void __launch_bounds__(kBlock) k_obj_float_rows(const double *values, int64_t rows, uint8_t *slots, uint8_t *lens,
                                                           int32_t *line_len, int64_t *block_sums)
{
    __shared__ int64_t sh[kBlock];
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t len = 0;
    if (r < rows) {
        len = (Cols == 3 ? 1 : 2) + 1;
        for (int c = 0; c < Cols; ++c) {
            const int64_t j = r * Cols + c;
            const int n = t4d_repr::format(values[j], slots + T4D_REPR_MAX_CHARS * j);
            lens[j] = (uint8_t)n;
            len += 1 + n;
        }
        line_len[r] = (int32_t)len;
    }
    int64_t tot;
    block_exclusive_scan<kBlock>(len, sh, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

template <int Cols>
__global__ void __launch_bounds__(kBlock) k_obj_float_emit(int64_t rows, const uint8_t *slots, const uint8_t *lens,
                                                           const int32_t *line_len, const int64_t *block_offs, uint8_t *out)
{
    __shared__ int64_t sh[kBlock];
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t tot;
    const int64_t ex = block_exclusive_scan<kBlock>(r < rows ? (int64_t)line_len[r] : (int64_t)0, sh, &tot);
    if (r >= rows) return;
    uint8_t *p = out + block_offs[blockIdx.x] + ex;
    *p++ = 'v';
    if (Cols == 2) *p++ = 't';
    for (int c = 0; c < Cols; ++c) {
        const int64_t j = r * Cols + c;
        const uint8_t *s = slots + T4D_REPR_MAX_CHARS * j;
        *p++ = ' ';
        for (int k = 0; k < lens[j]; ++k) *p++ = s[k];
    }
    *p = '\n';
}

__global__ void __launch_bounds__(kBlock) k_obj_face_rows(const int64_t *face_off, const int64_t *v_idx, const int64_t *uv_idx,
                                                          int64_t n_faces, int64_t n_corners, int32_t *line_len, int64_t *block_sums)
{
    __shared__ int64_t sh[kBlock];
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t len = 0;
    if (f < n_faces) {
        len = 2;                                                       // "f" and '\n'
        const int64_t b = max(face_off[f], (int64_t)0), e = min(face_off[f + 1], n_corners);
        for (int64_t i = b; i < e; ++i) len += 2 + int_chars(v_idx[i] + 1) + int_chars(uv_idx[i] + 1);
        line_len[f] = (int32_t)len;
    }
    int64_t tot;
    block_exclusive_scan<kBlock>(len, sh, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kBlock) k_obj_face_emit(const int64_t *face_off, const int64_t *v_idx, const int64_t *uv_idx,
                                                          int64_t n_faces, int64_t n_corners, const int32_t *line_len,
                                                          const int64_t *block_offs, uint8_t *out, int64_t out_capacity)
{
    __shared__ int64_t sh[kBlock];
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t tot;
    const int64_t ex = block_exclusive_scan<kBlock>(f < n_faces ? (int64_t)line_len[f] : (int64_t)0, sh, &tot);
    if (f >= n_faces) return;
    const int64_t at = block_offs[blockIdx.x] + ex;
    if (at + line_len[f] > out_capacity) return;                      // only with an inconsistent face_off (checked on the host)
    uint8_t *p = out + at;
    *p++ = 'f';
    const int64_t b = max(face_off[f], (int64_t)0), e = min(face_off[f + 1], n_corners);
    for (int64_t i = b; i < e; ++i) {
        *p++ = ' ';
        p += write_int(v_idx[i] + 1, p);
        *p++ = '/';
        p += write_int(uv_idx[i] + 1, p);
    }
    *p = '\n';
}

unsigned grid_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

constexpr int64_t kMaxRows = (int64_t)1 << 31;   // grid and int32 line lengths

int cols_of(int32_t kind) { return kind == T4D_OBJ_V ? 3 : kind == T4D_OBJ_VT ? 2 : 0; }

struct TextLayout {
    size_t slots, lens, line_len, block_sums, total;
};

// rows = lines; corners = the face corners (T4D_OBJ_F only)
TextLayout text_layout(int32_t kind, int64_t rows)
{
    const int64_t vals = rows * cols_of(kind), blocks = (rows + kBlock - 1) / kBlock;
    TextLayout L;
    L.slots = 0;
    L.lens = align_up((size_t)vals * T4D_REPR_MAX_CHARS);
    L.line_len = L.lens + align_up((size_t)vals);
    L.block_sums = L.line_len + align_up((size_t)rows * 4);
    L.total = L.block_sums + align_up((size_t)(blocks + 1) * 8);
    return L;
}

bool text_args_ok(int32_t kind, int64_t rows, int64_t corners)
{
    if (kind != T4D_OBJ_V && kind != T4D_OBJ_VT && kind != T4D_OBJ_F) return false;
    if (rows < 0 || rows >= kMaxRows) return false;
    return kind != T4D_OBJ_F || (corners >= 0 && corners < ((int64_t)1 << 40));
}

int64_t text_max_bytes(int32_t kind, int64_t rows, int64_t corners)
{
    if (kind == T4D_OBJ_F) return 2 * rows + (2 + 2 * kIntChars) * corners;
    return rows * (cols_of(kind) + 1 + cols_of(kind) * (1 + T4D_REPR_MAX_CHARS));
}

}  // namespace

T4D_EXPORT size_t t4d_obj_csr_scratch_bytes(int32_t n_vert)
{
    if (n_vert < 1) {
        t4d_fail(T4D_ERR_ARG, "t4d_obj_csr_scratch_bytes: need n_vert >= 1");
        return 0;
    }
    return align_up((size_t)n_vert * 4);
}

T4D_EXPORT int t4d_obj_vertex_faces(const int32_t *faces, int64_t n_faces, int32_t n_vert, int32_t *offsets, int32_t *entries,
                                    int32_t *status, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!faces || !offsets || !entries || !status || !scratch || n_vert < 1 || n_faces < 1 || n_faces > (INT32_MAX - 2) / 3)
        return t4d_fail(T4D_ERR_ARG, "t4d_obj_vertex_faces: bad arguments (need n_vert >= 1 and 1 <= n_faces < 2^31 / 3)");
    if (scratch_bytes < align_up((size_t)n_vert * 4)) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_obj_vertex_faces: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    int32_t *cnt = (int32_t *)scratch;
    const int64_t corners = 3 * n_faces;
    T4D_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)n_vert * 4, stream));
    T4D_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), stream));
    hipLaunchKernelGGL(k_obj_count, dim3(grid_of(corners)), dim3(kBlock), 0, stream, faces, corners, n_vert, cnt, status);
    hipLaunchKernelGGL(k_obj_scan<int32_t>, dim3(1), dim3(kBlock), 0, stream, (const int32_t *)cnt, (int64_t)n_vert, offsets,
                       (int64_t *)nullptr);
    T4D_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)n_vert * 4, stream));
    hipLaunchKernelGGL(k_obj_fill, dim3(grid_of(corners)), dim3(kBlock), 0, stream, faces, corners, n_vert, (const int32_t *)offsets,
                       cnt, entries);
    hipLaunchKernelGGL(k_obj_sort_rows, dim3(grid_of(n_vert)), dim3(kBlock), 0, stream, (const int32_t *)offsets, n_vert, entries,
                       status);
    return t4d_launch_status("t4d_obj_vertex_faces");
}

T4D_EXPORT size_t t4d_obj_normals_scratch_bytes(int64_t n_faces)
{
    if (n_faces < 1 || n_faces > (INT32_MAX - 2) / 3) {
        t4d_fail(T4D_ERR_ARG, "t4d_obj_normals_scratch_bytes: need 1 <= n_faces < 2^31 / 3");
        return 0;
    }
    return align_up((size_t)n_faces * kFaceDoubles * sizeof(double));
}

T4D_EXPORT int t4d_obj_vertex_normals(const void *vertices, int32_t is_float64, int32_t n_vert, const int32_t *faces, int64_t n_faces,
                                      const int32_t *offsets, const int32_t *entries, double *normals, void *scratch,
                                      size_t scratch_bytes, void *hip_stream)
{
    if (!vertices || !faces || !offsets || !entries || !normals || !scratch || (is_float64 != 0 && is_float64 != 1) || n_vert < 1 ||
        n_faces < 1 || n_faces > (INT32_MAX - 2) / 3)
        return t4d_fail(T4D_ERR_ARG, "t4d_obj_vertex_normals: bad arguments");
    if (scratch_bytes < (size_t)n_faces * kFaceDoubles * sizeof(double))
        return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_obj_vertex_normals: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    double *face_data = (double *)scratch;
    if (is_float64)
        hipLaunchKernelGGL(k_obj_face_terms<double>, dim3(grid_of(n_faces)), dim3(kBlock), 0, stream, (const double *)vertices, n_vert,
                           faces, n_faces, face_data);
    else
        hipLaunchKernelGGL(k_obj_face_terms<float>, dim3(grid_of(n_faces)), dim3(kBlock), 0, stream, (const float *)vertices, n_vert,
                           faces, n_faces, face_data);
    hipLaunchKernelGGL(k_obj_vertex_normals, dim3(grid_of(n_vert)), dim3(kBlock), 0, stream, offsets, entries, n_vert, n_faces,
                       (const double *)face_data, normals);
    return t4d_launch_status("t4d_obj_vertex_normals");
}

T4D_EXPORT int t4d_obj_frame_vertices(const float *means3D, const float *log_scales, const float *rotations, const double *normals,
                                      int32_t n_vert, const double *transform, double *out, void *hip_stream)
{
    if (!means3D || !transform || !out || n_vert < 1 || (normals && (!log_scales || !rotations)))
        return t4d_fail(T4D_ERR_ARG, "t4d_obj_frame_vertices: bad arguments");
    GlobalTransform g;
    for (int i = 0; i < 9; ++i) g.r[i] = transform[i];
    for (int i = 0; i < 3; ++i) g.t[i] = transform[9 + i];
    hipLaunchKernelGGL(k_obj_frame_vertices, dim3(grid_of(n_vert)), dim3(kBlock), 0, (hipStream_t)hip_stream, means3D, log_scales,
                       rotations, normals, n_vert, g, out);
    return t4d_launch_status("t4d_obj_frame_vertices");
}

T4D_EXPORT int t4d_obj_format_doubles(const double *values, int64_t n, uint8_t *chars, uint8_t *lengths, void *hip_stream)
{
    if (!values || !chars || !lengths || n < 1 || n >= kMaxRows) return t4d_fail(T4D_ERR_ARG, "t4d_obj_format_doubles: bad arguments");
    hipLaunchKernelGGL(k_obj_format, dim3(grid_of(n)), dim3(kBlock), 0, (hipStream_t)hip_stream, values, n, chars, lengths);
    return t4d_launch_status("t4d_obj_format_doubles");
}

T4D_EXPORT size_t t4d_obj_text_max_bytes(int32_t kind, int64_t rows, int64_t corners)
{
    if (!text_args_ok(kind, rows, corners)) {
        t4d_fail(T4D_ERR_ARG, "t4d_obj_text_max_bytes: need kind in {V, VT, F}, 0 <= rows < 2^31 and 0 <= corners < 2^40");
        return 0;
    }
    return (size_t)text_max_bytes(kind, rows, corners);
}

T4D_EXPORT size_t t4d_obj_text_scratch_bytes(int32_t kind, int64_t rows, int64_t corners)
{
    if (!text_args_ok(kind, rows, corners)) {
        t4d_fail(T4D_ERR_ARG, "t4d_obj_text_scratch_bytes: need kind in {V, VT, F}, 0 <= rows < 2^31 and 0 <= corners < 2^40");
        return 0;
    }
    return text_layout(kind, rows).total;
}

T4D_EXPORT int t4d_obj_float_lines(int32_t kind, const double *values, int64_t rows, uint8_t *out, size_t out_capacity,
                                   int64_t *out_bytes, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if ((kind != T4D_OBJ_V && kind != T4D_OBJ_VT) || !values || !out || !out_bytes || !scratch || rows < 1 || rows >= kMaxRows)
        return t4d_fail(T4D_ERR_ARG, "t4d_obj_float_lines: bad arguments");
    if (out_capacity < (size_t)text_max_bytes(kind, rows, 0))
        return t4d_fail(T4D_ERR_ARG, "t4d_obj_float_lines: out_capacity below t4d_obj_text_max_bytes");
    const TextLayout L = text_layout(kind, rows);
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_obj_float_lines: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    char *b = (char *)scratch;
    uint8_t *slots = (uint8_t *)(b + L.slots), *lens = (uint8_t *)(b + L.lens);
    int32_t *line_len = (int32_t *)(b + L.line_len);
    int64_t *sums = (int64_t *)(b + L.block_sums);
    const unsigned g = grid_of(rows);
    if (kind == T4D_OBJ_V)
        hipLaunchKernelGGL(k_obj_float_rows<3>, dim3(g), dim3(kBlock), 0, stream, values, rows, slots, lens, line_len, sums);
    else
        hipLaunchKernelGGL(k_obj_float_rows<2>, dim3(g), dim3(kBlock), 0, stream, values, rows, slots, lens, line_len, sums);
    hipLaunchKernelGGL(k_obj_scan<int64_t>, dim3(1), dim3(kBlock), 0, stream, (const int64_t *)sums, (int64_t)g, sums, out_bytes);
    if (kind == T4D_OBJ_V)
        hipLaunchKernelGGL(k_obj_float_emit<3>, dim3(g), dim3(kBlock), 0, stream, rows, (const uint8_t *)slots, (const uint8_t *)lens,
                           (const int32_t *)line_len, (const int64_t *)sums, out);
    else
        hipLaunchKernelGGL(k_obj_float_emit<2>, dim3(g), dim3(kBlock), 0, stream, rows, (const uint8_t *)slots, (const uint8_t *)lens,
                           (const int32_t *)line_len, (const int64_t *)sums, out);
    return t4d_launch_status("t4d_obj_float_lines");
}

T4D_EXPORT int t4d_obj_face_lines(const int64_t *face_off, const int64_t *v_idx, const int64_t *uv_idx, int64_t n_faces, int64_t n_corners,
                                  uint8_t *out, size_t out_capacity, int64_t *out_bytes, void *scratch, size_t scratch_bytes,
                                  void *hip_stream)
{
    if (!face_off || !v_idx || !uv_idx || !out || !out_bytes || !scratch || !text_args_ok(T4D_OBJ_F, n_faces, n_corners) || n_faces < 1)
        return t4d_fail(T4D_ERR_ARG, "t4d_obj_face_lines: bad arguments");
    if (out_capacity < (size_t)text_max_bytes(T4D_OBJ_F, n_faces, n_corners))
        return t4d_fail(T4D_ERR_ARG, "t4d_obj_face_lines: out_capacity below t4d_obj_text_max_bytes");
    const TextLayout L = text_layout(T4D_OBJ_F, n_faces);
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_obj_face_lines: scratch too small");
    hipStream_t stream = (hipStream_t)hip_stream;
    char *b = (char *)scratch;
    int32_t *line_len = (int32_t *)(b + L.line_len);
    int64_t *sums = (int64_t *)(b + L.block_sums);
    const unsigned g = grid_of(n_faces);
    hipLaunchKernelGGL(k_obj_face_rows, dim3(g), dim3(kBlock), 0, stream, face_off, v_idx, uv_idx, n_faces, n_corners, line_len, sums);
    hipLaunchKernelGGL(k_obj_scan<int64_t>, dim3(1), dim3(kBlock), 0, stream, (const int64_t *)sums, (int64_t)g, sums, out_bytes);
    hipLaunchKernelGGL(k_obj_face_emit, dim3(g), dim3(kBlock), 0, stream, face_off, v_idx, uv_idx, n_faces, n_corners,
                       (const int32_t *)line_len, (const int64_t *)sums, out, (int64_t)out_capacity);
    return t4d_launch_status("t4d_obj_face_lines");
}
