// Non-rigid fit of a template mesh to a scan (Amberg, Romdhani, Vetter: "Optimal Step Nonrigid ICP", CVPR 2007): the device
// half of topo4d_amd/startup.py.  One outer step asks csrc/t4d_closest.hip for every moved vertex's closest point on the scan,
// classifies the pairs and fills the data terms (k_nricp_classify), builds the right-hand side and the block-Jacobi
// preconditioner's Cholesky factors (k_nricp_assemble), and solves the three coordinate columns of the normal equations by
// conjugate gradients in lock-step: three plain launches an iteration (k_nricp_apply, k_nricp_update, k_nricp_direction), the
// scalars computed on the device from sums every workgroup folds in index order for itself, so that nothing waits on the host and
// nothing spins.  k_nricp_positions moves the vertices and reports the largest move.
//
// The rules, the layouts and the reduction order are fixed in include/topo4d_raster.h, and tests/startup_ref.py states them in
// numpy bit for bit: float64, no contraction, no atomics.  A field is [3][4][n] (column, row, vertex), so that the lanes of a
// wave read consecutive doubles of every entry, for 8,280 vertices and for a few million alike.
#include <stdint.h>
#include <math.h>

#include "t4d_host.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kWaves = kBlock / kWave;
constexpr int kRec = T4D_NRICP_RECORD_DOUBLES;
constexpr int kState = T4D_NRICP_STATE_DOUBLES;
constexpr int kStateRec = 16;
constexpr int64_t kMaxVerts = INT32_MAX / 2;
constexpr int kFoldBatch = 32;
constexpr int kDotsApply = 3;                                    // P . Q per column
constexpr int kDotsUpdate = 6;                                   // R . Z, R . R per column
constexpr int kDotsStart = 9;                                    // and B . B

static_assert(T4D_NRICP_ITER + 1 == kStateRec && T4D_NRICP_STATE_BB + 3 <= kState && 2 * kStateRec <= T4D_NRICP_STATE_BB, "the state's layout");

int64_t groups_of(int64_t n)
{
    const int64_t g = (n + kBlock - 1) / kBlock;
    return g < 1 ? 1 : g > T4D_NRICP_MAX_GROUPS ? T4D_NRICP_MAX_GROUPS : g;
}

size_t area_a_bytes(int64_t groups) { return align_up(sizeof(double) * kDotsApply * (size_t)groups); }
size_t area_b_bytes(int64_t groups) { return align_up(sizeof(double) * kDotsStart * (size_t)groups); }

__device__ __forceinline__ double dot3(const double *u, const double *v)
{
#pragma clang fp contract(off)
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

__device__ __forceinline__ double dot4(const double *u, const double *v)
{
#pragma clang fp contract(off)
    return ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) + u[3] * v[3];
}

// a workgroup's sums of W values per lane, in the order of the header, to partial[blockIdx.x * W ..]
template <int W>
__device__ __forceinline__ void group_sums(double (&acc)[W], double *partial)
{
#pragma clang fp contract(off)
    __shared__ double s[kWaves][W];
#pragma unroll
    for (int w = kWave / 2; w > 0; w >>= 1) {
#pragma unroll
        for (int k = 0; k < W; k++) acc[k] = acc[k] + __shfl_down(acc[k], w, kWave);
    }
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
#pragma unroll
        for (int k = 0; k < W; k++) s[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < W) partial[(int64_t)blockIdx.x * W + threadIdx.x] = (s[0][threadIdx.x] + s[1][threadIdx.x]) + (s[2][threadIdx.x] + s[3][threadIdx.x]);
}

// entry k of the `groups` workgroup sums of width W, added to zero in index order (a batch's loads in flight together)
__device__ __forceinline__ double fold_in_order(const double *partial, int groups, int W, int k)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    int b = 0;
    for (; b + kFoldBatch <= groups; b += kFoldBatch) {
        double v[kFoldBatch];
#pragma unroll
        for (int j = 0; j < kFoldBatch; j++) v[j] = partial[(int64_t)(b + j) * W + k];
#pragma unroll
        for (int j = 0; j < kFoldBatch; j++) acc = acc + v[j];
    }
    for (; b < groups; b++) acc = acc + partial[(int64_t)b * W + k];
    return acc;
}

__global__ __launch_bounds__(kWave) void k_nricp_fold(const double *partial, int groups, int W, double *out)
{
    if ((int)threadIdx.x < W) out[threadIdx.x] = fold_in_order(partial, groups, W, threadIdx.x);
}

__global__ __launch_bounds__(kBlock) void k_nricp_classify(const double *rec, int64_t n_prims, int is_tri, const double *p, int64_t n,
                                                           const double *d2, const int32_t *prim, const double *closest,
                                                           const double *normals, const double *weights, double gate2, double cos2,
                                                           double ncos, int32_t *cls_out, double *w_out, double *target, double *partial)
{
#pragma clang fp contract(off)
    double acc[kRec];
#pragma unroll
    for (int k = 0; k < kRec; k++) acc[k] = 0.0;
    const int64_t lanes = (int64_t)gridDim.x * kBlock;
#pragma unroll 1
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += lanes) {
        const int32_t t = prim[i];
        const bool matched = t >= 0 && (int64_t)t < n_prims;
        const double dd = d2[i];
        const double pt[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
        const double cl[3] = {closest[3 * i], closest[3 * i + 1], closest[3 * i + 2]};
        const double wt = weights ? weights[i] : 1.0;
        bool degenerate = false, off = false, flipped = false;
        if (is_tri) {
            const double *a = rec + 9 * (int64_t)(matched ? t : 0), *b = a + 3, *c = a + 6;
            const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
            const double ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            const double nv[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
            const double nn = dot3(nv, nv);
            const double e[3] = {pt[0] - cl[0], pt[1] - cl[1], pt[2] - cl[2]};
            const double en = dot3(e, nv);
            degenerate = nn == 0.0;
            off = dd > 0.0 && en * en < (cos2 * dd) * nn;
            if (normals) {
                const double len = sqrt(nn);
                const double nh[3] = {nv[0] / len, nv[1] / len, nv[2] / len};
                const double m[3] = {normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]};
                flipped = dot3(m, nh) < ncos;
            }
        }
        const int cls = !matched ? 0 : (gate2 >= 0.0 && dd > gate2) ? 1 : degenerate ? 2 : off ? 3 : flipped ? 4 : wt == 0.0 ? 5 : 6;
        const bool keep = cls == 6;
        cls_out[i] = cls;
        w_out[i] = keep ? wt : 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) target[3 * i + k] = keep ? cl[k] : 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) acc[k] = acc[k] + (cls == k ? 1.0 : 0.0);
        acc[T4D_NRICP_SUM_D2] = acc[T4D_NRICP_SUM_D2] + (keep ? dd : 0.0);
    }
    group_sums<kRec>(acc, partial);
}

// z = M^-1 r for one vertex and column, L the block's Cholesky factor (entry r (r + 1) / 2 + q of L[r][q])
__device__ __forceinline__ void block_solve(const double *L, const double *r, double *z)
{
#pragma clang fp contract(off)
    double y[4];
    y[0] = r[0] / L[0];
    y[1] = (r[1] - L[1] * y[0]) / L[2];
    y[2] = ((r[2] - L[3] * y[0]) - L[4] * y[1]) / L[5];
    y[3] = (((r[3] - L[6] * y[0]) - L[7] * y[1]) - L[8] * y[2]) / L[9];
    z[3] = y[3] / L[9];
    z[2] = (y[2] - L[8] * z[3]) / L[5];
    z[1] = ((y[1] - L[4] * z[2]) - L[7] * z[3]) / L[2];
    z[0] = (((y[0] - L[1] * z[1]) - L[3] * z[2]) - L[6] * z[3]) / L[0];
}

__device__ __forceinline__ void load_block(const double *chol, int64_t n, int64_t i, double *L)
{
#pragma unroll
    for (int k = 0; k < 10; k++) L[k] = chol[(int64_t)k * n + i];
}

__global__ __launch_bounds__(kBlock) void k_nricp_assemble(const double *v, int64_t n, const int32_t *nbr_off, const double *w, const double *c,
                                                           const double *lw, const double *lt, double a2, double a2g, double beta2,
                                                           double *s_out, double *b, double *chol)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double vt[4] = {v[3 * i], v[3 * i + 1], v[3 * i + 2], 1.0};
    const double wi = w[i];
    const double bl = lw ? beta2 * lw[i] : 0.0;
    const double s = wi + bl;
    s_out[i] = s;
#pragma unroll
    for (int col = 0; col < 3; col++) {
        const double lterm = lw ? bl * lt[3 * i + col] : 0.0;
        const double m = wi * c[3 * i + col] + lterm;
#pragma unroll
        for (int r = 0; r < 4; r++) b[(int64_t)(4 * col + r) * n + i] = r < 3 ? vt[r] * m : m;
    }
    const int deg = nbr_off[i + 1] - nbr_off[i];
    double L[10];
    if (deg == 0) {
#pragma unroll
        for (int k = 0; k < 10; k++) L[k] = (k == 0 || k == 2 || k == 5 || k == 9) ? 1.0 : 0.0;
    } else {
        const double dg = (double)deg;
        double A[10];
#pragma unroll
        for (int r = 0; r < 4; r++) {
#pragma unroll
            for (int q = 0; q <= r; q++) A[r * (r + 1) / 2 + q] = (s * vt[r]) * vt[q];
            A[r * (r + 1) / 2 + r] = A[r * (r + 1) / 2 + r] + dg * (r < 3 ? a2 : a2g);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double sum = A[j * (j + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; k++) sum = sum - L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            const double d = sqrt(sum);
            L[j * (j + 1) / 2 + j] = d;
#pragma unroll
            for (int r = j + 1; r < 4; r++) {
                double t = A[r * (r + 1) / 2 + j];
#pragma unroll
                for (int k = 0; k < j; k++) t = t - L[r * (r + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
                L[r * (r + 1) / 2 + j] = t / d;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 10; k++) chol[(int64_t)k * n + i] = L[k];
}

__global__ __launch_bounds__(kBlock) void k_nricp_precond(const double *chol, int64_t n, const double *r, double *z)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double L[10];
    load_block(chol, n, i, L);
#pragma unroll
    for (int col = 0; col < 3; col++) {
        double rr[4], zz[4];
#pragma unroll
        for (int k = 0; k < 4; k++) rr[k] = r[(int64_t)(4 * col + k) * n + i];
        block_solve(L, rr, zz);
#pragma unroll
        for (int k = 0; k < 4; k++) z[(int64_t)(4 * col + k) * n + i] = zz[k];
    }
}

// Q = K P by gather over the neighbours' CSR, and the workgroup sums of P . Q per column
__global__ __launch_bounds__(kBlock) void k_nricp_apply(const double *v, int64_t n, const int32_t *nbr_off, const int32_t *nbr, const double *s,
                                                        double a2, double a2g, const double *p, double *q, double *partial)
{
#pragma clang fp contract(off)
    double acc[kDotsApply] = {0.0, 0.0, 0.0};
    const int64_t lanes = (int64_t)gridDim.x * kBlock;
#pragma unroll 1
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += lanes) {
        double pi[12], lap[12];
#pragma unroll
        for (int k = 0; k < 12; k++) {
            pi[k] = p[(int64_t)k * n + i];
            lap[k] = 0.0;
        }
        const int32_t lo = nbr_off[i], hi = nbr_off[i + 1];
#pragma unroll 1
        for (int32_t e = lo; e < hi; e++) {
            const int64_t j = nbr[e];
            double pj[12];
#pragma unroll
            for (int k = 0; k < 12; k++) pj[k] = p[(int64_t)k * n + j];
#pragma unroll
            for (int k = 0; k < 12; k++) lap[k] = lap[k] + (pi[k] - pj[k]);
        }
        const double vt[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
        const double si = s[i];
#pragma unroll
        for (int col = 0; col < 3; col++) {
            const double *pc = pi + 4 * col;
            const double t = dot3(vt, pc) + pc[3];
            const double d = si * t;
            double qc[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                qc[r] = (r < 3 ? a2 : a2g) * lap[4 * col + r] + (r < 3 ? vt[r] * d : d);
                q[(int64_t)(4 * col + r) * n + i] = qc[r];
            }
            acc[col] = acc[col] + dot4(pc, qc);
        }
    }
    group_sums<kDotsApply>(acc, partial);
}

// R = B - Q (Q = K X), Z = M^-1 R, P = Z, and the workgroup sums of R . Z, R . R, B . B per column
__global__ __launch_bounds__(kBlock) void k_nricp_residual(int64_t n, const double *chol, const double *b, const double *q, double *r, double *z,
                                                           double *p, double *partial)
{
#pragma clang fp contract(off)
    double acc[kDotsStart];
#pragma unroll
    for (int k = 0; k < kDotsStart; k++) acc[k] = 0.0;
    const int64_t lanes = (int64_t)gridDim.x * kBlock;
#pragma unroll 1
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += lanes) {
        double L[10];
        load_block(chol, n, i, L);
#pragma unroll
        for (int col = 0; col < 3; col++) {
            double bb[4], rr[4], zz[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                bb[k] = b[(int64_t)(4 * col + k) * n + i];
                rr[k] = bb[k] - q[(int64_t)(4 * col + k) * n + i];
            }
            block_solve(L, rr, zz);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                r[(int64_t)(4 * col + k) * n + i] = rr[k];
                z[(int64_t)(4 * col + k) * n + i] = zz[k];
                p[(int64_t)(4 * col + k) * n + i] = zz[k];
            }
            acc[col] = acc[col] + dot4(rr, zz);
            acc[3 + col] = acc[3 + col] + dot4(rr, rr);
            acc[6 + col] = acc[6 + col] + dot4(bb, bb);
        }
    }
    group_sums<kDotsStart>(acc, partial);
}

// record 0 of the state and ||B||^2 from the workgroup sums of k_nricp_residual
__global__ __launch_bounds__(kWave) void k_nricp_start_record(const double *partial, int groups, double *state)
{
    __shared__ double t[kDotsStart];
    if (threadIdx.x < kDotsStart) t[threadIdx.x] = fold_in_order(partial, groups, kDotsStart, threadIdx.x);
    __syncthreads();
    const int k = threadIdx.x;
    if (k < kState) state[k] = k < 6 ? t[k] : (k >= T4D_NRICP_STATE_BB && k < T4D_NRICP_STATE_BB + 3) ? t[6 + k - T4D_NRICP_STATE_BB] : 0.0;
}

// step 2 of an iteration: alpha from the folded P . Q, X = X + alpha P, R = R - alpha Q, Z = M^-1 R, the sums of R . Z and R . R
__global__ __launch_bounds__(kBlock) void k_nricp_update(int64_t n, const double *chol, const double *state_in, double *state_out, int stop_mask,
                                                         const double *partial_pq, int groups, double *x, double *r, double *z, const double *p,
                                                         const double *q, double *partial)
{
#pragma clang fp contract(off)
    __shared__ double sh_alpha[3];
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        const double pq = fold_in_order(partial_pq, groups, kDotsApply, c);
        const double alpha = (((stop_mask >> c) & 1) || pq == 0.0) ? 0.0 : state_in[T4D_NRICP_RZ + c] / pq;
        sh_alpha[c] = alpha;
        if (blockIdx.x == 0) {
            state_out[T4D_NRICP_PQ + c] = pq;
            state_out[T4D_NRICP_ALPHA + c] = alpha;
        }
    }
    __syncthreads();
    const double alpha[3] = {sh_alpha[0], sh_alpha[1], sh_alpha[2]};
    double acc[kDotsUpdate];
#pragma unroll
    for (int k = 0; k < kDotsUpdate; k++) acc[k] = 0.0;
    const int64_t lanes = (int64_t)gridDim.x * kBlock;
#pragma unroll 1
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += lanes) {
        double L[10];
        load_block(chol, n, i, L);
#pragma unroll
        for (int col = 0; col < 3; col++) {
            const double a = alpha[col];
            double rr[4], zz[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t at = (int64_t)(4 * col + k) * n + i;
                const double r0 = r[at];
                rr[k] = a == 0.0 ? r0 : r0 - a * q[at];
                if (a != 0.0) {
                    x[at] = x[at] + a * p[at];
                    r[at] = rr[k];
                }
            }
            block_solve(L, rr, zz);
#pragma unroll
            for (int k = 0; k < 4; k++) z[(int64_t)(4 * col + k) * n + i] = zz[k];
            acc[col] = acc[col] + dot4(rr, zz);
            acc[3 + col] = acc[3 + col] + dot4(rr, rr);
        }
    }
    group_sums<kDotsUpdate>(acc, partial);
}

// step 3: beta from the folded R . Z, P = Z + beta P, and the next record
__global__ __launch_bounds__(kBlock) void k_nricp_direction(int64_t n, const double *state_in, double *state_out, const double *partial_rz,
                                                            int groups, const double *z, double *p)
{
#pragma clang fp contract(off)
    __shared__ double sh_sum[kDotsUpdate];
    __shared__ double sh_beta[3];
    if (threadIdx.x < kDotsUpdate) sh_sum[threadIdx.x] = fold_in_order(partial_rz, groups, kDotsUpdate, threadIdx.x);
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        const double beta = state_out[T4D_NRICP_ALPHA + c] == 0.0 ? 0.0 : sh_sum[c] / state_in[T4D_NRICP_RZ + c];
        sh_beta[c] = beta;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (threadIdx.x < 3) {
            state_out[T4D_NRICP_RZ + threadIdx.x] = sh_sum[threadIdx.x];
            state_out[T4D_NRICP_RR + threadIdx.x] = sh_sum[3 + threadIdx.x];
            state_out[T4D_NRICP_BETA + threadIdx.x] = sh_beta[threadIdx.x];
        }
        if (threadIdx.x == 3) state_out[T4D_NRICP_ITER] = state_in[T4D_NRICP_ITER] + 1.0;
    }
    const double beta[3] = {sh_beta[0], sh_beta[1], sh_beta[2]};
    const int64_t lanes = (int64_t)gridDim.x * kBlock;
#pragma unroll 1
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += lanes) {
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const int64_t at = (int64_t)k * n + i;
            const double b = beta[k / 4];
            p[at] = b == 0.0 ? z[at] : z[at] + b * p[at];
        }
    }
}

// pos = X^T vt, and a workgroup's largest squared move
__global__ __launch_bounds__(kBlock) void k_nricp_positions(const double *v, int64_t n, const double *x, const double *prev, double *pos,
                                                            double *partial)
{
#pragma clang fp contract(off)
    __shared__ double s[kWaves];
    double best = 0.0;
    const int64_t lanes = (int64_t)gridDim.x * kBlock;
#pragma unroll 1
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += lanes) {
        const double vt[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
        double out[3], e[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int col = 0; col < 3; col++) {
            const double xc[3] = {x[(int64_t)(4 * col) * n + i], x[(int64_t)(4 * col + 1) * n + i], x[(int64_t)(4 * col + 2) * n + i]};
            out[col] = dot3(vt, xc) + x[(int64_t)(4 * col + 3) * n + i];
            if (prev) e[col] = out[col] - prev[3 * i + col];
        }
#pragma unroll
        for (int col = 0; col < 3; col++) pos[3 * i + col] = out[col];
        const double m2 = dot3(e, e);
        best = m2 > best ? m2 : best;
    }
#pragma unroll
    for (int w = kWave / 2; w > 0; w >>= 1) {
        const double o = __shfl_down(best, w, kWave);
        best = o > best ? o : best;
    }
    if (threadIdx.x % kWave == 0) s[threadIdx.x / kWave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = s[0];
#pragma unroll
        for (int k = 1; k < kWaves; k++) m = s[k] > m ? s[k] : m;
        partial[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(kWave) void k_nricp_fold_max(const double *partial, int groups, double *out)
{
    double best = 0.0;
    for (int b = threadIdx.x; b < groups; b += kWave) best = partial[b] > best ? partial[b] : best;
#pragma unroll
    for (int w = kWave / 2; w > 0; w >>= 1) {
        const double o = __shfl_down(best, w, kWave);
        best = o > best ? o : best;
    }
    if (threadIdx.x == 0) *out = best;
}

bool count_ok(int64_t n) { return n >= 0 && n <= kMaxVerts; }

bool stiffness_ok(double a2, double a2g) { return isfinite(a2) && isfinite(a2g) && a2 > 0.0 && a2g > 0.0; }

unsigned blocks_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace

T4D_EXPORT size_t t4d_nricp_scratch_bytes(int64_t n)
{
    if (!count_ok(n)) {
        t4d_fail(T4D_ERR_ARG, "t4d_nricp_scratch_bytes: need 0 <= n < 2^30");
        return 0;
    }
    const int64_t g = groups_of(n);
    return area_a_bytes(g) + area_b_bytes(g);
}

// the refusals every entry point with a scratch shares; 1: nothing to do
static int check_scratch(const char *entry, int64_t n, const void *scratch, size_t scratch_bytes)
{
    if (!count_ok(n)) return t4d_fail(T4D_ERR_ARG, "%s: need 0 <= n < 2^30", entry);
    if (n == 0) return -1;
    if (!scratch) return t4d_fail(T4D_ERR_ARG, "%s: NULL scratch", entry);
    const size_t need = t4d_nricp_scratch_bytes(n);
    if (scratch_bytes < need) return t4d_fail(T4D_ERR_STATE_SIZE, "%s: scratch too small (%zu < %zu)", entry, scratch_bytes, need);
    return T4D_OK;
}

T4D_EXPORT int t4d_nricp_classify(const void *index, size_t index_bytes, const double *points, int64_t n, const double *d2,
                                  const int32_t *prim_index, const double *closest, const double *normals, const double *weights,
                                  double gate2, double cos2, double normal_cos, int32_t *cls, double *w, double *target, double *record,
                                  void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!record) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_classify: NULL record");
    if (!isfinite(gate2) || !isfinite(cos2) || cos2 < 0.0 || cos2 > 1.0 || !isfinite(normal_cos) || normal_cos < -1.0 || normal_cos > 1.0)
        return t4d_fail(T4D_ERR_ARG, "t4d_nricp_classify: need a finite gate2 (< 0: no gate), 0 <= cos2 <= 1 and -1 <= normal_cos <= 1");
    const int rc0 = check_scratch("t4d_nricp_classify", n, scratch, scratch_bytes);
    if (rc0 > 0) return rc0;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (rc0 < 0) {
        T4D_HIP_CHECK(hipMemsetAsync(record, 0, sizeof(double) * kRec, stream));
        return T4D_OK;
    }
    if (!index || !points || !d2 || !prim_index || !closest || !cls || !w || !target || index_bytes < 256)
        return t4d_fail(T4D_ERR_ARG, "t4d_nricp_classify: NULL buffer, or an index buffer too small to hold an index");
    const double *rec = nullptr;
    int64_t n_prims = 0;
    int is_tri = 0;
    const int rc = t4d_closest_index_records("t4d_nricp_classify", index, index_bytes, hip_stream, &rec, &n_prims, &is_tri);
    if (rc != T4D_OK) return rc;
    const int64_t groups = groups_of(n);
    double *area_b = (double *)((char *)scratch + area_a_bytes(groups));
    hipLaunchKernelGGL(k_nricp_classify, dim3((unsigned)groups), dim3(kBlock), 0, stream, rec, n_prims, is_tri, points, n, d2, prim_index, closest,
                       normals, weights, gate2, cos2, normal_cos, cls, w, target, area_b);
    hipLaunchKernelGGL(k_nricp_fold, dim3(1), dim3(kWave), 0, stream, (const double *)area_b, (int)groups, kRec, record);
    return t4d_launch_status("t4d_nricp_classify");
}

T4D_EXPORT int t4d_nricp_assemble(const double *v, int64_t n, const int32_t *nbr_off, const double *w, const double *c, const double *lw,
                                  const double *lt, double a2, double a2g, double beta2, double *s, double *b, double *chol, void *hip_stream)
{
    if (!count_ok(n)) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_assemble: need 0 <= n < 2^30");
    if (!stiffness_ok(a2, a2g) || !isfinite(beta2) || beta2 < 0.0)
        return t4d_fail(T4D_ERR_ARG, "t4d_nricp_assemble: need finite a2 > 0, a2g > 0 and beta2 >= 0");
    if (n == 0) return T4D_OK;
    if (!v || !nbr_off || !w || !c || !s || !b || !chol || (lw && !lt))
        return t4d_fail(T4D_ERR_ARG, "t4d_nricp_assemble: NULL buffer, or landmark weights without landmark targets");
    hipLaunchKernelGGL(k_nricp_assemble, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)hip_stream, v, n, nbr_off, w, c, lw, lt, a2, a2g, beta2,
                       s, b, chol);
    return t4d_launch_status("t4d_nricp_assemble");
}

T4D_EXPORT int t4d_nricp_precond(const double *chol, int64_t n, const double *r, double *z, void *hip_stream)
{
    if (!count_ok(n)) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_precond: need 0 <= n < 2^30");
    if (n == 0) return T4D_OK;
    if (!chol || !r || !z) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_precond: NULL buffer");
    hipLaunchKernelGGL(k_nricp_precond, dim3(blocks_of(n)), dim3(kBlock), 0, (hipStream_t)hip_stream, chol, n, r, z);
    return t4d_launch_status("t4d_nricp_precond");
}

T4D_EXPORT int t4d_nricp_apply(const double *v, int64_t n, const int32_t *nbr_off, const int32_t *nbr, const double *s, double a2, double a2g,
                               const double *p, double *q, double *dots, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!stiffness_ok(a2, a2g)) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_apply: need finite a2 > 0 and a2g > 0");
    if (!dots) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_apply: NULL dots");
    const int rc0 = check_scratch("t4d_nricp_apply", n, scratch, scratch_bytes);
    if (rc0 > 0) return rc0;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (rc0 < 0) {
        T4D_HIP_CHECK(hipMemsetAsync(dots, 0, sizeof(double) * kDotsApply, stream));
        return T4D_OK;
    }
    if (!v || !nbr_off || !nbr || !s || !p || !q) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_apply: NULL buffer");
    const int64_t groups = groups_of(n);
    hipLaunchKernelGGL(k_nricp_apply, dim3((unsigned)groups), dim3(kBlock), 0, stream, v, n, nbr_off, nbr, s, a2, a2g, p, q, (double *)scratch);
    hipLaunchKernelGGL(k_nricp_fold, dim3(1), dim3(kWave), 0, stream, (const double *)scratch, (int)groups, kDotsApply, dots);
    return t4d_launch_status("t4d_nricp_apply");
}

T4D_EXPORT int t4d_nricp_cg_start(const double *v, int64_t n, const int32_t *nbr_off, const int32_t *nbr, const double *s, double a2,
                                  double a2g, const double *chol, const double *b, const double *x, double *r, double *z, double *p,
                                  double *q, double *state, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!stiffness_ok(a2, a2g)) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_cg_start: need finite a2 > 0 and a2g > 0");
    if (!state) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_cg_start: NULL state");
    const int rc0 = check_scratch("t4d_nricp_cg_start", n, scratch, scratch_bytes);
    if (rc0 > 0) return rc0;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (rc0 < 0) {
        T4D_HIP_CHECK(hipMemsetAsync(state, 0, sizeof(double) * kState, stream));
        return T4D_OK;
    }
    if (!v || !nbr_off || !nbr || !s || !chol || !b || !x || !r || !z || !p || !q) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_cg_start: NULL buffer");
    const int64_t groups = groups_of(n);
    double *area_a = (double *)scratch, *area_b = (double *)((char *)scratch + area_a_bytes(groups));
    hipLaunchKernelGGL(k_nricp_apply, dim3((unsigned)groups), dim3(kBlock), 0, stream, v, n, nbr_off, nbr, s, a2, a2g, x, q, area_a);
    hipLaunchKernelGGL(k_nricp_residual, dim3((unsigned)groups), dim3(kBlock), 0, stream, n, chol, b, (const double *)q, r, z, p, area_b);
    hipLaunchKernelGGL(k_nricp_start_record, dim3(1), dim3(kWave), 0, stream, (const double *)area_b, (int)groups, state);
    return t4d_launch_status("t4d_nricp_cg_start");
}

T4D_EXPORT int t4d_nricp_cg_run(const double *v, int64_t n, const int32_t *nbr_off, const int32_t *nbr, const double *s, double a2, double a2g,
                                const double *chol, double *x, double *r, double *z, double *p, double *q, double *state, int32_t done,
                                int32_t iters, int32_t stop_mask, void *scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!stiffness_ok(a2, a2g)) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_cg_run: need finite a2 > 0 and a2g > 0");
    if (done < 0 || iters < 0 || iters > T4D_NRICP_MAX_RUN || stop_mask < 0 || stop_mask > 7)
        return t4d_fail(T4D_ERR_ARG, "t4d_nricp_cg_run: need done >= 0, 0 <= iters <= %d and a stop_mask in 0..7", T4D_NRICP_MAX_RUN);
    if (!state) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_cg_run: NULL state");
    const int rc0 = check_scratch("t4d_nricp_cg_run", n, scratch, scratch_bytes);
    if (rc0 > 0) return rc0;
    if (rc0 < 0 || iters == 0) return T4D_OK;
    if (!v || !nbr_off || !nbr || !s || !chol || !x || !r || !z || !p || !q) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_cg_run: NULL buffer");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int64_t groups = groups_of(n);
    double *area_a = (double *)scratch, *area_b = (double *)((char *)scratch + area_a_bytes(groups));
    for (int32_t k = 0; k < iters; k++) {
        const int parity = (int)(((int64_t)done + k) & 1);
        const double *in = state + kStateRec * parity;
        double *out = state + kStateRec * (1 - parity);
        hipLaunchKernelGGL(k_nricp_apply, dim3((unsigned)groups), dim3(kBlock), 0, stream, v, n, nbr_off, nbr, s, a2, a2g, (const double *)p, q, area_a);
        hipLaunchKernelGGL(k_nricp_update, dim3((unsigned)groups), dim3(kBlock), 0, stream, n, chol, in, out, (int)stop_mask, (const double *)area_a,
                           (int)groups, x, r, z, (const double *)p, (const double *)q, area_b);
        hipLaunchKernelGGL(k_nricp_direction, dim3((unsigned)groups), dim3(kBlock), 0, stream, n, in, out, (const double *)area_b, (int)groups,
                           (const double *)z, p);
    }
    return t4d_launch_status("t4d_nricp_cg_run");
}

T4D_EXPORT int t4d_nricp_positions(const double *v, int64_t n, const double *x, const double *prev, double *pos, double *move2, void *scratch,
                                   size_t scratch_bytes, void *hip_stream)
{
    if (!move2) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_positions: NULL move2");
    const int rc0 = check_scratch("t4d_nricp_positions", n, scratch, scratch_bytes);
    if (rc0 > 0) return rc0;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (rc0 < 0) {
        T4D_HIP_CHECK(hipMemsetAsync(move2, 0, sizeof(double), stream));
        return T4D_OK;
    }
    if (!v || !x || !pos) return t4d_fail(T4D_ERR_ARG, "t4d_nricp_positions: NULL buffer");
    const int64_t groups = groups_of(n);
    hipLaunchKernelGGL(k_nricp_positions, dim3((unsigned)groups), dim3(kBlock), 0, stream, v, n, x, prev, pos, (double *)scratch);
    hipLaunchKernelGGL(k_nricp_fold_max, dim3(1), dim3(kWave), 0, stream, (const double *)scratch, (int)groups, move2);
    return t4d_launch_status("t4d_nricp_positions");
}
