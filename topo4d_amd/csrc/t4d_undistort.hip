// t4d_undistort.hip — capture views undistorted by Metashape's lens model, turned and box-filtered down in one resampling
// (include/topo4d_raster.h T4DLensView; the map and the sampling are csrc/t4d_lens.h, shared with the CPU tests).
//
//   k_undistort   one block per output tile of one view (t4d_lens::tile_side by the view's supersample): the tile's source
//                 footprint, bounded by the map of the virtual tile's perimeter plus a margin, is staged in LDS; every thread
//                 then takes output pixels and sums their supersample x supersample samples in float64.  The map is not affine,
//                 so the bound is a guess and not a guarantee: a tap outside the staged rows and columns is read from global
//                 memory, as is every tap of a tile whose footprint does not fit.
#include <hip/hip_runtime.h>

#include "t4d_block.h"
#include "t4d_host.h"
#include "t4d_lens.h"

namespace {

constexpr int kBlock = 256;
constexpr int kLds = 49152;                   // staged source bytes per tile
constexpr int kMargin = 2;                    // samples around the perimeter's bounding box

__host__ __device__ inline int64_t view_tiles(const T4DLensView &v)
{
    const int t = t4d_lens::tile_side(v.supersample);
    return div_up(v.out_rows, t) * div_up(v.out_cols, t);
}

__global__ void __launch_bounds__(kBlock) k_undistort(const T4DLensView *V, int n)
{
    __shared__ uint8_t lds[kLds];
    __shared__ double red[kBlock / 64][4];
    int64_t lt;
    const int vi = find_view(V, n, blockIdx.x, &lt, [](const T4DLensView &w) { return view_tiles(w); });
    if (vi < 0) return;
    const T4DLensView v = V[vi];                  // by value: uniform registers, not re-read from memory after every store to dst
    const int s = v.supersample, T = t4d_lens::tile_side(s);
    const int64_t tc = div_up(v.out_cols, T);
    const int64_t r0 = lt / tc * T, c0 = lt % tc * T;
    const int64_t r1 = (r0 + T < v.out_rows ? r0 + T : v.out_rows) - 1;
    const int64_t c1 = (c0 + T < v.out_cols ? c0 + T : v.out_cols) - 1;
    // the virtual tile and the source coordinates of its perimeter
    const int64_t vr0 = r0 * s, vc0 = c0 * s, vr1 = (r1 + 1) * s - 1, vc1 = (c1 + 1) * s - 1;
    const int64_t W = vc1 - vc0 + 1, H = vr1 - vr0 + 1;
    double rmin = INFINITY, rmax = -INFINITY, cmin = INFINITY, cmax = -INFINITY;
    for (int64_t k = threadIdx.x; k < 2 * (W + H); k += kBlock) {
        int64_t ru, cu;
        if (k < W) ru = vr0, cu = vc0 + k;
        else if (k < 2 * W) ru = vr1, cu = vc0 + (k - W);
        else if (k < 2 * W + H) ru = vr0 + (k - 2 * W), cu = vc0;
        else ru = vr0 + (k - 2 * W - H), cu = vc1;
        double R, C, rs, cs;
        t4d_lens::sensor_rc(v.matrix, ru, cu, &R, &C);
        t4d_lens::source_rc(v.lens, R, C, &rs, &cs);
        if (!(fabs(rs) < 1e9 && fabs(cs) < 1e9)) rs = cs = INFINITY, rmin = cmin = -INFINITY;   // not finite: nothing is staged
        rmin = fmin(rmin, rs);
        rmax = fmax(rmax, rs);
        cmin = fmin(cmin, cs);
        cmax = fmax(cmax, cs);
    }
    for (int off = 32; off > 0; off >>= 1) {
        rmin = fmin(rmin, __shfl_xor(rmin, off));
        rmax = fmax(rmax, __shfl_xor(rmax, off));
        cmin = fmin(cmin, __shfl_xor(cmin, off));
        cmax = fmax(cmax, __shfl_xor(cmax, off));
    }
    if ((threadIdx.x & 63) == 0) {
        double *o = red[threadIdx.x >> 6];
        o[0] = rmin, o[1] = rmax, o[2] = cmin, o[3] = cmax;
    }
    __syncthreads();
    for (int w = 0; w < kBlock / 64; w++) {
        rmin = fmin(rmin, red[w][0]);
        rmax = fmax(rmax, red[w][1]);
        cmin = fmin(cmin, red[w][2]);
        cmax = fmax(cmax, red[w][3]);
    }
    const bool finite = rmin > -1e9 && rmax < 1e9 && cmin > -1e9 && cmax < 1e9 && rmin <= rmax && cmin <= cmax;
    int64_t br = finite ? (int64_t)floor(rmin) - kMargin : 0, bc = finite ? (int64_t)floor(cmin) - kMargin : 0;
    int64_t er = finite ? (int64_t)ceil(rmax) + kMargin : -1, ec = finite ? (int64_t)ceil(cmax) + kMargin : -1;
    br = br < 0 ? 0 : br;
    bc = bc < 0 ? 0 : bc;
    er = er > v.rows - 1 ? v.rows - 1 : er;
    ec = ec > v.cols - 1 ? v.cols - 1 : ec;
    const int64_t bh = er - br + 1, bw = ec - bc + 1;
    const bool staged = finite && bh > 0 && bw > 0 && bh * bw * v.channels <= kLds;
    const int nch = v.channels;
    const int64_t pitch = v.src_pitch;
    const uint8_t *src = v.src;
    if (staged) {
        const int64_t row_bytes = bw * nch;
        for (int64_t e = threadIdx.x; e < bh * row_bytes; e += kBlock) {
            const int64_t lr = e / row_bytes;
            lds[e] = src[(br + lr) * pitch + bc * nch + (e - lr * row_bytes)];
        }
    }
    __syncthreads();
    const int64_t sh = staged ? bh : 0, sw = staged ? bw : 0;
    auto fetch = [&](int64_t r, int64_t c, int ch) -> uint8_t {
        const int64_t lr = r - br, lc = c - bc;
        return (lr >= 0 && lr < sh && lc >= 0 && lc < sw) ? lds[(lr * sw + lc) * nch + ch] : src[r * pitch + c * nch + ch];
    };
    const int64_t plane = (int64_t)v.out_rows * v.out_cols;
    for (int idx = threadIdx.x; idx < T * T; idx += kBlock) {
        const int64_t ro = r0 + idx / T, co = c0 + idx % T;
        if (ro > r1 || co > c1) continue;
        double px[4];
        t4d_lens::pixel(v, ro, co, fetch, px);
        for (int ch = 0; ch < nch; ch++) v.dst[ch * plane + ro * v.out_cols + co] = (float)px[ch];
    }
}

bool finite_all(const double *x, int n)
{
    for (int i = 0; i < n; i++)
        if (!(fabs(x[i]) <= 1.7e308)) return false;
    return true;
}

}  // namespace

T4D_EXPORT int t4d_undistort_views(const T4DLensView *views, const T4DLensView *d_views, int32_t n_views, void *hip_stream)
{
    if (!views || !d_views || n_views < 1) return t4d_fail(T4D_ERR_ARG, "t4d_undistort_views: bad arguments");
    int64_t tiles = 0;
    for (int i = 0; i < n_views; i++) {
        const T4DLensView &v = views[i];
        if (!v.src || !v.dst || v.rows < 1 || v.cols < 1 || v.channels < 1 || v.channels > 4 || v.out_rows < 1 || v.out_cols < 1 ||
            (int64_t)v.src_pitch < (int64_t)v.cols * v.channels)
            return t4d_fail(T4D_ERR_ARG, "t4d_undistort_views: view %d: bad image descriptor", i);
        if (v.supersample < 1 || v.supersample > T4D_LENS_MAX_SUPERSAMPLE || (v.nearest != 0 && v.nearest != 1))
            return t4d_fail(T4D_ERR_ARG, "t4d_undistort_views: view %d: supersample outside 1..%d or nearest not 0 / 1", i,
                            T4D_LENS_MAX_SUPERSAMPLE);
        if ((int64_t)v.out_rows * v.supersample > 0x7fffffff || (int64_t)v.out_cols * v.supersample > 0x7fffffff)
            return t4d_fail(T4D_ERR_ARG, "t4d_undistort_views: view %d: the supersampled image is too large", i);
        if (!finite_all(v.matrix, 6) || !finite_all(v.lens, 11) || !finite_all(&v.cval, 1) || !(v.lens[t4d_lens::kF] > 0))
            return t4d_fail(T4D_ERR_ARG, "t4d_undistort_views: view %d: matrix, lens or cval not finite, or f <= 0", i);
        tiles += view_tiles(v);
    }
    if (tiles > 0x7fffffff) return t4d_fail(T4D_ERR_ARG, "t4d_undistort_views: too many tiles");
    hipLaunchKernelGGL(k_undistort, dim3((unsigned)tiles), dim3(kBlock), 0, (hipStream_t)hip_stream, d_views, n_views);
    return t4d_launch_status("t4d_undistort_views");
}
