// t4d_lens.h — Metashape's frame-camera lens model and the sampling of T4DLensView (include/topo4d_raster.h), as device
// functions and as host ones for the CPU tests (tests/native/lens_host.cpp).  csrc/t4d_undistort.hip runs them on the GPU.
//
// Everything is float64 with every product and every sum rounded (no contraction), in the operation order written here, so that
// the numpy restatement of tests/undistort_ref.py reproduces it bit for bit.  The model is the displacement form of the
// manual's formulas: with all eight coefficients zero the source coordinates are the undistorted ones exactly.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"

#if defined(__HIPCC__)
#define T4D_LENS_FN __host__ __device__ static inline
#else
#define T4D_LENS_FN static inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)      // another host compiler: build with -ffp-contract=off
#endif

namespace t4d_lens {

enum { kF, kCxa, kCya, kK1, kK2, kK3, kK4, kP1, kP2, kB1, kB2 };  // T4DLensView::lens

// output side of a block's tile of views with this supersample: the virtual tile stays at most 88 samples wide, so that its
// source footprint (up to 4 channels, a modest magnification) fits the staged bytes
T4D_LENS_FN int tile_side(int supersample)
{
    int t = 32;
    while (t > 1 && t * supersample > 88) t >>= 1;
    return t;
}

// U's pixel (ru, cu) -> index coordinates of the undistorted sensor image (skimage's _transform_affine)
T4D_LENS_FN void sensor_rc(const double *m, int64_t ru, int64_t cu, double *r, double *c)
{
    const double x = (double)cu, y = (double)ru;
    *c = m[0] * x + m[1] * y + m[2];
    *r = m[3] * x + m[4] * y + m[5];
}

// index coordinates (R, C) of the undistorted sensor image -> index coordinates of the photograph
T4D_LENS_FN void source_rc(const double *L, double R, double C, double *rs, double *cs)
{
    const double x = ((C + 0.5) - L[kCxa]) / L[kF];
    const double y = ((R + 0.5) - L[kCya]) / L[kF];
    const double r2 = x * x + y * y;
    const double rad = r2 * (L[kK1] + r2 * (L[kK2] + r2 * (L[kK3] + r2 * L[kK4])));
    const double dx = x * rad + L[kP1] * (r2 + 2 * x * x) + 2 * L[kP2] * x * y;
    const double dy = y * rad + L[kP2] * (r2 + 2 * y * y) + 2 * L[kP1] * x * y;
    *cs = C + L[kF] * dx + L[kB1] * (x + dx) + L[kB2] * (y + dy);
    *rs = R + L[kF] * dy;
}

// fetch(r, c, ch): the photograph's byte at an in-range (r, c)
template <typename Fetch>
T4D_LENS_FN double tap(const T4DLensView &v, int64_t r, int64_t c, int ch, Fetch fetch)
{
    if (r < 0 || r >= v.rows || c < 0 || c >= v.cols) return v.cval;
    return (double)fetch(r, c, ch) / 255.0;
}

// skimage's bilinear_interpolation (mode constant), as warp_sample of t4d_ingest.hip writes it
template <typename Fetch>
T4D_LENS_FN double sample_linear(const T4DLensView &v, double r, double c, int ch, Fetch fetch)
{
    const double fr = floor(r), fc = floor(c), cr = ceil(r), cc = ceil(c);
    const int64_t minr = (int64_t)fr, minc = (int64_t)fc, maxr = (int64_t)cr, maxc = (int64_t)cc;
    const double dr = r - (double)minr, dc = c - (double)minc;
    const double tl = tap(v, minr, minc, ch, fetch), tr = tap(v, minr, maxc, ch, fetch);
    const double bl = tap(v, maxr, minc, ch, fetch), bt = tap(v, maxr, maxc, ch, fetch);
    const double top = (1 - dc) * tl + dc * tr;
    const double bottom = (1 - dc) * bl + dc * bt;
    return (1 - dr) * top + dr * bottom;
}

template <typename Fetch>
T4D_LENS_FN double sample_nearest(const T4DLensView &v, double r, double c, int ch, Fetch fetch)
{
    return tap(v, (int64_t)floor(r + 0.5), (int64_t)floor(c + 0.5), ch, fetch);
}

// a coordinate more than a sample outside the photograph (or not a number): no tap is in range and the sample is cval itself,
// without the interpolation arithmetic (whose integer conversions such a coordinate may overflow)
T4D_LENS_FN bool far_outside(const T4DLensView &v, double r, double c)
{
    return !(r > -2.0 && r < (double)v.rows + 1.0 && c > -2.0 && c < (double)v.cols + 1.0);
}

// sample (i, j) of the supersample x supersample block of dst's pixel (ro, co), every channel
template <typename Fetch>
T4D_LENS_FN void block_sample(const T4DLensView &v, int64_t ro, int64_t co, int i, int j, Fetch fetch, double *u)
{
    const int s = v.supersample;
    double R, C, rs, cs;
    sensor_rc(v.matrix, ro * s + i, co * s + j, &R, &C);
    source_rc(v.lens, R, C, &rs, &cs);
    const bool far = far_outside(v, rs, cs);
    for (int ch = 0; ch < v.channels; ch++)
        u[ch] = far ? v.cval : v.nearest ? sample_nearest(v, rs, cs, ch, fetch) : sample_linear(v, rs, cs, ch, fetch);
}

// dst's pixel (ro, co), every channel: the mean of the supersample x supersample block of U, summed in row-major order
template <typename Fetch>
T4D_LENS_FN void pixel(const T4DLensView &v, int64_t ro, int64_t co, Fetch fetch, double *out)
{
    const int s = v.supersample;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < s; i++)
        for (int j = 0; j < s; j++) {
            double u[4];
            block_sample(v, ro, co, i, j, fetch, u);
            for (int ch = 0; ch < v.channels; ch++) sum[ch] = sum[ch] + u[ch];
        }
    const double area = (double)(s * s);
    for (int ch = 0; ch < v.channels; ch++) out[ch] = sum[ch] / area;
}

}  // namespace t4d_lens
