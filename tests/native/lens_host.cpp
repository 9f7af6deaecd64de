// Host build of csrc/t4d_lens.h for the CPU tests: the undistortion kernel's per-pixel work run pixel after pixel on the CPU.
// stdin: one T4DLensView (include/topo4d_raster.h; src and dst are ignored), an int32 count of buffer rows (>= rows) and that
// many rows of src_pitch bytes.  stdout: float32 [channels, out_rows, out_cols].  Exit status: 0, or 64 on bad input.
#include <stdio.h>

#include <vector>

#include "../../topo4d_amd/csrc/t4d_lens.h"

int main()
{
    T4DLensView v;
    int32_t buf_rows;
    if (fread(&v, sizeof v, 1, stdin) != 1 || fread(&buf_rows, 4, 1, stdin) != 1) return 64;
    if (v.rows < 1 || v.cols < 1 || v.channels < 1 || v.channels > 4 || v.out_rows < 1 || v.out_cols < 1 || buf_rows < v.rows ||
        v.src_pitch < v.cols * v.channels || v.supersample < 1 || v.supersample > T4D_LENS_MAX_SUPERSAMPLE)
        return 64;
    std::vector<uint8_t> src((size_t)buf_rows * v.src_pitch);
    if (fread(src.data(), 1, src.size(), stdin) != src.size()) return 64;
    const int64_t plane = (int64_t)v.out_rows * v.out_cols;
    std::vector<float> dst((size_t)plane * v.channels);
    auto fetch = [&](int64_t r, int64_t c, int ch) -> uint8_t { return src[(size_t)(r * v.src_pitch + c * v.channels + ch)]; };
    for (int64_t ro = 0; ro < v.out_rows; ro++)
        for (int64_t co = 0; co < v.out_cols; co++) {
            double px[4];
            t4d_lens::pixel(v, ro, co, fetch, px);
            for (int ch = 0; ch < v.channels; ch++) dst[(size_t)(ch * plane + ro * v.out_cols + co)] = (float)px[ch];
        }
    return fwrite(dst.data(), sizeof(float), dst.size(), stdout) == dst.size() ? 0 : 64;
}
