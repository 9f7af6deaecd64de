// t4d_pngdec.hip — PNG decode on the device: the read side of t4d_png.hip (png.decode_png; masks, PNG views, run-tree textures).
//
// The host parses the chunks (png.parse_png); the device inflates the IDAT stream, checks its Adler-32 and undoes the row filters.
// The inflate core and the unfilter rule are csrc/t4d_inflate.h (shared with tests/native/png_host.cpp).  Every kernel here runs one
// wave per workgroup on the inflate side, so the core's barrier is a wave barrier.  Launches, in order:
//
//  * k_pngdec_layout   one thread: each image's span of the filtered-byte arena and of the Adler partials.
//  * k_pngdec_plan     one wave per image: the stream offset of every payload (a scan of the chunk table) and its class -
//                      deflate data, header/trailer bytes, or mixed.  The image is eligible for the chunk-parallel schedule when no
//                      payload is mixed.
//  * k_pngdec_count    one wave per payload of an eligible image: inflate it alone, writing nothing; its output size, or -1 when it
//                      does not verify (t4d_inflate.h, inflate(as_chunk)).
//  * k_pngdec_scan     one wave per image: every payload verified and the sizes sum to height*row -> path 1 and the output offsets
//                      (exclusive scan), the zlib header check and the trailer; else path 2.
//  * k_pngdec_inflate  path 1: one wave per payload inflates it to its offset.  Path 2: one wave inflates the whole stream.
//  * k_pngdec_adler    one workgroup per 16 KiB of inflated bytes: the Adler-32 partial (sum, weighted sum), as k_png_encode's.
//  * k_pngdec_final    one wave per image: the partials combined as k_png_finalize combines them, compared with the trailer.
//  * k_pngdec_unfilter one wave per row that starts a band (row 0, or a row with filter 0 or 1: rows depend on the row above only
//                      under filters 2..4).  It takes its band in groups of 64 rows, lane j one pixel behind lane j - 1, so the
//                      pixel above and above-left come from the neighbouring lane's registers; the last row of a group is read
//                      back for the next.  Loads go eight steps at a time.  The same pass strips the filter bytes and swaps 16-bit
//                      samples to little-endian.
//
// No cross-workgroup flags: kernel boundaries do the ordering.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/topo4d_raster.h"
#include "t4d_block.h"
#include "t4d_host.h"
#include "t4d_inflate.h"

namespace {

using namespace t4d_inflate;

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kSeg = 16384;                       // bytes per Adler partial
constexpr int kChunkCap = 65536;                  // a payload that inflates to more does not verify
constexpr int64_t kMaxFiltered = (int64_t)1 << 38;
constexpr int kMaxImages = 65535;                 // grid.y

struct ImgPlan {
    int64_t filt_off;                             // the image's inflated bytes in the arena
    int64_t n, row;                               // height * row, 1 + width * channels * bytes_per_sample
    int64_t seg_first;                            // its first Adler partial
    int32_t eligible;
    int32_t last_data;                            // table index of the last deflate-data payload, -1
    int32_t path;
    int32_t unfilter;                             // the inflated bytes are whole and checked
    uint32_t trailer;                             // the stream's Adler-32
    uint32_t pad;
};

struct AdlerPart { uint32_t a, b; };

struct Layout {
    size_t plans, cls, csize, coff, adler, filt, total;
    int64_t segs;
    int32_t max_chunks, max_segs, max_h;
};

__host__ __device__ inline int64_t row_bytes(const T4DPngImage &im) { return 1 + (int64_t)im.width * im.channels * im.bytes_per_sample; }

bool make_layout(const T4DPngImage *images, int32_t n, int32_t n_chunks, Layout *L)
{
    if (!images || n < 1 || n > kMaxImages || n_chunks < 0) return false;
    int64_t filt = 0, segs = 0, next_chunk = 0;
    L->max_chunks = L->max_segs = L->max_h = 1;
    for (int i = 0; i < n; i++) {
        const T4DPngImage &im = images[i];
        if (im.width < 1 || im.height < 1 || im.channels < 1 || im.channels > 4 ||
            !(im.bytes_per_sample == 1 || (im.bytes_per_sample == 2 && im.channels == 1)))
            return false;
        if (im.n_chunks < 0 || im.first_chunk != next_chunk || (int64_t)im.first_chunk + im.n_chunks > n_chunks) return false;
        if (im.out_offset < 0 || (im.bytes_per_sample == 2 && (im.out_offset & 1))) return false;
        next_chunk += im.n_chunks;
        const int64_t nb = im.height * row_bytes(im);
        if (nb > kMaxFiltered) return false;
        const int64_t s = (nb + kSeg - 1) / kSeg;
        filt += (int64_t)align_up((size_t)nb);
        segs += s;
        if (im.n_chunks > L->max_chunks) L->max_chunks = im.n_chunks;
        if (s > L->max_segs) L->max_segs = (int32_t)s;
        if (im.height > L->max_h) L->max_h = im.height;
    }
    const size_t nc = (size_t)(n_chunks > 0 ? n_chunks : 1);
    size_t o = 0;
    L->plans = o; o += align_up(sizeof(ImgPlan) * (size_t)n);
    L->cls = o;   o += align_up(4 * nc);
    L->csize = o; o += align_up(4 * nc);
    L->coff = o;  o += align_up(8 * nc);
    L->adler = o; o += align_up(sizeof(AdlerPart) * (size_t)segs);
    L->filt = o;  o += (size_t)filt;
    L->total = o;
    L->segs = segs;
    return true;
}

__global__ void k_pngdec_layout(const T4DPngImage *images, int n, ImgPlan *plans)
{
    int64_t filt = 0, segs = 0;
    for (int i = 0; i < n; i++) {
        ImgPlan p;
        p.row = row_bytes(images[i]);
        p.n = images[i].height * p.row;
        p.filt_off = filt;
        p.seg_first = segs;
        p.eligible = 0; p.last_data = -1; p.path = 2; p.unfilter = 0; p.trailer = 0; p.pad = 0;
        plans[i] = p;
        filt += (int64_t)((p.n + 255) / 256 * 256);
        segs += (p.n + kSeg - 1) / kSeg;
    }
}

__global__ __launch_bounds__(kWave) void k_pngdec_plan(const T4DPngImage *images, const int64_t *chunks, ImgPlan *plans, int32_t *cls)
{
    __shared__ int64_t tmp[kWave];
    __shared__ int s_mixed[kWave], s_last[kWave];
    const int lane = threadIdx.x;
    const T4DPngImage im = images[blockIdx.x];
    const int per = (im.n_chunks + kWave - 1) / kWave;
    const int c0 = min(lane * per, im.n_chunks), c1 = min(c0 + per, im.n_chunks);
    int64_t mine = 0;
    for (int c = c0; c < c1; c++) mine += max(chunks[2 * (int64_t)(im.first_chunk + c) + 1], (int64_t)0);
    int64_t total = 0;
    int64_t soff = block_exclusive_scan<kWave>(mine, tmp, &total);
    int mixed = 0, last = -1;
    for (int c = c0; c < c1; c++) {
        const int k = im.first_chunk + c;
        const int64_t nb = max(chunks[2 * (int64_t)k + 1], (int64_t)0);
        const int cl = chunk_class(soff, nb, total);
        cls[k] = cl;
        if (cl == 3) mixed = 1;
        if (cl == 1) last = k;
        soff += nb;
    }
    s_mixed[lane] = mixed;
    s_last[lane] = last;
    __syncthreads();
    if (lane == 0) {
        for (int j = 0; j < kWave; j++) { mixed |= s_mixed[j]; last = max(last, s_last[j]); }
        ImgPlan &p = plans[blockIdx.x];
        p.last_data = last;
        p.eligible = (!mixed && last >= 0 && total >= 6) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kWave) void k_pngdec_count(const T4DPngImage *images, const int64_t *chunks, const uint8_t *data,
                                                       const ImgPlan *plans, const int32_t *cls, int32_t *csize)
{
    __shared__ Tables T;
    const int lane = threadIdx.x;
    const T4DPngImage im = images[blockIdx.y];
    if ((int)blockIdx.x >= im.n_chunks) return;
    const int k = im.first_chunk + blockIdx.x;
    const ImgPlan &p = plans[blockIdx.y];
    if (!p.eligible || cls[k] != 1) {
        if (lane == 0) csize[k] = 0;
        return;
    }
    if (lane == 0) T.fixed = 0;
    __syncthreads();
    Reader r = reader(data, chunks, k, 1);
    int64_t made = 0;
    const int err = inflate<false, kWave>(r, T, nullptr, kChunkCap, lane, true, k == p.last_data, &made);
    if (lane == 0) csize[k] = err ? -1 : (int32_t)made;
}

__global__ __launch_bounds__(kWave) void k_pngdec_scan(const T4DPngImage *images, const int64_t *chunks, const uint8_t *data,
                                                      ImgPlan *plans, const int32_t *cls, const int32_t *csize, int64_t *coff,
                                                      int32_t *status, int32_t *path)
{
    __shared__ int64_t tmp[kWave];
    __shared__ int s_bad[kWave];
    const int lane = threadIdx.x;
    const T4DPngImage im = images[blockIdx.x];
    ImgPlan &p = plans[blockIdx.x];
    int ok = p.eligible;
    if (ok) {
        const int per = (im.n_chunks + kWave - 1) / kWave;
        const int c0 = min(lane * per, im.n_chunks), c1 = min(c0 + per, im.n_chunks);
        int64_t mine = 0;
        int bad = 0;
        for (int c = c0; c < c1; c++) {
            const int32_t s = csize[im.first_chunk + c];
            if (s < 0) bad = 1;
            else mine += s;
        }
        int64_t total = 0;
        int64_t o = block_exclusive_scan<kWave>(mine, tmp, &total);
        s_bad[lane] = bad;
        __syncthreads();
        for (int j = 0; j < kWave; j++) bad |= s_bad[j];
        ok = !bad && total == p.n;
        if (ok)
            for (int c = c0; c < c1; c++) {
                coff[im.first_chunk + c] = o;
                o += csize[im.first_chunk + c];
            }
    }
    if (lane != 0) return;
    p.path = ok ? 1 : 2;
    path[blockIdx.x] = p.path;
    if (!ok) return;
    // the header's two bytes and the trailer's four, which lie in payloads of their own
    Reader r = reader(data, chunks, im.first_chunk, im.n_chunks);
    int st = 0;
    if (!need(r, 16)) st |= kErrEnd;
    else {
        const uint32_t cmf = take(r, 8), flg = take(r, 8);
        if (!zlib_header_ok(cmf, flg)) st |= kErrBlock;
    }
    uint32_t tr = 0;
    int got = 0;
    for (int c = im.n_chunks - 1; c >= 0 && got < 4; c--) {
        const int64_t o = chunks[2 * (int64_t)(im.first_chunk + c)], nb = chunks[2 * (int64_t)(im.first_chunk + c) + 1];
        for (int64_t j = nb - 1; j >= 0 && got < 4; j--) tr |= (uint32_t)data[o + j] << (8 * got++);
    }
    p.trailer = tr;
    if (st) atomicOr(&status[blockIdx.x], st);
}

__global__ __launch_bounds__(kWave) void k_pngdec_inflate(const T4DPngImage *images, const int64_t *chunks, const uint8_t *data,
                                                         ImgPlan *plans, const int32_t *cls, const int32_t *csize, const int64_t *coff,
                                                         uint8_t *filt, int32_t *status)
{
    __shared__ Tables T;
    const int lane = threadIdx.x;
    const T4DPngImage im = images[blockIdx.y];
    ImgPlan &p = plans[blockIdx.y];
    if (p.path == 1 ? (int)blockIdx.x >= im.n_chunks : blockIdx.x != 0) return;
    if (lane == 0) T.fixed = 0;
    __syncthreads();
    uint8_t *out = filt + p.filt_off;
    int64_t made = 0;
    if (p.path == 1) {
        const int k = im.first_chunk + blockIdx.x;
        if (cls[k] != 1) return;
        const int64_t o = coff[k], cap = csize[k];
        if (o < 0 || cap < 0 || o + cap > p.n) return;                // cannot happen: k_pngdec_scan summed these to p.n
        Reader r = reader(data, chunks, k, 1);
        const int err = inflate<true, kWave>(r, T, out + o, cap, lane, true, k == p.last_data, &made);
        if ((err || made != cap) && lane == 0) atomicOr(&status[blockIdx.y], kErrCode);     // cannot happen: the same parse twice
        return;
    }
    Reader r = reader(data, chunks, im.first_chunk, im.n_chunks);
    int st = 0;
    if (!need(r, 16)) st = kErrEnd;
    else {
        const uint32_t cmf = take(r, 8), flg = take(r, 8);
        if (!zlib_header_ok(cmf, flg)) st = kErrBlock;
    }
    uint32_t tr = 0;
    if (!st) {
        st = inflate<true, kWave>(r, T, out, p.n, lane, false, false, &made);
        if (!st && made != p.n) st = kErrLength;
        if (!st) {
            byte_align(r);
            if (!need(r, 32)) st = kErrEnd;
            else
                for (int j = 0; j < 4; j++) tr = (tr << 8) | take(r, 8);
        }
    }
    if (lane == 0) {
        p.trailer = tr;
        if (st) atomicOr(&status[blockIdx.y], st);
    }
}

__global__ __launch_bounds__(kBlock) void k_pngdec_adler(const ImgPlan *plans, const uint8_t *filt, AdlerPart *parts)
{
    __shared__ unsigned long long sa[kBlock], sb[kBlock];
    const ImgPlan &p = plans[blockIdx.y];
    const int64_t base = (int64_t)blockIdx.x * kSeg;
    if (base >= p.n) return;
    const int n = (int)min((int64_t)kSeg, p.n - base);
    const uint8_t *in = filt + p.filt_off + base;
    const int t = threadIdx.x;
    unsigned long long a = 0, b = 0;
    for (int i = t; i < n; i += kBlock) { const unsigned v = in[i]; a += v; b += (unsigned long long)(n - i) * v; }
    sa[t] = a; sb[t] = b;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if (t < st) { sa[t] += sa[t + st]; sb[t] += sb[t + st]; }
        __syncthreads();
    }
    if (t == 0) {
        AdlerPart q;
        q.a = (uint32_t)(sa[0] % kAdlerMod);
        q.b = (uint32_t)(sb[0] % kAdlerMod);
        parts[p.seg_first + blockIdx.x] = q;
    }
}

__global__ __launch_bounds__(kWave) void k_pngdec_final(ImgPlan *plans, const AdlerPart *parts, int32_t *status)
{
    __shared__ unsigned long long sa[kWave], sb[kWave];
    const int lane = threadIdx.x;
    ImgPlan &p = plans[blockIdx.x];
    const int64_t segs = (p.n + kSeg - 1) / kSeg;
    const uint64_t N = (uint64_t)p.n;
    unsigned long long a = 0, b = 0;
    for (int64_t k = lane; k < segs; k += kWave) {
        const AdlerPart q = parts[p.seg_first + k];
        const uint64_t nk = (uint64_t)min((int64_t)kSeg, p.n - k * kSeg);
        const uint64_t after = (N - (uint64_t)k * kSeg - nk) % kAdlerMod;        // bytes after the segment
        a = (a + q.a) % kAdlerMod;
        b = (b + q.b + after * q.a % kAdlerMod) % kAdlerMod;
    }
    sa[lane] = a; sb[lane] = b;
    __syncthreads();
    if (lane != 0) return;
    for (int j = 1; j < kWave; j++) { a += sa[j]; b += sb[j]; }
    const uint32_t aa = (uint32_t)((1 + a) % kAdlerMod);
    const uint32_t bb = (uint32_t)((N % kAdlerMod + b) % kAdlerMod);
    int st = status[blockIdx.x];
    if (!st && ((bb << 16) | aa) != p.trailer) {
        st = kErrAdler;
        atomicOr(&status[blockIdx.x], st);
    }
    p.unfilter = st ? 0 : 1;
}

// one band [y0, y1) of an image with BPP bytes per pixel, by one wave: groups of 64 rows, lane j one pixel behind lane j - 1.  The
// filtered bytes of kUnroll steps (and, for lane 0 of a later group, the pixels of the previous group's last row) are loaded
// together before the steps that use them, so the wave waits for memory once per kUnroll steps
constexpr int kUnroll = 8;

template <int BPP>
__device__ void unfilter_band(const uint8_t *__restrict__ in, uint8_t *out, int64_t row, int32_t width, int flip, int64_t y0, int64_t y1)
{
    const int lane = threadIdx.x;
    const int64_t pitch = (int64_t)width * BPP;
    for (int64_t g = y0; g < y1; g += kWave) {
        const int64_t y = g + lane;
        const bool active = y < y1;
        int ft = active ? in[y * row] : 0;
        if (ft > 4) ft = 0;                                           // flagged; the pixels are unspecified
        const uint8_t *src = in + (active ? y : y0) * row + 1;
        uint8_t *dst = out + (active ? y : y0) * pitch;
        const bool above_in_memory = lane == 0 && g > y0;             // the previous group's last row
        const int rows = (int)min((int64_t)kWave, y1 - g);
        const int64_t steps = (int64_t)width + rows - 1;
        uint32_t a = 0, c = 0, mine = 0;
        for (int64_t s0 = 0; s0 < steps; s0 += kUnroll) {
            uint32_t raw[kUnroll], up[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const int64_t x = s0 + u - lane;
                raw[u] = up[u] = 0;
                if (active && x >= 0 && x < width) {
#pragma unroll
                    for (int k = 0; k < BPP; k++) raw[u] |= (uint32_t)src[x * BPP + k] << (8 * k);
                    if (above_in_memory) {
#pragma unroll
                        for (int k = 0; k < BPP; k++) up[u] |= (uint32_t)dst[-pitch + x * BPP + (k ^ flip)] << (8 * k);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kUnroll; u++) {
                const int64_t x = s0 + u - lane;
                uint32_t b = __shfl_up(mine, 1);
                if (lane == 0) b = up[u];
                if (x == 0) a = c = 0;
                if (active && x >= 0 && x < width) {
                    uint32_t cur = 0;
#pragma unroll
                    for (int k = 0; k < BPP; k++) {
                        const uint32_t v = unfilter_byte(ft, (raw[u] >> (8 * k)) & 0xFFu, (a >> (8 * k)) & 0xFFu, (b >> (8 * k)) & 0xFFu,
                                                         (c >> (8 * k)) & 0xFFu);
                        cur |= v << (8 * k);
                        dst[x * BPP + (k ^ flip)] = (uint8_t)v;
                    }
                    a = mine = cur;
                    c = b;
                }
            }
        }
        __threadfence_block();
    }
}

__global__ __launch_bounds__(kWave) void k_pngdec_unfilter(const T4DPngImage *images, const ImgPlan *plans, const uint8_t *filt,
                                                          uint8_t *out_all, int32_t *status)
{
    const int lane = threadIdx.x;
    const T4DPngImage im = images[blockIdx.y];
    const ImgPlan &p = plans[blockIdx.y];
    const int64_t y0 = blockIdx.x;
    if (y0 >= im.height || !p.unfilter) return;
    const uint8_t *in = filt + p.filt_off;
    const int f0 = in[y0 * p.row];
    if (y0 > 0 && f0 >= 2 && f0 <= 4) return;                         // inside a band another wave takes
    if (f0 > 4 && lane == 0) atomicOr(&status[blockIdx.y], kErrFilter);
    int64_t y1 = y0 + 1;
    while (y1 < im.height) {
        const int f = in[y1 * p.row];
        if (f < 2 || f > 4) break;
        ++y1;
    }
    const int flip = im.bytes_per_sample == 2 ? 1 : 0;                // big-endian samples to little-endian
    uint8_t *out = out_all + im.out_offset;
    switch (im.channels * im.bytes_per_sample) {
    case 1: unfilter_band<1>(in, out, p.row, im.width, flip, y0, y1); break;
    case 2: unfilter_band<2>(in, out, p.row, im.width, flip, y0, y1); break;
    case 3: unfilter_band<3>(in, out, p.row, im.width, flip, y0, y1); break;
    default: unfilter_band<4>(in, out, p.row, im.width, flip, y0, y1); break;
    }
}

}  // namespace

T4D_EXPORT size_t t4d_pngdec_scratch_bytes(const T4DPngImage *images, int32_t n, int32_t n_chunks)
{
    Layout L;
    if (!make_layout(images, n, n_chunks, &L)) {
        t4d_fail(T4D_ERR_ARG, "t4d_pngdec_scratch_bytes: bad image descriptors (size, channels, sample bytes, chunk ranges not consecutive, "
                              "out_offset) or more than %d images", kMaxImages);
        return 0;
    }
    return L.total;
}

T4D_EXPORT int t4d_png_decode(const T4DPngImage *images, const T4DPngImage *d_images, int32_t n, const int64_t *d_chunks, int32_t n_chunks,
                              const uint8_t *data, uint8_t *out, size_t out_capacity, int32_t *status, int32_t *path, void *scratch,
                              size_t scratch_bytes, void *hip_stream)
{
    if (!images || !d_images || n < 1 || !d_chunks || n_chunks < 1 || !data || !out || !status || !path || !scratch)
        return t4d_fail(T4D_ERR_ARG, "t4d_png_decode: bad arguments");
    Layout L;
    if (!make_layout(images, n, n_chunks, &L)) return t4d_fail(T4D_ERR_ARG, "t4d_png_decode: bad image descriptors");
    if (scratch_bytes < L.total) return t4d_fail(T4D_ERR_STATE_SIZE, "t4d_png_decode: scratch below t4d_pngdec_scratch_bytes");
    for (int i = 0; i < n; i++) {
        const T4DPngImage &im = images[i];
        const size_t nb = (size_t)im.width * im.height * im.channels * im.bytes_per_sample;
        if ((size_t)im.out_offset > out_capacity || nb > out_capacity - (size_t)im.out_offset)
            return t4d_fail(T4D_ERR_ARG, "t4d_png_decode: image %d does not fit the output buffer", i);
    }
    hipStream_t stream = (hipStream_t)hip_stream;
    char *b = (char *)scratch;
    ImgPlan *plans = (ImgPlan *)(b + L.plans);
    int32_t *cls = (int32_t *)(b + L.cls), *csize = (int32_t *)(b + L.csize);
    int64_t *coff = (int64_t *)(b + L.coff);
    AdlerPart *parts = (AdlerPart *)(b + L.adler);
    uint8_t *filt = (uint8_t *)(b + L.filt);
    const dim3 per_chunk((unsigned)L.max_chunks, (unsigned)n), per_image((unsigned)n);
    T4D_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)n, stream));
    hipLaunchKernelGGL(k_pngdec_layout, dim3(1), dim3(1), 0, stream, d_images, n, plans);
    hipLaunchKernelGGL(k_pngdec_plan, per_image, dim3(kWave), 0, stream, d_images, d_chunks, plans, cls);
    hipLaunchKernelGGL(k_pngdec_count, per_chunk, dim3(kWave), 0, stream, d_images, d_chunks, data, plans, cls, csize);
    hipLaunchKernelGGL(k_pngdec_scan, per_image, dim3(kWave), 0, stream, d_images, d_chunks, data, plans, cls, csize, coff, status, path);
    hipLaunchKernelGGL(k_pngdec_inflate, per_chunk, dim3(kWave), 0, stream, d_images, d_chunks, data, plans, cls, csize, coff, filt,
                       status);
    hipLaunchKernelGGL(k_pngdec_adler, dim3((unsigned)L.max_segs, (unsigned)n), dim3(kBlock), 0, stream, plans, filt, parts);
    hipLaunchKernelGGL(k_pngdec_final, per_image, dim3(kWave), 0, stream, plans, parts, status);
    hipLaunchKernelGGL(k_pngdec_unfilter, dim3((unsigned)L.max_h, (unsigned)n), dim3(kWave), 0, stream, d_images, plans, filt, out,
                       status);
    return t4d_launch_status("t4d_png_decode");
}
