// Host build of csrc/t4d_inflate.h for the CPU tests: the steps of csrc/t4d_pngdec.hip run one after another on the CPU, one lane.
// stdin: one T4DPngImage (include/topo4d_raster.h, first_chunk 0), its chunk table (int64 [n_chunks, 2]: offset, bytes), an int64
// data_bytes and the data.  stdout: the image, uint8 [height, width, channels] or little-endian uint16 [height, width].  Exit status:
// the decoder's status bits (0: ok) plus 128 when the serial schedule decoded the stream; 255 on bad input.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/topo4d_raster.h"
#include "../../topo4d_amd/csrc/t4d_inflate.h"

using namespace t4d_inflate;

int main()
{
    T4DPngImage im;
    if (fread(&im, sizeof im, 1, stdin) != 1) return 255;
    if (im.width < 1 || im.height < 1 || im.channels < 1 || im.channels > 4 || im.n_chunks < 1 || im.n_chunks > (1 << 24) ||
        !(im.bytes_per_sample == 1 || (im.bytes_per_sample == 2 && im.channels == 1)))
        return 255;
    std::vector<int64_t> chunks(2 * (size_t)im.n_chunks);
    int64_t data_bytes = 0;
    if (fread(chunks.data(), 16, im.n_chunks, stdin) != (size_t)im.n_chunks || fread(&data_bytes, 8, 1, stdin) != 1) return 255;
    if (data_bytes < 0 || data_bytes > ((int64_t)1 << 32)) return 255;
    // exactly data_bytes: a read outside the payloads is a read outside this allocation
    std::vector<uint8_t> data((size_t)data_bytes);
    if (data_bytes && fread(data.data(), 1, data.size(), stdin) != data.size()) return 255;
    for (int k = 0; k < im.n_chunks; k++)
        if (chunks[2 * k] < 0 || chunks[2 * k + 1] < 0 || chunks[2 * k] + chunks[2 * k + 1] > data_bytes) return 255;

    const int bpp = im.channels * im.bytes_per_sample;
    const int64_t row = 1 + (int64_t)im.width * bpp, n = im.height * row;
    std::vector<uint8_t> filt((size_t)n);                           // exactly height * row
    static Tables T;
    int status = 0, path = 2;

    // plan: stream offsets and classes
    int64_t total = 0;
    for (int k = 0; k < im.n_chunks; k++) total += chunks[2 * k + 1];
    std::vector<int> cls(im.n_chunks);
    bool mixed = false;
    int last = -1;
    int64_t soff = 0;
    for (int k = 0; k < im.n_chunks; k++) {
        cls[k] = chunk_class(soff, chunks[2 * k + 1], total);
        mixed |= cls[k] == 3;
        if (cls[k] == 1) last = k;
        soff += chunks[2 * k + 1];
    }
    uint32_t trailer = 0;
    if (!mixed && last >= 0 && total >= 6) {
        // count
        std::vector<int64_t> size(im.n_chunks, 0);
        bool ok = true;
        int64_t sum = 0;
        for (int k = 0; k < im.n_chunks && ok; k++) {
            if (cls[k] != 1) continue;
            Reader r = reader(data.data(), chunks.data(), k, 1);
            T.fixed = 0;
            ok = inflate<false, 1>(r, T, nullptr, 65536, 0, true, k == last, &size[k]) == 0;
            sum += size[k];
        }
        if (ok && sum == n) {
            path = 1;
            int64_t o = 0;
            for (int k = 0; k < im.n_chunks; k++) {
                if (cls[k] != 1) continue;
                Reader r = reader(data.data(), chunks.data(), k, 1);
                T.fixed = 0;
                int64_t made = 0;
                if (inflate<true, 1>(r, T, filt.data() + o, size[k], 0, true, k == last, &made) || made != size[k]) status |= kErrCode;
                o += size[k];
            }
            Reader r = reader(data.data(), chunks.data(), 0, im.n_chunks);
            if (!need(r, 16)) status |= kErrEnd;
            else {
                const uint32_t cmf = take(r, 8), flg = take(r, 8);
                if (!zlib_header_ok(cmf, flg)) status |= kErrBlock;
            }
            int got = 0;
            for (int k = im.n_chunks - 1; k >= 0 && got < 4; k--)
                for (int64_t j = chunks[2 * k + 1] - 1; j >= 0 && got < 4; j--) trailer |= (uint32_t)data[chunks[2 * k] + j] << (8 * got++);
        }
    }
    if (path == 2) {
        Reader r = reader(data.data(), chunks.data(), 0, im.n_chunks);
        T.fixed = 0;
        if (!need(r, 16)) status = kErrEnd;
        else {
            const uint32_t cmf = take(r, 8), flg = take(r, 8);
            if (!zlib_header_ok(cmf, flg)) status = kErrBlock;
        }
        if (!status) {
            int64_t made = 0;
            status = inflate<true, 1>(r, T, filt.data(), n, 0, false, false, &made);
            if (!status && made != n) status = kErrLength;
            if (!status) {
                byte_align(r);
                if (!need(r, 32)) status = kErrEnd;
                else
                    for (int j = 0; j < 4; j++) trailer = (trailer << 8) | take(r, 8);
            }
        }
    }
    if (!status) {
        uint32_t a = 1, b = 0;
        for (int64_t i = 0; i < n; i++) { a = (a + filt[i]) % kAdlerMod; b = (b + a) % kAdlerMod; }
        if (((b << 16) | a) != trailer) status = kErrAdler;
    }
    if (status) return status | (path == 2 ? 128 : 0);

    const int64_t pitch = (int64_t)im.width * bpp;
    const int flip = im.bytes_per_sample == 2 ? 1 : 0;
    std::vector<uint8_t> out((size_t)(im.height * pitch));
    std::vector<uint8_t> rec((size_t)(2 * pitch), 0);                // the row above and this row, in stream byte order
    for (int64_t y = 0; y < im.height; y++) {
        const uint8_t *src = filt.data() + y * row;
        uint8_t *cur = rec.data() + (y & 1) * pitch, *up = rec.data() + ((y + 1) & 1) * pitch;
        int ft = src[0];
        if (ft > 4) { status |= kErrFilter; ft = 0; }
        for (int64_t x = 0; x < pitch; x++) {
            const uint32_t a = x >= bpp ? cur[x - bpp] : 0u, b = y > 0 ? up[x] : 0u, c = (y > 0 && x >= bpp) ? up[x - bpp] : 0u;
            cur[x] = (uint8_t)unfilter_byte(ft, src[1 + x], a, b, c);
            out[y * pitch + (x ^ flip)] = cur[x];
        }
    }
    if (status) return status | (path == 2 ? 128 : 0);
    fwrite(out.data(), 1, out.size(), stdout);
    return path == 2 ? 128 : 0;
}
