// Host build of csrc/t4d_jpeg.h for the CPU tests: the GPU decoder's steps run one after another on the CPU.
// stdin: one T4DJpegImage (include/topo4d_raster.h, data_offset 0), an int32 chunk_bits (0: decode each restart interval, or the
// whole scan, as one lane) and the entropy-coded segment's data_bytes bytes.  stdout: uint8 [height, width, 3].  Exit status:
// the decoder's status bits (0: ok), 64 on bad input, 128 if the chunk lanes needed the sequential fallback.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../topo4d_amd/csrc/t4d_jpeg.h"

using namespace t4d_jpeg;

static bool is_rst(uint8_t b) { return b >= 0xD0 && b <= 0xD7; }

int main()
{
    T4DJpegImage im;
    int32_t chunk_bits;
    if (fread(&im, sizeof im, 1, stdin) != 1 || fread(&chunk_bits, 4, 1, stdin) != 1) return 64;
    std::vector<uint8_t> raw((size_t)im.data_bytes);
    if (im.data_bytes && fread(raw.data(), 1, raw.size(), stdin) != raw.size()) return 64;
    const Geom g = geometry(im);
    Huff hf[8];
    int status = 0;
    for (int s = 0; s < 8; s++)
        if (!build_huff(im.huff_bits[s], im.huff_vals[s], &hf[s])) status |= kErrCode;
    const Tables tb = tables(im, hf);
    // unstuff, RSTn positions
    std::vector<uint8_t> d;
    std::vector<int64_t> rst;
    const int64_t nb = im.data_bytes;
    for (int64_t j = 0; j < nb; j++) {
        const uint8_t b = raw[j];
        if (b == 0xFF && j + 1 < nb && is_rst(raw[j + 1])) {
            if ((raw[j + 1] - 0xD0) != (int)(rst.size() & 7)) status |= kErrRestart;
            rst.push_back((int64_t)d.size());
            continue;
        }
        if (j > 0 && raw[j - 1] == 0xFF && (b == 0 || is_rst(b))) continue;
        d.push_back(b);
    }
    d.push_back(0);
    const int64_t clen = (int64_t)d.size() - 1;
    std::vector<int16_t> coef((size_t)g.n_blocks * 64, 0);
    int rc = 0;
    if (im.restart_interval > 0) {
        if ((int64_t)rst.size() != g.n_seg - 1) return status | kErrRestart;
        if (status & kErrRestart) return status;               // as k_jpeg_decode: no lane of an image whose markers are out of order
        for (int64_t s = 0; s < g.n_seg; s++) {
            const int64_t a = s == 0 ? 0 : rst[s - 1], b = s + 1 < g.n_seg ? rst[s] : clen;
            const int64_t lim = (s + 1) * im.restart_interval < g.n_mcu ? (s + 1) * im.restart_interval : g.n_mcu;
            int32_t pred[3] = {0, 0, 0};
            status |= decode_lane(d.data() + a, b - a, tb, g, State{0, 0, 0}, (b - a) * 8, true, s * im.restart_interval * g.bpm - 1,
                                  lim * g.bpm, pred, coef.data());
        }
    } else {
        const int64_t cb = chunk_bits > 0 ? chunk_bits : (clen * 8 > 0 ? clen * 8 : 1);
        // lanes are counted on the stuffed bytes, as the GPU counts them; those past the compacted data have no chunk
        const int64_t bits = clen * 8, n = nb > 0 ? (nb * 8 + cb - 1) / cb : 1, last = bits > 0 ? (bits - 1) / cb : 0;
        std::vector<State> S(n), E(n), En(n);
        std::vector<LaneCounts> cnt(n);
        auto end_of = [&](int64_t t) { return (t + 1) * cb < bits ? (t + 1) * cb : bits; };
        for (int64_t t = 0; t <= last; t++) {                   // round 0: every lane from a guessed state
            S[t] = State{t * cb, 0, 0};
            State s = S[t];
            run_counts(d.data(), clen, tb, g, s, end_of(t), cnt[t]);
            E[t] = s;
        }
        bool changed = last > 0;
        for (int r = 1; r < kRounds && changed; r++) {               // the GPU's rounds: lane t restarts from lane t-1's last exit
            changed = false;
            En = E;
            for (int64_t t = 1; t <= last; t++) {
                if (same(E[t - 1], S[t])) continue;
                S[t] = E[t - 1];
                State s = S[t];
                run_counts(d.data(), clen, tb, g, s, end_of(t), cnt[t]);
                En[t] = s;
                changed = true;
            }
            E = En;
        }
        if (changed) {                                         // the sequential fallback
            rc = 128;
            State s{0, 0, 0};
            for (int64_t t = 0; t <= last; t++) {
                S[t] = s;
                run_counts(d.data(), clen, tb, g, s, end_of(t), cnt[t]);
            }
        }
        int64_t blk = 0;
        int32_t pre[3] = {0, 0, 0};
        for (int64_t t = 0; t <= last; t++) {
            int32_t pred[3] = {pre[0], pre[1], pre[2]};
            status |= decode_lane(d.data(), clen, tb, g, S[t], end_of(t), end_of(t) >= bits, blk - 1, g.n_blocks, pred, coef.data());
            blk += cnt[t].blocks;
            for (int c = 0; c < 3; c++) pre[c] = (int32_t)((uint32_t)pre[c] + (uint32_t)cnt[t].dc[c]);
        }
    }
    if (status) return status;
    std::vector<uint8_t> planes[3];
    for (int c = 0; c < 3; c++) planes[c].assign((size_t)g.pitch[c] * g.rows[c], 0);
    for (int64_t b = 0; b < g.n_blocks; b++) {
        int c;
        int64_t x, y;
        block_origin(g, b, &c, &x, &y);
        idct_islow(&coef[b * 64], im.quant[im.comp_quant[c]], planes[c].data() + y * g.pitch[c] + x, g.pitch[c]);
    }
    std::vector<uint8_t> out((size_t)im.width * im.height * 3);
    for (int y = 0; y < im.height; y++)
        for (int x = 0; x < im.width; x++) {
            const int Y = planes[0][(size_t)y * g.pitch[0] + x];
            const int cb = upsample(planes[1].data(), g.pitch[1], g.cw[1], g.ch[1], g.hs, g.vs, x, y);
            const int cr = upsample(planes[2].data(), g.pitch[2], g.cw[2], g.ch[2], g.hs, g.vs, x, y);
            ycc_to_rgb(Y, cb, cr, &out[((size_t)y * im.width + x) * 3]);
        }
    fwrite(out.data(), 1, out.size(), stdout);
    return rc;
}
