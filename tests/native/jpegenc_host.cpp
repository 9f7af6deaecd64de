// Host build of csrc/t4d_jpeg_fdct.h for tests/test_jpegenc_host.py: the encoder's per-block arithmetic on the CPU.
// stdin: int32 height, width, subsampling, quality (little-endian), then height * width * 3 bytes of RGB.
// stdout: the file header in hex on one line, then one line per block in scan order: component, dummy flag, and the 64 quantised
// coefficients in natural order.  A dummy block (a luma block of the last MCU column or row outside the component's own block grid)
// has zero AC terms and the DC of the block before it in the MCU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../topo4d_amd/csrc/t4d_jpeg_fdct.h"

int main()
{
    int32_t head[4];
    if (fread(head, sizeof(int32_t), 4, stdin) != 4) return 2;
    const int h = head[0], w = head[1], ss = head[2], quality = head[3];
    if (h < 1 || w < 1 || h > 65535 || w > 65535 || ss < 0 || ss > 2) return 2;
    std::vector<uint8_t> img((size_t)h * w * 3);
    if (fread(img.data(), 1, img.size(), stdin) != img.size()) return 2;

    uint8_t header[kJpegEncHeaderBytes];
    t4d_jpeg_header(header, h, w, quality, ss);
    for (int i = 0; i < kJpegEncHeaderBytes; ++i) printf("%02x", header[i]);
    printf("\n");

    uint16_t q[2][64];
    t4d_jpeg_quant_tables(quality, q[0], q[1]);
    const int hs = t4d_jpeg_hs(ss), vs = t4d_jpeg_vs(ss);
    const int mx = (w + 8 * hs - 1) / (8 * hs), my = (h + 8 * vs - 1) / (8 * vs);
    const int yw = (w + 7) / 8, yh = (h + 7) / 8;
    int16_t prev[64], cur[64];
    for (int m = 0; m < mx * my; ++m) {
        const int mcx = m % mx, mcy = m / mx;
        for (int k = 0; k < hs * vs + 2; ++k) {
            const int comp = k < hs * vs ? 0 : k - hs * vs + 1;
            int dummy = 0;
            if (comp == 0) {
                const int bx = mcx * hs + k % hs, by = mcy * vs + k / hs;
                dummy = bx >= yw || by >= yh;
                if (dummy) {
                    memset(cur, 0, sizeof(cur));
                    cur[0] = prev[0];
                } else {
                    t4d_jpeg_block(img.data(), (int64_t)w * 3, w, h, ss, 0, bx, by, q[0], cur);
                }
            } else {
                t4d_jpeg_block(img.data(), (int64_t)w * 3, w, h, ss, comp, mcx, mcy, q[1], cur);
            }
            printf("%d %d", comp, dummy);
            for (int i = 0; i < 64; ++i) printf(" %d", cur[i]);
            printf("\n");
            memcpy(prev, cur, sizeof(cur));
        }
    }
    return 0;
}
