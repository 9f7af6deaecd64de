// Host build of csrc/t4d_png_huff.h for tests/test_png_ref_host.py: the PNG encoder's length-limited Huffman lengths and canonical
// codes on the CPU.
// stdin: one histogram per line: max_bits (7 or 15), n (1..286), then n frequencies.
// stdout: two lines per histogram: the n code lengths, then the n codes (bit-reversed, as the encoder writes them).
// The ranks by (frequency, symbol) that the kernel computes one symbol per thread are computed here by the same comparison.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../topo4d_amd/csrc/t4d_png_huff.h"

int main()
{
    HuffScratch *hs = new HuffScratch;                               // on the heap: the address sanitizer guards its ends
    int max_bits, n;
    while (scanf("%d %d", &max_bits, &n) == 2) {
        if ((max_bits != 7 && max_bits != 15) || n < 1 || n > kPngLit) return 2;
        std::vector<uint32_t> freq(n);
        for (int s = 0; s < n; ++s)
            if (scanf("%u", &freq[s]) != 1) return 2;
        std::vector<uint8_t> len(n, 0);
        std::vector<uint16_t> code(n, 0);
        hs->count = 0;
        for (int s = 0; s < n; ++s) {
            const uint32_t f = freq[s];
            if (!f) continue;
            int rank = 0;
            for (int u = 0; u < n; ++u) {
                const uint32_t g = freq[u];
                rank += (g && (g < f || (g == f && u < s))) ? 1 : 0;
            }
            hs->sorted[rank] = (uint16_t)s;
            hs->w_leaf[rank] = f;
            hs->count++;
        }
        t4d_png_huff_assign(max_bits, len.data(), *hs);
        t4d_png_canonical_codes(len.data(), n, code.data(), *hs);
        for (int s = 0; s < n; ++s) printf("%d%c", len[s], s + 1 < n ? ' ' : '\n');
        for (int s = 0; s < n; ++s) printf("%d%c", code[s], s + 1 < n ? ' ' : '\n');
    }
    delete hs;
    return 0;
}
