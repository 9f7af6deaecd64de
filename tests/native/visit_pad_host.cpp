// Host build of csrc/t4d_raster_visit_pad.h for the CPU tests: a wave's four visit lists, prefilled with the null entry by the
// wave-wide stores the render kernels issue and then built, against the old formulation - built first, then padded row by row
// with the null entry up to (and GROUP - 1 entries beyond) the wave's longest list.  Every (list length, longest list) pair up to
// 200 entries, for every list block the kernels instantiate.  The block is a heap allocation of exactly its size: built with the
// address sanitizer, a store outside it is an error.  Prints "ok <checks>" and exits 0, or prints the first failure and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../topo4d_amd/csrc/t4d_raster_visit_pad.h"

static unsigned long long g_checks = 0;

// the kernels' prefill, lane by lane: VEC bytes of the null entry at every offset the schedule names
template <int BYTES, int VEC>
static void prefill(unsigned char *block, const uint16_t null_entry)
{
    unsigned char val[VEC];
    for (int i = 0; i < VEC; i += 2) memcpy(val + i, &null_entry, 2);
    for (int k = 0; k < visit_prefill_stores<BYTES, VEC>(); k++)
        for (int lane = 0; lane < 64; lane++) {
            int off = 0;
            if (visit_prefill_store<BYTES, VEC>(k, lane, off)) memcpy(block + off, val, VEC);
        }
}

// pad_visit_list as the kernels ran it: lane by lane, 64 entries a trip
static void pad_old(uint16_t *list, const int cnt, const int nsteps, const int group, const uint16_t null_entry)
{
    for (int lane = 0; lane < 64; lane++)
        for (int p = cnt + lane; p < nsteps + group - 1; p += 64) list[p] = null_entry;
}

template <int STRIDE, int VEC, int GROUP, int MAXLEN>
static int check_block(const char *what)
{
    constexpr int kBytes = 4 * STRIDE * 2;
    static_assert(MAXLEN + GROUP - 1 <= STRIDE, "a full list and its padding fit a row");
    const uint16_t nul = 0xbeef, stale = 0x7777;
    std::vector<unsigned char> now(kBytes), old(kBytes);          // exactly the block: the sanitizer sees a store beyond it
    for (int nsteps = 0; nsteps <= MAXLEN && nsteps <= 200; nsteps++)
        for (int cnt = 0; cnt <= nsteps; cnt++)
            for (int row = 0; row < 4; row++) {
                // row `row` holds cnt entries, the row after it the longest list, the others something in between
                int cnts[4];
                for (int r = 0; r < 4; r++) cnts[r] = r == row ? cnt : (r == ((row + 1) & 3) ? nsteps : (cnt + nsteps) / 2);
                for (int i = 0; i < kBytes; i += 2) { memcpy(&now[i], &stale, 2); memcpy(&old[i], &stale, 2); }
                uint16_t *ln = reinterpret_cast<uint16_t *>(now.data()), *lo = reinterpret_cast<uint16_t *>(old.data());
                prefill<kBytes, VEC>(now.data(), nul);
                for (int r = 0; r < 4; r++)
                    for (int i = 0; i < cnts[r]; i++) ln[r * STRIDE + i] = lo[r * STRIDE + i] = (uint16_t)(40 * ((r * 131 + i * 7) % 129));
                for (int r = 0; r < 4; r++) pad_old(lo + r * STRIDE, cnts[r], nsteps, GROUP, nul);
                for (int r = 0; r < 4; r++) {
                    // what a walk reads: nsteps entries rounded up to a group, and (the backward) one group fetched ahead of it
                    for (int i = 0; i < nsteps + GROUP - 1; i++) {
                        g_checks++;
                        if (ln[r * STRIDE + i] != lo[r * STRIDE + i]) {
                            printf("FAIL %s: nsteps=%d row=%d cnt=%d entry %d: %04x, was %04x\n", what, nsteps, r, cnts[r], i,
                                   ln[r * STRIDE + i], lo[r * STRIDE + i]);
                            return 1;
                        }
                    }
                    // and nothing stale anywhere behind the entries
                    for (int i = cnts[r]; i < STRIDE; i++) {
                        g_checks++;
                        if (ln[r * STRIDE + i] != nul) {
                            printf("FAIL %s: nsteps=%d row=%d cnt=%d entry %d is not null: %04x\n", what, nsteps, r, cnts[r], i, ln[r * STRIDE + i]);
                            return 1;
                        }
                    }
                }
            }
    return 0;
}

int main()
{
    // backward: kBwdBatch + 4 entries a row, 8-byte stores (the block sits 8 bytes off a 16-byte boundary), groups of four
    if (check_block<128 + 4, 8, 4, 128>("backward, 128 per batch")) return 1;
    if (check_block<64 + 4, 8, 4, 64>("backward, segments of 64")) return 1;
    // forward: kSub + 8 entries a row, 16-byte stores; groups of four (throughput) or eight (latency)
    if (check_block<192 + 8, 16, 4, 192>("forward, 192 per batch")) return 1;
    if (check_block<256 + 8, 16, 4, 256>("forward, 256 per batch")) return 1;
    if (check_block<256 + 8, 16, 8, 256>("forward, latency build")) return 1;
    if (check_block<128 + 8, 16, 4, 128>("forward, segments of 128")) return 1;
    if (check_block<128 + 8, 16, 8, 128>("forward, latency build, segments of 128")) return 1;
    if (check_block<64 + 8, 16, 4, 64>("forward, segments of 64 (less than one store)")) return 1;
    if (check_block<64 + 8, 16, 8, 64>("forward, latency build, segments of 64")) return 1;
    printf("ok %llu\n", g_checks);
    return 0;
}
