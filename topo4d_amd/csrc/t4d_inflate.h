// t4d_inflate.h — the inflate core (RFC 1951, zlib's acceptance rules) and the PNG unfilter rule of the PNG decoder, as
// __host__ __device__ code: the same text compiles into the kernels of t4d_pngdec.hip and into tests/native/png_host.cpp.
//
// One decoder, run by W lanes that hold the same state (W = 64: one wave; W = 1: the host).  Every lane decodes every symbol; the
// lanes share the writes: a run of literals is kept one per lane and written W at a time, a match copy is dealt over the lanes
// (out[pos + i] = out[pos - dist + i % dist], so an overlapping copy reads only bytes written before the match).  The Huffman tables
// (canonical counts + symbols, and a 9-bit first-level table for the literal/length code) live in a Tables the caller provides (LDS
// on the device).  The bit reader runs over the payloads of a chunk table, [offset, bytes] pairs into one data buffer, and never
// reads outside them; every write is checked against the caller's capacity.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define T4D_INF_FN __host__ __device__ static inline
#else
#define T4D_INF_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define T4D_INF_FENCE() __threadfence_block()     // one lane's global writes visible to the other lanes of its wave
#define T4D_INF_BARRIER() __syncthreads()         // the workgroup is one wave
#else
#define T4D_INF_FENCE() ((void)0)
#define T4D_INF_BARRIER() ((void)0)
#endif

namespace t4d_inflate {

// status bits (include/topo4d_raster.h, T4D_PNG_ERR_*)
constexpr int kErrEnd = 1;        // the stream ended early, or ran past the capacity
constexpr int kErrBlock = 2;      // bad zlib header, block type 3, or LEN != ~NLEN
constexpr int kErrTable = 4;      // a code table zlib refuses
constexpr int kErrCode = 8;       // an invalid code, or a distance before the start of the output
constexpr int kErrLength = 16;    // inflated length != height * row
constexpr int kErrFilter = 32;    // a filter byte above 4
constexpr int kErrAdler = 64;     // Adler-32 mismatch

constexpr uint32_t kAdlerMod = 65521u;

struct Reader {
    const uint8_t *data;
    const int64_t *chunks;        // [offset, bytes] pairs
    int32_t k, k_end;             // the chunk being read, one past the last
    int64_t pos, end;             // the unread bytes of chunk k
    uint64_t buf;                 // bits not yet taken, LSB first
    int32_t cnt;
    uint64_t cw, nxt;             // the bytes being moved into buf, and the next ones, loaded one word ahead of their use
    int32_t cn, nn;               // how many each holds; nn == 0: the payloads are exhausted
};

// nxt <- the next (up to 8) bytes of the payloads
T4D_INF_FN void fetch(Reader &r)
{
    r.nxt = 0;
    r.nn = 0;
    while (r.pos >= r.end) {
        if (r.k + 1 >= r.k_end) return;
        ++r.k;
        const int64_t o = r.chunks[2 * (int64_t)r.k], n = r.chunks[2 * (int64_t)r.k + 1];
        r.pos = o;
        r.end = n > 0 ? o + n : o;
    }
    const int n = (int)(r.end - r.pos < 8 ? r.end - r.pos : 8);
    uint64_t w = 0;
    for (int i = 0; i < n; ++i) w |= (uint64_t)r.data[r.pos + i] << (8 * i);
    r.pos += n;
    r.nxt = w;
    r.nn = n;
}

T4D_INF_FN Reader reader(const uint8_t *data, const int64_t *chunks, int32_t first, int32_t count)
{
    Reader r;
    r.data = data; r.chunks = chunks;
    r.k = first - 1; r.k_end = first + count;
    r.pos = r.end = 0;
    r.buf = 0; r.cnt = 0;
    r.cw = 0; r.cn = 0;
    fetch(r);
    return r;
}

T4D_INF_FN void refill(Reader &r)
{
    while (r.cnt <= 56) {
        if (r.cn == 0) {
            if (r.nn == 0) return;
            r.cw = r.nxt;
            r.cn = r.nn;
            fetch(r);
        }
        const int t = r.cn < ((64 - r.cnt) >> 3) ? r.cn : ((64 - r.cnt) >> 3);            // >= 1
        const uint64_t m = t == 8 ? ~(uint64_t)0 : (((uint64_t)1 << (8 * t)) - 1);
        r.buf |= (r.cw & m) << r.cnt;
        r.cw = t == 8 ? 0 : r.cw >> (8 * t);
        r.cn -= t;
        r.cnt += 8 * t;
    }
}

T4D_INF_FN bool need(Reader &r, int n)            // n <= 32
{
    if (r.cnt < n) refill(r);
    return r.cnt >= n;
}

T4D_INF_FN uint32_t take(Reader &r, int n)        // after need(r, n)
{
    const uint32_t v = (uint32_t)(r.buf & (((uint64_t)1 << n) - 1));
    r.buf >>= n;
    r.cnt -= n;
    return v;
}

T4D_INF_FN void byte_align(Reader &r)
{
    const int drop = r.cnt & 7;
    r.buf >>= drop;
    r.cnt -= drop;
}

struct Tables {
    uint16_t lcount[16], lsymbol[288];            // literal/length code (and the code-length code while a header is read)
    uint16_t dcount[16], dsymbol[32];             // distance code
    uint16_t fast[512];                           // literal/length: (symbol << 4) | length for codes of <= 9 bits, else 0
    uint16_t offs[16];
    uint8_t lens[320];
    int32_t fixed;                                // the tables hold the fixed codes
};

// canonical code of lens[0..n): 0 complete, < 0 over-subscribed, > 0 incomplete (the unused part of the code space)
T4D_INF_FN int construct(uint16_t *count, uint16_t *symbol, uint16_t *offs, const uint8_t *lens, int n)
{
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) count[lens[s]]++;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; ++s)
        if (lens[s]) symbol[offs[lens[s]]++] = (uint16_t)s;
    return left;
}

// the next symbol of a canonical code: >= 0, -1 no such code, -2 out of data
T4D_INF_FN int decode_slow(Reader &r, const uint16_t *count, const uint16_t *symbol)
{
    if (r.cnt < 15) refill(r);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        if (l > r.cnt) return -2;
        code |= (int)((r.buf >> (l - 1)) & 1);
        const int c = count[l];
        if (code - c < first) {
            r.buf >>= l;
            r.cnt -= l;
            return symbol[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

T4D_INF_FN int decode_lit(Reader &r, const Tables &T)
{
    if (r.cnt < 15) refill(r);
    const uint32_t e = T.fast[r.buf & 511];
    const int l = (int)(e & 15);
    if (e && l <= r.cnt) {
        r.buf >>= l;
        r.cnt -= l;
        return (int)(e >> 4);
    }
    return decode_slow(r, T.lcount, T.lsymbol);
}

template <int W>
T4D_INF_FN void build_fast(Tables &T, int lane)
{
    for (int i = lane; i < 512; i += W) {
        int code = 0, first = 0, index = 0;
        uint32_t e = 0;
        for (int l = 1; l <= 9; ++l) {
            code |= (i >> (l - 1)) & 1;
            const int c = T.lcount[l];
            if (code - c < first) {
                e = ((uint32_t)T.lsymbol[index + (code - first)] << 4) | (uint32_t)l;
                break;
            }
            index += c;
            first += c;
            first <<= 1;
            code <<= 1;
        }
        T.fast[i] = (uint16_t)e;
    }
}

T4D_INF_FN int len_extra(int s) { return s < 8 || s == 28 ? 0 : (s >> 2) - 1; }                 // s = symbol - 257, 0..28
T4D_INF_FN int len_base(int s) { return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s >> 2) - 1)); }
T4D_INF_FN int dist_extra(int d) { return d < 4 ? 0 : (d >> 1) - 1; }                           // d = 0..29
T4D_INF_FN int dist_base(int d) { return d < 4 ? 1 + d : 1 + ((2 + (d & 1)) << ((d >> 1) - 1)); }

// the literal/length and distance codes of a dynamic block's header: 0 or status bits.  zlib's rules: at most 286 / 30 codes; the
// code-length code complete; no repeat without a previous length or past the end; symbol 256 present; neither code over-subscribed,
// and incomplete only as a single code of length 1.
template <int W>
T4D_INF_FN int dynamic_tables(Reader &r, Tables &T, int lane)
{
    if (!need(r, 14)) return kErrEnd;
    const int nlen = (int)take(r, 5) + 257, ndist = (int)take(r, 5) + 1, ncode = (int)take(r, 4) + 4;
    if (nlen > 286 || ndist > 30) return kErrTable;
    const char *order = "\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f";
    T4D_INF_BARRIER();                                               // nobody still decodes with the previous block's tables
    for (int i = 0; i < 19; ++i) {
        uint32_t v = 0;
        if (i < ncode) {
            if (!need(r, 3)) return kErrEnd;
            v = take(r, 3);
        }
        if (lane == 0) T.lens[(int)order[i]] = (uint8_t)v;
    }
    T4D_INF_BARRIER();
    if (lane == 0) {
        const int left = construct(T.lcount, T.lsymbol, T.offs, T.lens, 19);
        T.fixed = (left != 0 || T.lcount[0] == 19) ? -1 : 0;
    }
    T4D_INF_BARRIER();
    if (T.fixed < 0) return kErrTable;
    int index = 0, prev = 0;
    while (index < nlen + ndist) {
        const int sym = decode_slow(r, T.lcount, T.lsymbol);
        if (sym < 0) return sym == -2 ? kErrEnd : kErrCode;
        int rep = 1, val = sym;
        if (sym >= 16) {
            const int eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
            if (sym == 16 && index == 0) return kErrTable;
            if (!need(r, eb)) return kErrEnd;
            rep = (sym == 18 ? 11 : 3) + (int)take(r, eb);
            val = sym == 16 ? prev : 0;
            if (index + rep > nlen + ndist) return kErrTable;
        }
        if (lane == 0)
            for (int j = 0; j < rep; ++j) T.lens[index + j] = (uint8_t)val;
        index += rep;
        prev = val;
    }
    T4D_INF_BARRIER();
    if (lane == 0) {
        int bad = T.lens[256] == 0;
        int left = construct(T.lcount, T.lsymbol, T.offs, T.lens, nlen);
        if (left < 0 || (left > 0 && nlen != T.lcount[0] + T.lcount[1])) bad = 1;
        left = construct(T.dcount, T.dsymbol, T.offs, T.lens + nlen, ndist);
        if (left < 0 || (left > 0 && ndist != T.dcount[0] + T.dcount[1])) bad = 1;
        T.fixed = bad ? -1 : 0;
    }
    T4D_INF_BARRIER();
    if (T.fixed < 0) return kErrTable;
    build_fast<W>(T, lane);
    T4D_INF_BARRIER();
    return 0;
}

template <int W>
T4D_INF_FN void fixed_tables(Tables &T, int lane)
{
    T4D_INF_BARRIER();
    if (T.fixed == 1) return;
    for (int s = lane; s < 320; s += W) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    T4D_INF_BARRIER();
    if (lane == 0) {
        construct(T.lcount, T.lsymbol, T.offs, T.lens, 288);         // symbols 286, 287 and distance codes 30, 31 take their part
        construct(T.dcount, T.dsymbol, T.offs, T.lens + 288, 32);    // of the code space and are refused when they are met
        T.fixed = 1;
    }
    T4D_INF_BARRIER();
    build_fast<W>(T, lane);
    T4D_INF_BARRIER();
}

// Inflate blocks from r into out[0, cap) (WRITE false: count only, out is not touched).  *produced receives the bytes made.
//  * as_chunk false: up to the end of the block with BFINAL set.  Returns 0 or status bits.
//  * as_chunk true: r is one IDAT payload decoded as if it began at a block boundary with no history.  Returns 0 when the chunk
//    verifies - whole blocks, every byte consumed, the end byte-aligned after a block end (padding bits only after the final
//    block), no distance before its own first byte, BFINAL in its last block exactly when want_final - and non-zero otherwise.
// T must start with fixed = 0.  The state is the same in every lane; lane and W only deal the writes.
template <bool WRITE, int W>
T4D_INF_FN int inflate(Reader &r, Tables &T, uint8_t *out, int64_t cap, int lane, bool as_chunk, bool want_final, int64_t *produced)
{
    int64_t pos = 0;
    int nlit = 0, err = 0;
    uint32_t lit = 0;
    auto flush = [&]() {
        if (WRITE && lane < nlit) out[pos - nlit + lane] = (uint8_t)lit;
        nlit = 0;
    };
    auto literal = [&](uint32_t b) -> bool {
        if (pos >= cap) return false;
        if (lane == nlit) lit = b;
        ++nlit;
        ++pos;
        if (nlit == W) flush();
        return true;
    };
    for (;;) {
        if (!need(r, 3)) { err = kErrEnd; break; }
        const int final = (int)take(r, 1), type = (int)take(r, 2);
        if (type == 0) {
            byte_align(r);
            if (!need(r, 32)) { err = kErrEnd; break; }
            const uint32_t len = take(r, 16), nlen = take(r, 16);
            if (len != (nlen ^ 0xFFFFu)) { err = kErrBlock; break; }
            for (uint32_t i = 0; i < len && !err; ++i) {
                if (!need(r, 8) || !literal(take(r, 8))) err = kErrEnd;
            }
        } else if (type == 3) {
            err = kErrBlock;
        } else {
            if (type == 1) fixed_tables<W>(T, lane);
            else err = dynamic_tables<W>(r, T, lane);
            while (!err) {
                const int sym = decode_lit(r, T);
                if (sym < 0) { err = sym == -2 ? kErrEnd : kErrCode; break; }
                if (sym < 256) {
                    if (!literal((uint32_t)sym)) err = kErrEnd;
                    continue;
                }
                if (sym == 256) break;
                const int s = sym - 257;
                if (s >= 29) { err = kErrCode; break; }
                int eb = len_extra(s);
                if (!need(r, eb)) { err = kErrEnd; break; }
                const int len = len_base(s) + (int)take(r, eb);
                const int d = decode_slow(r, T.dcount, T.dsymbol);
                if (d < 0) { err = d == -2 ? kErrEnd : kErrCode; break; }
                if (d >= 30) { err = kErrCode; break; }
                eb = dist_extra(d);
                if (!need(r, eb)) { err = kErrEnd; break; }
                const int64_t dist = dist_base(d) + (int64_t)take(r, eb);
                if (dist > pos) { err = kErrCode; break; }
                if (pos + len > cap) { err = kErrEnd; break; }
                if (WRITE) {
                    flush();
                    T4D_INF_FENCE();
                    const uint8_t *src = out + (pos - dist);
                    for (int i = lane; i < len; i += W) out[pos + i] = src[i < dist ? i : i % (int)dist];
                }
                pos += len;
            }
        }
        if (err) break;
        if (final) {
            if (as_chunk) {
                byte_align(r);
                refill(r);
                if (!want_final || r.cnt != 0) err = kErrBlock;
            }
            break;
        }
        if (as_chunk) {
            refill(r);
            if (r.cnt == 0) {                                        // the payload ends here, on a byte boundary
                if (want_final) err = kErrBlock;
                break;
            }
        }
    }
    flush();
    T4D_INF_FENCE();
    *produced = pos;
    return err;
}

// zlib header (CMF, FLG): deflate, window <= 32 KiB, check bits, no preset dictionary
T4D_INF_FN bool zlib_header_ok(uint32_t cmf, uint32_t flg)
{
    return (cmf & 15) == 8 && (cmf >> 4) <= 7 && ((cmf << 8) | flg) % 31 == 0 && !(flg & 0x20);
}

// How a payload at bytes [soff, soff + bytes) of a zlib stream of `total` bytes takes part in the chunk-parallel schedule:
// 0 empty, 1 deflate data only, 2 header or trailer bytes only, 3 mixed (the schedule does not apply)
T4D_INF_FN int chunk_class(int64_t soff, int64_t bytes, int64_t total)
{
    if (bytes <= 0) return 0;
    const int64_t e = soff + bytes;
    if (e <= 2 || soff >= total - 4) return 2;
    if (soff >= 2 && e <= total - 4) return 1;
    return 3;
}

// ---- unfilter (PNG specification, 9.2): arithmetic mod 256 at a byte distance of bytes per pixel ---------------------------------
T4D_INF_FN uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int p = (int)a + (int)b - (int)c;
    const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p,
              pc = p > (int)c ? p - (int)c : (int)c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);          // ties in the order a, b, c
}

// the reconstructed byte: ft 0..4; a left, b above, c above left (0 outside the image)
T4D_INF_FN uint32_t unfilter_byte(int ft, uint32_t raw, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t pred = ft == 0 ? 0u : ft == 1 ? a : ft == 2 ? b : ft == 3 ? ((a + b) >> 1) : paeth(a, b, c);
    return (raw + pred) & 0xFFu;
}

}  // namespace t4d_inflate
