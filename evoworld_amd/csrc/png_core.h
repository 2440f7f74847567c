// png_core.h -- the serial parts of the PNG encoder (png.hip), one deflate segment each: PNG filter arithmetic, the greedy LZ77 parse
// and the bit writer.  Plain integer C++ without any device intrinsic, marked for host and device, so that the very code the kernels run
// can also be compiled into a host program and inflated by zlib.  RFC 1951 (deflate), RFC 2083 section 6 (filters).
#pragma once
#include <stdint.h>

#ifndef EW_HD
#define EW_HD __host__ __device__ __forceinline__
#endif

constexpr int PNG_HASH_BITS = 13;                // 8192 entries of 16 bits = 16 KiB of LDS per segment in flight
constexpr int PNG_HASH_SIZE = 1 << PNG_HASH_BITS;
constexpr int PNG_NLIT = 286, PNG_NDIST = 30, PNG_NSYM = PNG_NLIT + PNG_NDIST;      // a histogram row: literal/length symbols, distance codes
constexpr int PNG_MAX_MATCH = 258, PNG_MIN_MATCH = 3, PNG_WINDOW = 32768;
constexpr int PNG_STORED_MAX = 65535;
constexpr unsigned ADLER_MOD = 65521u;

// ------------------------------------------------------------------------------------------------ filters
EW_HD int png_paeth(int a, int b, int c) {      // RFC 2083 6.6: ties in the order a, b, c
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// x filtered with type f; a = left, b = above, c = above left (0 outside the image)
EW_HD unsigned png_filter_byte(int f, int x, int a, int b, int c) {
    const int pred = f == 0 ? 0 : f == 1 ? a : f == 2 ? b : f == 3 ? ((a + b) >> 1) : png_paeth(a, b, c);
    return (unsigned)(x - pred) & 255u;
}
EW_HD unsigned png_filter_cost(unsigned v) { return v < 128u ? v : 256u - v; }

// ------------------------------------------------------------------------------------------------ deflate symbols
EW_HD int png_log2(unsigned v) { return 31 - __builtin_clz(v); }                    // v >= 1
// match length 3 .. 258 -> length symbol 257 .. 285, number of extra bits, their value
EW_HD void png_len_symbol(int len, int& sym, int& nextra, unsigned& extra) {
    const unsigned m = (unsigned)(len - PNG_MIN_MATCH);
    if (len == PNG_MAX_MATCH) { sym = 285; nextra = 0; extra = 0; return; }
    if (m < 8u) { sym = 257 + (int)m; nextra = 0; extra = 0; return; }
    const int e = png_log2(m);                                                      // 3 .. 7
    sym = 257 + 4 * (e - 1) + (int)((m >> (e - 2)) & 3u);
    nextra = e - 2;
    extra = m & ((1u << nextra) - 1u);
}
// distance 1 .. 32768 -> distance code 0 .. 29, number of extra bits, their value
EW_HD void png_dist_symbol(int dist, int& sym, int& nextra, unsigned& extra) {
    const unsigned d = (unsigned)(dist - 1);
    if (d < 4u) { sym = (int)d; nextra = 0; extra = 0; return; }
    const int e = png_log2(d);                                                      // 2 .. 14
    sym = 2 * e + (int)((d >> (e - 1)) & 1u);
    nextra = e - 1;
    extra = d & ((1u << nextra) - 1u);
}

// ------------------------------------------------------------------------------------------------ LZ77
EW_HD unsigned png_hash3(const uint8_t* p) {
    const unsigned v = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    return (v * 2654435761u) >> (32 - PNG_HASH_BITS);
}
// Greedy parse of d[0, n) with one probe per position: tab (PNG_HASH_SIZE entries, zeroed by the caller) keeps the low 16 bits of the last
// position of every 3-byte hash; a candidate is rebuilt below pos, refused when it lies before the segment or more than PNG_WINDOW back,
// and believed only as far as its bytes compare equal -- so a stale or never-written entry costs a comparison, nothing else.  Positions
// inside a match are not entered.  tok receives at most n tokens; hist (PNG_NSYM counts, zeroed by the caller) counts every symbol and
// the end-of-block symbol once.  Returns the token count.
EW_HD int png_lz77_segment(const uint8_t* d, int n, uint32_t* tok, uint16_t* tab, int* hist) {
    int pos = 0, nt = 0;
    while (pos < n) {
        int len = 0, dist = 0;
        if (pos + PNG_MIN_MATCH <= n) {
            const unsigned h = png_hash3(d + pos);
            int cand = (pos & ~0xFFFF) | (int)tab[h];
            if (cand >= pos) cand -= 65536;
            tab[h] = (uint16_t)(pos & 0xFFFF);
            if (cand >= 0 && pos - cand <= PNG_WINDOW) {
                const int maxlen = n - pos < PNG_MAX_MATCH ? n - pos : PNG_MAX_MATCH;
                while (len < maxlen && d[cand + len] == d[pos + len]) ++len;
                dist = pos - cand;
            }
        }
        if (len >= PNG_MIN_MATCH) {
            int ls, ds, ne;
            unsigned ex;
            png_len_symbol(len, ls, ne, ex);
            png_dist_symbol(dist, ds, ne, ex);
            ++hist[ls];
            ++hist[PNG_NLIT + ds];
            tok[nt++] = 0x80000000u | (unsigned)(len - PNG_MIN_MATCH) | ((unsigned)(dist - 1) << 8);
            pos += len;
        } else {
            const unsigned lit = d[pos];
            ++hist[lit];
            tok[nt++] = lit;
            ++pos;
        }
    }
    ++hist[256];
    return nt;
}

// ------------------------------------------------------------------------------------------------ bit writer
// LSB-first bit stream into out[0, cap): a byte beyond cap is counted, never stored
struct PngBits {
    uint8_t* out;
    long long cap, at;
    unsigned long long acc;
    int nb;
    EW_HD void put(unsigned v, int len) {       // len <= 16, v < 2^len
        acc |= (unsigned long long)v << nb;
        nb += len;
        while (nb >= 8) {
            if (at < cap) out[at] = (uint8_t)(acc & 255u);
            ++at;
            acc >>= 8;
            nb -= 8;
        }
    }
    EW_HD void align() {                        // zero bits up to the next byte
        if (nb > 0) put(0u, 8 - nb);
    }
};

// One segment as a dynamic-Huffman block.  lut[PNG_NSYM]: bit-reversed code | length << 16 of every literal/length symbol, then of every
// distance code.  hdr: the block header (BFINAL = 0, BTYPE = 10, HLIT .. the coded code lengths), hdr_bits bits, LSB-first.  A frame's
// last segment (final) sets BFINAL and pads with zero bits; every other one is followed by an empty stored block (000, pad, 00 00 FF FF),
// so that the next segment starts on a byte.  Returns the byte count.
EW_HD long long png_emit_coded(const uint32_t* tok, int nt, const uint32_t* lut, const uint8_t* hdr, int hdr_bits, bool final, uint8_t* out,
                               long long cap) {
    PngBits w = {out, cap, 0, 0ull, 0};
    for (int i = 0; i < hdr_bits; i += 8) {
        const int nbits = hdr_bits - i < 8 ? hdr_bits - i : 8;
        unsigned v = hdr[i >> 3] & ((1u << nbits) - 1u);
        if (i == 0 && final) v |= 1u;
        w.put(v, nbits);
    }
    for (int i = 0; i < nt; ++i) {
        const uint32_t t = tok[i];
        if (t & 0x80000000u) {
            int sym, ne;
            unsigned ex;
            png_len_symbol((int)(t & 255u) + PNG_MIN_MATCH, sym, ne, ex);
            uint32_t e = lut[sym];
            w.put(e & 0xFFFFu, (int)(e >> 16));
            if (ne) w.put(ex, ne);
            png_dist_symbol((int)((t >> 8) & 0x7FFFu) + 1, sym, ne, ex);
            e = lut[PNG_NLIT + sym];
            w.put(e & 0xFFFFu, (int)(e >> 16));
            if (ne) w.put(ex, ne);
        } else {
            const uint32_t e = lut[t & 255u];
            w.put(e & 0xFFFFu, (int)(e >> 16));
        }
    }
    w.put(lut[256] & 0xFFFFu, (int)(lut[256] >> 16));
    if (final) {
        w.align();
    } else {
        w.put(0u, 3);
        w.align();
        w.put(0x0000u, 16);
        w.put(0xFFFFu, 16);
    }
    return w.at;
}

// bytes of d[0, n) as stored blocks of at most PNG_STORED_MAX bytes (5 bytes of overhead each)
EW_HD long long png_stored_bytes(long long n) { return n + 5 * ((n + PNG_STORED_MAX - 1) / PNG_STORED_MAX); }
