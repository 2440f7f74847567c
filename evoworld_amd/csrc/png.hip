// png.hip -- PNG files encoded on the device (ABI 20, symbols added without a bump): only the compressed stream of a frame leaves the
// GPU.  The lossless sibling of video.hip: 8-bit RGB, colour type 2, no interlace, one IDAT whose zlib stream (78 01) is the frame's
// filtered scanlines cut into segments of whole rows, every segment deflated on its own (no back-reference reaches before its first
// byte) and closed by an empty stored block, so that it ends on a byte -- the pigz construction; the frame's last segment carries
// BFINAL instead.  The Huffman tables are per frame and built on the host between ew_png_lz77 and ew_png_emit (evoworld_amd/png.py;
// DESIGN.md 4.7), from the histograms the parse leaves behind.  Integer code throughout; compiled with -ffp-contract=off like its
// neighbours.
//
//   ew_png_filter   one workgroup per row: the five filter types of RFC 2083 section 6 on 12 bytes (4 pixels) per thread, read as words
//                   where every row starts on a word (3 W % 4 == 0); libpng's minimum sum of absolute differences picks the type, ties
//                   go to the lowest number.  A second kernel, one workgroup per segment, writes the segment's Adler-32 halves.
//   ew_png_lz77     one wave per segment, two per workgroup: the wave clears the segment's hash table and histogram in LDS, lane 0
//                   runs the greedy single-probe parse (png_core.h), the wave writes the histogram out.
//   ew_png_emit     one wave per segment: a coded segment is written by lane 0 through a 64-bit bit buffer with its frame's code table in
//                   LDS, a stored one is copied by the whole wave; both go straight to the segment's final offset.
// No atomics and no data-dependent order: two calls return identical bytes.
#include "common.h"
#define EW_HD __host__ __device__ __forceinline__
#include "png_core.h"

namespace {

constexpr int NT = 256;
constexpr int WAVES = NT / 64;                   // segments per workgroup of the emitter
constexpr int LZ_WAVES = 2;                      // segments per workgroup of the parse: 2 x (16 KiB hash table + histogram) of LDS
constexpr int FILTER_BYTES = 12;                 // per thread and pass: 4 pixels = 3 words

// the segment's place in the filtered rows of its frame
struct SegGeom {
    int H, rows_per_segment, segs_per_frame;
    long long row_bytes;                         // 1 + 3 W
    __host__ __device__ void locate(long long seg, long long& first_byte, long long& n_bytes, bool& last) const {
        const long long v = seg / segs_per_frame;
        const int k = (int)(seg - v * segs_per_frame);
        const int r0 = k * rows_per_segment;
        const int rows = H - r0 < rows_per_segment ? H - r0 : rows_per_segment;
        first_byte = (v * H + r0) * row_bytes;
        n_bytes = rows * row_bytes;
        last = k == segs_per_frame - 1;
    }
};

// ------------------------------------------------------------------------------------------------ filter
// out[0 .. 15] = row[x - 4 .. x + 11], 0 outside [0, n); row == nullptr: the row above the image
template <bool WORDS>
__device__ __forceinline__ void load16(const uint8_t* __restrict__ row, int x, int n, unsigned (&out)[16]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = x - 4 + 4 * k;
        if (WORDS) {                             // x % 4 == 0 and n % 4 == 0: a word lies inside the row or outside it
            const unsigned w = (row && i >= 0 && i < n) ? *reinterpret_cast<const unsigned*>(row + i) : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[4 * k + j] = (w >> (8 * j)) & 255u;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) out[4 * k + j] = (row && i + j >= 0 && i + j < n) ? row[i + j] : 0u;
        }
    }
}

template <bool WORDS>
__global__ __launch_bounds__(NT) void filter_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int mode) {
    __shared__ unsigned s_cost[WAVES][5];
    const int t = threadIdx.x, y = blockIdx.x;
    const long long v = blockIdx.y;
    const int n = 3 * W;
    const uint8_t* cur = src + (v * H + y) * n;
    const uint8_t* up = y > 0 ? cur - n : nullptr;
    uint8_t* out = dst + (v * H + y) * ((long long)n + 1);
    int type = mode;
    if (mode == EW_PNG_FILTER_ADAPTIVE) {
        unsigned cost[5] = {0u, 0u, 0u, 0u, 0u};
        for (int x = t * FILTER_BYTES; x < n; x += NT * FILTER_BYTES) {
            unsigned c16[16], u16[16];
            load16<WORDS>(cur, x, n, c16);
            load16<WORDS>(up, x, n, u16);
#pragma unroll
            for (int j = 0; j < FILTER_BYTES; ++j) {
#pragma unroll
                for (int f = 0; f < 5; ++f)
                    if (x + j < n) cost[f] += png_filter_cost(png_filter_byte(f, (int)c16[4 + j], (int)c16[1 + j], (int)u16[4 + j], (int)u16[1 + j]));
            }
        }
#pragma unroll
        for (int f = 0; f < 5; ++f) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cost[f] += __shfl_xor(cost[f], o, 64);
            if ((t & 63) == 0) s_cost[t >> 6][f] = cost[f];
        }
        __syncthreads();
        unsigned best = 0xFFFFFFFFu;
        type = 0;
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            unsigned c = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) c += s_cost[w][f];
            if (c < best) { best = c; type = f; }                // strict: a tie keeps the lower type
        }
    }
    if (t == 0) out[0] = (uint8_t)type;
    for (int x = t * FILTER_BYTES; x < n; x += NT * FILTER_BYTES) {
        unsigned c16[16], u16[16];
        load16<WORDS>(cur, x, n, c16);
        load16<WORDS>(up, x, n, u16);
#pragma unroll
        for (int j = 0; j < FILTER_BYTES; ++j) {
            if (x + j < n) out[1 + x + j] = (uint8_t)png_filter_byte(type, (int)c16[4 + j], (int)c16[1 + j], (int)u16[4 + j], (int)u16[1 + j]);
        }
    }
}

// Adler-32 of one segment as its halves: a = 1 + sum d[i], b = n + sum (n - i) d[i] (mod 65521)
__global__ __launch_bounds__(NT) void adler_kernel(const uint8_t* __restrict__ filtered, int* __restrict__ adler, SegGeom g) {
    __shared__ unsigned s_a[WAVES], s_b[WAVES];
    const int t = threadIdx.x;
    const long long seg = blockIdx.x;
    long long first, n;
    bool last;
    g.locate(seg, first, n, last);
    const uint8_t* d = filtered + first;
    unsigned long long sa = 0, sb = 0;
    for (long long i = t; i < n; i += NT) {
        const unsigned x = d[i];
        sa += x;
        sb += (unsigned long long)((unsigned)((n - i) % ADLER_MOD)) * x;
    }
    unsigned a = (unsigned)(sa % ADLER_MOD), b = (unsigned)(sb % ADLER_MOD);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if ((t & 63) == 0) { s_a[t >> 6] = a; s_b[t >> 6] = b; }
    __syncthreads();
    if (t == 0) {
        unsigned ta = 1u, tb = (unsigned)(n % ADLER_MOD);
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { ta += s_a[w]; tb += s_b[w]; }
        adler[2 * seg] = (int)(ta % ADLER_MOD);
        adler[2 * seg + 1] = (int)(tb % ADLER_MOD);
    }
}

// ------------------------------------------------------------------------------------------------ LZ77
__global__ __launch_bounds__(64 * LZ_WAVES) void lz77_kernel(const uint8_t* __restrict__ filtered, uint32_t* __restrict__ tokens, int* __restrict__ n_tokens,
                                                  int* __restrict__ hist, long long n_segments, long long token_stride, SegGeom g) {
    __shared__ uint16_t s_tab[LZ_WAVES][PNG_HASH_SIZE];
    __shared__ int s_hist[LZ_WAVES][PNG_NSYM];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long seg = (long long)blockIdx.x * LZ_WAVES + w;
    if (seg >= n_segments) return;               // whole waves leave; nothing below synchronises across waves
    for (int i = lane; i < PNG_HASH_SIZE; i += 64) s_tab[w][i] = 0;
    for (int i = lane; i < PNG_NSYM; i += 64) s_hist[w][i] = 0;
    ew_wave_lds_sync();
    long long first, n;
    bool last;
    g.locate(seg, first, n, last);
    if (lane == 0) n_tokens[seg] = png_lz77_segment(filtered + first, (int)n, tokens + seg * token_stride, s_tab[w], s_hist[w]);
    ew_wave_lds_sync();
    for (int i = lane; i < PNG_NSYM; i += 64) hist[seg * PNG_NSYM + i] = s_hist[w][i];
}

// ------------------------------------------------------------------------------------------------ emit
__global__ __launch_bounds__(NT) void emit_kernel(const uint32_t* __restrict__ tokens, const int* __restrict__ n_tokens,
                                                  const uint8_t* __restrict__ filtered, const int* __restrict__ seg_mode,
                                                  const long long* __restrict__ seg_offsets, const long long* __restrict__ seg_bytes,
                                                  const uint32_t* __restrict__ luts, const uint8_t* __restrict__ headers,
                                                  const int* __restrict__ header_bits, int header_stride, uint8_t* __restrict__ out,
                                                  long long out_bytes, long long n_segments, long long token_stride, SegGeom g) {
    __shared__ uint32_t s_lut[WAVES][PNG_NSYM];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long seg = (long long)blockIdx.x * WAVES + w;
    if (seg >= n_segments) return;
    const long long off = seg_offsets[seg], cap = seg_bytes[seg];
    if (off < 0 || cap < 0 || off > out_bytes || cap > out_bytes - off) return;            // never outside the stream
    long long first, n;
    bool last;
    g.locate(seg, first, n, last);
    const long long v = seg / g.segs_per_frame;
    uint8_t* o = out + off;
    if (seg_mode[seg] == EW_PNG_SEG_STORED) {
        const uint8_t* d = filtered + first;
        const long long blocks = (n + PNG_STORED_MAX - 1) / PNG_STORED_MAX;
        if (png_stored_bytes(n) > cap) return;
        for (long long b = 0; b < blocks; ++b) {
            const long long at = b * PNG_STORED_MAX;
            const unsigned len = (unsigned)(n - at < PNG_STORED_MAX ? n - at : PNG_STORED_MAX);
            uint8_t* ob = o + at + 5 * b;
            if (lane == 0) {
                ob[0] = (uint8_t)((last && b == blocks - 1) ? 1 : 0);
                ob[1] = (uint8_t)(len & 255u);
                ob[2] = (uint8_t)(len >> 8);
                ob[3] = (uint8_t)(~len & 255u);
                ob[4] = (uint8_t)((~len >> 8) & 255u);
            }
            for (unsigned i = lane; i < len; i += 64) ob[5 + i] = d[at + i];
        }
        return;
    }
    for (int i = lane; i < PNG_NSYM; i += 64) s_lut[w][i] = luts[v * PNG_NSYM + i];
    ew_wave_lds_sync();
    if (lane == 0) {
        int nt = n_tokens[seg];
        if (nt < 0) nt = 0;
        if (nt > n) nt = (int)n;                 // the token slot holds n tokens
        int hb = header_bits[v];
        hb = hb < 0 ? 0 : (hb > 8 * header_stride ? 8 * header_stride : hb);               // the header row holds header_stride bytes
        png_emit_coded(tokens + seg * token_stride, nt, s_lut[w], headers + v * header_stride, hb, last, o, cap);
    }
}

inline bool geom_ok(int V, int H, int W, int rows_per_segment) {
    return V >= 1 && V <= 65535 && H >= 1 && H <= 65535 && W >= 1 && W <= 65535 && rows_per_segment >= 1;
}
inline SegGeom make_geom(int H, int W, int rows_per_segment) {
    SegGeom g;
    g.H = H;
    g.rows_per_segment = rows_per_segment < H ? rows_per_segment : H;
    g.segs_per_frame = (H + g.rows_per_segment - 1) / g.rows_per_segment;
    g.row_bytes = 1 + 3LL * W;
    return g;
}

}  // namespace

extern "C" ew_status ew_png_filter(const uint8_t* frames, uint8_t* filtered, int* adler, int V, int H, int W, int filter_mode,
                                   int rows_per_segment, void* stream) {
    EW_REQUIRE(frames && filtered && adler, "ew_png_filter: NULL pointer");
    EW_REQUIRE(geom_ok(V, H, W, rows_per_segment), "ew_png_filter: V = %d, H = %d, W = %d must be 1 .. 65535 and rows_per_segment = %d >= 1", V,
               H, W, rows_per_segment);
    EW_REQUIRE(filter_mode >= 0 && filter_mode <= EW_PNG_FILTER_ADAPTIVE, "ew_png_filter: filter_mode = %d must be 0 .. 4 or EW_PNG_FILTER_ADAPTIVE",
               filter_mode);
    EW_REQUIRE(((uintptr_t)adler & 3) == 0, "ew_png_filter: adler must be 4-byte aligned");
    const SegGeom g = make_geom(H, W, rows_per_segment);
    EW_REQUIRE(g.rows_per_segment * g.row_bytes <= EW_PNG_MAX_SEGMENT_BYTES, "ew_png_filter: a segment of %d rows of %lld bytes exceeds %d bytes",
               g.rows_per_segment, g.row_bytes, EW_PNG_MAX_SEGMENT_BYTES);
    const long long n_segments = (long long)V * g.segs_per_frame;
    EW_REQUIRE(n_segments < (1LL << 31), "ew_png_filter: n_segments = %lld must be below 2^31", n_segments);
    const dim3 grid((unsigned)H, (unsigned)V);
    if (((uintptr_t)frames & 3) == 0 && (3 * W) % 4 == 0)
        hipLaunchKernelGGL(filter_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, frames, filtered, H, W, filter_mode);
    else
        hipLaunchKernelGGL(filter_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, frames, filtered, H, W, filter_mode);
    const ew_status s = ew_check_launch("png filter_kernel");
    if (s != EW_OK) return s;
    hipLaunchKernelGGL(adler_kernel, dim3((unsigned)n_segments), dim3(NT), 0, (hipStream_t)stream, filtered, adler, g);
    return ew_check_launch("png adler_kernel");
}

extern "C" ew_status ew_png_lz77(const uint8_t* filtered, uint32_t* tokens, int* n_tokens, int* hist, int V, int H, int W, int rows_per_segment,
                                 long long token_stride, void* stream) {
    EW_REQUIRE(filtered && tokens && n_tokens && hist, "ew_png_lz77: NULL pointer");
    EW_REQUIRE(geom_ok(V, H, W, rows_per_segment), "ew_png_lz77: V = %d, H = %d, W = %d must be 1 .. 65535 and rows_per_segment = %d >= 1", V, H,
               W, rows_per_segment);
    EW_REQUIRE((((uintptr_t)tokens | (uintptr_t)n_tokens | (uintptr_t)hist) & 3) == 0, "ew_png_lz77: tokens, n_tokens and hist must be 4-byte aligned");
    const SegGeom g = make_geom(H, W, rows_per_segment);
    const long long seg_bytes = g.rows_per_segment * g.row_bytes;
    EW_REQUIRE(seg_bytes <= EW_PNG_MAX_SEGMENT_BYTES, "ew_png_lz77: a segment of %d rows of %lld bytes exceeds %d bytes", g.rows_per_segment,
               g.row_bytes, EW_PNG_MAX_SEGMENT_BYTES);
    EW_REQUIRE(token_stride >= seg_bytes, "ew_png_lz77: token_stride = %lld is below the segment's %lld bytes (one token per byte at worst)",
               token_stride, seg_bytes);
    const long long n_segments = (long long)V * g.segs_per_frame;
    EW_REQUIRE(n_segments < (1LL << 31), "ew_png_lz77: n_segments = %lld must be below 2^31", n_segments);
    hipLaunchKernelGGL(lz77_kernel, dim3((unsigned)((n_segments + LZ_WAVES - 1) / LZ_WAVES)), dim3(64 * LZ_WAVES), 0, (hipStream_t)stream, filtered, tokens,
                       n_tokens, hist, n_segments, token_stride, g);
    return ew_check_launch("png lz77_kernel");
}

extern "C" ew_status ew_png_emit(const uint32_t* tokens, const int* n_tokens, const uint8_t* filtered, const int* seg_mode,
                                 const long long* seg_offsets, const long long* seg_bytes, const uint32_t* luts, const uint8_t* headers,
                                 const int* header_bits, int header_stride, uint8_t* out, long long out_bytes, int V, int H, int W,
                                 int rows_per_segment, long long token_stride, void* stream) {
    EW_REQUIRE(tokens && n_tokens && filtered && seg_mode && seg_offsets && seg_bytes && luts && headers && header_bits && out,
               "ew_png_emit: NULL pointer");
    EW_REQUIRE(geom_ok(V, H, W, rows_per_segment), "ew_png_emit: V = %d, H = %d, W = %d must be 1 .. 65535 and rows_per_segment = %d >= 1", V, H,
               W, rows_per_segment);
    EW_REQUIRE((((uintptr_t)tokens | (uintptr_t)n_tokens | (uintptr_t)seg_mode | (uintptr_t)luts | (uintptr_t)header_bits) & 3) == 0 &&
                   (((uintptr_t)seg_offsets | (uintptr_t)seg_bytes) & 7) == 0,
               "ew_png_emit: the int32 arrays must be 4-byte, seg_offsets and seg_bytes 8-byte aligned");
    EW_REQUIRE(header_stride >= 1 && out_bytes >= 1, "ew_png_emit: header_stride = %d and out_bytes = %lld must be positive", header_stride,
               out_bytes);
    const SegGeom g = make_geom(H, W, rows_per_segment);
    const long long sb = g.rows_per_segment * g.row_bytes;
    EW_REQUIRE(sb <= EW_PNG_MAX_SEGMENT_BYTES, "ew_png_emit: a segment of %d rows of %lld bytes exceeds %d bytes", g.rows_per_segment, g.row_bytes,
               EW_PNG_MAX_SEGMENT_BYTES);
    EW_REQUIRE(token_stride >= sb, "ew_png_emit: token_stride = %lld is below the segment's %lld bytes", token_stride, sb);
    const long long n_segments = (long long)V * g.segs_per_frame;
    EW_REQUIRE(n_segments < (1LL << 31), "ew_png_emit: n_segments = %lld must be below 2^31", n_segments);
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)((n_segments + WAVES - 1) / WAVES)), dim3(NT), 0, (hipStream_t)stream, tokens, n_tokens,
                       filtered, seg_mode, seg_offsets, seg_bytes, luts, headers, header_bits, header_stride, out, out_bytes, n_segments,
                       token_stride, g);
    return ew_check_launch("png emit_kernel");
}
