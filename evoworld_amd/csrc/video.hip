// video.hip -- Motion-JPEG frames encoded on the device (ABI 19, symbols added without a bump): only the compressed scan of a clip
// leaves the GPU.  Reference: Navigator.save_video / save_gif (evoworld/inference/navigator_evoworld.py:233-274, imageio -> ffmpeg) and
// the navigated.mp4 / original.mp4 that calculate_scores.py loads; no H.264 encoder exists here, so the frames are baseline JPEG
// (ITU-T T.81) in an AVI written by evoworld_amd/video.py.  Compiled with -ffp-contract=off: every product and sum below is one
// float32 rounding, except the DCT's dot products, which are explicit fmaf chains (one rounding per term).
//
// The stream: SOF0, 8 bit, YCbCr full range (JFIF), 4:2:0 (MCU 16x16 = Y00 Y01 Y10 Y11 Cb Cr) or 4:4:4 (MCU 8x8 =
// Y Cb Cr), the four Annex K Huffman tables, Annex K quantisation tables under libjpeg's quality rule, restart interval = one MCU row.
//
//   ew_jpeg_dct_quant  one workgroup = 128 pixels of one MCU row of one frame (48 blocks under either sampling): RGB -> YCbCr (the
//                      2x2 chroma mean for 4:2:0) into LDS, partial MCUs filled by replicating the last column / row; 8-point
//                      orthonormal DCT-II along the rows, then along the columns, in place; quotient c / t (IEEE division) rounded
//                      half to even, clamped (AC +-1023, DC [-1024, 1023]), written in zigzag order as 16-byte vectors.
//   ew_jpeg_entropy    one workgroup per restart segment (one MCU row of one frame), 256 blocks per round, one lane per block: DC
//                      difference against the previous block of the component inside the segment, run / category codes with ZRL and
//                      EOB, the block's bit length; a prefix sum places the bit strings in an LDS bit buffer (atomic or on LDS words);
//                      a second prefix sum over the 0xFF bytes places the stuffed bytes; a partial byte is carried into the next
//                      round, the segment's tail is padded with 1-bits.  Slots are sized by the provable worst case: 26 bits per
//                      coefficient (a 16-bit code + 10 value bits), doubled by stuffing = 416 bytes per block.
//   ew_jpeg_pack       the segments of all frames -> one contiguous stream, RSTm (m = row mod 8) behind every row but a frame's last;
//                      the offsets are the caller's scan of the byte counts.
// No global atomics and no data-dependent order: two calls return identical bytes.
#include "common.h"
#include "jpeg_tables.h"

namespace {

constexpr int NT = 256;
constexpr int TILE_W = 128;                      // pixels per workgroup of the DCT kernel: 8 MCUs (4:2:0) or 16 MCUs (4:4:4)
constexpr int TILE_BLOCKS = 48;                  // 8 x 6 = 16 x 3
constexpr int BLK_LD = 9;                        // LDS row stride of a block (8 + 1: rows and columns both walk conflict-free)
constexpr int BLK_SZ = 8 * BLK_LD;
constexpr int BLOCK_MAX_BYTES = 64 * 26 / 8;     // 208: unstuffed worst case of one block
constexpr int ENT_BLOCKS = NT;                   // blocks per round of the entropy kernel
constexpr int ENT_WORDS = ENT_BLOCKS * BLOCK_MAX_BYTES / 4 + 4;   // + the carried partial byte and the word a code may spill into

struct QuantTables { unsigned char q[2][64]; };  // natural (row-major) order; [0] luminance, [1] chrominance

// Annex K.1 / K.2, natural order
const unsigned char K1_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                   69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                   81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72,  92,  95,  98,  112, 100, 103, 99};
const unsigned char K2_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                     99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// libjpeg's jpeg_quality_scaling + jpeg_add_quant_table (baseline: entries clamped to 1..255)
QuantTables quant_tables(int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    QuantTables t;
    for (int i = 0; i < 64; ++i) {
        const int base[2] = {K1_LUMA[i], K2_CHROMA[i]};
        for (int c = 0; c < 2; ++c) {
            int v = (base[c] * scale + 50) / 100;
            t.q[c][i] = (unsigned char)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    }
    return t;
}

// ------------------------------------------------------------------------------------------------ DCT + quantisation
// p[0], p[stride], ... p[7 * stride] <- their DCT
__device__ __forceinline__ void dct8(float* p, int stride) {
    float x[8], y[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = p[n * stride];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        float a = dct_m(k, 0) * x[0];
#pragma unroll
        for (int n = 1; n < 8; ++n) a = fmaf(dct_m(k, n), x[n], a);
        y[k] = a;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k * stride] = y[k];
}

__device__ __forceinline__ void to_ycc(const uint8_t* __restrict__ p, float& y, float& cb, float& cr) {
    const float r = (float)p[0], g = (float)p[1], b = (float)p[2];
    y = 0.299f * r + 0.587f * g + 0.114f * b - 128.0f;
    cb = -0.168735892f * r - 0.331264108f * g + 0.5f * b;
    cr = 0.5f * r - 0.418687589f * g - 0.081312411f * b;
}

template <bool SUB420>
__global__ __launch_bounds__(NT) void dct_quant_kernel(const uint8_t* __restrict__ src, short* __restrict__ coef, int H, int W, int mr, int mc,
                                                       int xtiles, QuantTables qt) {
    constexpr int BPM = SUB420 ? 6 : 3;                  // blocks per MCU
    constexpr int MPT = TILE_BLOCKS / BPM;               // MCUs per tile
    __shared__ float s_blk[TILE_BLOCKS * BLK_SZ];
    __shared__ float s_q[2][64];                         // divisors in zigzag order
    const int t = threadIdx.x;
    const int xt = (int)(blockIdx.x % (unsigned)xtiles), my = (int)(blockIdx.x / (unsigned)xtiles), v = blockIdx.y;
    if (t < 128) s_q[t >> 6][t & 63] = (float)qt.q[t >> 6][d_zigzag[t & 63]];
    const uint8_t* fr = src + (long long)v * H * W * 3;
    const int x0 = xt * TILE_W;
    if (SUB420) {
        const int y0 = my * 16;
        for (int q = t; q < 8 * 64; q += NT) {           // one 2x2 quad = one chroma sample
            const int cy = q >> 6, cx = q & 63;
            float sb = 0.0f, sr = 0.0f;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int ty = 2 * cy + (d >> 1), tx = 2 * cx + (d & 1);
                const int gy = min(y0 + ty, H - 1), gx = min(x0 + tx, W - 1);
                float y, cb, cr;
                to_ycc(fr + ((long long)gy * W + gx) * 3, y, cb, cr);
                s_blk[((tx >> 4) * 6 + (ty >> 3) * 2 + ((tx >> 3) & 1)) * BLK_SZ + (ty & 7) * BLK_LD + (tx & 7)] = y;
                sb += cb;
                sr += cr;
            }
            const int at = ((cx >> 3) * 6 + 4) * BLK_SZ + cy * BLK_LD + (cx & 7);
            s_blk[at] = sb * 0.25f;
            s_blk[at + BLK_SZ] = sr * 0.25f;
        }
    } else {
        const int y0 = my * 8;
        for (int q = t; q < 8 * TILE_W; q += NT) {
            const int ty = q >> 7, tx = q & 127;
            const int gy = min(y0 + ty, H - 1), gx = min(x0 + tx, W - 1);
            float y, cb, cr;
            to_ycc(fr + ((long long)gy * W + gx) * 3, y, cb, cr);
            const int at = (tx >> 3) * 3 * BLK_SZ + ty * BLK_LD + (tx & 7);
            s_blk[at] = y;
            s_blk[at + BLK_SZ] = cb;
            s_blk[at + 2 * BLK_SZ] = cr;
        }
    }
    __syncthreads();
    for (int i = t; i < TILE_BLOCKS * 8; i += NT) dct8(s_blk + (i >> 3) * BLK_SZ + (i & 7) * BLK_LD, 1);          // rows
    __syncthreads();
    for (int i = t; i < TILE_BLOCKS * 8; i += NT) dct8(s_blk + (i >> 3) * BLK_SZ + (i & 7), BLK_LD);              // columns
    __syncthreads();
    for (int i = t; i < TILE_BLOCKS * 8; i += NT) {      // 8 consecutive zigzag positions of one block = one 16-byte store
        const int b = i >> 3, g = i & 7;
        const int m = b / BPM, j = b - m * BPM;
        const int mx = xt * MPT + m;
        if (mx >= mc) continue;
        const int tab = SUB420 ? (j >= 4) : (j > 0);
        const float* blk = s_blk + b * BLK_SZ;
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = g * 8 + e;
            const int nat = d_zigzag[k];
            float qv = rintf(__fdiv_rn(blk[(nat >> 3) * BLK_LD + (nat & 7)], s_q[tab][k]));       // round half to even
            qv = fminf(fmaxf(qv, k == 0 ? -1024.0f : -1023.0f), 1023.0f);
            const unsigned u = (unsigned)(int)qv & 0xffffu;
            if (e & 1) w[e >> 1] |= u << 16;
            else w[e >> 1] = u;
        }
        const long long at = ((((long long)v * mr + my) * mc + mx) * BPM + j) * 64 + g * 8;
        *reinterpret_cast<uint4*>(coef + at) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ------------------------------------------------------------------------------------------------ entropy coding
// Annex K.3.3 (tables K.3 - K.6): the number of codes of each length 1 .. 16, then the symbols in code order
struct HuffSpec {
    unsigned char bits[16];
    unsigned char vals[162];
};
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// symbol -> code << 5 | length (T.81 annex C); a symbol the table does not hold stays 0 and is never looked up (values are clamped)
struct HuffLut {
    unsigned ac[2][256];
    unsigned dc[2][16];
};
constexpr void fill_lut(unsigned* lut, const HuffSpec& s) {
    unsigned code = 0;
    int at = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) lut[s.vals[at++]] = (code++ << 5) | (unsigned)len;
        code <<= 1;
    }
}
constexpr HuffLut make_lut() {
    HuffLut l{};
    fill_lut(l.ac[0], AC_LUMA);
    fill_lut(l.ac[1], AC_CHROMA);
    fill_lut(l.dc[0], DC_LUMA);
    fill_lut(l.dc[1], DC_CHROMA);
    return l;
}
constexpr HuffLut H_LUT = make_lut();
__device__ __constant__ HuffLut d_lut = H_LUT;

// exclusive prefix of v over the block's 256 threads; total = the sum.  s_w: 4 words.
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* s_w, unsigned& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();                                     // the previous scan's readers are done with s_w
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    unsigned base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        if (i < w) base += s_w[i];
        total += s_w[i];
    }
    return base + inc - v;
}

// `len` (<= 26) bits of val at bit position pos of the buffer: bit p is bit 31 - p % 32 of word p / 32
__device__ __forceinline__ void put_bits(unsigned* buf, unsigned pos, unsigned val, unsigned len) {
    const unsigned long long v = (unsigned long long)val << (64 - (pos & 31) - len);
    const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)v;
    atomicOr(&buf[pos >> 5], hi);
    if (lo) atomicOr(&buf[(pos >> 5) + 1], lo);
}

__device__ __forceinline__ unsigned buf_byte(const unsigned* buf, unsigned i) { return (buf[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }

// one symbol: Huffman code of (run, size) followed by the size low bits of the value (v - 1 for a negative one)
template <bool EMIT>
__device__ __forceinline__ void symbol(unsigned entry, int value, unsigned size, unsigned* buf, unsigned& pos) {
    const unsigned len = (entry & 31u) + size;
    if (EMIT) {
        const unsigned extra = (unsigned)(value < 0 ? value - 1 : value) & ((1u << size) - 1u);
        put_bits(buf, pos, ((entry >> 5) << size) | extra, len);
    }
    pos += len;
}

// the bits of one block from position pos on; returns the position behind them.  Values are clamped to what the tables hold (DC
// difference +-2047, AC +-1023), so that no input makes a block longer than BLOCK_MAX_BYTES.
template <bool EMIT>
__device__ __forceinline__ unsigned code_block(const short* __restrict__ blk, int dc_pred, const unsigned* s_dc, const unsigned* s_ac,
                                               unsigned* buf, unsigned pos) {
    int run = 0;
#pragma unroll 1
    for (int g = 0; g < 8; ++g) {
        const uint4 raw = *reinterpret_cast<const uint4*>(blk + g * 8);
        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            int c = (int)(short)(w[e >> 1] >> (16 * (e & 1)));
            if (g == 0 && e == 0) {
                c = min(max(c - dc_pred, -2047), 2047);
                const unsigned size = 32 - __clz(abs(c));        // __clz(0) = 32
                symbol<EMIT>(s_dc[size], c, size, buf, pos);
            } else if (c == 0) {
                ++run;
            } else {
                c = min(max(c, -1023), 1023);
                while (run > 15) {
                    symbol<EMIT>(s_ac[0xF0], 0, 0, buf, pos);     // ZRL
                    run -= 16;
                }
                const unsigned size = 32 - __clz(abs(c));
                symbol<EMIT>(s_ac[(run << 4) | size], c, size, buf, pos);
                run = 0;
            }
        }
    }
    if (run > 0) symbol<EMIT>(s_ac[0], 0, 0, buf, pos);           // EOB
    return pos;
}

template <bool SUB420>
__global__ __launch_bounds__(NT) void entropy_kernel(const short* __restrict__ coef, uint8_t* __restrict__ slots, int* __restrict__ seg_bytes,
                                                     int nb, size_t slot_bytes) {
    constexpr int BPM = SUB420 ? 6 : 3;
    __shared__ unsigned s_buf[ENT_WORDS];
    __shared__ unsigned s_ac[2][256], s_dc[2][16];
    __shared__ unsigned s_w[NT / 64];
    const int t = threadIdx.x;
    for (int i = t; i < 512; i += NT) s_ac[i >> 8][i & 255] = d_lut.ac[i >> 8][i & 255];
    if (t < 32) s_dc[t >> 4][t & 15] = d_lut.dc[t >> 4][t & 15];
    const long long seg = blockIdx.x;
    const short* sc = coef + seg * nb * 64;
    uint8_t* out = slots + (size_t)seg * slot_bytes;
    unsigned carry_bits = 0, carry_val = 0;              // the bits of the last round's partial byte, in the byte's high bits
    size_t out_pos = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += ENT_BLOCKS) {
        const int b = b0 + t;
        const bool have = b < nb, last = b0 + ENT_BLOCKS >= nb;
        int pred = 0, tab = 0;
        if (have) {
            const int j = b % BPM;                       // the previous block of the same component inside the segment
            int pb;
            if (SUB420) {
                tab = j >= 4;
                pb = (j >= 1 && j <= 3) ? b - 1 : (j == 0 ? b - 3 : b - 6);
            } else {
                tab = j > 0;
                pb = b - 3;
            }
            if (pb >= 0) pred = sc[(long long)pb * 64];
        }
        const unsigned mine = have ? code_block<false>(sc + (long long)b * 64, pred, s_dc[tab], s_ac[tab], nullptr, 0) : 0;
        unsigned sum;
        const unsigned at = carry_bits + block_scan(mine, s_w, sum);
        const unsigned T = carry_bits + sum;
        for (unsigned i = t; i < (T + 31) / 32 + 1; i += NT) s_buf[i] = 0;
        __syncthreads();
        if (t == 0 && carry_bits) atomicOr(&s_buf[0], carry_val << 24);
        if (have) code_block<true>(sc + (long long)b * 64, pred, s_dc[tab], s_ac[tab], s_buf, at);
        __syncthreads();
        unsigned nbytes = T >> 3;
        if (last && (T & 7)) {                           // pad the segment's last byte with 1-bits
            if (t == 0) put_bits(s_buf, T, (1u << (8 - (T & 7))) - 1u, 8 - (T & 7));
            ++nbytes;
            __syncthreads();
        }
        // byte stuffing: thread t owns bytes [lo, hi); a 0x00 follows every 0xFF
        const unsigned per = (nbytes + NT - 1) / NT;
        const unsigned lo = min((unsigned)t * per, nbytes), hi = min(lo + per, nbytes);
        unsigned ff = 0;
        for (unsigned i = lo; i < hi; ++i) ff += buf_byte(s_buf, i) == 255u;
        unsigned ff_all;
        size_t o = out_pos + lo + block_scan(ff, s_w, ff_all);
        for (unsigned i = lo; i < hi; ++i) {
            const unsigned v = buf_byte(s_buf, i);
            if (o < slot_bytes) out[o] = (uint8_t)v;
            ++o;
            if (v == 255u) {
                if (o < slot_bytes) out[o] = 0;
                ++o;
            }
        }
        out_pos += nbytes + ff_all;
        carry_bits = last ? 0 : (T & 7);
        carry_val = carry_bits ? (buf_byte(s_buf, nbytes) & (0xff00u >> carry_bits)) : 0;
        // the next round zeroes s_buf only behind the barriers of its first scan
    }
    if (t == 0) seg_bytes[seg] = (int)(out_pos < slot_bytes ? out_pos : slot_bytes);
}

// ------------------------------------------------------------------------------------------------ pack
__global__ __launch_bounds__(NT) void pack_kernel(const uint8_t* __restrict__ slots, const int* __restrict__ seg_bytes,
                                                  const long long* __restrict__ seg_offsets, uint8_t* __restrict__ out, int mr, size_t slot_bytes,
                                                  long long out_bytes) {
    const long long seg = blockIdx.x;
    const long long n = seg_bytes[seg], off = seg_offsets[seg];
    const int row = (int)(seg % mr);
    const bool marker = row != mr - 1;
    if (n < 0 || (size_t)n > slot_bytes || off < 0 || off + n + (marker ? 2 : 0) > out_bytes) return;      // never outside either buffer
    const uint8_t* s = slots + (size_t)seg * slot_bytes;
    for (long long i = threadIdx.x; i < n; i += NT) out[off + i] = s[i];
    if (marker && threadIdx.x < 2) out[off + n + threadIdx.x] = threadIdx.x ? (uint8_t)(0xD0 + (row & 7)) : (uint8_t)0xFF;
}

inline bool sampling_ok(int s) { return s == EW_JPEG_420 || s == EW_JPEG_444; }

}  // namespace

extern "C" size_t ew_jpeg_segment_slot_bytes(int mcu_cols, int blocks_per_mcu) {
    if (mcu_cols <= 0 || blocks_per_mcu <= 0) return 0;
    return (size_t)mcu_cols * blocks_per_mcu * (2 * BLOCK_MAX_BYTES);
}

extern "C" ew_status ew_jpeg_dct_quant(const uint8_t* frames, int16_t* coef, int V, int H, int W, int quality, int subsampling, void* stream) {
    EW_REQUIRE(frames && coef, "ew_jpeg_dct_quant: NULL frames or coefficients");
    EW_REQUIRE(V >= 1 && V <= 65535, "ew_jpeg_dct_quant: V = %d must be 1 .. 65535", V);
    EW_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "ew_jpeg_dct_quant: H = %d, W = %d must be 1 .. 65535", H, W);
    EW_REQUIRE(quality >= 1 && quality <= 100, "ew_jpeg_dct_quant: quality = %d must be 1 .. 100", quality);
    EW_REQUIRE(sampling_ok(subsampling), "ew_jpeg_dct_quant: subsampling = %d must be EW_JPEG_420 or EW_JPEG_444", subsampling);
    EW_REQUIRE(((uintptr_t)coef & 15) == 0, "ew_jpeg_dct_quant: coef must be 16-byte aligned");
    const int mcu = subsampling == EW_JPEG_420 ? 16 : 8;
    const int mr = (H + mcu - 1) / mcu, mc = (W + mcu - 1) / mcu;
    const int xtiles = (W + TILE_W - 1) / TILE_W;
    const dim3 grid((unsigned)xtiles * (unsigned)mr, (unsigned)V);
    const QuantTables qt = quant_tables(quality);
    if (subsampling == EW_JPEG_420)
        hipLaunchKernelGGL(dct_quant_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, frames, (short*)coef, H, W, mr, mc, xtiles, qt);
    else
        hipLaunchKernelGGL(dct_quant_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, frames, (short*)coef, H, W, mr, mc, xtiles, qt);
    return ew_check_launch("dct_quant_kernel");
}

extern "C" ew_status ew_jpeg_entropy(const int16_t* coef, uint8_t* slots, int* seg_bytes, long long n_segments, int mcu_cols,
                                     int blocks_per_mcu, size_t slot_bytes, void* stream) {
    EW_REQUIRE(coef && slots && seg_bytes, "ew_jpeg_entropy: NULL pointer");
    EW_REQUIRE(n_segments >= 1 && n_segments < (1LL << 31), "ew_jpeg_entropy: n_segments = %lld must be 1 .. 2^31 - 1", n_segments);
    EW_REQUIRE(mcu_cols >= 1 && mcu_cols <= 8192, "ew_jpeg_entropy: mcu_cols = %d must be 1 .. 8192", mcu_cols);
    EW_REQUIRE(blocks_per_mcu == 6 || blocks_per_mcu == 3, "ew_jpeg_entropy: blocks_per_mcu = %d must be 6 (4:2:0) or 3 (4:4:4)", blocks_per_mcu);
    EW_REQUIRE(slot_bytes >= ew_jpeg_segment_slot_bytes(mcu_cols, blocks_per_mcu),
               "ew_jpeg_entropy: slot_bytes = %zu is below the worst case %zu (ew_jpeg_segment_slot_bytes)", slot_bytes,
               ew_jpeg_segment_slot_bytes(mcu_cols, blocks_per_mcu));
    EW_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)seg_bytes & 3) == 0, "ew_jpeg_entropy: coef must be 16-byte, seg_bytes 4-byte aligned");
    const int nb = mcu_cols * blocks_per_mcu;
    if (blocks_per_mcu == 6)
        hipLaunchKernelGGL(entropy_kernel<true>, dim3((unsigned)n_segments), dim3(NT), 0, (hipStream_t)stream, (const short*)coef, slots,
                           seg_bytes, nb, slot_bytes);
    else
        hipLaunchKernelGGL(entropy_kernel<false>, dim3((unsigned)n_segments), dim3(NT), 0, (hipStream_t)stream, (const short*)coef, slots,
                           seg_bytes, nb, slot_bytes);
    return ew_check_launch("entropy_kernel");
}

extern "C" ew_status ew_jpeg_pack(const uint8_t* slots, const int* seg_bytes, const long long* seg_offsets, uint8_t* out, long long n_segments,
                                  int mcu_rows, size_t slot_bytes, long long out_bytes, void* stream) {
    EW_REQUIRE(slots && seg_bytes && seg_offsets && out, "ew_jpeg_pack: NULL pointer");
    EW_REQUIRE(n_segments >= 1 && n_segments < (1LL << 31), "ew_jpeg_pack: n_segments = %lld must be 1 .. 2^31 - 1", n_segments);
    EW_REQUIRE(mcu_rows >= 1 && n_segments % mcu_rows == 0, "ew_jpeg_pack: n_segments = %lld must be a multiple of mcu_rows = %d", n_segments,
               mcu_rows);
    EW_REQUIRE(slot_bytes >= 1 && out_bytes >= 1, "ew_jpeg_pack: slot_bytes = %zu and out_bytes = %lld must be positive", slot_bytes, out_bytes);
    EW_REQUIRE(((uintptr_t)seg_bytes & 3) == 0 && ((uintptr_t)seg_offsets & 7) == 0, "ew_jpeg_pack: seg_bytes must be 4-byte, seg_offsets 8-byte aligned");
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)n_segments), dim3(NT), 0, (hipStream_t)stream, slots, seg_bytes, seg_offsets, out, mcu_rows,
                       slot_bytes, out_bytes);
    return ew_check_launch("pack_kernel");
}
