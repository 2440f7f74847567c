// video_decode.hip -- baseline JPEG frames decoded on the device (ABI 19, symbols added without a bump): the way back from the MJPEG
// files of video.hip / evoworld_amd/video.py to pixels, so that the navigated.avi / original.avi of a run can be scored as the
// reference's evoworld/metrics/other_metrics/calculate_scores.py scores its navigated.mp4 / original.mp4.  Compiled
// with -ffp-contract=off: every product and sum below is one float32 rounding, except the IDCT's dot products, which are explicit
// fmaf chains (one rounding per term).
//
//   ew_jpeg_huffman_decode  one lane per restart segment: a 64-bit bit buffer refilled byte by byte (FF 00 unstuffed), symbols through
//                           a 9-bit prefix table with the canonical maxcode / valptr walk behind it (tables built by the caller from
//                           the file's DHT segments, held in LDS), DC predictors reset at the segment's start.  The coefficients are
//                           zeroed by a memset in front of the kernel; a lane writes the values it decodes, inside its own blocks.
//   ew_jpeg_idct            32 blocks per workgroup in LDS: dequantise, inverse 8-point DCT along the columns, then along the rows,
//                           + 128, round half to even, clamp, one 8-byte store per block row into the padded sample planes.
//   ew_jpeg_planes_to_rgb   one lane per pixel: centred triangle upsampling of the 4:2:0 chroma planes (taps clamped to the padded
//                           plane), JFIF YCbCr -> RGB, cropped to H x W.
//   ew_resize_linear_u8     one lane per output pixel: bilinear sampling at half-pixel centres without antialiasing.
// No global atomics and no data-dependent order: two calls return identical bytes.
#include "common.h"
#include "jpeg_tables.h"

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------------------------------------ Huffman decoding
constexpr int HD_NT = 64;                         // one wave loads the tables
constexpr int HD_LANES = 4;                       // segments per workgroup: few, so that the segments spread over the CUs and a wave
                                                  // serialises the divergent paths of 4 bit streams, not 64
constexpr int HT_BYTES = EW_JPEG_HUFF_TABLE_BYTES;
constexpr int HT_WORDS = HT_BYTES / 4;
constexpr int HT_LOOK_BITS = 9;
static_assert(HT_BYTES == 512 * 2 + 18 * 4 + 18 * 4 + 256, "the table layout of evoworld_hip.h");

struct HuffView {
    const unsigned short* look;                   // [512]  9-bit prefix -> length << 8 | symbol, 0 = no code of <= 9 bits
    const int* maxcode;                           // [18]   the largest code of length l (l = 1 .. 16), -1 = none
    const int* valoff;                            // [18]   index of the first symbol of length l minus its first code
    const unsigned char* vals;                    // [256]  symbols in code order
};

__device__ __forceinline__ HuffView huff_view(const unsigned* s_tab, int which) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(s_tab + which * HT_WORDS);
    return {reinterpret_cast<const unsigned short*>(b), reinterpret_cast<const int*>(b + 1024), reinterpret_cast<const int*>(b + 1096), b + 1168};
}

// The segment's bits, most significant first.  Reads stay inside p[0, end): `pos` only grows and is compared against `end` before every
// load.  Bits past the end read as zeros and are never handed out: take() refuses more than `nbits`.
struct BitReader {
    const uint8_t* p;
    int pos, end;
    unsigned long long acc;                       // the next bits, left-aligned
    int nbits;
    bool marker;                                  // an FF not followed by 00 was met: the bytes from there on are not scan data

    __device__ __forceinline__ void fill() {
        while (nbits <= 56 && pos < end) {        // at most 8 rounds, each consumes a byte
            const unsigned b = p[pos++];
            if (b == 0xFFu) {
                if (pos < end && p[pos] == 0) ++pos;
                else {
                    marker = true;
                    pos = end;
                    break;
                }
            }
            acc |= (unsigned long long)b << (56 - nbits);
            nbits += 8;
        }
    }
    __device__ __forceinline__ unsigned peek(int n) const { return (unsigned)(acc >> (64 - n)); }          // n = 1 .. 16
    __device__ __forceinline__ bool take(int n) {
        if (n > nbits) return false;
        acc <<= n;
        nbits -= n;
        return true;
    }
    __device__ __forceinline__ int short_of_bits() const { return marker ? EW_JPEG_SEG_MARKER : EW_JPEG_SEG_EXHAUSTED; }
};

// the next Huffman symbol (0 .. 255), or -1 with `status` set
__device__ __forceinline__ int next_symbol(BitReader& br, const HuffView& h, int& status) {
    br.fill();
    const unsigned e = h.look[br.peek(HT_LOOK_BITS)];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (e == 0) {
        len = 0;
#pragma unroll 1
        for (int l = HT_LOOK_BITS + 1; l <= 16; ++l) {
            const int code = (int)br.peek(l);
            if (code <= h.maxcode[l]) {
                len = l;
                sym = h.vals[(code + h.valoff[l]) & 255];
                break;
            }
        }
    }
    if (len < 1 || len > 16) {
        status = EW_JPEG_SEG_BAD_CODE;
        return -1;
    }
    if (!br.take(len)) {
        status = br.short_of_bits();
        return -1;
    }
    return sym;
}

// the next `size` (1 .. 11) bits as a signed value (T.81 F.2.2.1 EXTEND); false with `status` set when the segment has run out
__device__ __forceinline__ bool next_value(BitReader& br, int size, int& value, int& status) {
    br.fill();
    const int v = (int)br.peek(size);
    if (!br.take(size)) {
        status = br.short_of_bits();
        return false;
    }
    value = v < (1 << (size - 1)) ? v - (1 << size) + 1 : v;
    return true;
}

__global__ __launch_bounds__(HD_NT) void huffman_decode_kernel(const uint8_t* __restrict__ scan, long long scan_bytes,
                                                               const long long* __restrict__ seg_start, const int* __restrict__ seg_bytes,
                                                               const unsigned* __restrict__ tables, short* __restrict__ coef,
                                                               int* __restrict__ seg_status, long long n_seg, int segs_per_frame,
                                                               int mcus_per_frame, int bpm, int interval) {
    __shared__ unsigned s_tab[4 * HT_WORDS];
    for (int i = threadIdx.x; i < 4 * HT_WORDS; i += HD_NT) s_tab[i] = tables[i];
    __syncthreads();
    const long long seg = (long long)blockIdx.x * HD_LANES + threadIdx.x;
    if (threadIdx.x >= HD_LANES || seg >= n_seg) return;
    const long long start = seg_start[seg];
    const int nbytes = seg_bytes[seg];
    if (start < 0 || nbytes < 0 || start + nbytes > scan_bytes) {
        seg_status[seg] = EW_JPEG_SEG_RANGE;
        return;
    }
    const long long frame = seg / segs_per_frame;
    const int first = (int)(seg % segs_per_frame) * interval;              // interval * segs_per_frame < mcus_per_frame + interval
    const int n_mcu = min(interval, mcus_per_frame - first);
    short* out = coef + (frame * mcus_per_frame + first) * bpm * 64;       // this segment's blocks: n_mcu * bpm of them
    const int n_y = bpm - 2;                                               // luminance blocks per MCU
    BitReader br = {scan + start, 0, nbytes, 0ull, 0, false};
    int pred_y = 0, pred_cb = 0, pred_cr = 0;
    int status = EW_JPEG_SEG_OK;
#pragma unroll 1
    for (int b = 0; b < n_mcu * bpm && status == EW_JPEG_SEG_OK; ++b) {
        const int j = b % bpm;
        const int comp = j < n_y ? 0 : j - n_y + 1;
        const HuffView dc = huff_view(s_tab, comp ? 1 : 0), ac = huff_view(s_tab, comp ? 3 : 2);
        short* blk = out + (long long)b * 64;
        const int size = next_symbol(br, dc, status);
        if (size < 0) break;
        if (size > 11) {
            status = EW_JPEG_SEG_SIZE;
            break;
        }
        int diff = 0;
        if (size && !next_value(br, size, diff, status)) break;
        const int p = (comp == 0 ? pred_y : (comp == 1 ? pred_cb : pred_cr)) + diff;     // selects, not an indexed array: registers
        if (comp == 0) pred_y = p;
        else if (comp == 1) pred_cb = p;
        else pred_cr = p;
        blk[0] = (short)min(max(p, -32768), 32767);
        int k = 1;
#pragma unroll 1
        while (k < 64) {                                                   // every round moves k forward by at least 1
            const int rs = next_symbol(br, ac, status);
            if (rs < 0) break;
            const int run = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                if (run == 0) break;                                       // EOB
                if (run != 15) {                                           // EOBn belongs to progressive scans
                    status = EW_JPEG_SEG_BAD_CODE;
                    break;
                }
                k += 16;                                                   // ZRL: a coefficient has to follow
                if (k > 63) status = EW_JPEG_SEG_INDEX;
                continue;
            }
            if (sz > 10) {
                status = EW_JPEG_SEG_SIZE;
                break;
            }
            k += run;
            if (k > 63) {
                status = EW_JPEG_SEG_INDEX;
                break;
            }
            int v;
            if (!next_value(br, sz, v, status)) break;
            blk[k++] = (short)v;
        }
    }
    if (status == EW_JPEG_SEG_OK) {
        if (br.marker) status = EW_JPEG_SEG_MARKER;
        else if (br.nbits + 8 * (br.end - br.pos) > 7) status = EW_JPEG_SEG_LEFTOVER;
    }
    seg_status[seg] = status;
}

// ------------------------------------------------------------------------------------------------ dequantisation + IDCT
constexpr int ID_BLOCKS = NT / 8;                // blocks per workgroup: 8 lanes per block, one column and then one row each
constexpr int BLK_LD = 9;                        // LDS row stride of a block (8 + 1: rows and columns both walk conflict-free)
constexpr int BLK_SZ = 8 * BLK_LD;

// y[n] = sum_k M[k][n] * p[k * stride]: the inverse (transpose) of video.hip's dct8
__device__ __forceinline__ void idct8(const float* p, int stride, float (&y)[8]) {
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = p[k * stride];
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        float a = dct_m(0, n) * x[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) a = fmaf(dct_m(k, n), x[k], a);
        y[n] = a;
    }
}

__device__ __forceinline__ unsigned sample_u8(float v) { return (unsigned)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

__global__ __launch_bounds__(NT) void idct_kernel(const short* __restrict__ coef, const uint8_t* __restrict__ qt, uint8_t* __restrict__ yp,
                                                  uint8_t* __restrict__ cbp, uint8_t* __restrict__ crp, long long n_blocks, int mr, int mc,
                                                  int bpm) {
    __shared__ float s_blk[ID_BLOCKS * BLK_SZ];
    __shared__ float s_q[2][64];                         // divisors in zigzag order
    const int t = threadIdx.x;
    if (t < 128) s_q[t >> 6][t & 63] = (float)qt[(t >> 6) * 64 + d_zigzag[t & 63]];
    __syncthreads();
    const int b = t >> 3, g = t & 7;
    const long long gb = (long long)blockIdx.x * ID_BLOCKS + b;
    const bool have = gb < n_blocks;
    const long long m = gb / bpm;
    const int j = (int)(gb - m * bpm);
    const int n_y = bpm - 2;
    float* blk = s_blk + b * BLK_SZ;
    if (have) {                                          // 8 consecutive zigzag positions = one 16-byte load
        const uint4 raw = *reinterpret_cast<const uint4*>(coef + gb * 64 + g * 8);
        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
        const float* q = s_q[j >= n_y];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = g * 8 + e, nat = d_zigzag[k];
            blk[(nat >> 3) * BLK_LD + (nat & 7)] = (float)(int)(short)(w[e >> 1] >> (16 * (e & 1))) * q[k];
        }
    }
    __syncthreads();
    float y[8];
    idct8(blk + g, BLK_LD, y);                           // column g
#pragma unroll
    for (int n = 0; n < 8; ++n) blk[n * BLK_LD + g] = y[n];
    __syncthreads();
    idct8(blk + g * BLK_LD, 1, y);                       // row g
    if (!have) return;
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        lo |= sample_u8(y[n] + 128.0f) << (8 * n);
        hi |= sample_u8(y[n + 4] + 128.0f) << (8 * n);
    }
    const long long v = m / ((long long)mr * mc);
    const int rem = (int)(m - v * mr * mc), my = rem / mc, mx = rem - my * mc;
    uint8_t* dst;
    if (j < n_y) {                                       // 4:2:0: Y00 Y01 Y10 Y11 inside a 16 x 16 MCU; 4:4:4: one block
        const int ms = n_y == 4 ? 16 : 8;
        const long long row = (v * mr + my) * ms + (j >> 1) * 8 + g;
        dst = yp + row * ((long long)mc * ms) + mx * ms + (j & 1) * 8;
    } else {
        const long long row = (v * mr + my) * 8 + g;
        dst = (j == n_y ? cbp : crp) + row * ((long long)mc * 8) + mx * 8;
    }
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
}

// ------------------------------------------------------------------------------------------------ planes -> RGB
template <bool SUB420>
__global__ __launch_bounds__(NT) void planes_to_rgb_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cbp,
                                                           const uint8_t* __restrict__ crp, uint8_t* __restrict__ out, int H, int W, int ph,
                                                           int pw) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int v = blockIdx.y, y = (int)(i / W), x = (int)(i - (long long)y * W);
    const float Y = (float)yp[((long long)v * ph + y) * pw + x];
    float cb, cr;
    if (SUB420) {
        // out[2i] = 3/4 p[i] + 1/4 p[i - 1], out[2i + 1] = 3/4 p[i] + 1/4 p[i + 1] on either axis; sums of 16ths of bytes: exact in float32
        const int ch = ph >> 1, cw = pw >> 1;
        const int cy = y >> 1, cx = x >> 1;
        const int oy = min(max(cy + ((y & 1) ? 1 : -1), 0), ch - 1), ox = min(max(cx + ((x & 1) ? 1 : -1), 0), cw - 1);
        const uint8_t* pb = cbp + (long long)v * ch * cw;
        const uint8_t* pr = crp + (long long)v * ch * cw;
        const long long a = (long long)cy * cw, o = (long long)oy * cw;
        const float b0 = 0.75f * (float)pb[a + cx] + 0.25f * (float)pb[o + cx], b1 = 0.75f * (float)pb[a + ox] + 0.25f * (float)pb[o + ox];
        const float r0 = 0.75f * (float)pr[a + cx] + 0.25f * (float)pr[o + cx], r1 = 0.75f * (float)pr[a + ox] + 0.25f * (float)pr[o + ox];
        cb = 0.75f * b0 + 0.25f * b1;
        cr = 0.75f * r0 + 0.25f * r1;
    } else {
        const long long at = ((long long)v * ph + y) * pw + x;
        cb = (float)cbp[at];
        cr = (float)crp[at];
    }
    cb -= 128.0f;
    cr -= 128.0f;
    uint8_t* px = out + ((long long)v * H * W + i) * 3;
    px[0] = (uint8_t)sample_u8(Y + 1.402f * cr);
    px[1] = (uint8_t)sample_u8(Y - 0.344136286f * cb - 0.714136286f * cr);
    px[2] = (uint8_t)sample_u8(Y + 1.772f * cb);
}

// ------------------------------------------------------------------------------------------------ bilinear resize
// source position of output index d: (d + 0.5) * n_src / n_dst - 0.5 = ((2 d + 1) n_src - n_dst) / (2 n_dst), split exactly in integers
// into the left neighbour (floor) and the weight of the right one
__device__ __forceinline__ void linear_tap(int d, int n_src, int n_dst, int& i0, int& i1, float& f) {
    const long long num = (2LL * d + 1) * n_src - n_dst, den = 2LL * n_dst;
    long long q = num / den;
    if (num - q * den < 0) --q;
    f = __fdiv_rn((float)(num - q * den), (float)den);
    i0 = (int)min(max(q, 0LL), (long long)n_src - 1);
    i1 = (int)min(max(q + 1, 0LL), (long long)n_src - 1);
}

__global__ __launch_bounds__(NT) void resize_linear_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int h,
                                                           int w) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= (long long)h * w) return;
    const int v = blockIdx.y, y = (int)(i / w), x = (int)(i - (long long)y * w);
    int y0, y1, x0, x1;
    float fy, fx;
    linear_tap(y, H, h, y0, y1, fy);
    linear_tap(x, W, w, x0, x1, fx);
    const uint8_t* f = src + (long long)v * H * W * 3;
    const uint8_t *p00 = f + ((long long)y0 * W + x0) * 3, *p01 = f + ((long long)y0 * W + x1) * 3;
    const uint8_t *p10 = f + ((long long)y1 * W + x0) * 3, *p11 = f + ((long long)y1 * W + x1) * 3;
    uint8_t* o = dst + ((long long)v * h * w + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (1.0f - fx) * (float)p00[c] + fx * (float)p01[c];
        const float bot = (1.0f - fx) * (float)p10[c] + fx * (float)p11[c];
        o[c] = (uint8_t)sample_u8((1.0f - fy) * top + fy * bot);
    }
}

}  // namespace

extern "C" ew_status ew_jpeg_huffman_decode(const uint8_t* scan, long long scan_bytes, const long long* seg_start, const int* seg_bytes,
                                            const uint8_t* tables, int16_t* coef, int* seg_status, long long n_segments, int V, int mcu_rows,
                                            int mcu_cols, int blocks_per_mcu, int restart_interval, void* stream) {
    EW_REQUIRE(scan && seg_start && seg_bytes && tables && coef && seg_status, "ew_jpeg_huffman_decode: NULL pointer");
    EW_REQUIRE(scan_bytes >= 1, "ew_jpeg_huffman_decode: scan_bytes = %lld must be positive", scan_bytes);
    EW_REQUIRE(V >= 1 && V <= 65535, "ew_jpeg_huffman_decode: V = %d must be 1 .. 65535", V);
    EW_REQUIRE(mcu_rows >= 1 && mcu_rows <= 8192 && mcu_cols >= 1 && mcu_cols <= 8192,
               "ew_jpeg_huffman_decode: mcu_rows = %d and mcu_cols = %d must be 1 .. 8192", mcu_rows, mcu_cols);
    EW_REQUIRE(blocks_per_mcu == 6 || blocks_per_mcu == 3, "ew_jpeg_huffman_decode: blocks_per_mcu = %d must be 6 (4:2:0) or 3 (4:4:4)",
               blocks_per_mcu);
    EW_REQUIRE(restart_interval >= 0 && restart_interval <= 65535, "ew_jpeg_huffman_decode: restart_interval = %d must be 0 .. 65535",
               restart_interval);
    const int mcus = mcu_rows * mcu_cols;
    const int interval = restart_interval == 0 || restart_interval > mcus ? mcus : restart_interval;
    const int per_frame = (mcus + interval - 1) / interval;
    EW_REQUIRE(n_segments == (long long)V * per_frame, "ew_jpeg_huffman_decode: n_segments = %lld, but %d frames of %d MCUs at interval %d hold %lld",
               n_segments, V, mcus, restart_interval, (long long)V * per_frame);
    EW_REQUIRE(((uintptr_t)tables & 3) == 0 && ((uintptr_t)seg_bytes & 3) == 0 && ((uintptr_t)seg_status & 3) == 0 &&
                   ((uintptr_t)seg_start & 7) == 0 && ((uintptr_t)coef & 1) == 0,
               "ew_jpeg_huffman_decode: tables, seg_bytes and seg_status must be 4-byte, seg_start 8-byte, coef 2-byte aligned");
    const hipError_t e = hipMemsetAsync(coef, 0, (size_t)V * mcus * blocks_per_mcu * 64 * sizeof(int16_t), (hipStream_t)stream);
    if (e != hipSuccess) {
        ew_set_error("ew_jpeg_huffman_decode: hipMemsetAsync: %s", hipGetErrorString(e));
        return EW_ERR_HIP;
    }
    const unsigned grid = (unsigned)((n_segments + HD_LANES - 1) / HD_LANES);
    hipLaunchKernelGGL(huffman_decode_kernel, dim3(grid), dim3(HD_NT), 0, (hipStream_t)stream, scan, scan_bytes, seg_start, seg_bytes,
                       (const unsigned*)tables, (short*)coef, seg_status, n_segments, per_frame, mcus, blocks_per_mcu, interval);
    return ew_check_launch("huffman_decode_kernel");
}

extern "C" ew_status ew_jpeg_idct(const int16_t* coef, const uint8_t* qtables, uint8_t* y, uint8_t* cb, uint8_t* cr, int V, int mcu_rows,
                                  int mcu_cols, int blocks_per_mcu, void* stream) {
    EW_REQUIRE(coef && qtables && y && cb && cr, "ew_jpeg_idct: NULL pointer");
    EW_REQUIRE(V >= 1 && V <= 65535, "ew_jpeg_idct: V = %d must be 1 .. 65535", V);
    EW_REQUIRE(mcu_rows >= 1 && mcu_rows <= 8192 && mcu_cols >= 1 && mcu_cols <= 8192, "ew_jpeg_idct: mcu_rows = %d and mcu_cols = %d must be 1 .. 8192",
               mcu_rows, mcu_cols);
    EW_REQUIRE(blocks_per_mcu == 6 || blocks_per_mcu == 3, "ew_jpeg_idct: blocks_per_mcu = %d must be 6 (4:2:0) or 3 (4:4:4)", blocks_per_mcu);
    EW_REQUIRE(((uintptr_t)coef & 15) == 0, "ew_jpeg_idct: coef must be 16-byte aligned");
    EW_REQUIRE((((uintptr_t)y | (uintptr_t)cb | (uintptr_t)cr) & 7) == 0, "ew_jpeg_idct: the planes must be 8-byte aligned");
    const long long n_blocks = (long long)V * mcu_rows * mcu_cols * blocks_per_mcu;
    EW_REQUIRE((n_blocks + ID_BLOCKS - 1) / ID_BLOCKS < (1LL << 31), "ew_jpeg_idct: %lld blocks are more than one launch holds", n_blocks);
    hipLaunchKernelGGL(idct_kernel, dim3((unsigned)((n_blocks + ID_BLOCKS - 1) / ID_BLOCKS)), dim3(NT), 0, (hipStream_t)stream, (const short*)coef,
                       qtables, y, cb, cr, n_blocks, mcu_rows, mcu_cols, blocks_per_mcu);
    return ew_check_launch("idct_kernel");
}

extern "C" ew_status ew_jpeg_planes_to_rgb(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint8_t* rgb, int V, int H, int W,
                                           int subsampling, void* stream) {
    EW_REQUIRE(y && cb && cr && rgb, "ew_jpeg_planes_to_rgb: NULL pointer");
    EW_REQUIRE(V >= 1 && V <= 65535, "ew_jpeg_planes_to_rgb: V = %d must be 1 .. 65535", V);
    EW_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "ew_jpeg_planes_to_rgb: H = %d, W = %d must be 1 .. 65535", H, W);
    EW_REQUIRE(subsampling == EW_JPEG_420 || subsampling == EW_JPEG_444, "ew_jpeg_planes_to_rgb: subsampling = %d must be EW_JPEG_420 or EW_JPEG_444",
               subsampling);
    const int mcu = subsampling == EW_JPEG_420 ? 16 : 8;
    const int ph = (H + mcu - 1) / mcu * mcu, pw = (W + mcu - 1) / mcu * mcu;
    const dim3 grid((unsigned)(((long long)H * W + NT - 1) / NT), (unsigned)V);
    if (subsampling == EW_JPEG_420)
        hipLaunchKernelGGL(planes_to_rgb_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, y, cb, cr, rgb, H, W, ph, pw);
    else
        hipLaunchKernelGGL(planes_to_rgb_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, y, cb, cr, rgb, H, W, ph, pw);
    return ew_check_launch("planes_to_rgb_kernel");
}

extern "C" ew_status ew_resize_linear_u8(const uint8_t* src, uint8_t* dst, int V, int H, int W, int h, int w, void* stream) {
    EW_REQUIRE(src && dst, "ew_resize_linear_u8: NULL pointer");
    EW_REQUIRE(V >= 1 && V <= 65535, "ew_resize_linear_u8: V = %d must be 1 .. 65535", V);
    EW_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535 && h >= 1 && h <= 65535 && w >= 1 && w <= 65535,
               "ew_resize_linear_u8: H = %d, W = %d, h = %d, w = %d must be 1 .. 65535", H, W, h, w);
    const dim3 grid((unsigned)(((long long)h * w + NT - 1) / NT), (unsigned)V);
    hipLaunchKernelGGL(resize_linear_kernel, grid, dim3(NT), 0, (hipStream_t)stream, src, dst, H, W, h, w);
    return ew_check_launch("resize_linear_kernel");
}
