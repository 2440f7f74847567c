// fp8.hip -- optional fp8 (OCP e4m3) path for the attention q / k / v projections (BASELINE.json configs[4]: "fp16 U-Net + fp8
// MFMA QKV").  Off by default (EW_QKV_FP8=1 / UNet(qkv_fp8=True)); it changes the numerics contract and carries its own
// stated tolerance (tests/test_gpu_fp8_qkv.py).
//   ew_quant_rows_fp8   x fp16 [M,K] -> q fp8 [M,K] + scale fp32 [M], scale = amax(row) / 448  (per-token dynamic scaling)
//   ew_gemm_fp8         out[m][n] = (sum_k qa[m][k] * qw[n][k]) * a_scale[m] * w_scale[n] * c_acc, fp32 accumulation on
//                       v_mfma_f32_16x16x32_fp8_fp8, fp16 out.  128x128 tile, 4 wave64 (2x2), 64-byte K-tiles through a
//                       double-buffered padded LDS tile; swapped operands (D[n][m]) so a lane owns 4 consecutive output columns.
//                       c_acc carries ops.QK_LOG2_PRESCALE for the spatial q|k projection (as ew_gemm_args.c_acc does on the fp16 path).
// The non-scaled fp8 MFMA runs at the fp16 rate on gfx950: what this path halves is the operand BYTES (HBM + LDS staging) of
// the projections, which are memory-bound at level 0 (K = 320).
#include "common.h"

namespace {

constexpr float FP8_MAX = 448.0f;

// one wave per row; the row lives in registers (K <= 2048, K % 8 == 0)
template <int NV>
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const f16* __restrict__ x, uint8_t* __restrict__ q,
                                                             float* __restrict__ scale, int rows, int K) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int VPP = K / 8;
    f16x8 v[NV];
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int vi = lane + k * 64;
        if (vi < VPP) {
            v[k] = *(const f16x8*)(x + (size_t)row * K + vi * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)v[k][e]));
        }
    }
    amax = wave_max(amax);
    const float sc = amax > 0.f ? amax / FP8_MAX : 1.0f;
    const float inv = 1.0f / sc;
    if (lane == 0) scale[row] = sc;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int vi = lane + k * 64;
        if (vi < VPP) {
            int w0 = 0, w1 = 0;
            w0 = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[k][0] * inv, (float)v[k][1] * inv, w0, false);
            w0 = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[k][2] * inv, (float)v[k][3] * inv, w0, true);
            w1 = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[k][4] * inv, (float)v[k][5] * inv, w1, false);
            w1 = __builtin_amdgcn_cvt_pk_fp8_f32((float)v[k][6] * inv, (float)v[k][7] * inv, w1, true);
            *(int2*)(q + (size_t)row * K + vi * 8) = make_int2(w0, w1);
        }
    }
}

constexpr int TM = 128, TN = 128, TK = 64, LDSROW = 80;       // 64 data bytes + 16 pad per LDS row
constexpr int STAGE_BYTES = (TM + TN) * LDSROW;               // 20,480 B

__global__ __launch_bounds__(256) void gemm_fp8_kernel(const uint8_t* __restrict__ A, const float* __restrict__ a_scale,
                                                       const uint8_t* __restrict__ W, const float* __restrict__ w_scale,
                                                       f16* __restrict__ out, int M, int N, int K, long long ld_out, float c_acc) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int tiles_n = (N + TN - 1) / TN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
    const int m0 = tm * TM, n0 = tn * TN;
    const int r = lane & 15, ks = lane >> 4;
    // staging: 256 threads x 2 x 16 B per operand: thread -> (row = tid >> 2 (+64), 16-byte column tid & 3)
    const int srow = tid >> 2, scol = (tid & 3) * 16;
    const int ma0 = min(m0 + srow, M - 1), ma1 = min(m0 + srow + 64, M - 1);      // rows past the edge re-read the last row: loaded, never stored
    const int nb0 = min(n0 + srow, N - 1), nb1 = min(n0 + srow + 64, N - 1);
    const uint8_t* ap0 = A + (size_t)ma0 * K + scol;
    const uint8_t* ap1 = A + (size_t)ma1 * K + scol;
    const uint8_t* wp0 = W + (size_t)nb0 * K + scol;
    const uint8_t* wp1 = W + (size_t)nb1 * K + scol;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nk = K / TK;
    int4 ra0, ra1, rw0, rw1;                                  // (scalars, not arrays behind lambdas: those ended up in scratch)
#define FP8_GLOAD(kt)                                                                                                            \
    do {                                                                                                                         \
        ra0 = *(const int4*)(ap0 + (kt) * TK); rw0 = *(const int4*)(wp0 + (kt) * TK);                                            \
        ra1 = *(const int4*)(ap1 + (kt) * TK); rw1 = *(const int4*)(wp1 + (kt) * TK);                                            \
    } while (0)
#define FP8_LSTORE(buf)                                                                                                          \
    do {                                                                                                                         \
        char* sb = smem + (buf) * STAGE_BYTES;                                                                                   \
        *(int4*)(sb + srow * LDSROW + scol) = ra0;        *(int4*)(sb + (TM + srow) * LDSROW + scol) = rw0;                      \
        *(int4*)(sb + (srow + 64) * LDSROW + scol) = ra1; *(int4*)(sb + (TM + srow + 64) * LDSROW + scol) = rw1;                 \
    } while (0)
    FP8_GLOAD(0);
    FP8_LSTORE(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const char* b = smem + (kt & 1) * STAGE_BYTES;
        if (kt + 1 < nk) FP8_GLOAD(kt + 1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {                      // two 32-wide MFMA k-slices per 64-byte K-tile
            long af[4], wf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *(const long*)(b + (wm * 64 + i * 16 + r) * LDSROW + kk * 32 + ks * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *(const long*)(b + (TM + wn * 64 + j * 16 + r) * LDSROW + kk * 32 + ks * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(wf[j], af[i], acc[i][j], 0, 0, 0);       // D[n][m]
        }
        if (kt + 1 < nk) FP8_LSTORE((kt + 1) & 1);             // the other buffer was last read in iteration kt-1
        __syncthreads();
    }
#undef FP8_GLOAD
#undef FP8_LSTORE
    // epilogue: lane holds D[n = 4*ks + e][m = r] of every 16x16 fragment
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm * 64 + i * 16 + r;
        if (m >= M) continue;
        const float sa = a_scale[m];                          // ((acc * sa) * sw) * c_acc: the scales first, c_acc last
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + ks * 4;
            if (n + 3 < N) {
                const f32x4 sw = *(const f32x4*)(w_scale + n);
                const f16x4 o = {(f16)(acc[i][j][0] * sa * sw[0] * c_acc), (f16)(acc[i][j][1] * sa * sw[1] * c_acc),
                                 (f16)(acc[i][j][2] * sa * sw[2] * c_acc), (f16)(acc[i][j][3] * sa * sw[3] * c_acc)};
                *(f16x4*)(out + (size_t)m * ld_out + n) = o;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < N) out[(size_t)m * ld_out + n + e] = (f16)(acc[i][j][e] * sa * w_scale[n + e] * c_acc);
            }
        }
    }
}

}  // namespace

extern "C" ew_status ew_quant_rows_fp8(const void* x, void* q, float* scale, int rows, int K, void* stream) {
    EW_REQUIRE(x && q && scale && rows > 0 && K > 0 && K % 8 == 0 && K <= 2048, "ew_quant_rows_fp8: need K %% 8 == 0, K <= 2048 (K=%d)", K);
    const int nv = (K / 8 + 63) / 64;
    dim3 grid(ew_cdiv(rows, 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
#define QL(NV) hipLaunchKernelGGL(quant_rows_fp8_kernel<NV>, grid, block, 0, s, (const f16*)x, (uint8_t*)q, scale, rows, K)
    if (nv == 1) QL(1); else if (nv == 2) QL(2); else if (nv == 3) QL(3); else QL(4);
#undef QL
    return ew_check_launch("ew_quant_rows_fp8");
}

extern "C" ew_status ew_gemm_fp8(const void* a, const float* a_scale, const void* w, const float* w_scale, void* out, int M,
                                 int N, int K, long long ld_out, float c_acc, void* stream) {
    EW_REQUIRE(a && a_scale && w && w_scale && out, "ew_gemm_fp8: null pointer");
    EW_REQUIRE(M > 0 && N > 0 && K > 0 && K % TK == 0 && N % 4 == 0 && ld_out % 4 == 0 && ld_out >= N, "ew_gemm_fp8: need K %% 64 == 0, N %% 4 == 0 (M=%d N=%d K=%d)", M, N, K);
    EW_REQUIRE((((uintptr_t)a | (uintptr_t)w) & 15) == 0 && ((uintptr_t)w_scale & 15) == 0, "ew_gemm_fp8: operands must be 16-byte aligned");
    EW_REQUIRE(((uintptr_t)out & 7) == 0, "ew_gemm_fp8: out must be 8-byte aligned");
    const long long tiles = (long long)ew_cdiv(M, TM) * ew_cdiv(N, TN);
    EW_REQUIRE(tiles < 0x7fffffffLL, "ew_gemm_fp8: grid too large");
    hipLaunchKernelGGL(gemm_fp8_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)a, a_scale,
                       (const uint8_t*)w, w_scale, (f16*)out, M, N, K, ld_out, c_acc);
    return ew_check_launch("ew_gemm_fp8");
}
