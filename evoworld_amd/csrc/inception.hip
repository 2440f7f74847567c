// inception.hip -- the non-GEMM kernels of the latent MSE's Inception-v4 network (timm `inception_v4`, classifier removed: 1536 pooled
// features) for the evaluation CLI (ABI 17).
// Reference: evoworld/metrics/other_metrics/calculate_latent_mse.py:11-79 (load_inception_v4_model, the Resize((299, 299)) + Normalize
// transform, calculate_latent_mse), run by evoworld/metrics/calculate_all_metrics.py:220-221.  The 149 BatchNorm-folded convolutions run
// on ew_gemm_f16 (dense mode, bias vector) over the patch rows ew_im2col3d_f16 writes with kt = 1, the max pools on
// ew_maxpool3d_relu_f16 (csrc/i3d.hip); conv outputs are stored PRE-ReLU and every reader below applies max(x, 0) itself.
// Compiled with -ffp-contract=off: k / 255 and (x - mean) / std are rounded where they are written.  The reference resizes on the host, and
// torch's x86 builds (AVX2 / AVX-512 code paths) contract each filter tap t += src[j] * w[j] to fma(src[j], w[j], t): the fmaf calls below are
// those, spelled out, and with the host's float32 tables they reproduce F.interpolate(antialias=True) bit for bit.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_TAPS = 4096;                             // per output index and axis

struct Norm { float mean[3], stdev[3]; };
struct AxisTable { const int* first; const int* count; const float* weights; int kmax; };

// One thread per output pixel: for every source row of the pixel's H window the W pass (a float32 fma chain in tap order), then the H pass over
// those row values in tap order -- the values a W pass over the whole frame followed by an H pass gives, without the intermediate frame.
// 3 normalised channels + 5 zeros in one 16-byte store.  KIND 1: uint8 [F,H,W,3]; KIND 2: fp32 [F,3,H,W].  Table entries are clamped to
// the frame, so that a table for another size cannot make the kernel read outside `src`.
template <int KIND>
__global__ __launch_bounds__(NT) void frames_resize_aa_norm_kernel(const void* __restrict__ src, f16* __restrict__ out, long long total, int H,
                                                                   int W, int oh, int ow, AxisTable ty, AxisTable tx, int swap, Norm nm) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int ox = (int)(i % ow);
        const long long r = i / ow;
        const int oy = (int)(r % oh);
        const long long f = r / oh;
        const int y0 = ty.first[oy], ny = min(ty.count[oy], ty.kmax);
        const int x0 = tx.first[ox], nx = min(tx.count[ox], tx.kmax);
        const float* wy = ty.weights + (long long)oy * ty.kmax;
        const float* wx = tx.weights + (long long)ox * tx.kmax;
        f16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (f16)0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sc = swap ? 2 - c : c;
            float acc = 0.0f;
            for (int jy = 0; jy < ny; ++jy) {
                const int iy = min(max(y0 + jy, 0), H - 1);
                float row = 0.0f;
                if (KIND == 1) {
                    const uint8_t* s = (const uint8_t*)src + ((f * H + iy) * W) * 3 + sc;
                    for (int jx = 0; jx < nx; ++jx) row = fmaf((float)s[(long long)min(max(x0 + jx, 0), W - 1) * 3] / 255.0f, wx[jx], row);
                } else {
                    const float* s = (const float*)src + ((f * 3 + sc) * H + iy) * W;
                    for (int jx = 0; jx < nx; ++jx) row = fmaf(s[min(max(x0 + jx, 0), W - 1)], wx[jx], row);
                }
                acc = fmaf(row, wy[jy], acc);
            }
            v[c] = (f16)((acc - nm.mean[c]) / nm.stdev[c]);
        }
        *reinterpret_cast<f16x8*>(out + i * 8) = v;
    }
}

// AvgPool2d(3, 1, 1, count_include_pad=False) of max(x, 0): one thread per 8 channels of one output pixel; the in-bounds taps are added in
// fp32 in (dy, dx) order and divided by their number (4 in a corner, 6 on an edge, 9 inside; fewer where H or W < 3)
__global__ __launch_bounds__(NT) void avgpool3x3_relu_kernel(const f16* __restrict__ src, f16* __restrict__ out, long long total_vec, int H, int W,
                                                             int C8) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total_vec; i += (long long)gridDim.x * NT) {
        const int c8 = (int)(i % C8);
        long long r = i / C8;
        const int x = (int)(r % W);
        r /= W;
        const int y = (int)(r % H);
        const long long n = r / H;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
        int taps = 0;
        for (int dy = -1; dy <= 1; ++dy) {
            const int iy = y + dy;
            if (iy < 0 || iy >= H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int ix = x + dx;
                if (ix < 0 || ix >= W) continue;
                const uint4 raw = *reinterpret_cast<const uint4*>(src + (((n * H + iy) * W + ix) * C8 + c8) * 8);
                const f16x8 h = *reinterpret_cast<const f16x8*>(&raw);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += h[e] > (f16)0 ? (float)h[e] : 0.0f;
                ++taps;
            }
        }
        const float d = (float)taps;
        f16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (f16)(acc[e] / d);
        *reinterpret_cast<f16x8*>(out + i * 8) = v;
    }
}

// mean over the h * w pixels of max(x, 0): one thread per 8 channels of one frame, the pixels added in fp32 in row-major order
__global__ __launch_bounds__(NT) void global_avgpool_relu_kernel(const f16* __restrict__ src, float* __restrict__ out, long long total_vec, int hw,
                                                                 int C8) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total_vec; i += (long long)gridDim.x * NT) {
        const int c8 = (int)(i % C8);
        const long long n = i / C8;
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
        for (int p = 0; p < hw; ++p) {
            const uint4 raw = *reinterpret_cast<const uint4*>(src + ((n * hw + p) * C8 + c8) * 8);
            const f16x8 h = *reinterpret_cast<const f16x8*>(&raw);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += h[e] > (f16)0 ? (float)h[e] : 0.0f;
        }
        const float d = (float)hw;
        f32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo[e] = acc[e] / d; hi[e] = acc[4 + e] / d; }
        *reinterpret_cast<f32x4*>(out + i * 8) = lo;
        *reinterpret_cast<f32x4*>(out + i * 8 + 4) = hi;
    }
}

inline int grid_for(long long total) {
    long long b = (total + NT - 1) / NT;
    return (int)(b < 8192 ? b : 8192);
}

}  // namespace

extern "C" ew_status ew_frames_resize_aa_norm_f16(const void* src, int src_kind, void* out, int F, int H, int W, int out_h, int out_w,
                                                  const int* y_first, const int* y_count, const float* y_weights, int y_taps, const int* x_first,
                                                  const int* x_count, const float* x_weights, int x_taps, int swap_rb, const float* mean_std,
                                                  void* stream) {
    EW_REQUIRE(src && out && y_first && y_count && y_weights && x_first && x_count && x_weights && mean_std, "ew_frames_resize_aa_norm_f16: NULL pointer");
    EW_REQUIRE(src_kind == 1 || src_kind == 2, "ew_frames_resize_aa_norm_f16: src_kind %d (1: uint8 [F,H,W,3] frames, 2: fp32 [F,3,H,W] frames)", src_kind);
    EW_REQUIRE(F > 0 && H > 0 && W > 0 && (long long)H * W * 3 < (1LL << 31), "ew_frames_resize_aa_norm_f16: bad frame size (F %d, %d x %d)", F, H, W);
    EW_REQUIRE(out_h > 0 && out_w > 0 && (long long)out_h * out_w < (1LL << 31), "ew_frames_resize_aa_norm_f16: bad output size %d x %d", out_h, out_w);
    EW_REQUIRE(y_taps > 0 && y_taps <= MAX_TAPS && x_taps > 0 && x_taps <= MAX_TAPS, "ew_frames_resize_aa_norm_f16: taps per output index (%d, %d) must lie in [1, %d]",
               y_taps, x_taps, MAX_TAPS);
    Norm nm;
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean_std[c];
        nm.stdev[c] = mean_std[3 + c];
        EW_REQUIRE(nm.stdev[c] > 0.0f && nm.mean[c] == nm.mean[c], "ew_frames_resize_aa_norm_f16: std[%d] = %g must be positive and mean[%d] a number", c,
                   (double)nm.stdev[c], c);
    }
    EW_REQUIRE((uintptr_t)out % 16 == 0 && (src_kind == 1 || (uintptr_t)src % 4 == 0), "ew_frames_resize_aa_norm_f16: out must be 16-byte, an fp32 source 4-byte aligned");
    EW_REQUIRE(((uintptr_t)y_first | (uintptr_t)y_count | (uintptr_t)y_weights | (uintptr_t)x_first | (uintptr_t)x_count | (uintptr_t)x_weights) % 4 == 0,
               "ew_frames_resize_aa_norm_f16: the tables must be 4-byte aligned");
    const long long total = (long long)F * out_h * out_w;
    const AxisTable ty{y_first, y_count, y_weights, y_taps}, tx{x_first, x_count, x_weights, x_taps};
    hipStream_t st = (hipStream_t)stream;
    if (src_kind == 1)
        hipLaunchKernelGGL(frames_resize_aa_norm_kernel<1>, dim3(grid_for(total)), dim3(NT), 0, st, src, (f16*)out, total, H, W, out_h, out_w, ty, tx,
                           swap_rb ? 1 : 0, nm);
    else
        hipLaunchKernelGGL(frames_resize_aa_norm_kernel<2>, dim3(grid_for(total)), dim3(NT), 0, st, src, (f16*)out, total, H, W, out_h, out_w, ty, tx,
                           swap_rb ? 1 : 0, nm);
    return ew_check_launch("frames_resize_aa_norm_kernel");
}

extern "C" ew_status ew_avgpool3x3_relu_f16(const void* src, void* out, int n_img, int H, int W, int C, void* stream) {
    EW_REQUIRE(src && out, "ew_avgpool3x3_relu_f16: NULL pointer");
    EW_REQUIRE(n_img > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "ew_avgpool3x3_relu_f16: needs n, H, W > 0 and C %% 8 == 0 (%d x %d x %d x %d)", n_img, H,
               W, C);
    EW_REQUIRE((long long)n_img * H * W < (1LL << 31), "ew_avgpool3x3_relu_f16: batch too large");
    EW_REQUIRE((uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0, "ew_avgpool3x3_relu_f16: pointers must be 16-byte aligned");
    const long long total_vec = (long long)n_img * H * W * (C / 8);
    hipLaunchKernelGGL(avgpool3x3_relu_kernel, dim3(grid_for(total_vec)), dim3(NT), 0, (hipStream_t)stream, (const f16*)src, (f16*)out, total_vec, H, W,
                       C / 8);
    return ew_check_launch("avgpool3x3_relu_kernel");
}

extern "C" ew_status ew_global_avgpool_relu_f32(const void* src, float* out, int n_img, int h, int w, int C, void* stream) {
    EW_REQUIRE(src && out, "ew_global_avgpool_relu_f32: NULL pointer");
    EW_REQUIRE(n_img > 0 && h > 0 && w > 0 && C > 0 && C % 8 == 0, "ew_global_avgpool_relu_f32: needs n, h, w > 0 and C %% 8 == 0 (%d x %d x %d x %d)", n_img,
               h, w, C);
    EW_REQUIRE((long long)h * w < (1LL << 24) && (long long)n_img * h * w < (1LL << 31), "ew_global_avgpool_relu_f32: batch too large");
    EW_REQUIRE((uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0, "ew_global_avgpool_relu_f32: pointers must be 16-byte aligned");
    const long long total_vec = (long long)n_img * (C / 8);
    hipLaunchKernelGGL(global_avgpool_relu_kernel, dim3(grid_for(total_vec)), dim3(NT), 0, (hipStream_t)stream, (const f16*)src, out, total_vec, h * w,
                       C / 8);
    return ew_check_launch("global_avgpool_relu_kernel");
}
