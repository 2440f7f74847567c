// inception.hip -- the kernel only the latent MSE's Inception-v4 network has (timm `inception_v4`, classifier removed: 1536 pooled
// features; ABI 17): the frames' resize + normalise.
// Reference: evoworld/metrics/other_metrics/calculate_latent_mse.py:11-79 (load_inception_v4_model, the Resize((299, 299)) + Normalize
// transform, calculate_latent_mse), run by evoworld/metrics/calculate_all_metrics.py:220-221.  The 149 BatchNorm-folded convolutions run
// on ew_gemm_f16 (dense mode, bias vector) over the patch rows ew_im2col3d_f16 writes with kt = 1, the pools on ew_maxpool3d_relu_f16,
// ew_avgpool3x3_relu_f16 and ew_global_avgpool_relu_f32 (all in convnet.hip).
// Compiled with -ffp-contract=off: k / 255 and (x - mean) / std are rounded where they are written.  The reference resizes on the host, and
// torch's x86 builds (AVX2 / AVX-512 code paths) contract each filter tap t += src[j] * w[j] to fma(src[j], w[j], t): the fmaf calls below are
// those, spelled out, and with the host's float32 tables they reproduce F.interpolate(antialias=True) bit for bit.
#include "convnet.h"

namespace {

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
