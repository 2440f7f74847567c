// i3d.hip -- the kernels only FVD's I3D network has (Inception-v1 inflated to 3-D, 400 Kinetics classes; ABI 16): the clip preprocessing and
// the head.  Reference: evoworld/metrics/fvd/styleganv/fvd.py (preprocess_single, frechet_distance) and
// evoworld/metrics/fvd/videogpt/pytorch_i3d.py (InceptionI3d).  The 57 BatchNorm-folded convolutions run on ew_gemm_f16 (dense mode, bias
// vector) over the patch rows of ew_im2col3d_f16, the max pools on ew_maxpool3d_relu_f16 (convnet.hip); conv outputs are stored PRE-ReLU
// and the head applies max(x, 0) itself.
// Compiled with -ffp-contract=off: the resize's k / 255, source index, weights and blend are rounded where torch's CPU kernel rounds them.
// preprocess_single runs on the host in the reference, and torch's x86 builds (AVX2 / AVX-512 code paths) contract the source index to
// fma(scale, i + 0.5, -0.5) and each two-term blend t0 * w0 + t1 * w1 to fma(t0, w0, t1 * w1): the fmaf calls below are those, spelled out.
#include "convnet.h"
#include <math.h>

namespace {

constexpr int SIDE = 224;                                  // I3D's input resolution
constexpr int HEAD_C = 1024, HEAD_HW = 49, HEAD_N = 400;   // Mixed_5c channels, its 7 x 7 pixels, Kinetics classes

// torch's bilinear source index (align_corners=False) in float32: i -> (i0, i1, lambda); equal sizes copy (lambda = 0 either way)
__device__ __forceinline__ void src_index(int i, float scale, int n_in, int& i0, int& i1, float& l1) {
    float s = fmaf(scale, (float)i + 0.5f, -0.5f);
    s = s < 0.0f ? 0.0f : s;
    i0 = min((int)s, n_in - 1);
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(s - (float)i0, 0.0f), 1.0f);
}

// one thread per output pixel: 3 blended channels + 5 zeros in one 16-byte store.  KIND 1: uint8 [T,H,W,3]; KIND 2: fp32 [T,3,H,W].
template <int KIND>
__global__ __launch_bounds__(NT) void video_preprocess_kernel(const void* __restrict__ src, f16* __restrict__ out, long long total, int H, int W,
                                                              float scale_h, float scale_w, int y0, int x0, int swap) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int x = (int)(i % SIDE);
        const long long r = i / SIDE;
        const int y = (int)(r % SIDE);
        const long long t = r / SIDE;
        int ya, yb, xa, xb;
        float ly, lx;
        src_index(y + y0, scale_h, H, ya, yb, ly);
        src_index(x + x0, scale_w, W, xa, xb, lx);
        const float wy0 = 1.0f - ly, wx0 = 1.0f - lx;
        f16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (f16)0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sc = swap ? 2 - c : c;
            float p00, p01, p10, p11;
            if (KIND == 1) {
                const uint8_t* s = (const uint8_t*)src + t * H * W * 3 + sc;
                p00 = (float)s[((long long)ya * W + xa) * 3] / 255.0f;
                p01 = (float)s[((long long)ya * W + xb) * 3] / 255.0f;
                p10 = (float)s[((long long)yb * W + xa) * 3] / 255.0f;
                p11 = (float)s[((long long)yb * W + xb) * 3] / 255.0f;
            } else {
                const float* s = (const float*)src + (t * 3 + sc) * H * W;
                p00 = s[(long long)ya * W + xa];
                p01 = s[(long long)ya * W + xb];
                p10 = s[(long long)yb * W + xa];
                p11 = s[(long long)yb * W + xb];
            }
            const float top = fmaf(p00, wx0, p01 * lx), bot = fmaf(p10, wx0, p11 * lx);
            const float val = fmaf(top, wy0, bot * ly);
            v[c] = (f16)((val - 0.5f) * 2.0f);
        }
        *reinterpret_cast<f16x8*>(out + i * 8) = v;
    }
}

// ---- the head ----
// Stage 1, one block per 64 channels: 8 lanes x 8 channels across, 32 pixel slots down.  A slot adds cnt(frame) * max(x, 0) of its pixels
// p = slot, slot + 32, ... in that order (cnt = the number of (2,7,7) windows the frame lies in: 1 for the first and last frame, else 2);
// the 32 slots are then added in slot order and scaled by 1 / (98 (T' - 1)): v[c], the mean over windows of the average pool.
constexpr int HEAD_SLOTS = NT / 8;

__global__ __launch_bounds__(NT) void i3d_head_mean_kernel(const f16* __restrict__ x, int Tp, float* __restrict__ v) {
    __shared__ float s_part[HEAD_SLOTS][64];
    const int tid = threadIdx.x, sub = tid & 7, slot = tid >> 3;
    const int c0 = blockIdx.x * 64 + sub * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
    const int npx = Tp * HEAD_HW;
    for (int p = slot; p < npx; p += HEAD_SLOTS) {
        const int j = p / HEAD_HW;
        const float cnt = (j == 0 || j == Tp - 1) ? 1.0f : 2.0f;
        const uint4 raw = relu8(*reinterpret_cast<const uint4*>(x + (long long)p * HEAD_C + c0));
        const f16x8 h = *reinterpret_cast<const f16x8*>(&raw);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += cnt * (float)h[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_part[slot][sub * 8 + e] = acc[e];
    __syncthreads();
    if (tid < 64) {
        float s = 0.0f;
        for (int q = 0; q < HEAD_SLOTS; ++q) s += s_part[q][tid];
        v[blockIdx.x * 64 + tid] = s / (float)(2 * HEAD_HW * (Tp - 1));
    }
}

// Stage 2, one wave per class: lane l adds W[n][4 (l + 64 q) ..] * v[..] for q = 0..3 in order, a butterfly adds the lanes, then + b[n]
__global__ __launch_bounds__(NT) void i3d_head_logits_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ v,
                                                             float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (n >= HEAD_N) return;                               // wave-uniform
    float s = 0.0f;
#pragma unroll
    for (int q = 0; q < HEAD_C / 256; ++q) {
        const int c = 4 * (lane + 64 * q);
        const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (long long)n * HEAD_C + c);
        const f32x4 vv = *reinterpret_cast<const f32x4*>(v + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += wv[e] * vv[e];
    }
    s = wave_sum(s);
    if (lane == 0) out[n] = s + b[n];
}

}  // namespace

extern "C" ew_status ew_video_preprocess_f16(const void* src, int src_kind, void* out, int T, int H, int W, int h_resized, int w_resized, int y0,
                                             int x0, int swap_rb, void* stream) {
    EW_REQUIRE(src && out, "ew_video_preprocess_f16: NULL pointer");
    EW_REQUIRE(src_kind == 1 || src_kind == 2, "ew_video_preprocess_f16: src_kind %d (1: uint8 [T,H,W,3] frames, 2: fp32 [T,3,H,W] frames)", src_kind);
    EW_REQUIRE(T > 0 && H > 0 && W > 0 && (long long)H * W * 3 < (1LL << 31), "ew_video_preprocess_f16: bad clip size (T %d, %d x %d)", T, H, W);
    EW_REQUIRE(h_resized >= SIDE && w_resized >= SIDE && (long long)h_resized * w_resized < (1LL << 40),
               "ew_video_preprocess_f16: the resized frame %d x %d must be at least %d x %d", h_resized, w_resized, SIDE, SIDE);
    EW_REQUIRE(y0 >= 0 && x0 >= 0 && y0 + SIDE <= h_resized && x0 + SIDE <= w_resized,
               "ew_video_preprocess_f16: the crop at (%d, %d) leaves the resized frame %d x %d", y0, x0, h_resized, w_resized);
    EW_REQUIRE((uintptr_t)out % 16 == 0 && (src_kind == 1 || (uintptr_t)src % 4 == 0), "ew_video_preprocess_f16: out must be 16-byte, an fp32 source 4-byte aligned");
    const long long total = (long long)T * SIDE * SIDE;
    const float sh = (float)H / (float)h_resized, sw = (float)W / (float)w_resized;
    hipStream_t st = (hipStream_t)stream;
    if (src_kind == 1)
        hipLaunchKernelGGL(video_preprocess_kernel<1>, dim3(grid_for(total)), dim3(NT), 0, st, src, (f16*)out, total, H, W, sh, sw, y0, x0, swap_rb ? 1 : 0);
    else
        hipLaunchKernelGGL(video_preprocess_kernel<2>, dim3(grid_for(total)), dim3(NT), 0, st, src, (f16*)out, total, H, W, sh, sw, y0, x0, swap_rb ? 1 : 0);
    return ew_check_launch("video_preprocess_kernel");
}

extern "C" size_t ew_i3d_head_workspace_bytes(void) { return HEAD_C * sizeof(float); }

extern "C" ew_status ew_i3d_head(const void* x, int t_in, int h_in, int w_in, int C, const float* w, const float* b, float* logits, void* workspace,
                                 void* stream) {
    EW_REQUIRE(x && w && b && logits && workspace, "ew_i3d_head: NULL pointer");
    EW_REQUIRE(t_in >= 2 && t_in <= 4096 && h_in == 7 && w_in == 7 && C == HEAD_C,
               "ew_i3d_head: expected the Mixed_5c output [T' >= 2, 7, 7, %d], got [%d, %d, %d, %d]", HEAD_C, t_in, h_in, w_in, C);
    EW_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0 && (uintptr_t)workspace % 16 == 0 && (uintptr_t)b % 4 == 0 && (uintptr_t)logits % 4 == 0,
               "ew_i3d_head: x, w and workspace must be 16-byte, b and logits 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(i3d_head_mean_kernel, dim3(HEAD_C / 64), dim3(NT), 0, st, (const f16*)x, t_in, (float*)workspace);
    ew_status s = ew_check_launch("i3d_head_mean_kernel");
    if (s != EW_OK) return s;
    hipLaunchKernelGGL(i3d_head_logits_kernel, dim3(ew_cdiv(HEAD_N, NT / 64)), dim3(NT), 0, st, w, b, (const float*)workspace, logits);
    return ew_check_launch("i3d_head_logits_kernel");
}
