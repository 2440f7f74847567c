// convnet.hip -- the layer kernels the metric networks of the evaluation CLI share (ABI 20): LPIPS/AlexNet (lpips.hip), FVD's I3D (i3d.hip)
// and the latent MSE's Inception-v4 (inception.hip).  Every convolution of the three runs on ew_gemm_f16 (dense mode, bias vector) over the
// patch rows ew_im2col3d_f16 writes -- a 2-D network passes kt = 1 with its image batch on the T axis; conv outputs are stored PRE-ReLU and
// every reader below applies max(x, 0) itself (the GEMM has no ReLU epilogue; ReLU commutes with max-pooling, and zero padding of a max pool
// over non-negative values equals skipping the taps).  All tensors are fp16 [T,H,W,C], channels innermost, C % 8 == 0, 16-byte aligned.
// Compiled with -ffp-contract=off, as the three files are: the average pools add and divide in fp32 where they are written.
#include "convnet.h"

namespace {

// fp16 [T,H,W,C] source, C % 8 == 0: one thread per 8 output columns (one 16-byte load and store; a vector never straddles a tap)
template <bool RELU>
__global__ __launch_bounds__(NT) void im2col3d_kernel(const f16* __restrict__ src, f16* __restrict__ out, long long total_vec, Dim3 in, int C,
                                                      Dim3 k, Dim3 s, Dim3 p, Dim3 o, int ldk8, int kC) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total_vec; i += (long long)gridDim.x * NT) {
        const int col8 = (int)(i % ldk8);
        long long row = i / ldk8;
        const int kk = col8 * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (kk < kC) {
            int tap = kk / C;
            const int c = kk - tap * C;
            const int dx = tap % k.w;
            tap /= k.w;
            const int dy = tap % k.h, dt = tap / k.h;
            const int ox = (int)(row % o.w);
            row /= o.w;
            const int oy = (int)(row % o.h), ot = (int)(row / o.h);
            const int it = ot * s.t + dt - p.t, iy = oy * s.h + dy - p.h, ix = ox * s.w + dx - p.w;
            if (it >= 0 && it < in.t && iy >= 0 && iy < in.h && ix >= 0 && ix < in.w) {
                v = *reinterpret_cast<const uint4*>(src + (((long long)it * in.h + iy) * in.w + ix) * C + c);
                if (RELU) v = relu8(v);
            }
        }
        *reinterpret_cast<uint4*>(out + i * 8) = v;
    }
}

// max over the window's taps inside the input of max(x, 0); 8 channels per thread
__global__ __launch_bounds__(NT) void maxpool3d_relu_kernel(const f16* __restrict__ src, f16* __restrict__ out, long long total_vec, Dim3 in, int C8,
                                                            Dim3 k, Dim3 s, Dim3 p, Dim3 o) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total_vec; i += (long long)gridDim.x * NT) {
        const int c8 = (int)(i % C8);
        long long r = i / C8;
        const int ox = (int)(r % o.w);
        r /= o.w;
        const int oy = (int)(r % o.h), ot = (int)(r / o.h);
        f16x8 m;
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = (f16)0;
        for (int dt = 0; dt < k.t; ++dt) {
            const int it = ot * s.t + dt - p.t;
            if (it < 0 || it >= in.t) continue;
            for (int dy = 0; dy < k.h; ++dy) {
                const int iy = oy * s.h + dy - p.h;
                if (iy < 0 || iy >= in.h) continue;
                for (int dx = 0; dx < k.w; ++dx) {
                    const int ix = ox * s.w + dx - p.w;
                    if (ix < 0 || ix >= in.w) continue;
                    const uint4 raw = *reinterpret_cast<const uint4*>(src + ((((long long)it * in.h + iy) * in.w + ix) * C8 + c8) * 8);
                    const f16x8 v = *reinterpret_cast<const f16x8*>(&raw);
#pragma unroll
                    for (int e = 0; e < 8; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
                }
            }
        }
        *reinterpret_cast<f16x8*>(out + i * 8) = m;
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
                const uint4 raw = relu8(*reinterpret_cast<const uint4*>(src + (((n * H + iy) * W + ix) * C8 + c8) * 8));
                const f16x8 h = *reinterpret_cast<const f16x8*>(&raw);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (float)h[e];
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
            const uint4 raw = relu8(*reinterpret_cast<const uint4*>(src + ((n * hw + p) * C8 + c8) * 8));
            const f16x8 h = *reinterpret_cast<const f16x8*>(&raw);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)h[e];
        }
        const float d = (float)hw;
        f32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) { lo[e] = acc[e] / d; hi[e] = acc[4 + e] / d; }
        *reinterpret_cast<f32x4*>(out + i * 8) = lo;
        *reinterpret_cast<f32x4*>(out + i * 8 + 4) = hi;
    }
}

}  // namespace

// shared geometry checks of the two window kernels: every window starts inside the padded input and overlaps the input itself
#define EW_REQUIRE_WINDOWS(name)                                                                                                              \
    EW_REQUIRE(t_in > 0 && h_in > 0 && w_in > 0 && C > 0 && C % 8 == 0, name ": needs T, H, W > 0 and C %% 8 == 0 (%d x %d x %d x %d)", t_in, \
               h_in, w_in, C);                                                                                                                \
    EW_REQUIRE(kt > 0 && kh > 0 && kw > 0 && st > 0 && sh > 0 && sw > 0, name ": kernel (%d,%d,%d) / stride (%d,%d,%d) must be positive", kt, \
               kh, kw, st, sh, sw);                                                                                                           \
    EW_REQUIRE(pt >= 0 && pt < kt && ph >= 0 && ph < kh && pw >= 0 && pw < kw, name ": front pads (%d,%d,%d) must lie in [0, kernel)", pt, ph, \
               pw);                                                                                                                           \
    EW_REQUIRE(t_out > 0 && h_out > 0 && w_out > 0 && (long long)(t_out - 1) * st - pt < t_in && (long long)(h_out - 1) * sh - ph < h_in &&   \
                   (long long)(w_out - 1) * sw - pw < w_in,                                                                                   \
               name ": an output of %d x %d x %d has windows that miss the %d x %d x %d input", t_out, h_out, w_out, t_in, h_in, w_in);      \
    EW_REQUIRE((long long)t_in * h_in * w_in < (1LL << 31) && (long long)t_out * h_out * w_out < (1LL << 31), name ": clip too large");     \
    EW_REQUIRE((uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0, name ": pointers must be 16-byte aligned")

extern "C" ew_status ew_im2col3d_f16(const void* src, void* out, int t_in, int h_in, int w_in, int C, int kt, int kh, int kw, int st, int sh,
                                     int sw, int pt, int ph, int pw, int t_out, int h_out, int w_out, int ldk, int relu, void* stream) {
    EW_REQUIRE(src && out, "ew_im2col3d_f16: NULL pointer");
    EW_REQUIRE_WINDOWS("ew_im2col3d_f16");
    const long long kC = (long long)kt * kh * kw * C;
    EW_REQUIRE(kC <= ldk && ldk % 8 == 0, "ew_im2col3d_f16: ldk = %d must be a multiple of 8 and >= kt*kh*kw*C = %lld", ldk, kC);
    const long long total_vec = (long long)t_out * h_out * w_out * (ldk / 8);
    const Dim3 in{t_in, h_in, w_in}, k{kt, kh, kw}, s{st, sh, sw}, p{pt, ph, pw}, o{t_out, h_out, w_out};
    if (relu)
        hipLaunchKernelGGL(im2col3d_kernel<true>, dim3(grid_for(total_vec)), dim3(NT), 0, (hipStream_t)stream, (const f16*)src, (f16*)out, total_vec,
                           in, C, k, s, p, o, ldk / 8, (int)kC);
    else
        hipLaunchKernelGGL(im2col3d_kernel<false>, dim3(grid_for(total_vec)), dim3(NT), 0, (hipStream_t)stream, (const f16*)src, (f16*)out, total_vec,
                           in, C, k, s, p, o, ldk / 8, (int)kC);
    return ew_check_launch("im2col3d_kernel");
}

extern "C" ew_status ew_maxpool3d_relu_f16(const void* src, void* out, int t_in, int h_in, int w_in, int C, int kt, int kh, int kw, int st, int sh,
                                           int sw, int pt, int ph, int pw, int t_out, int h_out, int w_out, void* stream) {
    EW_REQUIRE(src && out, "ew_maxpool3d_relu_f16: NULL pointer");
    EW_REQUIRE_WINDOWS("ew_maxpool3d_relu_f16");
    const long long total_vec = (long long)t_out * h_out * w_out * (C / 8);
    const Dim3 in{t_in, h_in, w_in}, k{kt, kh, kw}, s{st, sh, sw}, p{pt, ph, pw}, o{t_out, h_out, w_out};
    hipLaunchKernelGGL(maxpool3d_relu_kernel, dim3(grid_for(total_vec)), dim3(NT), 0, (hipStream_t)stream, (const f16*)src, (f16*)out, total_vec, in,
                       C / 8, k, s, p, o);
    return ew_check_launch("maxpool3d_relu_kernel");
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
