// lpips.hip -- the kernels only LPIPS (AlexNet backbone) has (ABI 14): the first layer's patch gather from the frames and the head.
// Reference: evoworld/metrics/other_metrics/calculate_lpips.py and calculate_all_metrics.py:195-221, i.e. lpips.LPIPS(net='alex',
// spatial=True).forward(img1, img2).mean() per frame pair.  The five convolutions run on ew_gemm_f16 (dense mode, bias vector) over
// the patch rows ew_im2col_frames_f16 (first layer) and ew_im2col3d_f16 with kt = 1 (convnet.hip) write, the max pools on
// ew_maxpool3d_relu_f16 (convnet.hip); conv outputs are stored PRE-ReLU and the head applies max(x, 0) itself.
// Compiled with -ffp-contract=off: the first layer's k / 255 -> 2x - 1 -> (x - shift) / scale are the reference's separate float32
// roundings.
#include "convnet.h"
#include <math.h>

namespace {

struct FirstAffine { float shift[3], scale[3]; };

__device__ __forceinline__ float first_value(float x01, int c, const FirstAffine& fa) {
    const float x = x01 * 2.0f - 1.0f;                     // calculate_lpips.py: frames in [0,1] -> [-1,1]
    return (x - fa.shift[c]) / fa.scale[c];                // lpips ScalingLayer
}

// first layer: uint8 [n,h,w,3] (KIND 1) or fp32 [n,3,h,w] (KIND 2) frames in [0,1]; column = (ky*k + kx)*3 + c, where network
// channel c reads frame channel (swap ? 2 - c : c) and takes the scaling constants of c
template <int KIND>
__global__ __launch_bounds__(NT) void im2col_first_kernel(const void* __restrict__ src, f16* __restrict__ out, long long total_vec,
                                                          int h_in, int w_in, int k, int stride, int pad, int h_out, int w_out,
                                                          int ldk8, int kkC, int swap, FirstAffine fa) {
    __shared__ f16 s_lut[3][256];
    if (KIND == 1) {
        for (int t = threadIdx.x; t < 768; t += NT) {
            const int c = t >> 8, kv = t & 255;
            s_lut[c][kv] = (f16)first_value((float)kv / 255.0f, c, fa);
        }
        __syncthreads();
    }
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total_vec; i += (long long)gridDim.x * NT) {
        const int col8 = (int)(i % ldk8);
        const long long row = i / ldk8;
        const int ox = (int)(row % w_out);
        const long long t = row / w_out;
        const int oy = (int)(t % h_out);
        const long long img = t / h_out;
        f16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = col8 * 8 + e;
            f16 r = (f16)0;
            if (kk < kkC) {
                const int tap = kk / 3, c = kk - tap * 3;
                const int ky = tap / k, kx = tap - ky * k;
                const int iy = oy * stride + ky - pad, ix = ox * stride + kx - pad;
                if (iy >= 0 && iy < h_in && ix >= 0 && ix < w_in) {
                    const int sc = swap ? 2 - c : c;
                    if (KIND == 1) r = s_lut[c][((const uint8_t*)src)[((img * h_in + iy) * w_in + ix) * 3 + sc]];
                    else r = (f16)first_value(((const float*)src)[((img * 3 + sc) * h_in + iy) * w_in + ix], c, fa);
                }
            }
            v[e] = r;
        }
        *reinterpret_cast<f16x8*>(out + i * 8) = v;
    }
}

// ---- the head of one tap ----
// A wave holds 64 / LPP pixels: LPP lanes per pixel, 8 channels per lane (C <= 8 * LPP) in one 16-byte load per tensor.  The sums over
// channels are butterflies inside the lane group (every lane ends with the same value, in an order that does not depend on which
// tensor is a and which is b); lane 0 of a group adds its pixels' d * wy * wx in fp64.  The block's 256 fp64 values are reduced in a
// fixed tree and stored; head_reduce_kernel adds a frame's blocks in a fixed order.  The number of blocks depends on (h, w, C) only.
constexpr int HEAD_MAX_BLOCKS = 128;

inline int head_lpp_host(int C) { return C <= 64 ? 8 : (C <= 256 ? 32 : 64); }
inline int head_blocks(int h, int w, int C) {
    const int ppb = (NT / 64) * (64 / head_lpp_host(C));
    const int b = ew_cdiv((long long)h * w, ppb);
    return b < HEAD_MAX_BLOCKS ? b : HEAD_MAX_BLOCKS;
}

template <int LPP>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = LPP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int LPP>
__global__ __launch_bounds__(NT) void lpips_head_kernel(const f16* __restrict__ fa, const f16* __restrict__ fb, const float* __restrict__ lin,
                                                        const double* __restrict__ wy, const double* __restrict__ wx, int h, int w, int C,
                                                        double* __restrict__ part) {
    __shared__ double s_red[NT];
    constexpr int PPW = 64 / LPP;                          // pixels per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % LPP, grp = lane / LPP;
    const int c0 = sub * 8;
    const bool active = c0 < C;                            // C % 8 == 0: a lane's 8 channels are all inside or all outside
    const int f = blockIdx.y;
    const int npx = h * w;
    float l[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) l[e] = active ? lin[c0 + e] : 0.0f;
    const f16* pa = fa + (long long)f * npx * C;
    const f16* pb = fb + (long long)f * npx * C;
    double acc = 0.0;
    const int step = gridDim.x * (NT / 64) * PPW;
    for (int base = (blockIdx.x * (NT / 64) + wave) * PPW; base < npx; base += step) {      // wave-uniform trip count
        const int p = base + grp;
        const bool valid = p < npx;
        uint4 ra = make_uint4(0u, 0u, 0u, 0u), rb = ra;
        if (valid && active) {
            ra = *reinterpret_cast<const uint4*>(pa + (long long)p * C + c0);
            rb = *reinterpret_cast<const uint4*>(pb + (long long)p * C + c0);
        }
        ra = relu8(ra);
        rb = relu8(rb);
        const f16x8 ha = *reinterpret_cast<const f16x8*>(&ra), hb = *reinterpret_cast<const f16x8*>(&rb);
        float a[8], b[8], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            a[e] = (float)ha[e];
            b[e] = (float)hb[e];
            sa += a[e] * a[e];
            sb += b[e] * b[e];
        }
        const float na = sqrtf(group_sum<LPP>(sa)) + 1e-10f, nb = sqrtf(group_sum<LPP>(sb)) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float t = a[e] / na - b[e] / nb;
            d += l[e] * (t * t);
        }
        d = group_sum<LPP>(d);
        if (sub == 0 && valid) {
            const int y = p / w, x = p - y * w;
            acc += (double)d * (wy[y] * wx[x]);
        }
    }
    s_red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] += s_red[tid + s];
        __syncthreads();
    }
    if (tid == 0) part[(long long)f * gridDim.x + blockIdx.x] = s_red[0];
}

__global__ __launch_bounds__(HEAD_MAX_BLOCKS) void lpips_head_reduce_kernel(const double* __restrict__ part, int nblk, double n_out,
                                                                            double* __restrict__ acc) {
    __shared__ double s_red[HEAD_MAX_BLOCKS];
    const int f = blockIdx.x, t = threadIdx.x;
    s_red[t] = t < nblk ? part[(long long)f * nblk + t] : 0.0;
    __syncthreads();
#pragma unroll
    for (int s = HEAD_MAX_BLOCKS / 2; s > 0; s >>= 1) {
        if (t < s) s_red[t] += s_red[t + s];
        __syncthreads();
    }
    if (t == 0) acc[f] += s_red[0] / n_out;
}

}  // namespace

extern "C" ew_status ew_im2col_frames_f16(const void* src, int src_kind, void* out, int n_img, int h_in, int w_in, int k, int stride, int pad,
                                          int h_out, int w_out, int ldk, int swap_rb, const float* first_affine, void* stream) {
    EW_REQUIRE(src && out, "ew_im2col_frames_f16: NULL pointer");
    EW_REQUIRE(src_kind == 1 || src_kind == 2, "ew_im2col_frames_f16: src_kind %d (1: uint8 NHWC frames, 2: fp32 NCHW frames)", src_kind);
    EW_REQUIRE(n_img > 0 && h_in > 0 && w_in > 0 && k > 0 && stride > 0 && pad >= 0 && pad < k,
               "ew_im2col_frames_f16: bad geometry (n %d, %d x %d x 3, k %d, stride %d, pad %d)", n_img, h_in, w_in, k, stride, pad);
    EW_REQUIRE(h_in + 2 * pad >= k && w_in + 2 * pad >= k && h_out == (h_in + 2 * pad - k) / stride + 1 && w_out == (w_in + 2 * pad - k) / stride + 1,
               "ew_im2col_frames_f16: output %d x %d is not floor((%d x %d + 2*%d - %d) / %d) + 1", h_out, w_out, h_in, w_in, pad, k, stride);
    EW_REQUIRE((long long)k * k * 3 <= ldk && ldk % 8 == 0, "ew_im2col_frames_f16: ldk = %d must be a multiple of 8 and >= k*k*C = %lld", ldk,
               (long long)k * k * 3);
    EW_REQUIRE((uintptr_t)out % 16 == 0, "ew_im2col_frames_f16: out must be 16-byte aligned");
    EW_REQUIRE((long long)h_in * w_in * 3 < (1LL << 31) && (long long)h_out * w_out < (1LL << 31), "ew_im2col_frames_f16: image too large");
    EW_REQUIRE(first_affine, "ew_im2col_frames_f16: frame sources take the six scaling constants");
    EW_REQUIRE(src_kind == 1 || (uintptr_t)src % 4 == 0, "ew_im2col_frames_f16: fp32 source must be 4-byte aligned");
    FirstAffine fa;
    for (int c = 0; c < 3; ++c) {
        fa.shift[c] = first_affine[c];
        fa.scale[c] = first_affine[3 + c];
        EW_REQUIRE(fa.scale[c] != 0.0f, "ew_im2col_frames_f16: scale[%d] is zero", c);
    }
    const long long total_vec = (long long)n_img * h_out * w_out * (ldk / 8);
    hipStream_t st = (hipStream_t)stream;
    if (src_kind == 1)
        hipLaunchKernelGGL(im2col_first_kernel<1>, dim3(grid_for(total_vec)), dim3(NT), 0, st, src, (f16*)out, total_vec, h_in, w_in, k, stride,
                           pad, h_out, w_out, ldk / 8, k * k * 3, swap_rb ? 1 : 0, fa);
    else
        hipLaunchKernelGGL(im2col_first_kernel<2>, dim3(grid_for(total_vec)), dim3(NT), 0, st, src, (f16*)out, total_vec, h_in, w_in, k, stride,
                           pad, h_out, w_out, ldk / 8, k * k * 3, swap_rb ? 1 : 0, fa);
    return ew_check_launch("im2col_first_kernel");
}

extern "C" size_t ew_lpips_head_workspace_bytes(int F, int h, int w, int C) {
    if (F <= 0 || h <= 0 || w <= 0 || C <= 0) return 0;
    return (size_t)F * head_blocks(h, w, C) * sizeof(double);
}

extern "C" ew_status ew_lpips_head(const void* fa, const void* fb, const float* lin, const double* wy, const double* wx, int F, int h, int w,
                                   int C, double n_out, double* acc, void* workspace, void* stream) {
    EW_REQUIRE(fa && fb && lin && wy && wx && acc && workspace, "ew_lpips_head: NULL pointer");
    EW_REQUIRE(F > 0 && F <= 65535 && h > 0 && w > 0 && (long long)h * w < (1LL << 30), "ew_lpips_head: F, h, w = %d, %d, %d out of range", F, h, w);
    EW_REQUIRE(C > 0 && C % 8 == 0 && C <= 512, "ew_lpips_head: C = %d must be a multiple of 8, at most 512", C);
    EW_REQUIRE(n_out > 0.0, "ew_lpips_head: n_out (the H * W of the upsampled map) must be positive");
    EW_REQUIRE((uintptr_t)fa % 16 == 0 && (uintptr_t)fb % 16 == 0 && (uintptr_t)workspace % 8 == 0 && (uintptr_t)acc % 8 == 0 &&
                   (uintptr_t)wy % 8 == 0 && (uintptr_t)wx % 8 == 0,
               "ew_lpips_head: features must be 16-byte, the fp64 vectors 8-byte aligned");
    const int nblk = head_blocks(h, w, C);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    const dim3 grid(nblk, F);
#define EW_HEAD(L) hipLaunchKernelGGL(lpips_head_kernel<L>, grid, dim3(NT), 0, st, (const f16*)fa, (const f16*)fb, lin, wy, wx, h, w, C, part)
    switch (head_lpp_host(C)) {
    case 8: EW_HEAD(8); break;
    case 32: EW_HEAD(32); break;
    default: EW_HEAD(64); break;
    }
#undef EW_HEAD
    ew_status s = ew_check_launch("lpips_head_kernel");
    if (s != EW_OK) return s;
    hipLaunchKernelGGL(lpips_head_reduce_kernel, dim3(F), dim3(HEAD_MAX_BLOCKS), 0, st, part, nblk, n_out, acc);
    return ew_check_launch("lpips_head_reduce_kernel");
}
