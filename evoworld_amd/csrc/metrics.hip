// metrics.hip -- per-frame PSNR / SSIM of video pairs and the 8-bit map of the ground-truth segment dumps (ABI 12); their
// row-weighted forms for equirectangular frames, WS-PSNR / WS-SSIM (ABI 18: ew_video_metrics_ws, no counterpart in the reference).
// Reference: evoworld/metrics/other_metrics/calculate_psnr.py:6-15, calculate_ssim.py:6-40 (run by calculate_all_metrics.py:222-226
// on uint8 / 255.0), unified_loop_consistency.py:87-93,437-439 (tensor_to_pil of the ground-truth frames).
// Compiled with -ffp-contract=off: the float32 difference and square of the PSNR, and the fp64 moment arithmetic of the SSIM map,
// are the reference's separate roundings.
//
// One block per 24x32 tile of a frame: the frame pair's tile plus a 5-pixel halo on the right and bottom is staged in LDS one
// channel at a time; a horizontal 11-tap pass writes the five moment rows (x, y, x^2, y^2, xy) in fp64, a vertical pass finishes
// the window and evaluates the SSIM map at the tile's valid outputs.  The tile's own 24x32 pixels (the whole frame over all tiles)
// give the squared error.  Partial sums go to the workspace in a fixed tree order, and a second kernel sums each frame's tiles in
// a fixed order: no atomics, two calls are bit-identical.
// The weighted form is the same kernel under a template flag: the tile's rows of the caller's fp64 weights are staged next to the
// pixels, a squared error is multiplied by its row's weight and an SSIM value by the weight of its window's CENTRE row (output row
// i sits on image row i + 5), both in fp64 before the sum.  The planar instantiation has no weighted operation in it.
#include "common.h"
#include <math.h>

namespace {

constexpr int TH = 24, TW = 32;                  // SSIM outputs (and SSE pixels) per tile
constexpr int IH = TH + 10, IW = TW + 10;        // staged input rows / columns
constexpr int NT = 256;
constexpr int NQ = 4;                            // partials per tile: SSIM map sum of channels 0..2, SSE

struct U8Table { float v[256]; };                // float32(k) / 255.0f, correctly rounded (host)
struct Gauss11 { double g[11]; };                // cv2.getGaussianKernel(11, 1.5) in double (host)
struct Map8 { unsigned char m[256]; };

__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

template <bool WS>
__global__ __launch_bounds__(NT) void metrics_tile_kernel(const void* __restrict__ a, const void* __restrict__ b, int layout, int C,
                                                          int H, int W, int tiles_x, int do_sse, int do_ssim, U8Table tab,
                                                          Gauss11 gk, const double* __restrict__ row_w, double* __restrict__ part) {
    __shared__ float s_tab[256];
    __shared__ float s_a[IH][IW], s_b[IH][IW];
    __shared__ double s_h[5][IH][TW];
    __shared__ double s_red[NT];
    __shared__ double s_g[11];                             // the taps from LDS: held in SGPRs they spilled
    __shared__ double s_w[WS ? IH : 1];                    // weights of the staged rows (image rows oy .. oy + IH - 1; 0 below the frame)
    const int t = threadIdx.x;
    const int tile = blockIdx.x, f = blockIdx.y;
    const int oy = (tile / tiles_x) * TH, ox = (tile % tiles_x) * TW;
    const int Ho = H - 10, Wo = W - 10;
    s_tab[t] = tab.v[t];
    if (t < 11) s_g[t] = gk.g[t];
    if constexpr (WS) {
        if (t < IH) s_w[t] = oy + t < H ? row_w[oy + t] : 0.0;
    }
    double sse = 0.0;
    double ssim_c[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        __syncthreads();                                   // s_tab, s_w ready / previous channel's s_a, s_b, s_h consumed
        for (int i = t; i < IH * IW; i += NT) {
            const int r = i / IW, q = i - r * IW;
            const int y = oy + r, x = ox + q;
            float va = 0.f, vb = 0.f;
            if (y < H && x < W) {
                if (layout == 0) {
                    const long long e = (((long long)f * H + y) * W + x) * C + c;
                    va = s_tab[((const uint8_t*)a)[e]];
                    vb = s_tab[((const uint8_t*)b)[e]];
                } else {
                    const long long e = (((long long)f * C + c) * H + y) * W + x;
                    va = ((const float*)a)[e];
                    vb = ((const float*)b)[e];
                }
            }
            s_a[r][q] = va;
            s_b[r][q] = vb;
        }
        __syncthreads();
        if (do_sse) {                                      // the tile's own pixels: d = a - b, d*d in float32, summed in fp64
            for (int i = t; i < TH * TW; i += NT) {
                const int r = i / TW, q = i - r * TW;
                if (oy + r < H && ox + q < W) {
                    const float d = s_a[r][q] - s_b[r][q];
                    const float d2 = d * d;
                    if constexpr (WS) sse += s_w[r] * (double)d2;
                    else sse += (double)d2;
                }
            }
        }
        if (!do_ssim) continue;
        for (int i = t; i < IH * TW; i += NT) {            // horizontal taps of the five moments
            const int r = i / TW, q = i - r * TW;
            double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
            if (oy + r < H && ox + q < Wo) {
#pragma unroll
                for (int j = 0; j < 11; ++j) {
                    const double x = (double)s_a[r][q + j], y = (double)s_b[r][q + j], g = s_g[j];
                    hx += g * x;
                    hy += g * y;
                    hxx += g * (x * x);
                    hyy += g * (y * y);
                    hxy += g * (x * y);
                }
            }
            s_h[0][r][q] = hx; s_h[1][r][q] = hy; s_h[2][r][q] = hxx; s_h[3][r][q] = hyy; s_h[4][r][q] = hxy;
        }
        __syncthreads();
        double acc = 0.0;
        for (int i = t; i < TH * TW; i += NT) {            // vertical taps and the SSIM map at the valid outputs
            const int r = i / TW, q = i - r * TW;
            if (oy + r < Ho && ox + q < Wo) {
                double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
                for (int j = 0; j < 11; ++j) {
                    const double g = s_g[j];
                    m1 += g * s_h[0][r + j][q];
                    m2 += g * s_h[1][r + j][q];
                    e11 += g * s_h[2][r + j][q];
                    e22 += g * s_h[3][r + j][q];
                    e12 += g * s_h[4][r + j][q];
                }
                const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
                const double m1s = m1 * m1, m2s = m2 * m2, m12 = m1 * m2;
                const double s1 = e11 - m1s, s2 = e22 - m2s, s12 = e12 - m12;
                const double v = ((2.0 * m12 + C1) * (2.0 * s12 + C2)) / ((m1s + m2s + C1) * (s1 + s2 + C2));
                if constexpr (WS) acc += s_w[r + 5] * v;   // the window's centre row
                else acc += v;
            }
        }
        ssim_c[c] = acc;
    }
    double* p = part + ((long long)f * gridDim.x + tile) * NQ;
    for (int c = 0; c < 3; ++c) {
        const double s = do_ssim && c < C ? block_sum(ssim_c[c], s_red) : 0.0;
        if (t == 0) p[c] = s;
    }
    const double s = do_sse ? block_sum(sse, s_red) : 0.0;
    if (t == 0) p[3] = s;
}

// one block per frame: the tiles' partials in a fixed order -> sse[f] = sum of squared errors, ssim[f] = mean over channels of the
// mean SSIM map (np.array(ssims).mean() of per-channel ssim_map.mean(): ((m0 + m1) + m2) / 3).  With row_w (the weighted form) the
// divisor is n_valid (there W - 10, the windows per row) times the weights of the H - 10 centre rows, summed here in a fixed order.
__global__ __launch_bounds__(NT) void metrics_reduce_kernel(const double* __restrict__ part, int ntiles, int C, double n_valid,
                                                            const double* __restrict__ row_w, int H, double* __restrict__ sse,
                                                            double* __restrict__ ssim) {
    __shared__ double s_red[NT];
    const int f = blockIdx.x, t = threadIdx.x;
    if (row_w && ssim) {
        double v = 0.0;
        for (int i = t; i < H - 10; i += NT) v += row_w[i + 5];
        n_valid = n_valid * block_sum(v, s_red);
    }
    const double* p = part + (long long)f * ntiles * NQ;
    double tot[NQ];
    for (int k = 0; k < NQ; ++k) {
        double v = 0.0;
        if ((k < C && ssim) || (k == 3 && sse))
            for (int i = t; i < ntiles; i += NT) v += p[(long long)i * NQ + k];
        tot[k] = block_sum(v, s_red);
    }
    if (t == 0) {
        if (sse) sse[f] = tot[3];
        if (ssim) {
            double m = tot[0] / n_valid;
            for (int k = 1; k < C; ++k) m += tot[k] / n_valid;
            ssim[f] = m / (double)C;
        }
    }
}

__global__ __launch_bounds__(NT) void map_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long n, Map8 map) {
    __shared__ unsigned char s_m[256];
    s_m[threadIdx.x] = map.m[threadIdx.x];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) dst[i] = s_m[src[i]];
}

inline int tiles_of(int H, int W, int* tx) {
    *tx = ew_cdiv(W, TW);
    return *tx * ew_cdiv(H, TH);
}

}  // namespace

extern "C" size_t ew_video_metrics_workspace_bytes(int F, int C, int H, int W) {
    (void)C;
    if (F <= 0 || H <= 0 || W <= 0) return 0;
    int tx;
    return (size_t)F * tiles_of(H, W, &tx) * NQ * sizeof(double);
}

namespace {

// both entry points: `name` prefixes the refusals; `weighted` selects the row-weighted instantiation, which needs row_w
ew_status video_metrics_launch(const char* name, const void* a, const void* b, int layout, int F, int C, int H, int W, int what,
                               const double* row_w, bool weighted, double* sse, double* ssim, void* workspace, void* stream) {
    EW_REQUIRE(a && b && workspace, "%s: NULL input or workspace", name);
    EW_REQUIRE(layout == 0 || layout == 1, "%s: layout %d (0: uint8 [F,H,W,C], 1: fp32 [F,C,H,W])", name, layout);
    EW_REQUIRE(C == 1 || C == 3, "%s: C = %d (the reference's SSIM takes 1 or 3 channels)", name, C);
    EW_REQUIRE(F > 0 && H > 0 && W > 0, "%s: F, H, W = %d, %d, %d must be positive", name, F, H, W);
    EW_REQUIRE(what >= 1 && what <= 3, "%s: what = %d (bit 0: SSE, bit 1: SSIM)", name, what);
    EW_REQUIRE(!weighted || row_w, "%s: NULL row_w (one fp64 weight per image row, on the device)", name);
    const int do_sse = what & 1, do_ssim = (what >> 1) & 1;
    EW_REQUIRE(!do_sse || sse, "%s: SSE asked for with a NULL output", name);
    EW_REQUIRE(!do_ssim || ssim, "%s: SSIM asked for with a NULL output", name);
    EW_REQUIRE(!do_ssim || (H >= 11 && W >= 11), "%s: SSIM needs H, W >= 11 (got %d x %d)", name, H, W);
    EW_REQUIRE((long long)H * W <= (1LL << 31) / 4, "%s: frame of %d x %d too large", name, H, W);
    U8Table tab;
    for (int k = 0; k < 256; ++k) tab.v[k] = (float)k / 255.0f;
    // cv2.getGaussianKernel(11, 1.5) for CV_64F: t_i = exp(-0.5 / sigma^2 * x_i^2), x_i = i - 5, then t_i * (1 / sum t)
    Gauss11 gk;
    double sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        const double x = i - 5.0;
        gk.g[i] = exp((-0.5 / (1.5 * 1.5)) * x * x);
        sum += gk.g[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < 11; ++i) gk.g[i] *= sum;
    int tiles_x;
    const int ntiles = tiles_of(H, W, &tiles_x);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    if (weighted)
        hipLaunchKernelGGL(metrics_tile_kernel<true>, dim3(ntiles, F), dim3(NT), 0, st, a, b, layout, C, H, W, tiles_x, do_sse, do_ssim, tab,
                           gk, row_w, part);
    else
        hipLaunchKernelGGL(metrics_tile_kernel<false>, dim3(ntiles, F), dim3(NT), 0, st, a, b, layout, C, H, W, tiles_x, do_sse, do_ssim, tab,
                           gk, (const double*)nullptr, part);
    ew_status s = ew_check_launch("metrics_tile_kernel");
    if (s != EW_OK) return s;
    // planar: the valid outputs of a frame; weighted: the windows per row, times the centre rows' weights in the reduce kernel
    const double n_valid = !do_ssim ? 1.0 : weighted ? (double)(W - 10) : (double)(H - 10) * (double)(W - 10);
    hipLaunchKernelGGL(metrics_reduce_kernel, dim3(F), dim3(NT), 0, st, part, ntiles, C, n_valid, weighted ? row_w : (const double*)nullptr, H,
                       do_sse ? sse : nullptr, do_ssim ? ssim : nullptr);
    return ew_check_launch("metrics_reduce_kernel");
}

}  // namespace

extern "C" ew_status ew_video_metrics(const void* a, const void* b, int layout, int F, int C, int H, int W, int what, double* sse,
                                      double* ssim, void* workspace, void* stream) {
    return video_metrics_launch("ew_video_metrics", a, b, layout, F, C, H, W, what, nullptr, false, sse, ssim, workspace, stream);
}

extern "C" size_t ew_video_metrics_ws_workspace_bytes(int F, int C, int H, int W) { return ew_video_metrics_workspace_bytes(F, C, H, W); }

extern "C" ew_status ew_video_metrics_ws(const void* a, const void* b, int layout, int F, int C, int H, int W, int what,
                                         const double* row_w, double* wsse, double* wssim, void* workspace, void* stream) {
    return video_metrics_launch("ew_video_metrics_ws", a, b, layout, F, C, H, W, what, row_w, true, wsse, wssim, workspace, stream);
}

extern "C" ew_status ew_gt_dump_map_u8(const uint8_t* src, uint8_t* dst, size_t n, void* stream) {
    EW_REQUIRE(src && dst, "ew_gt_dump_map_u8: NULL pointer");
    if (n == 0) return EW_OK;
    // the ground-truth frame as the reference dumps it: ToTensor (k / 255) -> x*2 - 1 -> tensor_to_pil: (x*0.5 + 0.5).clamp(0, 1)
    // .mul(255).byte(), each step one float32 rounding, the last a truncation
    Map8 map;
    for (int k = 0; k < 256; ++k) {
        const float v = (float)k / 255.0f;
        const float x = v * 2.0f - 1.0f;
        float y = x * 0.5f + 0.5f;
        y = y < 0.f ? 0.f : (y > 1.f ? 1.f : y);
        map.m[k] = (unsigned char)(int)(y * 255.0f);
    }
    long long blocks = ((long long)n + NT - 1) / NT;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(map_u8_kernel, dim3((int)blocks), dim3(NT), 0, (hipStream_t)stream, src, dst, (long long)n, map);
    return ew_check_launch("map_u8_kernel");
}
