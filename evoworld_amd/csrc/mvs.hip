// mvs.hip -- plane-sweep multi-view stereo on posed perspective views (ABI 20, symbols added without a bump): a
// weight-free depth source for the N-segment loop, standing in for the depth network of unified_loop_consistency.py:336-368.
// fp32 throughout in a fixed operation order (compiled with -ffp-contract=off like its neighbours), restated by tests/mvs_ref.py.
//
//   ew_mvs_luma_u8       (77 R + 150 G + 29 B + 128) >> 8 per pixel, grid-stride.
//   ew_mvs_plane_sweep   one workgroup of 256 threads owns a 32 x 8 tile of one reference view.  The tile's grey levels plus a halo of
//                        r pixels sit in LDS as floats.  Per plane: every thread warps its share of the halo'd tile into each present
//                        source and writes the SUM over the sources of the absolute differences to LDS (ad); a row pass adds the
//                        2r + 1 horizontal taps (rs), a column pass the 2r + 1 vertical ones -- the box filter of the patch cost, which
//                        commutes with the mean over the sources because a source is present for a whole view.  The four lowest costs,
//                        the winner's two neighbours and the previous plane's cost stay in registers, so the volume is never stored.
//                        Two workgroup barriers per plane; no atomics, no communication between workgroups, every loop bound an argument.
//   ew_mvs_plane_sweep_volume   the same tile kernel instantiated with VOLUME = true: the same C(k), quantised and staged in LDS
//                        (mvs_volume.h) so that the uint16 [n,H,W,D] volume is written in runs of hypotheses per pixel -- the input of the
//                        opt-in semi-global aggregation (mvs_sgm.hip).
//   ew_mvs_consistency   per pixel: lift, move into each present source with the relative pose, compare with the source's depth at the
//                        nearest pixel; the confidence is zeroed in place where fewer than min_consistent sources agree.
#include "common.h"
#include "mvs_volume.h"

namespace {

constexpr int NT = 256;
constexpr int TW = 32, TH = 8;                     // tile of one workgroup
constexpr int RMAX = 3;
constexpr int HW_MAX = TW + 2 * RMAX, HH_MAX = TH + 2 * RMAX;
static_assert(NT == 256 && TW == 32 && TH == 8, "mvs_volume.h stages the costs of this tile");

__global__ __launch_bounds__(NT) void luma_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ grey, long long n) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const uint8_t* p = rgb + 3 * i;
        grey[i] = (uint8_t)((77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8);
    }
}

// |ref - bilinear(src at H (x, y, 1))|, or oob where the sample is behind the source or leaves [0, W-1] x [0, H-1]
__device__ __forceinline__ float warped_ad(const uint8_t* __restrict__ src, const float* __restrict__ h, float x, float y, float ref,
                                           int H, int W, float oob) {
    const float q0 = (h[0] * x + h[1] * y) + h[2];
    const float q1 = (h[3] * x + h[4] * y) + h[5];
    const float q2 = (h[6] * x + h[7] * y) + h[8];
    if (!(q2 > 0.0f)) return oob;
    const float sx = q0 / q2, sy = q1 / q2;
    if (!(sx >= 0.0f && sx <= (float)(W - 1) && sy >= 0.0f && sy <= (float)(H - 1))) return oob;
    const float x0f = floorf(sx), y0f = floorf(sy);
    const float ax = sx - x0f, ay = sy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1;
    const int y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const uint8_t* r0 = src + (long long)y0 * W;
    const uint8_t* r1 = src + (long long)y1 * W;
    const float v00 = r0[x0], v01 = r0[x1], v10 = r1[x0], v11 = r1[x1];
    const float top = v00 * (1.0f - ax) + v01 * ax;
    const float bot = v10 * (1.0f - ax) + v11 * ax;
    return fabsf(ref - (top * (1.0f - ay) + bot * ay));
}

// VOLUME = false: the fused sweep (ew_mvs_plane_sweep), f = blockIdx.z.  VOLUME = true: the same C(k), quantised and stored
// (ew_mvs_plane_sweep_volume): f = view_begin + blockIdx.z, `vol` [gridDim.z,H,W,D]; the four output planes are not touched.
template <bool VOLUME>
__global__ __launch_bounds__(NT) void plane_sweep_kernel(const uint8_t* __restrict__ grey, const float* __restrict__ homog,
                                                         const int* __restrict__ src_index, const float* __restrict__ inv_depth,
                                                         float* __restrict__ depth, float* __restrict__ conf, int* __restrict__ winner,
                                                         float* __restrict__ win_cost, int F, int H, int W, int S, int D, int r, float oob,
                                                         uint16_t* __restrict__ vol, float cost_scale, int view_begin) {
    __shared__ float s_ref[HH_MAX * HW_MAX];       // the reference tile with its halo
    __shared__ float s_ad[HH_MAX * HW_MAX];        // per plane: the sum over the sources of the absolute differences
    __shared__ float s_rs[HH_MAX * TW];            // per plane: s_ad summed over the 2r + 1 horizontal taps
    const int t = threadIdx.x;
    const int f = (VOLUME ? view_begin : 0) + blockIdx.z;
    const int x_org = blockIdx.x * TW - r, y_org = blockIdx.y * TH - r;       // image position of the halo'd tile's corner
    const int hw = TW + 2 * r, hh = TH + 2 * r;
    const long long plane = (long long)H * W;
    const uint8_t* ref_img = grey + f * plane;

    for (int i = t; i < hh * hw; i += NT) {
        const int ly = i / hw, lx = i - ly * hw;
        const int x = x_org + lx, y = y_org + ly;
        s_ref[i] = (x >= 0 && x < W && y >= 0 && y < H) ? (float)ref_img[(long long)y * W + x] : 0.0f;
    }
    int n_src = 0;                                 // present sources: an index outside [0, F) is absent
    for (int s = 0; s < S; ++s) {
        const int si = src_index[f * S + s];
        n_src += (si >= 0 && si < F) ? 1 : 0;
    }
    __syncthreads();

    const int tx = t & (TW - 1), ty = t / TW;
    const int px = blockIdx.x * TW + tx, py = blockIdx.y * TH + ty;
    const bool live = px < W && py < H;
    // taps of the window that lie inside the reference image
    const int cx = (px + r < W ? px + r : W - 1) - (px - r > 0 ? px - r : 0) + 1;
    const int cy = (py + r < H ? py + r : H - 1) - (py - r > 0 ? py - r : 0) + 1;
    const float denom = (float)(cx * cy) * (float)(n_src > 0 ? n_src : 1);

    // the four lowest (cost, plane) pairs in ascending order, ties to the lower plane
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
    int k0 = -1, k1 = -1, k2 = -1, k3 = -1;
    float prev = 0.0f, left = 0.0f, right = 0.0f;  // C(k - 1); C(k0 - 1) and C(k0 + 1) of the running winner
    bool has_left = false, has_right = false;

    for (int k = 0; k < D; ++k) {
        for (int i = t; i < hh * hw; i += NT) {
            const int ly = i / hw, lx = i - ly * hw;
            const int x = x_org + lx, y = y_org + ly;
            float sum = 0.0f;
            if (x >= 0 && x < W && y >= 0 && y < H) {
                const float ref = s_ref[i];
                for (int s = 0; s < S; ++s) {
                    const int si = src_index[f * S + s];
                    if (si < 0 || si >= F) continue;
                    const float* h = homog + (((long long)f * S + s) * D + k) * 9;
                    sum += warped_ad(grey + si * plane, h, (float)x, (float)y, ref, H, W, oob);
                }
            }
            s_ad[i] = sum;
        }
        __syncthreads();
        for (int i = t; i < hh * TW; i += NT) {
            const int ly = i / TW, lx = i - ly * TW;
            const float* a = s_ad + ly * hw + lx;
            float sum = 0.0f;
            for (int d = 0; d <= 2 * r; ++d) sum += a[d];
            s_rs[i] = sum;
        }
        __syncthreads();                           // also orders this plane's reads of s_ad before the next plane's writes
        float c = 0.0f;
        for (int d = 0; d <= 2 * r; ++d) c += s_rs[(ty + d) * TW + tx];
        c = c / denom;
        // s_rs is written again only behind the next plane's first barrier
        if constexpr (VOLUME) {
            ew_mvs_stage_cost(c, cost_scale, k, D, vol + (long long)blockIdx.z * plane * D, H, W);
            continue;
        }

        if (has_left && !has_right && k == k0 + 1) { right = c; has_right = true; }
        if (c < b0) {
            b3 = b2; k3 = k2; b2 = b1; k2 = k1; b1 = b0; k1 = k0; b0 = c; k0 = k;
            left = prev; has_left = true; has_right = false;
        } else if (c < b1) {
            b3 = b2; k3 = k2; b2 = b1; k2 = k1; b1 = c; k1 = k;
        } else if (c < b2) {
            b3 = b2; k3 = k2; b2 = c; k2 = k;
        } else if (c < b3) {
            b3 = c; k3 = k;
        }
        prev = c;
    }
    if (VOLUME || !live) return;

    if (k0 < 0) { k0 = 0; b0 = prev; has_right = false; }          // every cost a NaN (non-finite homographies): plane 0, no refinement
    const float* invd = inv_depth + (long long)f * D;
    float inv = invd[k0];
    if (k0 > 0 && k0 < D - 1 && has_right) {
        const float curv = (left + right) - 2.0f * b0;
        if (curv > 0.0f) {
            float off = 0.5f * (left - right) / curv;
            off = fminf(fmaxf(off, -0.5f), 0.5f);
            inv = off >= 0.0f ? inv + off * (invd[k0 + 1] - inv) : inv + (-off) * (invd[k0 - 1] - inv);
        }
    }
    // runner-up: the lowest cost among the planes more than one step from the winner; it is among the four lowest
    float c2 = 0.0f;
    bool has_c2 = false;
    if (k1 >= 0 && abs(k1 - k0) > 1) { c2 = b1; has_c2 = true; }
    else if (k2 >= 0 && abs(k2 - k0) > 1) { c2 = b2; has_c2 = true; }
    else if (k3 >= 0 && abs(k3 - k0) > 1) { c2 = b3; has_c2 = true; }
    const long long o = f * plane + (long long)py * W + px;
    depth[o] = 1.0f / inv;
    conf[o] = (has_c2 && n_src > 0) ? (c2 - b0) / fmaxf(c2, 1e-6f) : 0.0f;
    winner[o] = k0;
    win_cost[o] = b0;
}

__global__ __launch_bounds__(NT) void consistency_kernel(const float* __restrict__ depth, const float* __restrict__ rel_pose,
                                                         const int* __restrict__ src_index, float* __restrict__ conf, int F, int H, int W,
                                                         int S, float fx, float fy, float cx, float cy, float rel_tol, int min_consistent) {
    const long long plane = (long long)H * W, total = (long long)F * plane;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int f = (int)(i / plane);
        const int p = (int)(i - f * plane);
        const int y = p / W, x = p - y * W;
        const float z = depth[i];
        const float xc = ((float)x - cx) * z / fx;
        const float yc = ((float)y - cy) * z / fy;
        int agree = 0;
        for (int s = 0; s < S; ++s) {
            const int si = src_index[f * S + s];
            if (si < 0 || si >= F) continue;
            const float* T = rel_pose + ((long long)f * S + s) * 12;
            const float X = ((T[0] * xc + T[1] * yc) + T[2] * z) + T[3];
            const float Y = ((T[4] * xc + T[5] * yc) + T[6] * z) + T[7];
            const float Z = ((T[8] * xc + T[9] * yc) + T[10] * z) + T[11];
            if (!(Z > 0.0f)) continue;
            const float u = floorf((fx * X / Z + cx) + 0.5f), v = floorf((fy * Y / Z + cy) + 0.5f);
            if (!(u >= 0.0f && u <= (float)(W - 1) && v >= 0.0f && v <= (float)(H - 1))) continue;
            const float zs = depth[si * plane + (long long)(int)v * W + (int)u];
            agree += fabsf(zs - Z) <= rel_tol * Z ? 1 : 0;
        }
        if (agree < min_consistent) conf[i] = 0.0f;
    }
}

unsigned stride_grid(long long n) {
    const long long blocks = (n + NT - 1) / NT;
    return (unsigned)(blocks < 65536 ? (blocks > 0 ? blocks : 1) : 65536);
}

}  // namespace

extern "C" ew_status ew_mvs_luma_u8(const uint8_t* rgb, uint8_t* grey, int F, int H, int W, void* stream) {
    EW_REQUIRE(rgb && grey, "ew_mvs_luma_u8: NULL pointer");
    EW_REQUIRE(F >= 1 && H >= 1 && W >= 1, "ew_mvs_luma_u8: F = %d, H = %d, W = %d must be positive", F, H, W);
    const long long n = (long long)F * H * W;
    hipLaunchKernelGGL(luma_kernel, dim3(stride_grid(n)), dim3(NT), 0, (hipStream_t)stream, rgb, grey, n);
    return ew_check_launch("mvs luma_kernel");
}

extern "C" ew_status ew_mvs_plane_sweep(const uint8_t* grey, const float* homographies, const int* src_index, const float* inv_depth,
                                        float* depth, float* conf, int* winner, float* winner_cost, int F, int H, int W, int S, int D,
                                        int patch_radius, float oob_cost, void* stream) {
    EW_REQUIRE(grey && homographies && src_index && inv_depth && depth && conf && winner && winner_cost, "ew_mvs_plane_sweep: NULL pointer");
    EW_REQUIRE(F >= 1 && F <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1LL << 31),
               "ew_mvs_plane_sweep: F = %d must be 1 .. 65535, H = %d and W = %d positive with H W below 2^31", F, H, W);
    EW_REQUIRE(S >= 1 && D >= 1 && (long long)F * S * D < (1LL << 31), "ew_mvs_plane_sweep: S = %d and D = %d must be positive, F S D below 2^31", S, D);
    EW_REQUIRE(patch_radius >= 0 && patch_radius <= RMAX, "ew_mvs_plane_sweep: patch_radius = %d must be 0 .. %d", patch_radius, RMAX);
    EW_REQUIRE((((uintptr_t)homographies | (uintptr_t)src_index | (uintptr_t)inv_depth | (uintptr_t)depth | (uintptr_t)conf | (uintptr_t)winner |
                 (uintptr_t)winner_cost) & 3) == 0, "ew_mvs_plane_sweep: the fp32 and int32 arrays must be 4-byte aligned");
    const unsigned gx = (unsigned)((W + TW - 1) / TW), gy = (unsigned)((H + TH - 1) / TH);
    EW_REQUIRE(gy <= 65535, "ew_mvs_plane_sweep: H = %d gives more than 65535 tile rows", H);
    hipLaunchKernelGGL(plane_sweep_kernel<false>, dim3(gx, gy, (unsigned)F), dim3(NT), 0, (hipStream_t)stream, grey, homographies, src_index,
                       inv_depth, depth, conf, winner, winner_cost, F, H, W, S, D, patch_radius, oob_cost, (uint16_t*)nullptr, 0.0f, 0);
    return ew_check_launch("mvs plane_sweep_kernel");
}

extern "C" ew_status ew_mvs_plane_sweep_volume(const uint8_t* grey, const float* homographies, const int* src_index, const float* inv_depth,
                                               uint16_t* cost, int F, int H, int W, int S, int D, int patch_radius, float oob_cost,
                                               float cost_scale, int view_begin, int n_views, void* stream) {
    EW_REQUIRE(grey && homographies && src_index && inv_depth && cost, "ew_mvs_plane_sweep_volume: NULL pointer");
    EW_REQUIRE(F >= 1 && F <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1LL << 31),
               "ew_mvs_plane_sweep_volume: F = %d must be 1 .. 65535, H = %d and W = %d positive with H W below 2^31", F, H, W);
    EW_REQUIRE(S >= 1 && D >= 1 && (long long)F * S * D < (1LL << 31),
               "ew_mvs_plane_sweep_volume: S = %d and D = %d must be positive, F S D below 2^31", S, D);
    EW_REQUIRE(patch_radius >= 0 && patch_radius <= RMAX, "ew_mvs_plane_sweep_volume: patch_radius = %d must be 0 .. %d", patch_radius, RMAX);
    EW_REQUIRE(cost_scale > 0.0f && cost_scale < INFINITY, "ew_mvs_plane_sweep_volume: cost_scale = %g must be positive and finite",
               (double)cost_scale);
    EW_REQUIRE(view_begin >= 0 && n_views >= 1 && n_views <= F - view_begin,
               "ew_mvs_plane_sweep_volume: views %d .. %d + %d - 1 must lie in [0, F = %d)", view_begin, view_begin, n_views, F);
    EW_REQUIRE((((uintptr_t)homographies | (uintptr_t)src_index | (uintptr_t)inv_depth) & 3) == 0 && ((uintptr_t)cost & 1) == 0,
               "ew_mvs_plane_sweep_volume: the fp32 and int32 arrays must be 4-byte aligned, the volume 2-byte aligned");
    const unsigned gx = (unsigned)((W + TW - 1) / TW), gy = (unsigned)((H + TH - 1) / TH);
    EW_REQUIRE(gy <= 65535, "ew_mvs_plane_sweep_volume: H = %d gives more than 65535 tile rows", H);
    hipLaunchKernelGGL(plane_sweep_kernel<true>, dim3(gx, gy, (unsigned)n_views), dim3(NT), EW_MVS_STAGE_BYTES, (hipStream_t)stream, grey,
                       homographies, src_index, inv_depth, (float*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr, F, H, W, S, D,
                       patch_radius, oob_cost, cost, cost_scale, view_begin);
    return ew_check_launch("mvs plane_sweep_kernel<volume>");
}

extern "C" ew_status ew_mvs_consistency(const float* depth, const float* rel_pose, const int* src_index, float* conf, int F, int H, int W,
                                        int S, float fx, float fy, float cx, float cy, float rel_tol, int min_consistent, void* stream) {
    EW_REQUIRE(depth && rel_pose && src_index && conf, "ew_mvs_consistency: NULL pointer");
    EW_REQUIRE(F >= 1 && H >= 1 && W >= 1 && S >= 1 && (long long)H * W < (1LL << 31) && (long long)F * S < (1LL << 27),
               "ew_mvs_consistency: F = %d, H = %d, W = %d, S = %d must be positive, H W below 2^31 and F S below 2^27", F, H, W, S);
    EW_REQUIRE(fx > 0.0f && fy > 0.0f && rel_tol >= 0.0f, "ew_mvs_consistency: fx = %g and fy = %g must be positive, rel_tol = %g not negative",
               (double)fx, (double)fy, (double)rel_tol);
    EW_REQUIRE((((uintptr_t)depth | (uintptr_t)rel_pose | (uintptr_t)src_index | (uintptr_t)conf) & 3) == 0,
               "ew_mvs_consistency: the arrays must be 4-byte aligned");
    hipLaunchKernelGGL(consistency_kernel, dim3(stride_grid((long long)F * H * W)), dim3(NT), 0, (hipStream_t)stream, depth, rel_pose, src_index,
                       conf, F, H, W, S, fx, fy, cx, cy, rel_tol, min_consistent);
    return ew_check_launch("mvs consistency_kernel");
}
