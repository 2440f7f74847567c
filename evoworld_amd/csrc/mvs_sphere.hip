// mvs_sphere.hip -- sphere-sweep multi-view stereo on posed equirectangular panoramas (ABI 20, symbols added without a bump; DESIGN.md
// 4.9): the depth stage of mvs.hip without the 90-degree crop.  Concentric spheres around each panorama camera take the place of the planes,
// the warp goes through the sphere instead of a homography, and the lift is spherical.  fp32 throughout in a fixed operation order
// (compiled with -ffp-contract=off like mvs.hip), restated by tests/mvs_sphere_ref.py.
//
//   ew_mvs_sphere_sweep        one workgroup of 256 threads owns a 32 x 8 tile of one reference panorama.  A thread's (at most three) cells of
//                              the halo'd tile -- halo columns taken modulo We, halo rows outside the panorama empty -- do not depend on the
//                              hypothesis: their grey level and unit direction are computed once and stay in registers.  Per hypothesis: every
//                              thread moves its cells' points into each present source, maps them to the source's pixels (atan2f, asinf, one
//                              square root) and writes the SUM over the sources of the absolute differences to LDS (ad); a row pass adds the
//                              2r + 1 horizontal taps (rs), a column pass the 2r + 1 vertical ones.  The four lowest costs, the winner's two
//                              neighbours and the previous hypothesis' cost stay in registers, so the volume is never stored.  Two workgroup
//                              barriers per hypothesis; no atomics, no communication between workgroups, every loop bound an argument.
//   ew_mvs_sphere_sweep_volume the same tile kernel instantiated with VOLUME = true: the same C(k), quantised and staged in LDS
//                              (mvs_volume.h), written as the uint16 [n,He,We,D] volume the semi-global aggregation reads (mvs_sgm.hip).
//   ew_mvs_sphere_consistency  per pixel: lift along the pixel's direction, move into each present source with the relative pose, compare the
//                              point's distance there with the source's distance at the nearest pixel of its direction.
//   ew_pano_unproject          per pixel: R (dir dist) + t.
#include "common.h"
#include "mvs_volume.h"

namespace {

constexpr int NT = 256;
constexpr int TW = 32, TH = 8;                     // tile of one workgroup
constexpr int RMAX = 3;
constexpr int HW_MAX = TW + 2 * RMAX, HH_MAX = TH + 2 * RMAX;
constexpr int CELLS = (HW_MAX * HH_MAX + NT - 1) / NT;      // halo'd cells per thread at most: 3
static_assert(NT == 256 && TW == 32 && TH == 8, "mvs_volume.h stages the costs of this tile");
constexpr float PI_F = 3.14159265358979323846f;

// pixel (x, y) -> unit direction in the panorama camera (x right, y down, z forward): the inverse of the map of ew_equi2pers
__device__ __forceinline__ void pixel_dir(int x, int y, float Wf, float Hf, float& dx, float& dy, float& dz) {
    const float lon = (((float)x - Wf * 0.5f) - 0.5f) * ((2.0f * PI_F) / Wf);
    const float lat = (((float)y - Hf * 0.5f) - 0.5f) * (PI_F / Hf);
    const float cl = cosf(lat);
    dx = cl * sinf(lon);
    dy = sinf(lat);
    dz = cl * cosf(lon);
}

// point (X, Y, Z) of norm nrm (positive, finite) in a panorama camera -> continuous pixel index (u unwrapped, v unclamped)
__device__ __forceinline__ void dir_pixel(float X, float Y, float Z, float nrm, float Wf, float Hf, float& u, float& v) {
    const float lon = atan2f(X, Z);
    const float lat = asinf(fminf(fmaxf(Y / nrm, -1.0f), 1.0f));
    u = ((lon * Wf) / (2.0f * PI_F) + Wf * 0.5f) + 0.5f;
    v = ((lat * Hf) / PI_F + Hf * 0.5f) + 0.5f;
}

__device__ __forceinline__ int clampi(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }

// |ref - bilinear(src)| at the pixel the point P = d rad lands on in the source (T = R | t, reference camera -> source camera); 0 when
// the point sits on the source's centre or is not finite
__device__ __forceinline__ float warped_ad(const uint8_t* __restrict__ src, const float* __restrict__ T, float dx, float dy, float dz,
                                           float rad, float ref, int He, int We, float Wf, float Hf) {
    const float px = dx * rad, py = dy * rad, pz = dz * rad;
    const float X = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const float Y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    const float Z = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    const float nrm = sqrtf((X * X + Y * Y) + Z * Z);
    if (!(nrm > 0.0f && nrm < INFINITY)) return 0.0f;
    float u, v;
    dir_pixel(X, Y, Z, nrm, Wf, Hf, u, v);
    u = u - floorf(u / Wf) * Wf;
    v = fminf(fmaxf(v, 0.0f), (float)(He - 1));
    const float x0f = floorf(u), y0f = floorf(v);
    const float ax = u - x0f, ay = v - y0f;
    int x0 = (int)x0f;
    x0 = x0 >= We ? x0 - We : x0;
    x0 = clampi(x0, 0, We - 1);                    // never moves a finite index; keeps every read inside the panorama whatever the inputs
    const int y0 = clampi((int)y0f, 0, He - 1);
    const int x1 = x0 + 1 >= We ? 0 : x0 + 1;
    const int y1 = y0 + 1 >= He ? He - 1 : y0 + 1;
    const uint8_t* r0 = src + (long long)y0 * We;
    const uint8_t* r1 = src + (long long)y1 * We;
    const float v00 = r0[x0], v01 = r0[x1], v10 = r1[x0], v11 = r1[x1];
    const float top = v00 * (1.0f - ax) + v01 * ax;
    const float bot = v10 * (1.0f - ax) + v11 * ax;
    return fabsf(ref - (top * (1.0f - ay) + bot * ay));
}

// VOLUME = false: the fused sweep (ew_mvs_sphere_sweep), f = blockIdx.z.  VOLUME = true: the same C(k), quantised and stored
// (ew_mvs_sphere_sweep_volume): f = view_begin + blockIdx.z, `vol` [gridDim.z,He,We,D]; the four output planes are not touched.
template <bool VOLUME>
__global__ __launch_bounds__(NT) void sphere_sweep_kernel(const uint8_t* __restrict__ grey, const float* __restrict__ rel_pose,
                                                          const int* __restrict__ src_index, const float* __restrict__ inv_dist,
                                                          float* __restrict__ dist, float* __restrict__ conf, int* __restrict__ winner,
                                                          float* __restrict__ win_cost, int F, int He, int We, int S, int D, int r,
                                                          uint16_t* __restrict__ vol, float cost_scale, int view_begin) {
    __shared__ float s_ad[HH_MAX * HW_MAX];        // per hypothesis: the sum over the sources of the absolute differences
    __shared__ float s_rs[HH_MAX * TW];            // per hypothesis: s_ad summed over the 2r + 1 horizontal taps
    const int t = threadIdx.x;
    const int f = (VOLUME ? view_begin : 0) + blockIdx.z;
    const int x_org = blockIdx.x * TW - r, y_org = blockIdx.y * TH - r;       // panorama position of the halo'd tile's corner
    const int hw = TW + 2 * r, hh = TH + 2 * r;
    const long long plane = (long long)He * We;
    const uint8_t* ref_img = grey + f * plane;
    const float Wf = (float)We, Hf = (float)He;

    // this thread's cells of the halo'd tile: grey level and direction, once for all hypotheses
    float c_ref[CELLS], c_dx[CELLS], c_dy[CELLS], c_dz[CELLS];
    bool c_in[CELLS];
#pragma unroll
    for (int j = 0; j < CELLS; ++j) {
        const int i = t + j * NT;
        const int ly = i / hw, lx = i - ly * hw;
        const int y = y_org + ly;
        int x = (x_org + lx) % We;                 // columns wrap across the seam
        x = x < 0 ? x + We : x;
        c_in[j] = i < hh * hw && y >= 0 && y < He;
        c_ref[j] = 0.0f; c_dx[j] = 0.0f; c_dy[j] = 0.0f; c_dz[j] = 0.0f;
        if (c_in[j]) {
            c_ref[j] = (float)ref_img[(long long)y * We + x];
            pixel_dir(x, y, Wf, Hf, c_dx[j], c_dy[j], c_dz[j]);
        }
    }
    int n_src = 0;                                 // present sources: an index outside [0, F) is absent
    for (int s = 0; s < S; ++s) {
        const int si = src_index[f * S + s];
        n_src += (si >= 0 && si < F) ? 1 : 0;
    }

    const int tx = t & (TW - 1), ty = t / TW;
    const int px = blockIdx.x * TW + tx, py = blockIdx.y * TH + ty;
    const bool live = px < We && py < He;
    // rows of the window inside the panorama; all 2r + 1 columns always count
    const int cy = (py + r < He ? py + r : He - 1) - (py - r > 0 ? py - r : 0) + 1;
    const float denom = (float)((2 * r + 1) * cy) * (float)(n_src > 0 ? n_src : 1);
    const float* invd = inv_dist + (long long)f * D;

    // the four lowest (cost, hypothesis) pairs in ascending order, ties to the lower hypothesis
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
    int k0 = -1, k1 = -1, k2 = -1, k3 = -1;
    float prev = 0.0f, left = 0.0f, right = 0.0f;  // C(k - 1); C(k0 - 1) and C(k0 + 1) of the running winner
    bool has_left = false, has_right = false;

    for (int k = 0; k < D; ++k) {
        const float rad = 1.0f / invd[k];
#pragma unroll
        for (int j = 0; j < CELLS; ++j) {
            const int i = t + j * NT;
            if (i < hh * hw) {
                float sum = 0.0f;
                if (c_in[j]) {
                    for (int s = 0; s < S; ++s) {
                        const int si = src_index[f * S + s];
                        if (si < 0 || si >= F) continue;
                        sum += warped_ad(grey + si * plane, rel_pose + ((long long)f * S + s) * 12, c_dx[j], c_dy[j], c_dz[j], rad, c_ref[j],
                                         He, We, Wf, Hf);
                    }
                }
                s_ad[i] = sum;
            }
        }
        __syncthreads();
        for (int i = t; i < hh * TW; i += NT) {
            const int ly = i / TW, lx = i - ly * TW;
            const float* a = s_ad + ly * hw + lx;
            float sum = 0.0f;
            for (int d = 0; d <= 2 * r; ++d) sum += a[d];
            s_rs[i] = sum;
        }
        __syncthreads();                           // also orders this hypothesis' reads of s_ad before the next one's writes
        float c = 0.0f;
        for (int d = 0; d <= 2 * r; ++d) c += s_rs[(ty + d) * TW + tx];
        c = c / denom;
        // s_rs is written again only behind the next hypothesis' first barrier
        if constexpr (VOLUME) {
            ew_mvs_stage_cost(c, cost_scale, k, D, vol + (long long)blockIdx.z * plane * D, He, We);
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

    if (k0 < 0) { k0 = 0; b0 = prev; has_right = false; }          // every cost a NaN (non-finite poses): hypothesis 0, no refinement
    float inv = invd[k0];
    if (k0 > 0 && k0 < D - 1 && has_right) {
        const float curv = (left + right) - 2.0f * b0;
        if (curv > 0.0f) {
            float off = 0.5f * (left - right) / curv;
            off = fminf(fmaxf(off, -0.5f), 0.5f);
            inv = off >= 0.0f ? inv + off * (invd[k0 + 1] - inv) : inv + (-off) * (invd[k0 - 1] - inv);
        }
    }
    // runner-up: the lowest cost among the hypotheses more than one step from the winner; it is among the four lowest
    float c2 = 0.0f;
    bool has_c2 = false;
    if (k1 >= 0 && abs(k1 - k0) > 1) { c2 = b1; has_c2 = true; }
    else if (k2 >= 0 && abs(k2 - k0) > 1) { c2 = b2; has_c2 = true; }
    else if (k3 >= 0 && abs(k3 - k0) > 1) { c2 = b3; has_c2 = true; }
    const long long o = f * plane + (long long)py * We + px;
    dist[o] = 1.0f / inv;
    conf[o] = (has_c2 && n_src > 0) ? (c2 - b0) / fmaxf(c2, 1e-6f) : 0.0f;
    winner[o] = k0;
    win_cost[o] = b0;
}

__global__ __launch_bounds__(NT) void sphere_consistency_kernel(const float* __restrict__ dist, const float* __restrict__ rel_pose,
                                                                const int* __restrict__ src_index, float* __restrict__ conf, int F, int He,
                                                                int We, int S, float rel_tol, int min_consistent) {
    const long long plane = (long long)He * We, total = (long long)F * plane;
    const float Wf = (float)We, Hf = (float)He;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int f = (int)(i / plane);
        const int p = (int)(i - f * plane);
        const int y = p / We, x = p - y * We;
        float dx, dy, dz;
        pixel_dir(x, y, Wf, Hf, dx, dy, dz);
        const float d = dist[i];
        const float px = dx * d, py = dy * d, pz = dz * d;
        int agree = 0;
        for (int s = 0; s < S; ++s) {
            const int si = src_index[f * S + s];
            if (si < 0 || si >= F) continue;
            const float* T = rel_pose + ((long long)f * S + s) * 12;
            const float X = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
            const float Y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
            const float Z = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
            const float nrm = sqrtf((X * X + Y * Y) + Z * Z);
            if (!(nrm > 0.0f && nrm < INFINITY)) continue;
            float u, v;
            dir_pixel(X, Y, Z, nrm, Wf, Hf, u, v);
            int xi = (int)floorf(u + 0.5f) % We;
            xi = xi < 0 ? xi + We : xi;
            const int yi = clampi((int)floorf(v + 0.5f), 0, He - 1);
            const float ds = dist[si * plane + (long long)yi * We + xi];
            agree += fabsf(ds - nrm) <= rel_tol * nrm ? 1 : 0;
        }
        if (agree < min_consistent) conf[i] = 0.0f;
    }
}

__global__ __launch_bounds__(NT) void pano_unproject_kernel(const float* __restrict__ dist, const float* __restrict__ c2w,
                                                            float* __restrict__ xyz, int F, int He, int We) {
    const long long plane = (long long)He * We, total = (long long)F * plane;
    const float Wf = (float)We, Hf = (float)He;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int f = (int)(i / plane);
        const int p = (int)(i - f * plane);
        const int y = p / We, x = p - y * We;
        float dx, dy, dz;
        pixel_dir(x, y, Wf, Hf, dx, dy, dz);
        const float d = dist[i];
        const float px = dx * d, py = dy * d, pz = dz * d;
        const float* T = c2w + (long long)f * 12;
        float* o = xyz + i * 3;
        o[0] = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
        o[1] = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
        o[2] = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    }
}

unsigned stride_grid(long long n) {
    const long long blocks = (n + NT - 1) / NT;
    return (unsigned)(blocks < 65536 ? (blocks > 0 ? blocks : 1) : 65536);
}

}  // namespace

extern "C" ew_status ew_mvs_sphere_sweep(const uint8_t* grey, const float* rel_pose, const int* src_index, const float* inv_dist, float* dist,
                                         float* conf, int* winner, float* winner_cost, int F, int He, int We, int S, int D, int patch_radius,
                                         void* stream) {
    EW_REQUIRE(grey && rel_pose && src_index && inv_dist && dist && conf && winner && winner_cost, "ew_mvs_sphere_sweep: NULL pointer");
    EW_REQUIRE(F >= 1 && F <= 65535 && He >= 1 && We >= 1 && (long long)He * We < (1LL << 31),
               "ew_mvs_sphere_sweep: F = %d must be 1 .. 65535, He = %d and We = %d positive with He We below 2^31", F, He, We);
    EW_REQUIRE(S >= 1 && D >= 1 && (long long)F * S < (1LL << 27) && (long long)F * D < (1LL << 31),
               "ew_mvs_sphere_sweep: S = %d and D = %d must be positive, F S below 2^27 and F D below 2^31", S, D);
    EW_REQUIRE(patch_radius >= 0 && patch_radius <= RMAX, "ew_mvs_sphere_sweep: patch_radius = %d must be 0 .. %d", patch_radius, RMAX);
    EW_REQUIRE(We >= 2 * patch_radius + 1, "ew_mvs_sphere_sweep: We = %d is narrower than the window of 2 x %d + 1 columns", We, patch_radius);
    EW_REQUIRE((((uintptr_t)rel_pose | (uintptr_t)src_index | (uintptr_t)inv_dist | (uintptr_t)dist | (uintptr_t)conf | (uintptr_t)winner |
                 (uintptr_t)winner_cost) & 3) == 0, "ew_mvs_sphere_sweep: the fp32 and int32 arrays must be 4-byte aligned");
    const unsigned gx = (unsigned)((We + TW - 1) / TW), gy = (unsigned)((He + TH - 1) / TH);
    EW_REQUIRE(gy <= 65535, "ew_mvs_sphere_sweep: He = %d gives more than 65535 tile rows", He);
    hipLaunchKernelGGL(sphere_sweep_kernel<false>, dim3(gx, gy, (unsigned)F), dim3(NT), 0, (hipStream_t)stream, grey, rel_pose, src_index,
                       inv_dist, dist, conf, winner, winner_cost, F, He, We, S, D, patch_radius, (uint16_t*)nullptr, 0.0f, 0);
    return ew_check_launch("mvs_sphere sphere_sweep_kernel");
}

extern "C" ew_status ew_mvs_sphere_sweep_volume(const uint8_t* grey, const float* rel_pose, const int* src_index, const float* inv_dist,
                                                uint16_t* cost, int F, int He, int We, int S, int D, int patch_radius, float cost_scale,
                                                int view_begin, int n_views, void* stream) {
    EW_REQUIRE(grey && rel_pose && src_index && inv_dist && cost, "ew_mvs_sphere_sweep_volume: NULL pointer");
    EW_REQUIRE(F >= 1 && F <= 65535 && He >= 1 && We >= 1 && (long long)He * We < (1LL << 31),
               "ew_mvs_sphere_sweep_volume: F = %d must be 1 .. 65535, He = %d and We = %d positive with He We below 2^31", F, He, We);
    EW_REQUIRE(S >= 1 && D >= 1 && (long long)F * S < (1LL << 27) && (long long)F * D < (1LL << 31),
               "ew_mvs_sphere_sweep_volume: S = %d and D = %d must be positive, F S below 2^27 and F D below 2^31", S, D);
    EW_REQUIRE(patch_radius >= 0 && patch_radius <= RMAX, "ew_mvs_sphere_sweep_volume: patch_radius = %d must be 0 .. %d", patch_radius, RMAX);
    EW_REQUIRE(We >= 2 * patch_radius + 1, "ew_mvs_sphere_sweep_volume: We = %d is narrower than the window of 2 x %d + 1 columns", We,
               patch_radius);
    EW_REQUIRE(cost_scale > 0.0f && cost_scale < INFINITY, "ew_mvs_sphere_sweep_volume: cost_scale = %g must be positive and finite",
               (double)cost_scale);
    EW_REQUIRE(view_begin >= 0 && n_views >= 1 && n_views <= F - view_begin,
               "ew_mvs_sphere_sweep_volume: views %d .. %d + %d - 1 must lie in [0, F = %d)", view_begin, view_begin, n_views, F);
    EW_REQUIRE((((uintptr_t)rel_pose | (uintptr_t)src_index | (uintptr_t)inv_dist) & 3) == 0 && ((uintptr_t)cost & 1) == 0,
               "ew_mvs_sphere_sweep_volume: the fp32 and int32 arrays must be 4-byte aligned, the volume 2-byte aligned");
    const unsigned gx = (unsigned)((We + TW - 1) / TW), gy = (unsigned)((He + TH - 1) / TH);
    EW_REQUIRE(gy <= 65535, "ew_mvs_sphere_sweep_volume: He = %d gives more than 65535 tile rows", He);
    hipLaunchKernelGGL(sphere_sweep_kernel<true>, dim3(gx, gy, (unsigned)n_views), dim3(NT), EW_MVS_STAGE_BYTES, (hipStream_t)stream, grey,
                       rel_pose, src_index, inv_dist, (float*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr, F, He, We, S, D,
                       patch_radius, cost, cost_scale, view_begin);
    return ew_check_launch("mvs_sphere sphere_sweep_kernel<volume>");
}

extern "C" ew_status ew_mvs_sphere_consistency(const float* dist, const float* rel_pose, const int* src_index, float* conf, int F, int He,
                                               int We, int S, float rel_tol, int min_consistent, void* stream) {
    EW_REQUIRE(dist && rel_pose && src_index && conf, "ew_mvs_sphere_consistency: NULL pointer");
    EW_REQUIRE(F >= 1 && He >= 1 && We >= 1 && S >= 1 && (long long)He * We < (1LL << 31) && (long long)F * S < (1LL << 27),
               "ew_mvs_sphere_consistency: F = %d, He = %d, We = %d, S = %d must be positive, He We below 2^31 and F S below 2^27", F, He, We, S);
    EW_REQUIRE(rel_tol >= 0.0f, "ew_mvs_sphere_consistency: rel_tol = %g must not be negative", (double)rel_tol);
    EW_REQUIRE((((uintptr_t)dist | (uintptr_t)rel_pose | (uintptr_t)src_index | (uintptr_t)conf) & 3) == 0,
               "ew_mvs_sphere_consistency: the arrays must be 4-byte aligned");
    hipLaunchKernelGGL(sphere_consistency_kernel, dim3(stride_grid((long long)F * He * We)), dim3(NT), 0, (hipStream_t)stream, dist, rel_pose,
                       src_index, conf, F, He, We, S, rel_tol, min_consistent);
    return ew_check_launch("mvs_sphere sphere_consistency_kernel");
}

extern "C" ew_status ew_pano_unproject(const float* dist, const float* c2w, float* xyz, int F, int He, int We, void* stream) {
    EW_REQUIRE(dist && c2w && xyz, "ew_pano_unproject: NULL pointer");
    EW_REQUIRE(F >= 1 && He >= 1 && We >= 1 && (long long)He * We < (1LL << 31) && (long long)F < (1LL << 27),
               "ew_pano_unproject: F = %d, He = %d, We = %d must be positive, He We below 2^31 and F below 2^27", F, He, We);
    EW_REQUIRE((((uintptr_t)dist | (uintptr_t)c2w | (uintptr_t)xyz) & 3) == 0, "ew_pano_unproject: the arrays must be 4-byte aligned");
    hipLaunchKernelGGL(pano_unproject_kernel, dim3(stride_grid((long long)F * He * We)), dim3(NT), 0, (hipStream_t)stream, dist, c2w, xyz, F, He,
                       We);
    return ew_check_launch("mvs_sphere pano_unproject_kernel");
}
