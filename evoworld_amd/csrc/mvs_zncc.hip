// mvs_zncc.hip -- the two sweeps of mvs.hip and mvs_sphere.hip with an opt-in matching cost that does not move when a view's exposure,
// contrast or tone drifts: zero-mean normalised cross-correlation over the patch window (ABI 20, symbols added without a bump; DESIGN.md
// 4.11).  The warps, the bilinear blends, the winner, parabola, runner-up and confidence rules are those of the SAD sweeps and are restated
// here in the header's order; mvs.hip, mvs_sphere.hip and mvs_sgm.hip are untouched.  fp32 throughout in a fixed operation order, sqrtf and
// IEEE division only (compiled with -ffp-contract=off like its neighbours), restated by tests/mvs_zncc_ref.py.
//
//   ew_mvs_plane_sweep_zncc    one workgroup of 256 threads owns a 32 x 8 tile of one reference view.  The tile's a = grey - 128 plus a
//                              halo of r pixels sit in LDS as floats; the window sums of a and a a of every pixel are taken once and stay
//                              in registers.  Per plane and per present source: every thread warps its share of the halo'd tile into the
//                              source and writes b = sample - 128 to LDS (a NaN where the sample leaves the source: it poisons every
//                              window that holds it); a row pass adds the 2r + 1 horizontal taps of b, b b and a b, a column pass the
//                              2r + 1 vertical ones; each thread turns its pixel's five sums into 100 (1 - zncc), or oob_cost where the
//                              sums are NaN, and adds it to a register.  After the last source: the mean over the sources, then the
//                              winner bookkeeping of the SAD sweep.  Two workgroup barriers per (plane, source); no atomics, no
//                              communication between workgroups, every loop bound an argument.  LDS: 9.4 KiB.
//   ew_mvs_sphere_sweep_zncc   the same on panoramas: a thread's (at most three) cells keep a and their unit direction in registers across
//                              the hypotheses, halo columns wrap modulo We, halo rows outside are empty, every sample lands in the source.
//   ew_mvs_*_sweep_zncc_volume the same tile kernels instantiated with VOLUME = true: the same C(k), quantised and staged in LDS
//                              (mvs_volume.h) as the uint16 volume the semi-global aggregation reads (mvs_sgm.hip).
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
constexpr float MID = 128.0f;                      // a = grey - MID, b = sample - MID

// bilinear(src at H (x, y, 1)) - 128, or NaN where the sample is behind the source or leaves [0, W-1] x [0, H-1]: ew_mvs_plane_sweep's warp
__device__ __forceinline__ float plane_sample(const uint8_t* __restrict__ src, const float* __restrict__ h, float x, float y, int H, int W) {
    const float q0 = (h[0] * x + h[1] * y) + h[2];
    const float q1 = (h[3] * x + h[4] * y) + h[5];
    const float q2 = (h[6] * x + h[7] * y) + h[8];
    if (!(q2 > 0.0f)) return NAN;
    const float sx = q0 / q2, sy = q1 / q2;
    if (!(sx >= 0.0f && sx <= (float)(W - 1) && sy >= 0.0f && sy <= (float)(H - 1))) return NAN;
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
    return (top * (1.0f - ay) + bot * ay) - MID;
}

// pixel (x, y) -> unit direction in the panorama camera (x right, y down, z forward): the header's dir(x, y)
__device__ __forceinline__ void pixel_dir(int x, int y, float Wf, float Hf, float& dx, float& dy, float& dz) {
    const float lon = (((float)x - Wf * 0.5f) - 0.5f) * ((2.0f * PI_F) / Wf);
    const float lat = (((float)y - Hf * 0.5f) - 0.5f) * (PI_F / Hf);
    const float cl = cosf(lat);
    dx = cl * sinf(lon);
    dy = sinf(lat);
    dz = cl * cosf(lon);
}

__device__ __forceinline__ int clampi(int a, int lo, int hi) { return a < lo ? lo : (a > hi ? hi : a); }

// bilinear(src) - 128 at the pixel the point P = d rad lands on in the source (T = R | t, reference camera -> source camera); a_ref, the
// neutral choice, when the point sits on the source's centre or is not finite: ew_mvs_sphere_sweep's warp
__device__ __forceinline__ float sphere_sample(const uint8_t* __restrict__ src, const float* __restrict__ T, float dx, float dy, float dz,
                                               float rad, float a_ref, int He, int We, float Wf, float Hf) {
    const float px = dx * rad, py = dy * rad, pz = dz * rad;
    const float X = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const float Y = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    const float Z = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    const float nrm = sqrtf((X * X + Y * Y) + Z * Z);
    if (!(nrm > 0.0f && nrm < INFINITY)) return a_ref;
    const float lon = atan2f(X, Z);
    const float lat = asinf(fminf(fmaxf(Y / nrm, -1.0f), 1.0f));
    float u = ((lon * Wf) / (2.0f * PI_F) + Wf * 0.5f) + 0.5f;
    float v = ((lat * Hf) / PI_F + Hf * 0.5f) + 0.5f;
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
    return (top * (1.0f - ay) + bot * ay) - MID;
}

// what the two tile kernels share once s_ref and s_b hold a and b of the halo'd tile
struct Tile {
    float* s_ref;                                  // a of the halo'd tile, 0 on the taps that do not count
    float* s_b;                                    // per (hypothesis, source): b, 0 on the taps that do not count
    float* s_r0;                                   // row sums: of b (of a before the loop)
    float* s_r1;                                   // of b b (of a a before the loop)
    float* s_r2;                                   // of a b
    int t, tx, ty, r, hw, hh;
    float nf, sa, saa;                             // taps of this pixel's window that count; its sums of a and of a a

    // the sums of a and a a, once: rows of taps left to right, then the row sums top to bottom.  s_ref is complete behind a barrier.
    __device__ __forceinline__ void reference_sums() {
        for (int i = t; i < hh * TW; i += NT) {
            const int ly = i / TW, lx = i - ly * TW;
            const float* a = s_ref + ly * hw + lx;
            float s0 = 0.0f, s1 = 0.0f;
            for (int d = 0; d <= 2 * r; ++d) { s0 += a[d]; s1 += a[d] * a[d]; }
            s_r0[i] = s0; s_r1[i] = s1;
        }
        __syncthreads();
        sa = 0.0f; saa = 0.0f;
        for (int d = 0; d <= 2 * r; ++d) { sa += s_r0[(ty + d) * TW + tx]; saa += s_r1[(ty + d) * TW + tx]; }
        // the row sums are written again only behind the first barrier of the hypothesis loop
    }

    // s_b of one (hypothesis, source) is written: -> this pixel's cost_s = 100 (1 - zncc), or oob where a NaN sits in its window
    __device__ __forceinline__ float slot_cost(float var_floor, float oob) {
        __syncthreads();
        for (int i = t; i < hh * TW; i += NT) {
            const int ly = i / TW, lx = i - ly * TW;
            const float* a = s_ref + ly * hw + lx;
            const float* b = s_b + ly * hw + lx;
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int d = 0; d <= 2 * r; ++d) { s0 += b[d]; s1 += b[d] * b[d]; s2 += a[d] * b[d]; }
            s_r0[i] = s0; s_r1[i] = s1; s_r2[i] = s2;
        }
        __syncthreads();                           // also orders these reads of s_b before the next source's writes
        float sb = 0.0f, sbb = 0.0f, sab = 0.0f;
        for (int d = 0; d <= 2 * r; ++d) {
            const int j = (ty + d) * TW + tx;
            sb += s_r0[j]; sbb += s_r1[j]; sab += s_r2[j];
        }
        // the row sums are written again only behind the next source's first barrier
        if (!(sb == sb)) return oob;
        const float cov = nf * sab - sa * sb;
        const float va = fmaxf(nf * saa - sa * sa, 0.0f);
        const float vb = fmaxf(nf * sbb - sb * sb, 0.0f);
        const float fl = var_floor * (nf * nf);
        const float den = sqrtf(va * vb + fl * fl);
        const float z = den > 0.0f ? cov / den : 0.0f;
        return 100.0f * (1.0f - z);
    }
};

// the winner bookkeeping of ew_mvs_plane_sweep, word for word: the four lowest (cost, hypothesis) pairs in ascending order, ties to the
// lower hypothesis; C(k - 1); C(k0 - 1) and C(k0 + 1) of the running winner
struct Winner {
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
    int k0 = -1, k1 = -1, k2 = -1, k3 = -1;
    float prev = 0.0f, left = 0.0f, right = 0.0f;
    bool has_left = false, has_right = false;

    __device__ __forceinline__ void take(float c, int k) {
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

    __device__ __forceinline__ void store(const float* __restrict__ invd, int D, int n_src, long long o, float* __restrict__ out,
                                          float* __restrict__ conf, int* __restrict__ winner, float* __restrict__ win_cost) {
        if (k0 < 0) { k0 = 0; b0 = prev; has_right = false; }      // every cost a NaN (non-finite tables): hypothesis 0, no refinement
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
        out[o] = 1.0f / inv;
        conf[o] = (has_c2 && n_src > 0) ? (c2 - b0) / fmaxf(c2, 1e-6f) : 0.0f;
        winner[o] = k0;
        win_cost[o] = b0;
    }
};

// VOLUME = false: the fused sweep (ew_mvs_plane_sweep_zncc), f = blockIdx.z.  VOLUME = true: the same C(k), quantised and stored
// (ew_mvs_plane_sweep_zncc_volume): f = view_begin + blockIdx.z, `vol` [gridDim.z,H,W,D]; the four output planes are not touched.
template <bool VOLUME>
__global__ __launch_bounds__(NT) void plane_zncc_kernel(const uint8_t* __restrict__ grey, const float* __restrict__ homog,
                                                        const int* __restrict__ src_index, const float* __restrict__ inv_depth,
                                                        float* __restrict__ depth, float* __restrict__ conf, int* __restrict__ winner,
                                                        float* __restrict__ win_cost, int F, int H, int W, int S, int D, int r, float oob,
                                                        float var_floor, uint16_t* __restrict__ vol, float cost_scale, int view_begin) {
    __shared__ float s_ref[HH_MAX * HW_MAX];
    __shared__ float s_b[HH_MAX * HW_MAX];
    __shared__ float s_rs[3][HH_MAX * TW];
    const int t = threadIdx.x;
    const int f = (VOLUME ? view_begin : 0) + blockIdx.z;
    const int x_org = blockIdx.x * TW - r, y_org = blockIdx.y * TH - r;       // image position of the halo'd tile's corner
    const int hw = TW + 2 * r, hh = TH + 2 * r;
    const long long plane = (long long)H * W;
    const uint8_t* ref_img = grey + f * plane;

    for (int i = t; i < hh * hw; i += NT) {
        const int ly = i / hw, lx = i - ly * hw;
        const int x = x_org + lx, y = y_org + ly;
        s_ref[i] = (x >= 0 && x < W && y >= 0 && y < H) ? (float)ref_img[(long long)y * W + x] - MID : 0.0f;
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
    Tile tile{s_ref, s_b, s_rs[0], s_rs[1], s_rs[2], t, tx, ty, r, hw, hh, (float)(cx * cy), 0.0f, 0.0f};
    tile.reference_sums();
    const float slots = (float)(n_src > 0 ? n_src : 1);
    Winner w;

    for (int k = 0; k < D; ++k) {
        float c = 0.0f;
        for (int s = 0; s < S; ++s) {
            const int si = src_index[f * S + s];
            if (si < 0 || si >= F) continue;       // uniform over the workgroup: the barriers below are reached by all or by none
            const float* h = homog + (((long long)f * S + s) * D + k) * 9;
            const uint8_t* src = grey + si * plane;
            for (int i = t; i < hh * hw; i += NT) {
                const int ly = i / hw, lx = i - ly * hw;
                const int x = x_org + lx, y = y_org + ly;
                s_b[i] = (x >= 0 && x < W && y >= 0 && y < H) ? plane_sample(src, h, (float)x, (float)y, H, W) : 0.0f;
            }
            c += tile.slot_cost(var_floor, oob);
        }
        c = c / slots;
        if constexpr (VOLUME) {
            ew_mvs_stage_cost(c, cost_scale, k, D, vol + (long long)blockIdx.z * plane * D, H, W);
            continue;
        }
        w.take(c, k);
    }
    if (VOLUME || !live) return;
    w.store(inv_depth + (long long)f * D, D, n_src, f * plane + (long long)py * W + px, depth, conf, winner, win_cost);
}

// VOLUME as above (ew_mvs_sphere_sweep_zncc, ew_mvs_sphere_sweep_zncc_volume)
template <bool VOLUME>
__global__ __launch_bounds__(NT) void sphere_zncc_kernel(const uint8_t* __restrict__ grey, const float* __restrict__ rel_pose,
                                                         const int* __restrict__ src_index, const float* __restrict__ inv_dist,
                                                         float* __restrict__ dist, float* __restrict__ conf, int* __restrict__ winner,
                                                         float* __restrict__ win_cost, int F, int He, int We, int S, int D, int r,
                                                         float var_floor, uint16_t* __restrict__ vol, float cost_scale, int view_begin) {
    __shared__ float s_ref[HH_MAX * HW_MAX];
    __shared__ float s_b[HH_MAX * HW_MAX];
    __shared__ float s_rs[3][HH_MAX * TW];
    const int t = threadIdx.x;
    const int f = (VOLUME ? view_begin : 0) + blockIdx.z;
    const int x_org = blockIdx.x * TW - r, y_org = blockIdx.y * TH - r;       // panorama position of the halo'd tile's corner
    const int hw = TW + 2 * r, hh = TH + 2 * r;
    const long long plane = (long long)He * We;
    const uint8_t* ref_img = grey + f * plane;
    const float Wf = (float)We, Hf = (float)He;

    // this thread's cells of the halo'd tile: a and direction, once for all hypotheses
    float c_a[CELLS], c_dx[CELLS], c_dy[CELLS], c_dz[CELLS];
    bool c_in[CELLS];
#pragma unroll
    for (int j = 0; j < CELLS; ++j) {
        const int i = t + j * NT;
        const int ly = i / hw, lx = i - ly * hw;
        const int y = y_org + ly;
        int x = (x_org + lx) % We;                 // columns wrap across the seam
        x = x < 0 ? x + We : x;
        c_in[j] = i < hh * hw && y >= 0 && y < He;
        c_a[j] = 0.0f; c_dx[j] = 0.0f; c_dy[j] = 0.0f; c_dz[j] = 0.0f;
        if (c_in[j]) {
            c_a[j] = (float)ref_img[(long long)y * We + x] - MID;
            pixel_dir(x, y, Wf, Hf, c_dx[j], c_dy[j], c_dz[j]);
        }
        if (i < hh * hw) s_ref[i] = c_a[j];
    }
    int n_src = 0;                                 // present sources: an index outside [0, F) is absent
    for (int s = 0; s < S; ++s) {
        const int si = src_index[f * S + s];
        n_src += (si >= 0 && si < F) ? 1 : 0;
    }
    __syncthreads();

    const int tx = t & (TW - 1), ty = t / TW;
    const int px = blockIdx.x * TW + tx, py = blockIdx.y * TH + ty;
    const bool live = px < We && py < He;
    // rows of the window inside the panorama; all 2r + 1 columns always count
    const int cy = (py + r < He ? py + r : He - 1) - (py - r > 0 ? py - r : 0) + 1;
    Tile tile{s_ref, s_b, s_rs[0], s_rs[1], s_rs[2], t, tx, ty, r, hw, hh, (float)((2 * r + 1) * cy), 0.0f, 0.0f};
    tile.reference_sums();
    const float slots = (float)(n_src > 0 ? n_src : 1);
    const float* invd = inv_dist + (long long)f * D;
    Winner w;

    for (int k = 0; k < D; ++k) {
        const float rad = 1.0f / invd[k];
        float c = 0.0f;
        for (int s = 0; s < S; ++s) {
            const int si = src_index[f * S + s];
            if (si < 0 || si >= F) continue;       // uniform over the workgroup: the barriers below are reached by all or by none
            const float* T = rel_pose + ((long long)f * S + s) * 12;
            const uint8_t* src = grey + si * plane;
#pragma unroll
            for (int j = 0; j < CELLS; ++j) {
                const int i = t + j * NT;
                if (i < hh * hw)
                    s_b[i] = c_in[j] ? sphere_sample(src, T, c_dx[j], c_dy[j], c_dz[j], rad, c_a[j], He, We, Wf, Hf) : 0.0f;
            }
            c += tile.slot_cost(var_floor, 0.0f);  // no sample is a NaN here unless the tables are: such a cost is 0 for the slot
        }
        c = c / slots;
        if constexpr (VOLUME) {
            ew_mvs_stage_cost(c, cost_scale, k, D, vol + (long long)blockIdx.z * plane * D, He, We);
            continue;
        }
        w.take(c, k);
    }
    if (VOLUME || !live) return;
    w.store(invd, D, n_src, f * plane + (long long)py * We + px, dist, conf, winner, win_cost);
}

// the checks the four entries share; `wide`: the plane sweep's limit on F S D (its homographies), otherwise the sphere sweep's two
#define EW_ZNCC_REQUIRE_SHAPE(name, wide)                                                                                                 \
    EW_REQUIRE(F >= 1 && F <= 65535 && H >= 1 && W >= 1 && (long long)H * W < (1LL << 31),                                                 \
               name ": F = %d must be 1 .. 65535, H = %d and W = %d positive with H W below 2^31", F, H, W);                                \
    EW_REQUIRE(S >= 1 && D >= 1 && ((wide) ? (long long)F * S * D < (1LL << 31) : ((long long)F * S < (1LL << 27) && (long long)F * D < (1LL << 31))), \
               name ": S = %d and D = %d must be positive, F S D below 2^31 (plane) or F S below 2^27 and F D below 2^31 (sphere)", S, D);  \
    EW_REQUIRE(patch_radius >= 1 && patch_radius <= RMAX, name ": patch_radius = %d must be 1 .. %d (a single tap has no variance)",        \
               patch_radius, RMAX);                                                                                                        \
    EW_REQUIRE(var_floor >= 0.0f && var_floor < INFINITY, name ": var_floor = %g must be finite and not negative", (double)var_floor);      \
    EW_REQUIRE((H + TH - 1) / TH <= 65535, name ": H = %d gives more than 65535 tile rows", H)

#define EW_ZNCC_REQUIRE_VOLUME(name)                                                                                                      \
    EW_REQUIRE(cost_scale > 0.0f && cost_scale < INFINITY, name ": cost_scale = %g must be positive and finite", (double)cost_scale);       \
    EW_REQUIRE(view_begin >= 0 && n_views >= 1 && n_views <= F - view_begin, name ": views %d .. %d + %d - 1 must lie in [0, F = %d)",      \
               view_begin, view_begin, n_views, F)

}  // namespace

extern "C" ew_status ew_mvs_plane_sweep_zncc(const uint8_t* grey, const float* homographies, const int* src_index, const float* inv_depth,
                                             float* depth, float* conf, int* winner, float* winner_cost, int F, int H, int W, int S, int D,
                                             int patch_radius, float oob_cost, float var_floor, void* stream) {
    EW_REQUIRE(grey && homographies && src_index && inv_depth && depth && conf && winner && winner_cost, "ew_mvs_plane_sweep_zncc: NULL pointer");
    EW_ZNCC_REQUIRE_SHAPE("ew_mvs_plane_sweep_zncc", true);
    EW_REQUIRE((((uintptr_t)homographies | (uintptr_t)src_index | (uintptr_t)inv_depth | (uintptr_t)depth | (uintptr_t)conf | (uintptr_t)winner |
                 (uintptr_t)winner_cost) & 3) == 0, "ew_mvs_plane_sweep_zncc: the fp32 and int32 arrays must be 4-byte aligned");
    const unsigned gx = (unsigned)((W + TW - 1) / TW), gy = (unsigned)((H + TH - 1) / TH);
    hipLaunchKernelGGL(plane_zncc_kernel<false>, dim3(gx, gy, (unsigned)F), dim3(NT), 0, (hipStream_t)stream, grey, homographies, src_index,
                       inv_depth, depth, conf, winner, winner_cost, F, H, W, S, D, patch_radius, oob_cost, var_floor, (uint16_t*)nullptr, 0.0f, 0);
    return ew_check_launch("mvs_zncc plane_zncc_kernel");
}

extern "C" ew_status ew_mvs_plane_sweep_zncc_volume(const uint8_t* grey, const float* homographies, const int* src_index,
                                                    const float* inv_depth, uint16_t* cost, int F, int H, int W, int S, int D, int patch_radius,
                                                    float oob_cost, float var_floor, float cost_scale, int view_begin, int n_views,
                                                    void* stream) {
    EW_REQUIRE(grey && homographies && src_index && inv_depth && cost, "ew_mvs_plane_sweep_zncc_volume: NULL pointer");
    EW_ZNCC_REQUIRE_SHAPE("ew_mvs_plane_sweep_zncc_volume", true);
    EW_ZNCC_REQUIRE_VOLUME("ew_mvs_plane_sweep_zncc_volume");
    EW_REQUIRE((((uintptr_t)homographies | (uintptr_t)src_index | (uintptr_t)inv_depth) & 3) == 0 && ((uintptr_t)cost & 1) == 0,
               "ew_mvs_plane_sweep_zncc_volume: the fp32 and int32 arrays must be 4-byte aligned, the volume 2-byte aligned");
    const unsigned gx = (unsigned)((W + TW - 1) / TW), gy = (unsigned)((H + TH - 1) / TH);
    hipLaunchKernelGGL(plane_zncc_kernel<true>, dim3(gx, gy, (unsigned)n_views), dim3(NT), EW_MVS_STAGE_BYTES, (hipStream_t)stream, grey,
                       homographies, src_index, inv_depth, (float*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr, F, H, W, S, D,
                       patch_radius, oob_cost, var_floor, cost, cost_scale, view_begin);
    return ew_check_launch("mvs_zncc plane_zncc_kernel<volume>");
}

extern "C" ew_status ew_mvs_sphere_sweep_zncc(const uint8_t* grey, const float* rel_pose, const int* src_index, const float* inv_dist,
                                              float* dist, float* conf, int* winner, float* winner_cost, int F, int He, int We, int S, int D,
                                              int patch_radius, float var_floor, void* stream) {
    const int H = He, W = We;
    EW_REQUIRE(grey && rel_pose && src_index && inv_dist && dist && conf && winner && winner_cost, "ew_mvs_sphere_sweep_zncc: NULL pointer");
    EW_ZNCC_REQUIRE_SHAPE("ew_mvs_sphere_sweep_zncc", false);
    EW_REQUIRE(We >= 2 * patch_radius + 1, "ew_mvs_sphere_sweep_zncc: We = %d is narrower than the window of 2 x %d + 1 columns", We, patch_radius);
    EW_REQUIRE((((uintptr_t)rel_pose | (uintptr_t)src_index | (uintptr_t)inv_dist | (uintptr_t)dist | (uintptr_t)conf | (uintptr_t)winner |
                 (uintptr_t)winner_cost) & 3) == 0, "ew_mvs_sphere_sweep_zncc: the fp32 and int32 arrays must be 4-byte aligned");
    const unsigned gx = (unsigned)((We + TW - 1) / TW), gy = (unsigned)((He + TH - 1) / TH);
    hipLaunchKernelGGL(sphere_zncc_kernel<false>, dim3(gx, gy, (unsigned)F), dim3(NT), 0, (hipStream_t)stream, grey, rel_pose, src_index,
                       inv_dist, dist, conf, winner, winner_cost, F, He, We, S, D, patch_radius, var_floor, (uint16_t*)nullptr, 0.0f, 0);
    return ew_check_launch("mvs_zncc sphere_zncc_kernel");
}

extern "C" ew_status ew_mvs_sphere_sweep_zncc_volume(const uint8_t* grey, const float* rel_pose, const int* src_index, const float* inv_dist,
                                                     uint16_t* cost, int F, int He, int We, int S, int D, int patch_radius, float var_floor,
                                                     float cost_scale, int view_begin, int n_views, void* stream) {
    const int H = He, W = We;
    EW_REQUIRE(grey && rel_pose && src_index && inv_dist && cost, "ew_mvs_sphere_sweep_zncc_volume: NULL pointer");
    EW_ZNCC_REQUIRE_SHAPE("ew_mvs_sphere_sweep_zncc_volume", false);
    EW_REQUIRE(We >= 2 * patch_radius + 1, "ew_mvs_sphere_sweep_zncc_volume: We = %d is narrower than the window of 2 x %d + 1 columns", We,
               patch_radius);
    EW_ZNCC_REQUIRE_VOLUME("ew_mvs_sphere_sweep_zncc_volume");
    EW_REQUIRE((((uintptr_t)rel_pose | (uintptr_t)src_index | (uintptr_t)inv_dist) & 3) == 0 && ((uintptr_t)cost & 1) == 0,
               "ew_mvs_sphere_sweep_zncc_volume: the fp32 and int32 arrays must be 4-byte aligned, the volume 2-byte aligned");
    const unsigned gx = (unsigned)((We + TW - 1) / TW), gy = (unsigned)((He + TH - 1) / TH);
    hipLaunchKernelGGL(sphere_zncc_kernel<true>, dim3(gx, gy, (unsigned)n_views), dim3(NT), EW_MVS_STAGE_BYTES, (hipStream_t)stream, grey,
                       rel_pose, src_index, inv_dist, (float*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr, F, He, We, S, D,
                       patch_radius, var_floor, cost, cost_scale, view_begin);
    return ew_check_launch("mvs_zncc sphere_zncc_kernel<volume>");
}
