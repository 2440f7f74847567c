// mvs_sgm.hip -- semi-global aggregation of a sweep's cost volume and the winner on the aggregated costs (ABI 20, symbols added without a
// bump): the opt-in smoothness prior between ew_mvs_*_sweep_volume and the depth.  Integer arithmetic in the
// aggregation, fp32 in a fixed operation order in the select (compiled with -ffp-contract=off like mvs.hip), restated by
// tests/mvs_sgm_ref.py.
//
//   ew_mvs_sgm_aggregate  one launch per path direction.  One wave owns one path line of one view and walks it from the pixel whose
//                         predecessor lies outside the image to the other border; lane l holds the hypotheses l, l + 64, ... (at most 4:
//                         D <= 256), hypotheses >= D carry a neutral BIG.  L_r of the previous pixel stays in registers; the k - 1 / k + 1
//                         neighbours are lane shuffles (the wave's edge lanes take the other register's edge), the minimum a shuffle
//                         butterfly.  The costs of the next STEPS pixels are loaded while the current ones are processed: their addresses
//                         do not depend on the recurrence.  The first direction stores L, every later one adds L to agg (uint16
//                         read-modify-write): a cell is touched by exactly one wave per launch, so there are no atomics and the sum is
//                         exact in any order.
//   ew_mvs_sgm_select     one thread per pixel: the sweeps' four-lowest scan, parabola and confidence rules on (float)agg.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int WAVE = 64;
constexpr int WAVES = NT / WAVE;
constexpr int STEPS = 4;                            // pixels of a line whose costs are in flight ahead of the recurrence
constexpr int BIG = 1 << 20;                        // above every L (<= 8190); BIG + P2 stays far from overflow

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int d = WAVE / 2; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, WAVE));
    return v;
}

// KPL = ceil(D / 64) hypotheses per lane.  dx, dy in {-1, 0, 1}, not both 0.  n_lines = lines of one view for this direction.
template <int KPL>
__global__ __launch_bounds__(NT) void sgm_path_kernel(const uint16_t* __restrict__ cost, uint16_t* __restrict__ agg, int N, int H, int W, int D,
                                                      int P1, int P2, int dx, int dy, int n_lines, int first) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long wid = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (wid >= (long long)N * n_lines) return;      // whole waves leave: no workgroup barrier below
    const int n = (int)(wid / n_lines), line = (int)(wid - (long long)n * n_lines);

    // the line's start pixel (its predecessor is outside the image) and its length
    int x, y;
    if (dy == 0) { x = dx > 0 ? 0 : W - 1; y = line; }
    else if (dx == 0) { x = line; y = dy > 0 ? 0 : H - 1; }
    else if (line < H) { x = dx > 0 ? 0 : W - 1; y = line; }                         // the entry column, every row
    else { const int t = line - H + 1; x = dx > 0 ? t : W - 1 - t; y = dy > 0 ? 0 : H - 1; }   // the entry row without the corner
    const int len_x = dx == 0 ? (1 << 30) : (dx > 0 ? W - x : x + 1);
    const int len_y = dy == 0 ? (1 << 30) : (dy > 0 ? H - y : y + 1);
    const int len = len_x < len_y ? len_x : len_y;

    const long long step = ((long long)dy * W + dx) * D;
    long long cell = (((long long)n * H + y) * W + x) * D;                           // first hypothesis of the current pixel
    bool live[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) live[j] = lane + j * WAVE < D;

    int cur[STEPS][KPL], nxt[STEPS][KPL];
#pragma unroll
    for (int u = 0; u < STEPS; ++u)
#pragma unroll
        for (int j = 0; j < KPL; ++j) cur[u][j] = (u < len && live[j]) ? (int)cost[cell + u * step + lane + j * WAVE] : 0;

    int prev[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) prev[j] = BIG;
    int m = 0;
    for (int i = 0; i < len; i += STEPS) {
#pragma unroll
        for (int u = 0; u < STEPS; ++u)
#pragma unroll
            for (int j = 0; j < KPL; ++j)
                nxt[u][j] = (i + STEPS + u < len && live[j]) ? (int)cost[cell + (STEPS + u) * step + lane + j * WAVE] : 0;
#pragma unroll
        for (int u = 0; u < STEPS; ++u) {
            if (i + u >= len) break;                // uniform over the wave
            int L[KPL];
            if (i + u == 0) {
#pragma unroll
                for (int j = 0; j < KPL; ++j) L[j] = live[j] ? cur[u][j] : BIG;
            } else {
#pragma unroll
                for (int j = 0; j < KPL; ++j) {
                    int lo = __shfl_up(prev[j], 1, WAVE), hi = __shfl_down(prev[j], 1, WAVE);
                    const int lo_edge = j > 0 ? __shfl(prev[j > 0 ? j - 1 : 0], WAVE - 1, WAVE) : BIG;       // hypothesis 64 j - 1
                    const int hi_edge = j + 1 < KPL ? __shfl(prev[j + 1 < KPL ? j + 1 : j], 0, WAVE) : BIG;  // hypothesis 64 (j + 1)
                    lo = lane == 0 ? lo_edge : lo;
                    hi = lane == WAVE - 1 ? hi_edge : hi;
                    const int best = min(min(prev[j], min(lo, hi) + P1), m + P2);
                    L[j] = live[j] ? cur[u][j] + best - m : BIG;
                }
            }
            int mm = L[0];
#pragma unroll
            for (int j = 1; j < KPL; ++j) mm = min(mm, L[j]);
            m = wave_min(mm);
            const long long o = cell + u * step;
#pragma unroll
            for (int j = 0; j < KPL; ++j) {
                prev[j] = L[j];
                if (live[j]) {
                    const long long a = o + lane + j * WAVE;
                    agg[a] = (uint16_t)(first ? L[j] : (int)agg[a] + L[j]);
                }
            }
        }
        cell += STEPS * step;
#pragma unroll
        for (int u = 0; u < STEPS; ++u)
#pragma unroll
            for (int j = 0; j < KPL; ++j) cur[u][j] = nxt[u][j];
    }
}

// The rules of ew_mvs_plane_sweep on (float)agg: the scan below is plane_sweep_kernel's, fed from memory instead of from the tile.
__global__ __launch_bounds__(NT) void sgm_select_kernel(const uint16_t* __restrict__ agg, const float* __restrict__ inv,
                                                        const int* __restrict__ src_index, float* __restrict__ depth, float* __restrict__ conf,
                                                        int* __restrict__ winner, float* __restrict__ win_cost, int F, int H, int W, int S, int D,
                                                        int view_begin, int n_views) {
    const long long plane = (long long)H * W, total = (long long)n_views * plane;
    const bool vec = (D & 7) == 0 && ((uintptr_t)agg & 15) == 0;                   // a pixel's run is whole 16-byte pieces
    for (long long o = (long long)blockIdx.x * NT + threadIdx.x; o < total; o += (long long)gridDim.x * NT) {
        const int f = view_begin + (int)(o / plane);
        int n_src = 0;
        for (int s = 0; s < S; ++s) {
            const int si = src_index[f * S + s];
            n_src += (si >= 0 && si < F) ? 1 : 0;
        }
        const uint16_t* a = agg + o * D;
        float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
        int k0 = -1, k1 = -1, k2 = -1, k3 = -1;
        float prev = 0.0f, left = 0.0f, right = 0.0f;
        bool has_left = false, has_right = false;
        auto take = [&](int k, float c) {
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
        };
        if (vec) {
            for (int k = 0; k < D; k += 8) {
                const uint4 v = *reinterpret_cast<const uint4*>(a + k);
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    take(k + 2 * j, (float)(w[j] & 0xffffu));
                    take(k + 2 * j + 1, (float)(w[j] >> 16));
                }
            }
        } else {
            for (int k = 0; k < D; ++k) take(k, (float)a[k]);
        }
        const float* invd = inv + (long long)f * D;
        float iv = invd[k0];
        if (k0 > 0 && k0 < D - 1 && has_right) {
            const float curv = (left + right) - 2.0f * b0;
            if (curv > 0.0f) {
                float off = 0.5f * (left - right) / curv;
                off = fminf(fmaxf(off, -0.5f), 0.5f);
                iv = off >= 0.0f ? iv + off * (invd[k0 + 1] - iv) : iv + (-off) * (invd[k0 - 1] - iv);
            }
        }
        float c2 = 0.0f;
        bool has_c2 = false;
        if (k1 >= 0 && abs(k1 - k0) > 1) { c2 = b1; has_c2 = true; }
        else if (k2 >= 0 && abs(k2 - k0) > 1) { c2 = b2; has_c2 = true; }
        else if (k3 >= 0 && abs(k3 - k0) > 1) { c2 = b3; has_c2 = true; }
        depth[o] = 1.0f / iv;
        conf[o] = (has_c2 && n_src > 0) ? (c2 - b0) / fmaxf(c2, 1e-6f) : 0.0f;
        winner[o] = k0;
        win_cost[o] = b0;
    }
}

unsigned stride_grid(long long n) {
    const long long blocks = (n + NT - 1) / NT;
    return (unsigned)(blocks < 65536 ? (blocks > 0 ? blocks : 1) : 65536);
}

template <int KPL>
void launch_path(const uint16_t* cost, uint16_t* agg, int N, int H, int W, int D, int P1, int P2, int dx, int dy, int first, hipStream_t st) {
    const int n_lines = dy == 0 ? H : (dx == 0 ? W : H + W - 1);
    const long long waves = (long long)N * n_lines;
    hipLaunchKernelGGL(sgm_path_kernel<KPL>, dim3((unsigned)((waves + WAVES - 1) / WAVES)), dim3(NT), 0, st, cost, agg, N, H, W, D, P1, P2, dx,
                       dy, n_lines, first);
}

}  // namespace

extern "C" ew_status ew_mvs_sgm_aggregate(const uint16_t* cost, uint16_t* agg, int N, int H, int W, int D, int P1, int P2, int paths,
                                          void* stream) {
    EW_REQUIRE(cost && agg && cost != agg, "ew_mvs_sgm_aggregate: NULL pointer, or agg is the cost volume itself");
    EW_REQUIRE(N >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1LL << 31) && (long long)N * ((long long)H + W) < (1LL << 31),
               "ew_mvs_sgm_aggregate: N = %d, H = %d, W = %d must be positive, H W and N (H + W) below 2^31", N, H, W);
    EW_REQUIRE(D >= 1 && D <= EW_MVS_SGM_MAX_D, "ew_mvs_sgm_aggregate: D = %d must be 1 .. %d", D, EW_MVS_SGM_MAX_D);
    EW_REQUIRE(0 <= P1 && P1 <= P2 && P2 <= EW_MVS_COST_MAX, "ew_mvs_sgm_aggregate: 0 <= P1 = %d <= P2 = %d <= %d does not hold", P1, P2,
               EW_MVS_COST_MAX);
    EW_REQUIRE(paths == 4 || paths == 8, "ew_mvs_sgm_aggregate: paths = %d must be 4 or 8", paths);
    EW_REQUIRE((((uintptr_t)cost | (uintptr_t)agg) & 1) == 0, "ew_mvs_sgm_aggregate: the volumes must be 2-byte aligned");
    static const int DIRS[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {-1, 1}, {1, -1}};
    const int kpl = (D + WAVE - 1) / WAVE;
    for (int r = 0; r < paths; ++r) {
        const int dx = DIRS[r][0], dy = DIRS[r][1], first = r == 0;
        switch (kpl) {
            case 1: launch_path<1>(cost, agg, N, H, W, D, P1, P2, dx, dy, first, (hipStream_t)stream); break;
            case 2: launch_path<2>(cost, agg, N, H, W, D, P1, P2, dx, dy, first, (hipStream_t)stream); break;
            case 3: launch_path<3>(cost, agg, N, H, W, D, P1, P2, dx, dy, first, (hipStream_t)stream); break;
            default: launch_path<4>(cost, agg, N, H, W, D, P1, P2, dx, dy, first, (hipStream_t)stream); break;
        }
        const ew_status st = ew_check_launch("mvs_sgm sgm_path_kernel");
        if (st != EW_OK) return st;
    }
    return EW_OK;
}

extern "C" ew_status ew_mvs_sgm_select(const uint16_t* agg, const float* inv, const int* src_index, float* depth, float* conf, int* winner,
                                       float* winner_cost, int F, int H, int W, int S, int D, int view_begin, int n_views, void* stream) {
    EW_REQUIRE(agg && inv && src_index && depth && conf && winner && winner_cost, "ew_mvs_sgm_select: NULL pointer");
    EW_REQUIRE(F >= 1 && H >= 1 && W >= 1 && S >= 1 && (long long)H * W < (1LL << 31) && (long long)F * S < (1LL << 27),
               "ew_mvs_sgm_select: F = %d, H = %d, W = %d, S = %d must be positive, H W below 2^31 and F S below 2^27", F, H, W, S);
    EW_REQUIRE(D >= 1 && D <= EW_MVS_SGM_MAX_D, "ew_mvs_sgm_select: D = %d must be 1 .. %d", D, EW_MVS_SGM_MAX_D);
    EW_REQUIRE(view_begin >= 0 && n_views >= 1 && n_views <= F - view_begin,
               "ew_mvs_sgm_select: views %d .. %d + %d - 1 must lie in [0, F = %d)", view_begin, view_begin, n_views, F);
    EW_REQUIRE((((uintptr_t)inv | (uintptr_t)src_index | (uintptr_t)depth | (uintptr_t)conf | (uintptr_t)winner | (uintptr_t)winner_cost) & 3) == 0 &&
                   ((uintptr_t)agg & 1) == 0,
               "ew_mvs_sgm_select: the fp32 and int32 arrays must be 4-byte aligned, the volume 2-byte aligned");
    hipLaunchKernelGGL(sgm_select_kernel, dim3(stride_grid((long long)n_views * H * W)), dim3(NT), 0, (hipStream_t)stream, agg, inv, src_index,
                       depth, conf, winner, winner_cost, F, H, W, S, D, view_begin, n_views);
    return ew_check_launch("mvs_sgm sgm_select_kernel");
}
