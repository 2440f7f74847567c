// mvs_volume.h -- what the VOLUME instantiations of the two sweep tile kernels (mvs.hip, mvs_sphere.hip) share: the quantisation of a
// cost and the LDS staging that turns "one plane at a time, one pixel per thread" into contiguous runs of hypotheses per pixel in the
// uint16 [N,H,W,D] cost volume.  The tile is the sweeps' own: 256 threads, 32 x 8 pixels, thread t owns pixel
// (t & 31, t / 32).
#pragma once
#include "common.h"

// planes staged before a flush.  64 (33 KiB) would make a pixel's run a whole 128-byte line at D = 64, but with the sweeps' own 4 - 6 KiB
// it leaves 4 workgroups per CU where the fused sweep has 8, and the sweep is latency-bound (gathers, divisions): measured 1.40 x the
// fused sweep's time at 64 planes per flush.  32 planes: 17 KiB, 6 workgroups per CU, 64-byte runs.
constexpr int EW_MVS_STAGE_PLANES = 32;
constexpr int EW_MVS_STAGE_PITCH = EW_MVS_STAGE_PLANES + 2;   // uint16 per pixel in LDS: 17 dwords, odd, so the 64 lanes of a wave hit 64 banks
constexpr size_t EW_MVS_STAGE_BYTES = 256 * EW_MVS_STAGE_PITCH * sizeof(uint16_t);

// q = min(4095, (int)floorf(C cost_scale + 0.5f)); a NaN stores 4095
__device__ __forceinline__ uint16_t ew_mvs_quantise(float c, float cost_scale) {
    const float v = floorf(c * cost_scale + 0.5f);
    return (uint16_t)(!(v < (float)EW_MVS_COST_MAX) ? EW_MVS_COST_MAX : (v < 0.0f ? 0 : (int)v));
}

// Called by all 256 threads of a tile's workgroup once per plane, k = 0 .. D - 1 in order, with the thread's cost of plane k.  After
// every 32nd plane and after the last one the staged planes are written out: consecutive threads write consecutive hypotheses of a
// pixel, then the next pixel of the tile row -- whole runs of the volume when D <= 32.  view: the [H,W,D] volume of the tile's view.
__device__ __forceinline__ void ew_mvs_stage_cost(float c, float cost_scale, int k, int D, uint16_t* __restrict__ view, int H, int W) {
    extern __shared__ uint16_t ew_mvs_stage[];
    const int t = threadIdx.x;
    const int kc = k & (EW_MVS_STAGE_PLANES - 1);
    ew_mvs_stage[t * EW_MVS_STAGE_PITCH + kc] = ew_mvs_quantise(c, cost_scale);
    if (kc != EW_MVS_STAGE_PLANES - 1 && k != D - 1) return;
    const int k_lo = k - kc, n = kc + 1;
    __syncthreads();
    for (int i = t; i < 256 * n; i += 256) {
        const int p = i / n, kk = i - p * n;
        const int px = blockIdx.x * 32 + (p & 31), py = blockIdx.y * 8 + (p >> 5);
        if (px < W && py < H) view[((long long)py * W + px) * D + (k_lo + kk)] = ew_mvs_stage[p * EW_MVS_STAGE_PITCH + kk];
    }
    __syncthreads();                               // the next plane's staging writes come behind this flush's reads
}
