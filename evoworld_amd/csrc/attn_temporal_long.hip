// attn_temporal_long.hip -- temporal self-attention core for clips of more than 64 frames (gfx950, head_dim 64): the third kernel behind
// ew_attn_temporal_f16 (attention.hip holds the one-block kernel for T <= 32, the 2x2-block kernel for T <= 64 and the dispatch).
//
// Same decomposition and memory convention as those two: one wave per (batch, pixel, head) problem, four problems per 256-thread block;
// a problem's q / k / v / o are T rows of 128 bytes, S*ld apart; every global access is a coalesced 16-byte chunk (8 lanes per row; chunk
// idx = it*64 + lane -> row idx>>3, column idx&7) staged through wave-private LDS rows of 144 B.  The products are the same swapped MFMA
// 32x32x16 pair, S^T = K Q^T (lane = query, the lane's keys are (r&3) + 8*(r>>2) + 4*lh) and O^T = V^T P^T with P kept in registers.
//
// New here: the wave walks its problem in query blocks of 32 and, per query block, STREAMS the keys / values in blocks of 32 with an online
// softmax: a running maximum m, a running normaliser l and the two f32x16 output accumulators live across key blocks, and l and the
// accumulators are multiplied by alpha = exp2((m_old - m_new) * scale*log2 e) in every block (alpha = 1 where the maximum did not rise).
// The first block starts from m = -inf, l = 0, O = 0: alpha = exp2(-inf) = 0 there, and no block is ever fully masked (only keys >= T of
// the last block are), so m is finite from the first block on.  P is rounded to fp16 and l sums the SAME rounded values, as in the
// T <= 64 kernels (exp2_p32 below is this file's copy of attention.hip's helper: that file's device code must not change).
//
// LDS: TWO wave-private regions of 32 rows x 144 B, independent of T: 4 waves x 2 x 4608 = 36,864 B per block.  Region A holds the q rows
// of a query block until their fragments are in registers, then each K block in turn, and at the end of the query block its o rows; region
// B holds the V block.  The K / V rows of the NEXT key block are loaded into registers before the current block's MFMAs, so that their
// latency is covered by the math; K / V are re-read once per query block (T x 128 B each per problem: they stay in L2).
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int ROW = 144, REGION = 32 * ROW;

// P = exp2(s*c + nm) of one 32-key block, rounded to fp16; returns l + the sum of the SAME rounded values (the normaliser)
__device__ __forceinline__ float exp2_p32(const f32x16& sacc, float c, float nm, f16x8 (&pf)[2], float l) {
#pragma unroll
    for (int g2 = 0; g2 < 2; ++g2)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const f16 ph = (f16)__builtin_amdgcn_exp2f(fmaf(sacc[g2 * 8 + e], c, nm));
            l += (float)ph;
            pf[g2][e] = ph;
        }
    return l;
}

__global__ __launch_bounds__(256) void attn_temporal_long_kernel(const f16* __restrict__ q, const f16* __restrict__ k,
                                                                 const f16* __restrict__ v, f16* __restrict__ o, int B, int T,
                                                                 int S, int heads, int ld, int ld_o, float scale_log2e,
                                                                 long long n_prob) {
    __shared__ __attribute__((aligned(16))) char smem_tl[4 * 2 * REGION];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lh = lane >> 5, lr = lane & 31;
    // problem decode: an idle wave (pid >= n_prob) recomputes the last problem and stores nothing
    const long long pid = (long long)blockIdx.x * 4 + wave;
    const bool active = pid < n_prob;
    const long long pc = active ? pid : n_prob - 1;
    const int h = (int)(pc % heads);
    const long long bs = pc / heads;
    const int b = (int)(bs / S), s = (int)(bs - (long long)b * S);
    const long long row0 = (long long)b * T * S + s;           // row of frame 0; frame r is r*S rows further
    char* const ra = smem_tl + wave * (2 * REGION);             // q rows -> K blocks -> o rows
    char* const rb = ra + REGION;                               // V blocks
    const int nblk = (T + 31) >> 5;

    // 32 rows [r0, r0 + 32) of one operand into registers: rows >= T are zero (0 * garbage must not become NaN in P V)
    auto load32 = [&](const f16* __restrict__ src, int r0, f16x8 (&tt)[4]) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = it * 64 + lane;
            const int r = r0 + (idx >> 3);
            const f16x8 z = {};
            tt[it] = z;
            if (r < T) tt[it] = *(const f16x8*)(src + (row0 + (long long)r * S) * ld + h * 64 + (idx & 7) * 8);
        }
    };
    auto put32 = [&](char* reg, const f16x8 (&tt)[4]) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = it * 64 + lane;
            *(f16x8*)(reg + (idx >> 3) * ROW + (idx & 7) * 16) = tt[it];
        }
    };

    for (int qb = 0; qb < nblk; ++qb) {
        f16x8 tk[4], tv[4];
        // ---- q rows of this block through region A into operand fragments: lane (row lr, k-chunk lh) holds [st*16 + lh*8, +8) of its row
        f16x8 qf[4];
        {
            f16x8 tq[4];
            load32(q, qb * 32, tq);
            load32(k, 0, tk);
            load32(v, 0, tv);
            put32(ra, tq);
            ew_wave_lds_sync();
#pragma unroll
            for (int st = 0; st < 4; ++st) qf[st] = *(const f16x8*)(ra + lr * ROW + st * 32 + lh * 16);
        }
        float m = -INFINITY, l = 0.f;
        f32x16 oacc[2];
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[db][i] = 0.f;

        for (int kb = 0; kb < nblk; ++kb) {
            ew_wave_lds_sync();                                 // every lane has consumed regions A and B: they may be overwritten
            put32(ra, tk);
            put32(rb, tv);
            ew_wave_lds_sync();
            if (kb + 1 < nblk) {                                // the next block's rows travel while this block is computed
                load32(k, (kb + 1) * 32, tk);
                load32(v, (kb + 1) * 32, tv);
            }
            // ---- S^T = K Q^T: lane = query lr, keys kb*32 + (r&3) + 8*(r>>2) + 4*lh
            f32x16 sacc;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[i] = 0.f;
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const f16x8 kf = *(const f16x8*)(ra + lr * ROW + st * 32 + lh * 16);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[st], sacc, 0, 0, 0);
            }
            float mx = m;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (key >= T) sacc[r] = -INFINITY;              // only the last block has such keys, and never all of its 32
                mx = fmaxf(mx, sacc[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));             // both halves of a query now agree on the new running maximum
            // ---- online softmax: everything accumulated under the old maximum shrinks by alpha (0 in the first block, where m = -inf)
            const float alpha = __builtin_amdgcn_exp2f((m - mx) * scale_log2e);
            m = mx;
            f16x8 pf[2];
            l = exp2_p32(sacc, scale_log2e, -mx * scale_log2e, pf, l * alpha);
            // ---- O^T = alpha * O^T + V^T P^T: A fragment (row d = db*32 + lr, k-slot (g2, lh, e)) = v[key(g2, lh, e)][d]
#pragma unroll
            for (int db = 0; db < 2; ++db) {
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[db][i] *= alpha;
#pragma unroll
                for (int g2 = 0; g2 < 2; ++g2) {
                    f16x8 vf;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int key = 16 * g2 + 4 * lh + (e & 3) + 8 * (e >> 2);
                        vf[e] = *(const f16*)(rb + key * ROW + (db * 32 + lr) * 2);
                    }
                    oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[g2], oacc[db], 0, 0, 0);
                }
            }
        }
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
        // ---- o rows into region A (lane = query lr; d = 32*db + 8*(r>>2) + 4*lh + (r&3)), then coalesced stores of the rows < T
        ew_wave_lds_sync();
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                f16x4 ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = (f16)(oacc[db][r4 * 4 + e] * inv);
                *(f16x4*)(ra + lr * ROW + (32 * db + 8 * r4 + 4 * lh) * 2) = ov;
            }
        ew_wave_lds_sync();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = it * 64 + lane;
            const int r = qb * 32 + (idx >> 3);
            if (r < T && active)
                *(f16x8*)(o + (row0 + (long long)r * S) * ld_o + h * 64 + (idx & 7) * 8) =
                    *(const f16x8*)(ra + (idx >> 3) * ROW + (idx & 7) * 16);
        }
        ew_wave_lds_sync();                                     // region A is read out before the next query block's q rows land in it
    }
}

}  // namespace

// arguments already validated by ew_attn_temporal_f16 (attention.hip), which owns the dispatch
ew_status ew_attn_temporal_long_launch(const void* q, const void* k, const void* v, void* o, int B, int T, int S, int heads, int ld,
                                       int ld_o, float scale, long long n_prob, unsigned nblk, void* stream) {
    hipLaunchKernelGGL(attn_temporal_long_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const f16*)q, (const f16*)k,
                       (const f16*)v, (f16*)o, B, T, S, heads, ld, ld_o, scale * LOG2E, n_prob);
    return ew_check_launch("ew_attn_temporal_f16");
}
