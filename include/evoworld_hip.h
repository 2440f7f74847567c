/* evoworld_hip.h -- C ABI of libevoworld_hip.so (gfx950 / MI355X).
 *
 * The reference (JiahaoPlus/EvoWorld) has no FFI / plugin registry: its hot path is Python calling
 * third-party libraries (diffusers / torch / open3d / pyequilib).  This header is the drop-in boundary
 * the Python call surface (evoworld_amd/ *.py, mirroring evoworld/pipeline, evoworld/trainer/unet_plucker,
 * utils/plucker_embedding, evoworld/reprojection) binds through ctypes.  Each entry point cites the
 * reference interface (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (a torch tensor's data_ptr()); the library
 *     never allocates, frees or synchronises; every call is asynchronous on `stream` (a hipStream_t
 *     passed as void*; NULL = the default stream).
 *   - activations are fp16 channels-last: [N, H, W, C] == [tokens, C] row-major.
 *   - return value: 0 = OK, <0 = error; ew_last_error() returns a thread-local message.
 */
#ifndef EVOWORLD_HIP_H
#define EVOWORLD_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef int ew_status;
#define EW_OK 0
#define EW_ERR_INVALID_ARG (-1)
#define EW_ERR_UNSUPPORTED (-2)
#define EW_ERR_HIP (-3)

#define EW_ABI_VERSION 20
int ew_abi_version(void);
const char* ew_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Fused MFMA GEMM / implicit-GEMM convolution  (fp16 in, fp32 accumulate, fp16 out).
 *   acc[m][n] = sum_k A(m,k) * W[n][k]                    W row-major [N, K], K = taps*(c1+c2); in the conv modes the K axis
 *                                                         is ordered [channel chunk of 64][tap][64 channels] (chunk-major,
 *                                                         tap-minor: the taps of a chunk re-hit its input lines in L2)
 *   v   = acc + bias[n] + rowbias[(m / rows_per_group) * ld_rowbias + n]
 *   v   = act(v)            act 0: none; 1: SiLU; 2: GEGLU -> out has N/2 columns (see w layout note below); 3: erf GELU
 *   out = c_acc*v + c_r1*r1[m][n] + c_r2*r2[m][n]
 * A-operand addressing modes (the gather happens in the global->LDS DMA address, no im2col buffer):
 *   EW_A_DENSE   A(m, k)          = a[m*lda + k]                      (k < c1; then a2[m*lda2 + k-c1])
 *   EW_A_CONV3X3 m -> (img, oy, ox) on an [n_img, h_out, w_out] grid; tap = ky*3+kx;
 *                A(m, (tap, c))   = in[img, iy, ix, c], iy = oy*stride+ky-1, ix = ox*stride+kx-1, zero
 *                outside; with upsample=1 the input is read as nearest-x2 upsampled ([h_in,w_in] -> 2x).
 *                upsample=2: the same conv (stride 1, h_out = 2 h_in, w_out = 2 w_in) as four 2x2 phase convs over the SOURCE image:
 *                for output parity (a, b) = (oy & 1, ox & 1) the nine taps land on 2x2 source pixels, so `w` holds, per phase, the
 *                sums of the taps that share a pixel: [4 phases 2a+b][N][c1/64][4 taps 2r+c][64], tap (r, c) = source pixel
 *                (oy/2 + a-1+r, ox/2 + b-1+c), rows ky of 3x3 kernel row group r: a=0: {0} {1,2}, a=1: {0,1} {2}; columns likewise
 *                (evoworld_amd.ops.pack_convup2_weight).  K = 4 c1: 4/9 of the MFMA work.  One source (no a2 / c2), bias only
 *                (no rowbias / r1 / r2 / act), out / out_lo; N and c1 as ew_gemm_convup2_ok says; runs on generation 3 whatever
 *                ew_set_gemm_generation selected.  M, c1 and mode are the caller's 3x3 problem (M = n_img*h_out*w_out).
 *   EW_A_CONVT3  m -> (b, t, p) on a [B, T, P] grid; A(m, (kt, c)) = in[b, t+kt-1, p, c], zero outside.
 * In the conv modes channels [0,c1) come from `a`, [c1,c1+c2) from `a2` (the up-block skip concat,
 * evoworld/trainer/unet_plucker.py:458-475 + diffusers up blocks) without materialising the concat.
 * Replaces: torch.nn.Linear / Conv2d / Conv3d(3,1,1) calls inside the diffusers blocks instantiated at
 * evoworld/trainer/unet_plucker.py:126-244 (ResnetBlock2D, TemporalResnetBlock, Down/Upsample2D, Attention
 * projections, FeedForward/GEGLU, proj_in/out) and the AlphaBlender / residual adds around them.
 * Constraints: c1 % 64 == 0, c2 % 64 == 0 (pad channels), all pointers 16-byte aligned, ld* % 8 == 0.
 * GEGLU weight layout: rows are pre-interleaved in blocks of 16: tile rows [32q,32q+16) = value rows
 * 16q.., [32q+16,32q+32) = gate rows (N/2 + 16q..); bias likewise (evoworld_amd.unet packs this).
 */
enum { EW_A_DENSE = 0, EW_A_CONV3X3 = 1, EW_A_CONVT3 = 2 };
enum { EW_ACT_NONE = 0, EW_ACT_SILU = 1, EW_ACT_GEGLU = 2, EW_ACT_GELU = 3 /* erf GELU (CLIP ViT-H MLP) */ };

typedef struct ew_gemm_args {
    const void* a;      /* fp16 */
    const void* a2;     /* fp16 or NULL */
    const void* w;      /* fp16 [N, K] */
    const void* bias;   /* fp16 [N] or NULL */
    const void* rowbias;/* fp16 [G, N] or NULL */
    const void* r1;     /* fp16 [M, ld_r1] or NULL */
    const void* r2;     /* fp16 [M, ld_r2] or NULL */
    void* out;          /* fp16 [M, ld_out] */
    const void* zero_page; /* >= 256 bytes of device zeros (conv padding source) */
    int M, N;
    int c1, c2;         /* channels from a / a2 per tap */
    int lda, lda2;      /* row strides (elements) of a / a2 */
    int ld_out, ld_r1, ld_r2, ld_rowbias;
    int mode;           /* EW_A_* */
    int n_img, h_in, w_in, h_out, w_out, stride, upsample; /* EW_A_CONV3X3 */
    int tB, tT, tP;     /* EW_A_CONVT3 */
    int rows_per_group; /* rowbias group size in rows (>=1) */
    int act;            /* EW_ACT_* */
    float c_acc, c_r1, c_r2;
    /* Split residual stream (ABI 4): a residual-stream tensor x is carried as hi = fp16(x) (round to nearest even) plus an
     * int8 companion lo8, ONE byte per element with the same element strides: bits(x) ~= bits((float)hi) + 32 * lo8 on the
     * fp32 bit patterns, i.e. 8 more mantissa bits (~19 in all; the reference keeps the stream in fp32,
     * unified_loop_consistency.py:188) for 3 bytes per element.  Consumers that only need an fp16 operand read `hi` alone.
     * r1_lo / r2_lo (element strides ld_r1 / ld_r2) refine r1 / r2; out_lo (element stride ld_out) receives the lo8 of the
     * fp32 result.  Any of them may be NULL; not available with GEGLU.  (ABI 2-3 carried a second fp16 plane instead.) */
    const void* r1_lo;
    const void* r2_lo;
    void* out_lo;
    /* EW_A_CONV3X3 tap origin: 0 = iy = oy*stride + ky - 1 (symmetric padding 1); 1 = iy = oy*stride + ky, zero beyond the
     * bottom / right edge (F.pad(x, (0,1,0,1)) + stride-2 conv of diffusers Downsample2D(padding=0), the VAE encoder). */
    int conv_shift;
} ew_gemm_args;

ew_status ew_gemm_f16(const ew_gemm_args* args, void* stream);
/* 1 if ew_gemm_f16 runs EW_A_CONV3X3 with upsample = 2 for N output and C input channels (N % 320 == 0, C % 64 == 0), else 0: a weight loader asks
 * once per layer and packs either the phase form or the nine taps. */
int ew_gemm_convup2_ok(int N, int C);
/* Kernel generation behind ew_gemm_f16: 1 = 128x160 tile, 2 blocks/CU; 2 = persistent 3-stage ring, 256x160 / 128x256 tiles;
 * 3 (default) = persistent 256x320 (and 256x256) tile with a stream-K tail where N % 320 == 0 (or
 * N % 256 == 0) and the problem fills the chip, generation 2 for everything else.  Same arguments, same results to rounding;
 * kept selectable for A/B measurements. */
void ew_set_gemm_generation(int gen);
int ew_get_gemm_generation(void);
/* Debug aid for measurement tools (bench.py): rocprof-style name of the kernel variant the last ew_gemm_f16 call on this
   thread's library instance launched, e.g. "gemm3_kernel<0, 8>".  Not part of the reference surface. */
const char* ew_gemm_last_kernel(void);
void ew_set_gemm_debug(int flags);   /* bit 2 (value 4): generation 3 runs the whole-tile schedule -- no stream-K tail, no half split -- the twin the stream-K parity
                                        test compares against (same results up to fp32 summation order); 0 = normal.  (ABI <= 9 also had result-destroying
                                        ablation bits 0 / 1 and the halo-slab loader bits 3 / 4: removed in ABI 10.) */
/* Generation 3 splits the last round of output tiles along K over its 256 persistent workgroups when whole-tile rounds would
 * leave > 4 % of the chip idle (stream-K tail: fp32 partial accumulators handed over through a library-owned uncached
 * workspace, one per (device, stream), allocated on first use: 84 MB + 67 MB for the 256-wide instance).  Deterministic: the
 * split depends on the shape only.  A consumed hand-over flag is cleared by its consumer, so a captured launch can be replayed.
 * ew_gemm_streamk_status() synchronises and returns 0 when every hand-over completed, 1 if a finisher ever timed out
 * (results of that launch are invalid), -1 on a HIP error.  ew_set_gemm_debug(4) switches the split off. */
int ew_gemm_streamk_status(void);
/* Allocates the stream-K workspace of (current device, stream).  Optional in eager use (the first launch that wants the tail
 * allocates it, under a mutex); call it BEFORE capturing launches into a hipGraph -- allocation is illegal during capture, and a
 * captured launch on a stream without a workspace runs the whole-tile schedule instead. */
ew_status ew_gemm_streamk_init(void* stream);

/* CU budget of the persistent kernels (ABI 8).  The persistent GEMM / feed-forward kernels launch one workgroup per CU and size their
 * tile schedule and stream-K split from the CU count: 256 on an MI355X.  A caller that runs the library on a stream restricted to a
 * subset of the CUs (ew_stream_create_cu_mask: two independent forwards -- the two rows of the CFG batch the reference concatenates,
 * evoworld/pipeline/pipeline_evoworld.py:689-711 -- side by side on disjoint halves of the chip) sets the budget to that subset's size
 * first: with more workgroups than CUs a stream-K finisher could wait for a contributor that is not resident.  Process-wide; a multiple
 * of 8 in [8, 256].  Returns the previous value.  Set it BEFORE any stream of the partition is in use: the value is atomic, but a launch reads it
 * more than once, so a change racing a launch on another thread may size that launch inconsistently. */
int ew_set_cu_budget(int n_cus);
int ew_get_cu_budget(void);
/* A HIP stream whose kernels only run on CUs [first_cu, first_cu + n_cus) of the CU-mask bit order (hipExtStreamCreateWithCUMask).
 * Returns NULL and sets ew_last_error on failure.  Destroy with ew_stream_destroy. */
void* ew_stream_create_cu_mask(int first_cu, int n_cus);
ew_status ew_stream_destroy(void* stream);

/* Fused GEGLU feed-forward for 320-channel tokens (ABI 5; level 0 of the U-Net: 460800 tokens per forward, 15 feed-forwards):
 *   out = c_acc * (GEGLU(x W1^T + b1) W2^T + b2 + rowbias[m / rows_per_group]) + c_r1 * r1 + c_r2 * r2
 * = diffusers FeedForward(320, activation_fn="geglu") (net.0 GEGLU projection 320 -> 2 x 1280, net.2 Linear 1280 -> 320) of
 * BasicTransformerBlock.ff / TemporalBasicTransformerBlock.ff_in / .ff (instantiated via evoworld/trainer/unet_plucker.py:161-233)
 * with the residual / AlphaBlender epilogue of ew_gemm_f16; the 1280-wide intermediate never goes to HBM.  x: fp16 [M, 320]
 * (the LayerNorm output); w1p / b1p / w2p: the weights in the kernel's LDS-image packs (layout: csrc/ff_fused.hip, built by
 * evoworld_amd.ops.ff_pack); b2 fp16 [320]; r1 / r2 / out [M, 320] with optional lo8 companions as in ew_gemm_args. */
typedef struct ew_ff_args {
    const void* x;
    const void* w1p;
    const void* b1p;
    const void* w2p;
    const void* b2;
    const void* rowbias;   /* fp16 [G, ld_rowbias] or NULL */
    const void* r1;
    const void* r1_lo;
    const void* r2;
    const void* r2_lo;
    void* out;
    void* out_lo;
    const void* zero_page;
    int M, C, hidden;      /* C = 320, hidden = 1280 */
    int rows_per_group, ld_rowbias;
    float c_acc, c_r1, c_r2;
    /* (ABI 5-9 carried an optional LayerNorm prologue here -- x_lo / ln_gamma / ln_beta / addvec / add_rows_per_group / ln_eps / ln_folded; both
     * forms measured slower than the separate ew_layernorm_f16 launch on the final kernels (+9 ms and +1.1 ms per forward)
     * and were removed in ABI 10.) */
} ew_ff_args;
ew_status ew_ff_geglu320_f16(const ew_ff_args* args, void* stream);

/* GroupNorm statistics + apply, channels-last fp16, over a (virtual) channel concat.
 * The normalised tensor has C_tot channels in `groups` groups; a stats/apply call handles the C_src channels
 * [c_off, c_off+C_src) that live in tensor `x` ([n_slabs*rows, C_src]); a skip-concat input is covered by
 * two calls (one per source) -- groups may straddle the seam.  x_lo (may be NULL) is the lo8 companion of a
 * split residual stream (int8, one byte per element, see ew_gemm_args).
 * Statistics are DETERMINISTIC and cancellation-safe (no atomics), whatever a single row holds: ew_groupnorm_stats_f16
 * writes a per-(slab, row chunk, channel) (mean, M2) pair into the workspace -- every thread sums (x - K) and (x - K)^2
 * shifted by a pivot of its own, K = the first row it reads, and the threads of a chunk are combined with Chan's formula;
 * ew_groupnorm_finalize (one call per GroupNorm, after the stats calls of all its sources) combines the chunks the same
 * way in a fixed order to (mean, biased variance) per (slab, group); ew_groupnorm_apply_f16 reads those.
 * `ws`: ew_groupnorm_workspace_floats(n_slabs, rows, C_tot, groups) floats, uninitialised, private to this GroupNorm call.
 *        slab n = `rows` consecutive rows (rows = H*W for the per-frame GN of ResnetBlock2D / transformer
 *        norm / conv_norm_out; rows = T*H*W for TemporalResnetBlock's GN over [B,C,T,H,W]).
 * apply: y[row][c_off+c] = (x-mean)*rstd*gamma[c_off+c]+beta[c_off+c], optional SiLU; y row stride = C_tot.
 * Replaces torch.nn.GroupNorm + SiLU at the diffusers blocks instantiated by
 * evoworld/trainer/unet_plucker.py:161-233 and conv_norm_out (:236, 478-479). */
size_t ew_groupnorm_workspace_floats(int n_slabs, int rows, int C_tot, int groups);
ew_status ew_groupnorm_stats_f16(const void* x, const void* x_lo, float* ws, int n_slabs, int rows, int C_src, int c_off,
                                 int C_tot, int groups, void* stream);
ew_status ew_groupnorm_finalize(float* ws, int n_slabs, int rows, int C_tot, int groups, void* stream);
ew_status ew_groupnorm_apply_f16(const void* x, const void* x_lo, const float* ws, const void* gamma, const void* beta,
                                 void* y, int n_slabs, int rows, int C_src, int c_off, int C_tot, int groups, float eps,
                                 int silu, void* stream);
/* Split-operand form of the apply (ABI 10): with f the fp32 result, y = fp16(f) and y_lo = fp16(f - float(y)), both with row stride ld_y
 * (>= C_tot).  y_lo = y + C_tot with ld_y = 2 * C_tot gives rows [x_hi | x_lo]: the A operand of a consumer whose weights are packed
 * [W_hi | W_hi | W_lo] over three K blocks (second source a2 = a, c2 = C_tot), i.e. x W formed to ~2^-21 in both operands.  Used where the
 * per-group energy analysis (tests/analysis_fp16_floor.py --per-group) puts a large share of the fp16 operand-rounding distance to the
 * reference's fp32 result in layers that are < 1 % of the flops: conv_norm_out -> conv_out (unet_plucker.py:236, 478-480) and the
 * level-0 TransformerSpatioTemporalModel.norm -> proj_in. */
ew_status ew_groupnorm_apply_split_f16(const void* x, const void* x_lo, const float* ws, const void* gamma, const void* beta,
                                       void* y, void* y_lo, int ld_y, int n_slabs, int rows, int C_src, int c_off, int C_tot,
                                       int groups, float eps, int silu, void* stream);

/* LayerNorm over the last dim (fp16 in/out, fp32 two-pass statistics).  x_lo (may be NULL): lo8 companion of a split
 * residual stream (int8).  Optional fused pre-add: x' = x + addvec[row / rows_per_group][:] is what gets normalised, and x' is
 * written to x_out (fp16) -- plus its lo8 companion to x_out_lo when non-NULL -- (the time_pos_embed add in
 * TransformerSpatioTemporalModel).  C % 8 == 0, C <= 2048.
 * Replaces torch.nn.LayerNorm in Basic/TemporalBasicTransformerBlock (diffusers, via unet_plucker.py:13). */
ew_status ew_layernorm_f16(const void* x, const void* x_lo, const void* addvec, int rows_per_group, void* x_out,
                           void* x_out_lo, const void* gamma, const void* beta, void* y, int rows, int C, float eps,
                           void* stream);

/* Spatial self-attention core, head_dim 64: o = softmax(q k^T * scale) v per (sequence, head), flash-tiled
 * on MFMA 32x32x16 with the swapped product S^T = K Q^T so each query's softmax row is lane-local.
 * q,k: fp16 token-major with row stride ld_qk (head h at +64h); vt: V TRANSPOSED [heads*64, n_seq*S]
 * (row = channel, tokens contiguous; produced by ew_gemm_f16 with swapped operands); o: [n_seq*S, ld_o].
 * Replaces F.scaled_dot_product_attention in AttnProcessor2_0 for BasicTransformerBlock.attn1
 * (SURVEY.md §8a U10). */
ew_status ew_attn_spatial_f16(const void* q, const void* k, const void* vt, void* o, int n_seq, int S, int heads,
                              int ld_qk, long long ld_vt, int ld_o, float scale, void* stream);

/* Same core for q and k that arrive PRE-SCALED (ABI 6): the projection GEMM's epilogue multiplied both by sqrt(scale * log2 e)
 * (ew_gemm_args.c_acc, applied in fp32 before the single rounding to fp16, so q and k carry the same relative rounding error as
 * unscaled ones), which makes q.k the softmax exponent in log2 units.  The kernel then lets the MFMA subtract the running maximum
 * (C operand = -m) and drops the per-score multiply-add: o = softmax_2(q k^T) v.  Same layouts and restrictions as above.
 * Replaces the same F.scaled_dot_product_attention call. */
ew_status ew_attn_spatial_log2_f16(const void* q, const void* k, const void* vt, void* o, int n_seq, int S, int heads,
                                   int ld_qk, long long ld_vt, int ld_o, void* stream);

/* Temporal self-attention core over the frame axis (any T > 0, head_dim 64) on frame-major tokens
 * [B, T, S, *]: sequence (b, s) attends over t -- the [B*T,S,C] <-> [B*S,T,C] regroup of
 * TemporalBasicTransformerBlock is done by addressing, not by a copy.  q,k,v row stride ld; o row stride ld_o.
 * Three kernels, one wave per (b, s, head) each: T <= 32 the one-block kernel; 32 < T <= 64 the 2x2-block kernel with the whole
 * problem resident in LDS; T > 64 the key-streaming kernel (32-query blocks, keys / values in blocks of 32, online softmax; LDS
 * use independent of T).
 * Replaces SDPA in TemporalBasicTransformerBlock.attn1. */
ew_status ew_attn_temporal_f16(const void* q, const void* k, const void* v, void* o, int B, int T, int S, int heads,
                               int ld, int ld_o, float scale, void* stream);

/* Layout changes at the U-Net boundary.
 * nchw->nhwc: y[n,h,w,c_off+c] = fp16(scale * x[n,c,h,w]) for c < C (row stride ldc; other channels untouched).
 * nhwc->nchw: y[n,c,h,w] = fp32(x[n,h,w,c]) for c < C. */
ew_status ew_nchw_f32_to_nhwc_f16(const float* x, void* y, int N, int C, int H, int W, int ldc, int c_off, float scale,
                                  void* stream);
ew_status ew_nhwc_f16_to_nchw_f32(const void* x, float* y, int N, int C, int H, int W, int ldc, void* stream);
/* Split-operand form (ABI 9): with v = scale * x[n,c,h,w] and hi = fp16(v) the row receives THREE channel blocks,
 *   y[.., c_off + c] = hi,   y[.., lo_off + c_off + c] = fp16(v - hi),   y[.., dup_off + c_off + c] = fp16(hi * 2^-10),
 * i.e. the A operand [x_hi | x_lo | x_hi 2^-10] of a conv_in whose weight rows are packed [W_hi | W_hi | W_lo 2^10] (the power of two keeps
 * W_lo ~ 2^-12 |W| a normal fp16 number): x W is then formed to ~2^-21
 * instead of 2^-11 in BOTH operands at no MFMA cost, because conv_in pads its 18 input channels to one 64-channel K tile anyway
 * (3 * 20 <= 64).  The reference's conv_in runs on fp32 operands (weight_dtype = torch.float32, unified_loop_consistency.py:188;
 * evoworld/trainer/unet_plucker.py:131-136); its two fp16 roundings were 12-15 % each of the build's squared distance to the fp32 oracle. */
ew_status ew_nchw_f32_to_nhwc_split_f16(const float* x, void* y, int N, int C, int H, int W, int ldc, int c_off, int lo_off,
                                        int dup_off, float scale, void* stream);

/* Sinusoidal embedding of scalars (ABI 10): out fp16 [n_rows, dim] = [cos(v f_j) | sin(v f_j)], j < dim / 2, f_j = exp(-ln(10000) j / (dim / 2)),
 * v = vals[row % n_vals] (device fp32).  diffusers `Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0)` as the reference's U-Net applies it
 * to the timestep and to the three added time ids in every forward (evoworld/trainer/unet_plucker.py:395-420): two launches per forward instead of
 * the arange / exp / mul / cos / sin / cat chain of torch elementwise kernels. */
ew_status ew_sinusoid_embed_f16(const float* vals, int n_vals, int n_rows, int dim, void* out, void* stream);

/* Fused denoise-step glue: CFG combine + Euler (v-prediction) step + scale_model_input + concat for the next
 * step.  eps: fp16 NHWC [2*T, h, w, ld_eps] (rows [0,T) uncond, [T,2T) cond; first 4 channels);
 * latents: fp32 [T,4,h,w] state (updated in place); guidance [T]; next_in: fp16 NHWC [2*T,h,w,cpad], channels
 * [0,4) are rewritten with latents_new / sqrt(sigma_next^2+1) for both CFG rows (cond channels untouched).
 * Replaces evoworld/pipeline/pipeline_evoworld.py:691-695,709-714 + EulerDiscreteScheduler.step/scale_model_input. */
ew_status ew_euler_cfg_step(const void* eps, int ld_eps, float* latents, const float* guidance, float sigma,
                            float sigma_next, void* next_in, int cpad, int T, int h, int w, void* stream);
/* Same step writing the next model input as a split operand (ABI 9; see ew_nchw_f32_to_nhwc_split_f16): channels [0,4) = hi,
 * [lo_off, lo_off+4) = fp16(value - hi), [dup_off, dup_off+4) = fp16(hi * 2^-10), for both CFG rows.  lo_off, dup_off: multiples of 4. */
ew_status ew_euler_cfg_step_split(const void* eps, int ld_eps, float* latents, const float* guidance, float sigma,
                                  float sigma_next, void* next_in, int cpad, int lo_off, int dup_off, int T, int h, int w,
                                  void* stream);

/* Row softmax for the VAE's single-head attention (AutoencoderKLTemporalDecoder mid blocks, head_dim 512: diffusers
 * Attention with upcast_softmax; pipeline_evoworld.py:307-328,358-385 via vae.encode / vae.decode): the [S,S] score matrix
 * of one frame comes out of ew_gemm_f16 split (hi fp16 + lo8 int8, so no fp16 rounding before the exponential);
 * out[r][:] = softmax(decode(hi[r][:], lo[r][:])) in fp32, stored fp16.  lo (element stride ld) may be NULL.  cols % 8 == 0. */
ew_status ew_softmax_rows_f16(const void* hi, const void* lo, void* out, long long rows, int cols, long long ld, void* stream);

/* TemporalDecoder.time_conv_out: Conv3d(C, C, (3,1,1), padding (1,0,0)) over fp32 frames x [B,T,C,HW] (C <= 4; w [C,C,3],
 * bias [C]); zero padding along T.  Replaces the last op of diffusers TemporalDecoder.forward. */
ew_status ew_time_conv3_f32(const float* x, const float* w, const float* bias, float* y, int B, int T, int C, int HW, void* stream);

/* CLIP image-encoder path (pipeline_evoworld.py:255-305 `_encode_image`, :746-850
 * `_resize_with_antialiasing`).  All fp32 planes [planes, H, W]:
 *   ew_blur_axis_f32       1-D correlation along H (axis 0) or W (axis 1) with torch 'reflect' padding, pad_front = (ksize-1)/2
 *                          (`_filter2d` with a [1,k] / [k,1] Gaussian)
 *   ew_bicubic_resize_f32  F.interpolate(mode="bicubic", align_corners=True) (A = -0.75), optional per-channel affine
 *                          out = v*scale[c] + shift[c] (folds (x+1)/2 and the CLIP mean / std normalisation)
 *   ew_vit_patchify_f16    pixel_values [N,3,S,S] -> fp16 [N*(S/P)^2, ldk] im2col of the stride-P patch embedding, K order (c,ky,kx)
 *   ew_attn_small_f16      softmax(q k^T * scale) v for short sequences (S <= 2048) and head_dim % 8 == 0, <= 256 (ViT-H: 257 x 80),
 *                          one wave per query, fp32 math; q,k,v token-major rows with stride ld, head h at +h*D. */
ew_status ew_blur_axis_f32(const float* x, const float* kern, int ksize, float* out, long long planes, int H, int W, int axis,
                           void* stream);
ew_status ew_bicubic_resize_f32(const float* x, float* out, int N, int C, int H, int W, int Ho, int Wo, const float* scale,
                                const float* shift, void* stream);
ew_status ew_vit_patchify_f16(const float* x, void* out, int N, int S, int P, int ldk, void* stream);
ew_status ew_attn_small_f16(const void* q, const void* k, const void* v, void* o, int n_seq, int S, int heads, int D, int ld,
                            int ld_o, float scale, void* stream);

/* Optional fp8 (OCP e4m3) q / k / v projections (ABI 15; BASELINE.json configs[4]: "fp16 U-Net + fp8 MFMA QKV").  Replaces, when the model is
 * built with qkv_fp8, the Attention.to_q / to_k / to_v Linear calls of `attn1` reached from diffusers' BasicTransformerBlock and
 * TemporalBasicTransformerBlock (instantiated through evoworld/trainer/unet_plucker.py:126-244); everything else of the blocks stays fp16.
 * Off by default: it changes the numerics contract (tests/test_gpu_fp8_qkv.py states its tolerance) and makes no speed claim -- the non-scaled
 * fp8 MFMA runs at the fp16 rate on gfx950, what the path halves is operand bytes.  (ABI 3-9 exported the pair without c_acc; ABI 10-14 did not
 * export it.)
 *   ew_quant_rows_fp8  x fp16 [rows, K] -> q e4m3 bytes [rows, K] + scale fp32 [rows]: scale = amax(row) / 448 (1 for an all-zero row),
 *                      q = e4m3(x * (1 / scale)), round to nearest even.  K % 8 == 0, K <= 2048; x, q 16- / 8-byte aligned rows.
 *   ew_gemm_fp8        out[m][n] = fp16((sum_k a[m][k] * w[n][k]) * a_scale[m] * w_scale[n] * c_acc), fp32 accumulation on
 *                      v_mfma_f32_16x16x32_fp8_fp8.  a [M, K], w [N, K] e4m3 bytes (row stride K), a_scale [M], w_scale [N] fp32, out fp16 with
 *                      row stride ld_out >= N.  c_acc: the factor ew_gemm_args.c_acc is on the fp16 path (the log2 prescale of the spatial q|k
 *                      projection).  Swapping (a, a_scale) with (w, w_scale) gives the transposed product (V^T = W_v X^T).
 *                      K % 64 == 0, N % 4 == 0, ld_out % 4 == 0; a, w, w_scale 16-byte aligned, out 8-byte aligned. */
ew_status ew_quant_rows_fp8(const void* x, void* q, float* scale, int rows, int K, void* stream);
ew_status ew_gemm_fp8(const void* a, const float* a_scale, const void* w, const float* w_scale, void* out, int M, int N, int K,
                      long long ld_out, float c_acc, void* stream);

/* Plücker embedding: out[n, 0:3, y, x] = R_n d(y,x); out[n, 3:6] = t_n x (R_n d)  (fp32).
 * rays [H,W,3] fp32, c2w [N,3,4] fp32 -> out [N,6,H,W] fp32.
 * Replaces utils/plucker_embedding.py:221-255 (ray_c2w_to_plucker). */
ew_status ew_plucker_embed(const float* rays, const float* c2w, float* out, int N, int H, int W, void* stream);

/* Cube -> equirect gather through the integer LUT (face, v, u) int16 [H,W,3]; faces uint8
 * [V,6,res,res,face_channels] (face order right,left,bottom,top,front,back; 3 = packed RGB, 4 = RGBX words) -> pano uint8
 * [V,H,W,3].  Four pixels per thread, dword stores; the LUT is decoded once for all V views.
 * Replaces CubemapRenderer.cube_to_equirectangular_cuda, reproject_vggt_open3d_utils.py:542-614. */
ew_status ew_cube2equi_gather(const uint8_t* faces, int face_channels, const int16_t* lut, uint8_t* pano, int V, int H,
                              int W, int res, void* stream);

/* Depth lift: xyz[s,y,x] = R_s^T (K_s^-1 [u,v,1] z - t_s); depth [S,H,W] f32, extr [S,3,4] world->cam,
 * intr [S,3,3] -> xyz [S,H,W,3] f32.  Replaces vggt unproject_depth_map_to_point_map
 * (unified_loop_consistency.py:352,365-367). */
ew_status ew_depth_unproject(const float* depth, const float* extr, const float* intr, float* xyz, int S, int H, int W,
                             void* stream);

/* Percentile filter of the lifted point cloud (PointCloudProcessor.filter_predictions / _apply_confidence_filter,
 * reproject_vggt_open3d_utils.py:174-222,294-310): np.percentile(conf, q) needs the two order statistics around the
 * virtual index; ew_select_kth_f32 finds x_(k) and x_(k+1) (0-based, ascending) of n floats by an MSD radix select
 * (4 histogram passes + 1 tail pass, no sort) and writes them to out2[0..1] (device).  ws: ew_select_workspace_bytes().
 * ew_filter_compact keeps the points with conf >= thr IN ORDER (boolean-mask semantics): xyz [n,3] f32 -> out_xyz, colours
 * (images * 255 truncated to uint8, :286-292) -> out_rgbx (one R|G<<8|B<<16 word per point); *total = number kept.
 * img: [n,3] floats (img_nchw = 0) or [S,3,hw] planes (img_nchw = 1, n = S*hw).  ws: ew_filter_compact_workspace_bytes(n). */
size_t ew_select_workspace_bytes(void);
ew_status ew_select_kth_f32(const float* x, size_t n, size_t k, void* ws, float* out2, void* stream);
size_t ew_filter_compact_workspace_bytes(size_t n);
ew_status ew_filter_compact(const float* conf, size_t n, float thr, const float* xyz, const float* img, int img_nchw,
                            unsigned hw, float* out_xyz, unsigned* out_rgbx, void* ws, unsigned* total, void* stream);

/* Point splat into cubemap z-buffers: for view v, face f: p_cam = w2c[v][f] * p; u = fx*x/z+cx, ...;
 * nearest pixel, min depth wins (64-bit atomicMin of depth-bits<<32 | point index -> deterministic winner), z > near.
 * Every point is read once (16-byte loads) and tested against all V*6 matrices (wave-uniform, in SGPRs); fragments that a
 * relaxed read of the cell already beats skip the atomic.  zbuf: uint64 [V,6,res,res], 16-byte aligned, UNINITIALISED on entry: since
 * ABI 10 the call itself sets every cell to 0xFF..FF ("no fragment") before the splat (ABI <= 9: the caller pre-filled it).
 * ew_splat_resolve writes the winners' colours (0 background): rgb = packed RGB bytes (rgb_stride 3) or RGBX words
 * (rgb_stride 4, as ew_filter_compact emits); faces uint8 [V,6,res,res,face_channels] (3 | 4).
 * Replaces Open3D OffscreenRenderer point rendering driven by render_face/render_cubemap,
 * reproject_vggt_open3d_utils.py:617-666 (parity unpinned: Filament GL). */
ew_status ew_splat_cubemap(const float* xyz, size_t npts, const float* w2c, unsigned long long* zbuf, int V, int res,
                           float fx, float fy, float cx, float cy, float z_near, void* stream);
ew_status ew_splat_resolve(const unsigned long long* zbuf, const uint8_t* rgb, int rgb_stride, uint8_t* faces,
                           int face_channels, int V, int res, void* stream);

/* The 3D memory as a point cloud to take away (ABI 19; csrc/pointcloud.hip).  The reference exports the filtered cloud through
 * predictions_to_glb -> SceneBuilder.build_scene (reproject_vggt_open3d_utils.py:713-766, 349-455) and save_point_cloud_to_ply
 * (utils/plucker_embedding.py:334); the voxel-grid downsample in front of the export (and, opt-in, in front of the splat) follows
 * Open3D's voxel_down_sample convention.  n < 2^31 everywhere.
 * ew_points_bounds: out6 (device) = min x, y, z, max x, y, z over the points whose three coordinates are all finite, *n_finite (device)
 *   their count; n == 0 or no finite point: +inf x3, -inf x3 and 0.  ws: ew_points_bounds_workspace_bytes(n), 8-byte aligned.
 * ew_voxel_keys: for a finite point, per axis i = (long long)floorf((p - origin) / voxel) in float32 (a subtraction, an IEEE division,
 *   a floor; origin3 on the device, by convention min - 0.5f * voxel computed in float32), key = ix << 42 | iy << 21 | iz.  A non-finite
 *   point gets 2^63 - 1 (sorts last, dropped by ew_voxel_reduce).  An index outside [0, 2^21) stores 1 to *overflow (device; the caller
 *   zeroes it beforehand and discards the keys when it is set).
 * ew_voxel_reduce: sorted_keys ascending with perm the permutation that sorted them (key i belongs to point perm[i]; the sort is the
 *   caller's); one output per run of equal keys, in ascending key order: out_xyz = the mean of the run's points (fp64 sums, divided by the
 *   count in fp64, rounded to float32), out_rgba = per channel round-half-to-even of sum / count in integer arithmetic with alpha 255
 *   (rgbx: the RGBX words of ew_filter_compact, X ignored), out_count = the run's length; *n_voxels (device) = the number of runs.  The
 *   outputs hold n entries.  Work per run is bounded by log-depth segmented scans whatever its length.  No atomics: two calls are
 *   bit-identical.  ws: ew_voxel_reduce_workspace_bytes(n), 16-byte aligned. */
size_t ew_points_bounds_workspace_bytes(size_t n);
ew_status ew_points_bounds(const float* xyz, size_t n, void* ws, float* out6, unsigned long long* n_finite, void* stream);
ew_status ew_voxel_keys(const float* xyz, size_t n, const float* origin3, float voxel, long long* keys, int* overflow, void* stream);
size_t ew_voxel_reduce_workspace_bytes(size_t n);
ew_status ew_voxel_reduce(const long long* sorted_keys, const long long* perm, size_t n, const float* xyz, const uint8_t* rgbx,
                          float* out_xyz, uint8_t* out_rgba, int* out_count, void* ws, unsigned long long* n_voxels, void* stream);

/* Motion-JPEG frames encoded on the device (csrc/video.hip; added to ABI 19 without a bump: new symbols only).  The
 * reference's Navigator.save_video / save_gif (evoworld/inference/navigator_evoworld.py:233-274) hand the frames to imageio / ffmpeg;
 * here each frame becomes a baseline JPEG (ITU-T T.81: SOF0, 8 bit, JFIF YCbCr full range, Annex K Huffman tables, Annex K.1 / K.2
 * quantisation tables under libjpeg's quality rule, restart interval = one MCU row) that evoworld_amd/video.py wraps in an AVI.
 * subsampling: EW_JPEG_420 (MCU 16x16 = Y00 Y01 Y10 Y11 Cb Cr, chroma = the mean of 2x2 converted samples) or EW_JPEG_444 (MCU 8x8 =
 * Y Cb Cr).  mcu_rows = ceil(H / mcu), mcu_cols = ceil(W / mcu); partial MCUs replicate the last column and row.
 * ew_jpeg_dct_quant: frames uint8 [V,H,W,3] -> coef int16 [V, mcu_rows, mcu_cols, blocks_per_mcu, 64] (16-byte aligned), each block in
 *   zigzag order: float32 colour transform, orthonormal 8x8 DCT-II (rows, then columns), round-half-even of the IEEE quotient c / t,
 *   AC clamped to +-1023 and DC to [-1024, 1023].  quality 1 .. 100; V, H, W 1 .. 65535.
 * ew_jpeg_entropy: one restart segment per MCU row of a frame (n_segments = V * mcu_rows, below 2^31): the Huffman-coded, byte-stuffed
 *   bytes of segment s, padded with 1-bits, go to slots + s * slot_bytes and their count to seg_bytes[s] (device).  DC predictors start
 *   at 0 in every segment.  slot_bytes >= ew_jpeg_segment_slot_bytes(mcu_cols, blocks_per_mcu), the provable worst case of 416 bytes
 *   per block (26 bits per coefficient, doubled by stuffing); values outside what the tables hold are clamped, never overrun.
 * ew_jpeg_pack: out[seg_offsets[s] ...] = segment s, followed by the marker RSTm (FF D0+m, m = row mod 8) unless s is its frame's last
 *   row; seg_offsets int64 (device) is the caller's exclusive scan of seg_bytes + 2 (+ 0 for a last row); a segment that would leave
 *   out_bytes is skipped.  No atomics anywhere: two calls return identical bytes. */
#define EW_JPEG_420 420
#define EW_JPEG_444 444
size_t ew_jpeg_segment_slot_bytes(int mcu_cols, int blocks_per_mcu);
ew_status ew_jpeg_dct_quant(const uint8_t* frames, int16_t* coef, int V, int H, int W, int quality, int subsampling, void* stream);
ew_status ew_jpeg_entropy(const int16_t* coef, uint8_t* slots, int* seg_bytes, long long n_segments, int mcu_cols, int blocks_per_mcu,
                          size_t slot_bytes, void* stream);
ew_status ew_jpeg_pack(const uint8_t* slots, const int* seg_bytes, const long long* seg_offsets, uint8_t* out, long long n_segments,
                       int mcu_rows, size_t slot_bytes, long long out_bytes, void* stream);

/* Baseline JPEG frames decoded on the device (csrc/video_decode.hip; added to ABI 19 without a bump: new symbols only):
 * the way back from the files above, and from any SOF0 / 8-bit / three-component stream with sampling 22 11 11 or 11 11 11 and one
 * interleaved scan, to pixels; evoworld_amd/video.py parses the headers and cuts the scan into restart segments on the host.
 * ew_jpeg_huffman_decode: V frames with identical headers.  scan [scan_bytes] (device) holds their entropy-coded bytes; segment s is
 *   scan[seg_start[s], seg_start[s] + seg_bytes[s]) without its RSTm marker (seg_start int64, seg_bytes int32, device) and codes
 *   restart_interval MCUs in scan order, the last segment of a frame the rest (restart_interval 0: the frame is one segment);
 *   n_segments = V * ceil(mcu_rows * mcu_cols / interval).  tables: 4 x EW_JPEG_HUFF_TABLE_BYTES (device, 4-byte aligned) in the order DC
 *   luminance, DC chrominance, AC luminance, AC chrominance, each { uint16 look[512]: 9-bit prefix -> length << 8 | symbol, 0 where no
 *   code of <= 9 bits matches; int32 maxcode[18]: the largest code of length l = 1 .. 16, -1 without one; int32 valoff[18]: index of
 *   the first symbol of length l minus its first code; uint8 vals[256]: the symbols in code order }, built by the caller from the
 *   file's DHT segments.  coef int16 [V, mcu_rows, mcu_cols, blocks_per_mcu, 64], each block in zigzag order (the layout
 *   ew_jpeg_dct_quant writes), is zeroed and then filled; DC predictors start at 0 in every segment, FF 00 is unstuffed.  seg_status
 *   int32 [n_segments] receives EW_JPEG_SEG_OK or the first thing that stopped the segment, whose remaining coefficients stay 0:
 *   BAD_CODE (no Huffman code matches, or an EOBn symbol), INDEX (a run or ZRL leads past coefficient 63), SIZE (DC category > 11,
 *   AC size > 10), EXHAUSTED (the bytes end before the MCUs), LEFTOVER (more than 7 bits unread behind the last MCU), MARKER (an FF
 *   followed by anything but 00 inside the segment), RANGE (the segment leaves scan_bytes; nothing is read).  No read leaves a
 *   segment's bytes and no write its blocks.
 * ew_jpeg_idct: coef -> uint8 sample planes of the padded size, y [V, mcu_rows * m, mcu_cols * m] (m = 16 for blocks_per_mcu 6, 8 for
 *   3) and cb, cr [V, mcu_rows * 8, mcu_cols * 8] (8-byte aligned): coefficient * qtables entry (qtables uint8 [2][64] on the device,
 *   natural order, [0] luminance), the inverse of the encoder's orthonormal DCT along the columns and then the rows as fmaf chains,
 *   + 128, round half to even, clamp to 0 .. 255 (T.81's 8-bit sample).
 * ew_jpeg_planes_to_rgb: the planes of H x W frames -> rgb uint8 [V,H,W,3]: for EW_JPEG_420 the chroma planes upsampled with the centred
 *   triangle filter (3/4, 1/4 per axis, taps clamped to the padded plane), then R = Y + 1.402 Cr', G = Y - 0.344136286 Cb' - 0.714136286
 *   Cr', B = Y + 1.772 Cb' (Cb' = Cb - 128, Cr' = Cr - 128) in float32, round half to even, clamp.
 * ew_resize_linear_u8: src [V,H,W,3] -> dst [V,h,w,3], bilinear without antialiasing: source position (d + 0.5) * n_src / n_dst - 0.5,
 *   neighbours clamped to the image, float32 weights, round half to even (what cv2.resize(frame, (w, h)) states; not ew_resize_aa_u8). */
#define EW_JPEG_HUFF_TABLE_BYTES 1424
#define EW_JPEG_SEG_OK 0
#define EW_JPEG_SEG_BAD_CODE 1
#define EW_JPEG_SEG_INDEX 2
#define EW_JPEG_SEG_SIZE 3
#define EW_JPEG_SEG_EXHAUSTED 4
#define EW_JPEG_SEG_LEFTOVER 5
#define EW_JPEG_SEG_MARKER 6
#define EW_JPEG_SEG_RANGE 7
ew_status ew_jpeg_huffman_decode(const uint8_t* scan, long long scan_bytes, const long long* seg_start, const int* seg_bytes,
                                 const uint8_t* tables, int16_t* coef, int* seg_status, long long n_segments, int V, int mcu_rows,
                                 int mcu_cols, int blocks_per_mcu, int restart_interval, void* stream);
ew_status ew_jpeg_idct(const int16_t* coef, const uint8_t* qtables, uint8_t* y, uint8_t* cb, uint8_t* cr, int V, int mcu_rows, int mcu_cols,
                       int blocks_per_mcu, void* stream);
ew_status ew_jpeg_planes_to_rgb(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, uint8_t* rgb, int V, int H, int W, int subsampling,
                                void* stream);
ew_status ew_resize_linear_u8(const uint8_t* src, uint8_t* dst, int V, int H, int W, int h, int w, void* stream);

/* PNG files encoded on the device (csrc/png.hip; added to ABI 20 without a bump: new symbols only).  The frame dumps of
 * the reference's --save_frames runs go through PIL's Image.save on one host thread; here only a frame's compressed bytes leave the
 * GPU and evoworld_amd/png.py adds the chunk framing.  The stream: 8-bit RGB, colour type 2, no interlace; the filtered scanlines
 * (a type byte, then 3 W bytes per row) of a frame are cut into segments of rows_per_segment whole rows (a value above H means H; the
 * last segment of a frame may be ragged; segs_per_frame = ceil(H / rows_per_segment), n_segments = V * segs_per_frame, below 2^31;
 * a segment holds at most EW_PNG_MAX_SEGMENT_BYTES bytes).  Every segment is deflated on its own -- no back-reference reaches before
 * its first byte -- as one dynamic-Huffman block followed by an empty stored block (000, pad, 00 00 FF FF), so that the next segment
 * starts on a byte; a frame's last segment sets BFINAL on its block instead and pads with zero bits.  V, H, W 1 .. 65535.
 * ew_png_filter: frames uint8 [V,H,W,3] -> filtered uint8 [V,H,1+3W].  filter_mode 0 .. 4 forces None / Sub / Up / Average / Paeth
 *   (RFC 2083 section 6; bpp = 3, bytes left of the first pixel and above row 0 are 0, Average is floor((a + b) / 2), Paeth breaks ties
 *   in the order a, b, c); EW_PNG_FILTER_ADAPTIVE picks per row the type with the smallest sum of cost(v) = v < 128 ? v : 256 - v over
 *   the row's filtered bytes (libpng's minimum sum of absolute differences), a tie going to the lowest type.  The frames are read as
 *   words when they are 4-byte aligned and 3 W % 4 == 0.  adler int32 [n_segments, 2] receives the Adler-32 halves (a, b) of every
 *   segment's filtered bytes, each on its own (a starts at 1); the caller combines them: A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1).
 * ew_png_lz77: filtered -> tokens uint32 [n_segments, token_stride] (token_stride >= the bytes of a full segment: one token per byte
 *   at worst), n_tokens int32 [n_segments], hist int32 [n_segments, 286 + 30].  A literal is its byte in bits 0 - 7; a match has bit 31
 *   set, length - 3 in bits 0 - 7 and distance - 1 in bits 8 - 22, length 3 .. 258, distance 1 .. min(32768, position in the segment).
 *   hist counts the segment's literal/length symbols (the end-of-block symbol 256 once) and, from column 286 on, its distance codes.
 *   Greedy parse, one probe of a 3-byte hash per position.
 * ew_png_emit: the segments' final bytes.  Segment s goes to out[seg_offsets[s], seg_offsets[s] + seg_bytes[s]) (int64, device; the
 *   caller's exact sizes and their exclusive scan) and nowhere else; one whose range leaves out_bytes is skipped.  seg_mode int32:
 *   EW_PNG_SEG_CODED writes the tokens with the frame's codes -- luts uint32 [V, 286 + 30]: bit-reversed code | length << 16 per
 *   literal/length symbol, then per distance code; headers uint8 [V, header_stride] and header_bits int32 [V]: the block header
 *   (BFINAL = 0, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code and the coded lengths) as an LSB-first bit string --,
 *   EW_PNG_SEG_STORED copies the segment's filtered bytes as stored blocks of at most 65535 bytes (5 bytes of overhead each, BFINAL on
 *   a frame's last).  Extra bits go LSB-first.  No atomics anywhere: two calls return identical bytes. */
#define EW_PNG_FILTER_ADAPTIVE 5
#define EW_PNG_SEG_CODED 0
#define EW_PNG_SEG_STORED 1
#define EW_PNG_HIST_COLS 316
#define EW_PNG_MAX_SEGMENT_BYTES 1073741824
ew_status ew_png_filter(const uint8_t* frames, uint8_t* filtered, int* adler, int V, int H, int W, int filter_mode, int rows_per_segment,
                        void* stream);
ew_status ew_png_lz77(const uint8_t* filtered, uint32_t* tokens, int* n_tokens, int* hist, int V, int H, int W, int rows_per_segment,
                      long long token_stride, void* stream);
ew_status ew_png_emit(const uint32_t* tokens, const int* n_tokens, const uint8_t* filtered, const int* seg_mode,
                      const long long* seg_offsets, const long long* seg_bytes, const uint32_t* luts, const uint8_t* headers,
                      const int* header_bits, int header_stride, uint8_t* out, long long out_bytes, int V, int H, int W,
                      int rows_per_segment, long long token_stride, void* stream);

/* Plane-sweep multi-view stereo on posed perspective views (csrc/mvs.hip; added to ABI 20 without a bump: new symbols only, DESIGN.md
 * 4.8).  A weight-free depth source that stands in for the depth network of unified_loop_consistency.py:336-368 (VGGT-1B: depth,
 * confidence, cameras): here the cameras are known and depth comes from photo-consistency.  fp32 in the order written below; no atomics:
 * two calls return identical bits, and a view's outputs depend only on that view and its sources.
 * ew_mvs_luma_u8 (stands in for the network's own preprocessing, unified_loop_consistency.py:336-368): rgb uint8 [F,H,W,3] -> grey uint8
 *   [F,H,W] = (77 R + 150 G + 29 B + 128) >> 8.
 * ew_mvs_plane_sweep (unified_loop_consistency.py:336-368, the depth and depth_conf outputs): grey uint8 [F,H,W]; homographies fp32
 *   [F,S,D,3,3] row-major, reference pixel -> source pixel for S source slots and D planes; src_index int32 [F,S], the view a slot reads
 *   (outside [0, F), e.g. -1: the slot is absent); inv_depth fp32 [F,D].  For the reference pixel (x, y) -- integer indices, the pixel
 *   convention of ew_depth_unproject --: q_i = (h_i0 x + h_i1 y) + h_i2, sx = q0 / q2, sy = q1 / q2; AD = |I_ref(x, y) - bilinear(I_src,
 *   sx, sy)| with x0 = floor(sx), ax = sx - x0, x1 = min(x0 + 1, W - 1) (rows alike), top = v00 (1 - ax) + v01 ax, bot = v10 (1 - ax) +
 *   v11 ax, value = top (1 - ay) + bot ay; AD = oob_cost unless q2 > 0 and 0 <= sx <= W - 1 and 0 <= sy <= H - 1.  A = the sum of AD over
 *   the present slots in slot order; C(k) = (the sum over the window's rows, top to bottom, of the sum over a row's taps, left to right,
 *   of A) / (taps inside the reference image x present slots): the mean over the (2 patch_radius + 1)^2 window, taps outside the image
 *   dropped, of the mean over the sources.  Winner k* = the lowest C, ties to the lowest k.  With 0 < k* < D - 1 and curv = (C(k* - 1) +
 *   C(k* + 1)) - 2 C(k*) > 0: off = clamp(0.5 (C(k* - 1) - C(k* + 1)) / curv, -0.5, 0.5) and the inverse depth moves from inv_depth[k*]
 *   by |off| of the way to the neighbour on that side; otherwise it is inv_depth[k*].  depth = 1 / that.  conf = (C2 - C1) / max(C2,
 *   1e-6), C1 = C(k*), C2 = the lowest C among the planes with |k - k*| > 1; 0 when there is no such plane or no slot is present (then
 *   every C is 0 and k* = 0).  Outputs depth, conf, winner_cost fp32 [F,H,W], winner int32 [F,H,W].  patch_radius 0 .. 3.
 * ew_mvs_consistency (unified_loop_consistency.py:336-368, what makes depth_conf mean agreement between views): depth fp32 [F,H,W];
 *   rel_pose fp32 [F,S,3,4], reference camera -> source camera (R | t); src_index as above; pinhole fx, fy, cx, cy.  Per pixel: Xc =
 *   ((x - cx) z / fx, (y - cy) z / fy, z), Xs = R Xc + t (each row ((r0 xc + r1 yc) + r2 z) + t); a slot agrees when Xs.z > 0, the nearest
 *   pixel (floor((fx Xs.x / Xs.z + cx) + 0.5), rows alike) lies in the source and |depth_src there - Xs.z| <= rel_tol Xs.z.  conf [F,H,W]
 *   is set to 0, in place, where fewer than min_consistent slots agree. */
ew_status ew_mvs_luma_u8(const uint8_t* rgb, uint8_t* grey, int F, int H, int W, void* stream);
ew_status ew_mvs_plane_sweep(const uint8_t* grey, const float* homographies, const int* src_index, const float* inv_depth, float* depth,
                             float* conf, int* winner, float* winner_cost, int F, int H, int W, int S, int D, int patch_radius,
                             float oob_cost, void* stream);
ew_status ew_mvs_consistency(const float* depth, const float* rel_pose, const int* src_index, float* conf, int F, int H, int W, int S,
                             float fx, float fy, float cx, float cy, float rel_tol, int min_consistent, void* stream);

/* Sphere-sweep multi-view stereo on posed equirectangular panoramas (csrc/mvs_sphere.hip; added to ABI 20 without a bump: new symbols
 * only).  The stage above without the 90-degree crop: concentric spheres around each panorama camera take the place of the
 * planes, the warp goes through the sphere, the lift is spherical.  Stands in for the same lines of the reference
 * (unified_loop_consistency.py:336-368).  fp32 in the order written below; no atomics: two calls return identical bits, and a view's
 * outputs depend only on that view and its sources.  PI = 3.14159265358979323846f, Wf = (float)We, Hf = (float)He.
 * Pixel <-> direction, the map of ew_equi2pers (x right, y down, z forward):
 *   dir(x, y), integer indices: lon = ((x - Wf 0.5) - 0.5) ((2 PI) / Wf), lat = ((y - Hf 0.5) - 0.5) (PI / Hf), dir = (cosf(lat) sinf(lon),
 *     sinf(lat), cosf(lat) cosf(lon)).
 *   pix(X, Y, Z): nrm = sqrtf((X X + Y Y) + Z Z), lon = atan2f(X, Z), lat = asinf(clamp(Y / nrm, -1, 1)), u = ((lon Wf) / (2 PI) + Wf 0.5)
 *     + 0.5, v = ((lat Hf) / PI + Hf 0.5) + 0.5.
 *   bilinear(I, u, v): u <- u - floorf(u / Wf) Wf, v <- clamp(v, 0, He - 1); x0 = floor(u) (We -> 0), ax = u - floor(u), x1 = (x0 + 1) mod
 *     We; y0 = floor(v), ay = v - y0, y1 = min(y0 + 1, He - 1); top = v00 (1 - ax) + v01 ax, bot = v10 (1 - ax) + v11 ax, value = top (1 -
 *     ay) + bot ay -- as ew_equi2pers samples.
 * ew_mvs_sphere_sweep: grey uint8 [F,He,We] (ew_mvs_luma_u8); rel_pose fp32 [F,S,3,4], reference panorama camera -> source panorama
 *   camera (R | t); src_index int32 [F,S] (outside [0, F): the slot is absent); inv_dist fp32 [F,D].  For the reference pixel (x, y) and
 *   hypothesis k: rad = 1 / inv_dist[k], P = dir(x, y) rad (three products), Ps = R P + t, each row ((r0 px + r1 py) + r2 pz) + t; AD =
 *   |I_ref(x, y) - bilinear(I_src, pix(Ps))|, and AD = 0 where |Ps| is 0 or not finite.  Every direction lands in the source: there is no
 *   out-of-image cost.  A = the sum of AD over the present slots in slot order; C(k) = (the sum over the window's rows inside [0, He), top
 *   to bottom, of the sum over a row's 2 patch_radius + 1 taps, left to right, columns taken modulo We, of A) / ((2 patch_radius + 1) x
 *   rows inside x present slots).  Winner, ties, parabola refinement (here of the inverse distance), runner-up C2 among |k - k*| > 1,
 *   conf = (C2 - C1) / max(C2, 1e-6) and conf = 0 without such a hypothesis or without a present slot: word for word the rules of
 *   ew_mvs_plane_sweep.  Outputs dist (the RADIAL distance 1 / inverse distance, not z), conf, winner_cost fp32 [F,He,We], winner int32
 *   [F,He,We].  patch_radius 0 .. 3, We >= 2 patch_radius + 1.
 * ew_mvs_sphere_consistency: dist fp32 [F,He,We]; rel_pose, src_index as above.  Per pixel: P = dir(x, y) dist, Ps = R P + t as above, nrm
 *   = |Ps| as in pix; a slot agrees when nrm > 0 and finite and |dist_src[yi, xi] - nrm| <= rel_tol nrm at the nearest pixel of Ps'
 *   direction, xi = floor(u + 0.5) mod We, yi = clamp(floor(v + 0.5), 0, He - 1) with (u, v) = pix(Ps).  conf [F,He,We] is set to 0, in
 *   place, where fewer than min_consistent slots agree.
 * ew_pano_unproject (the spherical counterpart of ew_depth_unproject): dist fp32 [F,He,We]; c2w fp32 [F,3,4], panorama camera -> world
 *   (R | t) -> xyz fp32 [F,He,We,3] = R (dir(x, y) dist) + t, rows in the order above. */
ew_status ew_mvs_sphere_sweep(const uint8_t* grey, const float* rel_pose, const int* src_index, const float* inv_dist, float* dist,
                              float* conf, int* winner, float* winner_cost, int F, int He, int We, int S, int D, int patch_radius,
                              void* stream);
ew_status ew_mvs_sphere_consistency(const float* dist, const float* rel_pose, const int* src_index, float* conf, int F, int He, int We,
                                    int S, float rel_tol, int min_consistent, void* stream);
ew_status ew_pano_unproject(const float* dist, const float* c2w, float* xyz, int F, int He, int We, void* stream);

/* Semi-global aggregation of the sweeps' cost volume (csrc/mvs_sgm.hip and the volume variants in csrc/mvs.hip, csrc/mvs_sphere.hip;
 * added to ABI 20 without a bump: new symbols only).  Opt-in: between the cost and the winner, 1-D dynamic programmes
 * along 4 or 8 path directions tie neighbouring pixels together (Hirschmueller's semi-global matching); ew_mvs_plane_sweep and
 * ew_mvs_sphere_sweep are untouched.  A cost volume is uint16 [N,H,W,D], hypothesis innermost, values <= EW_MVS_COST_MAX; it holds the
 * views view_begin .. view_begin + N - 1 of a batch of F.  No atomics anywhere: two calls return identical bits, and a view's outputs
 * depend only on that view and its sources.
 * ew_mvs_plane_sweep_volume / ew_mvs_sphere_sweep_volume: the inputs of ew_mvs_plane_sweep / ew_mvs_sphere_sweep (grey holds all F views:
 *   the sources may lie outside the range written) -> cost uint16 [n_views,H,W,D] of the views view_begin .. view_begin + n_views - 1 (0
 *   <= view_begin, 1 <= n_views <= F - view_begin).  C(k) is exactly the C(k) defined above for the fused sweep -- one cost routine is
 *   instantiated for both, so the bits of C agree -- and the entry stored is q = min(4095, (int)floorf(C cost_scale + 0.5f)) (product and
 *   sum rounded separately; cost_scale positive and finite); a NaN stores 4095.  A view without a present slot stores 0 everywhere.
 * ew_mvs_sgm_aggregate: cost -> agg uint16 [N,H,W,D] (another buffer).  0 <= P1 <= P2 <= 4095, paths 4 or 8, 1 <= D <= EW_MVS_SGM_MAX_D.
 *   Path directions r = (dx, dy), in order: (+1, 0), (-1, 0), (0, +1), (0, -1), (+1, +1), (-1, -1), (-1, +1), (+1, -1); the last four only
 *   with paths = 8.  For the pixel p and its predecessor q = p - r: L_r(p, k) = C(p, k) when q is outside the image; otherwise, with m =
 *   min_j L_r(q, j): L_r(p, k) = C(p, k) + min(L_r(q, k), L_r(q, k - 1) + P1 [k > 0], L_r(q, k + 1) + P1 [k < D - 1], m + P2) - m.
 *   agg(p, k) = the sum over r of L_r(p, k).  Integers throughout: L <= 4095 + P2 <= 8190, agg <= 65520; exact and independent of any
 *   order.  The columns of a panorama do NOT wrap here: a ring has no start, so column 0 has no predecessor for (+1, 0) and column W - 1
 *   none for (-1, 0), whichever sweep made the volume.  Views are aggregated independently of one another.
 * ew_mvs_sgm_select: agg uint16 [n_views,H,W,D] of the views view_begin .. ; inv fp32 [F,D] (inverse depths or distances); src_index int32
 *   [F,S] (only the number of present slots of a view is used).  The rules of ew_mvs_plane_sweep, word for word, on S(k) = (float)agg(k)
 *   in place of C(k): winner k* = the lowest S, ties to the lowest k; with 0 < k* < D - 1 and curv = (S(k* - 1) + S(k* + 1)) - 2 S(k*) > 0:
 *   off = clamp(0.5 (S(k* - 1) - S(k* + 1)) / curv, -0.5, 0.5) and the inverse moves from inv[k*] by |off| of the way to the neighbour on
 *   that side; out = 1 / inverse; conf = (S2 - S1) / max(S2, 1e-6), S1 = S(k*), S2 = the lowest S among |k - k*| > 1; conf = 0 without such
 *   a hypothesis or when the view has no present slot.  Outputs depth (or distance), conf, winner_cost fp32 and winner int32, each
 *   [n_views,H,W]; winner_cost = S1 is in AGGREGATED units (the sum over the paths of quantised costs), not in grey levels. */
#define EW_MVS_COST_MAX 4095
#define EW_MVS_SGM_MAX_D 256
ew_status ew_mvs_plane_sweep_volume(const uint8_t* grey, const float* homographies, const int* src_index, const float* inv_depth,
                                    uint16_t* cost, int F, int H, int W, int S, int D, int patch_radius, float oob_cost, float cost_scale,
                                    int view_begin, int n_views, void* stream);
ew_status ew_mvs_sphere_sweep_volume(const uint8_t* grey, const float* rel_pose, const int* src_index, const float* inv_dist, uint16_t* cost,
                                     int F, int He, int We, int S, int D, int patch_radius, float cost_scale, int view_begin, int n_views,
                                     void* stream);
ew_status ew_mvs_sgm_aggregate(const uint16_t* cost, uint16_t* agg, int N, int H, int W, int D, int P1, int P2, int paths, void* stream);
ew_status ew_mvs_sgm_select(const uint16_t* agg, const float* inv, const int* src_index, float* depth, float* conf, int* winner,
                            float* winner_cost, int F, int H, int W, int S, int D, int view_begin, int n_views, void* stream);

/* Zero-mean normalised cross-correlation as the sweeps' matching cost (csrc/mvs_zncc.hip; added to ABI 20 without a bump: new symbols
 * only).  Opt-in, for views whose exposure, contrast or tone drift against each other: a sum of absolute differences
 * reads such a drift as a depth error, a correlation of zero-mean patches does not.  The four SAD entries above are untouched.  Stands in
 * for the same lines of the reference (unified_loop_consistency.py:336-368).  fp32 in the order written below, sqrtf and IEEE division
 * only; no atomics: two calls return identical bits, and a view's outputs depend only on that view and its sources.
 * Notation: reference view f, pixel p, hypothesis k, present source slot s; nf = (float)n.
 * Window: the (2 patch_radius + 1)^2 window of p.  Plane: only the taps inside the reference image count.  Sphere: only the rows inside
 *   [0, He) count, and the columns are taken modulo We.  n = the taps that count.  patch_radius 1 .. 3 (a single tap has no variance: 0 is
 *   refused with EW_ERR_INVALID_ARG); sphere: We >= 2 patch_radius + 1.
 * Samples: a(t) = I_ref(t) - 128; b(t) = bilinear(I_src, warp_k(t)) - 128, the warp and the bilinear blend exactly those of
 *   ew_mvs_plane_sweep / ew_mvs_sphere_sweep (same formulas, same order; the 128 is subtracted last).  Plane: a tap whose sample leaves
 *   the source -- q2 <= 0 (or not a number) or (sx, sy) outside [0, W - 1] x [0, H - 1] -- makes the whole window of that slot invalid.
 *   Sphere: a point on the source's centre or a non-finite point (|Ps| not positive and finite) gives b(t) = a(t), the neutral choice
 *   ew_mvs_sphere_sweep makes with AD = 0; no window is invalid.
 * Sums: Sa, Saa, Sb, Sbb, Sab = the sums of a, a a, b, b b, a b over the window, each product rounded, then added in the box filter's
 *   order: a row's taps left to right starting from 0, then the row sums top to bottom starting from 0.
 * Correlation: cov = nf Sab - Sa Sb; va = max(nf Saa - Sa Sa, 0), vb = max(nf Sbb - Sb Sb, 0); fl = var_floor (nf nf); den = sqrtf(va vb +
 *   fl fl); zncc = cov / den, and 0 where den is 0 (possible only with var_floor = 0).  var_floor is in grey levels squared, finite and not
 *   negative: with var_floor > 0 a flat window scores zncc = 0, never a NaN.
 * Cost per slot: cost_s = 100 (1 - zncc), a percentage in [0, 200]; an invalid plane window gives cost_s = oob_cost (also in percent).
 * Cost per hypothesis: C(k) = (the sum of cost_s over the present slots in slot order, starting from 0) / present slots.  A view without a
 *   present slot: every C is 0, k* = 0, conf = 0, as in the SAD entries.
 * ew_mvs_plane_sweep_zncc / ew_mvs_sphere_sweep_zncc: the arguments of ew_mvs_plane_sweep / ew_mvs_sphere_sweep plus var_floor.  Winner,
 *   ties, parabola, runner-up, confidence and the four outputs follow the rules of ew_mvs_plane_sweep, word for word, on this C;
 *   winner_cost is in percent.
 * ew_mvs_plane_sweep_zncc_volume / ew_mvs_sphere_sweep_zncc_volume: the arguments of ew_mvs_plane_sweep_volume /
 *   ew_mvs_sphere_sweep_volume plus var_floor -> cost uint16 [n_views,H,W,D]: q = min(4095, (int)floorf(C cost_scale + 0.5f)) of exactly the
 *   C of the fused entry (one cost routine is instantiated for both).  cost_scale = 16 maps 200 % to 3200. */
ew_status ew_mvs_plane_sweep_zncc(const uint8_t* grey, const float* homographies, const int* src_index, const float* inv_depth, float* depth,
                                  float* conf, int* winner, float* winner_cost, int F, int H, int W, int S, int D, int patch_radius,
                                  float oob_cost, float var_floor, void* stream);
ew_status ew_mvs_plane_sweep_zncc_volume(const uint8_t* grey, const float* homographies, const int* src_index, const float* inv_depth,
                                         uint16_t* cost, int F, int H, int W, int S, int D, int patch_radius, float oob_cost, float var_floor,
                                         float cost_scale, int view_begin, int n_views, void* stream);
ew_status ew_mvs_sphere_sweep_zncc(const uint8_t* grey, const float* rel_pose, const int* src_index, const float* inv_dist, float* dist,
                                   float* conf, int* winner, float* winner_cost, int F, int He, int We, int S, int D, int patch_radius,
                                   float var_floor, void* stream);
ew_status ew_mvs_sphere_sweep_zncc_volume(const uint8_t* grey, const float* rel_pose, const int* src_index, const float* inv_dist,
                                          uint16_t* cost, int F, int He, int We, int S, int D, int patch_radius, float var_floor,
                                          float cost_scale, int view_begin, int n_views, void* stream);

/* Equirect -> perspective bilinear gather (pyequilib Equi2Pers restatement; unified_loop_consistency.py:299-334).
 * equi uint8 [F,He,We,3]; rot [F,3,3] f32 (camera->pano rotation); out uint8 [F,Hp,Wp,3]. */
ew_status ew_equi2pers(const uint8_t* equi, const float* rot, uint8_t* out, int F, int He, int We, int Hp, int Wp,
                       float fov_x_deg, void* stream);

/* Pillow-exact antialiased bilinear resize of 8-bit RGB images (two fixed-point passes, horizontal then vertical, 8-bit
 * intermediate), i.e. what torchvision.transforms.Resize does to the PIL memory panoramas before they enter the pipeline
 * (dataset/CameraTrajDataset.py:586-619 via unified_loop_consistency.py:422).  Coefficient tables kk [n_out, ksize] (int32,
 * 22 fractional bits) and bounds [n_out, 2] = (xmin, count) are built on the host (evoworld_amd.reprojection.resample_coeffs).
 * src [V,Hi,Wi,3] -> tmp [V,Hi,Wo,3] -> dst [V,Ho,Wo,3].  ew_u8_hwc_to_f32_chw: (x/255)*2-1 -> fp32 [V,3,H,W]. */
ew_status ew_resize_aa_u8(const uint8_t* src, uint8_t* tmp, uint8_t* dst, const int* kk_h, const int* bounds_h, int ksize_h,
                          const int* kk_v, const int* bounds_v, int ksize_v, int V, int Hi, int Wi, int Ho, int Wo, void* stream);
ew_status ew_u8_hwc_to_f32_chw(const uint8_t* src, float* dst, int V, int H, int W, void* stream);
/* The 8-bit frame the reference carries between segments: fp32 [V,3,H,W] in [-1,1] -> u8 [V,H,W,3] =
 * round_half_even(clamp(x/2+0.5, 0, 1)*255), i.e. the pipeline's PIL output (pipeline_evoworld.py:727-732 via diffusers
 * VideoProcessor) that unified_loop_consistency.py:418-419,432-436 feeds to the next segment and to pano->pers. */
ew_status ew_f32_chw_to_u8_hwc(const float* src, uint8_t* dst, int V, int H, int W, void* stream);

/* Yaw rotation of V equirectangular panoramas, one yaw per panorama (Navigator.rotate_panorama, navigator_evoworld.py:466-512,
 * the turn between two straight runs of navigate_path :335-392): nearest-neighbour gather dst[v,c,y,x] = src[v,c,vi(y),ui(v,x)]
 * whose indices reproduce the reference's float32 torch operations bit for bit (the sequence is spelled out in csrc/reproject.hip).
 * src_u8 = 0: src fp32 [V,3,H,W]; src_u8 = 1: src uint8 [V,H,W,3], converted (x/255)*2-1 in the same pass (bit-identical to
 * ew_u8_hwc_to_f32_chw followed by the fp32 form).  yaw_deg fp32 [V] (device), degrees; dst fp32 [V,3,H,W].  H, W < 2^24;
 * fp32 operands 4-byte aligned. */
ew_status ew_pano_yaw_rotate(const void* src, int src_u8, const float* yaw_deg, float* dst, int V, int H, int W, void* stream);

/* Per-frame PSNR / SSIM inputs of video pairs (ABI 12; evoworld/metrics/calculate_all_metrics.py:222-226, which runs
 * other_metrics/calculate_psnr.py:6-15 and calculate_ssim.py:6-40 per frame and channel in float64 on the CPU).
 * a, b: layout 0 = uint8 [F,H,W,C] (a pixel is float32(k) / 255.0f, correctly rounded, as torch's uint8 / 255.0),
 *       layout 1 = fp32 [F,C,H,W] (values as they are).  C = 1 or 3.  what: bit 0 SSE, bit 1 SSIM.
 * sse [F] (fp64, device): sum over C*H*W of d*d with d = a - b and d*d both rounded to float32 (numpy on float32 arrays), summed in
 *   fp64; the caller forms mse = sse / (C*H*W) and PSNR (100 when mse < 1e-10).
 * ssim [F] (fp64, device): the widened values, window outer(g, g) with g = cv2.getGaussianKernel(11, 1.5) (double), 'valid' region
 *   only ([5:-5, 5:-5]: no border handling), sigma^2 = E[x^2] - mu^2, C1 = 0.01^2, C2 = 0.03^2; the map's mean over (H-10)*(W-10)
 *   per channel, then the mean over the channels.  Needs H, W >= 11.
 * Fixed-order partial sums, no atomics: two calls are bit-identical.  workspace: ew_video_metrics_workspace_bytes(F, C, H, W) bytes
 * (8-byte aligned).  Refused: C not in {1, 3}, F, H or W <= 0, H or W < 11 with SSIM, a NULL output that `what` asks for. */
size_t ew_video_metrics_workspace_bytes(int F, int C, int H, int W);
ew_status ew_video_metrics(const void* a, const void* b, int layout, int F, int C, int H, int W, int what, double* sse, double* ssim,
                           void* workspace, void* stream);

/* The same two quantities under one weight per image row (ABI 18): WS-PSNR / WS-SSIM of equirectangular frames when row_w is the
 * cosine of the row's latitude (evoworld_amd.metrics.latitude_weights); the kernel itself is projection-agnostic.  Nothing of this is
 * in the reference.  a, b, layout, F, C, H, W, what: as ew_video_metrics.  row_w: fp64 [H] on the device, expected finite and >= 0
 * (the Python wrapper checks; the library does not read it on the host).
 * wsse [F]:  sum over c, y, x of row_w[y] * d2(c,y,x), d2 the float32 (a - b)^2 of ew_video_metrics widened to fp64 before the
 *   multiplication; not normalised: the caller forms wmse = wsse / (C * W * sum_y row_w[y]).
 * wssim [F]: (1/C) sum_c [ sum_{i<H-10, j<W-10} row_w[i+5] S_c(i,j) ] / [ (W-10) sum_{i<H-10} row_w[i+5] ] with S_c the SSIM map
 *   of ew_video_metrics unchanged: a window counts with the weight of its CENTRE row.  A zero sum of the centre rows' weights gives
 *   a non-finite value.  Needs H, W >= 11.
 * Fixed-order partial sums, no atomics: two calls are bit-identical; with row_w == 1 both outputs are ew_video_metrics' values.
 * workspace: ew_video_metrics_ws_workspace_bytes(F, C, H, W) bytes (8-byte aligned).  Refused: what ew_video_metrics refuses, and a
 * NULL row_w. */
size_t ew_video_metrics_ws_workspace_bytes(int F, int C, int H, int W);
ew_status ew_video_metrics_ws(const void* a, const void* b, int layout, int F, int C, int H, int W, int what, const double* row_w,
                              double* wsse, double* wssim, void* workspace, void* stream);

/* The 8-bit ground-truth frame of the episode-mode dumps predictions_gt_{seg}/NNN.png (unified_loop_consistency.py:87-93,437-439):
 * the resized uint8 frame k -> ToTensor (k / 255) -> x*2 - 1 -> (x*0.5 + 0.5).clamp(0, 1).mul(255).byte(), every step a float32
 * rounding and the last a truncation, i.e. a fixed 256-entry map (63 levels come out one lower).  src, dst uint8 [n]. */
ew_status ew_gt_dump_map_u8(const uint8_t* src, uint8_t* dst, size_t n, void* stream);

/* Equirectangular panoramas -> the reference's cube cross (ABI 13; Navigator.convert_panorama_to_cubemap,
 * evoworld/inference/navigator_evoworld.py:514-705, which does this in numpy on the host): pano uint8 [V,H,W,3] with W == 2 H and
 * W % 4 == 0 -> cross uint8 [V,3E,W,3], E = W / 4.  Middle row of cells: back, left, front, right; top is cell 2 of the first row, bottom
 * cell 2 of the third, the other six cells are written black (:551-553, :648-659); the six faces are crops of the cross (:672-693).
 * Source coordinates are evaluated on the device in float64 in the reference's order (pixel_to_xyz :555-593, uf / vf :597-603).
 * interpolation = 1: floor and +1 neighbours, all four clipped (no wrap at the seam), float64 four-term blend, truncated to uint8 (:605-634);
 * interpolation = 0: round half to even, pixels whose index falls outside the panorama (uf == W on the seam) stay black (:638-646).
 * cross 4-byte aligned; one launch for all V panoramas. */
ew_status ew_equi2cube_u8(const uint8_t* pano, uint8_t* cross, int V, int H, int W, int interpolation, void* stream);

/* The layer kernels the metric networks share (csrc/convnet.hip; ABI 20 gave them one home: LPIPS/AlexNet, FVD's I3D and the latent MSE's
 * Inception-v4 below).  Every convolution of the three runs on ew_gemm_f16 (dense mode, bias vector) over the patch rows of
 * ew_im2col3d_f16; a 2-D network passes kt = 1 with its image batch on the T axis.  Conv outputs are stored PRE-ReLU and the kernels apply
 * max(x, 0) where they read (ReLU commutes with max-pooling).  All tensors are fp16 [T,H,W,C] (channels innermost, C % 8 == 0), 16-byte
 * aligned; no atomics, fixed summation orders: two calls are bit-identical.
 *
 * ew_im2col3d_f16: (kt,kh,kw) / stride (st,sh,sw) patch gather with front pads (pt,ph,pw), 0 <= pad < kernel -> out [t_out*h_out*w_out, ldk],
 *   column ((dt*kh + dy)*kw + dx)*C + c; taps outside the input and the columns [kt*kh*kw*C, ldk) are zero (ldk % 8 == 0: pad K to the
 *   multiple of 64 ew_gemm_f16 wants).  The caller chooses the output size (TensorFlow "SAME": ceil(in / stride), front pad = total // 2,
 *   evoworld_amd.fvd.same_pad; or torch's floor((in + 2 pad - k) / stride) + 1); every window must overlap the input.  relu = 1 reads max(x, 0).
 * ew_maxpool3d_relu_f16: max over the window's taps inside the input of max(x, 0), same geometry arguments -> out [t_out,h_out,w_out,C].
 *   Equals a zero-padded max pool of post-ReLU input (the reference's MaxPool3dSamePadding): every value is >= 0.
 * ew_avgpool3x3_relu_f16: AvgPool2d(3, stride=1, padding=1, count_include_pad=False) of max(x, 0), fp16 [n_img,H,W,C] -> the same shape,
 *   C % 8 == 0: the taps inside the image added in fp32 in (dy, dx) order, divided by their number (4, 6 or 9 when H, W >= 3).
 * ew_global_avgpool_relu_f32: fp16 [n_img,h,w,C] -> fp32 [n_img,C], the mean over h * w of max(x, 0): per (image, channel) one fp32 sum
 *   in row-major pixel order, divided by h * w.  C % 8 == 0, pointers 16-byte aligned. */
ew_status ew_im2col3d_f16(const void* src, void* out, int t_in, int h_in, int w_in, int C, int kt, int kh, int kw, int st, int sh, int sw,
                          int pt, int ph, int pw, int t_out, int h_out, int w_out, int ldk, int relu, void* stream);
ew_status ew_maxpool3d_relu_f16(const void* src, void* out, int t_in, int h_in, int w_in, int C, int kt, int kh, int kw, int st, int sh, int sw,
                                int pt, int ph, int pw, int t_out, int h_out, int w_out, void* stream);
ew_status ew_avgpool3x3_relu_f16(const void* src, void* out, int n_img, int H, int W, int C, void* stream);
ew_status ew_global_avgpool_relu_f32(const void* src, float* out, int n_img, int h, int w, int C, void* stream);

/* LPIPS with the AlexNet backbone (ABI 14; evoworld/metrics/other_metrics/calculate_lpips.py, calculate_all_metrics.py:195-221:
 * lpips.LPIPS(net='alex', spatial=True).forward(img1, img2).mean() per frame pair).  The first convolution's patch rows come from
 * ew_im2col_frames_f16, the other four's from ew_im2col3d_f16 and the two max pools from ew_maxpool3d_relu_f16 (csrc/convnet.hip, kt = 1,
 * the image batch on T); the two kernels below are in csrc/lpips.hip.  Weights come from the caller: the project ships none.
 *
 * ew_im2col_frames_f16 (ABI 20): the first layer's k x k / stride / zero-pad patch gather from a
 *   batch of frames -> out fp16 [n_img*h_out*w_out, ldk], column (ky*k + kx)*3 + c, columns [k*k*3, ldk) zero (ldk % 8 == 0: pad K to the
 *   multiple of 64 ew_gemm_f16 wants).  h_out = floor((h_in + 2 pad - k) / stride) + 1.  src_kind 1: src uint8 [n_img,h_in,w_in,3] (a pixel
 *   is float32(k) / 255.0f); 2: fp32 [n_img,3,h_in,w_in]; frames in [0,1]: network channel c reads frame channel (swap_rb ? 2 - c : c),
 *   v -> 2v - 1 -> (x - shift[c]) / scale[c] (the [-1,1] map of calculate_lpips.py and lpips' ScalingLayer), each step one float32
 *   rounding, then fp16.  first_affine: HOST pointer to {shift[3], scale[3]} (read during the call).
 * ew_lpips_head, one tap of F frame pairs: fa, fb fp16 [F, h, w, C] pre-ReLU (C % 8 == 0, <= 512); per pixel
 *   d = sum_c lin[c] * (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 with |.| over channels, in fp32; then
 *   acc[f] += sum_yx d[y,x] * wy[y] * wx[x] / n_out in fp64 (acc fp64 [F], read and written: zero it before the first tap).
 *   wy [h], wx [w] (fp64, device): how often bilinear upsampling (align_corners=False) to the frame size counts each row / column, so that
 *   with n_out = H * W this is the mean of the upsampled map without materialising it (evoworld_amd.lpips.upsample_mean_weights).
 *   lin fp32 [C].  Two fixed-order reduction stages through `workspace` (ew_lpips_head_workspace_bytes(F, h, w, C) bytes, 8-byte aligned;
 *   the block count depends on (h, w, C) only), no atomics: two calls are bit-identical, f's value does not depend on F, swapping fa and
 *   fb gives the same bits, identical inputs give exactly 0. */
enum { EW_IM2COL_U8_HWC = 1, EW_IM2COL_F32_CHW = 2 };
ew_status ew_im2col_frames_f16(const void* src, int src_kind, void* out, int n_img, int h_in, int w_in, int k, int stride, int pad, int h_out,
                               int w_out, int ldk, int swap_rb, const float* first_affine, void* stream);
size_t ew_lpips_head_workspace_bytes(int F, int h, int w, int C);
ew_status ew_lpips_head(const void* fa, const void* fb, const float* lin, const double* wy, const double* wx, int F, int h, int w, int C,
                        double n_out, double* acc, void* workspace, void* stream);

/* FVD's I3D network (ABI 16; evoworld/metrics/fvd/styleganv/fvd.py preprocess_single and evoworld/metrics/fvd/videogpt/pytorch_i3d.py
 * InceptionI3d(400): Inception-v1 inflated to 3-D, one clip per call).  The 57 BatchNorm-folded convolutions run on ew_gemm_f16 (dense
 * mode, bias vector, ld_out = the module's concat width) over the patch rows of ew_im2col3d_f16, the max pools on ew_maxpool3d_relu_f16
 * (csrc/convnet.hip); the two kernels below are in csrc/i3d.hip.  Weights come from the caller: the project ships none.
 *
 * ew_video_preprocess_f16: preprocess_single of one clip.  src_kind 1: uint8 [T,H,W,3] (a pixel is float32(k) / 255.0f); 2: fp32 [T,3,H,W] in
 *   [0,1] -> out [T,224,224,8], channels 3..7 zero.  Bilinear resize (align_corners=False, no antialias) to h_resized x w_resized with torch's
 *   float32 index arithmetic (scale = in / out, src = max(0, scale * (i + 0.5) - 0.5), i0 = floor(src), i1 = min(i0 + 1, in - 1)), rounded as
 *   torch's CPU kernel rounds (fma(scale, i + 0.5, -0.5); each blend t0 * w0 + t1 * w1 as fma(t0, w0, t1 * w1)), the 224 x 224
 *   crop at (y0, x0) of the resized frame, then (x - 0.5) * 2.  Network channel c reads frame channel (swap_rb ? 2 - c : c).  The caller
 *   computes h_resized, w_resized, y0, x0 (evoworld_amd.fvd.preprocess_geometry); only the cropped pixels are evaluated.
 * ew_i3d_head: x = the pre-ReLU Mixed_5c output [t_in >= 2, 7, 7, 1024] (any other shape is refused) -> logits fp32 [400] =
 *   mean over time of logits(AvgPool3d((2,7,7), 1)(relu(x))) = W v + b with v[c] = sum_j cnt_j sum_yx max(x[j,y,x,c], 0) / (98 (t_in - 1)),
 *   cnt_j = the number of windows frame j lies in.  w fp32 [400,1024], b fp32 [400]; fp32 throughout; workspace: ew_i3d_head_workspace_bytes()
 *   bytes, 16-byte aligned. */
ew_status ew_video_preprocess_f16(const void* src, int src_kind, void* out, int T, int H, int W, int h_resized, int w_resized, int y0, int x0,
                                  int swap_rb, void* stream);
size_t ew_i3d_head_workspace_bytes(void);
ew_status ew_i3d_head(const void* x, int t_in, int h_in, int w_in, int C, const float* w, const float* b, float* logits, void* workspace,
                      void* stream);

/* The latent MSE's Inception-v4 network (ABI 17; evoworld/metrics/other_metrics/calculate_latent_mse.py:11-79, run by
 * evoworld/metrics/calculate_all_metrics.py:220-221: timm's `inception_v4` with the classifier removed, 1536 pooled features per frame,
 * behind torchvision's Resize((299, 299)) + Normalize(ImageNet mean, std)).  The 149 BatchNorm-folded convolutions run on ew_gemm_f16
 * (dense mode, bias vector, ld_out = the module's concat width) over the patch rows of ew_im2col3d_f16 with kt = 1, the pools on
 * ew_maxpool3d_relu_f16, ew_avgpool3x3_relu_f16 and ew_global_avgpool_relu_f32 (csrc/convnet.hip); the kernel below is in
 * csrc/inception.hip.  Weights come from the caller: the project ships none.
 *
 * ew_frames_resize_aa_norm_f16: the first layer's input.  src_kind 1: uint8 [F,H,W,3] (a pixel is float32(k) / 255.0f); 2: fp32 [F,3,H,W] in
 *   [0,1] -> out fp16 [F,out_h,out_w,8], channels 3..7 zero.  The resize is F.interpolate(mode="bilinear", align_corners=False,
 *   antialias=True), what Resize does to a float tensor: a separable triangle filter, the W pass then the H pass, each a float32 chain
 *   t = fma(src[j], w[j], t) in tap order (what torch's x86 builds compile their loop to).  Per axis and output index i the DEVICE
 *   tables give the first source index (int [n_out]), the tap count (int [n_out]) and the weights (float [n_out, taps], rows padded), as evoworld_amd.latent_mse.resize_table computes them on the host; also an upscale
 *   goes through the table (with antialias it is not plain bilinear).  Indices are clamped to the frame and counts to `taps`.  Then
 *   (x - mean[c]) / std[c] in float32, then fp16.  Network channel c reads frame channel (swap_rb ? 2 - c : c); mean and std are indexed
 *   by the network channel.  mean_std: HOST pointer to {mean[3], std[3]} (read during the call), std > 0. */
ew_status ew_frames_resize_aa_norm_f16(const void* src, int src_kind, void* out, int F, int H, int W, int out_h, int out_w, const int* y_first,
                                       const int* y_count, const float* y_weights, int y_taps, const int* x_first, const int* x_count,
                                       const float* x_weights, int x_taps, int swap_rb, const float* mean_std, void* stream);

#ifdef __cplusplus
}
#endif
#endif
