// gemm_common.h -- parameter block shared by the GEMM kernel generations, and what the host front end and the kernel families call of each other.
#pragma once
#include "common.h"

struct GemmP {
    const f16* a;
    const f16* a2;
    const f16* w;
    const f16* bias;
    const f16* rowbias;
    const f16* r1;
    const f16* r2;
    f16* out;
    const f16* zero_page;
    const int8_t* r1_lo;   // split residual stream: lo8 companions, one byte per element, same element strides (may be null)
    const int8_t* r2_lo;
    int8_t* out_lo;
    int M, N, K;
    int c1, c2, lda, lda2, ld_out, ld_r1, ld_r2, ld_rowbias;
    int mode, n_img, h_in, w_in, h_out, w_out, stride, upsample;
    int tB, tT, tP;
    int conv_shift;  // conv3x3: 0 = taps centred on oy*stride (padding 1), 1 = taps start at oy*stride (padding (0,1): diffusers Downsample2D(padding=0))
    int rows_per_group, act;
    float c_acc, c_r1, c_r2;
    int tiles_m, tiles_n;
    int band;  // generation 3: tile columns per band of the tile order (0 = plain tn-fastest order)
    int dbg;   // ew_set_gemm_debug: bit 2 (value 4) = generation 3 runs the whole-tile schedule (no stream-K tail / half split)
};

// Internal A-mode of generation 3 (never in ew_gemm_args.mode: the caller passes EW_A_CONV3X3 with upsample = 2): the 3x3 conv over a nearest-x2
// upsampled image as four 2x2 phase convs over the SOURCE image.  For a fixed output parity (a, b) = (oy & 1, ox & 1) the nine taps land on 2x2
// source pixels, so the taps that share a pixel are summed once at load time (evoworld_amd.ops.pack_convup2_weight): K = 4 C instead of 9 C.
//   GEMM row m  = source pixel (img, i, j), n_img * h_in * w_in rows per phase; the M tiles are phase-major (every row of a tile shares W):
//                 tile row tm = phase * ceil(M / 256) + tile row inside the phase
//   tap (r, c)  = source pixel (i + a - 1 + r, j + b - 1 + c), zero outside the source image (== outside the upsampled image for the 3x3 taps)
//   W           = [4 phases (2a + b)][N][C/64 chunks][4 taps (2r + c)][64]
//   output row  = (img, 2i + a, 2j + b) = 2m + 2 (m / w_in) w_in + 2 a w_in + b
// The kernel's GemmP then carries M = rows per phase, K = 4 C and tiles_m = 4 * ceil(M / 256).
constexpr int EW_A_CONVUP2 = 3;

// generation 3, stream-K tail (gemm3_f16.hip), passed as a second kernel argument (GemmP is kept under 256 bytes: beyond that the
// by-value kernel argument was copied to scratch instead of being read from the kernarg segment): the last `tiles` (G <= tiles <
// 2G) output tiles are split along K over the G persistent blocks; 0 = off.  ws: uncached fp32 partial-accumulator slots, flags:
// one word per slot, epoch: the value a slot's flag takes when its partial of THIS launch is complete.
struct SkP {
    float* ws;
    unsigned* flags;
    unsigned epoch;
    int tiles, dp_rounds;
};

// ---- host front end (gemm_dispatch.cpp): ew_gemm_f16 validates, fills GemmP and asks the kernel families in routing order ----
// try: the family decides once per call whether it takes the problem (*taken) and, if so, launches it
ew_status ew_conv_small_n_try(const GemmP& p, hipStream_t s, bool* taken);   // conv_small_n.hip: 3x3 convs with N <= 16 (conv_out)
ew_status ew_gemm3_try(const GemmP& p, hipStream_t s, bool* taken);          // gemm3_f16.hip, 256x320 tile
ew_status ew_gemm3_convup2(const GemmP& p, hipStream_t s);                   // gemm3_f16.hip: conv3x3 with upsample = 2 (EW_A_CONVUP2), any tile count
ew_status ew_gemm3_try_b256(const GemmP& p, hipStream_t s, bool* taken);     // gemm3_f16.hip compiled with EW3_BN=256
ew_status ew_gemm2_dispatch(const GemmP& p, hipStream_t s);                  // gemm2_f16.hip: takes everything
ew_status ew_gemm1_dispatch(const GemmP& p, hipStream_t s);                  // gemm_f16.hip: takes everything (the suite's cross-check)
// epilogue variant of generations 2 and 3 (EPI bit0 row-bias, bit1 r1, bit2 r2, bit3 GEGLU, bit4 lo8 operands); EW_ERR_UNSUPPORTED
// with the message set for operand sets no kernel is compiled for
ew_status ew_gemm_select_epi(const GemmP& p, int generation, int* epi);
void ew_gemm_note_kernel(const char* fmt, ...);     // records the rocprof-style name of the kernel about to be launched (ew_gemm_last_kernel)
// Stream-K workspace pool of generation 3: one workspace per (tile instance, device, stream) -- launches on one stream are ordered,
// so consecutive GEMMs may share it.  inst: 0 = 256x320, 1 = 256x256; each instance reports its kernel name and slot size.
struct SkInstance { const char* kernel; size_t slot_floats; };
extern const SkInstance ew_gemm3_sk, ew_gemm3_sk_b256;
struct SkWorkspace;
// the workspace of (current device, s), created now unless s is being captured into a hipGraph (allocation and the flag memset must
// not happen there -- call ew_gemm_streamk_init(stream) before the capture to get the split inside it); nullptr if there is none
SkWorkspace* ew_sk_workspace(int inst, hipStream_t s);
void ew_sk_begin(int inst, SkWorkspace* w, int mode, int epi, const GemmP& p, SkP* sk);   // fills ws / flags / the next epoch for one launch

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __forceinline__ void glds16(const f16* src, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_wave_base, 16, 0, 0);
}

