// gemm_gen23.h -- what generations 2 and 3 (gemm2_f16.hip, gemm3_f16.hip) share: wait / fence / barrier primitives, the tap walk of the
// implicit-GEMM loaders and the table of compiled (MODE, EPI) variants.  (The A-row geometry, the epilogue operand preamble and the
// residual add are still one copy per family: moved into shared helpers they changed the shipped ISA -- see DESIGN.md section 3.)
// Generation 1 (gemm_f16.hip) is the suite's independent cross-check and deliberately does NOT include this file.
#pragma once
#include "gemm_common.h"
#include <type_traits>

// ---------------- wait / fence / barrier ----------------
// gfx9 s_waitcnt simm16: vmcnt[3:0]=bits3:0, expcnt=bits6:4, lgkmcnt=bits11:8, vmcnt[5:4]=bits15:14.  The BUILTIN form is
// used for lgkmcnt so that hipcc's own waitcnt model knows the LDS queue is empty (an inline-asm wait is opaque to it).
__device__ __forceinline__ void ew_wait_lgkm0() { __builtin_amdgcn_s_waitcnt(0xC07F); }
// vmcnt keeps the inline-asm form: the counts are the kernels' own (instructions issued since the DMA / stores waited for)
template <int N>
__device__ __forceinline__ void ew_wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void ew_fence() { asm volatile("" ::: "memory"); }                  // compiler-only
__device__ __forceinline__ void ew_block_barrier() { ew_fence(); __builtin_amdgcn_s_barrier(); ew_fence(); }
__device__ __forceinline__ void ew_pin() { __builtin_amdgcn_sched_barrier(0); }                // nothing is scheduled across

// ---------------- K walk of the A loaders: channel-chunk major, tap minor (dense / conv3x3 / temporal 3-tap) ----------------
template <int MODE>
constexpr int ew_a_ntap = MODE == EW_A_CONV3X3 ? 9 : (MODE == EW_A_CONVT3 ? 3 : 1);

// wave-uniform pixel delta of tap `tap` against the centre tap
template <int MODE>
__device__ __forceinline__ int ew_a_tap_delta(const GemmP& p, int tap) {
    if constexpr (MODE == EW_A_CONV3X3) return (tap / 3 - 1) * p.w_in + (tap % 3 - 1);
    else if constexpr (MODE == EW_A_CONVT3) return (tap - 1) * p.tP;
    else return 0;
}

// ---------------- compiled variants ----------------
// THE list of (MODE, EPI) pairs generation GEN (2 or 3) compiles a kernel for; both generations' dispatchers are this function with
// their own launch functor.  EPI: bit0 row-bias, bit1 residual r1, bit2 residual r2, bit3 GEGLU, bit4 lo8 operands.
// Contract: every value ew_gemm_select_epi (gemm_dispatch.cpp: the single place that maps an operand set to an EPI) can return for
// (GEN, MODE) must be listed here for (GEN, MODE); tests/test_gpu_gemm_variants.py walks the operand sets.
template <int GEN, int MODE, class Launch>
ew_status ew_gemm_visit_variant(int epi, Launch&& launch) {
    constexpr bool D = MODE == EW_A_DENSE;
#define EW_VARIANT(E, COMPILED)                                                        \
    case (E):                                                                          \
        if constexpr (COMPILED) return launch(std::integral_constant<int, (E)>{});     \
        break;
    switch (epi) {        // (keep the order: hipcc emits the kernels in it)
        EW_VARIANT(8, D)
        EW_VARIANT(16 | 1, GEN == 3)
        EW_VARIANT(16 | 2, !D)
        EW_VARIANT(16 | 3, true)
        EW_VARIANT(16 | 7, D)
        EW_VARIANT(0, true)
        EW_VARIANT(1, true)
        EW_VARIANT(2, true)
        EW_VARIANT(3, D)
        EW_VARIANT(6, D)
        EW_VARIANT(7, true)
    }
#undef EW_VARIANT
    ew_set_error("ew_gemm_f16: generation %d has no kernel <%d, %d>", GEN, MODE, epi);
    return EW_ERR_UNSUPPORTED;
}
