// gemm_gen23.h -- what generations 2 and 3 (gemm2_f16.hip, gemm3_f16.hip) share: the tap walk of the implicit-GEMM loaders and the table
// of compiled (MODE, EPI) variants; the wait / fence / barrier primitives they use are common.h's.  (The A-row geometry, the epilogue operand preamble and the
// residual add are still one copy per family: moved into shared helpers they changed the shipped ISA -- see DESIGN.md section 3.)
// Generation 1 (gemm_f16.hip) is the suite's independent cross-check and deliberately does NOT include this file.
#pragma once
#include "gemm_common.h"
#include <type_traits>

// ---------------- K walk of the A loaders: channel-chunk major, tap minor (dense / conv3x3 / temporal 3-tap) ----------------
template <int MODE>
constexpr int ew_a_ntap = MODE == EW_A_CONV3X3 ? 9 : (MODE == EW_A_CONVUP2 ? 4 : (MODE == EW_A_CONVT3 ? 3 : 1));

// wave-uniform pixel delta of tap `tap` against the centre tap (EW_A_CONVUP2: against tap (0, 0) of the tile's phase, whose own delta the loader adds)
template <int MODE>
__device__ __forceinline__ int ew_a_tap_delta(const GemmP& p, int tap) {
    if constexpr (MODE == EW_A_CONV3X3) return (tap / 3 - 1) * p.w_in + (tap % 3 - 1);
    else if constexpr (MODE == EW_A_CONVUP2) return (tap >> 1) * p.w_in + (tap & 1);
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
    // the four-phase upsample conv (generation 3 only) is bias + split output and nothing else: one kernel
    if constexpr (MODE == EW_A_CONVUP2) {
        if (GEN == 3 && epi == (16 | 1)) return launch(std::integral_constant<int, (16 | 1)>{});
    } else {
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
    }
#undef EW_VARIANT
    ew_set_error("ew_gemm_f16: generation %d has no kernel <%d, %d>", GEN, MODE, epi);
    return EW_ERR_UNSUPPORTED;
}
