"""-m gpu: the compiled-variant table of GEMM generations 2 and 3 (csrc/gemm_gen23.h, ew_gemm_visit_variant) against
ew_gemm_select_epi (csrc/gemm_dispatch.cpp), as a whole: for every A addressing mode and every epilogue operand set -- row-bias /
r1 / r2 on or off, the lo8 companions of the split residual stream on or off, GEGLU -- ew_gemm_f16 under generation 2 and under
generation 3 either fails with EW_ERR_UNSUPPORTED and a message (the sets select_epi rejects) or launches a kernel whose EPI
covers the operands, with the output of the independent generation-1 kernels.  A value select_epi returns that a generation's
list lacks shows up here as "has no kernel <MODE, EPI>"."""
import math
import re

import pytest
import torch

from kernel_checks import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("dense", "conv3x3", "temporal")
# generation N against generation 1: the bounds test_gpu_gemm_gen3.py puts on the same comparison (fp16 outputs / split hi + lo8 outputs)
BOUND, BOUND_SPLIT = 1e-3, 2e-5


def operand_sets():
    """(rb, r1, r2, split, geglu); GEGLU takes no other operand (ew_gemm_f16 rejects the combination as an invalid argument)"""
    sets = [(rb, r1, r2, split, False) for split in (False, True) for r2 in (False, True) for r1 in (False, True) for rb in (False, True)]
    return sets + [(False, False, False, False, True)]


def rejected(mode, rb, r1, r2, split, geglu):
    """what ew_gemm_select_epi has no EPI for: GEGLU on a conv mode, conv + split residual stream + r2"""
    return mode != "dense" and (geglu or (split and r2))


def geometry(ops, gen, mode):
    """gemm() keywords, M, rows per row-bias group, taps.  Generation 2: the smallest at which the variant TABLE can still go wrong -- 300 rows = one full
    256-row tile + a ragged one, every workgroup computing at most one tile (what only shows when a workgroup chains tiles -- ring across tiles, counted
    vmcnt waits after an epilogue -- is covered by test_gpu_gemm_gen2.py).  Generation 3: 51237 rows (201 tiles per 320 columns: enough for its router,
    ragged last tile)."""
    if gen == 2:
        n, h, w, B, T, P = 2, 10, 15, 2, 5, 30
    else:
        n, h, w, B, T, P = 3, 3, 5693, 3, 3, 5693
    if mode == "dense":
        return dict(), n * h * w, h * w, 1
    if mode == "conv3x3":
        return dict(mode=ops.A_CONV3X3, conv=(n, h, w, h, w, 1, 0)), n * h * w, h * w, 9
    return dict(mode=ops.A_CONVT3, tconv=(B, T, P)), B * T * P, T * P, 3


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gen", [2, 3])
def test_every_operand_set_has_its_kernel(gen, mode):
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    kw, M, rpg, taps = geometry(ops, gen, mode)
    C, NMAX = 64, 640                                   # one 64-channel K chunk; N = 320, or 640 where 320 cannot be used (below)
    g = torch.Generator(device=DEV).manual_seed(100 * gen + MODES.index(mode))
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)
    a = rnd(M, C).half()
    w = (rnd(NMAX, taps * C) / math.sqrt(taps * C)).half()
    bias, rowbias = rnd(NMAX).half(), rnd(M // rpg + 1, NMAX).half()
    res = [ops.Res.from_float(rnd(M, NMAX)) for _ in range(2)]
    want = f"gemm{gen}_kernel<"
    gen_before = lib.ew_get_gemm_generation()
    off = []                                            # every operand set is run and reported before the test fails

    def run(generation, N, rb, r1, r2, split, geglu):
        n_out = N // 2 if geglu else N
        out = ops.Res(torch.zeros(M, n_out, dtype=torch.float16, device=DEV), torch.zeros(M, n_out, dtype=torch.int8, device=DEV) if split else None)
        r = [(x if split else x.hi) if on else None for x, on in zip(res, (r1, r2))]
        lib.ew_set_gemm_generation(generation)
        ops.gemm(a, w[:N], out if split else out.hi, M=M, N=N, c1=C, lda=C, bias=bias, rowbias=rowbias if rb else None, ld_rowbias=NMAX,
                 rows_per_group=rpg, r1=r[0], ld_r1=NMAX, r2=r[1], ld_r2=NMAX, act=ops.ACT_GEGLU if geglu else ops.ACT_NONE,
                 c_acc=0.7, c_r1=0.6, c_r2=-1.5, **kw)
        return out.float(), lib.ew_gemm_last_kernel().decode()

    try:
        lib.ew_set_gemm_debug(0)
        for rb, r1, r2, split, geglu in operand_sets():
            # N = 640: GEGLU needs N % 128 == 0, and generation 3 leaves dense N = 320 problems with a residual and a short K to generation 2
            N = 640 if geglu or (gen == 3 and mode == "dense" and (r1 or r2)) else 320
            case = f"gen{gen} {mode} {M}x{N} rb{int(rb)} r1{int(r1)} r2{int(r2)} split{int(split)} geglu{int(geglu)}"
            if rejected(mode, rb, r1, r2, split, geglu):
                with pytest.raises(_lib.EvoWorldHipError) as e:
                    run(gen, N, rb, r1, r2, split, geglu)
                status = re.search(r"failed \((-?\d+)\)", str(e.value))
                assert status and int(status.group(1)) == _lib.EW_ERR_UNSUPPORTED == -2, (case, str(e.value))
                assert lib.ew_last_error(), case
                continue
            got, name = run(gen, N, rb, r1, r2, split, geglu)
            assert name.startswith(want), (case, name)           # a routing fallback must not pass silently
            mode_k, epi = (int(v) for v in name[name.index("<") + 1: -1].split(",")[-2:])
            asked = (1 if rb else 0) | (2 if r1 else 0) | (4 if r2 else 0) | (8 if geglu else 0)
            assert mode_k == MODES.index(mode) and epi & asked == asked, (case, name)
            assert not split or epi & 16, (case, name)            # (split: out_lo is passed, and r1_lo / r2_lo with r1 / r2)
            ref, name1 = run(1, N, rb, r1, r2, split, geglu)
            assert name1.startswith("gemm_kernel"), (case, name1)
            bound = BOUND_SPLIT if split else BOUND
            try:
                report(case, got, ref, bound, bound)
            except AssertionError as err:
                d = (got - ref).abs()
                off.append(f"{err} [{int((d > 1e-4 * ref.abs().clamp_min(1e-3)).sum())} elements off by more than 1e-4 relative, max |delta| {float(d.max()):.3e}]")
    finally:
        lib.ew_set_gemm_generation(gen_before)
        lib.ew_set_gemm_debug(0)
    torch.cuda.synchronize()
    ops.streamk_check()
    assert not off, "\n".join(off)
