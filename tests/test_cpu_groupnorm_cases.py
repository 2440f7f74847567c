"""tests/groupnorm_cases.py holds on the CPU: every case of tests/test_gpu_groupnorm.py bears its bound without the kernel (fp64
statistics rounded to fp32, the fp32 apply in the kernel's evaluation order and the split output stay at or below a fifth of the
bound), the statistics cases tell a summation that pivots on row 0 from one that does not, and the tables reach the launch
geometries their comments claim."""
import numpy as np
import pytest
import torch

import groupnorm_cases as gc
from kernel_checks import worst_row

# slabs of a statistics shape that the CPU looks at (the 64-slab shape repeats its two noise slabs at 32 means)
CPU_SLABS = {"2x9216x64": [0, 1], "2x9216x320": [0, 1], "64x9216x64": [0, 63]}


@pytest.fixture(scope="module")
def noise():
    return {s: gc.stat_noise(s) for s in gc.STAT_SHAPES}


def _floor(x, gamma, beta, groups, silu):
    """worst row of the fp32 floor against fp64: fp64 statistics rounded to fp32, fp32 apply, split output"""
    ref, mean, var = gc.reference(x, gamma, beta, groups, silu=silu)
    got = gc.split_out(gc.apply_fp32(x, mean, var, gamma, beta, groups, silu=silu))
    return worst_row(got, ref)[0]


@pytest.mark.parametrize("shape", list(gc.STAT_SHAPES))
@pytest.mark.parametrize("dist", list(gc.DISTS))
def test_stat_cases_bear_their_bound(noise, shape, dist):
    n, rows, C = gc.STAT_SHAPES[shape]
    gamma, beta = gc.params(C)
    for kind in gc.KINDS:
        for split in (False, True):
            for rolled in (False, True):
                x = gc.stat_input(noise[shape], shape, dist, kind, CPU_SLABS[shape])
                x = gc.operand(x, split)[2]
                if rolled:
                    x = torch.roll(x, 1, dims=1)
                w = _floor(x, gamma, beta, 32, gc.STAT_SILU)
                print(f"floor {shape} {dist} {kind} split={split} rolled={rolled}: {w:.2e} (bound {gc.BOUND_SPLIT[dist]:.0e})")
                assert w <= gc.BOUND_SPLIT[dist] / 5, (shape, dist, kind, split, rolled, w)


@pytest.mark.parametrize("name", list(gc.ABI_CASES))
def test_abi_cases_bear_their_bound(name):
    n, rows, groups, Cs = gc.ABI_CASES[name]
    C = sum(Cs)
    gamma, beta = gc.params(C)
    x = gc.abi_input(name)
    if n > 4:
        x = x[:4]
    for split in (False, True):
        xv = gc.operand(x, split)[2]
        for silu in (False, True):
            w = _floor(xv, gamma, beta, groups, silu)
            ref = gc.reference(xv, gamma, beta, groups, silu=silu)[0]
            f = gc.apply_fp32(xv, *gc.reference(xv, gamma, beta, groups, silu=silu)[1:], gamma, beta, groups, silu=silu)
            wp = worst_row(f.half(), ref)[0]
            print(f"floor {name} split={split} silu={silu}: split out {w:.2e}, plain out {wp:.2e}")
            assert w <= gc.BOUND_SPLIT["n03"] / 5, (name, split, silu, w)
            assert wp <= 2.0 ** -11 + 1e-4 / 5, (name, split, silu, wp)      # the fp16 rounding itself can reach 2^-11


@pytest.mark.parametrize("shape", list(gc.STAT_SHAPES))
@pytest.mark.parametrize("dist", list(gc.DISTS))
def test_stat_cases_discriminate(noise, shape, dist):
    """relative error of rstd.  Pivot on row 0: more than 3x above the bound wherever row 0 alone is atypical, more than 5x below
    it on the 'all rows alike' twins.  Pivot per thread + Chan's combine: more than 3x below it on every case (the thread that
    starts on a row of 300 still cancels over its own 29 rows of the 10-chunk shape: 3e-6)."""
    n, rows, C = gc.STAT_SHAPES[shape]
    bound = gc.BOUND_SPLIT[dist]
    for kind in gc.KINDS:
        for rolled in (False, True):
            if rolled and kind not in ("alike", "last_row", "row0_zero"):
                continue
            x = gc.operand(gc.stat_input(noise[shape], shape, dist, kind, CPU_SLABS[shape][:1]), True)[2]
            if rolled:
                x = torch.roll(x, 1, dims=1)
            _, mean, var = gc.reference(x, *gc.params(C), 32)
            e0 = gc.rstd_error(gc.emulate_row0_pivot_stats(x, 32, n)[1], var.numpy())
            m1, v1 = gc.emulate_thread_pivot_stats(x, 32, n)
            e1 = gc.rstd_error(v1, var.numpy())
            em = float((np.abs(m1 - mean.numpy()) / np.sqrt(var.numpy() + gc.EPS)).max())          # error of the mean in units of std
            print(f"rstd error {shape} {dist} {kind} rolled={rolled}: row-0 pivot {e0:.2e}, thread pivots {e1:.2e}, "
                  f"their mean {em:.2e} std (bound {bound:.0e})")
            # the channel mean and the sum over the group's channels are each rounded once at the mean's size whatever the
            # summation order: up to 3 half-ulps of 75 = 4.5e-5 std in all
            assert em < bound / 2, (shape, dist, kind, rolled, em)
            if gc.row0_alone_atypical(dist, kind, rolled):
                assert e0 > 3 * bound, (shape, dist, kind, rolled, e0)
            elif kind == "alike":
                assert e0 < bound / 5, (shape, dist, kind, rolled, e0)
            assert e1 < bound / 3, (shape, dist, kind, rolled, e1)


def test_emulations_agree_with_fp64_on_small_shapes():
    """both restatements are GroupNorm statistics: on well-conditioned inputs at ragged shapes (two sources, empty chunks, two
    finalize passes) they agree with fp64 to fp32 rounding"""
    for name in ("seam 40+24 g4", "g1 C512", "rows 5 C64", "rows 129 C64", "40000 rows", "g16 C960"):
        n, rows, groups, Cs = gc.ABI_CASES[name]
        x = gc.abi_input(name)[:2]
        _, mean, var = gc.reference(x, *gc.params(sum(Cs)), groups)
        for emu in (gc.emulate_row0_pivot_stats, gc.emulate_thread_pivot_stats):
            m, v = emu(x, groups, n, Cs)
            assert np.abs(m - mean.numpy()).max() < 1e-6, (name, emu.__name__)
            assert gc.rstd_error(v, var.numpy()) < 2e-6, (name, emu.__name__)


def test_tables_reach_what_they_claim():
    assert [gc.gn_chunks(*gc.STAT_SHAPES[s][:2]) for s in gc.STAT_SHAPES] == [144, 144, 10]
    assert gc.layout(8) == (1, 256) and gc.layout(2048) == (256, 1) and gc.layout(2056) == (257, 1) and gc.layout(8192) == (1024, 1)
    assert gc.layout(8192)[1] * 2 * 8192 * 4 == 64 * 1024                 # the statistics LDS of C_src = 8192
    assert gc.layout(64)[1] == 32 and gc.layout(320)[1] == 6
    assert gc.gn_chunks(700, 70) == 1
    assert gc.gn_chunks(1, 40000) == 512 and gc.empty_chunks(1, 40000) == [507, 508, 509, 510, 511]
    assert [gc.gn_chunks(3, r) for r in (63, 64, 65, 127, 129)] == [1, 1, 2, 2, 3]
    gs = {name: sum(Cs) // groups for name, (n, rows, groups, Cs) in gc.ABI_CASES.items()}
    assert gs["g1 C512"] == 512 and gs["g2 C640"] == 320 and gs["g8 C64"] == 8 and gs["g16 C960"] == 60 and gs["g3 C72"] == 24
    assert 40 % gs["seam 40+24 g4"] and 328 % gs["seam 328+312 g32"]      # the seams fall inside a group
    r, _ = gc.atypical_rows("border", 9216)
    assert r.numel() == 2 * 128 + 2 * 70 and int(r[0]) == 0 and int(r[-1]) == 9215
    # every combination of the issue's table is there
    assert len(gc.STAT_CASES) == 3 * 2 * 7
