"""-m gpu: the generation-2 GEMM (gemm2_kernel, 256x160 and 128x256 tiles) on MULTI-ROUND persistent schedules: more tiles than
workgroups, so that a workgroup's K-tile stream crosses output tiles -- the loader changes tile mid-stream, the epilogue patch
sits in the ring slot just freed, and the counted vmcnt waits after a full tile assume the epilogue's exact store count.  (The
small generation-2 problems of test_gpu_ops.py and test_gpu_gemm_variants.py run at most one tile per workgroup; generation 3's
chained tiles get the same treatment in test_gpu_gemm_gen3_rounds.py.)

Per case of gemm_cases.GEN2_CASES, under the default launch grid (G = ew_get_cu_budget(); every case asserts tiles > G):
  1. guards: output and lo8 plane in guarded buffers, two prefills bit-identical, nothing written outside the view;
  2. fp64 reference: rel-L2 below BOUND / BOUND_SPLIT, worst row below WORST_ROW;
  3. generation 1 (independent kernels) on the same problem: same bounds against fp64, same rel-L2 bound between the two;
  4. piece identity: the problem cut into tile-aligned pieces of at most one tile per workgroup, each launched alone under
     generation 2 -- same kernel, same tile decomposition, same K order, but no chained tiles -- must reproduce the rows of the whole
     launch BIT FOR BIT (hi and lo8).  A4u / A7u cannot tile-align and rely on 1-3."""
import pytest
import torch

from gemm_cases import DEV, GEN2_CASES, case_dims, case_pieces, gen2_schedule, guarded_planes, piece_diff, problem
from kernel_checks import fill_pattern, rel_l2, report

pytestmark = pytest.mark.gpu
# generation N against the reference / generation 1: the bounds of test_gpu_gemm_gen3.py and test_gpu_gemm_variants.py
BOUND, BOUND_SPLIT = 1e-3, 2e-5

# worst-row bounds per case: (bound, worst row of GENERATION 1 against fp64 measured on an MI355X) -- not of the code under test;
# bound = 2 x that measurement rounded down to two digits (the margin covers the different fp32 summation order of the tile
# shapes), applied to generation 2 and to generation 1
WORST_ROW = {
    "A1": (0.00049, 0.0002457),  # generation 1 vs fp64: rel-L2 0.000207, worst row 15305
    "A2s": (2e-06, 1.047e-06),  # generation 1 vs fp64: rel-L2 8.16e-07, worst row 53377
    "A2h": (0.0005, 0.000253),  # generation 1 vs fp64: rel-L2 0.000207, worst row 22617
    "A3": (0.00055, 0.0002756),  # generation 1 vs fp64: rel-L2 0.000207, worst row 96834
    "A4": (2.4e-06, 1.231e-06),  # generation 1 vs fp64: rel-L2 8.17e-07, worst row 42253
    "A4u": (0.00057, 0.0002888),  # generation 1 vs fp64: rel-L2 0.000207, worst row 121278
    "A5": (0.00056, 0.0002837),  # generation 1 vs fp64: rel-L2 0.000207, worst row 448
    "A6": (0.00054, 0.0002732),  # generation 1 vs fp64: rel-L2 0.000207, worst row 127961
    "A7": (2.5e-06, 1.268e-06),  # generation 1 vs fp64: rel-L2 8.16e-07, worst row 33420
    "A7u": (0.00056, 0.0002801),  # generation 1 vs fp64: rel-L2 0.000207, worst row 91755
    "B8": (0.00048, 0.0002438),  # generation 1 vs fp64: rel-L2 0.000207, worst row 2198
    "B8c": (0.00048, 0.0002418),  # generation 1 vs fp64: rel-L2 0.000207, worst row 25922
    "B9": (0.00069, 0.000346),  # generation 1 vs fp64: rel-L2 0.000208, worst row 24399
    "B10": (0.00052, 0.0002647),  # generation 1 vs fp64: rel-L2 0.000207, worst row 56374
    "B11": (2.3e-06, 1.179e-06),  # generation 1 vs fp64: rel-L2 8.15e-07, worst row 304
}


@pytest.fixture(scope="module")
def ops():
    from evoworld_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from evoworld_amd import _lib
    L = _lib.load()
    yield L
    L.ew_set_gemm_generation(3)


def test_worst_row_table_is_bounded_by_the_rel_l2_limits():
    assert set(WORST_ROW) == set(GEN2_CASES)
    for cid, (bound, measured) in WORST_ROW.items():
        assert 0 < bound <= (BOUND_SPLIT if GEN2_CASES[cid].get("split") else BOUND), cid
        assert bound <= 2 * measured, cid                                  # (2 x the measurement, rounded DOWN to two digits)


@pytest.mark.parametrize("cid", list(GEN2_CASES))
def test_multi_round(ops, lib, cid):
    from evoworld_amd.ops import Res
    c = GEN2_CASES[cid]
    G = lib.ew_get_cu_budget()
    M, N, K, geglu, _, _ = case_dims(c)
    BM, BN, tiles_m, tiles_n, lo_t, hi_t = gen2_schedule(M, N, geglu, G)
    assert tiles_m * tiles_n > G and hi_t >= 2, f"{cid}: {tiles_m * tiles_n} tiles on {G} workgroups is a single round"
    p = problem(ops, c, G)
    split, n_out = p.split, p.n_out
    ld_pad = 8 if list(GEN2_CASES).index(cid) % 2 == 0 else 64
    tol = BOUND_SPLIT if split else BOUND
    want = f"gemm2_kernel<{BM}, {BN},"
    dec = lambda hi, lo: Res(hi, lo).float() if split else hi.float()
    failed = []                                          # every figure is printed before the test fails

    def check(fn):
        try:
            fn()
        except AssertionError as e:
            failed.append(str(e))

    # 1. the whole launch (default generation where the case pins the router, else generation 2), guarded, two prefills
    hi2, lo2, name = guarded_planes(lib, c.get("gen", 2), want, p.run, M, n_out, ld_pad, split)
    assert "epi" not in c or name.endswith(c["epi"]), name
    # 3. generation 1 on the same problem, into its own guarded buffers
    hi1, lo1, _ = guarded_planes(lib, 1, "gemm_kernel", p.run, M, n_out, ld_pad, split)
    got2, got1 = dec(hi2, lo2), dec(hi1, lo1)
    # 2. fp64 reference
    ref = p.ref()
    print(f"{cid}: {name} M {M} N {N} K {K}: {tiles_m} x {tiles_n} tiles on {G} workgroups, {lo_t}-{hi_t} per workgroup, ld_out {n_out + ld_pad}")
    check(lambda: report(f"{cid} generation 1", got1, ref, WORST_ROW[cid][0], tol))
    check(lambda: report(f"{cid} generation 2", got2, ref, WORST_ROW[cid][0], tol))
    e12 = rel_l2(got2, got1)
    print(f"{cid}: generation 2 vs generation 1 rel-L2 {e12:.3e}")
    if not e12 < tol:
        failed.append(f"{cid}: generation 2 vs generation 1 rel-L2 {e12:.3e}")
    del ref, got1, got2, hi1, lo1
    # 4. piece identity
    pieces = case_pieces(c, G)
    if pieces is not None:
        ld = n_out + ld_pad
        planes = [fill_pattern(torch.empty(M, ld, dtype=dt, device=DEV), 0) for dt in ([torch.float16, torch.int8] if split else [torch.float16])]
        names = set()
        lib.ew_set_gemm_generation(2)
        try:
            for r0, r1 in pieces:
                assert gen2_schedule(r1 - r0, N, geglu, G)[5] == 1
                v = [pl[r0:r1, :n_out] for pl in planes]
                p.run(Res(*v) if split else v[0], ld, r0, r1)
                names.add(lib.ew_gemm_last_kernel().decode())
        finally:
            lib.ew_set_gemm_generation(3)
        torch.cuda.synchronize()
        assert names == {name}, (names, name)
        n_bad, where = piece_diff([hi2] + ([lo2] if split else []), [pl[:, :n_out] for pl in planes], N, geglu, G)
        print(f"{cid} pieces: {len(pieces)} launches, {n_bad} differing words")
        if n_bad:
            failed.append(f"{cid}: {n_bad} words of the whole launch differ from its single-round pieces: {where}")
    ops.streamk_check()
    assert not failed, "\n".join(failed)
