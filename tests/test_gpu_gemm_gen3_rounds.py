"""-m gpu: the generation-3 GEMM (gemm3_kernel, 256x320 and 256x256 tiles) on MULTI-ROUND persistent schedules: more tiles than
workgroups, so that a workgroup's K-tile stream crosses output tiles -- the loader opens the next work item during the last
K-tile of the current one, init_acc folds the next tile's bias / row-bias into the accumulators, the RES_LDS epilogues stage the next
item's first K-tile, and the banded tile order and the stream-K tail decide which tile follows which.  (The cases of
test_gpu_gemm_gen3.py are sized to one tile per workgroup, and its stream-K test compares the kernel with its own whole-tile twin.)

Per case of gemm_cases.GEN3_CASES, under the default launch grid, generation and stream (G = ew_get_cu_budget(); every case asserts,
from the restated plan gemm_cases.gen3_plan, tiles > G, a workgroup with two work items and the schedule its comment claims):
  1. guards: output and lo8 plane in guarded buffers, two prefills bit-identical, nothing written outside the view; the kernel
     name is the instance's, with the <MODE, EPI> of the restated plan;
  2. fp64 reference: rel-L2 below BOUND / BOUND_SPLIT, worst row below WORST_ROW;
  3. generation 1 (independent kernels) on the same problem: same bounds against fp64, same rel-L2 bound between the two;
  4. piece identity: under ew_set_gemm_debug(4) (whole tiles only; G4's <0, 23> is compiled without the split and needs no flag) the
     whole launch, and the problem cut into pieces of 200 ... G tiles, each launched alone -- same kernel, same tile decomposition,
     same K order, but one tile per workgroup -- must agree BIT FOR BIT (hi and lo8).  Each piece is compared with its rows of
     the whole launch, so the overlapping last piece agrees with its neighbour too.  G8u / G11u cannot tile-align and rely on 1-3;
  5. stream-K tail (G5, G10, G12, G14): the default launch against the debug-4 launch -- the data-parallel tiles (ids < dp_rounds * G,
     through tile_coords) bit-identical, the tail tiles within TAIL_BOUND, and, with a split output, at least one lo8 word of the tail
     different (else the tail did not run and the restated plan is wrong); cases without a tail: the two launches bit-identical."""
import pytest
import torch

from gemm_cases import (DEV, GEN3_CASES, case_dims, gen3_case_plan, gen3_family, gen3_piece_ranges, gen3_rowbias_rows,
                        gen3_tile_ids, guarded_planes, piece_diff, problem)
from kernel_checks import _INT, Guarded, rel_l2, report

pytestmark = pytest.mark.gpu
# generation N against the reference / generation 1: the bounds of test_gpu_gemm_gen3.py and test_gpu_gemm_gen2.py
BOUND, BOUND_SPLIT = 1e-3, 2e-5
TAIL_BOUND = 2e-5                      # stream-K tail tiles against the whole-tile schedule (test_streamk_tail_matches_whole_tile_schedule)

# worst-row bounds per case: (bound, worst row of GENERATION 1 against fp64 measured on an MI355X) -- not of the code under test;
# bound = 2 x that measurement rounded down to two digits (the margin covers the different fp32 summation order of the tile
# shapes), applied to generation 3 and to generation 1
WORST_ROW = {
    "G1": (0.0005, 0.0002534),  # generation 1 vs fp64: rel-L2 0.000207, worst row 76284
    "G2": (1.9e-06, 9.628e-07),  # generation 1 vs fp64: rel-L2 8.16e-07, worst row 34405
    "G3": (0.00046, 0.0002331),  # generation 1 vs fp64: rel-L2 0.000207, worst row 12427
    "G4": (1.9e-06, 9.534e-07),  # generation 1 vs fp64: rel-L2 8.18e-07, worst row 41826
    "G5": (2e-06, 1.006e-06),  # generation 1 vs fp64: rel-L2 8.18e-07, worst row 12449
    "G6": (0.00054, 0.000274),  # generation 1 vs fp64: rel-L2 0.000207, worst row 6117
    "G7": (0.00044, 0.0002233),  # generation 1 vs fp64: rel-L2 0.000207, worst row 2342
    "G8": (0.0005, 0.000253),  # generation 1 vs fp64: rel-L2 0.000207, worst row 83681
    "G8u": (0.00051, 0.0002553),  # generation 1 vs fp64: rel-L2 0.000207, worst row 110597
    "G9": (0.0005, 0.0002523),  # generation 1 vs fp64: rel-L2 0.000207, worst row 62801
    "G10": (2e-06, 1.036e-06),  # generation 1 vs fp64: rel-L2 8.17e-07, worst row 33847
    "G11": (2.1e-06, 1.061e-06),  # generation 1 vs fp64: rel-L2 8.16e-07, worst row 107329
    "G11u": (0.00051, 0.000257),  # generation 1 vs fp64: rel-L2 0.000207, worst row 80774
    "G12": (0.00052, 0.0002612),  # generation 1 vs fp64: rel-L2 0.000207, worst row 133796
    "G13": (1.7e-06, 8.750e-07),  # generation 1 vs fp64: rel-L2 8.27e-07, worst row 3291
    "G14": (1.9e-06, 9.890e-07),  # generation 1 vs fp64: rel-L2 8.17e-07, worst row 47492
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
    L.ew_set_gemm_debug(0)


def test_worst_row_table_is_bounded_by_the_rel_l2_limits():
    assert set(WORST_ROW) == set(GEN3_CASES)
    for cid, (bound, measured) in WORST_ROW.items():
        assert 0 < bound <= (BOUND_SPLIT if GEN3_CASES[cid].get("split") else BOUND), cid
        assert bound <= 2 * measured, cid                                  # (2 x the measurement, rounded DOWN to two digits)


def _bits(t):
    return t.contiguous().view(_INT[t.dtype])


@pytest.mark.parametrize("cid", list(GEN3_CASES))
def test_multi_round(ops, lib, cid):
    from evoworld_amd.ops import Res
    c = GEN3_CASES[cid]
    G = lib.ew_get_cu_budget()
    M, N, K, geglu, _, _ = case_dims(c)
    plan = gen3_case_plan(c, G)
    n_items = [len(it) for it in plan.items]
    assert plan.taken and plan.tiles > G and max(n_items) >= 2, f"{cid}: {plan.tiles} tiles on {G} workgroups is a single round"
    assert plan.schedule == c.get("schedule", "whole"), (cid, plan.schedule, plan.dp_rounds, plan.sk_tiles)
    assert "epi" not in c or plan.kernel.endswith(c["epi"]), plan.kernel
    fam = gen3_family(N)
    ids = gen3_tile_ids(plan.tiles_m, plan.tiles_n, plan.band)
    pieces = gen3_piece_ranges(c, G)
    p = problem(ops, c, G, rpg=gen3_rowbias_rows(c, G) if c["kind"] == "dense" else None)
    split, n_out = p.split, p.n_out
    ld_pad = 8 if list(GEN3_CASES).index(cid) % 2 == 0 else 64
    ld = n_out + ld_pad
    tol = BOUND_SPLIT if split else BOUND
    dec = lambda hi, lo: Res(hi, lo).float() if split else hi.float()
    failed = []                                          # every figure is printed before the test fails

    def check(fn):
        try:
            fn()
        except AssertionError as e:
            failed.append(str(e))

    # 1. the whole launch under the default generation, guarded, two prefills (with a tail: two tail-on runs bit-identical)
    hi3, lo3, name = guarded_planes(lib, 3, plan.kernel, p.run, M, n_out, ld_pad, split)
    assert name == plan.kernel, (name, plan.kernel)
    # 3. generation 1 on the same problem, into its own guarded buffers
    hi1, lo1, _ = guarded_planes(lib, 1, "gemm_kernel", p.run, M, n_out, ld_pad, split)
    got3, got1 = dec(hi3, lo3), dec(hi1, lo1)
    # 2. fp64 reference
    ref = p.ref()
    print(f"{cid}: {name} M {M} N {N} K {K}: {plan.tiles_m} x {plan.tiles_n} = {plan.tiles} tiles on {G} workgroups, {min(n_items)}-{max(n_items)} "
          f"work items per workgroup, schedule {plan.schedule} (band {plan.band}, dp_rounds {plan.dp_rounds}, sk_tiles {plan.sk_tiles}), ld_out {ld}")
    check(lambda: report(f"{cid} generation 1", got1, ref, WORST_ROW[cid][0], tol))
    check(lambda: report(f"{cid} generation 3", got3, ref, WORST_ROW[cid][0], tol))
    e13 = rel_l2(got3, got1)
    print(f"{cid}: generation 3 vs generation 1 rel-L2 {e13:.3e}")
    if not e13 < tol:
        failed.append(f"{cid}: generation 3 vs generation 1 rel-L2 {e13:.3e}")
    del ref, got1, got3, hi1, lo1
    # 4. / 5. the whole launch again on the whole-tile schedule, then its single-round pieces
    dts = [torch.float16, torch.int8] if split else [torch.float16]
    planes_of = lambda rows: [Guarded(rows, n_out, dt, ld=ld, prefill=0, device=DEV) for dt in dts]        # NaN pattern, guarded like step 1
    launch = lambda gs, r0, r1: p.run(Res(*[g.view for g in gs]) if split else gs[0].view, ld, r0, r1)
    lib.ew_set_gemm_debug(c.get("debug", 4))
    try:
        gw = planes_of(M)
        launch(gw, 0, M)
        names = {lib.ew_gemm_last_kernel().decode()}
        whole4 = [g.view for g in gw]
        n_bad, where, n_pieces = 0, [], 0
        for r0, r1 in pieces or []:
            pl1 = gen3_case_plan(c, G, debug=c.get("debug", 4), rows=r1 - r0)
            assert pl1.taken and pl1.schedule == "whole" and max(len(it) for it in pl1.items) == 1, (cid, r0, r1)
            planes = planes_of(r1 - r0)
            launch(planes, r0, r1)
            names.add(lib.ew_gemm_last_kernel().decode())
            torch.cuda.synchronize()
            for g in planes:
                g.check()
            n, w = piece_diff([pl[r0:r1] for pl in whole4], [g.view for g in planes], N, geglu, G, family=fam,
                              tile_id=lambda tm, tn: ids[tm][tn], row0=r0)
            n_bad, n_pieces = n_bad + n, n_pieces + 1
            if n:
                where.append(w)
            del planes
    finally:
        lib.ew_set_gemm_debug(0)
    torch.cuda.synchronize()
    for g in gw:
        g.check()
    assert names == {name}, (names, name)
    if pieces is not None:
        print(f"{cid} pieces: {n_pieces} launches, {n_bad} differing words")
        if n_bad:
            failed.append(f"{cid}: {n_bad} words of the whole launch differ from its single-round pieces: {'; '.join(where)}")
    # default launch against the whole-tile launch
    diff = [_bits(a) != _bits(b) for a, b in zip([hi3] + ([lo3] if split else []), whole4)]
    if plan.schedule == "tail":
        tail = torch.tensor(ids, device=DEV) >= plan.dp_rounds * G                          # [tiles_m, tiles_n]: tile in the stream-K tail
        tail = tail.repeat_interleave(plan.BM, 0)[:M].repeat_interleave(plan.BN, 1)
        assert tail.shape == (M, n_out) and int(tail[::plan.BM, ::plan.BN].sum()) == plan.sk_tiles
        n_in = [int((d & tail).sum()) for d in diff]
        n_out_ = [int((d & ~tail).sum()) for d in diff]
        e_tail = rel_l2(dec(hi3, lo3)[tail], dec(whole4[0], whole4[1] if split else None)[tail])
        print(f"{cid} tail: {plan.sk_tiles} tail tiles; differing words inside the tail {n_in} (hi, lo8) of {int(tail.sum())}, outside {n_out_}; "
              f"tail rel-L2 vs whole-tile schedule {e_tail:.3e}")
        if sum(n_out_):
            failed.append(f"{cid}: {n_out_} words of the data-parallel tiles differ between the tail and the whole-tile schedule")
        if not e_tail < TAIL_BOUND:
            failed.append(f"{cid}: tail tiles rel-L2 {e_tail:.3e} vs the whole-tile schedule")
        # a condition on the test: identical lo8 words everywhere mean that the tail did not run
        assert not split or n_in[1] >= 1, f"{cid}: no lo8 word of the tail tiles differs from the whole-tile schedule: the tail did not run"
        assert lib.ew_gemm_streamk_status() == 0
    else:
        n_diff = sum(int(d.sum()) for d in diff)
        print(f"{cid}: default launch vs debug launch {n_diff} differing words")
        if n_diff:
            failed.append(f"{cid}: {n_diff} words differ between two launches of the same whole-tile schedule")
    ops.streamk_check()
    assert not failed, "\n".join(failed)
