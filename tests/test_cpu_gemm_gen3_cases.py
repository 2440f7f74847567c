"""The case table of tests/test_gpu_gemm_gen3_rounds.py really reaches generation 3's multi-round schedules, the restated plan
(gemm_cases.gen3_plan / tile_coords) is consistent with itself, and the generalised piece_diff names the right tile (CPU only)."""
import pytest
import torch

from gemm_cases import (GEN3_CASES, case_dims, case_operands, gen3_case_plan, gen3_family, gen3_piece_ranges, gen3_plan,
                        gen3_rowbias_rows, gen3_tile_ids, piece_diff, tile_coords)

G = 256
TAIL = ("G5", "G10", "G12", "G14")
B256 = {"G12": "gemm3b_kernel<1, 0>", "G13": "gemm3b_kernel<0, 17>", "G14": "gemm3b_kernel<1, 18>"}      # the 256-wide instance


def test_every_case_has_the_schedule_its_comment_claims():
    for cid, c in GEN3_CASES.items():
        M, N, K, geglu, unit, _ = case_dims(c)
        pl = gen3_case_plan(c, G)
        assert pl.taken, cid
        assert (pl.BM, pl.BN) == ((256, 256) if cid in B256 else (256, 320)), cid
        assert pl.kernel == B256[cid] if cid in B256 else pl.kernel.startswith("gemm3_kernel<"), (cid, pl.kernel)
        assert "epi" not in c or pl.kernel.endswith(c["epi"]), (cid, pl.kernel)
        assert pl.tiles == c["tiles"] > G and pl.tiles == pl.tiles_m * pl.tiles_n, (cid, pl.tiles)
        n_items = [len(it) for it in pl.items]
        assert (min(n_items), max(n_items)) == c["per_wg"] and max(n_items) >= 2, (cid, min(n_items), max(n_items))
        assert pl.schedule == c.get("schedule", "whole") == ("tail" if cid in TAIL else "whole"), (cid, pl.schedule)
        assert (pl.band, pl.dp_rounds, pl.sk_tiles) == (c.get("band", 0), c.get("dp_rounds", 0), c.get("sk_tiles", 0)), (cid, pl.band, pl.dp_rounds, pl.sk_tiles)
        assert K % 64 == 0 and pl.nk == K // 64
        # under ew_set_gemm_debug(4) every case runs whole tiles, same instance and tile grid
        p4 = gen3_case_plan(c, G, debug=4)
        assert p4.taken and p4.schedule == "whole" and (p4.kernel, p4.tiles_m, p4.tiles_n, p4.band) == (pl.kernel, pl.tiles_m, pl.tiles_n, pl.band), cid
    # the facts the table's comments rely on
    plan = lambda cid: gen3_case_plan(GEN3_CASES[cid], G)
    assert (plan("G1").nk, plan("G3").nk, plan("G8").nk, plan("G11").nk, plan("G12").nk, plan("G13").nk, plan("G14").nk) == (1, 2, 9, 3, 18, 8, 9)
    assert (plan("G2").tiles_n, plan("G3").tiles_n, plan("G6").tiles_n, plan("G7").tiles_n) == (2, 3, 8, 6)
    assert (plan("G12").tiles_n, plan("G13").tiles_n, plan("G14").tiles_n) == (1, 13, 2)
    assert (plan("G2").epi & 6 and plan("G2").epi & 16) and plan("G4").epi == 23 and plan("G10").kernel == "gemm3_kernel<1, 19>"
    assert GEN3_CASES["G1"]["M"] % 256 and GEN3_CASES["G6"]["N"] * GEN3_CASES["G6"]["K"] * 2 <= 3 << 20
    # G7: a workgroup's consecutive tiles lie in different bands (band 0 holds ids < 4 * tiles_m)
    p7 = plan("G7")
    two = [it for it in p7.items if len(it) == 2]
    assert two and all(tile_coords(a[0], p7.tiles_m, 6, 4)[1] < 4 <= tile_coords(b[0], p7.tiles_m, 6, 4)[1] for a, b in two)
    # G13: split output without a residual; 20 x 13 tiles in three full bands and a ragged band of ONE column (ids 240 .. 259 run down
    # column 12); the last row tile is ragged; the workgroups with two items cross from band 0 into the ragged band
    p13, c13 = plan("G13"), GEN3_CASES["G13"]
    assert case_operands(c13) == {"lo"} and p13.epi == 17 and c13["M"] % 256 and c13["N"] * c13["K"] * 2 > 3 << 20
    assert (p13.tiles_m, p13.tiles_n, p13.band) == (20, 13, 4) and 13 % 4 == 1
    assert [tile_coords(i, 20, 13, 4) for i in (0, 3, 4, 79, 80, 239, 240, 259)] == [(0, 0), (0, 3), (1, 0), (19, 3), (0, 4), (19, 11), (0, 12), (19, 12)]
    two = [it for it in p13.items if len(it) == 2]
    assert len(two) == 4 and all(tile_coords(a[0], 20, 13, 4)[1] < 4 and tile_coords(b[0], 20, 13, 4)[1] == 12 for a, b in two)
    # the VAE's own launches take the same instance, variant and band: scores (whole tiles, 5-6 per workgroup) and P V (half split)
    ps = gen3_plan(9216, 9216, 512, "dense", {"lo"}, G)
    assert ps.taken and (ps.kernel, ps.schedule, ps.tiles, ps.band) == (p13.kernel, "whole", 1296, 4)
    assert sorted({len(it) for it in ps.items}) == [5, 6]
    # G14: two tile columns on the 256-wide instance, split residual staged through LDS (EPI & 6), tail
    p14 = plan("G14")
    assert p14.epi == 18 and p14.epi & 6 and p14.epi & 16 and (p14.BN, p14.tiles_n) == (256, 2)
    # G8 / G9: 500 tiles lose 2.3 % of two rounds; the issue's 150-image form of G12 (750 tiles) loses 2.3 % of three and has no tail
    assert 1 - 500 / 512 <= 0.04 < 1 - 550 / 768
    assert gen3_plan(150 * 1280, 256, 1152, "conv", set(), G).schedule == "whole"
    # every tail workgroup: stream-K items first, then exactly one whole data-parallel tile
    for cid in TAIL:
        pl = plan(cid)
        for it in pl.items:
            assert it[-1][0] < G and it[-1][1:] == (0, pl.nk) and all(i[0] >= G for i in it[:-1]) and len(it) >= 2, (cid, it)


def test_plan_routing_rules():
    """the rules by which generation 3 declines a problem, each at its edge"""
    take = lambda *a, **k: gen3_plan(*a, **k).taken
    assert take(51200, 320, 64, "dense", set(), G) and not take(51199 - 255, 320, 64, "dense", set(), G)       # 200 of 256 tiles
    assert take(25600, 320, 64, "dense", set(), 128) and not take(25600 - 256, 320, 64, "dense", set(), 128)   # ... scaled to the CU budget
    assert not take(100000, 480, 64, "dense", set(), G) and not take(319, 320 * 300, 64, "dense", set(), G)   # N % BN, M >= 320
    assert take(320, 320 * 200, 64, "dense", set(), G)
    assert gen3_family(512)[1] == 256 and gen3_family(1280)[1] == 320 and gen3_family(256)[1] == 256
    for r in ("r1", "r2"):                                                                       # the short-K rule
        assert not take(100000, 320, 1280, "dense", {r}, G) and take(100000, 320, 1344, "dense", {r}, G)
        assert take(100000, 640, 1280, "dense", {r}, G) and not take(100000, 256, 1280, "dense", {r}, G)
    assert take(100000, 320, 1280, "dense", {"rb"}, G)
    assert take(100000, 320, 64, "dense", {"silu", "rb"}, G) and not take(100000, 320, 64, "dense", {"silu", "r1"}, G)
    assert take(100000, 320, 64, "dense", {"gelu"}, G) and not take(100000, 320, 64, "dense", {"gelu", "rb"}, G)
    assert not take(128000, 320, 576, "conv", {"silu"}, G) and not take(128000, 320, 576, "conv", {"geglu"}, G)
    # tail split: shape, more than one round, not a whole number of rounds, loss > 4 %, not <0, 23>
    sched = lambda *a, **k: gen3_plan(*a, **k).schedule
    assert sched(70013, 640, 1280, "dense", set(), G) == "tail" and sched(70013, 640, 1216, "dense", set(), G) == "whole"
    assert sched(70013, 640, 1280, "dense", {"rb", "r1", "r2", "lo"}, G) == "whole"
    assert sched(46000, 960, 1280, "dense", set(), G) == "whole" and sched(46000, 960, 1280, "conv", set(), G) == "tail"
    assert sched(256 * 491, 320, 576, "conv", set(), G) == "tail" and sched(256 * 492, 320, 576, "conv", set(), G) == "whole"    # 4.1 % / 3.9 %
    assert sched(256 * 512, 320, 576, "conv", set(), G) == "whole" and sched(256 * 250, 320, 576, "conv", set(), G) == "whole"
    assert sched(70013, 640, 1280, "dense", set(), G, debug=4) == "whole"
    pl = gen3_plan(256 * 900, 320, 576, "conv", set(), G)
    assert (pl.dp_rounds, pl.sk_tiles) == (2, 388)
    # band: weight matrix above 3 MiB
    assert gen3_plan(15000, 1920, 832, "dense", set(), G).band == 4 and gen3_plan(15000, 1920, 768, "dense", set(), G).band == 0
    # half split: at most G / 2 tiles, K >= 8192
    pl = gen3_plan(7200, 1280, 10240, "dense", {"r1", "lo"}, G)
    assert pl.taken and (pl.schedule, pl.grid, pl.sk_tiles, pl.dp_rounds) == ("half", 232, 116, 0)
    assert all(len(it) == 1 and it[0][2] - it[0][1] == 80 for it in pl.items)
    assert not take(7200, 1280, 8128, "dense", set(), G) and not take(7200, 1280, 10240, "dense", set(), G, debug=4)
    # ... on the 256-wide instance: 8 tiles is the fewest (test_gpu_gemm_gen3.py's half_b256_min, also with a ragged last row tile), and
    # the VAE attention's P V at 9216 tokens
    for M in (1024, 1000):
        pl = gen3_plan(M, 512, 8192, "dense", {"r1", "lo"}, G)
        assert pl.taken and (pl.kernel, pl.schedule, pl.grid, pl.sk_tiles) == ("gemm3b_kernel<0, 19>", "half", 16, 8)
        assert all(len(it) == 1 and it[0][2] - it[0][1] == 64 for it in pl.items)
    assert not take(768, 512, 8192, "dense", {"r1", "lo"}, G) and not take(1024, 512, 8128, "dense", {"r1", "lo"}, G)
    pl = gen3_plan(9216, 512, 9216, "dense", set(), G)
    assert pl.taken and (pl.kernel, pl.schedule, pl.grid, pl.sk_tiles) == ("gemm3b_kernel<0, 0>", "half", 144, 72)
    assert all(len(it) == 1 and it[0][2] - it[0][1] == 72 for it in pl.items)
    assert not take(512, 9216, 512, "dense", set(), G)                   # V^T = W_v X^T: generation 2


def _check_schedule(pl):
    """every K-tile of every tile is computed exactly once; the sequence follows seq0"""
    Gk, nk = pl.grid, pl.nk
    assert len(pl.items) == Gk
    cover = {}
    for b, items in enumerate(pl.items):
        seq0 = (b & 7) * (Gk >> 3) + (b >> 3)
        for j, (tid, k0, k1) in enumerate(items):
            assert 0 <= k0 < k1 <= nk, (b, tid, k0, k1)
            cover.setdefault(tid, []).append((k0, k1))
            if tid < pl.dp_rounds * Gk or not pl.sk_tiles:
                assert tid % Gk == seq0 and (k0, k1) == (0, nk), (b, tid)
        sk = [it for it in items if pl.sk_tiles and it[0] >= pl.dp_rounds * Gk]
        assert items[:len(sk)] == sk                                      # stream-K items first
        assert all(a[0] + 1 == c[0] and a[2] == nk and c[1] == 0 for a, c in zip(sk, sk[1:]))     # one contiguous unit range
        if pl.sk_tiles:
            U = pl.sk_tiles * nk
            u0 = (sk[0][0] - pl.dp_rounds * Gk) * nk + sk[0][1]
            u1 = (sk[-1][0] - pl.dp_rounds * Gk) * nk + sk[-1][2]
            assert (u0, u1) == (seq0 * U // Gk, (seq0 + 1) * U // Gk), (b, u0, u1)
    assert sorted(cover) == list(range(pl.tiles))
    for tid, ranges in cover.items():
        ranges.sort()
        assert ranges[0][0] == 0 and ranges[-1][1] == nk and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), (tid, ranges)
        if tid < pl.dp_rounds * Gk or not pl.sk_tiles:
            assert len(ranges) == 1, (tid, ranges)
    if pl.sk_tiles:
        assert sorted(t for t in cover if len(cover[t]) == 1 and t < pl.dp_rounds * Gk) == list(range(pl.dp_rounds * Gk))
        assert pl.tiles - pl.dp_rounds * Gk == pl.sk_tiles


def test_schedules_cover_every_tile_once():
    for cid, c in GEN3_CASES.items():
        _check_schedule(gen3_case_plan(c, G))
        _check_schedule(gen3_case_plan(c, G, debug=4))
    for args in [(256 * 900, 320, 576, "conv", set(), G), (7200, 1280, 10240, "dense", set(), G), (256 * 700, 640, 1280, "dense", set(), 64),
                 (256 * 230, 320, 64, "dense", set(), G), (256 * 61, 1280, 64, "dense", set(), 64),
                 (9216, 9216, 512, "dense", {"lo"}, G), (9216, 512, 9216, "dense", set(), G), (1000, 512, 8192, "dense", {"r1", "lo"}, G)]:
        pl = gen3_plan(*args)
        assert pl.taken, args
        _check_schedule(pl)
    assert gen3_plan(256 * 230, 320, 64, "dense", set(), G).grid == 232          # fewer tiles than workgroups shrink the grid


@pytest.mark.parametrize("tiles_m,tiles_n,band", [(59, 6, 4), (59, 6, 0), (7, 8, 4), (7, 9, 4), (5, 4, 4), (3, 3, 4), (11, 13, 4), (1, 7, 4), (6, 5, 2)])
def test_tile_coords_is_a_bijection(tiles_m, tiles_n, band):
    seen = [tile_coords(i, tiles_m, tiles_n, band) for i in range(tiles_m * tiles_n)]
    assert sorted(seen) == [(tm, tn) for tm in range(tiles_m) for tn in range(tiles_n)]
    ids = gen3_tile_ids(tiles_m, tiles_n, band)
    assert all(ids[tm][tn] == i for i, (tm, tn) in enumerate(seen))
    if band and tiles_n > band:
        # ids run through whole bands: band k holds the columns [k * band, (k + 1) * band), tn fastest inside it
        for i, (tm, tn) in enumerate(seen):
            k = min(i // (band * tiles_m), -(-tiles_n // band) - 1)
            assert k * band <= tn < min((k + 1) * band, tiles_n), (i, tm, tn)
        assert seen[:band] == [(0, t) for t in range(band)] and seen[band] == (1 if tiles_m > 1 else 0, 0 if tiles_m > 1 else band)
    else:
        assert seen == [divmod(i, tiles_n) for i in range(tiles_m * tiles_n)]


def test_pieces_run_one_round_on_the_same_tile_grid():
    for cid, c in GEN3_CASES.items():
        M, N, K, geglu, unit, _ = case_dims(c)
        whole = gen3_case_plan(c, G)
        pieces = gen3_piece_ranges(c, G)
        if pieces is None:
            assert M % 256 and cid in ("G8u", "G11u"), cid                 # only the cases that cannot tile-align go without
            continue
        assert len(pieces) >= 2 and pieces[0][0] == 0 and pieces[-1][1] == M, (cid, pieces)
        assert all(a[1] >= b[0] and a[0] < b[0] for a, b in zip(pieces, pieces[1:])), (cid, pieces)           # they cover [0, M)
        rpg = gen3_rowbias_rows(c, G) if c["kind"] == "dense" else c.get("rb_imgs", 1) * unit
        if c["kind"] == "dense" and c.get("rb"):
            assert 256 % rpg and rpg % 256, (cid, rpg)                     # groups change inside tiles
        for r0, r1 in pieces:
            assert r0 % 256 == 0 and r0 % unit == 0 and r0 % rpg == 0, (cid, r0)
            assert r1 == M or r1 % unit == 0, (cid, r1)
            for dbg in (0, 4):
                pl = gen3_case_plan(c, G, debug=dbg, rows=r1 - r0)
                assert pl.taken and (pl.kernel, pl.tiles_n) == (whole.kernel, whole.tiles_n), (cid, r0, r1)
                assert 200 <= pl.tiles <= G and pl.schedule == "whole" and max(len(it) for it in pl.items) == 1, (cid, r0, r1, pl.tiles)


@pytest.mark.parametrize("split", [False, True])
def test_piece_diff_names_tile_and_round_of_generation_3(split):
    """A whole launch equal to its pieces passes; one stale 16-row fragment of a second-round tile (the values of the tile the same
    workgroup computed one round earlier), and one lo8 byte, are reported with generation 3's tile id (banded order), round and
    wave tile."""
    Gs, M, N = 16, 2500, 1920                                         # 10 x 6 tiles of 256 x 320 on 16 workgroups, bands of 4: 4 rounds
    fam = gen3_family(N)
    pl = gen3_plan(M, N, 1024, "dense", set(), Gs)
    assert pl.taken and (pl.tiles_m, pl.tiles_n, pl.band) == (10, 6, 4) and max(len(it) for it in pl.items) == 4
    ids = gen3_tile_ids(pl.tiles_m, pl.tiles_n, pl.band)
    tid_of = lambda tm, tn: ids[tm][tn]
    g = torch.Generator().manual_seed(0)
    whole = [torch.randn(M, N, generator=g).half()] + ([torch.randint(-128, 128, (M, N), generator=g, dtype=torch.int8)] if split else [])
    pieces = [p.clone() for p in whole]
    assert piece_diff(whole, pieces, N, False, Gs, family=fam, tile_id=tid_of) == (0, "")
    # tile (5, 5) lies in the ragged band: id 4 * 10 + 5 * 2 + 1 = 51, round 3 of the workgroup with seq0 = 3; its predecessor there is tile 35
    assert ids[5][5] == 51 and tile_coords(35, 10, 6, 4) == (8, 3)
    b = [b for b, it in enumerate(pl.items) if (51, 0, pl.nk) in it][0]
    assert [i[0] for i in pl.items[b]] == [3, 19, 35, 51]
    r, c = 5 * 256 + 3 * 64 + 32, 5 * 320 + 160 + 24                   # wave tile (3, 1), fragment row 2
    bad = [p.clone() for p in whole]
    for p in bad:
        p[r: r + 16, c: c + 8] = p[8 * 256 + 3 * 64 + 32: 8 * 256 + 3 * 64 + 48, 3 * 320 + 184: 3 * 320 + 192]
    n, where = piece_diff(bad, pieces, N, False, Gs, family=fam, tile_id=tid_of)
    assert n >= 100 and "tile 51 = (5, 5), round 3, wave tile (3, 1), fragment row 2" in where, (n, where)
    # the same fragment seen through one piece that starts at row 1024
    n2, where2 = piece_diff([p[1024:2048] for p in bad], [p[1024:2048] for p in pieces], N, False, Gs, family=fam, tile_id=tid_of, row0=1024)
    assert n2 == n and f"({r}, {c}): tile 51 = (5, 5), round 3" in where2, where2
    if split:                                                         # one lo8 byte alone
        one = [whole[0], whole[1].clone()]
        one[1][r + 5, c + 3] ^= 1
        n, where = piece_diff(one, pieces, N, False, Gs, family=fam, tile_id=tid_of)
        assert n == 1 and where == f"lo8 ({r + 5}, {c + 3}): tile 51 = (5, 5), round 3, wave tile (3, 1), fragment row 2", where
