"""The case table of tests/test_gpu_gemm_gen2.py really reaches multi-round schedules, and its checks catch what they are for
(CPU only: the "launches" here are Python slices)."""
import pytest
import torch

from gemm_cases import GEN2_CASES, case_dims, case_pieces, gen2_family, gen2_schedule, piece_diff, piece_ranges
from kernel_checks import worst_row


def test_every_case_chains_tiles_on_256_workgroups():
    G = 256
    for cid, c in GEN2_CASES.items():
        M, N, K, geglu, unit, _ = case_dims(c)
        BM, BN, tiles_m, tiles_n, lo, hi = gen2_schedule(M, N, geglu, G)
        assert (BM, BN) == c["family"], cid
        assert tiles_m * tiles_n == c["tiles"] > G, (cid, tiles_m, tiles_n)
        if cid in ("A7", "A7u"):
            # 5 batch elements of 100 tiles: 500 / 501 tiles < 2 * 256, so workgroups with seq0 >= 244 / 245 stop after one tile;
            # the other 95 % chain two
            assert (lo, hi) == (1, 2) and c["tiles"] - G >= 244, (cid, lo, hi)
        else:
            assert lo >= (5 if cid == "A1" else 2) and hi - lo <= 1, (cid, lo, hi)
        assert K % 64 == 0
        pieces = case_pieces(c, G)
        if pieces is None:
            assert M % 256 and cid in ("A4u", "A7u"), cid            # only the cases that cannot tile-align go without
            continue
        assert pieces[0][0] == 0 and pieces[-1][1] == M and all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])), cid
        for r0, r1 in pieces:                                        # one round each, on the whole launch's tile grid
            assert r0 % 256 == 0 and r0 % BM == 0 and r0 % unit == 0, (cid, r0)
            assert gen2_schedule(r1 - r0, N, geglu, G)[5] == 1, (cid, r0, r1)
        assert len(pieces) >= 2, cid
    # the facts the table's comments rely on
    assert gen2_schedule(GEN2_CASES["A1"]["M"], 480, False, G)[4:] == (5, 6)
    assert gen2_family(128, False)[:2] == (256, 160) and gen2_family(640, True)[:2] == (128, 256) and gen2_family(192, False)[:2] == (128, 256)


@pytest.mark.parametrize("split", [False, True])
def test_piece_identity_and_worst_row_flag_one_stale_fragment(split):
    """A "whole launch" equal to its concatenated pieces passes; one 16-row x 8-column group of a later round holding the values of
    the tile the same workgroup computed one round earlier (a stale LDS fragment) trips the piece-identity check, which names
    the tile and the round, and worst_row (far above any bound of the WORST_ROW table)."""
    G, M, N = 16, 10005, 320                                          # 40 x 2 tiles of 256 x 160 on 16 workgroups: 5 rounds
    BM, BN, tiles_m, tiles_n, lo, hi = gen2_schedule(M, N, False, G)
    assert (BM, BN, tiles_m * tiles_n, lo, hi) == (256, 160, 80, 5, 5)
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(M, N, generator=g, dtype=torch.float64)
    whole_hi = (ref * (1 + 3e-4 * torch.randn(M, N, generator=g, dtype=torch.float64))).half()       # fp16-like background noise
    whole = [whole_hi] + ([torch.randint(-128, 128, (M, N), generator=g, dtype=torch.int8)] if split else [])
    ranges = piece_ranges(M, N, False, G)
    assert len(ranges) == 5 and ranges[1] == (2048, 4096)
    pieces = [torch.cat([p[r0:r1].clone() for r0, r1 in ranges]) for p in whole]
    assert piece_diff(whole, pieces, N, False, G) == (0, "")
    w0, _ = worst_row(whole_hi, ref)
    assert w0 < 1e-3
    # tile 53 = (26, 1): round 3 of the workgroup with seq0 = 5; wave tile (2, 0), fragment row 1, columns 24..31 of the wave tile
    r, c = 26 * 256 + 2 * 64 + 16, 160 + 24
    bad = [p.clone() for p in whole]
    for p in bad:
        p[r: r + 16, c: c + 8] = p[r - 8 * 256: r - 8 * 256 + 16, c: c + 8]      # tile 37 = 53 - G: the round before
    n, where = piece_diff(bad, pieces, N, False, G)
    assert n >= 100 and "tile 53 = (26, 1), round 3, wave tile (2, 0), fragment row 1" in where, (n, where)
    w, i = worst_row(bad[0], ref)
    assert r <= i < r + 16 and w > 0.1
    if split:                                                         # a difference in the lo8 plane alone is seen too
        only_lo = [whole[0], bad[1]]
        n, where = piece_diff(only_lo, pieces, N, False, G)
        assert n >= 100 and where.startswith("lo8 (")
