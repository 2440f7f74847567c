"""-m 'not gpu': the semi-global aggregation of the sweeps' cost volume on the host -- the oracle of tests/mvs_sgm_ref.py
against a brute-force statement of the recurrence, the benefit on the weakly textured noisy scene, the argument checks of the new ops and
of the two stage classes, the view-chunk arithmetic and the flags' way from the command lines to the stages."""
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvs_ref as R  # noqa: E402
import mvs_sgm_ref as G  # noqa: E402
from evoworld_amd import mvs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the recurrence
def _line(H, W, x, y, dx, dy):
    """the pixels of the path through (x, y) from the image border up to (x, y), in path order"""
    pts = [(x, y)]
    while 0 <= pts[0][0] - dx < W and 0 <= pts[0][1] - dy < H:
        pts.insert(0, (pts[0][0] - dx, pts[0][1] - dy))
    return pts


def _brute_path_cost(C, P1, P2, direction):
    """L_r as an explicit minimum over label sequences.  E_t(k) = the cheapest labelling k_0 .. k_t = k of the path's first t + 1 pixels,
    sum of C(p_i, k_i) plus V(k_{i-1}, k_i) with V = 0 | P1 (one step) | P2 (further); unrolling the recurrence's '- m' gives
    L_r(p_t, k) = E_t(k) - min_j E_{t-1}(j), and L_r(p_0, k) = C(p_0, k)."""
    H, W, D = C.shape
    dx, dy = direction
    V = lambda a, b: 0 if a == b else (P1 if abs(a - b) == 1 else P2)

    def E(pts, k):
        best = None
        for seq in itertools.product(range(D), repeat=len(pts) - 1):
            labels = seq + (k,)
            v = sum(int(C[y, x, l]) for (x, y), l in zip(pts, labels)) + sum(V(a, b) for a, b in zip(labels, labels[1:]))
            best = v if best is None else min(best, v)
        return best

    L = np.zeros((H, W, D), np.int64)
    for y in range(H):
        for x in range(W):
            pts = _line(H, W, x, y, dx, dy)
            for k in range(D):
                L[y, x, k] = E(pts, k) - (min(E(pts[:-1], j) for j in range(D)) if len(pts) > 1 else 0)
    return L


@pytest.mark.parametrize("shape", [(4, 4, 3), (1, 4, 3), (4, 1, 2), (3, 4, 1), (2, 3, 3)])
@pytest.mark.parametrize("P", [(0, 0), (1, 3), (2, 2), (0, 5)])
def test_recurrence_equals_the_minimum_over_label_sequences(shape, P):
    rng = np.random.default_rng(sum(shape) + 10 * P[0] + P[1])
    C = rng.integers(0, 9, size=shape).astype(np.uint16)
    for d in G.DIRECTIONS:
        want = _brute_path_cost(C, P[0], P[1], d)
        got = G.path_costs_ref(C[None], P[0], P[1], d)[0]
        assert np.array_equal(got, want), d
    for paths in (4, 8):
        want = sum(_brute_path_cost(C, P[0], P[1], d) for d in G.DIRECTIONS[:paths])
        assert np.array_equal(G.sgm_aggregate_ref(C[None], P[0], P[1], paths)[0], want)


def test_aggregate_fits_sixteen_bits_at_the_largest_costs_and_penalties():
    C = np.full((1, 5, 6, 7), G.COST_MAX, np.uint16)
    agg = G.sgm_aggregate_ref(C, G.COST_MAX, G.COST_MAX, 8)
    assert agg.max() <= 65520 and agg.min() >= 8 * G.COST_MAX
    rng = np.random.default_rng(0)
    C = rng.choice(np.array([0, G.COST_MAX], np.uint16), size=(2, 6, 7, 5))       # jumps everywhere: L reaches C + P2
    for d in G.DIRECTIONS:
        L = G.path_costs_ref(C, G.COST_MAX, G.COST_MAX, d)
        assert L.max() <= G.COST_MAX + G.COST_MAX and (L >= C).all()
    assert G.sgm_aggregate_ref(C, G.COST_MAX, G.COST_MAX, 8).max() <= 65520


def test_identities_without_penalties_and_with_one_hypothesis():
    """P1 = P2 = 0: the bracket min(L(q, k), L(q, k -+ 1), m) is m itself, so L_r = C + m - m = C on every path and agg = paths x C at
    EVERY cell.  With P2 > 0 that holds only at D = 1 (the one hypothesis is the minimum) and at pixels without a predecessor on any
    of the paths; in general C <= L_r <= C + P2, so paths x C <= agg <= paths x (C + P2)."""
    rng = np.random.default_rng(1)
    C = rng.integers(0, G.COST_MAX + 1, size=(2, 6, 5, 4)).astype(np.uint16)
    for paths in (4, 8):
        assert np.array_equal(G.sgm_aggregate_ref(C, 0, 0, paths), paths * C.astype(np.int64))
        one = C[..., :1]
        assert np.array_equal(G.sgm_aggregate_ref(one, 7, 900, paths), paths * one.astype(np.int64))
        agg = G.sgm_aggregate_ref(C, 7, 900, paths)
        assert (agg >= paths * C.astype(np.int64)).all() and (agg <= paths * (C.astype(np.int64) + 900)).all()
        assert not np.array_equal(agg, paths * C.astype(np.int64))
    lone = C[:, :1, :1]                                    # a 1 x 1 image: no pixel has a predecessor
    assert np.array_equal(G.sgm_aggregate_ref(lone, 7, 900, 8), 8 * lone.astype(np.int64))
    agg = G.sgm_aggregate_ref(C, 0, 900, 4)               # P1 = 0 < P2: a free step to a neighbour is not a free jump
    assert not np.array_equal(agg, 4 * C.astype(np.int64))


def test_quantise_rounds_half_up_clips_and_stores_4095_for_a_nan():
    C = np.array([0.0, 0.0156, 0.015625, 1.0, 127.96, 127.99, 200.0, np.nan, np.inf], np.float32)
    assert G.quantise(C, 32.0).tolist() == [0, 0, 1, 32, 4095, 4095, 4095, 4095, 4095]
    assert G.quantise(C, 32.0).dtype == np.uint16
    assert G.quantise(np.float32(127.95), 32.0) == 4094


def test_select_in_float32_follows_the_winner_rules():
    agg = np.array([[[[50, 20, 10, 20, 60, 30]]], [[[5, 5, 9, 9, 9, 9]]]], np.uint16).transpose(0, 1, 2, 3)       # [2,1,1,6]
    inv = np.linspace(0.1, 0.6, 6, dtype=np.float32)[None].repeat(2, 0)
    out, conf, win, cost = G.sgm_select_ref(agg, inv, np.array([2, 0]))
    assert win[:, 0, 0].tolist() == [2, 0] and cost[:, 0, 0].tolist() == [10.0, 5.0]          # ties to the lowest k
    assert out.dtype == conf.dtype == cost.dtype == np.float32
    assert out[0, 0, 0] == np.float32(1) / inv[0, 2]                                         # symmetric neighbours: no move
    assert conf[0, 0, 0] == (np.float32(30) - np.float32(10)) / np.float32(30)                # the runner-up is two or more steps away
    assert conf[1, 0, 0] == 0                                                                # no present source
    skew = np.array([[[[50, 12, 10, 30, 60, 30]]]], np.uint16)
    out, _, win, _ = G.sgm_select_ref(skew, inv[:1], np.array([1]))
    off = np.float32(0.5) * (np.float32(12) - np.float32(30)) / np.float32(22)
    assert win[0, 0, 0] == 2 and out[0, 0, 0] == np.float32(1) / (inv[0, 2] + (-off) * (inv[0, 1] - inv[0, 2]))


# ------------------------------------------------------------------ the benefit
@pytest.mark.parametrize("case", ["plane", "sphere"])
def test_sgm_recovers_more_of_the_weak_noisy_scene_than_the_winner_alone(case):
    """The all-pixel share within 1.5 hypothesis steps after SGM (4 paths, P1 = 32, P2 = 256 at 32 units per grey level) is at least the
    winner-take-all share + 0.05; quantisation alone moves the winner-take-all share by at most 0.01.  Measured with this oracle: plane
    0.6781 -> 0.7780 (quantised winner 0.6768; 8 paths 0.7247), sphere 0.7491 -> 0.9232 (quantised winner 0.7497; 8 paths 0.8895)."""
    c = G.plane_benefit_case() if case == "plane" else G.sphere_benefit_case()
    assert (c.F, c.S, c.D, c.r) == (5, 4, 32, 1) and c.grey.shape == ((5, 48, 64) if case == "plane" else (5, 48, 96))
    wta, wta_q, sgm = G.benefit_shares(c, 4)
    print(f"{case}: winner-take-all {wta:.4f} (quantised {wta_q:.4f}), SGM 4 paths {sgm:.4f}, gain {sgm - wta:+.4f}")
    assert abs(wta_q - wta) <= G.QUANTISATION_MARGIN
    assert sgm >= wta + G.BENEFIT_MARGIN


def test_the_weak_scene_and_the_noise_are_what_the_issue_states():
    P = np.random.default_rng(2).uniform(-3, 3, size=(50, 3))
    np.testing.assert_allclose(G.weak_scene().texture(P), 128 + 0.2 * (R.BoxScene().texture(P) - 128), rtol=0, atol=1e-12)
    g = np.full((3, 4, 5), 128, np.uint8)
    n = G.noisy(g).astype(int) - 128
    assert np.array_equal(n, np.random.default_rng(7).integers(-3, 4, g.shape)) and np.array_equal(G.noisy(g), G.noisy(g))
    assert G.noisy(np.zeros((40, 40), np.uint8)).min() == 0 and G.noisy(np.full((40, 40), 255, np.uint8)).max() == 255


# ------------------------------------------------------------------ argument checks and plumbing
def test_header_constants_and_build_rule():
    from evoworld_amd import _lib, ops
    assert (_lib.EW_MVS_COST_MAX, _lib.EW_MVS_SGM_MAX_D) == (4095, 256) == (ops.MVS_COST_MAX, ops.MVS_SGM_MAX_D) == (G.COST_MAX, G.MAX_D)
    n_args = {"ew_mvs_plane_sweep_volume": 16, "ew_mvs_sphere_sweep_volume": 15, "ew_mvs_sgm_aggregate": 10, "ew_mvs_sgm_select": 15}
    for name, n in n_args.items():
        assert len(_lib.HEADER.functions[name][1]) == n and _lib.HEADER.functions[name][0] == "ew_status"
        assert hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 20
    make = open(os.path.join(ROOT, "evoworld_amd", "csrc", "Makefile")).read()
    rule = make[make.index("mvs_sgm.o: mvs_sgm.hip"):]
    assert "-ffp-contract=off" in rule.split("\n")[1] and " mvs_sgm.o" in make.split("\n")[4]


def test_ops_check_ranges_before_anything_is_launched():
    from evoworld_amd import _lib, ops
    assert ops.mvs_sgm_check_penalties(0, 0, 4) == (0, 0, 4) and ops.mvs_sgm_check_penalties(32, 4095, 8) == (32, 4095, 8)
    for bad in ((-1, 5, 4), (6, 5, 4), (0, 4096, 4), (1.5, 5, 4), (1, 5, 5), (1, 5, 0)):
        with pytest.raises(ValueError):
            ops.mvs_sgm_check_penalties(*bad)
    assert ops._mvs_view_range(0, None, 5) == (0, 5) and ops._mvs_view_range(2, None, 5) == (2, 3) and ops._mvs_view_range(1, 2, 5) == (1, 2)
    for bad in ((-1, 1), (0, 0), (4, 2), (5, None)):
        with pytest.raises(ValueError):
            ops._mvs_view_range(*bad, 5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops._mvs_cost_scale(bad)
    vol = torch.zeros((1, 2, 3, 4), dtype=torch.uint16)
    with pytest.raises(ValueError):
        ops.mvs_sgm_aggregate(vol[0], 1, 2)                       # not [N,H,W,D]
    with pytest.raises(ValueError):
        ops.mvs_sgm_select(vol[0], torch.zeros(1, 4), torch.zeros(1, 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.mvs_plane_sweep_volume(torch.zeros((2, 3), dtype=torch.uint8), None, None, None)
    with pytest.raises(ValueError):
        ops.mvs_sphere_sweep_volume(torch.zeros((2, 3), dtype=torch.uint8), None, None, None)
    with pytest.raises(_lib.EvoWorldHipError, match="must live on the GPU"):   # there is no host path
        ops.mvs_sgm_aggregate(vol, 1, 2)
    with pytest.raises(_lib.EvoWorldHipError, match="must live on the GPU"):
        ops.mvs_sgm_select(vol, torch.zeros(1, 4), torch.zeros(1, 1, dtype=torch.int32))


def test_stage_classes_check_the_sgm_options():
    for cls in (mvs.PlaneSweepDepth, mvs.SphereSweepDepth):
        d = cls()
        assert d.aggregate == "box" and (d.sgm.P1, d.sgm.P2, d.sgm.paths, d.sgm.cost_scale, d.sgm.workspace_bytes) == (32, 256, 4, 32.0, 2 << 30)
        s = cls(aggregate="sgm", sgm_p1=0.5, sgm_p2=127.9, sgm_paths=8, cost_scale=16.0, workspace_bytes=1000)
        assert s.aggregate == "sgm" and (s.sgm.P1, s.sgm.P2, s.sgm.paths, s.sgm.workspace_bytes) == (8, int(round(127.9 * 16.0)), 8, 1000)
        assert cls(sgm_p1=0.0, sgm_p2=0.0).sgm.P1 == 0 and cls(sgm_p2=4095 / 32.0).sgm.P2 == 4095
        for bad in (dict(aggregate="census"), dict(aggregate=None), dict(sgm_p1=-0.1), dict(sgm_p1=9.0), dict(sgm_p2=128.1), dict(sgm_paths=5),
                    dict(sgm_paths=16), dict(cost_scale=0.0), dict(cost_scale=float("nan")), dict(sgm_p1=float("nan")), dict(workspace_bytes=0),
                    dict(aggregate="sgm", planes=257)):
            with pytest.raises(ValueError):
                cls(**bad)
        assert cls(planes=257).planes == 257                      # the fused sweep has no such limit


def test_view_chunks_cover_every_view_once(monkeypatch):
    from evoworld_amd import ops
    assert mvs.sgm_chunk_views(2 << 30, 384, 512, 64) == (2 << 30) // (4 * 384 * 512 * 64) == 42
    assert mvs.sgm_chunk_views(4 * 48 * 64 * 32, 48, 64, 32) == 1 and mvs.sgm_chunk_views(1, 48, 64, 32) == 1
    assert mvs.sgm_chunk_views(3 * 4 * 6 * 8 * 2 * 4 - 1, 6, 8, 2) == 11 and mvs.sgm_chunk_views(3 * 4 * 6 * 8 * 2 * 4, 6, 8, 2) == 12
    calls = []
    monkeypatch.setattr(ops, "mvs_sgm_aggregate", lambda cost, P1, P2, paths, out=None: calls.append(("agg", tuple(cost.shape), P1, P2, paths, tuple(out.shape))))
    monkeypatch.setattr(ops, "mvs_sgm_select", lambda agg, inv, src, view_begin=0, out=None: calls.append(("sel", tuple(agg.shape), view_begin, tuple(out[0].shape))))
    F, H, W, D = 5, 6, 8, 2
    for ws, want in ((2 * 4 * H * W * D, [(0, 2), (2, 2), (4, 1)]), (1, [(i, 1) for i in range(5)]), (2 << 30, [(0, 5)])):
        calls.clear()
        ranges = []
        opt = mvs.sgm_options("sgm", 1.0, 8.0, 8, 32.0, ws)
        outs = mvs.sgm_sweep(lambda b, m, out: ranges.append((b, m, tuple(out.shape))), torch.zeros(F, D), torch.zeros(F, 1, dtype=torch.int32),
                             F, H, W, D, opt)
        assert [(b, m) for b, m, _ in ranges] == want and all(s == (m, H, W, D) for _, m, s in ranges)
        assert [c for c in calls if c[0] == "agg"] == [("agg", (m, H, W, D), 32, 256, 8, (m, H, W, D)) for _, m in want]
        assert [c for c in calls if c[0] == "sel"] == [("sel", (m, H, W, D), b, (m, H, W)) for b, m in want]
        assert [tuple(o.shape) for o in outs] == [(F, H, W)] * 4 and [o.dtype for o in outs] == [torch.float32, torch.float32, torch.int32, torch.float32]


def test_flags_reach_the_stages_from_both_command_lines():
    import unified_loop_consistency as cli
    from evoworld_amd.stages import load_stages
    a = cli.parse_arguments(["--unet_path", "X"])
    assert (a.mvs_aggregate, a.mvs_p1, a.mvs_p2, a.mvs_paths) == ("box", 1.0, 8.0, 4)
    b = cli.parse_arguments(["--unet_path", "X", "--depth_stage", "mvs", "--mvs_aggregate", "sgm", "--mvs_p1", "2", "--mvs_p2", "10.5", "--mvs_paths", "8",
                             "--mvs_planes", "48"])
    for stage, cls in (("mvs", mvs.PlaneSweepDepth), ("mvs_pano", mvs.SphereSweepDepth)):
        d = load_stages(None, b, depth_stage=stage, camera_params=R.POSE_CAM).depth_model
        assert isinstance(d, cls) and d.aggregate == "sgm" and (d.sgm.P1, d.sgm.P2, d.sgm.paths, d.planes) == (64, 336, 8, 48)
        d = load_stages(None, a, depth_stage=stage, camera_params=R.POSE_CAM).depth_model
        assert d.aggregate == "box" and (d.sgm.P1, d.sgm.P2, d.sgm.paths) == (32, 256, 4)
        d = load_stages(None, SimpleNamespace(svd_path=None), depth_stage=stage, camera_params=R.POSE_CAM).depth_model      # no such attributes
        assert d.aggregate == "box" and d.planes == 64
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--unet_path", "X", "--mvs_aggregate", "census"])
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--unet_path", "X", "--mvs_paths", "6"])
    with pytest.raises(ValueError):                                  # P1 > P2 surfaces where the stage is made
        load_stages(None, cli.parse_arguments(["--unet_path", "X", "--mvs_p1", "9"]), depth_stage="mvs", camera_params=R.POSE_CAM)
    p = mvs.build_parser().parse_args(["cloud", "--frames", "d", "--poses", "p", "--output", "s.ply"])
    assert (p.aggregate, p.sgm_p1, p.sgm_p2, p.sgm_paths) == ("box", 1.0, 8.0, 4)
    p = mvs.build_parser().parse_args(["cloud", "--frames", "d", "--poses", "p", "--output", "s.ply", "--aggregate", "sgm", "--sgm_p1", "0.5", "--sgm_p2", "4",
                                       "--sgm_paths", "8"])
    assert (p.aggregate, p.sgm_p1, p.sgm_p2, p.sgm_paths) == ("sgm", 0.5, 4.0, 8)
    sh = open(os.path.join(ROOT, "run_unified_pipeline.sh")).read()
    for env, flag in (("MVS_AGGREGATE", "--mvs_aggregate"), ("MVS_P1", "--mvs_p1"), ("MVS_P2", "--mvs_p2"), ("MVS_PATHS", "--mvs_paths")):
        assert f'[ -n "${env}" ] && CMD="$CMD {flag} ${env}"' in sh
