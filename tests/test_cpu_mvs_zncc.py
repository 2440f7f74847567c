"""-m 'not gpu': the ZNCC matching cost of the two sweeps on the host -- the float32-order margin of the oracle of
tests/mvs_zncc_ref.py on the inputs of the GPU tests, the cost's invariance to a gain and an offset, what it recovers of the box scene when
the views flicker against what the SAD cost recovers, a flat image, the argument checks of the new ops and of the two stage classes, and
the option's way from the command lines to the stages."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvs_ref as R  # noqa: E402
import mvs_sphere_ref as S  # noqa: E402
import mvs_zncc_ref as Z  # noqa: E402
from evoworld_amd import mvs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"plane": Z.PLANE_CASES, "sphere": Z.SPHERE_CASES}


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_margin_constant_covers_the_measured_float32_error(kind):
    """|float32-order cost - float64 cost| over every GPU case with r >= 1, ambiguous pairs left out (at most 0.5 % of a case, the SAD
    oracles' cap, unchanged: no case had to be dropped).  Measured: plane 8.6e-3, sphere 7.9e-2 percent of cost."""
    assert all(kw["r"] >= 1 for kw in CASES[kind]) and Z.MAX_AMBIGUOUS_SHARE == R.MAX_AMBIGUOUS_SHARE == S.MAX_AMBIGUOUS_SHARE == 0.005
    worst = 0.0
    for kw in CASES[kind]:
        c, Z64, amb = Z.cached(kind, **kw)
        Z32, amb32 = Z.zncc_volume(kind, c, dtype=np.float32)
        assert Z32.dtype == np.float32 and Z64.dtype == np.float64 and np.array_equal(amb, amb32)
        assert float(amb.mean()) <= Z.MAX_AMBIGUOUS_SHARE, Z.case_id(kw)
        assert np.isfinite(Z64).all() and np.isfinite(Z32).all() and Z64.min() >= 0 and Z64.max() <= 200
        err = float(np.abs(Z32.astype(np.float64) - Z64)[~amb].max())
        print(f"{kind} {Z.case_id(kw)}: float32 order within {err:.3e} % of float64; ambiguous pairs left out {float(amb.mean()):.5f}")
        worst = max(worst, err)
    print(f"{kind}: measured margin {worst:.3e}, constant {Z.F32_MARGIN[kind]:.1e}")
    assert worst <= Z.F32_MARGIN[kind] <= Z.ZNCC_F32_MARGIN
    assert Z.ZNCC_F32_MARGIN <= 0.5, "above 0.5 % the rule has to change (subtract the window's centre), not the tolerance"
    assert Z.COST_TOL[kind] == 2 * Z.F32_MARGIN[kind]


def test_cases_are_the_sad_cases_without_the_r0_rows():
    assert len(Z.PLANE_CASES) == 8 and len(Z.SPHERE_CASES) == 7
    assert Z.PLANE_R0["r"] == 0 and Z.SPHERE_R0["r"] == 0
    assert any(kw.get("push_out") for kw in Z.PLANE_CASES) and any(kw.get("no_source_view") is not None for kw in Z.PLANE_CASES)


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_cost_does_not_move_under_a_gain_and_an_offset_of_a_source(kind):
    """An image with values <= 100; view 1 replaced by 2 g + 10 (exact in uint8): wherever the reference's and the source's windows
    have variance, the float64 cost at var_floor = 0 is the same to 1e-9, as a reference (view 0, 2, whose sources include view 1)
    and as the view that changed."""
    if kind == "plane":
        c = R.sweep_case(F=3, H=37, W=53, S=2, D=8, r=2)
    else:
        c = S.sphere_case(F=3, He=20, We=40, S=2, D=8, r=2)
    g = (c.grey.astype(np.float64) * (100.0 / 255.0)).astype(np.uint8)
    assert g.max() <= 100
    g2 = g.copy()
    g2[1] = 2 * g[1] + 10
    A, _, va, vb = Z.zncc_volume(kind, c, var_floor=0.0, grey=g, with_variances=True)
    B, _, va2, vb2 = Z.zncc_volume(kind, c, var_floor=0.0, grey=g2, with_variances=True)
    ok = (va[:, None] > 0) & (vb > 0) & np.isfinite(vb) & (va2[:, None] > 0) & (vb2 > 0)
    assert ok.mean() > 0.5                                   # the comparison is not vacuous (plane: windows that leave a source are left out)
    assert (c.src_index == 1).any(1)[[0, 2]].all()
    assert np.abs(A - B)[ok].max() <= 1e-9
    sad_a = R.cost_volume(g, c.homographies, c.src_index, c.r, 48.0)[0] if kind == "plane" else S.cost_volume(g, c.rel_pose, c.src_index, c.inv_dist, c.r)[0]
    sad_b = R.cost_volume(g2, c.homographies, c.src_index, c.r, 48.0)[0] if kind == "plane" else S.cost_volume(g2, c.rel_pose, c.src_index, c.inv_dist, c.r)[0]
    assert np.abs(sad_a - sad_b).max() > 10                  # the SAD cost reads the same change as tens of grey levels


def test_flicker_is_what_the_issue_states():
    g = np.stack([np.linspace(0, 255, 64).reshape(8, 8)] * 6)
    f = Z.flicker(g)
    assert f.dtype == np.uint8 and np.array_equal(f[0], np.rint(g[0]).astype(np.uint8)) and np.array_equal(f[5], f[0])     # view 0 (and 5) untouched
    v = np.clip(128 + 0.7 * (g[1] - 128) + 20, 0, 255)
    assert np.array_equal(f[1], np.rint(255 * (v / 255) ** 0.8).astype(np.uint8))
    assert (Z.FLICKER_GAIN, Z.FLICKER_OFFSET, Z.FLICKER_GAMMA) == ((1, 0.7, 1.3, 0.75, 1.25), (0, 20, -25, 15, -10), (1, 0.8, 1.25, 1.2, 0.85))


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_zncc_recovers_the_flickering_scene_and_sad_does_not(kind):
    """RECOVERY_CASE, the float64 oracles, R.kept_and_correct.  Measured: plane ZNCC 0.9142 clean, 0.9148 flicker; SAD 0.9635 clean, 0.5977
    flicker.  Sphere ZNCC 0.9645 clean, 0.9624 flicker; SAD 0.9992 clean, 0.6383 flicker."""
    s = Z.recovery_shares(kind)
    print(f"{kind}: ZNCC {s['zncc_clean']:.4f} clean, {s['zncc_flicker']:.4f} flicker; SAD {s['sad_clean']:.4f} clean, {s['sad_flicker']:.4f} flicker")
    assert abs(s["zncc_flicker"] - s["zncc_clean"]) <= 0.02
    assert s["zncc_flicker"] >= s["sad_flicker"] + 0.2


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_a_flat_image_costs_100_everywhere(kind):
    """No variance anywhere: zncc = 0 through the floor, so every cost is 100 -- winner 0, confidence 0, nothing non-finite; in both
    precisions.  (Plane: a window that leaves a source costs oob_cost = 100 as well.)"""
    c = R.sweep_case(F=3, H=20, W=40, S=2, D=5, r=1) if kind == "plane" else S.sphere_case(F=3, He=20, We=40, S=2, D=5, r=1)
    flat = np.full_like(c.grey, 93)
    _, inv, _ = Z.truth_and_tables(kind, c)
    for dt in (np.float64, np.float32):
        C, _ = Z.zncc_volume(kind, c, dtype=dt, grey=flat)
        assert np.isfinite(C).all() and (C == 100).all()
        for f in range(c.F):
            out, conf, k, cost = R.sweep_ref(C[f], inv[f], 2)
            assert (k == 0).all() and (conf == 0).all() and (cost == 100).all() and np.isfinite(out).all()


def test_correlation_rules_on_hand_made_sums():
    """n = 4 taps, a = (1, 2, 3, 4): b = a -> zncc = 1 without a floor; b = -a -> -1; b flat -> 0 and never a NaN, also at var_floor = 0;
    the floor pulls a weak window towards 0"""
    a = np.array([1.0, 2.0, 3.0, 4.0])
    sums = lambda b: (4, a.sum(), (a * a).sum(), b.sum(), (b * b).sum(), (a * b).sum())
    for dt in (np.float64, np.float32):
        f = lambda b, vf: float(Z.correlation_cost(*[np.asarray(v, dt) if i else v for i, v in enumerate(sums(b))], vf, dt)[0])
        assert f(a, 0.0) == 0.0 and f(3 * a + 7, 0.0) == pytest.approx(0.0, abs=1e-4) and f(-a, 0.0) == 200.0
        assert f(np.full(4, 9.0), 0.0) == 100.0 and f(np.full(4, 9.0), 1.0) == 100.0
        va = 4 * 30.0 - 100.0                                # n Saa - Sa Sa = 20
        assert f(a, 1.0) == pytest.approx(100 * (1 - va / np.sqrt(va * va + 16.0 ** 2)), rel=1e-6)


# ------------------------------------------------------------------ header, build rule, argument checks
def test_header_symbols_and_build_rule():
    from evoworld_amd import _lib
    n_args = {"ew_mvs_plane_sweep_zncc": 17, "ew_mvs_plane_sweep_zncc_volume": 17, "ew_mvs_sphere_sweep_zncc": 16, "ew_mvs_sphere_sweep_zncc_volume": 16}
    for name, n in n_args.items():
        assert len(_lib.HEADER.functions[name][1]) == n and _lib.HEADER.functions[name][0] == "ew_status"
        assert hasattr(_lib.load(), name)
        sad = name.replace("_zncc", "")
        twin = list(_lib.HEADER.functions[sad][1])
        at = {17: 15, 16: 14}[n] if name.endswith("zncc") else {17: 12, 16: 11}[n]
        assert _lib.HEADER.functions[name][1] == twin[:at] + ["float"] + twin[at:], name     # the SAD entry's arguments plus var_floor
    assert _lib.ABI_VERSION == 20
    make = open(os.path.join(ROOT, "evoworld_amd", "csrc", "Makefile")).read()
    rule = make[make.index("mvs_zncc.o: mvs_zncc.hip"):]
    assert "-ffp-contract=off" in rule.split("\n")[1] and "fast-math" not in make and " mvs_zncc.o" in make.split("\n")[4]


def test_ops_check_the_zncc_options_before_anything_is_launched():
    from evoworld_amd import _lib, ops
    assert ops._mvs_zncc_options(1, 0) == (1, 0.0) and ops._mvs_zncc_options(3, 2.5) == (3, 2.5)
    for bad in ((0, 1.0), (4, 1.0), (-1, 1.0), (2, -0.1), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(ValueError, match=repr(bad[0]) if bad[0] not in (1, 2, 3) else "var_floor"):
            ops._mvs_zncc_options(*bad)
    g = torch.zeros((2, 8, 16), dtype=torch.uint8)
    for fn in (ops.mvs_plane_sweep_zncc, ops.mvs_plane_sweep_zncc_volume, ops.mvs_sphere_sweep_zncc, ops.mvs_sphere_sweep_zncc_volume):
        with pytest.raises(ValueError, match="patch_radius"):
            fn(g, None, None, None, patch_radius=0)
        with pytest.raises(ValueError, match="var_floor"):
            fn(g, None, None, None, var_floor=-1.0)
        with pytest.raises(ValueError, match="grey"):
            fn(g[0], None, None, None)
        with pytest.raises(_lib.EvoWorldHipError, match="must live on the GPU"):       # there is no host path
            fn(g, torch.zeros(2, 1, 4, 3, 3), torch.zeros(2, 1, dtype=torch.int32), torch.ones(2, 4))


def test_stage_classes_check_the_cost_options():
    assert mvs.COSTS == ("sad", "zncc")
    for cls in (mvs.PlaneSweepDepth, mvs.SphereSweepDepth):
        d = cls()
        assert d.cost == "sad" and d.sgm.cost_scale == 32.0 and (d.sgm.P1, d.sgm.P2) == (32, 256)
        z = cls(cost="zncc")
        assert z.cost == "zncc" and z.var_floor == 1.0 and z.sgm.cost_scale == 16.0 and (z.sgm.P1, z.sgm.P2) == (16, 128) and z.aggregate == "box"
        z = cls(cost="zncc", aggregate="sgm", sgm_p1=2, sgm_p2=32, var_floor=0.0, cost_scale=8.0)
        assert (z.sgm.P1, z.sgm.P2, z.sgm.cost_scale, z.var_floor, z.aggregate) == (16, 256, 8.0, 0.0, "sgm")
        assert cls(cost="sad", cost_scale=16.0).sgm.cost_scale == 16.0 and cls(patch_radius=0).patch_radius == 0
        for bad, word in ((dict(cost="census"), "census"), (dict(cost=None), "None"), (dict(cost="zncc", patch_radius=0), "0"),
                          (dict(cost="zncc", var_floor=-0.5), "-0.5"), (dict(var_floor=float("nan")), "nan"), (dict(var_floor=float("inf")), "inf"),
                          (dict(cost="zncc", cost_scale=0.0), "0.0")):
            with pytest.raises(ValueError, match=word):
                cls(**bad)
    assert mvs.PlaneSweepDepth(cost="zncc").zncc_oob_cost == 100.0 and mvs.PlaneSweepDepth(cost="zncc").oob_cost == 48.0
    assert mvs.PlaneSweepDepth(cost="zncc", zncc_oob_cost=150).zncc_oob_cost == 150.0


def test_stage_calls_the_zncc_entries_and_the_default_calls_the_old_ones(monkeypatch):
    """Which ops a stage reaches, with every op replaced by a recorder: cost='sad' reaches exactly today's calls."""
    from evoworld_amd import ops
    calls = []

    def fake(name, n_out):
        def f(grey, *a, **kw):
            calls.append((name, a[3:], kw.keys()))
            if n_out == 1:
                return None
            return tuple(torch.ones(grey.shape, dtype=dt) for dt in (torch.float32, torch.float32, torch.int32, torch.float32))
        return f

    for name in ("mvs_plane_sweep", "mvs_plane_sweep_zncc", "mvs_sphere_sweep", "mvs_sphere_sweep_zncc"):
        monkeypatch.setattr(ops, name, fake(name, 4))
    for name in ("mvs_plane_sweep_volume", "mvs_plane_sweep_zncc_volume", "mvs_sphere_sweep_volume", "mvs_sphere_sweep_zncc_volume"):
        monkeypatch.setattr(ops, name, fake(name, 1))
    monkeypatch.setattr(ops, "mvs_luma", lambda frames: frames[..., 0].contiguous())
    monkeypatch.setattr(ops, "mvs_consistency", lambda *a, **k: None)
    monkeypatch.setattr(ops, "mvs_sphere_consistency", lambda *a, **k: None)
    monkeypatch.setattr(ops, "pano_unproject", lambda dist, c2w: torch.zeros(dist.shape + (3,)))
    monkeypatch.setattr(ops, "mvs_sgm_aggregate", lambda *a, **k: None)
    monkeypatch.setattr(ops, "mvs_sgm_select", lambda *a, **k: None)
    frames = torch.zeros((3, 16, 32, 3), dtype=torch.uint8)
    w2c = R.arc_path(3)
    for cls, word, kw in ((mvs.PlaneSweepDepth, "plane", "view_w2c"), (mvs.SphereSweepDepth, "sphere", "pano_w2c")):
        for cost, agg, want in (("sad", "box", f"mvs_{word}_sweep"), ("zncc", "box", f"mvs_{word}_sweep_zncc"),
                                ("sad", "sgm", f"mvs_{word}_sweep_volume"), ("zncc", "sgm", f"mvs_{word}_sweep_zncc_volume")):
            calls.clear()
            cls(n_src=2, planes=4, cost=cost, aggregate=agg, var_floor=0.25, cost_scale=None)(frames, **{kw: w2c})
            assert [c[0] for c in calls] == [want], (cost, agg, calls)
            tail = calls[0][1]
            if cost == "zncc" and word == "plane":
                assert tail[:3] == (2, 100.0, 0.25) and (agg == "box" or tail[3] == 16.0)
            elif cost == "zncc":
                assert tail[:2] == (2, 0.25) and (agg == "box" or tail[2] == 16.0)
            elif word == "plane":
                assert tail[:2] == (2, 48.0) and (agg == "box" or tail[2] == 32.0)
            else:
                assert tail[:1] == (2,) and (agg == "box" or tail[1] == 32.0)


def test_option_reaches_the_stages_from_both_command_lines():
    import unified_loop_consistency as cli
    from evoworld_amd.stages import MVS_OPTIONS, load_stages
    assert ("cost", "mvs_cost") in MVS_OPTIONS
    a = cli.parse_arguments(["--unet_path", "X"])
    assert a.mvs_cost == "sad" and (a.mvs_aggregate, a.mvs_p1, a.mvs_p2) == ("box", 1.0, 8.0)
    b = cli.parse_arguments(["--unet_path", "X", "--depth_stage", "mvs", "--mvs_cost", "zncc", "--mvs_aggregate", "sgm", "--mvs_p2", "32"])
    for stage, cls in (("mvs", mvs.PlaneSweepDepth), ("mvs_pano", mvs.SphereSweepDepth)):
        d = load_stages(None, b, depth_stage=stage, camera_params=R.POSE_CAM).depth_model
        assert isinstance(d, cls) and d.cost == "zncc" and d.aggregate == "sgm" and (d.sgm.P1, d.sgm.P2, d.sgm.cost_scale) == (16, 512, 16.0)
        d = load_stages(None, a, depth_stage=stage, camera_params=R.POSE_CAM).depth_model
        assert d.cost == "sad" and d.sgm.cost_scale == 32.0
        d = load_stages(None, SimpleNamespace(svd_path=None), depth_stage=stage, camera_params=R.POSE_CAM).depth_model        # no such attribute
        assert d.cost == "sad"
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--unet_path", "X", "--mvs_cost", "census"])
    with pytest.raises(SystemExit):                                 # --mvs_aggregate keeps its two choices
        cli.parse_arguments(["--unet_path", "X", "--mvs_aggregate", "zncc"])
    p = mvs.build_parser().parse_args(["cloud", "--frames", "d", "--poses", "p", "--output", "s.ply"])
    assert p.cost == "sad" and (p.sgm_p1, p.sgm_p2) == (1.0, 8.0)
    p = mvs.build_parser().parse_args(["cloud", "--frames", "d", "--poses", "p", "--output", "s.ply", "--cost", "zncc"])
    assert p.cost == "zncc"
    with pytest.raises(SystemExit):
        mvs.build_parser().parse_args(["cloud", "--frames", "d", "--poses", "p", "--output", "s.ply", "--cost", "census"])
    sh = open(os.path.join(ROOT, "run_unified_pipeline.sh")).read()
    assert '[ -n "$MVS_COST" ] && CMD="$CMD --mvs_cost $MVS_COST"' in sh
