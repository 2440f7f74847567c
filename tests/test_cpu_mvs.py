"""CPU tests of the plane-sweep stereo stage (evoworld_amd/mvs.py): the host geometry, the numpy oracle on the analytic
box scene (tests/mvs_ref.py), the margin and the ambiguity share that the GPU tests (tests/test_gpu_mvs.py) rely on, and the opt-in wiring.
No GPU and no library call."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvs_ref as R  # noqa: E402
from evoworld_amd import mvs  # noqa: E402


def _project(K, w2c, X):
    x = K @ (w2c[:3, :3] @ X + w2c[:3, 3])
    return x[:2] / x[2], x[2]


# ------------------------------------------------------------------ sweep geometry
def test_homographies_map_plane_points_between_views():
    """A 3D point on plane k of the reference view projects into the source where the homography sends its reference pixel: 1e-9 px."""
    w2c = R.arc_path(5)
    K = mvs.pinhole(48, 64)
    st = mvs.sweep_setup(w2c, K, 4, 32)
    E = np.concatenate([w2c, np.tile([[[0, 0, 0, 1.0]]], (5, 1, 1))], 1)
    rng = np.random.default_rng(0)
    worst = 0.0
    for f in range(5):
        c2w = np.linalg.inv(E[f])
        for s in range(4):
            j = st.src_index[f, s]
            for k in (0, 7, 31):
                for _ in range(4):
                    p = np.array([rng.uniform(0, 63), rng.uniform(0, 47), 1.0])
                    z = 1.0 / st.inv_depth[f, k]
                    Xw = c2w[:3, :3] @ (np.linalg.inv(K) @ p * z) + c2w[:3, 3]
                    want, depth_in_src = _project(K, w2c[j], Xw)
                    q = st.homographies[f, s, k] @ p
                    worst = max(worst, float(np.abs(q[:2] / q[2] - want).max()))
                    assert abs(q[2] - depth_in_src / z) < 1e-9           # q2 is the source depth over the reference depth
                    T = np.concatenate([st.rel_pose[f, s], [[0, 0, 0, 1.0]]])
                    np.testing.assert_allclose(T, E[j] @ c2w, atol=1e-12)
    assert worst < 1e-9, worst


def test_default_range_is_one_pixel_of_disparity_per_plane():
    w2c = R.arc_path(5)
    K = mvs.pinhole(48, 64)
    for D in (2, 3, 32):
        st = mvs.sweep_setup(w2c, K, 4, D)
        b_max = st.baseline.max(1)
        np.testing.assert_allclose(st.z_far, K[0, 0] * b_max, rtol=1e-12)
        np.testing.assert_allclose(st.z_near, st.z_far / D, rtol=1e-12)
        steps = np.diff(st.inv_depth, axis=1)
        np.testing.assert_allclose(K[0, 0] * b_max[:, None] * steps, 1.0, rtol=1e-9)     # f b d(1/z) = 1 px at the widest baseline
        np.testing.assert_allclose(st.inv_depth[:, 0], 1 / st.z_far)
        np.testing.assert_allclose(st.inv_depth[:, -1], 1 / st.z_near)
    given = mvs.sweep_setup(w2c, K, 2, 8, z_near=2.0, z_far=10.0)
    np.testing.assert_allclose(given.inv_depth, np.tile(np.linspace(0.1, 0.5, 8), (5, 1)))
    assert given.homographies_f32.dtype == np.float32 and given.homographies.dtype == np.float64


def test_sources_at_the_ends_with_a_repeated_pose_and_alone():
    centres = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0], [5, 0, 0]])
    src = mvs.choose_sources(centres, 4)
    assert src[0].tolist() == [1, 2, 3, 4] and src[5].tolist() == [4, 3, 2, 1]       # an end fills from the one side there is
    assert src[2].tolist() == [1, 3, 0, 4] and src[1].tolist() == [0, 2, 3, 4]       # nearest first, lower index first
    rep = centres.copy()
    rep[3] = rep[2]                                                                  # a repeated pose is no source: zero baseline
    src = mvs.choose_sources(rep, 2)
    assert src[2].tolist() == [1, 0] and src[3].tolist() == [4, 1] and src[4].tolist() == [3, 5]
    assert mvs.choose_sources(centres[:2], 4).tolist() == [[1, -1, -1, -1], [0, -1, -1, -1]]
    K = mvs.pinhole(8, 8)
    one = mvs.sweep_setup(R.arc_path(1), K, 4, 16)
    assert one.src_index.tolist() == [[-1] * 4] and not one.has_source[0]
    np.testing.assert_allclose(one.inv_depth, 1.0)                                    # nothing to sweep: depth 1.0, one value
    w2c = R.arc_path(3)
    w2c[2] = w2c[1]
    st = mvs.sweep_setup(np.stack([w2c[0], w2c[0], w2c[0]]), K, 2, 4)                  # all poses equal: no view has a source
    assert (st.src_index == -1).all() and np.allclose(st.inv_depth, 1.0)
    lone = mvs.sweep_setup(w2c, K, 1, 4, min_baseline=1e-6)
    assert lone.src_index[:, 0].tolist() == [1, 0, 0]


# ------------------------------------------------------------------ the oracle on the box scene
@pytest.fixture(scope="module")
def recovery():
    c = R.cached_case(**R.RECOVERY_CASE)
    st = c.setup
    outs = [R.sweep_ref(c.C64[f], st.inv_depth[f], int(R.present(c.src_index, c.F)[f].sum())) for f in range(c.F)]
    depth, conf = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    K = c.K
    conf2, _, _ = R.consistency_ref(depth, c.rel_pose, c.src_index, conf, K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0.02, 2)
    return c, depth, conf, conf2


def test_float64_oracle_recovers_the_box_scene(recovery):
    """5 views of 48 x 64 on a curved path, D = 32, r = 2: of the pixels the pipeline would keep (confidence >= its 50th percentile) at least
    95 % lie within 1.5 plane steps of the true inverse depth.  A condition on the inputs (path, texture, box), met by the float64
    oracle; the device is asked 90 % of the same scene."""
    c, depth, conf, conf2 = recovery
    step = np.diff(c.setup.inv_depth, axis=1)[:, 0]
    raw, n_raw = R.kept_and_correct(conf, depth, c.true_depth, step)
    share, n = R.kept_and_correct(conf2, depth, c.true_depth, step)
    print(f"recovery: sweep alone {raw:.4f} of {n_raw}, after the consistency check {share:.4f} of {n}; zeroed {float((conf2 == 0).mean()):.3f}")
    assert np.percentile(conf2, 50.0) > 0, "the consistency check rejects more than half of the pixels: the percentile filter keeps all"
    assert share >= 0.95 and raw >= 0.95, (share, raw)


@pytest.mark.parametrize("kw", R.GPU_CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items() if k in "FHWSDr"))
def test_ambiguous_taps_are_rare_on_the_gpu_inputs(kw):
    c = R.cached_case(**kw)
    share = float(c.ambiguous.mean())
    print(f"{c.id}: ambiguous (pixel, plane) pairs {share:.5f}")
    assert share <= R.MAX_AMBIGUOUS_SHARE, share


def test_margin_constant_covers_the_measured_float32_error():
    """The largest |float32-order cost - float64 cost| over the GPU tests' inputs, ambiguous taps left out: the GPU tests allow twice
    the constant, which must therefore still cover what is measured here."""
    worst = 0.0
    for kw in R.GPU_CASES:
        c = R.cached_case(**kw)
        C32, _ = R.cost_volume(c.grey, c.homographies, c.src_index, c.r, c.oob, np.float32)
        assert C32.dtype == np.float32
        d = np.abs(C32.astype(np.float64) - c.C64)[~c.ambiguous]
        worst = max(worst, float(d.max()))
        print(f"{c.id}: float32-order vs float64 cost, max {float(d.max()):.3e} grey levels")
    print(f"measured margin {worst:.3e}; constant {R.F32_ORDER_MARGIN:.3e}; GPU tolerance {R.COST_TOL:.3e}")
    assert R.F32_ORDER_MARGIN >= worst
    assert R.F32_ORDER_MARGIN <= 2 * worst, "the constant has drifted far above the measurement: re-measure and lower it"
    assert R.COST_TOL == 2 * R.F32_ORDER_MARGIN


def test_winner_rules_on_hand_made_costs():
    C = np.array([5.0, 3.0, 1.0, 2.0, 4.0, 1.0])[:, None, None]                       # tie between planes 2 and 5: the lowest wins
    k = R.winner_ref(C)
    assert k.item() == 2
    off, refined, curv = R.parabola_offset(C, k)
    assert refined.item() and curv.item() == 3.0 and abs(off.item() - 0.5 * (3 - 2) / 3) < 1e-15
    conf, has = R.confidence_ref(C, k, 1)
    assert has.item() and conf.item() == 0.0                                          # runner-up: plane 5, more than one step away, same cost
    inv = np.linspace(0.1, 0.6, 6)
    assert abs(R.inverse_depth_at(inv, k, off).item() - (0.3 + off.item() * 0.1)) < 1e-15
    assert abs(R.inverse_depth_at(inv, k, -off).item() - (0.3 - off.item() * 0.1)) < 1e-15
    edge = np.array([1.0, 2.0, 3.0])[:, None, None]
    k = R.winner_ref(edge)
    assert k.item() == 0 and not R.parabola_offset(edge, k)[1].item()
    assert R.confidence_ref(edge, k, 1)[0].item() == pytest.approx(2 / 3) and R.confidence_ref(edge, k, 0)[0].item() == 0.0
    two = np.array([2.0, 1.0])[:, None, None]
    assert not R.confidence_ref(two, R.winner_ref(two), 1)[1].item()                  # D = 2: no plane more than one step away
    flat = np.array([2.0, 1.0, 1.0, 1.0, 2.0])[:, None, None]                         # not convex around the winner: no refinement
    assert not R.parabola_offset(flat, np.array([[2]]))[1].item()
    steep = np.array([9.0, 1.0, 1.0, 5.0])[:, None, None]                             # a tie with the neighbour: half a step, the bound
    assert R.parabola_offset(steep, R.winner_ref(steep))[0].item() == 0.5


# ------------------------------------------------------------------ the views' poses
POSE_CAM = R.POSE_CAM


def test_view_poses_are_the_cameras_of_the_cut_views():
    """Panoramas of the box scene at the episode's cameras, cut into views the way ew_equi2pers does it (the oracle's float32
    restatement, truncated to 8 bits), against the scene rendered directly at view_poses: within 2 grey levels away from box edges."""
    from evoworld_amd import reprojection as RP
    from evoworld_amd.geometry import xyz_euler_to_four_by_four_matrix_batch
    from oracle.reproject_ref import equi2pers_ref32
    scene = R.pose_scene()
    n = 5
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(POSE_CAM[:n]), relative=False).numpy()
    panos = scene.render_panos(c2w, 128, 256)
    yaws = RP.calculate_target_yaws(POSE_CAM, n, 0)
    rot = np.stack([RP.Equi2Pers.rotation({"pitch": 0, "roll": 0, "yaw": float(y)}) for y in yaws])
    cut = np.clip(equi2pers_ref32(panos, rot, 48, 64, 90.0), 0, 255).astype(np.uint8)[..., 0]
    w2c = mvs.view_poses(POSE_CAM, n, 0, relative=False)
    direct, _, face, _ = scene.render_views(w2c, mvs.pinhole(48, 64), 48, 64)
    edge = R.near_face_edge(face)
    diff = np.abs(cut.astype(int) - direct.astype(int))
    print(f"cut vs direct: max {diff[~edge].max()} grey levels away from edges; edge share {edge.mean():.4f}")
    assert edge.mean() <= 0.03 and diff[~edge].max() <= 2
    rel = mvs.view_poses(POSE_CAM, n, 0)
    np.testing.assert_allclose(rel[0], np.eye(4)[:3], atol=1e-12)                     # relative to the first view
    E = lambda w: np.concatenate([w, np.tile([[[0, 0, 0, 1.0]]], (len(w), 1, 1))], 1)
    np.testing.assert_allclose(E(rel), E(w2c) @ np.linalg.inv(E(w2c)[0])[None], atol=1e-12)
    with pytest.raises(ValueError):
        mvs.view_poses(POSE_CAM[:3], 5, 0)


# ------------------------------------------------------------------ wiring, CLI, loader
def test_depth_stage_dispatch_leaves_a_plain_callable_untouched():
    calls = []

    def plain(*a, **kw):
        calls.append((a, kw))
        return "plain"

    class Wants:
        wants_view_poses = True

        def __call__(self, *a, **kw):
            calls.append((a, kw))
            return "wants"

    pers = torch.zeros(5, 4, 4, 3, dtype=torch.uint8)
    assert mvs.call_depth_model(plain, pers, POSE_CAM, 0) == "plain"
    (a, kw), = calls
    assert len(a) == 1 and a[0] is pers and kw == {}                                  # one positional argument, as before
    calls.clear()
    assert mvs.call_depth_model(Wants(), pers, POSE_CAM, 0) == "wants"
    (a, kw), = calls
    assert len(a) == 1 and a[0] is pers and list(kw) == ["view_w2c"]
    np.testing.assert_array_equal(kw["view_w2c"], mvs.view_poses(POSE_CAM, 5, 0))
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    src = inspect.getsource(UnifiedLoopConsistencyPipeline.process_episode)
    assert "call_depth_model(self.depth_model, pers, camera_params, seg)" in src and "self.depth_model(" not in src
    assert mvs.PlaneSweepDepth.wants_view_poses is True


def test_cli_flag_and_loader_defaults():
    import unified_loop_consistency as cli
    from evoworld_amd.stages import SyntheticStages, load_stages
    a = cli.parse_arguments(["--unet_path", "X"])
    assert a.depth_stage == "synthetic" and a.mvs_planes == 64 and a.mvs_sources == 4
    b = cli.parse_arguments(["--unet_path", "X", "--depth_stage", "mvs", "--mvs_planes", "48", "--mvs_sources", "2"])
    assert (b.depth_stage, b.mvs_planes, b.mvs_sources) == ("mvs", 48, 2)
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--unet_path", "X", "--depth_stage", "vggt"])
    for ds in (None, "synthetic"):
        st = load_stages(None, a, depth_stage=ds, camera_params=POSE_CAM)
        assert type(st) is SyntheticStages and st.depth_model.__func__ is SyntheticStages.depth_model and st.depth_model.__self__ is st
    st = load_stages(None, a, camera_params=POSE_CAM)                                  # the call every existing caller makes
    assert type(st) is SyntheticStages and st.depth_model.__func__ is SyntheticStages.depth_model
    m = load_stages(None, b, depth_stage="mvs", camera_params=POSE_CAM)
    assert type(m) is SyntheticStages and isinstance(m.depth_model, mvs.PlaneSweepDepth)
    assert (m.depth_model.planes, m.depth_model.n_src) == (48, 2) and m.vae is not None   # only depth_model is replaced
    np.testing.assert_array_equal(m.depth_model.camera_params, POSE_CAM)
    with pytest.raises(ValueError):
        load_stages(None, a, depth_stage="vggt")
    p = mvs.build_parser().parse_args(["cloud", "--frames", "d", "--poses", "camera_poses.txt", "--segment", "1", "--output", "s.ply"])
    assert (p.command, p.segment, p.planes, p.sources, p.output) == ("cloud", 1, 64, 4, "s.ply")
