"""CPU tests of the sphere-sweep stereo stage (evoworld_amd/mvs.py): the host geometry, the numpy oracle on the analytic box
scene seen by panorama cameras (tests/mvs_sphere_ref.py), the margin and the ambiguity share that the GPU tests
(tests/test_gpu_mvs_sphere.py) rely on, the panorama cameras' poses and the opt-in wiring.  No GPU and no library call."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvs_ref as R  # noqa: E402
import mvs_sphere_ref as S  # noqa: E402
from evoworld_amd import mvs  # noqa: E402

POSE_CAM = R.POSE_CAM


# ------------------------------------------------------------------ the direction <-> pixel map
def test_pixel_and_direction_maps_are_inverse_and_are_the_maps_of_equi2pers():
    """pix(dir(x, y)) = (x, y) modulo We away from row 0 (whose latitude lies beyond the pole, as render_panos renders it), in float64 to 1e-9 px
    and in the float32 order to 1e-3 px; and the forward side is the one oracle/reproject_ref.py restates: a 90-degree view's centre ray
    lands where equi2pers_ref32 samples it."""
    from oracle.reproject_ref import equi2pers_ref32
    for He, We in ((8, 16), (20, 40), (48, 96)):
        y, x = np.meshgrid(np.arange(He, dtype=np.float64), np.arange(We, dtype=np.float64), indexing="ij")
        for dt, tol in ((np.float64, 1e-9), (np.float32, 1e-3)):
            d = S.pixel_dir(He, We, dt)
            np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=-1), 1.0, atol=1e-6)
            u, v, nrm = S.dir_pixel(d[..., 0], d[..., 1], d[..., 2], He, We, dt)
            du = (u - x + We / 2) % We - We / 2                                        # column 0 lies beyond the seam: u = We
            assert np.abs(du)[1:].max() <= tol and np.abs(v - y)[1:].max() <= tol
    # a ramp panorama whose red channel is the column index: the view's centre pixel looks along +z and must read column We / 2 + 0.5
    He, We = 16, 32
    pano = np.zeros((1, He, We, 3), np.uint8)
    pano[..., 0] = np.arange(We)[None, None]
    pano[..., 1] = np.arange(He)[None, :, None]
    cut = equi2pers_ref32(pano, np.eye(3, dtype=np.float32)[None], 4, 4, 90.0)[0, 2, 2]
    u, v, _ = S.dir_pixel(np.float64(0), np.float64(0), np.float64(1), He, We)
    assert (u, v) == (We / 2 + 0.5, He / 2 + 0.5) and abs(cut[0] - u) < 1e-5 and abs(cut[1] - v) < 1e-5


def test_box_filter_wraps_across_the_seam_and_drops_rows_outside():
    rng = np.random.default_rng(1)
    for (He, We), r in (((5, 7), 3), ((8, 16), 2), ((4, 9), 0)):
        a = rng.uniform(0, 9, (He, We))
        got = S._box(a, r, np.float64)
        for y in range(He):
            for x in range(We):
                want = sum(a[yy, xx % We] for yy in range(y - r, y + r + 1) if 0 <= yy < He for xx in range(x - r, x + r + 1))
                assert abs(got[y, x] - want) < 1e-12
        assert S.window_rows(He, r).tolist() == [min(y + r, He - 1) - max(y - r, 0) + 1 for y in range(He)]


# ------------------------------------------------------------------ set-up
def test_default_range_is_one_pixel_of_angular_disparity_per_hypothesis():
    w2c = R.arc_path(5)
    E = S._four(w2c)
    for D in (2, 3, 32):
        st = mvs.sphere_setup(w2c, 96, 4, D)
        b_max = st.baseline.max(1)
        np.testing.assert_allclose(st.d_far, b_max * 96 / (2 * np.pi), rtol=1e-12)
        np.testing.assert_allclose(st.d_near, st.d_far / D, rtol=1e-12)
        steps = np.diff(st.inv_dist, axis=1)
        np.testing.assert_allclose(b_max[:, None] * steps * 96 / (2 * np.pi), 1.0, rtol=1e-9)   # b d(1/d) = one pixel's angle
        np.testing.assert_allclose(st.inv_dist[:, 0], 1 / st.d_far)
        np.testing.assert_allclose(st.inv_dist[:, -1], 1 / st.d_near)
        assert np.array_equal(st.src_index, mvs.choose_sources(np.linalg.inv(E)[:, :3, 3], 4))
        for f in range(5):
            for s in range(4):
                np.testing.assert_allclose(st.rel_pose[f, s], (E[st.src_index[f, s]] @ np.linalg.inv(E[f]))[:3], atol=1e-12)
    given = mvs.sphere_setup(w2c, 96, 2, 8, d_near=2.0, d_far=10.0)
    np.testing.assert_allclose(given.inv_dist, np.tile(np.linspace(0.1, 0.5, 8), (5, 1)))
    assert given.inv_dist_f32.dtype == np.float32 and given.rel_pose_f32.dtype == np.float32 and given.rel_pose.dtype == np.float64
    one = mvs.sphere_setup(R.arc_path(1), 16, 4, 16)                                  # nothing to sweep: distance 1.0, one value
    assert one.src_index.tolist() == [[-1] * 4] and not one.has_source[0]
    np.testing.assert_allclose(one.inv_dist, 1.0)
    rep = R.arc_path(3)
    rep[2] = rep[1]
    st = mvs.sphere_setup(np.stack([rep[1], rep[1], rep[1]]), 16, 2, 4)
    assert (st.src_index == -1).all() and np.allclose(st.inv_dist, 1.0)
    np.testing.assert_allclose(st.rel_pose, np.tile(np.eye(4)[:3], (3, 2, 1, 1)))
    with pytest.raises(ValueError):
        mvs.sphere_setup(w2c, 96, 0, 4)


# ------------------------------------------------------------------ the oracle on the box scene
def test_float64_oracle_recovers_the_box_scene():
    """5 panoramas of 48 x 96 on the arc, D = 32, r = 2, 4 sources: of the pixels the pipeline would keep (confidence >= its 50th
    percentile) at least 95 % lie within 1.5 hypothesis steps of the true inverse distance.  A condition on the inputs, met by the
    float64 oracle (0.9993 when this was written; 0.9914 of ALL pixels); the device is asked 90 % of the same scene."""
    c = S.cached_case(**S.RECOVERY_CASE)
    st = c.setup
    outs = [R.sweep_ref(c.C64[f], st.inv_dist[f], int(R.present(c.src_index, c.F)[f].sum())) for f in range(c.F)]
    dist, conf = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    conf2, _, border = S.consistency_ref(dist, c.rel_pose, c.src_index, conf, 0.02, 2)
    step = np.diff(st.inv_dist, axis=1)[:, 0]
    raw, n_raw = R.kept_and_correct(conf, dist, c.true_dist, step)
    share, n = R.kept_and_correct(conf2, dist, c.true_dist, step)
    every = float((np.abs(1 / dist - 1 / c.true_dist) / step[:, None, None] <= 1.5).mean())
    print(f"recovery: sweep alone {raw:.4f} of {n_raw}, after the consistency check {share:.4f} of {n}, all pixels {every:.4f}; "
          f"zeroed {float((conf2 == 0).mean()):.3f}")
    assert np.percentile(conf2, 50.0) > 0, "the consistency check rejects more than half of the pixels: the percentile filter keeps all"
    assert share >= 0.95 and raw >= 0.95, (share, raw)


_ids = lambda kw: "-".join(f"{k}{v}" for k, v in kw.items() if k in ("F", "He", "We", "S", "D", "r")) + ("-yaw" if kw.get("yaw_step") else "")


@pytest.mark.parametrize("kw", S.GPU_CASES, ids=_ids)
def test_ambiguous_pairs_are_rare_on_the_gpu_inputs(kw):
    c = S.cached_case(**kw)
    share = float(c.ambiguous.mean())
    print(f"{c.id}: ambiguous (pixel, hypothesis) pairs {share:.5f}")
    assert share <= S.MAX_AMBIGUOUS_SHARE, share
    assert share == 0.0                                   # on the arc path no point of a sphere comes near a source's centre


def test_gpu_cases_cover_what_they_are_meant_to():
    cases = [S.cached_case(**kw) for kw in S.GPU_CASES]
    assert {(c.F, c.H, c.W) for c in cases} == {(3, 20, 40), (2, 8, 16), (5, 48, 96)}
    assert {c.S for c in cases} == {1, 4} and {c.D for c in cases} == {2, 3, 32} and {c.r for c in cases} == {0, 2, 3}
    assert any((R.present(c.src_index, c.F).sum(1) == 0).any() for c in cases)          # a view without sources
    assert any(kw.get("absent") for kw in S.GPU_CASES)
    # cameras of different yaw: the source's seam (its direction -z) lies in the middle half of the reference panorama
    c = S.cached_case(**S.GPU_CASES[1])
    back = np.linalg.inv(S._four(c.rel_pose[0, :1].astype(np.float64)))[0, :3, :3] @ np.array([0, 0, -1.0])
    u, _, _ = S.dir_pixel(back[0], back[1], back[2], c.H, c.W)
    assert c.W / 4 < u < 3 * c.W / 4, u


def test_margin_constant_covers_the_measured_float32_error():
    """The largest |float32-order cost - float64 cost| over the GPU tests' inputs: the GPU tests allow twice the constant, which must
    therefore still cover what is measured here.  The largest differences sit where a point lands within a pixel of a source's pole:
    there asinf and atan2f turn an ulp of the point into 1e-3 px."""
    worst = 0.0
    for kw in S.GPU_CASES:
        c = S.cached_case(**kw)
        C32, _ = S.cost_volume(c.grey, c.rel_pose, c.src_index, c.inv_dist, c.r, np.float32)
        assert C32.dtype == np.float32
        d = np.abs(C32.astype(np.float64) - c.C64)[~c.ambiguous]
        worst = max(worst, float(d.max()))
        print(f"{c.id}: float32-order vs float64 cost, max {float(d.max()):.3e} grey levels")
    print(f"measured margin {worst:.3e}; constant {S.SPHERE_F32_MARGIN:.3e}; GPU tolerance {S.COST_TOL:.3e}")
    assert S.SPHERE_F32_MARGIN >= worst
    assert S.SPHERE_F32_MARGIN <= 2 * worst, "the constant has drifted far above the measurement: re-measure and lower it"
    assert S.COST_TOL == 2 * S.SPHERE_F32_MARGIN


# ------------------------------------------------------------------ the panorama cameras' poses
def _on_walls(pano_w2c, first_view_to_scene, dist, step):
    """share of the points lifted with pano_w2c (world = the first view's frame) and moved into the scene that lie within 1.5 hypothesis
    steps of a wall"""
    pts = S.unproject_ref(dist, np.linalg.inv(S._four(pano_w2c))[:, :3, :4])
    P = pts @ first_view_to_scene[:3, :3].T + first_view_to_scene[:3, 3]
    return float((R.pose_scene().wall_distance(P) <= 1.5 * step[:, None, None] * dist ** 2).mean())


def test_pano_poses_share_the_frame_and_the_centres_of_the_views():
    from evoworld_amd.geometry import xyz_euler_to_four_by_four_matrix_batch
    n = 5
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(POSE_CAM[:n]), relative=False).numpy()
    w2c = mvs.pano_poses(POSE_CAM, n, 0)
    assert w2c.shape == (n, 3, 4) and w2c.dtype == np.float64
    first = np.linalg.inv(S._four(mvs.view_poses(POSE_CAM, n, 0, relative=False)[:1]))[0]            # first view -> scene
    np.testing.assert_allclose(first[None] @ np.linalg.inv(S._four(w2c)), c2w, atol=1e-12)          # the panorama cameras, in that frame
    views = np.linalg.inv(S._four(mvs.view_poses(POSE_CAM, n, 0)))
    np.testing.assert_allclose(np.linalg.inv(S._four(w2c))[:, :3, 3], views[:, :3, 3], atol=1e-12)  # what align_extrinsics reads
    assert np.abs(w2c[0, :, :3] - np.eye(3)).max() > 0.1      # the first PANORAMA is not the origin's orientation: the first view is
    with pytest.raises(ValueError):
        mvs.pano_poses(POSE_CAM[:3], 5, 0)


def test_a_wrong_pose_convention_leaves_the_walls():
    """The criterion of the device's end-to-end test (tests/test_gpu_mvs_sphere.py), here on the TRUE distances of the pose scene's
    panoramas: lifted with pano_poses every point lies on a wall; with the yaw sign flipped, or with the panorama's frame mistaken for
    the view's, fewer than 90 % do -- so that test fails on either mistake."""
    from evoworld_amd.geometry import xyz_euler_to_four_by_four_matrix_batch
    n, He, We = 5, 128, 256
    scene = R.pose_scene()
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(POSE_CAM[:n]), relative=False).numpy()
    dist = S.true_distance(scene, np.linalg.inv(c2w)[:, :3, :4], He, We)
    good = mvs.pano_poses(POSE_CAM, n, 0)
    step = np.diff(mvs.sphere_setup(good, We, 4, 32).inv_dist, axis=1)[:, 0]
    first = np.linalg.inv(S._four(mvs.view_poses(POSE_CAM, n, 0, relative=False)[:1]))[0]
    assert _on_walls(good, first, dist, step) == 1.0
    flipped = POSE_CAM.copy()
    flipped[:, 4] = -flipped[:, 4]
    wrong_yaw = _on_walls(mvs.pano_poses(flipped, n, 0), first, dist, step)
    pano_frame = np.linalg.inv(np.linalg.inv(c2w[0])[None] @ c2w)[:, :3, :4]           # world = the first PANORAMA's frame
    mixed = _on_walls(pano_frame, first, dist, step)
    print(f"on the walls: yaw sign flipped {wrong_yaw:.3f}, panorama frame for view frame {mixed:.3f}")
    assert wrong_yaw < 0.9 and mixed < 0.9


# ------------------------------------------------------------------ wiring, CLI, loader
def test_depth_stage_dispatch_has_three_call_shapes():
    calls = []

    def plain(*a, **kw):
        calls.append((a, kw))
        return "plain"

    class Views:
        wants_view_poses = True

        def __call__(self, *a, **kw):
            calls.append((a, kw))
            return "views"

    class Panos:
        wants_panoramas = True

        def __call__(self, *a, **kw):
            calls.append((a, kw))
            return "panos"

    pers = torch.zeros(5, 4, 4, 3, dtype=torch.uint8)
    panos = torch.zeros(5, 8, 16, 3, dtype=torch.uint8)
    assert mvs.call_depth_model(plain, pers, POSE_CAM, 0, panos_u8=panos) == "plain"
    (a, kw), = calls
    assert len(a) == 1 and a[0] is pers and kw == {}                                  # one positional argument, as before
    calls.clear()
    assert mvs.call_depth_model(Views(), pers, POSE_CAM, 0, panos_u8=panos) == "views"
    (a, kw), = calls
    assert len(a) == 1 and a[0] is pers and list(kw) == ["view_w2c"]
    calls.clear()
    assert mvs.call_depth_model(Panos(), pers, POSE_CAM, 0, panos_u8=panos) == "panos"
    (a, kw), = calls
    assert len(a) == 1 and a[0] is panos and list(kw) == ["pano_w2c"]
    np.testing.assert_array_equal(kw["pano_w2c"], mvs.pano_poses(POSE_CAM, 5, 0))
    with pytest.raises(ValueError):
        mvs.call_depth_model(Panos(), pers, POSE_CAM, 0)                              # the panoramas are not optional for such a stage
    assert mvs.SphereSweepDepth.wants_panoramas is True and not getattr(mvs.SphereSweepDepth, "wants_view_poses", False)
    assert not getattr(mvs.PlaneSweepDepth, "wants_panoramas", False)
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    src = inspect.getsource(UnifiedLoopConsistencyPipeline.process_episode)
    assert "panos_u8=all_u8" in src and "self.depth_model(" not in src
    assert src.index("out.perspective(seg, pers)") < src.index("panos_u8=all_u8")     # the crops are still cut and dumped first


def test_cli_flag_loader_and_stage_arguments():
    import unified_loop_consistency as cli
    from evoworld_amd.stages import DEPTH_STAGES, SyntheticStages, load_stages
    assert DEPTH_STAGES == ("synthetic", "mvs", "mvs_pano")
    a = cli.parse_arguments(["--unet_path", "X"])
    assert a.depth_stage == "synthetic"
    b = cli.parse_arguments(["--unet_path", "X", "--depth_stage", "mvs_pano", "--mvs_planes", "48", "--mvs_sources", "2"])
    assert (b.depth_stage, b.mvs_planes, b.mvs_sources) == ("mvs_pano", 48, 2)
    m = load_stages(None, b, depth_stage="mvs_pano", camera_params=POSE_CAM)
    assert type(m) is SyntheticStages and isinstance(m.depth_model, mvs.SphereSweepDepth)
    assert (m.depth_model.planes, m.depth_model.n_src, m.depth_model.sweep_size) == (48, 2, None) and m.vae is not None
    np.testing.assert_array_equal(m.depth_model.camera_params, POSE_CAM)
    assert isinstance(load_stages(None, b, depth_stage="mvs", camera_params=POSE_CAM).depth_model, mvs.PlaneSweepDepth)
    st = load_stages(None, a, camera_params=POSE_CAM)
    assert st.depth_model.__func__ is SyntheticStages.depth_model
    p = mvs.build_parser().parse_args(["cloud", "--frames", "d", "--poses", "camera_poses.txt", "--output", "s.ply"])
    assert p.stage == "plane" and p.sweep_size is None
    p = mvs.build_parser().parse_args(["cloud", "--frames", "d", "--poses", "p", "--output", "s.ply", "--stage", "sphere", "--sweep_size", "64", "128"])
    assert p.stage == "sphere" and p.sweep_size == [64, 128]
    d = mvs.SphereSweepDepth()
    assert (d.n_src, d.planes, d.patch_radius, d.min_consistent, d.rel_tol, d.sweep_size) == (4, 64, 2, 2, 0.02, None)
    for bad in (dict(patch_radius=4), dict(n_src=0), dict(planes=0), dict(sweep_size=(0, 4))):
        with pytest.raises(ValueError):
            mvs.SphereSweepDepth(**bad)
    with pytest.raises(TypeError):
        d(torch.zeros(2, 8, 16, 3))                                                   # not uint8
    with pytest.raises(ValueError):
        mvs.SphereSweepDepth(POSE_CAM)._poses(7)                                      # 7 panoramas: no segment has that many


def test_header_declares_the_entries_and_the_build_keeps_their_operation_order():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "evoworld_hip.h")).read()
    for name in ("ew_mvs_sphere_sweep", "ew_mvs_sphere_consistency", "ew_pano_unproject"):
        assert f"ew_status {name}(" in header
    assert "#define EW_ABI_VERSION 20" in header
    make = open(os.path.join(root, "evoworld_amd", "csrc", "Makefile")).read()
    rule = make[make.index("mvs_sphere.o: mvs_sphere.hip"):]
    assert "-ffp-contract=off" in rule.split("\n")[1] and " mvs_sphere.o" in make.split("\n")[4]
