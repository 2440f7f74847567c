"""-m gpu: the sphere-sweep stereo stage on the device (csrc/mvs_sphere.hip, evoworld_amd/mvs.py) against the numpy oracle
of tests/mvs_sphere_ref.py.  Cost tolerance: mvs_sphere_ref.COST_TOL = twice the float32-order margin that tests/test_cpu_mvs_sphere.py
measures on these very inputs; no (pixel, hypothesis) pair of them is ambiguous (a point on a source's centre), which the CPU test asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvs_ref as R  # noqa: E402
import mvs_sphere_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = {torch.float32: -777.25, torch.int32: -777}
PAD = 4096


class Guarded:
    """`view` of the given shape in the middle of a buffer filled with a pattern; check() asserts the bands either side still hold it"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.buf = torch.full((PAD + n + PAD,), FILL[dtype], dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + n].view(shape)
        self.n, self.fill = n, FILL[dtype]

    def check(self):
        assert bool((self.buf[:PAD] == self.fill).all()), "guard band in front of the output was written"
        assert bool((self.buf[PAD + self.n:] == self.fill).all()), "guard band behind the output was written"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sweep(c, guarded=False):
    from evoworld_amd import ops
    shape = (c.F, c.H, c.W)
    g = [Guarded(shape, dt) for dt in (torch.float32, torch.float32, torch.int32, torch.float32)] if guarded else None
    out = ops.mvs_sphere_sweep(_dev(c.grey), _dev(c.rel_pose), _dev(c.src_index), _dev(c.inv_dist), c.r, out=[x.view for x in g] if g else None)
    torch.cuda.synchronize()
    for x in g or ():
        x.check()
    return [o.cpu().numpy() for o in out]


_ids = lambda kw: "-".join(f"{k}{v}" for k, v in kw.items() if k in ("F", "He", "We", "S", "D", "r")) + ("-yaw" if kw.get("yaw_step") else "")


# ------------------------------------------------------------------ ew_mvs_sphere_sweep against the oracle
@pytest.mark.parametrize("kw", S.GPU_CASES, ids=_ids)
def test_sphere_sweep_matches_the_float64_oracle(kw):
    """Every pixel, columns 0 and We - 1 and rows 0 and He - 1 like any other: the winner's cost, its regret, the refined distance and the
    confidence against the float64 cost volume, within COST_TOL carried through the rules."""
    c = S.cached_case(**kw)
    tol = S.COST_TOL
    dist, conf, win, cost = _sweep(c, guarded=True)
    again = _sweep(c)
    for a, b in zip((dist, conf, win, cost), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ"
    assert float(c.ambiguous.mean()) <= S.MAX_AMBIGUOUS_SHARE
    assert win.min() >= 0 and win.max() < c.D
    n_present = R.present(c.src_index, c.F).sum(1)
    inv32 = c.inv_dist
    worst_cost = worst_regret = 0.0
    for f in range(c.F):
        C, amb, k = c.C64[f], c.ambiguous[f], win[f].astype(np.int64)
        if n_present[f] == 0:                             # no source: every cost 0, hypothesis 0, no confidence
            assert (k == 0).all() and (cost[f] == 0).all() and (conf[f] == 0).all()
            assert np.array_equal(dist[f], np.full_like(dist[f], np.float32(1) / inv32[f, 0]))
            continue
        at = lambda A, kk: np.take_along_axis(A, kk[None], 0)[0]
        clear = ~at(amb, k)
        d_cost = np.abs(cost[f].astype(np.float64) - at(C, k))[clear]
        regret = (at(C, k) - np.where(amb, np.inf, C).min(0))[clear]
        worst_cost, worst_regret = max(worst_cost, float(d_cost.max())), max(worst_regret, float(regret.max()))
        print(f"{c.id} view {f}: winner cost within {d_cost.max():.3e}, regret {regret.max():.3e} (tolerance {tol:.1e})")
        assert d_cost.max() <= tol, f"view {f}: winner cost off by {d_cost.max():.3e} (tolerance {tol:.1e})"
        assert regret.max() <= tol, f"view {f}: the device's winner costs {regret.max():.3e} more than the best hypothesis (tolerance {tol:.1e})"
        # distance: the parabola rule on the float64 costs around the device's winner, the tolerance carried through the rule
        inner = (k > 0) & (k < c.D - 1)
        clear3 = clear & ~at(amb, np.maximum(k - 1, 0)) & ~at(amb, np.minimum(k + 1, c.D - 1))
        off, _, curv = R.parabola_offset(C, k)
        num = np.abs(at(C, np.maximum(k - 1, 0)) - at(C, np.minimum(k + 1, c.D - 1)))
        inv_dev = 1.0 / dist[f].astype(np.float64)
        base = inv32[f].astype(np.float64)[k]
        step = float(np.abs(np.diff(inv32[f].astype(np.float64))).max()) if c.D > 1 else 0.0
        exact = ~inner | (curv < -4 * tol)                # the rule gives no refinement, whatever the last bits of the costs
        assert np.array_equal(dist[f][exact & clear3], (np.float32(1) / inv32[f][k])[exact & clear3])
        sure = inner & (curv > 4 * tol) & clear3          # refined on both sides: |d off| <= (tol curv + 2 tol |cl - cr|) / (curv (curv - 4 tol))
        with np.errstate(all="ignore"):
            d_off = np.where(sure, (tol * curv + 2 * tol * num) / (curv * (curv - 4 * tol)), 0.0) + 1e-5
        want = base + off * np.sign(np.diff(inv32[f].astype(np.float64)).mean() if c.D > 1 else 1.0) * step
        assert (np.abs(inv_dev - want)[sure] <= (d_off * step + 4e-6 * base)[sure]).all(), f"view {f}: refined distance"
        unsure = inner & ~sure & ~exact & clear3          # convexity hangs on the last bits: anywhere within half a step
        assert (np.abs(inv_dev - base)[unsure] <= 0.5 * step * (1 + 1e-5) + 4e-6 * base[unsure]).all()
        # confidence: 0 exactly where the rules say 0; elsewhere the rule's value
        far = np.abs(np.arange(c.D)[:, None, None] - k[None]) > 1
        none = ~far.any(0)
        assert (conf[f][none] == 0).all()
        c64, has = R.confidence_ref(C, k, n_present[f])
        c2 = np.where(far, C, np.inf).min(0)
        ok = has & ~amb.any(0) & (c2 > 1.0)
        assert (np.abs(conf[f] - c64)[ok] <= (3 * tol / c2 + 1e-5)[ok]).all(), f"view {f}: confidence"
        assert (conf[f] >= 0).all() and (conf[f] <= 1).all()
    print(f"{c.id}: winner cost within {worst_cost:.3e}, regret {worst_regret:.3e} (tolerance {tol:.1e})")


@pytest.mark.parametrize("view", [0, 2, 4])
def test_a_view_does_not_depend_on_the_rest_of_the_batch(view):
    """View i of the F = 5 call against a call that holds only it and its sources: bit-identical."""
    c = S.cached_case(**S.RECOVERY_CASE)
    full = _sweep(c)
    srcs = [int(s) for s in c.src_index[view] if s >= 0]
    sub = [view] + srcs
    one = S.SimpleNamespace(F=len(sub), H=c.H, W=c.W, r=c.r, grey=c.grey[sub], rel_pose=c.rel_pose[sub].copy(), inv_dist=c.inv_dist[sub].copy(),
                            src_index=np.full((len(sub), c.S), -1, np.int32))
    remap = {v: i for i, v in enumerate(sub)}
    one.src_index[0] = [remap.get(int(s), -1) for s in c.src_index[view]]
    alone = _sweep(one)
    for a, b, name in zip(full, alone, ("dist", "conf", "winner", "cost")):
        assert np.array_equal(a[view].view(np.int32), b[0].view(np.int32)), name


def test_argument_checks_of_the_wrappers_and_of_the_entry():
    from evoworld_amd import _lib, ops
    c = S.cached_case(**S.GPU_CASES[4])                    # 8 x 16
    g, pose, src, inv = _dev(c.grey), _dev(c.rel_pose), _dev(c.src_index), _dev(c.inv_dist)
    with pytest.raises(ValueError):
        ops.mvs_sphere_sweep(g[:, :, :5].contiguous(), pose, src, inv, 3)              # We = 5 < 2 x 3 + 1
    with pytest.raises(ValueError):
        ops.mvs_sphere_sweep(g, pose, src, inv, 4)
    with pytest.raises(ValueError):
        ops.mvs_sphere_sweep(g, pose[:, :, :2].contiguous(), src, inv, 1)
    with pytest.raises(TypeError):
        ops.mvs_sphere_sweep(g.float(), pose, src, inv, 1)
    with pytest.raises(ValueError):
        ops.mvs_sphere_sweep(g, pose, src, inv, 1, out=[torch.empty(1, device=DEV)] * 4)
    out = [torch.empty(c.F, c.H, 5, dtype=dt, device=DEV) for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]
    with pytest.raises(_lib.EvoWorldHipError):             # the entry's own check, behind the wrapper's
        ops._call("ew_mvs_sphere_sweep", ops._ptr(g), ops._ptr(pose), ops._ptr(src), ops._ptr(inv), *[ops._ptr(o) for o in out], c.F, c.H, 5,
                  c.S, c.D, 3)
    d = torch.ones(c.F, c.H, c.W, device=DEV)
    with pytest.raises(ValueError):
        ops.mvs_sphere_consistency(d, pose, src, torch.ones(c.F, c.H, c.W + 1, device=DEV))
    with pytest.raises(ValueError):
        ops.mvs_sphere_consistency(d, pose, src, d.clone(), rel_tol=-1.0)
    with pytest.raises(ValueError):
        ops.pano_unproject(d, torch.zeros(c.F, 4, 4, device=DEV))
    with pytest.raises(_lib.EvoWorldHipError):
        ops.pano_unproject(d.cpu(), torch.zeros(c.F, 3, 4))


# ------------------------------------------------------------------ ew_mvs_sphere_consistency
@pytest.fixture(scope="module")
def true_maps():
    """3 panoramas of 20 x 40 of the pose scene with their true distance maps, cameras turned against each other"""
    from evoworld_amd import mvs
    w2c = S.turned(R.arc_path(3, radius=7.0, centre=(0.5, 0.0, 4.0)), 130.0)
    dist = S.true_distance(R.pose_scene(), w2c, 20, 40).astype(np.float32)
    return dist, mvs.sphere_setup(w2c, 40, 2, 4)


def _consistency(dist, st, src, rel_tol, need, rel_pose=None):
    from evoworld_amd import ops
    pose = st.rel_pose_f32 if rel_pose is None else rel_pose
    g = Guarded(dist.shape, torch.float32)
    g.view.fill_(1.0)
    out = ops.mvs_sphere_consistency(_dev(dist), _dev(pose), _dev(src), g.view, rel_tol, need)
    torch.cuda.synchronize()
    assert out is g.view                                  # in place
    g.check()
    want, agree, border = S.consistency_ref(dist, pose, src, np.ones(dist.shape, np.float32), rel_tol, need)
    return g.view.cpu().numpy(), want, agree, border


def test_consistency_keeps_agreeing_pixels_and_drops_what_the_oracle_drops(true_maps):
    dist, st = true_maps
    got, want, agree, border = _consistency(dist, st, st.src_index, 0.02, 2)
    print(f"borderline share {border.mean():.4f}; kept {float((want == 1).mean()):.3f}")
    assert border.mean() <= 0.02
    assert np.array_equal(got[~border], want[~border]) and set(np.unique(got)) <= {0.0, 1.0}
    # agreeing pixels are kept; both verdicts are well represented (at 20 x 40 a neighbouring pixel of an oblique wall is often more than
    # 2 % nearer or farther, so many pixels fail with the true distances too: a property of the input, counted by the oracle)
    assert (got[(agree >= 2) & ~border] == 1).all() and 0.25 < (agree >= 2).mean() < 0.75
    bad = dist.copy()
    bad[1] *= np.float32(1.06)                            # one source beyond rel_tol: exactly the oracle's pixels go
    got2, want2, agree2, border2 = _consistency(bad, st, st.src_index, 0.02, 2)
    assert border2.mean() <= 0.02
    assert np.array_equal(got2[~border2], want2[~border2])
    assert (want2 == 0).sum() > (want == 0).sum()


def test_consistency_does_not_count_absent_sources(true_maps):
    dist, st = true_maps
    src = st.src_index.copy()
    src[:, 1] = -1
    pose = st.rel_pose_f32.copy()
    pose[:, 1] = np.nan                                   # an absent slot's pose is never read
    got, want, agree, border = _consistency(dist, st, src, 0.02, 2, pose)
    assert (got == 0).all() and (want == 0).all()         # one source present: two can never agree
    got, want, agree, border = _consistency(dist, st, src, 0.02, 1, pose)
    assert np.array_equal(got[~border], want[~border]) and agree.max() == 1 and (got == 1).mean() > 0.5
    src[:] = 7                                            # an index outside [0, F) is absent too
    got, _, _, _ = _consistency(dist, st, src, 0.02, 1, pose)
    assert (got == 0).all()


# ------------------------------------------------------------------ ew_pano_unproject
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 7, 13), (2, 48, 96), (1, 130, 517)])
def test_pano_unproject_is_the_spherical_lift(shape):
    """Against float64 within 16 x 2^-23 x (dist + max |t|) per coordinate: the direction's two angles, three sines and cosines, the
    products and the three sums of a row each add an ulp or two of a quantity no larger than dist + |t|."""
    from evoworld_amd import ops
    F, He, We = shape
    rng = np.random.default_rng(He)
    dist = rng.uniform(0.3, 40.0, shape).astype(np.float32)
    c2w = np.linalg.inv(S._four(S.turned(R.arc_path(max(F, 2)), 130.0)))[:F, :3, :4].astype(np.float32)
    g = Guarded((F, He, We, 3), torch.float32)
    got = ops.pano_unproject(_dev(dist), _dev(c2w), out=g.view)
    torch.cuda.synchronize()
    g.check()
    again = ops.pano_unproject(_dev(dist), _dev(c2w))
    assert torch.equal(got, again)
    want = S.unproject_ref(dist, c2w)
    bound = 16 * 2.0 ** -23 * (dist.astype(np.float64) + np.abs(c2w[:, :, 3]).max())[..., None]
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"{shape}: worst error {float((err / bound).max()):.3f} of the bound")
    assert (err <= bound).all()


# ------------------------------------------------------------------ recovery and the pose convention
def test_device_recovers_the_box_scene():
    """The CPU test's scene through the whole stage on the device: >= 90 % of the kept pixels within 1.5 hypothesis steps (the float64
    oracle is held to 95 % by tests/test_cpu_mvs_sphere.py)."""
    from evoworld_amd import mvs
    c = S.cached_case(**S.RECOVERY_CASE)
    stage = mvs.SphereSweepDepth(n_src=c.S, planes=c.D, patch_radius=c.r)
    rgb = _dev(np.repeat(c.grey[..., None], 3, -1))
    preds = stage(rgb, pano_w2c=c.w2c)
    assert set(preds) == {"world_points_from_depth", "depth_conf", "depth", "images", "extrinsic"}
    assert preds["depth"].shape == (c.F, c.H, c.W, 1) and preds["depth_conf"].shape == (c.F, c.H, c.W) and preds["depth"].is_cuda
    assert preds["world_points_from_depth"].shape == (c.F, c.H, c.W, 3) and preds["extrinsic"].shape == (c.F, 3, 4)
    assert torch.equal(preds["images"], rgb.permute(0, 3, 1, 2).float() / 255)
    dist = preds["depth"][..., 0].cpu().numpy().astype(np.float64)
    step = np.diff(c.setup.inv_dist, axis=1)[:, 0]
    share, n = R.kept_and_correct(preds["depth_conf"].cpu().numpy(), dist, c.true_dist, step)
    print(f"device recovery: {share:.4f} of {n} kept pixels within 1.5 hypothesis steps")
    assert share >= 0.90, share
    # the lift: the points are the distances along the pixels' directions, in the frame pano_w2c is given in
    want = S.unproject_ref(dist, np.linalg.inv(S._four(c.w2c))[:, :3, :4])
    np.testing.assert_allclose(preds["world_points_from_depth"].cpu().numpy(), want, atol=1e-3)


def test_pose_convention_end_to_end():
    """Panoramas of the pose scene at the episode's cameras -> SphereSweepDepth with the poses from camera_params: the kept points, moved
    from the first view's frame into the scene, lie on the box's walls -- a wrong yaw sign or a panorama-vs-view frame mix-up fails
    (tests/test_cpu_mvs_sphere.py shows that either does) --, and the same episode through PlaneSweepDepth puts its kept points on the
    same walls by the same transform: one frame for both clouds."""
    from evoworld_amd import mvs, reprojection as RP
    from evoworld_amd.geometry import xyz_euler_to_four_by_four_matrix_batch
    scene, cam, n = R.pose_scene(), R.POSE_CAM, 5
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(cam[:n]), relative=False).numpy()
    panos = _dev(scene.render_panos(c2w, 128, 256))
    first = np.linalg.inv(S._four(mvs.view_poses(cam, n, 0, relative=False)[:1]))[0]   # first view -> scene
    stage = mvs.SphereSweepDepth(cam, n_src=4, planes=32, patch_radius=2, sweep_size=None, segment_id=0)
    preds = stage(panos)                                  # the poses from camera_params, as a user's direct call gets them
    np.testing.assert_allclose(preds["extrinsic"].cpu().numpy(), mvs.pano_poses(cam, n, 0), atol=1e-6)
    P = preds["world_points_from_depth"].cpu().numpy().astype(np.float64) @ first[:3, :3].T + first[:3, 3]
    d = preds["depth"][..., 0].cpu().numpy().astype(np.float64)
    conf = preds["depth_conf"].cpu().numpy()
    step = np.diff(stage.last_setup.inv_dist, axis=1)[:, 0]
    keep = conf >= np.percentile(conf, 50.0)
    on_wall = scene.wall_distance(P) <= 1.5 * step[:, None, None] * d ** 2              # 1.5 hypothesis steps, as a distance at range d
    print(f"sphere: kept points within 1.5 hypothesis steps of a wall: {on_wall[keep].mean():.4f} of {int(keep.sum())}")
    assert on_wall[keep].mean() >= 0.90
    views = RP.Equi2Pers(height=48, width=64, fov_x=90.0, mode="bilinear").batch(
        panos, [{"pitch": 0, "roll": 0, "yaw": float(y)} for y in RP.calculate_target_yaws(cam, n, 0)])
    plane = mvs.PlaneSweepDepth(cam, n_src=4, planes=32, patch_radius=2, segment_id=0)
    pp = plane(views)
    pts = RP.depth_to_world_points(pp["depth"], pp["extrinsic"], pp["intrinsic"]).cpu().numpy().astype(np.float64)
    Q = pts @ first[:3, :3].T + first[:3, 3]
    z = pp["depth"][..., 0].cpu().numpy().astype(np.float64)
    pconf = pp["depth_conf"].cpu().numpy()
    pstep = np.diff(plane.last_setup.inv_depth, axis=1)[:, 0]
    pkeep = pconf >= np.percentile(pconf, 50.0)
    p_on = scene.wall_distance(Q) <= 1.5 * pstep[:, None, None] * z ** 2
    print(f"plane: kept points within 1.5 plane steps of a wall: {p_on[pkeep].mean():.4f} of {int(pkeep.sum())}")
    assert p_on[pkeep].mean() >= 0.90
    # the camera centres SceneBuilder.align_extrinsics reads are the same for both stages
    centre = lambda e: np.linalg.inv(S._four(e.cpu().numpy()))[:, :3, 3]
    np.testing.assert_allclose(centre(preds["extrinsic"]), centre(pp["extrinsic"]), atol=1e-5)


def test_cloud_cli_sphere_stage_writes_a_readable_cloud_on_the_walls(tmp_path, capsys):
    """python -m evoworld_amd.mvs cloud --stage sphere, in process: panorama files + camera_poses.txt -> sphere-sweep depth -> the
    filtered cloud as a PLY in the first view's frame; its points lie on the box's walls.  --sweep_size resizes first."""
    import json
    from PIL import Image
    from evoworld_amd import mvs
    from evoworld_amd.geometry import UNITY_TO_OPENCV, xyz_euler_to_four_by_four_matrix_batch
    from evoworld_amd.memory import read_ply
    scene, cam, n = R.pose_scene(), R.POSE_CAM, 5
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(cam[:n]), relative=False).numpy()
    (tmp_path / "frames").mkdir()
    for i, p in enumerate(scene.render_panos(c2w, 128, 256)):
        Image.fromarray(p).save(tmp_path / "frames" / f"{i + 1:03}.png")
    with open(tmp_path / "camera_poses.txt", "w") as f:
        f.write("Frame,PosX,PosY,PosZ,RotX,RotY,RotZ\n")
        for i, row in enumerate(cam * np.asarray(UNITY_TO_OPENCV, np.float64)):
            f.write(",".join([str(i + 1)] + [repr(float(v)) for v in row]) + "\n")
    out = tmp_path / "scene.ply"
    base = ["cloud", "--frames", str(tmp_path / "frames"), "--poses", str(tmp_path / "camera_poses.txt"), "--segment", "0", "--planes", "32",
            "--stage", "sphere"]
    mvs.main(base + ["--output", str(out)])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    pts, rgb = read_ply(str(out))
    assert rec["stage"] == "sphere" and rec["views"] == 5 and rec["points_in"] == rec["points_out"] == len(pts)
    assert 5 * 128 * 256 // 2 <= len(pts) < 5 * 128 * 256
    first = np.linalg.inv(S._four(mvs.view_poses(cam, n, 0, relative=False)[:1]))[0]
    P = pts.astype(np.float64) @ first[:3, :3].T + first[:3, 3]
    st = mvs.sphere_setup(mvs.pano_poses(cam, n, 0), 256, 4, 32)
    rng = np.linalg.norm(P - first[:3, 3], axis=1)                                     # the point's distance from the first camera ...
    reach = rng + np.linalg.norm(np.linalg.inv(S._four(mvs.pano_poses(cam, n, 0)))[:, :3, 3], axis=1).max()   # ... bounds it from any camera
    share = float((scene.wall_distance(P) <= 1.5 * np.diff(st.inv_dist, axis=1).max() * reach ** 2).mean())
    print(f"cloud CLI --stage sphere: {len(pts)} points, {share:.4f} within 1.5 hypothesis steps of a wall")
    assert share >= 0.90 and (rgb[:, 0] == rgb[:, 1]).all()
    small = tmp_path / "small.ply"
    mvs.main(base + ["--output", str(small), "--sweep_size", "64", "128"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    # half of the resized panoramas' pixels or more (all of them when the check zeroes over half the confidences: the percentile is 0)
    assert 5 * 64 * 128 // 2 <= rec["points_out"] == len(read_ply(str(small))[0]) <= 5 * 64 * 128


# ------------------------------------------------------------------ the episode
@pytest.fixture(scope="module")
def tiny():
    from evoworld_amd.pipeline import StableVideoDiffusionPipeline
    from evoworld_amd.unet import DEFAULT_CONFIG, UNetSpatioTemporalConditionModel, random_state_dict
    from oracle.unet_ref import tiny_config
    cfg = tiny_config()
    cfg["num_frames"] = 25
    sd = random_state_dict({**DEFAULT_CONFIG, **cfg}, 0)
    unet = UNetSpatioTemporalConditionModel(**cfg).load_state_dict(sd, device="cuda")
    return cfg, StableVideoDiffusionPipeline(unet=unet)


def test_episode_with_the_sphere_stage_and_the_other_stages_untouched(tiny, tmp_path):
    """The tiny 2-segment synthetic episode: default loader and depth_stage='mvs', then depth_stage='mvs_pano', then the first two again
    in the same process.  The mvs_pano run goes through, renders other memory panoramas than the stand-in's and fills directions the mvs
    stage leaves black; the runs either side of it are bit-identical, frames and panoramas, and the dumped crops do not change."""
    from types import SimpleNamespace
    from PIL import Image
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.mvs import PlaneSweepDepth, SphereSweepDepth
    from evoworld_amd.stages import load_stages
    cfg, pipe = tiny
    H, W, T = 128, 256, 25
    i = np.arange(60, dtype=np.float64)
    cam = np.stack([0.04 * i * np.sin(i / 9), 0 * i, 0.04 * i * np.cos(i / 9), 0 * i, 95 + 3.6 * i, 0 * i], 1)
    args = SimpleNamespace(svd_path=None, mvs_planes=16, mvs_sources=2)
    start = (torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    saved = (pipe.vae, pipe.image_encoder, pipe.vae_scale_factor)

    def pngs(d, n, fmt):
        return np.stack([np.asarray(Image.open(d / fmt.format(k))) for k in range(n)])

    def run(name, depth_stage):
        st = load_stages(None, args, depth_stage=depth_stage, cross_attention_dim=cfg["cross_attention_dim"], camera_params=cam, depth_hw=(48, 64))
        assert isinstance(st.depth_model, SphereSweepDepth) == (depth_stage == "mvs_pano")
        assert isinstance(st.depth_model, PlaneSweepDepth) == (depth_stage == "mvs")
        pipe.set_components(vae=st.vae, image_encoder=st.image_encoder)
        loop = UnifiedLoopConsistencyPipeline(pipe, st.depth_model, height=H, width=W, num_frames=T, num_segments=2, num_inference_steps=1,
                                              pano_size=(64, 128), face_res=32)
        frames = loop.process_episode(start, cam, save_dir=str(tmp_path / name), save_segment_frames=True)
        crops = sorted(os.listdir(tmp_path / name / "perspective_look_at_center_0"))
        return frames, pngs(tmp_path / name / "rendered_panorama_vggt_open3d_0", 24, "{:02}.png"), \
            [np.asarray(Image.open(tmp_path / name / "perspective_look_at_center_0" / f)) for f in crops]

    try:
        f0, p0, c0 = run("default_before", None)
        f1, p1, c1 = run("mvs_before", "mvs")
        f2, p2, c2 = run("mvs_pano", "mvs_pano")
        f3, p3, c3 = run("default_after", None)
        f4, p4, c4 = run("mvs_after", "mvs")
    finally:
        pipe.vae, pipe.image_encoder, pipe.vae_scale_factor = saved
    assert f2.shape == (49, 3, H, W) and torch.isfinite(f2).all()
    assert not np.array_equal(p2, p0), "the memory panoramas of the mvs_pano run equal the stand-in's"
    assert not np.array_equal(p2, p1), "the memory panoramas of the mvs_pano run equal the mvs stage's"
    lit = lambda p: (p != 0).any(-1)
    new = lit(p2) & ~lit(p1)                               # directions the plane sweep's forward cone leaves black
    print(f"non-black memory pixels: stand-in {int(lit(p0).sum())}, mvs {int(lit(p1).sum())}, mvs_pano {int(lit(p2).sum())}, "
          f"of which where mvs is black {int(new.sum())}")
    # the plane sweep lifts a 90-degree cone per view, so its memory panoramas stay black outside what that cloud covers; the sphere sweep's
    # cloud surrounds every camera, and a target pose on the path then sees a point in nearly every direction: it must fill most of the
    # pixels the plane sweep leaves black (half is asked), and those must be many (a tenth of all pixels)
    assert lit(p1).sum() > 0 and (~lit(p1)).sum() > 0.1 * lit(p1).size
    assert new.sum() > 0.5 * (~lit(p1)).sum()
    assert torch.equal(f0, f3) and np.array_equal(p0, p3) and torch.equal(f1, f4) and np.array_equal(p1, p4)
    assert len(c0) == len(c2) == 25 and all(np.array_equal(a, b) for a, b in zip(c0, c3))
    # segment 0 is generated before any depth stage runs: the crops cut from it are the same files whatever the stage
    assert all(np.array_equal(a, b) for a, b in zip(c0, c2)) and all(np.array_equal(a, b) for a, b in zip(c0, c1))
