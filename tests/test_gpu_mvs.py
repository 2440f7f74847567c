"""-m gpu: the plane-sweep stereo stage on the device (csrc/mvs.hip, evoworld_amd/mvs.py) against the numpy oracle of
tests/mvs_ref.py.  Cost tolerance: mvs_ref.COST_TOL = twice the float32-order margin that tests/test_cpu_mvs.py measures on these very
inputs; (pixel, plane) pairs whose window holds a tap that may fall on either side of a source's border are left out (at most 0.5 %)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvs_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = {torch.float32: -777.25, torch.int32: -777, torch.uint8: 0xA5}
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
    out = ops.mvs_plane_sweep(_dev(c.grey), _dev(c.homographies), _dev(c.src_index), _dev(c.inv_depth), c.r, c.oob,
                              out=[x.view for x in g] if g else None)
    torch.cuda.synchronize()
    for x in g or ():
        x.check()
    return [o.cpu().numpy() for o in out]


# ------------------------------------------------------------------ ew_mvs_luma_u8
@pytest.mark.parametrize("W", [1, 7, 130])
def test_luma_is_exact_on_every_level(W):
    from evoworld_amd import ops
    rng = np.random.default_rng(W)
    H = -(-768 // W) + 1
    rgb = rng.integers(0, 256, size=(2, H * W, 3), dtype=np.uint8)
    for ch in range(3):                                   # every level of every channel, in both frames
        rgb[:, ch * 256:(ch + 1) * 256, ch] = np.arange(256, dtype=np.uint8)
    rgb[1, :768, :] = rgb[1, :768, ::-1]
    rgb = rgb.reshape(2, H, W, 3)
    g = Guarded((2, H, W), torch.uint8)
    got = ops.mvs_luma(_dev(rgb), out=g.view)
    torch.cuda.synchronize()
    g.check()
    assert np.array_equal(got.cpu().numpy(), R.luma_ref(rgb))
    flat = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None, None], 3, -1)      # R = G = B = v -> v
    assert np.array_equal(ops.mvs_luma(_dev(flat)).cpu().numpy()[0, :, 0], np.arange(256))


# ------------------------------------------------------------------ ew_mvs_plane_sweep against the oracle
@pytest.mark.parametrize("kw", R.GPU_CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items() if k in "FHWSDr") + ("-out" if kw.get("push_out") else ""))
def test_plane_sweep_matches_the_float64_oracle(kw):
    c = R.cached_case(**kw)
    tol = R.COST_TOL
    depth, conf, win, cost = _sweep(c, guarded=True)
    again = _sweep(c)
    for a, b in zip((depth, conf, win, cost), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ"
    assert float(c.ambiguous.mean()) <= R.MAX_AMBIGUOUS_SHARE
    assert win.min() >= 0 and win.max() < c.D
    n_present = R.present(c.src_index, c.F).sum(1)
    inv32 = c.inv_depth
    worst_cost = worst_regret = 0.0
    for f in range(c.F):
        C, amb, k = c.C64[f], c.ambiguous[f], win[f].astype(np.int64)
        if n_present[f] == 0:                             # no source: every cost 0, plane 0, no confidence
            assert (k == 0).all() and (cost[f] == 0).all() and (conf[f] == 0).all()
            assert np.array_equal(depth[f], np.full_like(depth[f], np.float32(1) / inv32[f, 0]))
            continue
        at = lambda A, kk: np.take_along_axis(A, kk[None], 0)[0]
        clear = ~at(amb, k)
        d_cost = np.abs(cost[f].astype(np.float64) - at(C, k))[clear]
        regret = (at(C, k) - np.where(amb, np.inf, C).min(0))[clear]
        worst_cost, worst_regret = max(worst_cost, float(d_cost.max())), max(worst_regret, float(regret.max()))
        assert d_cost.max() <= tol, f"view {f}: winner cost off by {d_cost.max():.3e} (tolerance {tol:.1e})"
        assert regret.max() <= tol, f"view {f}: the device's winner costs {regret.max():.3e} more than the best plane (tolerance {tol:.1e})"
        # depth: the parabola rule on the float64 costs around the device's winner, the tolerance carried through the rule
        inner = (k > 0) & (k < c.D - 1)
        clear3 = clear & ~at(amb, np.maximum(k - 1, 0)) & ~at(amb, np.minimum(k + 1, c.D - 1))
        off, _, curv = R.parabola_offset(C, k)
        num = np.abs(at(C, np.maximum(k - 1, 0)) - at(C, np.minimum(k + 1, c.D - 1)))
        inv_dev = 1.0 / depth[f].astype(np.float64)
        base = inv32[f].astype(np.float64)[k]
        step = float(np.abs(np.diff(inv32[f].astype(np.float64))).max()) if c.D > 1 else 0.0
        exact = ~inner | (curv < -4 * tol)                # the rule gives no refinement, whatever the last bits of the costs
        assert np.array_equal(depth[f][exact & clear3], (np.float32(1) / inv32[f][k])[exact & clear3])
        sure = inner & (curv > 4 * tol) & clear3          # refined on both sides: |d off| <= (tol curv + 2 tol |cl - cr|) / (curv (curv - 4 tol))
        with np.errstate(all="ignore"):
            d_off = np.where(sure, (tol * curv + 2 * tol * num) / (curv * (curv - 4 * tol)), 0.0) + 1e-5
        want = base + off * np.sign(np.diff(inv32[f].astype(np.float64)).mean() if c.D > 1 else 1.0) * step
        assert (np.abs(inv_dev - want)[sure] <= (d_off * step + 4e-6 * base)[sure]).all(), f"view {f}: refined depth"
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
    print(f"{c.id}: winner cost within {worst_cost:.3e}, regret {worst_regret:.3e} (tolerance {tol:.1e}); "
          f"ambiguous pairs left out {float(c.ambiguous.mean()):.5f}")


@pytest.mark.parametrize("view", [0, 2, 4])
def test_a_view_does_not_depend_on_the_rest_of_the_batch(view):
    """View i of the F = 5 call against a call that holds only it and its sources: bit-identical."""
    c = R.cached_case(**R.RECOVERY_CASE)
    full = _sweep(c)
    srcs = [int(s) for s in c.src_index[view] if s >= 0]
    sub = [view] + srcs
    one = R.SimpleNamespace(F=len(sub), H=c.H, W=c.W, r=c.r, oob=c.oob, grey=c.grey[sub], homographies=c.homographies[sub].copy(),
                            inv_depth=c.inv_depth[sub].copy(), src_index=np.full((len(sub), c.S), -1, np.int32))
    remap = {v: i for i, v in enumerate(sub)}
    one.src_index[0] = [remap.get(int(s), -1) for s in c.src_index[view]]
    alone = _sweep(one)
    for a, b, name in zip(full, alone, ("depth", "conf", "winner", "cost")):
        assert np.array_equal(a[view].view(np.int32), b[0].view(np.int32)), name


# ------------------------------------------------------------------ ew_mvs_consistency
@pytest.fixture(scope="module")
def hand_made():
    """3 views of 16 x 24: the true depth maps of the pose scene's wall (nearly fronto-parallel, so neighbouring pixels agree within rel_tol)"""
    from evoworld_amd import mvs
    K = mvs.pinhole(16, 24)
    w2c = R.arc_path(3, radius=7.0, centre=(0.5, 0.0, 4.0))
    _, depth, _, _ = R.pose_scene().render_views(w2c, K, 16, 24)
    st = mvs.sweep_setup(w2c, K, 2, 4)
    return K, depth.astype(np.float32), st


def _consistency(depth, st, src, K, rel_tol, need, rel_pose=None):
    from evoworld_amd import ops
    conf = torch.ones(depth.shape, device=DEV)
    out = ops.mvs_consistency(_dev(depth), _dev(st.rel_pose_f32 if rel_pose is None else rel_pose), _dev(src), conf, K[0, 0], K[1, 1], K[0, 2],
                              K[1, 2], rel_tol, need)
    assert out is conf                                    # in place
    want, agree, border = R.consistency_ref(depth, st.rel_pose_f32 if rel_pose is None else rel_pose, src, np.ones(depth.shape, np.float32),
                                            K[0, 0], K[1, 1], K[0, 2], K[1, 2], rel_tol, need)
    return conf.cpu().numpy(), want, agree, border


def test_consistency_keeps_agreeing_pixels_and_drops_what_the_oracle_drops(hand_made):
    K, depth, st = hand_made
    got, want, agree, border = _consistency(depth, st, st.src_index, K, 0.02, 2)
    assert border.mean() <= 0.02
    assert np.array_equal(got[~border], want[~border]) and set(np.unique(got)) <= {0.0, 1.0}
    assert (got[(agree >= 2) & ~border] == 1).all() and (agree >= 2).mean() > 0.5       # agreeing pixels are kept, and there are many
    bad = depth.copy()
    bad[1] *= np.float32(1.06)                            # one source beyond rel_tol: exactly the oracle's pixels go
    got2, want2, agree2, border2 = _consistency(bad, st, st.src_index, K, 0.02, 2)
    assert border2.mean() <= 0.02
    assert np.array_equal(got2[~border2], want2[~border2])
    assert (want2 == 0).sum() > (want == 0).sum() and (got2[[0, 2]][(agree[[0, 2]] >= 2) & ~border2[[0, 2]] & ~border[[0, 2]]] == 0).all()


def test_consistency_does_not_count_absent_sources(hand_made):
    K, depth, st = hand_made
    src = st.src_index.copy()
    src[:, 1] = -1
    pose = st.rel_pose_f32.copy()
    pose[:, 1] = np.nan                                   # an absent slot's pose is never read
    got, want, agree, border = _consistency(depth, st, src, K, 0.02, 2, pose)
    assert (got == 0).all() and (want == 0).all()         # one source present: two can never agree
    got, want, agree, border = _consistency(depth, st, src, K, 0.02, 1, pose)
    assert np.array_equal(got[~border], want[~border]) and agree.max() == 1 and (got == 1).mean() > 0.5
    src[:] = 7                                            # an index outside [0, F) is absent too
    got, _, _, _ = _consistency(depth, st, src, K, 0.02, 1, pose)
    assert (got == 0).all()


# ------------------------------------------------------------------ recovery and the pose convention
def test_device_recovers_the_box_scene():
    """The CPU test's scene through the whole stage on the device: >= 90 % of the kept pixels within 1.5 plane steps (the float64
    oracle is held to 95 % by tests/test_cpu_mvs.py)."""
    from evoworld_amd import mvs
    c = R.cached_case(**R.RECOVERY_CASE)
    stage = mvs.PlaneSweepDepth(n_src=c.S, planes=c.D, patch_radius=c.r, oob_cost=c.oob)
    rgb = _dev(np.repeat(c.grey[..., None], 3, -1))
    preds = stage(rgb, view_w2c=c.w2c)
    assert preds["depth"].shape == (c.F, c.H, c.W, 1) and preds["depth_conf"].shape == (c.F, c.H, c.W) and preds["depth"].is_cuda
    assert preds["images"].shape == (c.F, 3, c.H, c.W) and preds["extrinsic"].shape == (c.F, 3, 4) and preds["intrinsic"].shape == (c.F, 3, 3)
    assert torch.equal(preds["images"], rgb.permute(0, 3, 1, 2).float() / 255)
    np.testing.assert_allclose(preds["intrinsic"][0].cpu().numpy(), [[32, 0, 32], [0, 32, 24], [0, 0, 1]])
    step = np.diff(c.setup.inv_depth, axis=1)[:, 0]
    share, n = R.kept_and_correct(preds["depth_conf"].cpu().numpy(), preds["depth"][..., 0].cpu().numpy().astype(np.float64), c.true_depth, step)
    print(f"device recovery: {share:.4f} of {n} kept pixels within 1.5 plane steps")
    assert share >= 0.90, share


def test_pose_convention_end_to_end():
    """Panoramas of the box scene -> convert_pano_to_pers == the scene rendered directly at view_poses (2 grey levels, away from box
    edges), and PlaneSweepDepth -> depth_to_world_points puts the kept points on the box's walls: a wrong sign or axis fails both."""
    from evoworld_amd import mvs, reprojection as RP
    from evoworld_amd.geometry import xyz_euler_to_four_by_four_matrix_batch
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    scene, cam, n = R.pose_scene(), R.POSE_CAM, 5
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(cam[:n]), relative=False).numpy()
    panos = _dev(scene.render_panos(c2w, 128, 256))
    loop = UnifiedLoopConsistencyPipeline(None, None, height=128, width=256, num_frames=25, num_segments=1, face_res=32)
    loop.equi2pers = RP.Equi2Pers(height=48, width=64, fov_x=90.0, mode="bilinear")
    pers, _ = loop.convert_pano_to_pers(panos, cam, 0)
    absolute = mvs.view_poses(cam, n, 0, relative=False)
    K = mvs.pinhole(48, 64)
    direct, true_depth, face, _ = scene.render_views(absolute, K, 48, 64)
    edge = R.near_face_edge(face)
    got = pers.cpu().numpy()
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    diff = np.abs(got[..., 0].astype(int) - direct.astype(int))
    print(f"views vs direct render: max {diff[~edge].max()} grey levels away from box edges; edge share {edge.mean():.4f}")
    assert edge.mean() <= 0.03
    assert diff[~edge].max() <= 2
    stage = mvs.PlaneSweepDepth(cam, n_src=4, planes=32, patch_radius=2, segment_id=0)
    preds = stage(pers)                                   # the poses from camera_params, as a user's direct call gets them
    pts = RP.depth_to_world_points(preds["depth"], preds["extrinsic"], preds["intrinsic"]).cpu().numpy().astype(np.float64)
    first = np.linalg.inv(np.concatenate([absolute[0], [[0, 0, 0, 1.0]]]))             # first view -> scene
    P = pts @ first[:3, :3].T + first[:3, 3]
    z = preds["depth"][..., 0].cpu().numpy().astype(np.float64)
    conf = preds["depth_conf"].cpu().numpy()
    step = np.diff(stage.last_setup.inv_depth, axis=1)[:, 0]
    keep = conf >= np.percentile(conf, 50.0)
    on_wall = scene.wall_distance(P) <= 1.5 * step[:, None, None] * z ** 2              # 1.5 plane steps of inverse depth, as a distance at depth z
    print(f"kept points within 1.5 plane steps of a wall: {on_wall[keep].mean():.4f} of {int(keep.sum())}")
    assert on_wall[keep].mean() >= 0.90


def test_cloud_cli_writes_the_filtered_cloud_on_the_walls(tmp_path, capsys):
    """python -m evoworld_amd.mvs cloud, in process: panorama files + camera_poses.txt -> views -> depth -> the filtered cloud as a PLY,
    in the first view's frame; its points lie on the box's walls."""
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
    mvs.main(["cloud", "--frames", str(tmp_path / "frames"), "--poses", str(tmp_path / "camera_poses.txt"), "--segment", "0", "--output", str(out),
              "--planes", "32", "--view_height", "48", "--view_width", "64"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    pts, rgb = read_ply(str(out))
    assert rec["views"] == 5 and rec["points_in"] == rec["points_out"] == len(pts) and 5 * 48 * 64 // 2 <= len(pts) < 5 * 48 * 64
    first = np.linalg.inv(np.concatenate([mvs.view_poses(cam, n, 0, relative=False)[0], [[0, 0, 0, 1.0]]]))
    P = pts.astype(np.float64) @ first[:3, :3].T + first[:3, 3]
    z_far = mvs.sweep_setup(mvs.view_poses(cam, n, 0), mvs.pinhole(48, 64), 4, 32).z_far
    depth = np.linalg.norm(P - first[:3, 3], axis=1)                                   # at least the point's depth in any view near the first
    share = float((scene.wall_distance(P) <= 1.5 / z_far.min() * depth ** 2).mean())  # 1.5 of the coarsest view's plane steps at that range
    print(f"cloud CLI: {len(pts)} points, {share:.4f} within 1.5 plane steps of a wall")
    assert share >= 0.90 and (rgb[:, 0] == rgb[:, 1]).all()


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


def test_episode_with_the_mvs_stage_and_the_default_untouched(tiny, tmp_path):
    """The tiny 2-segment synthetic episode: default loader, then depth_stage='mvs', then the default loader again in the same process.
    The mvs run goes through and renders other memory panoramas; the two default runs are bit-identical, frames and panoramas."""
    from types import SimpleNamespace
    from PIL import Image
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.mvs import PlaneSweepDepth
    from evoworld_amd.stages import load_stages
    cfg, pipe = tiny
    H, W, T = 128, 256, 25
    i = np.arange(60, dtype=np.float64)
    cam = np.stack([0.04 * i * np.sin(i / 9), 0 * i, 0.04 * i * np.cos(i / 9), 0 * i, 95 + 3.6 * i, 0 * i], 1)
    args = SimpleNamespace(svd_path=None, mvs_planes=16, mvs_sources=2)
    start = (torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    saved = (pipe.vae, pipe.image_encoder, pipe.vae_scale_factor)

    def run(name, depth_stage):
        st = load_stages(None, args, depth_stage=depth_stage, cross_attention_dim=cfg["cross_attention_dim"], camera_params=cam, depth_hw=(48, 64))
        assert isinstance(st.depth_model, PlaneSweepDepth) == (depth_stage == "mvs")
        pipe.set_components(vae=st.vae, image_encoder=st.image_encoder)
        loop = UnifiedLoopConsistencyPipeline(pipe, st.depth_model, height=H, width=W, num_frames=T, num_segments=2, num_inference_steps=1,
                                              pano_size=(64, 128), face_res=32)
        frames = loop.process_episode(start, cam, save_dir=str(tmp_path / name))
        d = tmp_path / name / "rendered_panorama_vggt_open3d_0"
        return frames, np.stack([np.asarray(Image.open(d / f"{k:02}.png")) for k in range(24)])

    try:
        f0, p0 = run("default_before", None)
        f1, p1 = run("mvs", "mvs")
        f2, p2 = run("default_after", None)
    finally:
        pipe.vae, pipe.image_encoder, pipe.vae_scale_factor = saved
    assert f1.shape == (49, 3, H, W) and torch.isfinite(f1).all()
    assert not np.array_equal(p1, p0), "the memory panoramas of the mvs run equal the stand-in's"
    assert (p1 != 0).any(), "the mvs memory rendered nothing"
    assert torch.equal(f0, f2) and np.array_equal(p0, p2)
