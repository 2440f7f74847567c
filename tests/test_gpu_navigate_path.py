"""-m gpu: the non-curve navigation mode -- ew_pano_yaw_rotate against the reference's rotate_panorama indices, Navigator.navigate_path
against a run of the reference's own navigate_path (tests/golden/navigate_path.npz), process_episode(curve_path=False) on the tiny
U-Net, and the CLI without --curve_path."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rotate_indices_torch(H, W, deg):
    """The reference's index arithmetic (navigator_evoworld.py:483-503) in torch on the host: (ui [W], vi [H])."""
    rad = torch.deg2rad(torch.tensor(deg, dtype=torch.float32))
    x, y = torch.linspace(0, W - 1, W), torch.linspace(0, H - 1, H)
    lon = (x / W) * 2 * torch.pi
    lat = (y / H) * torch.pi - (torch.pi / 2)
    uf = ((lon + rad) % (2 * torch.pi)) / (2 * torch.pi) * W
    vf = (lat + (torch.pi / 2)) / torch.pi * H
    return torch.clamp(uf, 0, W - 1).long(), torch.clamp(vf, 0, H - 1).long()


def _encoded(V, H, W):
    """fp32 [V,3,H,W] whose pixel value is c*H*W + y*W + x (exact in fp32)"""
    base = (torch.arange(H)[:, None] * W + torch.arange(W)[None, :]).float()
    return torch.stack([base + c * H * W for c in range(3)])[None].repeat(V, 1, 1, 1).to(DEV)


def _decode(out, H, W):
    o = out.long().cpu() - torch.arange(3)[None, :, None, None] * H * W
    return o % W, o // W


def test_pano_yaw_rotate_indices_match_reference_golden(golden_dir):
    """576x1024, all golden yaws in ONE call (V = 8, mixed yaws): every gathered index equals the reference's ui / vi."""
    from evoworld_amd import ops
    g = np.load(f"{golden_dir}/navigate_path.npz")
    H, W = g["b_hw"].tolist()
    yaws = torch.from_numpy(g["b_yaws"])
    u, v = _decode(ops.pano_yaw_rotate(_encoded(len(yaws), H, W), yaws), H, W)
    for k in range(len(yaws)):
        want_u = torch.from_numpy(g["b_ui"][k].astype(np.int64))
        want_v = torch.from_numpy(g["b_vi"][k].astype(np.int64))
        assert torch.equal(u[k], want_u[None, None, :].expand(3, H, W)), f"columns, yaw {float(yaws[k])}"
        assert torch.equal(v[k], want_v[None, :, None].expand(3, H, W)), f"rows, yaw {float(yaws[k])}"
    # not a plain roll, even at 0 degrees
    assert int((torch.from_numpy(g["b_vi"][0].astype(np.int64)) != torch.arange(H)).sum()) == 73


@pytest.mark.parametrize("H,W", [(7, 13), (64, 128), (33, 300)])
def test_pano_yaw_rotate_odd_sizes_and_mixed_yaws(H, W):
    from evoworld_amd import ops
    yaws = torch.tensor([0.0, 45.0, -123.25, 359.9, 1e-3], dtype=torch.float32)
    u, v = _decode(ops.pano_yaw_rotate(_encoded(len(yaws), H, W), yaws), H, W)
    for k, d in enumerate(yaws.tolist()):
        wu, wv = _rotate_indices_torch(H, W, d)
        assert torch.equal(u[k], wu[None, None, :].expand(3, H, W)) and torch.equal(v[k], wv[None, :, None].expand(3, H, W))


@pytest.mark.parametrize("H,W", [(576, 1024), (7, 13)])
def test_pano_yaw_rotate_u8_is_conversion_then_rotation(H, W):
    from evoworld_amd import ops
    g = torch.Generator().manual_seed(5)
    src = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    yaws = torch.tensor([90.0, -37.5, 0.0], dtype=torch.float32)
    got = ops.pano_yaw_rotate(src, yaws)
    want = ops.pano_yaw_rotate(ops.u8_hwc_to_f32_chw(src), yaws)
    assert got.shape == (3, 3, H, W) and torch.equal(got, want)
    # the conversion is the ToTensor + CustomRescale arithmetic, the gather the reference's
    wu, wv = _rotate_indices_torch(H, W, -37.5)
    ref = (src[1].cpu().permute(2, 0, 1).float() / 255.0 * 2 - 1)[:, wv][:, :, wu]
    assert torch.equal(got[1].cpu(), ref)


def test_pano_yaw_rotate_refuses_bad_arguments():
    from evoworld_amd import _lib, ops
    from evoworld_amd._lib import EvoWorldHipError
    lib = _lib.load()
    src = torch.zeros(1, 3, 8, 16, device=DEV)
    yaw = torch.zeros(1, device=DEV)
    dst = torch.empty(1, 3, 8, 16, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(t, off=0):
        return ctypes.c_void_p(t.data_ptr() + off)
    bad = [(None, 0, p(yaw), p(dst), 1, 8, 16), (p(src), 0, None, p(dst), 1, 8, 16), (p(src), 0, p(yaw), None, 1, 8, 16),
           (p(src), 0, p(yaw), p(dst), 0, 8, 16), (p(src), 0, p(yaw), p(dst), 1, 0, 16), (p(src), 0, p(yaw), p(dst), 1, 8, -1),
           (p(src), 2, p(yaw), p(dst), 1, 8, 16), (p(src, 2), 0, p(yaw), p(dst), 1, 8, 16), (p(src), 0, p(yaw), p(dst, 2), 1, 8, 16),
           (p(src), 0, p(yaw), p(dst), 1, 1 << 24, 16)]
    for args in bad:
        with pytest.raises(EvoWorldHipError):
            _lib.check(lib.ew_pano_yaw_rotate(*args, s), "ew_pano_yaw_rotate")
    with pytest.raises(EvoWorldHipError):
        ops.pano_yaw_rotate(src.cpu(), yaw)                                 # no CPU path
    with pytest.raises(ValueError):
        ops.pano_yaw_rotate(src, torch.zeros(2))                            # one yaw per panorama
    with pytest.raises(TypeError):
        ops.pano_yaw_rotate(src, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.pano_yaw_rotate(torch.zeros(1, 4, 8, 16, device=DEV), yaw)


def _stub_frame(call, i, H, W):
    """the recording pipe's frame i of call `call` (tools/make_goldens_navigate_path.py: stub_frame)"""
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(5 * x + 11 * y + 17 * i + 31 * call + 70 * c) % 256 for c in range(3)], -1).astype(np.uint8)


@pytest.mark.parametrize("start_kind", ["f32", "u8"])
def test_navigate_path_vs_reference_run(golden_dir, start_kind):
    """segment_id 0..3 with infer_segment=True, then one chained call: the rotated image handed to the pipe and the frame
    count bit-exact, mask_mem, the re-seeded default generator, current_pose; Plücker at the tolerance of the window test."""
    from types import SimpleNamespace
    from evoworld_amd.inference import Navigator
    g = np.load(f"{golden_dir}/navigate_path.npz")
    H, W = g["c_hw"].tolist()
    path = torch.from_numpy(g["c_path"].copy()).to(DEV)
    path0 = path.clone()
    start_u8 = torch.from_numpy(g["c_start_u8"])
    # the f32 start image is made on the host, as the reference's transform makes it (torch's device division by a scalar is a
    # multiplication by its reciprocal: not the same bits)
    start = start_u8.to(DEV) if start_kind == "u8" else (start_u8.permute(2, 0, 1).float() / 255.0 * 2 - 1).to(DEV)
    memory = torch.zeros(1, 25, 3, H, W, device=DEV)
    seeded = torch.manual_seed(-1).get_state()
    calls = []

    def pipe(image, **kw):
        c = len(calls)
        calls.append(dict(image=image.clone(), plucker=kw["plucker_embedding"].clone(), mask_mem=kw["mask_mem"],
                          reseeded=kw["generator"] is torch.default_generator and torch.equal(kw["generator"].get_state(), seeded)))
        return SimpleNamespace(frames=[[Image.fromarray(_stub_frame(c, i, H, W)) for i in range(25)]])
    nav = Navigator(pipe, height=H, width=W, num_frames=25, fps=7)
    poses = []
    n_infer = int(g["c_call_infer"].sum())
    for k in range(n_infer):
        gens = nav.navigate_path(path, start, num_inference_steps=7, memorized_images=memory, infer_segment=True, segment_id=k)
        assert len(gens) == 1
        calls[-1]["n_frames"] = len(gens[0][0][0][:gens[0][1]])
        poses.append(nav.current_pose.clone())
    gens = nav.navigate_path(path, start, num_inference_steps=7, memorized_images=memory)
    for c, (frames, n) in zip(calls[n_infer:], gens):
        c["n_frames"] = len(frames[0][:n])
    assert len(calls) == len(g["c_call_segment"]) and torch.equal(path, path0)
    want_img = torch.from_numpy(g["c_image_u8_hwc"]).permute(0, 3, 1, 2).float() / 255.0 * 2 - 1
    for i, c in enumerate(calls):
        assert torch.equal(c["image"][0].cpu(), want_img[i]), f"call {i}: image handed to the pipe"
        assert c["n_frames"] == int(g["c_n_frames"][i]) and c["mask_mem"] == bool(g["c_mask_mem"][i])
        assert c["reseeded"] and bool(g["c_reseeded"][i])
        want_pl = torch.from_numpy(g[f"c_plucker_seg{int(g['c_call_segment'][i])}"])
        assert c["plucker"].shape == (1, 25, 6, H // 8, W // 8) and rel_l2(c["plucker"][0].cpu(), want_pl) < 5e-6, f"call {i}: Plücker"
    for k in range(n_infer):
        assert np.array_equal(poses[k].cpu().numpy(), g["c_current_pose"][k])
    assert np.array_equal(nav.current_pose.cpu().numpy(), g["c_current_pose"][-1])


def _loop_cam(runs, step=0.4):
    """unscaled RDF poses: straight runs [(yaw, rows)] joined by in-place turns"""
    rows, x, z = [], 0.0, 0.0
    for yaw, n in runs:
        for i in range(n):
            if rows:
                x, z = x + step * np.sin(np.deg2rad(yaw)), z + step * np.cos(np.deg2rad(yaw))
            rows.append([x, 0.0, z, 0.0, yaw, 0.0])
    return np.asarray(rows, np.float64)


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


@pytest.mark.parametrize("layout,runs_spec,counts", [
    ("loop", [(95.0, 25), (185.0, 24), (275.0, 24)], [25, 49, 73]),      # straight runs of exactly one window
    ("short", [(95.0, 10), (185.0, 60)], [10, 34]),                        # a 10-pose run (extended, trimmed) then a 61-pose run
])
def test_process_episode_path_mode(tiny, layout, runs_spec, counts):
    """curve_path=False on straight runs joined by in-place 90-degree turns: frame counts follow the runs (frames[:n]), window
    k's Plücker = the k-th turn-split run, segment k > 0 starts from the last frame so far rotated by the turn, and the memory of
    every later segment equals the oracle composition bit for bit (as tests/test_gpu_inference.py checks for curve mode)."""
    from evoworld_amd import ops
    from evoworld_amd import reprojection as RP
    from evoworld_amd.geometry import xyz_euler_to_four_by_four_matrix_batch
    from evoworld_amd.geometry import xyz_euler_to_three_by_four_matrix_batch as _c2w
    from evoworld_amd.inference import Navigator, UnifiedLoopConsistencyPipeline
    from evoworld_amd.plucker import ray_c2w_to_plucker as _pl
    from oracle import reproject_ref as R
    cfg, pipe = tiny
    H, W, T, S = 128, 256, 25, len(runs_spec)
    cam = _loop_cam(runs_spec)
    captured = {"preds": [], "memories": []}

    def depth_model(pers_u8):                       # VGGT stand-in, as in tests/test_gpu_inference.py
        F_, Hp, Wp, _ = pers_u8.shape
        gg = torch.Generator().manual_seed(4 + F_)
        poses = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(cam[:F_], dtype=torch.float32), relative=True).double().numpy()
        preds = {"depth": (torch.rand(F_, Hp // 8, Wp // 8, 1, generator=gg) * 6 + 1).numpy(),
                 "depth_conf": torch.rand(F_, Hp // 8, Wp // 8, generator=gg).numpy(),
                 "images": (pers_u8[:, ::8, ::8].permute(0, 3, 1, 2).float() / 255).cpu().numpy(),
                 "extrinsic": np.linalg.inv(poses)[:, :3, :4].astype(np.float32),
                 "intrinsic": np.repeat(np.array([[[Wp / 16, 0, Wp / 16], [0, Wp / 16, Hp / 16], [0, 0, 1]]], np.float32), F_, 0)}
        captured["preds"].append(preds)
        return preds

    def frames_from_latents(lat):
        x = torch.nn.functional.interpolate(lat[0, :, :3], scale_factor=8.0, mode="nearest")
        return torch.tanh(x / 300.0)

    def image_latents_fn(first, memory):
        x = torch.cat([first[None], memory], 0)
        lat = torch.nn.functional.avg_pool2d(x, 8)
        captured["memories"].append(memory.clone())
        return dict(image_latents=torch.cat([lat, lat[:, :1]], 1)[None], image_embeddings=torch.ones(1, 1, cfg["cross_attention_dim"]) * 0.1)

    loop = UnifiedLoopConsistencyPipeline(pipe, depth_model, frames_from_latents, height=H, width=W, num_frames=T, num_segments=S,
                                          num_inference_steps=1, pano_size=(64, 128), face_res=32, curve_path=False)
    start = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV) * 2 - 1
    seen = []
    orig_call = pipe.__class__.__call__

    def spy(self, image, **k):
        seen.append((k["plucker_embedding"].clone(), k["mask_mem"], image.clone()))
        return orig_call(self, image, **k)
    pipe.__class__.__call__ = spy
    try:
        frames = loop.process_episode(start, cam, image_latents_fn)
    finally:
        pipe.__class__.__call__ = orig_call
    assert frames.shape == (counts[-1], 3, H, W) and len(seen) == S
    assert [p["depth"].shape[0] for p in captured["preds"]] == counts[:-1]
    scaled = torch.tensor(cam, dtype=torch.float32)
    scaled[:, :3] *= 0.1
    runs = Navigator.split_path_into_segments(scaled)
    assert len(runs) == S
    for seg in range(S):
        window = loop.nav.extend_segment(runs[seg], T).to(DEV)          # a short run is extrapolated to 25 poses (navigator :186-188)
        assert torch.equal(seen[seg][0][0], _pl(loop.nav.rays, _c2w(window, relative=True))[:T])
        assert seen[seg][1] is (seg == 0)
        if seg:
            turn = runs[seg][0][4] - runs[seg - 1][-1][4]
            assert float(turn) == 90.0
            last = frames[counts[seg - 1] - 1]
            want = ops.pano_yaw_rotate(last[None].contiguous(), turn.reshape(1))[0]     # the fp32 form on the float frame
            assert torch.equal(seen[seg][2].reshape(3, H, W), want) and not torch.equal(want, last)
    mems = captured["memories"]
    assert len(mems) == S and not mems[0].any() and len(captured["preds"]) == S - 1
    for seg in range(S - 1):
        assert torch.equal(mems[seg + 1][0], start)
        n_have = counts[seg]
        p = captured["preds"][seg]
        _, yaws = loop.convert_pano_to_pers(loop.last_frames_u8[:n_have], cam, seg)
        _s, end_idx, _l = RP.calculate_segment_indices(seg)
        temp = cam.copy()
        s0 = max(0, end_idx - n_have)
        temp[s0:end_idx, 4] = yaws[: end_idx - s0]
        poses = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(temp, dtype=torch.float32), relative=True).numpy()
        xyz = ops.depth_unproject(torch.tensor(p["depth"][..., 0]).to(DEV), torch.tensor(p["extrinsic"]).to(DEV), torch.tensor(p["intrinsic"]).to(DEV)).cpu().numpy()
        v, c = R.confidence_filter_ref(xyz, p["depth_conf"], R.extract_colors_ref(p["images"]), 50.0)
        faces, _ = R.splat_ref(v, c, R.face_w2c_ref(R.target_c2w_ref(poses, p["extrinsic"], seg)), 32, 16.0, 16.0, 16.0, 16.0, 0.1)
        pano = R.cube2equi_gather_ref(faces, R.cube2equi_lut_ref(128, 64, 32))
        want = torch.stack([(torch.tensor(np.array(Image.fromarray(pp).resize((W, H), Image.BILINEAR))).permute(2, 0, 1).float() / 255) * 2 - 1 for pp in pano])
        assert torch.equal(mems[seg + 1][1:].cpu(), want), f"memory for segment {seg + 1}"


def test_process_episode_path_mode_refuses_what_the_reference_cannot_do(tiny):
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    _cfg, pipe = tiny
    start = torch.zeros(3, 128, 256, device=DEV)

    def mk(S):
        return UnifiedLoopConsistencyPipeline(pipe, None, height=128, width=256, num_segments=S, num_inference_steps=1, curve_path=False)
    with pytest.raises(ValueError, match="segment 2"):
        mk(3).process_episode(start, _loop_cam([(95.0, 50), (185.0, 40)]))                # two straight runs, three segments
    with pytest.raises(ValueError, match="segment 1"):
        mk(3).process_episode(start, _loop_cam([(95.0, 25), (185.0, 24), (275.0, 10)]))   # 59 poses: segment 2's memory needs 73
    import unified_loop_consistency as cli
    with pytest.raises(ValueError, match="segment 0: the memory hand-off would align on 1 generated frame"):
        mk(2).process_episode(start, cli.synthetic_episode(56))                         # turns at every pose: a 1-pose first run


def _write_ckpt(tmp_path):
    """the tiny U-Net in the diffusers folder layout under tmp_path/ckpt"""
    import json
    from safetensors.torch import save_file
    from evoworld_amd.unet import DEFAULT_CONFIG, random_state_dict
    from oracle.unet_ref import tiny_config
    cfg = tiny_config()
    cfg["num_frames"] = 25
    ck = tmp_path / "ckpt" / "unet"
    ck.mkdir(parents=True)
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, open(ck / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in random_state_dict({**DEFAULT_CONFIG, **cfg}, 0).items()}, str(ck / "diffusion_pytorch_model.safetensors"))


def _write_episode(tmp_path, cam_unity):
    _write_ckpt(tmp_path)
    ep = tmp_path / "data" / "case_000"
    ep.mkdir(parents=True)
    with open(ep / "camera_poses.txt", "w") as f:
        f.write("Frame,PosX,PosY,PosZ,RotX,RotY,RotZ\n")
        for i, r in enumerate(cam_unity):
            f.write(f"{i + 1}," + ",".join(repr(float(x)) for x in r) + "\n")


def test_cli_without_curve_path_runs_the_path_mode(tmp_path):
    """unified_loop_consistency.py without --curve_path: segment 1 gets the turn-split window and frame 24 rotated by the turn,
    predictions_{seg} hold 25 + 24 frames; the same episode with --curve_path does not rotate."""
    import os
    import unified_loop_consistency as cli
    from evoworld_amd import ops
    from evoworld_amd.geometry import xyz_euler_to_three_by_four_matrix_batch as _c2w
    from evoworld_amd.inference import Navigator
    from evoworld_amd.pipeline import StableVideoDiffusionPipeline
    from evoworld_amd.plucker import equirectangular_to_ray, ray_c2w_to_plucker as _pl
    unity = _loop_cam([(95.0, 25), (185.0, 24), (275.0, 24)]) * np.array([1, -1, 1, -1, 1, -1.0])
    unity[:, 1] = 1.78
    _write_episode(tmp_path, unity)
    cam = cli.load_camera_poses(str(tmp_path / "data" / "case_000"))
    scaled = torch.tensor(cam, dtype=torch.float32)
    scaled[:, :3] *= 0.1
    rays = torch.tensor(equirectangular_to_ray(16, 32)).float().to(DEV)
    orig = StableVideoDiffusionPipeline.__call__
    out = {}
    for mode in ("path", "curve"):
        seen = []

        def spy(self, image, **k):
            seen.append((image.clone(), k["plucker_embedding"].clone()))
            return orig(self, image, **k)
        StableVideoDiffusionPipeline.__call__ = spy
        try:
            rep = cli.main(["--unet_path", str(tmp_path / "ckpt"), "--base_folder", str(tmp_path / "data"), "--save_dir", str(tmp_path / mode),
                            "--num_segments", "2", "--num_inference_steps", "1", "--height", "128", "--width", "256", "--save_frames"]
                           + (["--curve_path"] if mode == "curve" else []))
        finally:
            StableVideoDiffusionPipeline.__call__ = orig
        assert rep[0]["frames"] == 49 and len(seen) == 2
        d = tmp_path / mode / "case_000"
        assert sorted(os.listdir(d / "predictions_0")) == [f"{i:03}.png" for i in range(1, 26)]
        assert sorted(os.listdir(d / "predictions_1")) == [f"{i:03}.png" for i in range(25, 49)]    # numbered from seg * 24 + 1 (:434)
        f24 = torch.from_numpy(np.array(Image.open(d / "predictions_0" / "025.png")))[None].to(DEV)
        out[mode] = (seen, f24)
    seen, f24 = out["path"]
    runs = Navigator.split_path_into_segments(scaled)
    turn = runs[1][0][4] - runs[0][-1][4]
    assert float(turn) == 90.0
    assert torch.equal(seen[1][0][0], ops.pano_yaw_rotate(f24, turn.reshape(1))[0])
    assert torch.equal(seen[1][1][0], _pl(rays, _c2w(runs[1].to(DEV), relative=True)))
    seen, f24 = out["curve"]
    assert torch.equal(seen[1][0][0], ops.u8_hwc_to_f32_chw(f24)[0])
    assert torch.equal(seen[1][1][0], _pl(rays, _c2w(scaled[24:49].to(DEV), relative=True)))


def test_cli_synthetic_episode_without_curve_path(tmp_path):
    """run_unified_pipeline.sh with CURVE_PATH=false and no episode folder: the synthetic path-mode episode (straight runs joined
    by 90-degree turns) runs to the end -- 25 + 24 frames, segment 1 started from frame 24 rotated by the turn."""
    import os
    import unified_loop_consistency as cli
    from evoworld_amd import ops
    from evoworld_amd.pipeline import StableVideoDiffusionPipeline
    _write_ckpt(tmp_path)
    orig = StableVideoDiffusionPipeline.__call__
    seen = []

    def spy(self, image, **k):
        seen.append(image.clone())
        return orig(self, image, **k)
    StableVideoDiffusionPipeline.__call__ = spy
    try:
        rep = cli.main(["--unet_path", str(tmp_path / "ckpt"), "--base_folder", str(tmp_path / "no_episodes"), "--save_dir", str(tmp_path / "out"),
                        "--num_segments", "2", "--num_inference_steps", "1", "--height", "128", "--width", "256", "--save_frames"])
    finally:
        StableVideoDiffusionPipeline.__call__ = orig
    assert rep[0]["frames"] == 49 and len(seen) == 2
    d = tmp_path / "out" / "synthetic_000"
    assert len(os.listdir(d / "predictions")) == 49
    f24 = torch.from_numpy(np.array(Image.open(d / "predictions" / "025.png")))[None].to(DEV)
    assert torch.equal(seen[1][0], ops.pano_yaw_rotate(f24, torch.tensor([90.0]))[0])
