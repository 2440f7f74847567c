"""-m gpu: ew_video_metrics and ew_gt_dump_map_u8 (csrc/metrics.hip) through evoworld_amd.metrics, against a run of the
reference's own evaluation (tests/golden/metrics.npz, tools/make_goldens_metrics.py) and the fp64 restatement (tests/metrics_ref.py);
the evaluation CLI on a PNG tree; the episode-mode ground-truth dumps predictions_gt_{seg} and the metrics of their segments."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


def _frames_f32(u8, C=3):
    """uint8 [...,H,W,3] -> fp32 [F,C,H,W] = uint8 / 255.0 (torch), as the reference's main builds its videos"""
    t = torch.from_numpy(np.ascontiguousarray(u8)).reshape(-1, *u8.shape[-3:]).permute(0, 3, 1, 2) / 255.0
    return t[:, :C].contiguous()


def test_per_frame_values_match_the_reference(g):
    from evoworld_amd import metrics as M, ops
    gt, gen = g["gt"], g["gen"]
    F_ = gt.shape[0] * gt.shape[1]
    p, s = M.video_metrics_u8(torch.from_numpy(gt).reshape(F_, 29, 41, 3).to(DEV), torch.from_numpy(gen).reshape(F_, 29, 41, 3).to(DEV))
    worst = {"u8": (np.abs(p - g["psnr_frames_c3"].ravel()).max(), np.abs(s - g["ssim_frames_c3"].ravel()).max())}
    for C in (3, 1):
        sse, ssim = ops.video_metrics(_frames_f32(gt, C).to(DEV), _frames_f32(gen, C).to(DEV))
        p = np.array([M.psnr_from_sse(v, C * 29 * 41) for v in sse.cpu().numpy()])
        worst[f"f32 C={C}"] = (np.abs(p - g[f"psnr_frames_c{C}"].ravel()).max(), np.abs(ssim.cpu().numpy() - g[f"ssim_frames_c{C}"].ravel()).max())
    print(worst)
    # bounds |dPSNR| <= 1e-5 dB, |dSSIM| <= 1e-9; measured on the MI355X: PSNR 5.3e-7 dB (u8, f32 C=3), 6.0e-7 dB (C=1) -- the
    # reference averages the squares in float32 --, SSIM 1.6e-14 (C=3), 3.2e-14 (C=1)
    for k, (dp, ds) in worst.items():
        assert dp <= 1e-5 and ds <= 1e-9, (k, dp, ds)


def _compare_dicts(got, want, tol):
    got = json.loads(json.dumps(got))
    assert got["video_setting"] == want["video_setting"] and got["video_setting_name"] == want["video_setting_name"]
    assert abs(got["value_mean"] - want["value_mean"]) <= tol
    for k in ("value", "value_std"):
        assert got[k].keys() == want[k].keys()
        assert max(abs(got[k][t] - want[k][t]) for t in got[k]) <= tol, k


def test_calculate_psnr_and_ssim_return_the_reference_dicts(g):
    from evoworld_amd import metrics as M
    v1 = torch.from_numpy(g["gt"]).permute(0, 1, 4, 2, 3) / 255.0                 # [B,T,C,H,W] on the host, as the reference takes it
    v2 = torch.from_numpy(g["gen"]).permute(0, 1, 4, 2, 3) / 255.0
    for tag, sl in (("c3", slice(0, 3)), ("c1", slice(0, 1))):
        _compare_dicts(M.calculate_psnr(v1[:, :, sl], v2[:, :, sl]), json.loads(str(g[f"psnr_dict_{tag}"])), 1e-5)
        _compare_dicts(M.calculate_ssim(v1[:, :, sl].to(DEV), v2[:, :, sl].to(DEV)), json.loads(str(g[f"ssim_dict_{tag}"])), 1e-9)


def _pair(F_, H, W, C, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([np.stack([(128 + 100 * np.sin(0.013 * x * (c + 1) + 0.021 * y + f)) for c in range(C)], -1) for f in range(F_)])
    a = np.clip(a + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _check_against_restatement(a, b, sse, ssim, tol_ssim=1e-9):
    for f in range(a.shape[0]):
        fa, fb = MR.u8_values(a[f]).transpose(2, 0, 1), MR.u8_values(b[f]).transpose(2, 0, 1)
        want = MR.sse_ref(fa, fb)
        assert abs(sse[f] - want) <= 1e-12 * max(1.0, want), (f, sse[f], want)
        if ssim is not None:
            assert abs(ssim[f] - MR.ssim_ref(fa, fb)) <= tol_ssim, (f, ssim[f], MR.ssim_ref(fa, fb))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("layout", ["u8", "f32"])
def test_full_size_frames_against_the_fp64_restatement(layout, C):
    from evoworld_amd import ops
    a, b = _pair(2, 576, 1024, C, 7 + C)
    if layout == "u8":
        sse, ssim = ops.video_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    else:
        sse, ssim = ops.video_metrics(_frames_f32(a, C).to(DEV), _frames_f32(b, C).to(DEV))
    _check_against_restatement(a, b, sse.cpu().numpy(), ssim.cpu().numpy())


@pytest.mark.parametrize("H,W", [(11, 11), (11, 12), (12, 11), (25, 33), (48, 64), (49, 65)])
def test_small_and_ragged_sizes(H, W):
    from evoworld_amd import ops
    a, b = _pair(3, H, W, 3, H * W)
    sse, ssim = ops.video_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    _check_against_restatement(a, b, sse.cpu().numpy(), ssim.cpu().numpy())


def test_constant_frames():
    """sigma = 0: equal constant frames give SSIM 1 and PSNR 100; two different constants the restatement's value"""
    from evoworld_amd import metrics as M
    a = np.full((3, 40, 70, 3), 64, np.uint8)
    b = a.copy()
    b[1] = 200
    b[2] = 65
    p, s = M.video_metrics_u8(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert p[0] == 100 and abs(s[0] - 1.0) <= 1e-12
    for f in (1, 2):
        fa, fb = MR.u8_values(a[f]).transpose(2, 0, 1), MR.u8_values(b[f]).transpose(2, 0, 1)
        assert abs(p[f] - MR.psnr_ref(fa, fb)) <= 1e-9 and abs(s[f] - MR.ssim_ref(fa, fb)) <= 1e-9
        m1, m2 = float(fa[0, 0, 0]), float(fb[0, 0, 0])                     # sigma = 0: the luminance term alone
        assert abs(s[f] - (2 * m1 * m2 + 1e-4) / (m1 * m1 + m2 * m2 + 1e-4)) <= 1e-12


def test_psnr_100_rule_at_11_and_12_differing_levels(g):
    from evoworld_amd import metrics as M
    base = (np.arange(3 * 576 * 1024) % 251).astype(np.uint8)
    for n in (11, 12):
        other = base.copy()
        other[g[f"edge_idx_{n}"]] += 1
        hwc = lambda v: torch.from_numpy(np.ascontiguousarray(v.reshape(3, 576, 1024).transpose(1, 2, 0)))[None].to(DEV)
        p, _ = M.video_metrics_u8(hwc(base), hwc(other))
        want = float(g[f"edge_psnr_{n}"])
        assert (p[0] == 100) == (want == 100) == (n == 11)
        assert abs(p[0] - want) <= 1e-5


def test_guarded_outputs_sse_only_and_bit_identical_reruns():
    from evoworld_amd import ops
    a, b = _pair(5, 40, 61, 3, 11)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    buf = torch.full((5 + 16,), float("nan"), dtype=torch.float64, device=DEV)
    buf2 = torch.full((5 + 16,), -7.25, dtype=torch.float64, device=DEV)
    sse, ssim = ops.video_metrics(ta, tb, sse=buf[8:13], ssim=buf2[8:13])
    assert sse.data_ptr() == buf[8:13].data_ptr() and ssim.data_ptr() == buf2[8:13].data_ptr()
    assert torch.isnan(buf[:8]).all() and torch.isnan(buf[13:]).all()
    assert (buf2[:8] == -7.25).all() and (buf2[13:] == -7.25).all()
    assert torch.isfinite(sse).all() and torch.isfinite(ssim).all()
    s2, m2 = ops.video_metrics(ta, tb)
    assert torch.equal(s2.view(torch.int64), sse.view(torch.int64)) and torch.equal(m2.view(torch.int64), ssim.view(torch.int64))
    # SSE only: no SSIM output is touched, and frames below the 11-pixel window are fine
    keep = torch.full((5,), -1.0, dtype=torch.float64, device=DEV)
    s3, m3 = ops.video_metrics(ta, tb, what=ops.METRIC_SSE, ssim=keep)
    assert m3 is None and (keep == -1.0).all() and torch.equal(s3.view(torch.int64), sse.view(torch.int64))
    small_a, small_b = a[:, :7, :9].copy(), b[:, :7, :9].copy()
    s4, _ = ops.video_metrics(torch.from_numpy(small_a).to(DEV), torch.from_numpy(small_b).to(DEV), what=ops.METRIC_SSE)
    _check_against_restatement(small_a, small_b, s4.cpu().numpy(), None)


def test_refusals():
    from evoworld_amd import _lib, ops
    from evoworld_amd._lib import EvoWorldHipError
    lib = _lib.load()
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    for C in (2, 4):
        with pytest.raises(EvoWorldHipError, match=f"C = {C}"):
            ops.video_metrics(u8(2, 16, 16, C), u8(2, 16, 16, C))
    for H, W in ((10, 16), (16, 10)):
        with pytest.raises(EvoWorldHipError, match="H, W >= 11"):
            ops.video_metrics(u8(2, H, W, 3), u8(2, H, W, 3))
    a, out, ws = u8(2, 16, 16, 3), torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(4096, dtype=torch.uint8, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    cases = [((0, 0, 3, 16, 16, 3, P(out), P(out)), "positive"),
             ((0, 2, 3, 16, 16, 1, None, P(out)), "SSE asked for with a NULL output"),
             ((0, 2, 3, 16, 16, 2, P(out), None), "SSIM asked for with a NULL output"),
             ((2, 2, 3, 16, 16, 3, P(out), P(out)), "layout 2"),
             ((0, 2, 3, 16, 16, 0, P(out), P(out)), "what = 0")]
    for (layout, F_, C, H, W, what, s, m), msg in cases:
        st = lib.ew_video_metrics(P(a), P(a), layout, F_, C, H, W, what, s, m, P(ws), None)
        assert st != 0 and msg in lib.ew_last_error().decode(), (msg, lib.ew_last_error())
    with pytest.raises(ValueError):
        ops.video_metrics(u8(2, 16, 16, 3), u8(2, 16, 17, 3))


def test_gt_dump_map_kernel(g):
    from evoworld_amd import ops
    k = torch.arange(256, dtype=torch.uint8, device=DEV)
    assert np.array_equal(ops.gt_dump_map_u8(k).cpu().numpy(), g["gt_map"])
    x = torch.randint(0, 256, (3, 37, 53, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    assert np.array_equal(ops.gt_dump_map_u8(x.to(DEV)).cpu().numpy(), g["gt_map"][x.numpy()])


def _write_tree(root, gt, gen, n_gen=None):
    for e in range(gt.shape[0]):
        for sub, v, n in (("predictions_gt_0", gt, gt.shape[1]), ("predictions_0", gen, n_gen or gen.shape[1])):
            d = os.path.join(root, f"ep_{e:03d}", sub)
            os.makedirs(d, exist_ok=True)
            for t in range(n):
                Image.fromarray(v[e, t]).save(os.path.join(d, f"{t + 1:03}.png"))


def test_cli_on_a_png_tree_matches_the_reference_main(g, tmp_path):
    from evoworld_amd import metrics as M
    _write_tree(str(tmp_path), g["gt"], g["gen"])
    M.main(["--data_path", str(tmp_path), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0", "--num_video", "3",
            "--result_file", "scores.json"])
    got = json.load(open(tmp_path / "scores.json"))
    want = json.loads(str(g["main_result"]))
    assert list(got) == ["ssim", "psnr", "not_computed"] and set(got["not_computed"]) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"}
    _compare_dicts(got["psnr"], want["psnr"], 1e-5)
    _compare_dicts(got["ssim"], want["ssim"], 1e-9)
    one, _ = M.main(["--data_path", str(tmp_path), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0", "--metrics", "ssim"])
    assert list(one) == ["ssim", "not_computed"]
    with pytest.raises(ValueError, match="I3D"):
        M.main(["--data_path", str(tmp_path), "--metrics", "psnr,fvd"])


def test_cli_count_mismatch_and_pair_by_name(g, tmp_path):
    """24 generated vs 25 ground-truth frames: the reference fails its shape assertion (golden); the CLI names the episode and the
    counts, and --pair_by_name scores the 24 shared file names"""
    from evoworld_amd import metrics as M
    _write_tree(str(tmp_path), g["gt"], g["gen"], n_gen=24)
    argv = ["--data_path", str(tmp_path), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0"]
    with pytest.raises(ValueError, match="episode ep_000: predictions_gt_0 holds 25 frames and predictions_0 holds 24"):
        M.main(argv)
    res, _ = M.main(argv + ["--pair_by_name"])
    assert list(res["psnr"]["video_setting"]) == [24, 3, 29, 41]
    B = g["gt"].shape[0]
    want = M.aggregate(g["ssim_frames_c3"][:, :24], None)
    assert max(abs(res["ssim"]["value"][t] - want["value"][t]) for t in range(24)) <= 1e-9 and len(res["ssim"]["value"]) == 24 and B == 3


# ------------------------------------------------------------------ episode mode: predictions_gt_{seg}
def _write_ckpt(tmp_path):
    from safetensors.torch import save_file
    from evoworld_amd.unet import DEFAULT_CONFIG, random_state_dict
    from oracle.unet_ref import tiny_config
    cfg = tiny_config()
    cfg["num_frames"] = 25
    ck = tmp_path / "ckpt" / "unet"
    ck.mkdir(parents=True)
    json.dump({k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, open(ck / "config.json", "w"))
    save_file({k: v.contiguous() for k, v in random_state_dict({**DEFAULT_CONFIG, **cfg}, 0).items()}, str(ck / "diffusion_pytorch_model.safetensors"))


def _pano(i, H=100, W=200):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(x * (c + 2) + y * 3 + 17 * i + 60 * c) % 256 for c in range(3)], -1).astype(np.uint8)


def test_episode_gt_dumps_and_their_segment_metrics(g, tmp_path):
    """a 2-segment curve-mode episode at 128x256 with real panoramas: predictions_gt_0 = ids 1..25 as 001..025, predictions_gt_1 =
    ids 26..50 as 025..049, each the map of the Pillow-exact resize; segment 1's metrics need --pair_by_name"""
    import unified_loop_consistency as cli
    from evoworld_amd import metrics as M
    _write_ckpt(tmp_path)
    ep = tmp_path / "data" / "case_000"
    (ep / "panorama").mkdir(parents=True)
    n = 56
    with open(ep / "camera_poses.txt", "w") as f:
        f.write("Frame,PosX,PosY,PosZ,RotX,RotY,RotZ\n")
        for i in range(n):
            f.write(f"{i + 1},{float(0.4 * i * np.sin(np.deg2rad(95.0)))!r},1.78,{float(0.4 * i * np.cos(np.deg2rad(95.0)))!r},0.0,95.0,0.0\n")
    for i in range(1, n + 1):
        Image.fromarray(_pano(i)).save(ep / "panorama" / f"{i:03}.png")
    rep = cli.main(["--unet_path", str(tmp_path / "ckpt"), "--base_folder", str(tmp_path / "data"), "--save_dir", str(tmp_path / "out"),
                    "--num_segments", "2", "--num_inference_steps", "1", "--height", "128", "--width", "256", "--save_frames", "--curve_path"])
    assert rep[0]["frames"] == 49
    d = tmp_path / "out" / "case_000"
    for seg, (ids, first) in enumerate(((range(1, 26), 1), (range(26, 51), 25))):
        names = sorted(os.listdir(d / f"predictions_gt_{seg}"))
        assert names == [f"{first + k:03}.png" for k in range(25)]
        for k, pid in enumerate(ids):
            want = g["gt_map"][np.array(Image.fromarray(_pano(pid)).resize((256, 128), Image.BILINEAR))]
            assert np.array_equal(np.array(Image.open(d / f"predictions_gt_{seg}" / names[k])), want), (seg, pid)
    argv = ["--data_path", str(tmp_path / "out"), "--gt_subdir", "predictions_gt_1", "--gen_subdir", "predictions_1"]
    with pytest.raises(ValueError, match="case_000: predictions_gt_1 holds 25 frames and predictions_1 holds 24"):
        M.main(argv)
    res, _ = M.main(argv + ["--pair_by_name"])
    assert list(res["psnr"]["video_setting"]) == [24, 3, 128, 256] and os.path.isfile(tmp_path / "out" / "eval_score.json")
    res0, _ = M.main(["--data_path", str(tmp_path / "out"), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0"])
    assert list(res0["ssim"]["video_setting"]) == [25, 3, 128, 256]


def test_episode_without_panoramas_writes_no_gt_dump(tmp_path):
    from evoworld_amd.dataset import load_gt_window_u8
    (tmp_path / "panorama").mkdir()
    assert load_gt_window_u8(str(tmp_path), 0, 25, 128, 256, DEV) is None
    Image.fromarray(_pano(1)).save(tmp_path / "panorama" / "001.png")
    Image.fromarray(_pano(2)).save(tmp_path / "panorama" / "002.png")
    w = load_gt_window_u8(str(tmp_path), 0, 25, 100, 200, DEV)
    assert w.shape == (2, 100, 200, 3) and np.array_equal(w[1].cpu().numpy(), _pano(2))
    assert load_gt_window_u8(str(tmp_path), 0, 25, 100, 200, DEV, n_poses=1).shape[0] == 1
