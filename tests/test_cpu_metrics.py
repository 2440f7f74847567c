"""-m 'not gpu': the host side of the metrics CLI (evoworld_amd/metrics.py: arguments, episode discovery, frame pairing, the
count-mismatch error), the reference's aggregation and the fp64 restatement the GPU tests use (tests/metrics_ref.py), both against
tests/golden/metrics.npz (a run of the reference's own calculate_psnr / calculate_ssim / main, tools/make_goldens_metrics.py)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import metrics_ref as MR


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


def _json(d):
    return json.loads(json.dumps(d))


def test_cli_arguments_follow_the_reference():
    from evoworld_amd import metrics as M
    a = M.parse_args(["--data_path", "out/x", "--num_video", "7", "--gt_subdir", "predictions_gt_2", "--gen_subdir", "predictions_2"])
    assert a.num_videos == 7 and a.result_file == os.path.join("out/x", "eval_score.json")
    assert (a.gt_subdir, a.gen_subdir, a.test_length, a.metrics, a.pair_by_name) == ("predictions_gt_2", "predictions_2", 25, "psnr,ssim", False)
    d = M.parse_args(["--pair_by_name", "--test_length", "3"])
    assert (d.data_path, d.gt_subdir, d.gen_subdir, d.num_videos, d.pair_by_name) == (
        "data/Segment_Consistency/test", "predictions_gt_1", "predictions_1", 100, True)


def test_metric_selection_names_the_missing_networks():
    from evoworld_amd import metrics as M
    assert M.selected_metrics("psnr,ssim") == ["psnr", "ssim"] and M.selected_metrics(" ssim ") == ["ssim"]
    assert set(M.NOT_COMPUTED) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"}
    for m, word in (("fvd", "I3D"), ("lpips", "LPIPS"), ("latent_mse", "VAE"), ("loop_closure_latent_mse", "VAE")):
        with pytest.raises(ValueError, match=word):
            M.selected_metrics(f"psnr,{m}")
    with pytest.raises(ValueError, match="unknown"):
        M.selected_metrics("dreamsim")


def _touch(d, ids):
    d.mkdir(parents=True)
    for i in ids:
        (d / f"{i:03}.png").write_bytes(b"")


def test_episode_folders_are_the_sorted_subdirectories(tmp_path):
    from evoworld_amd import metrics as M
    for e in ["case_002", "case_000", "case_001"]:
        (tmp_path / e).mkdir()
    (tmp_path / "eval_score.json").write_text("{}")
    assert M.list_episode_folders(str(tmp_path)) == ["case_000", "case_001", "case_002"]
    assert M.list_episode_folders(str(tmp_path), 2) == ["case_000", "case_001"]


def test_frame_pairing_and_the_count_mismatch(tmp_path):
    """segment 1 of an episode: predictions_gt_1 holds 025..049 (25 frames), predictions_1 holds 025..048 (24)"""
    from evoworld_amd import metrics as M
    _touch(tmp_path / "case_000" / "predictions_gt_1", range(25, 50))
    _touch(tmp_path / "case_000" / "predictions_1", range(25, 49))
    with pytest.raises(ValueError, match=r"episode case_000: predictions_gt_1 holds 25 frames and predictions_1 holds 24"):
        M.frame_pairs(str(tmp_path), "case_000", "predictions_gt_1", "predictions_1")
    gt, gen = M.frame_pairs(str(tmp_path), "case_000", "predictions_gt_1", "predictions_1", pair_by_name=True)
    names = [f"{i:03}.png" for i in range(25, 49)]
    assert [os.path.basename(p) for p in gt] == names == [os.path.basename(p) for p in gen]
    assert all(p.endswith(os.path.join("predictions_gt_1", n)) for p, n in zip(gt, names))
    # more than 25 files: the last 25 of each folder, or of the shared names
    _touch(tmp_path / "case_001" / "predictions_gt_0", range(1, 31))
    _touch(tmp_path / "case_001" / "predictions_0", range(3, 33))
    gt, gen = M.frame_pairs(str(tmp_path), "case_001", "predictions_gt_0", "predictions_0")
    assert [os.path.basename(p) for p in gt] == [f"{i:03}.png" for i in range(6, 31)]
    assert [os.path.basename(p) for p in gen] == [f"{i:03}.png" for i in range(8, 33)]
    gt, gen = M.frame_pairs(str(tmp_path), "case_001", "predictions_gt_0", "predictions_0", pair_by_name=True)
    assert [os.path.basename(p) for p in gen] == [f"{i:03}.png" for i in range(6, 31)]
    # the CLI refuses before any decode or device work
    args = SimpleNamespace(data_path=str(tmp_path), gt_subdir="predictions_gt_1", gen_subdir="predictions_1", num_videos=1,
                           metrics="psnr,ssim", pair_by_name=False)
    with pytest.raises(ValueError, match="case_000"):
        M.evaluate(args)


def test_golden_records_the_reference_failure_on_24_vs_25_frames(g):
    assert str(g["main_mismatch_error"]) == "AssertionError"


def test_aggregation_reproduces_the_reference_dicts(g):
    from evoworld_amd import metrics as M
    for tag, C in (("c3", 3), ("c1", 1)):
        for name in ("psnr", "ssim"):
            want = json.loads(str(g[f"{name}_dict_{tag}"]))
            got = _json(M.aggregate(g[f"{name}_frames_{tag}"], torch.Size([25, C, 29, 41])))
            assert got == want, (name, tag)


def test_main_result_is_the_aggregation_of_the_per_frame_values(g):
    """main reads BGR (cv2.imread) where the per-frame golden is RGB: the same values up to the order of the channel sums"""
    from evoworld_amd import metrics as M
    main = json.loads(str(g["main_result"]))
    for name, tol in (("psnr", 1e-5), ("ssim", 1e-12)):
        got = _json(M.aggregate(g[f"{name}_frames_c3"], torch.Size([25, 3, 29, 41])))
        assert got["video_setting"] == main[name]["video_setting"] == [25, 3, 29, 41]
        assert got["video_setting_name"] == main[name]["video_setting_name"]
        assert abs(got["value_mean"] - main[name]["value_mean"]) <= tol
        for k in ("value", "value_std"):
            assert got[k].keys() == main[name][k].keys()
            assert max(abs(got[k][t] - main[name][k][t]) for t in got[k]) <= tol


def test_restatement_matches_the_reference_per_frame(g):
    gt, gen = g["gt"], g["gen"]
    dp = ds1 = ds3 = 0.0
    for e in range(gt.shape[0]):
        for t in range(gt.shape[1]):
            a, b = MR.u8_values(gt[e, t]).transpose(2, 0, 1), MR.u8_values(gen[e, t]).transpose(2, 0, 1)
            dp = max(dp, abs(MR.psnr_ref(a, b) - g["psnr_frames_c3"][e, t]))
            ds3 = max(ds3, abs(MR.ssim_ref(a, b) - g["ssim_frames_c3"][e, t]))
            ds1 = max(ds1, abs(MR.ssim_ref(a[:1], b[:1]) - g["ssim_frames_c1"][e, t]))
    # measured: 5.3e-7 dB (the reference averages the squares in float32), SSIM 3.2e-14
    assert dp <= 1e-5 and ds3 <= 1e-12 and ds1 <= 1e-12, (dp, ds3, ds1)


def test_pixel_values_and_the_psnr_100_rule(g):
    k = np.arange(256)
    t = (torch.arange(256, dtype=torch.uint8) / 255.0).numpy()
    assert np.array_equal(MR.u8_values(k), t)
    assert int((MR.u8_values(k) != (k.astype(np.float32) * np.float32(1 / 255.0)).astype(np.float32)).sum()) == 126
    base = (np.arange(3 * 576 * 1024) % 251).astype(np.uint8)
    for n in (11, 12):
        other = base.copy()
        other[g[f"edge_idx_{n}"]] += 1
        p, want = MR.psnr_ref(MR.u8_values(base), MR.u8_values(other)), float(g[f"edge_psnr_{n}"])
        assert (p == 100) == (want == 100) == (n == 11)
        assert abs(p - want) <= 1e-6


def test_gt_dump_map(g):
    x = (torch.arange(256, dtype=torch.uint8).float() / 255.0) * 2 - 1
    want = (x * 0.5 + 0.5).clamp(0, 1).mul(255).byte().numpy()
    assert np.array_equal(g["gt_map"], want)
    low = want != np.arange(256)
    assert int(low.sum()) == 63 and np.all(want[low] == np.arange(256)[low] - 1) and low[1] and low[2] and low[3]
