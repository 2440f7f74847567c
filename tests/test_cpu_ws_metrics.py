"""-m 'not gpu': the host side of the spherical metrics (WS-PSNR / WS-SSIM / WS-LPIPS, cube-face viewports): the latitude weights,
the weighted form of lpips.upsample_mean_weights against torch's own interpolation, metric selection and its refusals, the header's
declarations.  None of it is in the reference; include/evoworld_hip.h and evoworld_amd/metrics.py state the definitions."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ws_metrics_ref as WR


def test_latitude_weights():
    from evoworld_amd import metrics as M
    for H in (11, 40, 576):
        w = M.latitude_weights(H)
        assert w.dtype == np.float64 and w.shape == (H,)
        want = np.array([math.cos((y + 0.5 - H / 2) * math.pi / H) for y in range(H)])
        assert np.abs(w - want).max() <= 1e-15 and np.abs(w - WR.latitude_weights(H)).max() <= 1e-15
        assert np.abs(w - w[::-1]).max() <= 1e-15 and w.min() > 0 and w.argmax() in (H // 2 - 1, H // 2)
        assert abs(w.sum() - 2 * H / math.pi) <= 0.005 * 2 * H / math.pi          # the midpoint rule of the integral of cos over the sphere
    assert M.latitude_weights(11)[5] == 1.0                                       # the equator row of an odd height
    assert abs(M.latitude_weights(576)[0] - math.sin(math.pi / 1152)) <= 1e-15    # half a row from the pole
    with pytest.raises(ValueError):
        M.latitude_weights(0)


def _today(n_in, n_out):
    """upsample_mean_weights as it was before it took output weights, restated"""
    i = np.arange(n_out, dtype=np.float64)
    src = np.maximum(0.0, (i + 0.5) * (float(n_in) / float(n_out)) - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w = np.zeros(n_in, dtype=np.float64)
    np.add.at(w, i0, 1.0 - (src - i0))
    np.add.at(w, i1, src - i0)
    return w


@pytest.mark.parametrize("n_in,n_out", [(7, 64), (15, 70), (1, 9)])
def test_upsample_mean_weights_under_output_weights(n_in, n_out):
    from evoworld_amd.lpips import upsample_mean_weights
    plain = upsample_mean_weights(n_in, n_out)
    assert np.array_equal(plain, _today(n_in, n_out))
    assert np.array_equal(upsample_mean_weights(n_in, n_out, None), plain)
    assert np.array_equal(upsample_mean_weights(n_in, n_out, np.ones(n_out)), plain)       # what makes WS-LPIPS under ones plain LPIPS
    rng = np.random.default_rng(n_in * 100 + n_out)
    w = rng.random(n_out) + 0.05
    m = torch.from_numpy(rng.standard_normal((n_in, 5)))                                    # fp64 map, 5 columns
    up = F.interpolate(m[None, None], size=(n_out, 5), mode="bilinear", align_corners=False)[0, 0].numpy()
    want = (w[:, None] * up).sum(0)
    got = (upsample_mean_weights(n_in, n_out, w)[:, None] * m.numpy()).sum(0)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert abs(upsample_mean_weights(n_in, n_out, w).sum() - w.sum()) <= 1e-12 * w.sum()
    with pytest.raises(ValueError):
        upsample_mean_weights(n_in, n_out, w[:-1])


def test_metric_selection_with_the_spherical_names():
    from evoworld_amd import metrics as M
    assert M.SUPPORTED == ("psnr", "ssim") and set(M.NOT_COMPUTED) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"}
    assert M.SPHERICAL == ("ws_psnr", "ws_ssim", "ws_lpips")
    assert M.selected_metrics("psnr,ssim,ws_psnr,ws_ssim") == ["psnr", "ssim", "ws_psnr", "ws_ssim"]
    assert M.selected_metrics("ws_ssim") == ["ws_ssim"]
    assert M.selected_metrics("ws_lpips,lpips", True) == ["ws_lpips", "lpips"]
    assert M.selected_metrics("ws_lpips", lpips_weights=True, projection="equirect") == ["ws_lpips"]
    for kw in ({}, {"lpips_weights": False}, {"fvd_weights": True, "latent_mse_weights": True}):
        with pytest.raises(ValueError, match="LPIPS"):
            M.selected_metrics("psnr,ws_lpips", **kw)
    for name in ("ws_psnr", "ws_ssim", "ws_lpips"):
        with pytest.raises(ValueError, match="cube"):
            M.selected_metrics(f"psnr,{name}", lpips_weights=True, projection="cube")
    assert M.selected_metrics("psnr,ssim", projection="cube") == ["psnr", "ssim"]
    with pytest.raises(ValueError, match="projection"):
        M.selected_metrics("psnr", projection="fisheye")
    with pytest.raises(ValueError, match="unknown"):
        M.selected_metrics("ws_fvd")


def test_cli_arguments_and_refusals_before_any_device_work(tmp_path):
    from evoworld_amd import metrics as M
    d = M.parse_args([])
    assert (d.projection, d.viewport_size, d.metrics) == ("equirect", None, "psnr,ssim")
    a = M.parse_args(["--projection", "cube", "--viewport_size", "48"])
    assert (a.projection, a.viewport_size) == ("cube", 48)
    with pytest.raises(SystemExit):
        M.parse_args(["--projection", "fisheye"])
    (tmp_path / "ep_000").mkdir()
    with pytest.raises(ValueError, match="cube"):
        M.evaluate(M.parse_args(["--data_path", str(tmp_path), "--projection", "cube", "--metrics", "psnr,ws_psnr"]))
    with pytest.raises(ValueError, match="LPIPS"):
        M.evaluate(M.parse_args(["--data_path", str(tmp_path), "--metrics", "psnr,ws_lpips"]))


def test_row_weight_validation():
    from evoworld_amd import ops
    w = ops.check_row_weights([1.0] * 12, 12, ssim=True)
    assert w.dtype == np.float64 and w.shape == (12,)
    assert np.array_equal(ops.check_row_weights(torch.ones(12), 12), w)
    edge = np.zeros(12)
    edge[:5] = 1.0                                        # positive overall, zero on the centre rows 5 .. 6
    assert ops.check_row_weights(edge, 12).sum() == 5.0
    for bad, kw, msg in ((np.ones(11), {}, "expected 12"), (np.ones((12, 1)), {}, "expected 12"), (np.full(12, np.nan), {}, "finite"),
                         (np.full(12, np.inf), {}, "finite"), (-np.ones(12), {}, ">= 0"), (np.zeros(12), {}, "sum to zero"),
                         (edge, {"ssim": True}, "centre rows")):
        with pytest.raises(ValueError, match=msg):
            ops.check_row_weights(bad, 12, **kw)


def test_header_declares_the_weighted_entry_points():
    from evoworld_amd import _lib
    H = _lib.HEADER
    assert H.functions["ew_video_metrics_ws_workspace_bytes"] == ("size_t", ["int"] * 4)
    ret, params = H.functions["ew_video_metrics_ws"]
    planar = H.functions["ew_video_metrics"][1]
    assert ret == "ew_status" and params == planar[:8] + ["const double*"] + planar[8:]
    assert H.constants["EW_ABI_VERSION"] == _lib.ABI_VERSION >= 18
