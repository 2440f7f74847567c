"""-m 'not gpu': the host side of the LPIPS feature -- the upsampling-mean weights against F.interpolate in float64, the
state-dict loader (both key layouts, the two-file merge, refusals), the CLI glue and the ABI entries."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref
from evoworld_amd import lpips as L
from evoworld_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SIZES = ((64, 64), (70, 93), (576, 1024))


def test_tap_sizes_match_the_restatement():
    for H, W in FRAME_SIZES[:2]:
        taps = lpips_ref.features(torch.zeros(1, 3, H, W), lpips_ref.random_weights(0))
        assert L.tap_sizes(H, W) == [tuple(t.shape[-2:]) for t in taps]
    assert L.tap_sizes(576, 1024) == [(143, 255), (71, 127), (35, 63), (35, 63), (35, 63)]
    assert L.tap_sizes(31, 31)[-1] == (1, 1)
    for H, W in ((30, 64), (64, 30), (8, 8)):
        with pytest.raises(ValueError, match="at least 31"):
            L.tap_sizes(H, W)


def test_upsample_mean_weights_equal_interpolate_mean():
    g = torch.Generator().manual_seed(5)
    for H, W in FRAME_SIZES:
        for h, w in sorted(set(L.tap_sizes(H, W))):
            wy, wx = L.upsample_mean_weights(h, H), L.upsample_mean_weights(w, W)
            assert wy.dtype == np.float64 and wy.shape == (h,) and wx.shape == (w,)
            assert abs(wy.sum() - H) < 1e-9 * H and abs(wx.sum() - W) < 1e-9 * W
            assert (wy >= 0).all() and (wx >= 0).all()
            m = torch.rand(1, 1, h, w, generator=g, dtype=torch.float64)
            want = float(F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False).mean())
            got = float((torch.from_numpy(wy)[:, None] * torch.from_numpy(wx)[None, :] * m[0, 0]).sum() / (H * W))
            assert abs(got - want) <= 1e-12, (H, W, h, w, got, want)
    assert np.array_equal(L.upsample_mean_weights(5, 5), np.ones(5))                        # identity resampling
    with pytest.raises(ValueError):
        L.upsample_mean_weights(0, 4)


def _torchvision_layout(sd):
    """the same weights as torchvision's AlexNet state dict and the lpips package's alex.pth"""
    alex, lin = {}, {}
    for k, v in sd.items():
        m = re.fullmatch(r"net\.slice\d\.(\d+)\.(weight|bias)", k)
        if m:
            alex[f"features.{m.group(1)}.{m.group(2)}"] = v
        else:
            lin[k] = v
    alex["classifier.1.weight"] = torch.zeros(4, 4)                                         # what else such a file holds is ignored
    return alex, lin


def _same_pack(p, q):
    assert p.keys() == q.keys()
    for k in p:
        if isinstance(p[k], torch.Tensor):
            assert p[k].dtype == q[k].dtype and torch.equal(p[k], q[k]), k
        else:
            assert p[k] == q[k], k


def test_state_dict_layouts_and_two_file_merge_pack_identically(tmp_path):
    from safetensors.torch import save_file
    sd = lpips_ref.random_weights(3)
    want = L.pack_state_dict(sd)
    for i, (_, co, ci, k, _, _) in enumerate(L.CONVS):
        K = k * k * ci
        assert want[f"w{i}"].dtype == torch.float16 and want[f"w{i}"].shape == (co, -(-K // 64) * 64)
        w = sd[f"net.slice{i + 1}.{L.CONVS[i][0]}.weight"]
        assert torch.equal(want[f"w{i}"][:, :K], w.permute(0, 2, 3, 1).reshape(co, K).half())   # K ordered (ky, kx, c_in)
        assert not want[f"w{i}"][:, K:].any()
        assert want[f"lin{i}"].dtype == torch.float32 and want[f"lin{i}"].shape == (co,)
    assert want["shift"] == L.SHIFT and want["scale"] == L.SCALE
    # the full lpips.LPIPS.state_dict(): scaling_layer buffers and the duplicate lins.* entries
    full = dict(sd)
    full["scaling_layer.shift"] = torch.tensor(L.SHIFT).view(1, 3, 1, 1)
    full["scaling_layer.scale"] = torch.tensor(L.SCALE).view(1, 3, 1, 1)
    for i in range(5):
        full[f"lins.{i}.model.1.weight"] = torch.full_like(sd[f"lin{i}.model.1.weight"], 7.0)   # ignored, whatever they hold
    got = L.pack_state_dict(full)
    assert got["shift"] == pytest.approx(L.SHIFT, rel=1e-6) and got["scale"] == pytest.approx(L.SCALE, rel=1e-6)
    _same_pack({k: v for k, v in got.items() if k not in ("shift", "scale")}, {k: v for k, v in want.items() if k not in ("shift", "scale")})
    # torchvision AlexNet + alex.pth, as dicts and as two files of either format
    alex, lin = _torchvision_layout(sd)
    _same_pack(L.pack_state_dict({**alex, **lin}), want)
    f_alex, f_lin, f_one = tmp_path / "alexnet.pth", tmp_path / "alex.safetensors", tmp_path / "lpips.safetensors"
    torch.save(alex, f_alex)
    save_file({k: v.contiguous() for k, v in lin.items()}, str(f_lin))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(f_one))
    _same_pack(L.pack_state_dict(L.load_state_files([f_alex, f_lin])), want)
    _same_pack(L.pack_state_dict(L.load_state_files(str(f_one))), want)
    model = L.LPIPSAlex.from_files([str(f_alex), str(f_lin)], device="cpu")                  # packing needs no GPU; calling it does
    assert torch.equal(model.w[1], want["w1"]) and model.chunk >= 1


def test_state_dict_refusals():
    sd = lpips_ref.random_weights(1)
    bad = {k: v for k, v in sd.items() if k not in ("net.slice2.3.bias", "lin4.model.1.weight")}
    with pytest.raises(KeyError) as e:
        L.pack_state_dict(bad)
    assert "missing 2 keys" in str(e.value) and "net.slice2.3.bias" in str(e.value) and "lin4.model.1.weight" in str(e.value)
    alex, _ = _torchvision_layout(sd)
    with pytest.raises(KeyError, match="lin0.model.1.weight"):
        L.pack_state_dict(alex)                                                              # the backbone alone: no lin weights
    bad = dict(sd)
    bad["net.slice3.6.weight"] = torch.zeros(384, 192, 5, 5)
    with pytest.raises(ValueError) as e:
        L.pack_state_dict(bad)
    assert "net.slice3.6.weight" in str(e.value) and "(384, 192, 3, 3)" in str(e.value) and "(384, 192, 5, 5)" in str(e.value)
    bad = dict(sd)
    bad["lin1.model.1.weight"] = torch.zeros(192)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        L.pack_state_dict(bad)


def test_random_state_dict_is_seeded_and_loadable():
    a, b = L.random_state_dict(4), L.random_state_dict(4)
    assert a.keys() == lpips_ref.random_weights(0).keys()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(float(a[f"lin{i}.model.1.weight"].min()) >= 0 for i in range(5))
    L.pack_state_dict(a)


def test_cli_flags_and_metric_selection():
    args = M.parse_args(["--data_path", "x"])
    assert args.lpips_weights is None and args.lpips_channel_order == "bgr" and args.metrics == "psnr,ssim"
    args = M.parse_args(["--data_path", "x", "--metrics", "psnr,ssim,lpips", "--lpips_weights", "a.pth", "b.safetensors",
                         "--lpips_channel_order", "rgb"])
    assert args.lpips_weights == ["a.pth", "b.safetensors"] and args.lpips_channel_order == "rgb"
    assert M.parse_args(["--lpips_weights", "one.safetensors"]).lpips_weights == ["one.safetensors"]
    with pytest.raises(SystemExit):
        M.parse_args(["--lpips_channel_order", "gbr"])
    # lpips only when weights exist; everything else as before
    assert M.selected_metrics("psnr,lpips", lpips_weights=True) == ["psnr", "lpips"]
    assert M.selected_metrics("lpips", True) == ["lpips"]
    with pytest.raises(ValueError, match="LPIPS"):
        M.selected_metrics("psnr,lpips")
    with pytest.raises(ValueError, match="LPIPS"):
        M.selected_metrics("psnr,lpips", lpips_weights=False)
    with pytest.raises(ValueError, match="I3D"):
        M.selected_metrics("fvd,lpips", lpips_weights=True)
    assert M.selected_metrics("psnr, ssim") == ["psnr", "ssim"]
    assert set(M.NOT_COMPUTED) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"} and M.SUPPORTED == ("psnr", "ssim")


def test_shell_script_passes_the_weights_through():
    sh = open(os.path.join(ROOT, "calculate_metrics.sh")).read()
    assert "LPIPS_WEIGHTS" in sh and "--lpips_weights $LPIPS_WEIGHTS" in sh and "psnr,ssim,lpips" in sh


def test_abi_declares_the_lpips_entries():
    from evoworld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "evoworld_hip.h")).read()
    for s in ("ew_im2col_frames_f16", "ew_im2col3d_f16", "ew_maxpool3d_relu_f16", "ew_lpips_head", "ew_lpips_head_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.HEADER.functions, s
    version = int(re.search(r"#define EW_ABI_VERSION (\d+)", hdr).group(1))
    assert version == _lib.ABI_VERSION and version >= 14
    lib = _lib.load()
    assert lib.ew_abi_version() == version
    for s in ("ew_im2col_frames_f16", "ew_im2col3d_f16", "ew_maxpool3d_relu_f16", "ew_lpips_head", "ew_lpips_head_workspace_bytes"):
        assert (getattr(lib, s).restype, list(getattr(lib, s).argtypes)) == _lib.HEADER.signatures[s], s
    # the workspace of the head: 8 bytes per (frame, block), a block count that depends on the tap alone
    one = lib.ew_lpips_head_workspace_bytes(1, 143, 255, 64)
    assert one > 0 and one % 8 == 0 and lib.ew_lpips_head_workspace_bytes(7, 143, 255, 64) == 7 * one
    assert lib.ew_lpips_head_workspace_bytes(0, 143, 255, 64) == 0


def test_ops_refuse_cpu_tensors():
    from evoworld_amd import ops
    from evoworld_amd._lib import EvoWorldHipError
    with pytest.raises(EvoWorldHipError):
        ops.maxpool3d_relu(torch.zeros(1, 8, 8, 8, dtype=torch.float16), (1, 3, 3), (1, 2, 2), (0, 0, 0), (1, 3, 3))
    with pytest.raises(EvoWorldHipError):
        ops.im2col3d(torch.zeros(1, 8, 8, 8, dtype=torch.float16), (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 8, 8), 128)
    with pytest.raises(EvoWorldHipError):
        ops.im2col_frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 3, 1, 1, 64, L.SHIFT, L.SCALE)
    with pytest.raises(EvoWorldHipError):
        L.LPIPSAlex.from_random(0, device="cpu")(torch.zeros(1, 64, 64, 3, dtype=torch.uint8), torch.zeros(1, 64, 64, 3, dtype=torch.uint8))
