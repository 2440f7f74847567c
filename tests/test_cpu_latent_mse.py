"""-m 'not gpu': the host side of the latent MSE feature -- the Inception-v4 table (149 units, 41,142,816 parameters, the stage shapes) and
the fp32 restatement tests/inception_v4_ref.py in the same key layout, the state-dict loader and packer with the BatchNorm fold, the
antialiased resize tables against F.interpolate, the aggregation, the CLI glue and the ABI entries."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_v4_ref as R
from evoworld_amd import latent_mse as L
from evoworld_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ew_frames_resize_aa_norm_f16", "ew_avgpool3x3_relu_f16", "ew_global_avgpool_relu_f32")
STAGES = [(149, 149, 32), (147, 147, 32), (147, 147, 64), (73, 73, 160), (71, 71, 192)] + [(35, 35, 384)] * 5 + [(17, 17, 1024)] * 8 + [(8, 8, 1536)] * 4


@pytest.fixture(scope="module")
def sd0():
    return L.random_state_dict(0)


@pytest.fixture(scope="module")
def net0(sd0):
    return R.build(sd0)


def test_table_has_149_units_and_the_published_parameter_count(sd0, net0):
    units = L.units()
    assert len(units) == 149 and len({u[0] for u in units}) == 149
    assert sum(co * ci * kh * kw + 2 * co for _, ci, co, (kh, kw), _, _ in units) == 41_142_816      # timm's 42.68 M minus the classifier
    assert sum(p.numel() for p in net0.parameters()) == 41_142_816
    # the restatement, written out module by module, has the table's units: names, shapes, strides and pads
    ref = R.units(net0)
    assert [n for n, _ in ref] == [u[0] for u in units]
    for (name, ci, co, k, s, p), (_, m) in zip(units, ref):
        c = m.conv
        assert (c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding) == (ci, co, k, (s, s), p), name
        assert m.bn.eps == 1e-3 and c.bias is None
    assert units[0] == ("features.0", 3, 32, (3, 3), 2, (0, 0)) and units[-1] == ("features.21.branch3.1", 1536, 256, (1, 1), 1, (0, 0))
    assert sorted({(u[3], u[4]) for u in units}) == sorted({((3, 3), 1), ((3, 3), 2), ((1, 1), 1), ((1, 7), 1), ((7, 1), 1), ((1, 3), 1), ((3, 1), 1)})


def test_stage_shapes(net0):
    assert L.stage_shapes() == STAGES and len(L.FEATURES) == 22
    eps = {}
    out = R.features(net0, torch.rand(1, 3, 40, 50, generator=torch.Generator().manual_seed(0)), endpoints=eps)
    assert tuple(out.shape) == (1, 1536) and list(eps) == [f"features.{i}" for i in range(22)]
    assert [(e.shape[2], e.shape[3], e.shape[1]) for e in eps.values()] == STAGES
    with pytest.raises(ValueError, match="does not fit"):
        L.stage_shapes(64)


def test_random_state_dict_is_seeded_and_loads_strictly(sd0, net0):
    again, other = L.random_state_dict(0), L.random_state_dict(1)
    assert len(sd0) == 149 * 6 and set(sd0) == set(net0.state_dict())
    assert all(torch.equal(sd0[k], again[k]) for k in sd0)
    assert not torch.equal(sd0["features.12.branch2.3.conv.weight"], other["features.12.branch2.3.conv.weight"])
    assert tuple(sd0["features.19.branch2_3b.conv.weight"].shape) == (256, 512, 3, 1) and tuple(sd0["features.4.branch1.1.conv.weight"].shape) == (64, 64, 1, 7)


def test_loader_refusals_and_ignored_keys(sd0):
    want = L.pack_state_dict(sd0)
    assert set(want) == {f"{u[0]}.{p}" for u in L.units() for p in ("w", "b")}
    wrapped = {"module." + k: v for k, v in sd0.items()}
    wrapped["module.last_linear.weight"], wrapped["module.last_linear.bias"] = torch.zeros(1001, 1536), torch.zeros(1001)
    wrapped["something.else"] = torch.zeros(3)
    got = L.pack_state_dict(wrapped)
    assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)
    canon = L.canonical_state_dict(wrapped)
    assert len(canon) == 149 * 5 and not any("num_batches_tracked" in k or "last_linear" in k for k in canon)
    bad = {k: v for k, v in sd0.items() if k not in ("features.7.branch2.1.bn.running_var", "features.21.branch0.conv.weight")}
    with pytest.raises(KeyError) as e:
        L.pack_state_dict(bad)
    assert "missing 2 keys" in str(e.value) and "features.7.branch2.1.bn.running_var" in str(e.value) and "features.21.branch0.conv.weight" in str(e.value)
    bad = dict(sd0)
    bad["features.11.branch1.1.conv.weight"] = torch.zeros(224, 192, 7, 1)                      # (1, 7) transposed
    with pytest.raises(ValueError) as e:
        L.pack_state_dict(bad)
    assert "features.11.branch1.1.conv.weight" in str(e.value) and "(224, 192, 1, 7)" in str(e.value) and "(224, 192, 7, 1)" in str(e.value)
    bad = dict(sd0)
    bad["features.2.bn.bias"] = torch.zeros(65)
    with pytest.raises(ValueError, match=r"features\.2\.bn\.bias"):
        L.pack_state_dict(bad)
    from evoworld_amd import fvd
    with pytest.raises(KeyError, match="Inception-v4 state dict is missing"):                   # another architecture fails loudly
        L.pack_state_dict({k: torch.zeros(1) for k in list(fvd._spec())[:20]})


def test_weight_files(tmp_path, sd0):
    from safetensors.torch import save_file
    want = L.pack_state_dict(sd0)
    f_st, f_pt, f_ckpt = tmp_path / "inception_v4.safetensors", tmp_path / "inception_v4.pth", tmp_path / "ckpt.pt"
    save_file({k: v.contiguous() for k, v in sd0.items()}, str(f_st))
    torch.save(sd0, f_pt)
    torch.save({"state_dict": sd0, "epoch": 3}, f_ckpt)
    for f in (f_st, str(f_pt), [f_ckpt]):
        got = L.pack_state_dict(L.load_state_files(f))
        assert all(torch.equal(got[k], want[k]) for k in want)
    model = L.InceptionV4.from_files(str(f_st), device="cpu")                                   # packing needs no GPU; calling it does
    assert torch.equal(model.p["features.21.branch3.1.w"], want["features.21.branch3.1.w"]) and model.chunk == 5


def test_pack_orders_columns_and_pads(sd0):
    packed = L.pack_state_dict(sd0)
    c = L.canonical_state_dict(sd0)
    for name, ci, co, (kh, kw), _, _ in L.units():
        cp = -(-ci // 8) * 8
        K = kh * kw * cp
        w, b = packed[f"{name}.w"], packed[f"{name}.b"]
        assert w.dtype == torch.float16 and tuple(w.shape) == (co, -(-K // 64) * 64) and not w[:, K:].any(), name
        assert b.dtype == torch.float16 and tuple(b.shape) == (co,)
        g, beta, mean, var = (sd0[f"{name}.bn.{p}"].double() for p in ("weight", "bias", "running_mean", "running_var"))
        s = g / torch.sqrt(var + 1e-3)
        want = torch.zeros(co, kh, kw, cp, dtype=torch.float64)
        want[..., :ci] = (sd0[f"{name}.conv.weight"].double() * s.view(-1, 1, 1, 1)).permute(0, 2, 3, 1)
        assert torch.equal(w[:, :K], want.reshape(co, K).half()), name
        assert torch.equal(b, (beta - mean * s).half()), name
        fw, fb = L.fold_batchnorm(c, name)
        assert fw.dtype == torch.float64 and torch.equal(fb.half(), b)
    assert packed["features.0.w"].shape[1] == 128 and not packed["features.0.w"][:, :72].view(32, 9, 8)[:, :, 3:].any()
    assert packed["features.4.branch0.0.w"].shape[1] == 192                                      # 160 channels: K padded to 64
    # a (1, 7) kernel: column dx * C + c; a (7, 1) kernel: column dy * C + c
    w17, w71 = sd0["features.4.branch1.1.conv.weight"], sd0["features.4.branch1.2.conv.weight"]
    s17 = sd0["features.4.branch1.1.bn.weight"].double() / (sd0["features.4.branch1.1.bn.running_var"].double() + 1e-3).sqrt()
    s71 = sd0["features.4.branch1.2.bn.weight"].double() / (sd0["features.4.branch1.2.bn.running_var"].double() + 1e-3).sqrt()
    for o, tap, ch in ((0, 0, 0), (5, 6, 63), (63, 3, 17)):
        assert float(packed["features.4.branch1.1.w"][o, tap * 64 + ch]) == float((w17[o, ch, 0, tap].double() * s17[o]).half())
        assert float(packed["features.4.branch1.2.w"][o, tap * 64 + ch]) == float((w71[o, ch, tap, 0].double() * s71[o]).half())


def test_batchnorm_fold_equals_batchnorm(sd0, net0):
    """the restatement with conv + bias from fold_batchnorm (fp32) against the restatement with BatchNorm, one frame"""
    c = L.canonical_state_dict(sd0)
    folded = R.fold_batchnorm(R.build(sd0), lambda name: L.fold_batchnorm(c, name)).eval()
    assert not any(isinstance(m, torch.nn.BatchNorm2d) for m in folded.modules())
    x = torch.rand(1, 3, 48, 64, generator=torch.Generator().manual_seed(3))
    ea, eb = {}, {}
    a, b = R.features(net0, x, endpoints=ea), R.features(folded, x, endpoints=eb)
    worst = max(float((ea[k] - eb[k]).norm() / ea[k].norm()) for k in ea)
    rel = float((a - b).norm() / a.norm())
    print(f"BatchNorm fold: features rel-L2 {rel:.3e}, worst stage {worst:.3e}")
    assert rel <= 1e-5 and worst <= 1e-5


@pytest.mark.parametrize("H,W,oh,ow", [(57, 91, 29, 29), (20, 30, 29, 29), (200, 640, 299, 299), (576, 1024, 299, 299)])
def test_resize_tables_match_interpolate_antialias(H, W, oh, ow):
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H))
    want = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=True)
    mats = []
    for n_in, n_out in ((H, oh), (W, ow)):
        first, count, weights = L.resize_table(n_in, n_out)
        assert first.dtype == np.int32 and count.dtype == np.int32 and weights.dtype == np.float32 and weights.shape == (n_out, count.max())
        assert first.min() >= 0 and (first + count).max() <= n_in and count.min() >= 1
        assert np.allclose(weights.sum(1), 1.0, atol=1e-6) and weights.min() >= 0
        m = torch.zeros(n_out, n_in)
        for i in range(n_out):
            assert not weights[i, count[i]:].any()
            m[i, first[i]:first[i] + count[i]] = torch.from_numpy(weights[i, :count[i]].copy())
        mats.append(m)
    got = torch.einsum("oh,fchw->fcow", mats[0], torch.einsum("fchw,pw->fchp", x, mats[1]))     # the W pass, then the H pass
    err = float((got - want).abs().max())
    plain = float((F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False) - want).abs().max())
    print(f"resize table {H}x{W} -> {oh}x{ow}: worst |error| {err:.2e} against antialias=True (plain bilinear is {plain:.2e} away)")
    assert err <= 5e-6
    assert L.resize_table(H, oh) is L.resize_table(H, oh)                                        # cached
    with pytest.raises(ValueError):
        L.resize_table(0, 4)


def test_restatement_preprocess_orders():
    u8 = torch.randint(0, 256, (2, 20, 30, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    f32 = u8.permute(0, 3, 1, 2).float() / 255.0
    rgb, bgr = R.preprocess(u8), R.preprocess(u8, "bgr")
    assert tuple(rgb.shape) == (2, 3, 299, 299) and torch.equal(R.preprocess(f32), rgb)
    for c in range(3):                                                                           # planes swapped, mean / std in place
        assert torch.allclose(bgr[:, c] * R.STD[c] + R.MEAN[c], rgb[:, 2 - c] * R.STD[2 - c] + R.MEAN[2 - c], atol=1e-6)


def test_aggregation_matches_the_restatement():
    g = np.random.default_rng(0)
    f1, f2 = g.standard_normal((3, 5, 1536)).astype(np.float32), g.standard_normal((3, 5, 1536)).astype(np.float32)
    setting = torch.Size([15, 3, 299, 299])
    got = L.latent_mse_result(f1, f2, setting)
    want = R.aggregate(f1.reshape(15, 1536), f2.reshape(15, 1536), 3, 5, setting)
    assert list(got) == ["value", "value_mean", "value_std", "video_setting", "video_setting_name"] == list(want)
    assert list(got["value"]) == list(range(5)) == list(got["value_std"]) and all(isinstance(v, float) for v in got["value"].values())
    for k in ("value", "value_std"):
        assert all(got[k][t] == pytest.approx(want[k][t], rel=1e-12) for t in range(5)), k
    assert got["value_mean"] == pytest.approx(want["value_mean"], rel=1e-12) and got["value_mean"] == float(np.mean(list(got["value"].values())))
    assert got["video_setting"] == setting and got["video_setting_name"] == "time, channel, heigth, width"
    d2 = (f1.astype(np.float64) - f2.astype(np.float64)) ** 2
    assert got["value"][2] == pytest.approx(float(d2[:, 2].mean()), rel=1e-12) and got["value_std"][4] == pytest.approx(float(d2[:, 4].std()), rel=1e-12)
    # loop closure: the last timestamp alone (numpy may add the same numbers in another order: 1e-12)
    last = L.latent_mse_result(f1[:, -1:], f2[:, -1:], torch.Size([3, 3, 299, 299]))
    want_last = R.aggregate(f1[:, -1].reshape(3, 1536), f2[:, -1].reshape(3, 1536), 3, 1, torch.Size([3, 3, 299, 299]))
    assert list(last["value"]) == [0] and last["value"][0] == pytest.approx(got["value"][4], rel=1e-12)
    assert last["value_std"][0] == pytest.approx(got["value_std"][4], rel=1e-12) and last["value_mean"] == last["value"][0]
    assert last["value"][0] == pytest.approx(want_last["value"][0], rel=1e-12) and last["value_std"][0] == pytest.approx(want_last["value_std"][0], rel=1e-12)
    same = L.latent_mse_result(f1, f1, setting)
    assert same["value_mean"] == 0.0 and set(same["value_std"].values()) == {0.0}
    assert L.latent_mse_result(torch.from_numpy(f1), torch.from_numpy(f2), setting)["value"] == got["value"]
    with pytest.raises(ValueError):
        L.latent_mse_result(f1, f2[:, :4], setting)


def test_cli_flags_and_metric_selection():
    args = M.parse_args(["--data_path", "x"])
    assert args.latent_mse_weights is None and args.latent_mse_channel_order == "bgr" and args.metrics == "psnr,ssim"
    args = M.parse_args(["--data_path", "x", "--metrics", "psnr,latent_mse", "--latent_mse_weights", "a.pth", "b.safetensors",
                         "--latent_mse_channel_order", "rgb"])
    assert args.latent_mse_weights == ["a.pth", "b.safetensors"] and args.latent_mse_channel_order == "rgb"
    with pytest.raises(SystemExit):
        M.parse_args(["--latent_mse_channel_order", "gbr"])
    assert M.selected_metrics("psnr,latent_mse,loop_closure_latent_mse", latent_mse_weights=True) == ["psnr", "latent_mse", "loop_closure_latent_mse"]
    assert M.selected_metrics("loop_closure_latent_mse", latent_mse_weights=True) == ["loop_closure_latent_mse"]
    for name in ("latent_mse", "loop_closure_latent_mse"):
        for kw in ({}, {"lpips_weights": True, "fvd_weights": True}, {"latent_mse_weights": False}):
            with pytest.raises(ValueError, match="VAE") as e:
                M.selected_metrics(f"psnr,{name}", **kw)
            assert "Inception-v4" in str(e.value) and "inception_v4" in str(e.value) and "--latent_mse_weights" in str(e.value)
    with pytest.raises(ValueError, match="LPIPS"):
        M.selected_metrics("latent_mse,lpips", latent_mse_weights=True)
    with pytest.raises(ValueError, match="I3D"):
        M.selected_metrics("fvd", latent_mse_weights=True)
    assert set(M.NOT_COMPUTED) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"} and M.SUPPORTED == ("psnr", "ssim")
    assert "encoder" not in M.NOT_COMPUTED["latent_mse"] and "encoder" not in M.NOT_COMPUTED["loop_closure_latent_mse"]
    sh = open(os.path.join(ROOT, "calculate_metrics.sh")).read()
    assert "--latent_mse_weights $LATENT_MSE_WEIGHTS" in sh and "LATENT_MSE_CHANNEL_ORDER" in sh and "latent_mse,loop_closure_latent_mse" in sh


def test_abi_declares_the_inception_entries():
    from evoworld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "evoworld_hip.h")).read()
    for s in ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.HEADER.functions, s
    version = int(re.search(r"#define EW_ABI_VERSION (\d+)", hdr).group(1))
    assert version == _lib.ABI_VERSION and version >= 17
    lib = _lib.load()
    assert lib.ew_abi_version() == version
    for s in ENTRIES:
        assert (getattr(lib, s).restype, list(getattr(lib, s).argtypes)) == _lib.HEADER.signatures[s], s
    assert [len(_lib.HEADER.functions[s][1]) for s in ENTRIES] == [19, 7, 7]
    assert "calculate_latent_mse.py:11-79" in hdr and "calculate_all_metrics.py:220-221" in hdr


def test_ops_refuse_cpu_tensors():
    from evoworld_amd import ops
    from evoworld_amd._lib import EvoWorldHipError
    x = torch.zeros(2, 8, 8, 1536, dtype=torch.float16)
    table = tuple(torch.from_numpy(np.array(a)) for a in L.resize_table(8, 4))
    with pytest.raises(EvoWorldHipError):
        ops.frames_resize_aa_norm(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), table, table, L.MEAN, L.STD)
    with pytest.raises(EvoWorldHipError):
        ops.avgpool3x3_relu(x)
    with pytest.raises(EvoWorldHipError):
        ops.global_avgpool_relu(x)
    with pytest.raises(EvoWorldHipError):
        L.InceptionV4.from_random(0, device="cpu").features(torch.zeros(1, 32, 32, 3, dtype=torch.uint8))
