"""-m 'not gpu': the host side of the FVD feature -- the SAME-padding rule and the preprocess geometry against the reference's own
values (tests/golden/fvd.npz, written by tools/make_goldens_fvd.py from the reference's InceptionI3d, preprocess_single and
frechet_distance), the fp32 restatement tests/i3d_ref.py against the same file, the Frechet distance, the state-dict loader and packer,
the CLI glue and the ABI entries."""
import os
import re

import numpy as np
import pytest
import torch

import i3d_ref
from evoworld_amd import fvd as V
from evoworld_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ew_video_preprocess_f16", "ew_im2col3d_f16", "ew_maxpool3d_relu_f16", "ew_i3d_head", "ew_i3d_head_workspace_bytes")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "fvd.npz"))


@pytest.fixture(scope="module")
def sd0():
    return V.random_state_dict(0)


def test_same_pad_matches_the_reference_table(gold):
    assert [tuple(r) for r in gold["pad_ks"]] == [(7, 2), (3, 1), (3, 2), (2, 2)]
    for (k, s), row in zip(gold["pad_ks"], gold["pad_table"]):
        for size in range(1, 17):
            out, front, back = V.same_pad(size, int(k), int(s))
            total = int(row[size - 1])
            assert (out, front, back) == (-(-size // int(s)), total // 2, total - total // 2), (k, s, size)
            assert i3d_ref.pad_total(size, int(k), int(s)) == total
    assert V.same_pad(10, 1, 1) == (10, 0, 0) and V.same_pad(3, 2, 2) == (2, 0, 1) and V.same_pad(224, 7, 2) == (112, 2, 3)
    with pytest.raises(ValueError):
        V.same_pad(0, 3, 1)


def test_preprocess_geometry_matches_the_reference(gold):
    for (H, W), (hr, wr) in zip(gold["geo_hw"], gold["geo_target"]):
        assert V.preprocess_geometry(int(H), int(W)) == (hr, wr, (hr - 224) // 2, (wr - 224) // 2), (H, W)
    assert V.preprocess_geometry(576, 1024) == (224, 399, 0, 87)
    assert V.preprocess_geometry(100, 100)[0] == 225                                       # 100 * (224 / 100) is just above 224 in float64
    with pytest.raises(ValueError):
        V.preprocess_geometry(0, 5)


def test_restatement_matches_the_reference(gold, sd0):
    """the preprocess samples exactly (the same F.interpolate); the logits to 1e-4 rel-L2 (the same convolutions, BatchNorm spelled out in
    another order: about 1e-5 expected)"""
    for i, shape in enumerate(((10, 45, 80, 3), (13, 60, 52, 3))):
        clip = torch.from_numpy(gold[f"clip{i}"])
        assert tuple(clip.shape) == shape and clip.dtype == torch.uint8
        x = i3d_ref.clip_input(clip)
        assert tuple(x.shape) == (1, 3, shape[0], 224, 224)
        assert np.array_equal(x[0].reshape(-1)[torch.from_numpy(gold[f"pre_idx{i}"])].numpy(), gold[f"pre_val{i}"])
        assert float(x.double().sum()) == pytest.approx(float(gold[f"pre_sum{i}"]), rel=1e-12)
        got, want = i3d_ref.endpoints(x, sd0)["Logits"][0].double().numpy(), gold[f"logits{i}"].astype(np.float64)
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        print(f"I3D restatement against the reference, clip {i}: rel-L2 {rel:.3e}")
        assert rel <= 1e-4


def test_frechet_distance_matches_the_reference(gold):
    for (n, d), bound in (((64, 8), 1e-9), ((16, 400), 1e-6), ((1, 400), 1e-9)):
        a, b, want = gold[f"fd_a_{n}x{d}"], gold[f"fd_b_{n}x{d}"], float(gold[f"fd_{n}x{d}"])
        for fn in (V.frechet_distance, i3d_ref.frechet):
            assert abs(fn(a, b) - want) <= bound * abs(want), (n, d, fn)
        assert abs(V.frechet_distance(torch.from_numpy(a), torch.from_numpy(b)) - want) <= bound * abs(want)
    a, b = gold["fd_a_64x8"], gold["fd_b_64x8"]
    assert V.frechet_distance(a, b) != V.frechet_distance(a[:32], b[:32])
    assert V.frechet_distance(a[:1], b[:1]) == float(np.square(a[0] - b[0]).sum())          # the N = 1 branch
    r = V.fvd_result({10: a, 11: a[:16]}, {10: b, 11: b[:16]}, torch.Size([64, 3, 11, 4, 4]))
    assert list(r["value"]) == [10, 11] and r["value"][10] == V.frechet_distance(a, b) and r["fvd_setting"] == "styleganv"
    assert r["value_mean"] == float(np.mean([r["value"][10], r["value"][11]])) and r["video_setting_name"] == "batch_size, channel, time, height, width"


def test_random_state_dict_is_seeded_and_has_the_reference_keys(gold, sd0):
    again, other = V.random_state_dict(0), V.random_state_dict(1)
    assert set(sd0) == set(gold["sd_names"].tolist()) and len(sd0) == 57 * 5 + 2
    for name, shape in zip(gold["sd_names"].tolist(), gold["sd_shapes"]):
        assert tuple(sd0[name].shape) == tuple(int(v) for v in shape[:sd0[name].ndim]), name
    assert all(torch.equal(sd0[k], again[k]) for k in sd0) and not torch.equal(sd0["Mixed_4c.b2b.conv3d.weight"], other["Mixed_4c.b2b.conv3d.weight"])
    assert len(V.units()) == 57 and V.ENDPOINTS == i3d_ref.ORDER


def test_pack_folds_batchnorm_and_orders_columns(sd0):
    packed = V.pack_state_dict(sd0)
    assert set(packed) == {f"{n}.{p}" for n, *_ in V.units() for p in ("w", "b")} | {"logits.w", "logits.b"}
    for name, ci, co, k in V.units():
        cp = -(-ci // 8) * 8
        K = k ** 3 * cp
        w, b = packed[f"{name}.w"], packed[f"{name}.b"]
        assert w.dtype == torch.float16 and tuple(w.shape) == (co, -(-K // 64) * 64) and not w[:, K:].any(), name
        assert b.dtype == torch.float16 and tuple(b.shape) == (co,)
        # the fold against float64 BatchNorm of the convolution's output, unit by unit
        g, beta, mean, var = (sd0[f"{name}.bn.{p}"].double() for p in ("weight", "bias", "running_mean", "running_var"))
        s = g / torch.sqrt(var + 1e-5)
        want = torch.zeros(co, k, k, k, cp, dtype=torch.float64)
        want[..., :ci] = (sd0[f"{name}.conv3d.weight"].double() * s.view(-1, 1, 1, 1, 1)).permute(0, 2, 3, 4, 1)
        assert torch.equal(w[:, :K], want.reshape(co, K).half()), name
        assert torch.equal(b, (beta - mean * s).half()), name
    assert packed["logits.w"].dtype == torch.float32 and tuple(packed["logits.w"].shape) == (400, 1024)
    assert torch.equal(packed["logits.w"], sd0["logits.conv3d.weight"].view(400, 1024)) and torch.equal(packed["logits.b"], sd0["logits.conv3d.bias"])
    assert packed["Conv3d_1a_7x7.w"].shape[1] == 2752 and not packed["Conv3d_1a_7x7.w"][:, :2744].view(64, 343, 8)[:, :, 3:].any()
    # y = BN(conv(x)) at one output position equals the packed row times the patch, in float64
    x = torch.randn(24, 3, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    name = "Mixed_4c.b2b"
    conv = torch.einsum("oczyx,czyx->o", sd0[f"{name}.conv3d.weight"].double(), x)
    g, beta, mean, var = (sd0[f"{name}.bn.{p}"].double() for p in ("weight", "bias", "running_mean", "running_var"))
    want = (conv - mean) / torch.sqrt(var + 1e-5) * g + beta
    got = packed[f"{name}.w"][:, :648].double() @ x.permute(1, 2, 3, 0).reshape(-1) + packed[f"{name}.b"].double()
    assert float((got - want).abs().max()) <= 2e-3 * float(want.abs().max())               # fp16 weights: 2^-11 per term


def test_pack_column_order_on_a_toy_kernel(monkeypatch):
    """a 2 x 2 x 2 kernel over 8 channels whose weight encodes its own index: column ((dt*2 + dy)*2 + dx)*8 + c, K = 64 exactly; and a
    5-channel unit whose channels are padded to 8 and K to 64"""
    monkeypatch.setattr(V, "units", lambda: [("toy", 8, 2, 2), ("odd", 5, 1, 1)])
    sd = {"toy.conv3d.weight": torch.arange(2 * 8 * 8, dtype=torch.float32).view(2, 8, 2, 2, 2), "odd.conv3d.weight": torch.arange(1.0, 6.0).view(1, 5, 1, 1, 1)}
    for n, co in (("toy", 2), ("odd", 1)):
        sd[f"{n}.bn.weight"], sd[f"{n}.bn.bias"] = torch.full((co,), 2.0), torch.full((co,), 0.5)
        sd[f"{n}.bn.running_mean"], sd[f"{n}.bn.running_var"] = torch.full((co,), 0.25), torch.full((co,), 4.0 - 1e-5)
    sd["logits.conv3d.weight"], sd["logits.conv3d.bias"] = torch.zeros(400, 1024, 1, 1, 1), torch.zeros(400)
    p = V.pack_state_dict({"module." + k: v for k, v in sd.items()})                       # the DataParallel prefix is stripped
    assert tuple(p["toy.w"].shape) == (2, 64) and tuple(p["odd.w"].shape) == (1, 64)
    for o in range(2):
        for dt in range(2):
            for dy in range(2):
                for dx in range(2):
                    for c in range(8):
                        assert float(p["toy.w"][o, ((dt * 2 + dy) * 2 + dx) * 8 + c]) == float(sd["toy.conv3d.weight"][o, c, dt, dy, dx]), (o, dt, dy, dx, c)
    assert p["odd.w"][0].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0] + [0.0] * 59                # scale = 2 / sqrt(4) = 1
    assert p["toy.b"].tolist() == [0.25, 0.25] and p["odd.b"].tolist() == [0.25]           # 0.5 - 0.25 * 1


def test_state_dict_prefix_extras_and_refusals(sd0):
    want = V.pack_state_dict(sd0)
    wrapped = {"module." + k: v for k, v in sd0.items()}
    wrapped["module.Conv3d_1a_7x7.bn.num_batches_tracked"] = torch.tensor(7)
    got = V.pack_state_dict(wrapped)
    assert got.keys() == want.keys() and all(torch.equal(got[k], want[k]) for k in want)
    bad = {k: v for k, v in sd0.items() if k not in ("Mixed_3c.b1b.bn.running_var", "logits.conv3d.bias")}
    with pytest.raises(KeyError) as e:
        V.pack_state_dict(bad)
    assert "missing 2 keys" in str(e.value) and "Mixed_3c.b1b.bn.running_var" in str(e.value) and "logits.conv3d.bias" in str(e.value)
    bad = dict(sd0)
    bad["Mixed_4b.b1b.conv3d.weight"] = torch.zeros(208, 96, 3, 3)
    with pytest.raises(ValueError) as e:
        V.pack_state_dict(bad)
    assert "Mixed_4b.b1b.conv3d.weight" in str(e.value) and "(208, 96, 3, 3, 3)" in str(e.value) and "(208, 96, 3, 3)" in str(e.value)
    bad = dict(sd0)
    bad["Conv3d_2b_1x1.bn.bias"] = torch.zeros(65)
    with pytest.raises(ValueError, match=r"Conv3d_2b_1x1\.bn\.bias"):
        V.pack_state_dict(bad)


def test_weight_files_and_the_torchscript_refusal(tmp_path, sd0):
    from safetensors.torch import save_file
    want = V.pack_state_dict(sd0)
    f_st, f_pt, f_ckpt = tmp_path / "i3d.safetensors", tmp_path / "i3d_pretrained_400.pt", tmp_path / "ckpt.pt"
    save_file({k: v.contiguous() for k, v in sd0.items()}, str(f_st))
    torch.save(sd0, f_pt)
    torch.save({"state_dict": sd0, "epoch": 3}, f_ckpt)
    for f in (f_st, str(f_pt), [f_ckpt]):
        got = V.pack_state_dict(V.load_state_files(f))
        assert all(torch.equal(got[k], want[k]) for k in want)
    model = V.I3D.from_files(str(f_st), device="cpu")                                       # packing needs no GPU; calling it does
    assert torch.equal(model.p["Mixed_5c.b3b.w"], want["Mixed_5c.b3b.w"]) and model.workspace_bytes == V.WORKSPACE_BYTES

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(4, 2)

        def forward(self, x):
            return self.lin(x)
    f_ts = tmp_path / "i3d_torchscript.pt"
    torch.jit.script(Tiny()).save(str(f_ts))
    assert V.is_torchscript_archive(f_ts) and not V.is_torchscript_archive(f_pt) and not V.is_torchscript_archive(f_st)
    for call in (lambda: V.load_state_files(f_ts), lambda: V.I3D.from_files([str(f_ts)], device="cpu")):
        with pytest.raises(ValueError) as e:
            call()
        assert "TorchScript archive" in str(e.value) and "InceptionI3d's key layout" in str(e.value) and "Conv3d_1a_7x7.conv3d.weight" in str(e.value)


def test_cli_flags_and_metric_selection():
    args = M.parse_args(["--data_path", "x"])
    assert args.fvd_weights is None and args.fvd_channel_order == "bgr" and args.metrics == "psnr,ssim"
    args = M.parse_args(["--data_path", "x", "--metrics", "psnr,ssim,fvd", "--fvd_weights", "a.pt", "b.safetensors", "--fvd_channel_order", "rgb"])
    assert args.fvd_weights == ["a.pt", "b.safetensors"] and args.fvd_channel_order == "rgb"
    with pytest.raises(SystemExit):
        M.parse_args(["--fvd_channel_order", "gbr"])
    assert M.selected_metrics("psnr,fvd", fvd_weights=True) == ["psnr", "fvd"]
    assert M.selected_metrics("fvd,lpips", lpips_weights=True, fvd_weights=True) == ["fvd", "lpips"]
    with pytest.raises(ValueError, match="I3D"):
        M.selected_metrics("psnr,fvd")
    with pytest.raises(ValueError, match="I3D"):
        M.selected_metrics("fvd", lpips_weights=True, fvd_weights=False)
    with pytest.raises(ValueError, match="LPIPS"):
        M.selected_metrics("fvd,lpips", fvd_weights=True)
    with pytest.raises(ValueError, match="VAE"):
        M.selected_metrics("latent_mse", lpips_weights=True, fvd_weights=True)
    assert "fvd" in M.NOT_COMPUTED and M.SUPPORTED == ("psnr", "ssim")
    sh = open(os.path.join(ROOT, "calculate_metrics.sh")).read()
    assert "--fvd_weights $FVD_WEIGHTS" in sh and "FVD_CHANNEL_ORDER" in sh


def test_abi_declares_the_i3d_entries():
    from evoworld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "evoworld_hip.h")).read()
    for s in ENTRIES:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.HEADER.functions, s
    version = int(re.search(r"#define EW_ABI_VERSION (\d+)", hdr).group(1))
    assert version == _lib.ABI_VERSION and version >= 16
    lib = _lib.load()
    assert lib.ew_abi_version() == version
    for s in ENTRIES:
        assert (getattr(lib, s).restype, list(getattr(lib, s).argtypes)) == _lib.HEADER.signatures[s], s
    assert len(_lib.HEADER.functions["ew_im2col3d_f16"][1]) == 21 and len(_lib.HEADER.functions["ew_maxpool3d_relu_f16"][1]) == 19
    assert lib.ew_i3d_head_workspace_bytes() == 4096


def test_ops_refuse_cpu_tensors():
    from evoworld_amd import ops
    from evoworld_amd._lib import EvoWorldHipError
    x = torch.zeros(2, 7, 7, 1024, dtype=torch.float16)
    with pytest.raises(EvoWorldHipError):
        ops.video_preprocess(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), 224, 224, 0, 0)
    with pytest.raises(EvoWorldHipError):
        ops.im2col3d(x, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 7, 7), 1024)
    with pytest.raises(EvoWorldHipError):
        ops.maxpool3d_relu(x, (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 7, 7))
    with pytest.raises(EvoWorldHipError):
        ops.i3d_head(x, torch.zeros(400, 1024), torch.zeros(400))
    with pytest.raises(EvoWorldHipError):
        V.I3D.from_random(0, device="cpu").logits(torch.zeros(10, 32, 32, 3, dtype=torch.uint8))
