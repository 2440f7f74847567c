"""-m gpu: the latent MSE's Inception-v4 network (user-supplied weights) on the device -- evoworld_amd.latent_mse over
ew_frames_resize_aa_norm_f16, ew_im2col3d_f16, ew_gemm_f16, ew_maxpool3d_relu_f16, ew_avgpool3x3_relu_f16 and ew_global_avgpool_relu_f32
(csrc/inception.hip) -- against the fp32 PyTorch restatement tests/inception_v4_ref.py run on the host with seeded random weights.  timm,
torchvision and the pretrained weights do not exist where these tests run: parity with timm itself is unpinned, the oracle is the restatement.

Parity bounds.  Every bound of test_network_matches_the_restatement is twice the worst value measured on the MI355X over its eight cases
(MEASURED below; the factor covers the seed-to-seed spread of the fp16 rounding): the rel-L2 of each of the 22 features.{i} outputs (ours
after max(x, 0)) and of the 1536-vector over the case's frames, and the relative error of each pair's mean squared feature difference, for
pairs of independent scenes and for perturbed copies (+-8 grey levels: a small feature distance, where the feature error is amplified).
The reference is always the restatement, never the code under test.
The 1536-vector measures 4.97e-4 ... 5.40e-4 rel-L2, the fp16 class of the other networks.  The stage outputs grow from 4.0e-4 (features.0)
to 1.42e-3 (features.17): the fp16 storage rounding of each unit's output accumulated over the up to 70 units in a row; the mean over the
8 x 8 positions averages part of it out again.  The mean squared difference of independent scenes (5e-4 ... 4e-2 with these weights) is
off by 7.5e-4 ... 3.2e-3; that of a copy perturbed by +-8 grey levels (3e-5 ... 7e-5, 5e-6 at 576 x 1024) by 3.1e-4 ... 2.6e-2: there the
features differ by a few per cent of their norm, and the feature error is amplified by that ratio.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import inception_v4_ref as R
import kernel_checks as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

# worst values on the MI355X over the eight cases of test_network_matches_the_restatement
MEASURED = {
    "features.0": 3.999e-04, "features.1": 5.069e-04, "features.2": 5.997e-04, "features.3": 6.006e-04, "features.4": 8.323e-04, "features.5": 8.365e-04,
    "features.6": 8.912e-04, "features.7": 9.499e-04, "features.8": 1.028e-03, "features.9": 1.101e-03, "features.10": 1.091e-03, "features.11": 1.139e-03,
    "features.12": 1.235e-03, "features.13": 1.216e-03, "features.14": 1.238e-03, "features.15": 1.290e-03, "features.16": 1.367e-03, "features.17": 1.423e-03,
    "features.18": 1.372e-03, "features.19": 1.399e-03, "features.20": 1.378e-03, "features.21": 1.407e-03,
    "vector": 5.401e-04, "mse_independent": 3.179e-03, "mse_perturbed": 2.584e-02,
}
BOUND = {k: 2 * v for k, v in MEASURED.items()}


def _scene_u8(g, T, H, W):
    """frames of smooth patterns with a random phase each under a random texture (as test_gpu_lpips._scene_u8)"""
    y = torch.arange(H, dtype=torch.float32)[:, None, None]
    x = torch.arange(W, dtype=torch.float32)[None, :, None]
    c = torch.arange(3, dtype=torch.float32)[None, None, :]
    out = []
    for _ in range(T):
        ph = float(torch.rand((), generator=g)) * 6.28
        base = 128 + 70 * torch.sin(0.05 * x * (c + 1) + 0.08 * y + ph) + 25 * torch.randn(H, W, 3, generator=g)
        out.append(base.round().clamp(0, 255).to(torch.uint8))
    return torch.stack(out)


def _perturbed(g, u8, amp):
    return (u8.to(torch.int16) + torch.randint(-amp, amp + 1, u8.shape, generator=g, dtype=torch.int16)).clamp(0, 255).to(torch.uint8)


def _ordinal(h):
    """fp16 -> an integer that counts representable values in order (adjacent values differ by one, -0 and +0 coincide)"""
    b = h.view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


@pytest.fixture(scope="module")
def models():
    from evoworld_amd import latent_mse as L
    cache = {}

    def get(seed):
        if seed not in cache:
            sd = L.random_state_dict(seed)
            cache[seed] = (sd, L.InceptionV4.from_state_dict(sd, DEV), R.build(sd))
        return cache[seed]
    return get


# ------------------------------------------------------------------ each kernel alone
@pytest.mark.parametrize("H,W,oh,ow", [(57, 91, 29, 29), (20, 30, 29, 29), (200, 640, 299, 299), (576, 1024, 299, 299)])
def test_resize_within_one_fp16_step(H, W, oh, ow):
    """against the restatement's fp32 result (F.interpolate(antialias=True), normalise) rounded to fp16: every value within one fp16 step,
    the padding channels exactly zero"""
    from evoworld_amd import _lib, ops
    from evoworld_amd import latent_mse as L
    lib = _lib.load()
    g = torch.Generator().manual_seed(H)
    n = 2
    u8 = _scene_u8(g, n, H, W)
    f32 = torch.rand(n, 3, H, W, generator=g)
    th, tw = (tuple(torch.from_numpy(np.array(a)).to(DEV) for a in L.resize_table(*s)) for s in ((H, oh), (W, ow)))
    mean_std = (ctypes.c_float * 6)(*L.MEAN, *L.STD)
    for frames in (u8, f32):
        for order in ("rgb", "bgr"):
            got = ops.frames_resize_aa_norm(frames.to(DEV), th, tw, L.MEAN, L.STD, order == "bgr")
            assert got.dtype == torch.float16 and tuple(got.shape) == (n, oh, ow, 8) and not got[..., 3:].any()
            want = R.preprocess(frames, order, (oh, ow)).permute(0, 2, 3, 1).half().to(DEV)
            steps = (_ordinal(got[..., :3].contiguous()) - _ordinal(want.contiguous())).abs()
            print(f"resize {H}x{W} -> {oh}x{ow} {str(frames.dtype)[6:]} {order}: {int((steps > 0).sum())} of {steps.numel()} values differ, "
                  f"worst {int(steps.max())} fp16 steps")
            assert int(steps.max()) <= 1, (H, W, frames.dtype, order)

            def run(view, prefill):
                src = frames.to(DEV)
                _lib.check(lib.ew_frames_resize_aa_norm_f16(P(src), 1 if frames.dtype == torch.uint8 else 2, P(view), n, H, W, oh, ow, P(th[0]), P(th[1]),
                                                            P(th[2]), th[2].shape[1], P(tw[0]), P(tw[1]), P(tw[2]), tw[2].shape[1], int(order == "bgr"),
                                                            mean_std, None), "ew_frames_resize_aa_norm_f16")
            if order == "rgb":                                                                   # guarded output, two prefills: the same bits
                raw = KC.two_prefills(run, (n * oh * ow, 8, torch.float16, {"ld": 8}))[0].view
                assert torch.equal(raw.reshape(n, oh, ow, 8), got)


@pytest.mark.parametrize("shape", [(2, 8, 8, 1536), (1, 17, 17, 1024), (1, 35, 35, 384), (1, 3, 5, 8)])
def test_avgpool3x3_relu_within_one_fp16_step(shape):
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    n, H, W, C = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(H * C)).half()
    assert bool((x < 0).any())
    x[..., 5] = -x[..., 5].abs()                                                                 # a channel the ReLU removes everywhere
    nchw = x.double().clamp_min(0).permute(0, 3, 1, 2)
    want64 = F.avg_pool2d(nchw, 3, stride=1, padding=1, count_include_pad=False)
    counts = (F.avg_pool2d(torch.ones(1, 1, H, W, dtype=torch.float64), 3, stride=1, padding=1, count_include_pad=True) * 9).round()
    assert {4.0, 6.0, 9.0} <= set(counts.unique().tolist())                                      # corners, edges and the interior
    assert torch.allclose(want64, F.avg_pool2d(nchw, 3, stride=1, padding=1, count_include_pad=True) * 9 / counts, rtol=1e-13, atol=0)
    want = want64.permute(0, 2, 3, 1).half().contiguous().to(DEV)
    xd = x.to(DEV)

    def run(view, prefill):
        _lib.check(lib.ew_avgpool3x3_relu_f16(P(xd), P(view), n, H, W, C, None), "ew_avgpool3x3_relu_f16")
    got = KC.two_prefills(run, (n * H * W, C, torch.float16, {"ld": C}))[0].view.reshape(shape)
    steps = (_ordinal(got.contiguous()) - _ordinal(want)).abs()
    print(f"avgpool3x3_relu {shape}: {int((steps > 0).sum())} of {steps.numel()} values differ, worst {int(steps.max())} fp16 steps")
    assert int(steps.max()) <= 1 and not got[..., 5].any()
    assert torch.equal(ops.avgpool3x3_relu(xd), got)


@pytest.mark.parametrize("shape", [(3, 8, 8, 1536), (1, 1, 1, 8)])
def test_global_avgpool_relu_against_fp64(shape):
    """a sequential fp32 sum of h * w non-negative terms and one division: relative error <= h * w * 2^-24 per value, with an absolute
    floor of one fp32 ulp of the value"""
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    n, h, w, C = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(C + h)).half()
    x[..., 3] = -x[..., 3].abs()
    want = x.double().clamp_min(0).mean((1, 2))
    xd = x.to(DEV)

    def run(view, prefill):
        _lib.check(lib.ew_global_avgpool_relu_f32(P(xd), P(view), n, h, w, C, None), "ew_global_avgpool_relu_f32")
    got = KC.two_prefills(run, (n, C, torch.float32, {"ld": C}))[0].view.cpu()
    err = (got.double() - want).abs()
    ulp = torch.from_numpy(np.spacing(want.float().numpy())).double()
    bound = torch.maximum(h * w * 2.0 ** -24 * want, ulp)
    rel = float((err / want.clamp_min(1e-30))[want > 0].max())
    print(f"global_avgpool_relu {shape}: worst relative error {rel:.3e} (bound {h * w * 2.0 ** -24:.3e})")
    assert bool((err <= bound).all()) and not got[:, 3].any()
    assert torch.equal(ops.global_avgpool_relu(xd).cpu(), got)


def test_kernel_entries_refuse_bad_arguments():
    from evoworld_amd import _lib, ops
    from evoworld_amd import latent_mse as L
    lib = _lib.load()
    x = torch.zeros(2, 8, 8, 16, dtype=torch.float16, device=DEV)
    out = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    t = tuple(torch.from_numpy(np.array(a)).to(DEV) for a in L.resize_table(8, 4))
    good, zero_std = (ctypes.c_float * 6)(*L.MEAN, *L.STD), (ctypes.c_float * 6)(*L.MEAN, 0.0, 1.0, 1.0)
    resize = lambda kind=1, taps=t[2].shape[1], ms=good, o=out, H=8: lib.ew_frames_resize_aa_norm_f16(
        P(u8), kind, P(o), 2, H, 8, 4, 4, P(t[0]), P(t[1]), P(t[2]), taps, P(t[0]), P(t[1]), P(t[2]), t[2].shape[1], 0, ms, None)
    cases = [(lambda: resize(kind=0), "src_kind 0"), (lambda: resize(taps=0), "taps per output index"), (lambda: resize(ms=zero_std), "must be positive"),
             (lambda: resize(ms=None), "NULL"), (lambda: resize(o=out[1:]), "16-byte"), (lambda: resize(H=0), "bad frame size"),
             (lambda: lib.ew_avgpool3x3_relu_f16(P(x), P(out), 2, 8, 8, 12, None), "C % 8"),
             (lambda: lib.ew_avgpool3x3_relu_f16(P(x), None, 2, 8, 8, 16, None), "NULL"),
             (lambda: lib.ew_avgpool3x3_relu_f16(P(x), P(out), 0, 8, 8, 16, None), "n, H, W > 0"),
             (lambda: lib.ew_global_avgpool_relu_f32(P(x), P(f), 2, 8, 8, 20, None), "C % 8"),
             (lambda: lib.ew_global_avgpool_relu_f32(P(x), P(f[1:]), 2, 8, 8, 16, None), "16-byte"),
             (lambda: lib.ew_global_avgpool_relu_f32(None, P(f), 2, 8, 8, 16, None), "NULL")]
    for call, msg in cases:
        assert call() == _lib.EW_ERR_INVALID_ARG and msg in lib.ew_last_error().decode(), (msg, lib.ew_last_error())
    with pytest.raises(TypeError):
        ops.avgpool3x3_relu(x.float())
    with pytest.raises(ValueError):
        ops.frames_resize_aa_norm(u8, (t[0], t[1][:2], t[2]), t, L.MEAN, L.STD)
    with pytest.raises(ValueError, match="channel_order"):
        L.InceptionV4({}, DEV).preprocess(u8, "gbr")


# ------------------------------------------------------------------ the network
def _case_frames(seed, kind):
    """(a, b, [pair kinds]): frame pairs of one case.  Pair 0 holds independent scenes, pair 1 a copy perturbed by +-8 grey levels; the
    576 x 1024 case is one perturbed pair."""
    g = torch.Generator().manual_seed(100 * seed + len(kind))
    if kind == "u8_576x1024":
        a = _scene_u8(g, 1, 576, 1024)
        return a, _perturbed(g, a, 8), ["perturbed"]
    H, W = (64, 96) if kind.startswith("u8_64x96") else (70, 93)
    a, other = _scene_u8(g, 2, H, W), _scene_u8(g, 1, H, W)
    b = torch.cat([other, _perturbed(g, a[1:], 8)])
    if kind.startswith("f32"):
        a, b = (v.permute(0, 3, 1, 2).float().div(255.0).contiguous() for v in (a, b))
    return a, b, ["independent", "perturbed"]


CASES = [(s, k) for s in (0, 1, 2) for k in ("u8_64x96", "f32_70x93")] + [(0, "u8_576x1024"), (0, "u8_64x96_bgr")]


@pytest.mark.parametrize("seed,kind", CASES)
def test_network_matches_the_restatement(seed, kind, models):
    _, model, net = models(seed)
    order = "bgr" if kind.endswith("_bgr") else "rgb"
    a, b, pair_kinds = _case_frames(seed, kind)
    frames, n = torch.cat([a, b]), a.shape[0]
    eps, ref = {}, {}
    got = model.features(frames.to(DEV), order, endpoints=eps)
    want = R.features(net, frames, order, endpoints=ref)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2 * n, 1536) and got.is_cuda and list(eps) == list(ref)
    errs = {}
    for name in ref:
        w = ref[name].permute(0, 2, 3, 1)
        assert tuple(eps[name].shape) == tuple(w.shape), (name, eps[name].shape, w.shape)
        errs[name] = KC.rel_l2(eps[name].float().clamp_min(0).cpu(), w)
    errs["vector"] = KC.rel_l2(got.cpu(), want)
    g64, w64 = got.double().cpu(), want.double()
    for j, pk in enumerate(pair_kinds):
        ours, theirs = float(((g64[j] - g64[n + j]) ** 2).mean()), float(((w64[j] - w64[n + j]) ** 2).mean())
        errs[f"mse_{pk}"] = abs(ours - theirs) / theirs
        print(f"LMSE seed {seed} {kind} pair {j} ({pk}): mse {ours:.6e} against {theirs:.6e}")
    print(f"LMSE seed {seed} {kind}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    first_bad = next((k for k, v in errs.items() if not v <= BOUND[k]), None)
    assert first_bad is None, f"{first_bad} is the first value beyond its bound: {errs[first_bad]:.3e} > {BOUND[first_bad]:.3e}"
    if order == "bgr":
        assert not torch.equal(got, model.features(frames.to(DEV), "rgb"))


def test_properties_bit_for_bit(models):
    from evoworld_amd import latent_mse as L
    _, model, _ = models(0)
    g = torch.Generator().manual_seed(77)
    clip = _scene_u8(g, 5, 64, 96).to(DEV)
    other = _scene_u8(g, 5, 64, 96).to(DEV)
    all5 = model.features(clip)
    alone = model.features(clip[3:4])
    assert torch.equal(all5[3:4], alone)                                                         # frame 3 of 5 and the frame alone
    model.features(other, "bgr")
    assert torch.equal(model.features(clip[3:4]), alone) and torch.equal(model.features(clip), all5)       # and in a second call
    one = type(model)(model.p, DEV, chunk=1)                                                     # the chunk only groups gathers and pools
    assert torch.equal(one.features(clip), all5)
    f32 = (clip.cpu().permute(0, 3, 1, 2).float() / 255.0).contiguous().to(DEV)                  # IEEE division, on the host
    assert torch.equal(model.features(f32), all5)                                                # uint8 frames are float32(k) / 255
    v1, v2 = f32.cpu()[None], (other.cpu().permute(0, 3, 1, 2).float() / 255.0)[None]
    same = L.calculate_latent_mse(v1, v1.clone(), model)
    assert same["value_mean"] == 0.0 and set(same["value"].values()) == {0.0} and set(same["value_std"].values()) == {0.0}
    ab, ba = L.calculate_latent_mse(v1, v2, model), L.calculate_latent_mse(v2, v1, model)
    assert ab["value"] == ba["value"] and ab["value_std"] == ba["value_std"] and ab["value_mean"] == ba["value_mean"] and ab["value_mean"] > 0
    assert ab["video_setting"] == torch.Size([5, 3, 299, 299]) and list(ab["value"]) == [0, 1, 2, 3, 4]
    with pytest.raises(AssertionError):
        L.calculate_latent_mse(v1, v2[:, :4], model)


# ------------------------------------------------------------------ the evaluation CLI
def _write_tree(root, gt, gen):
    for e in range(gt.shape[0]):
        for sub, v in (("predictions_gt_0", gt), ("predictions_0", gen)):
            d = os.path.join(root, f"ep_{e:03d}", sub)
            os.makedirs(d, exist_ok=True)
            for t in range(v.shape[1]):
                Image.fromarray(v[e, t]).save(os.path.join(d, f"{t + 1:03}.png"))


def test_cli_end_to_end(tmp_path):
    from safetensors.torch import save_file
    from evoworld_amd import latent_mse as L
    from evoworld_amd import metrics as M
    E, T, H, W = 2, 12, 64, 96
    g = torch.Generator().manual_seed(31)
    gt = torch.stack([_scene_u8(g, T, H, W) for _ in range(E)])
    gen = _perturbed(g, gt, 24)
    _write_tree(str(tmp_path), gt.numpy(), gen.numpy())
    weights = str(tmp_path / "inception_v4.safetensors")
    save_file({k: v.contiguous() for k, v in L.random_state_dict(0).items()}, weights)
    argv = ["--data_path", str(tmp_path), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0"]
    M.main(argv + ["--metrics", "psnr,ssim,latent_mse,loop_closure_latent_mse", "--latent_mse_weights", weights, "--result_file", "scores.json"])
    got = json.load(open(tmp_path / "scores.json"))
    assert list(got) == ["ssim", "psnr", "latent_mse", "loop_closure_latent_mse", "not_computed"]
    assert set(got["not_computed"]) == {"fvd", "lpips"}
    lm, lc = got["latent_mse"], got["loop_closure_latent_mse"]
    for d, n_t, setting in ((lm, T, [E * T, 3, 299, 299]), (lc, 1, [E, 3, 299, 299])):
        assert list(d) == ["value", "value_mean", "value_std", "video_setting", "video_setting_name"]
        assert list(d["value"]) == [str(t) for t in range(n_t)] == list(d["value_std"])
        assert d["video_setting"] == setting and d["video_setting_name"] == "time, channel, heigth, width"
        assert d["value_mean"] == float(np.mean(list(d["value"].values()))) and d["value_mean"] > 0
    # the B, G, R default equals calculate_latent_mse called directly on B, G, R; loop closure is the last timestamp's features
    model = L.InceptionV4.from_files(weights, DEV)
    v1, v2 = (v.permute(0, 1, 4, 2, 3).float() / 255.0 for v in (gt, gen))
    direct = L.calculate_latent_mse(v1, v2, model, "bgr")
    assert {str(k): v for k, v in direct["value"].items()} == lm["value"] and direct["value_mean"] == lm["value_mean"]
    assert {str(k): v for k, v in direct["value_std"].items()} == lm["value_std"] and direct["video_setting"] == torch.Size([E * T, 3, 299, 299])
    last = L.calculate_latent_mse(v1[:, -1:], v2[:, -1:], model, "bgr")
    assert last["value"][0] == lc["value"]["0"] and last["value_std"][0] == lc["value_std"]["0"] and last["value_mean"] == lc["value_mean"]
    assert last["video_setting"] == torch.Size([E, 3, 299, 299])
    f1, f2 = (model.features(v[:, -1].to(DEV), "bgr").double().cpu().numpy() for v in (gt, gen))
    assert lc["value"]["0"] == pytest.approx(float(((f1 - f2) ** 2).mean()), rel=1e-12)
    assert lc["value"]["0"] == pytest.approx(lm["value"][str(T - 1)], rel=1e-12) and lc["value_std"]["0"] == pytest.approx(lm["value_std"][str(T - 1)], rel=1e-12)
    # rgb is another number; one latent metric alone
    rgb, _ = M.main(argv + ["--metrics", "loop_closure_latent_mse", "--latent_mse_weights", weights, "--latent_mse_channel_order", "rgb"])
    assert list(rgb) == ["loop_closure_latent_mse", "not_computed"] and set(rgb["not_computed"]) == {"fvd", "lpips", "latent_mse"}
    assert rgb["loop_closure_latent_mse"]["value"][0] != lc["value"]["0"]
    # without the flag nothing changes: the three keys, all four names not computed, both latent metrics refused
    plain, _ = M.main(argv + ["--result_file", "plain.json"])
    assert list(plain) == ["ssim", "psnr", "not_computed"] and plain["not_computed"] == M.NOT_COMPUTED
    plain = json.load(open(tmp_path / "plain.json"))
    assert plain["psnr"] == got["psnr"] and plain["ssim"] == got["ssim"] and set(plain["not_computed"]) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"}
    for name in ("latent_mse", "loop_closure_latent_mse"):
        with pytest.raises(ValueError, match="VAE"):
            M.main(argv + ["--metrics", f"psnr,{name}"])
