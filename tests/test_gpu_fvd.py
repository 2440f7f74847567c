"""-m gpu: FVD's I3D network (user-supplied weights) on the device -- evoworld_amd.fvd over ew_video_preprocess_f16, ew_im2col3d_f16,
ew_gemm_f16, ew_maxpool3d_relu_f16 and ew_i3d_head (csrc/i3d.hip) -- against the fp32 PyTorch restatement tests/i3d_ref.py run on the
host with seeded random weights (tests/test_cpu_fvd.py pins that restatement to the reference's own network).

Parity bound.  REL_BOUND is a rel-L2 per clip over the 400 logits: twice the worst value measured on the MI355X over the seven cases of
test_logits_and_endpoints_match_the_restatement (the factor covers the seed-to-seed spread of the fp16 rounding).  Measured logits rel-L2:
  224 x 224, T = 10 / 13:  seed 0 4.346e-4 / 4.704e-4, seed 1 4.283e-4 / 5.160e-4 (the worst), seed 2 4.186e-4 / 4.249e-4
  96 x 160,  T = 25:       seed 0 3.855e-4
A CPU emulation (fp16-rounded folded weights, every unit's output rounded to fp16) had predicted 5.4e-4 ... 6.4e-4.  The same bound is asserted
for every endpoint tensor of the clip, so that a wrong pad shows where it starts.  Worst rel-L2 per endpoint over the seven cases:
  Conv3d_1a_7x7 3.60e-4  MaxPool3d_2a_3x3 3.30e-4  Conv3d_2b_1x1 4.43e-4  Conv3d_2c_3x3 5.31e-4  MaxPool3d_3a_3x3 5.08e-4  Mixed_3b 6.18e-4
  Mixed_3c 6.81e-4  MaxPool3d_4a_3x3 5.89e-4  Mixed_4b 7.20e-4  Mixed_4c 8.02e-4  Mixed_4d 9.62e-4  Mixed_4e 9.21e-4  Mixed_4f 9.88e-4
  MaxPool3d_5a_2x2 9.02e-4  Mixed_5b 9.70e-4  Mixed_5c 1.031e-3 (seed 1, T = 13)
Mixed_5c sits 0.1 % inside the bound.  The bound follows the rule above (twice the worst LOGITS value, applied to every endpoint); it was not
fitted to the endpoints.  The kernels are deterministic, so the figure repeats; but another GEMM tile choice or patch-row cap moves the
summation order, and a failure on Mixed_5c alone by a fraction of a percent, with the logits and the earlier endpoints where they are
above, reflects that rule and the fp16 activation storage, not a wrong pad or a regression.
It is the fp16 storage rounding of each unit's output (2.9e-4 rel-L2 per rounding) accumulated over the 21 units in a row; the mean over
98 (T' - 1) positions in the head averages part of it out again, which is why the logits are closer than Mixed_5c.
FVD_REL_BOUND is twice the worst relative difference of the CLI's distances from the restatement's through the same frechet_distance
(test_cli_end_to_end: 3 episodes of 12 frames at 64 x 96), measured the same way: 1.525e-4, 1.036e-4 and 5.817e-5 at clip lengths 10, 11 and 12.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import i3d_ref
import kernel_checks as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEASURED = {"logits": 5.160e-4, "fvd": 1.525e-4}           # worst values on the MI355X (docstring)
REL_BOUND = 2 * MEASURED["logits"]                         # 1.032e-3
FVD_REL_BOUND = 2 * MEASURED["fvd"]                        # 3.05e-4
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
POOLS = (((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((2, 2, 2), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)))


def _scene_u8(g, T, H, W):
    """a clip of smooth patterns with a random phase each under a random texture (as test_gpu_lpips._scene_u8)"""
    y = torch.arange(H, dtype=torch.float32)[:, None, None]
    x = torch.arange(W, dtype=torch.float32)[None, :, None]
    c = torch.arange(3, dtype=torch.float32)[None, None, :]
    out = []
    for _ in range(T):
        ph = float(torch.rand((), generator=g)) * 6.28
        base = 128 + 70 * torch.sin(0.05 * x * (c + 1) + 0.08 * y + ph) + 25 * torch.randn(H, W, 3, generator=g)
        out.append(base.round().clamp(0, 255).to(torch.uint8))
    return torch.stack(out)


def _geometry(shape, kernel, stride):
    from evoworld_amd.fvd import same_pad
    geo = [same_pad(n, k, s) for n, k, s in zip(shape, kernel, stride)]
    return [g[0] for g in geo], [g[1] for g in geo], [g[2] for g in geo]


def _pad_cthw(x_thwc, front, back):
    return F.pad(x_thwc.permute(3, 0, 1, 2).float(), (front[2], back[2], front[1], back[1], front[0], back[0]))


@pytest.fixture(scope="module")
def models():
    from evoworld_amd import fvd as V
    cache = {}

    def get(seed):
        if seed not in cache:
            sd = V.random_state_dict(seed)
            cache[seed] = (sd, V.I3D.from_state_dict(sd, DEV))
        return cache[seed]
    return get


# ------------------------------------------------------------------ each kernel alone
@pytest.mark.parametrize("shape,k,s,ldk", [((5, 7, 9, 8), 7, 2, 2752), ((3, 6, 5, 16), 3, 1, 448), ((4, 5, 5, 24), 1, 1, 64), ((2, 7, 7, 48), 3, 1, 1344)])
def test_im2col3d_is_exact(shape, k, s, ldk):
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    T, H, W, C = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(T * 100 + C)).half().to(DEV)
    out_size, front, back = _geometry(shape, (k,) * 3, (s,) * 3)
    rows, K = out_size[0] * out_size[1] * out_size[2], k ** 3 * C
    assert K <= ldk and ldk % 64 == 0
    for relu in (0, 1):
        xp = _pad_cthw(x.clamp_min(0) if relu else x, front, back)
        u = xp.unfold(1, k, s).unfold(2, k, s).unfold(3, k, s)                               # [C, To, Ho, Wo, dt, dy, dx]
        assert list(u.shape[1:4]) == out_size
        want = torch.zeros(rows, ldk, dtype=torch.float16, device=DEV)
        want[:, :K] = u.permute(1, 2, 3, 4, 5, 6, 0).reshape(rows, K).half()

        def run(view, prefill):
            _lib.check(lib.ew_im2col3d_f16(P(x), P(view), T, H, W, C, k, k, k, s, s, s, *front, *out_size, ldk, relu, None), "ew_im2col3d_f16")
        got = KC.two_prefills(run, (rows, ldk, torch.float16, {"ld": ldk}))[0].view
        assert torch.equal(got, want), (shape, k, s, relu)
        assert torch.equal(ops.im2col3d(x, (k,) * 3, (s,) * 3, front, out_size, ldk, relu), want)


@pytest.mark.parametrize("shape", [(3, 7, 6, 16), (4, 8, 9, 8)])
def test_maxpool3d_relu_is_exact(shape):
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    T, H, W, C = shape
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(T + C)).half().to(DEV)
    for kernel, stride in POOLS:
        out_size, front, back = _geometry(shape, kernel, stride)
        want = F.max_pool3d(_pad_cthw(x.clamp_min(0), front, back)[None], kernel, stride)[0].permute(1, 2, 3, 0).half().contiguous()
        assert list(want.shape) == out_size + [C]
        rows = out_size[0] * out_size[1] * out_size[2]

        def run(view, prefill):
            _lib.check(lib.ew_maxpool3d_relu_f16(P(x), P(view), T, H, W, C, *kernel, *stride, *front, *out_size, None), "ew_maxpool3d_relu_f16")
        got = KC.two_prefills(run, (rows, C, torch.float16, {"ld": C}))[0].view
        assert torch.equal(got.view(*out_size, C), want), (shape, kernel, stride)
        assert torch.equal(ops.maxpool3d_relu(x, kernel, stride, front, out_size), want)
    assert not ops.maxpool3d_relu(-x.abs(), (3, 3, 3), (1, 1, 1), (1, 1, 1), shape[:3]).any()      # all negative: the ReLU gives zeros


def _ordinal(h):
    """fp16 -> an integer that counts representable values in order (adjacent values differ by one, -0 and +0 coincide)"""
    b = h.view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


@pytest.mark.parametrize("H,W", [(45, 80), (60, 52), (224, 224), (576, 1024)])
def test_preprocess_within_one_fp16_ulp(H, W, models):
    """against the restatement's fp32 result rounded to fp16: every element within one fp16 step, the padding channels exactly zero"""
    _, model = models(0)
    g = torch.Generator().manual_seed(H)
    T = 3
    u8 = _scene_u8(g, T, H, W)
    f32 = torch.rand(T, 3, H, W, generator=g)
    for clip in (u8, f32):
        for order in ("rgb", "bgr"):
            got = model.preprocess(clip.to(DEV), order)
            assert got.dtype == torch.float16 and tuple(got.shape) == (T, 224, 224, 8) and not got[..., 3:].any()
            want = i3d_ref.clip_input(clip, order)[0].permute(1, 2, 3, 0).half().to(DEV)                       # [T,224,224,3]
            steps = (_ordinal(got[..., :3].contiguous()) - _ordinal(want.contiguous())).abs()
            print(f"preprocess {H}x{W} {str(clip.dtype)[6:]} {order}: {int((steps > 0).sum())} of {steps.numel()} elements differ, worst {int(steps.max())} fp16 steps")
            assert int(steps.max()) <= 1, (H, W, clip.dtype, order)
    with pytest.raises(ValueError, match="channel_order"):
        model.preprocess(u8.to(DEV), "gbr")


@pytest.mark.parametrize("Tp", [2, 4])
def test_head_against_fp64(Tp):
    """fp32 sums of non-negative terms against fp64: (n + 16) * 2^-24 covers any order of n terms; here n = 98 per window for the mean
    plus 1024 for the dot product, relative to the sum of the absolute values of the terms"""
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(Tp)
    x = torch.randn(Tp, 7, 7, 1024, generator=g).half().to(DEV)
    x[:, :, :, 5] = -1.0                                                                      # a channel the ReLU removes everywhere
    w, b = (0.05 * torch.randn(400, 1024, generator=g)).to(DEV), torch.randn(400, generator=g).to(DEV)
    cnt = torch.tensor([1.0 if j in (0, Tp - 1) else 2.0 for j in range(Tp)], dtype=torch.float64, device=DEV)
    v = (x.double().clamp_min(0) * cnt.view(-1, 1, 1, 1)).sum((0, 1, 2)) / (98 * (Tp - 1))
    pooled = F.avg_pool3d(x.double().clamp_min(0).permute(3, 0, 1, 2)[None], (2, 7, 7), 1)[0, :, :, 0, 0]     # [1024, Tp - 1]: the definition
    assert float((pooled.mean(1) - v).abs().max()) <= 1e-12
    want = w.double() @ v + b.double()
    scale = w.double().abs() @ v + b.double().abs()
    bound = ((Tp - 1) * 98 + 1024 + 16) * 2.0 ** -24

    def run(out, ws, prefill):
        _lib.check(lib.ew_i3d_head(P(x), Tp, 7, 7, 1024, P(w), P(b), P(out), P(ws), None), "ew_i3d_head")
    got = KC.two_prefills(run, (1, 400, torch.float32, {"ld": 400}), (1, 1024, torch.float32, {"ld": 1024}))[0].view.reshape(400)
    err = float(((got.double() - want).abs() / scale).max())
    print(f"I3D head T' = {Tp}: worst error {err:.3e} of the terms' absolute sum (bound {bound:.2e})")
    assert err <= bound
    assert torch.equal(ops.i3d_head(x, w, b), got)


def test_kernel_entries_refuse_bad_arguments():
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(4, 8, 8, 8, dtype=torch.float16, device=DEV)
    out = torch.zeros(1 << 18, dtype=torch.float16, device=DEV)
    f = torch.zeros(400 * 1024, dtype=torch.float32, device=DEV)
    u8 = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device=DEV)
    cases = [(lambda: lib.ew_im2col3d_f16(P(x), P(out), 4, 8, 8, 8, 3, 3, 3, 1, 1, 1, 1, 1, 1, 4, 8, 8, 128, 0, None), "ldk = 128"),
             (lambda: lib.ew_im2col3d_f16(P(x), P(out), 4, 8, 8, 12, 3, 3, 3, 1, 1, 1, 1, 1, 1, 4, 8, 8, 384, 0, None), "C % 8"),
             (lambda: lib.ew_im2col3d_f16(P(x), P(out), 4, 8, 8, 8, 3, 3, 3, 1, 1, 1, 3, 1, 1, 4, 8, 8, 256, 0, None), "front pads"),
             (lambda: lib.ew_im2col3d_f16(P(x), P(out), 4, 8, 8, 8, 3, 3, 3, 1, 1, 1, 1, 1, 1, 6, 8, 8, 256, 0, None), "miss the"),
             (lambda: lib.ew_im2col3d_f16(None, P(out), 4, 8, 8, 8, 3, 3, 3, 1, 1, 1, 1, 1, 1, 4, 8, 8, 256, 0, None), "NULL"),
             (lambda: lib.ew_maxpool3d_relu_f16(P(x), P(out), 4, 8, 8, 8, 3, 3, 3, 2, 2, 2, 0, 0, 0, 2, 5, 4, None), "miss the"),
             (lambda: lib.ew_maxpool3d_relu_f16(P(x), P(out), 4, 8, 8, 8, 3, 3, 3, 0, 2, 2, 0, 0, 0, 2, 4, 4, None), "must be positive"),
             (lambda: lib.ew_video_preprocess_f16(P(u8), 0, P(out), 2, 8, 8, 224, 224, 0, 0, 0, None), "src_kind 0"),
             (lambda: lib.ew_video_preprocess_f16(P(u8), 1, P(out), 2, 8, 8, 224, 223, 0, 0, 0, None), "at least 224"),
             (lambda: lib.ew_video_preprocess_f16(P(u8), 1, P(out), 2, 8, 8, 224, 300, 0, 77, 0, None), "leaves the resized frame"),
             (lambda: lib.ew_i3d_head(P(x), 1, 7, 7, 1024, P(f), P(f), P(f), P(f), None), "Mixed_5c"),
             (lambda: lib.ew_i3d_head(P(x), 2, 7, 8, 1024, P(f), P(f), P(f), P(f), None), "Mixed_5c"),
             (lambda: lib.ew_i3d_head(P(x), 2, 7, 7, 832, P(f), P(f), P(f), P(f), None), "Mixed_5c")]
    for call, msg in cases:
        assert call() != 0 and msg in lib.ew_last_error().decode(), (msg, lib.ew_last_error())
    with pytest.raises(TypeError):
        ops.maxpool3d_relu(x.float(), (3, 3, 3), (1, 1, 1), (1, 1, 1), (4, 8, 8))
    with pytest.raises(ValueError):
        ops.i3d_head(torch.zeros(2, 7, 7, 1024, dtype=torch.float16, device=DEV), f[:400 * 512].view(400, 512), f[:400])


# ------------------------------------------------------------------ the network
def _endpoint_errors(eps, ref):
    """rel-L2 of every endpoint, device [T,H,W,C] against the restatement's [1,C,T,H,W]"""
    errs = {}
    for name in i3d_ref.ORDER:
        want = ref[name][0].permute(1, 2, 3, 0)
        assert tuple(eps[name].shape) == tuple(want.shape), (name, eps[name].shape, want.shape)
        errs[name] = KC.rel_l2(eps[name].cpu(), want)
    errs["Logits"] = KC.rel_l2(eps["Logits"].cpu(), ref["Logits"][0])
    return errs


@pytest.mark.parametrize("seed,T,H,W", [(s, T, 224, 224) for s in (0, 1, 2) for T in (10, 13)] + [(0, 25, 96, 160)])
def test_logits_and_endpoints_match_the_restatement(seed, T, H, W, models):
    sd, model = models(seed)
    clip = _scene_u8(torch.Generator().manual_seed(1000 * seed + T), T, H, W)
    eps = model.endpoints(clip.to(DEV))
    assert eps["Logits"].dtype == torch.float32 and tuple(eps["Logits"].shape) == (400,) and eps["Logits"].is_cuda
    errs = _endpoint_errors(eps, i3d_ref.endpoints(i3d_ref.clip_input(clip), sd))
    print(f"I3D seed {seed} T {T} {H}x{W}: logits rel-L2 {errs['Logits']:.3e} (bound {REL_BOUND:.2e}); endpoints " +
          " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    first_bad = next((k for k, v in errs.items() if not v <= REL_BOUND), None)
    assert first_bad is None, f"{first_bad} is the first endpoint beyond the bound: {errs[first_bad]:.3e}"
    assert torch.equal(model.logits(clip.to(DEV)), eps["Logits"])


def test_logits_do_not_depend_on_history_or_on_the_rest_of_the_clip(models):
    _, model = models(0)
    g = torch.Generator().manual_seed(77)
    a, b = _scene_u8(g, 12, 64, 96).to(DEV), _scene_u8(g, 10, 80, 72).to(DEV)
    alone = model.logits(a)
    assert torch.equal(model.logits(a), alone)                                                # two runs agree bit for bit
    model.logits(b)
    model.logits(b, channel_order="bgr")
    assert torch.equal(model.logits(a), alone)                                                # and after other clips
    for L in (10, 11):
        assert torch.equal(model.logits(a, n_frames=L), model.logits(a[:L].contiguous())), L
        assert torch.equal(model.forward(model.preprocess(a), L), model.logits(a[:L].contiguous())), L
    assert not torch.equal(model.logits(a, n_frames=10), alone) and not torch.equal(model.logits(a, channel_order="bgr"), alone)
    f32 = (a.cpu().permute(0, 3, 1, 2).float() / 255.0).contiguous().to(DEV)                 # IEEE division, on the host
    assert torch.equal(model.logits(f32), alone)                                              # uint8 frames are float32(k) / 255
    small = type(model)(model.p, DEV, workspace_bytes=8 << 20)                                # many slabs of output frames: other GEMM shapes,
    slabbed = small.logits(a)                                                                 # so the same values up to summation order
    print(f"I3D with an 8 MiB patch-row cap: rel-L2 {KC.rel_l2(slabbed, alone):.3e} from the default cap, bit-identical: {torch.equal(slabbed, alone)}")
    assert KC.rel_l2(slabbed, alone) <= REL_BOUND and torch.equal(small.logits(a), slabbed)
    with pytest.raises(ValueError, match="n_frames"):
        model.logits(a[:8].contiguous())


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
    from evoworld_amd import fvd as V
    from evoworld_amd import metrics as M
    E, T, H, W = 3, 12, 64, 96
    g = torch.Generator().manual_seed(31)
    gt = torch.stack([_scene_u8(g, T, H, W) for _ in range(E)])
    gen = (gt.to(torch.int16) + torch.randint(-24, 25, gt.shape, generator=g, dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
    _write_tree(str(tmp_path), gt.numpy(), gen.numpy())
    sd = V.random_state_dict(0)
    weights = str(tmp_path / "i3d.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, weights)
    argv = ["--data_path", str(tmp_path), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0"]
    M.main(argv + ["--metrics", "psnr,ssim,fvd", "--fvd_weights", weights, "--result_file", "scores.json"])
    got = json.load(open(tmp_path / "scores.json"))
    assert list(got) == ["fvd", "ssim", "psnr", "not_computed"]
    assert set(got["not_computed"]) == {"lpips", "latent_mse", "loop_closure_latent_mse"}
    fvd = got["fvd"]
    assert set(fvd) == {"value", "value_mean", "fvd_setting", "video_setting", "video_setting_name"}
    assert list(fvd["value"]) == ["10", "11", "12"] and fvd["fvd_setting"] == "styleganv"
    assert fvd["video_setting"] == [E, 3, T, H, W] and fvd["video_setting_name"] == "batch_size, channel, time, height, width"
    assert fvd["value_mean"] == float(np.mean(list(fvd["value"].values())))
    # the B, G, R default against the restatement fed B, G, R, through the same frechet_distance (ground truth first)
    worst = 0.0
    for L in (10, 11, 12):
        batch = torch.cat([i3d_ref.clip_input(v[e, :L], "bgr") for v in (gt, gen) for e in range(E)])
        feats = i3d_ref.endpoints(batch, sd)["Logits"].double().numpy()
        want = V.frechet_distance(feats[:E], feats[E:])
        rel = abs(fvd["value"][str(L)] - want) / abs(want)
        worst = max(worst, rel)
        print(f"FVD CLI {H}x{W} clip length {L}: {fvd['value'][str(L)]:.6f} against {want:.6f}, off by {rel:.3e} (bound {FVD_REL_BOUND:.2e})")
    assert worst <= FVD_REL_BOUND
    # rgb is another number, and calculate_fvd gives the same dict from [B,T,C,H,W] videos
    rgb, _ = M.main(argv + ["--metrics", "fvd", "--fvd_weights", weights, "--fvd_channel_order", "rgb"])
    assert list(rgb) == ["fvd", "not_computed"] and rgb["fvd"]["value"][10] != fvd["value"]["10"]
    v1, v2 = (v.permute(0, 1, 4, 2, 3).float() / 255.0 for v in (gt, gen))
    d = V.calculate_fvd(v1, v2, V.I3D.from_files(weights, DEV), "rgb")
    assert d["value"] == rgb["fvd"]["value"] and d["video_setting"] == torch.Size([E, 3, T, H, W])
    # without weights nothing changes: the three keys, all four names not computed, fvd refused
    plain, _ = M.main(argv + ["--result_file", "plain.json"])
    assert list(plain) == ["ssim", "psnr", "not_computed"] and plain["not_computed"] == M.NOT_COMPUTED
    plain = json.load(open(tmp_path / "plain.json"))
    assert plain["psnr"] == got["psnr"] and plain["ssim"] == got["ssim"] and set(plain["not_computed"]) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"}
    with pytest.raises(ValueError, match="I3D"):
        M.main(argv + ["--metrics", "psnr,fvd"])
