"""-m gpu: LPIPS (AlexNet backbone, user-supplied weights) on the device -- evoworld_amd.lpips over ew_im2col_frames_f16 and ew_lpips_head
(csrc/lpips.hip), ew_im2col3d_f16 and ew_maxpool3d_relu_f16 with kt = 1 (csrc/convnet.hip) and ew_gemm_f16 -- against the fp32 PyTorch restatement tests/lpips_ref.py run on the host
with seeded random weights (no LPIPS weights or package exist here: this row is not pinned by the reference's own run).

Parity bound.  REL_BOUND is a relative error per frame pair: twice the worst value measured on the MI355X over every case of
test_parity_* below (the factor covers the seed-to-seed spread of the fp16 operand rounding).  Measured worst values:
  64 x 64    (3 seeds x uint8 / fp32 x rgb / bgr, 2 noise + 2 perturbed pairs each):   2.733e-4 (a perturbed pair, LPIPS 0.057)
  70 x 93    (the same):                                                                2.759e-4 (a perturbed pair, LPIPS 0.069)
  576 x 1024 (1 seed x uint8 / fp32 x rgb / bgr, 1 noise + 1 perturbed pair each):      7.141e-5 (a perturbed pair, LPIPS 0.066)
Noise pairs (LPIPS 0.84 ... 0.96) stay below 8.2e-5 at every size.  All of it is inside the project's 1e-3 class.  Per-tap errors of the
worst pairs (each tap's own contribution against the restatement's): tap 1 1e-6, tap 2 4e-5 ... 9e-5, taps 3-5 7e-5 ... 2.3e-4 -- the error
is the fp16 operand and storage rounding accumulated over conv2 ... conv5; conv1's operand rounding contributes nothing visible, so a
hi / lo split of its operand would change nothing.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import kernel_checks as KC
import lpips_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEASURED = {"64x64": 2.733e-4, "70x93": 2.759e-4, "576x1024": 7.141e-5}      # worst relative error per frame pair on the MI355X
REL_BOUND = 2 * max(MEASURED.values())                                       # 5.518e-4
# the head alone, fp32 sums of C <= 384 non-negative terms against fp64: (C + 16) * 2^-24 covers any summation order
HEAD_BOUND = 400 * 2.0 ** -24


def _noise_u8(g, n, H, W):
    return torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)


def _scene_u8(g, n, H, W):
    """a smooth pattern under a random texture: what a frame pair with a small perturbation starts from"""
    y = torch.arange(H, dtype=torch.float32)[:, None, None]
    x = torch.arange(W, dtype=torch.float32)[None, :, None]
    c = torch.arange(3, dtype=torch.float32)[None, None, :]
    out = []
    for _ in range(n):
        ph = float(torch.rand((), generator=g)) * 6.28
        base = 128 + 70 * torch.sin(0.05 * x * (c + 1) + 0.08 * y + ph) + 25 * torch.randn(H, W, 3, generator=g)
        out.append(base.round().clamp(0, 255).to(torch.uint8))
    return torch.stack(out)


def _pairs(seed, H, W, n_noise, n_pert, dtype):
    """(a, b): n_noise pairs of independent noise frames, then n_pert frames against perturbed copies (+-24 levels / sigma 0.06, which
    puts LPIPS with these weights at 0.05 ... 0.2, where real evaluations are).
    uint8 [F,H,W,3], or fp32 [F,3,H,W] in [0,1] with values off the 8-bit grid."""
    g = torch.Generator().manual_seed(seed)
    scene = _scene_u8(g, n_pert, H, W)
    if dtype == torch.uint8:
        pert = (scene.to(torch.int16) + torch.randint(-24, 25, scene.shape, generator=g, dtype=torch.int16)).clamp(0, 255).to(torch.uint8)
        return torch.cat([_noise_u8(g, n_noise, H, W), scene]), torch.cat([_noise_u8(g, n_noise, H, W), pert])
    s = scene.permute(0, 3, 1, 2).float() / 255.0
    a = torch.cat([torch.rand(n_noise, 3, H, W, generator=g), (s + 0.002 * torch.randn(s.shape, generator=g)).clamp(0, 1)])
    b = torch.cat([torch.rand(n_noise, 3, H, W, generator=g), (s + 0.06 * torch.randn(s.shape, generator=g)).clamp(0, 1)])
    return a.contiguous(), b.contiguous()


def _as_ref_input(t):
    return t.permute(0, 3, 1, 2).float() / 255.0 if t.dtype == torch.uint8 else t


def _model(sd, **kw):
    from evoworld_amd.lpips import LPIPSAlex
    return LPIPSAlex.from_state_dict(sd, DEV, **kw)


def _per_tap(model, sd, a, b, order):
    """relative error of each tap's own contribution (device against the restatement), for the first frame pair"""
    from evoworld_amd import ops
    from evoworld_amd.lpips import tap_sizes
    H, W = (a.shape[1], a.shape[2]) if a.dtype == torch.uint8 else (a.shape[2], a.shape[3])
    taps = model.features(torch.cat([a[:1], b[:1]]).to(DEV).contiguous(), order)
    maps = lpips_ref.tap_maps(_as_ref_input(a[:1]), _as_ref_input(b[:1]), sd, order)
    errs = []
    for i, t in enumerate(taps):
        acc = torch.zeros(1, dtype=torch.float64, device=DEV)
        wy, wx = model._weights_for(*tap_sizes(H, W)[i], H, W)
        ops.lpips_head(t[:1], t[1:], model.lin[i], wy, wx, H * W, acc)
        want = float(maps[i].double().mean())
        errs.append(abs(float(acc[0]) - want) / want)
    return errs


def _parity(H, W, seeds, n_noise, n_pert):
    worst, worst_case = 0.0, None
    for seed in seeds:
        sd = lpips_ref.random_weights(seed)
        model = _model(sd)
        for dtype in (torch.uint8, torch.float32):
            a, b = _pairs(100 * seed + H, H, W, n_noise, n_pert, dtype)
            for order in ("rgb", "bgr"):
                got = model(a.to(DEV), b.to(DEV), order)
                assert got.dtype == torch.float64 and got.shape == (n_noise + n_pert,) and got.is_cuda
                want = lpips_ref.lpips_alex(_as_ref_input(a), _as_ref_input(b), sd, order).double()
                rel = ((got.cpu() - want).abs() / want).tolist()
                print(f"LPIPS {H}x{W} seed {seed} {str(dtype)[6:]} {order}: ref {[f'{v:.4f}' for v in want.tolist()]} "
                      f"rel err {[f'{v:.2e}' for v in rel]}")
                if max(rel) > worst:
                    worst, worst_case = max(rel), (seed, dtype, order, a, b, sd, model)
    seed, dtype, order, a, b, sd, model = worst_case
    print(f"LPIPS {H}x{W}: worst relative error per frame pair {worst:.3e} (seed {seed}, {dtype}, {order}); per-tap errors of its first "
          f"pair {[f'{v:.2e}' for v in _per_tap(model, sd, a, b, order)]}; bound {REL_BOUND:.1e}")
    return worst


def test_parity_64x64():
    """the lpips package's own demo size"""
    assert _parity(64, 64, (0, 1, 2), 2, 2) <= REL_BOUND


def test_parity_70x93():
    """odd sizes: floor in the conv / pool shapes, asymmetric border weights of the upsampling"""
    assert _parity(70, 93, (0, 1, 2), 2, 2) <= REL_BOUND


def test_parity_576x1024():
    """the product's frame size"""
    assert _parity(576, 1024, (0,), 1, 1) <= REL_BOUND


def test_exact_properties():
    """nothing here has a tolerance: zero on identical frames, symmetry, run-to-run and chunking invariance hold bit for bit"""
    sd = lpips_ref.random_weights(7)
    model = _model(sd, chunk=4)
    for dtype in (torch.uint8, torch.float32):
        a, b = (t.to(DEV) for t in _pairs(11, 70, 93, 3, 4, dtype))
        ab = model(a, b)
        assert ab.dtype == torch.float64 and ab.shape == (7,) and ab.device.type == "cuda"
        assert bool(torch.isfinite(ab).all()) and bool((ab >= 0).all()) and float(ab.min()) > 0
        assert torch.equal(model(a, a), torch.zeros(7, dtype=torch.float64, device=DEV))
        assert torch.equal(model(b, a), ab)                                  # symmetric
        assert torch.equal(model(a, b), ab)                                  # deterministic
        for chunk in (1, 2, 3, 7, 100):
            assert torch.equal(model(a, b, chunk=chunk), ab), chunk
        assert torch.equal(_model(sd, chunk=1)(a, b), ab)
        assert torch.equal(model(a[2:5], b[2:5]), ab[2:5])                   # a pair's value does not depend on its neighbours
        assert not torch.equal(model(a, b, "bgr"), ab)
    with pytest.raises(ValueError, match="at least 31"):
        model(torch.zeros(1, 30, 64, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 30, 64, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        model(a, b[:2])
    with pytest.raises(ValueError, match="channel_order"):
        model(a, b, "gbr")


# ------------------------------------------------------------------ each kernel alone, at the five tap shapes of a 576 x 1024 frame
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
TAPS = ((143, 255, 64), (71, 127, 192), (35, 63, 384), (35, 63, 256), (35, 63, 256))
FRAME = (576, 1024)


def _unfold_rows(x_nhwc, k, stride, pad, ldk):
    """fp16 NHWC -> the expected patch rows [n*ho*wo, ldk], column (ky*k + kx)*C + c (values pass through fp32 unchanged)"""
    n, h, w, C = x_nhwc.shape
    cols = F.unfold(x_nhwc.permute(0, 3, 1, 2).float(), k, padding=pad, stride=stride)               # [n, C*k*k, L], rows (c, ky, kx)
    L_ = cols.shape[-1]
    rows = cols.view(n, C, k * k, L_).permute(0, 3, 2, 1).reshape(n * L_, k * k * C).half()
    out = torch.zeros(n * L_, ldk, dtype=torch.float16, device=x_nhwc.device)
    out[:, :k * k * C] = rows
    return out


def _run_im2col(src, kind, n, h, w, C, k, stride, pad, ldk, relu, swap, affine):
    """kind 1 / 2: the frames' entry; kind 0: the fp16 gather, the 3-D entry with kt = 1 and the image batch on T"""
    from evoworld_amd import _lib
    lib = _lib.load()
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

    def run(view, prefill):
        if kind:
            _lib.check(lib.ew_im2col_frames_f16(P(src), kind, P(view), n, h, w, k, stride, pad, ho, wo, ldk, swap, affine, None), "ew_im2col_frames_f16")
        else:
            _lib.check(lib.ew_im2col3d_f16(P(src), P(view), n, h, w, C, 1, k, k, 1, stride, stride, 0, pad, pad, n, ho, wo, ldk, relu, None),
                       "ew_im2col3d_f16")
    return KC.two_prefills(run, (n * ho * wo, ldk, torch.float16, {"ld": ldk}))[0].view


def test_im2col_first_layer_is_exact():
    from evoworld_amd.lpips import SCALE, SHIFT
    H, W = FRAME
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    f32 = torch.rand(2, 3, H, W, generator=g)
    affine = (ctypes.c_float * 6)(*SHIFT, *SCALE)
    shift, scale = np.array(SHIFT, np.float32), np.array(SCALE, np.float32)
    for swap in (0, 1):
        # the reference's float32 steps in numpy (IEEE division): k / 255 -> 2x - 1 -> (x - shift) / scale, per network channel
        x01 = {1: u8.numpy().astype(np.float32) / np.float32(255.0), 2: f32.permute(0, 2, 3, 1).numpy()}
        for kind, src in ((1, u8), (2, f32)):
            x = x01[kind][..., ::-1] if swap else x01[kind]
            want_in = torch.from_numpy(np.ascontiguousarray(((x * np.float32(2) - np.float32(1)) - shift) / scale)).half().to(DEV)
            want = _unfold_rows(want_in, 11, 4, 2, 384)
            got = _run_im2col(src.to(DEV), kind, 2, H, W, 3, 11, 4, 2, 384, 0, swap, affine)
            assert got.shape == (2 * 143 * 255, 384) and torch.equal(got, want), (kind, swap)


def test_im2col_f16_is_exact():
    from evoworld_amd import ops
    g = torch.Generator().manual_seed(4)
    for (h, w, C), k, pad, relu in (((71, 127, 64), 5, 2, 0), ((35, 63, 192), 3, 1, 0), ((35, 63, 384), 3, 1, 1), ((35, 63, 256), 3, 1, 1),
                                    ((143, 255, 64), 3, 1, 1)):
        x = torch.randn(2, h, w, C, generator=g).half().to(DEV)
        ldk = -(-k * k * C // 64) * 64 + (64 if C == 64 and k == 3 else 0)               # the last case also pads K
        want = _unfold_rows(x.clamp_min(0) if relu else x, k, 1, pad, ldk)
        got = _run_im2col(x, 0, 2, h, w, C, k, 1, pad, ldk, relu, 0, None)
        assert torch.equal(got, want), (h, w, C, k)
        assert torch.equal(ops.im2col3d(x, (1, k, k), (1, 1, 1), (0, pad, pad), (2, h, w), ldk, relu), want)


def test_maxpool3s2_relu_is_exact():
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    for h, w, C in TAPS:
        x = torch.randn(2, h, w, C, generator=g).half().to(DEV)
        ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        want = F.max_pool2d(x.permute(0, 3, 1, 2).float().clamp_min(0), 3, 2).permute(0, 2, 3, 1).half().contiguous()
        assert want.shape == (2, ho, wo, C)

        def run(view, prefill):
            _lib.check(lib.ew_maxpool3d_relu_f16(P(x), P(view), 2, h, w, C, 1, 3, 3, 1, 2, 2, 0, 0, 0, 2, ho, wo, None), "ew_maxpool3d_relu_f16")
        got = KC.two_prefills(run, (2 * ho * wo, C, torch.float16, {"ld": C}))[0].view
        assert torch.equal(got.view(2, ho, wo, C), want), (h, w, C)
        assert torch.equal(ops.maxpool3d_relu(x, (1, 3, 3), (1, 2, 2), (0, 0, 0), (2, ho, wo)), want)
    neg = -torch.rand(1, 7, 7, 8, generator=g).half().to(DEV)                            # all negative: the ReLU gives zeros
    assert not ops.maxpool3d_relu(neg, (1, 3, 3), (1, 2, 2), (0, 0, 0), (1, 3, 3)).any()


def test_lpips_head_against_fp64():
    from evoworld_amd import _lib
    from evoworld_amd.lpips import upsample_mean_weights
    lib = _lib.load()
    H, W = FRAME
    g = torch.Generator().manual_seed(6)
    F_ = 3
    for h, w, C in TAPS:
        fa = torch.randn(F_, h, w, C, generator=g).half().to(DEV)
        fb = (fa.cpu().float() + 0.3 * torch.randn(F_, h, w, C, generator=g)).half().to(DEV)
        fb[2] = fa[2]                                                                    # an identical pair: exactly zero
        fa[0, 0, 0] = -1.0                                                               # a pixel whose features are all zero after the ReLU
        lin = torch.rand(C, generator=g).to(DEV)
        wy, wx = (torch.from_numpy(upsample_mean_weights(n_in, n_out)).to(DEV) for n_in, n_out in ((h, H), (w, W)))
        start = torch.tensor([0.0, 0.25, 0.5], dtype=torch.float64, device=DEV)          # the entry accumulates
        na, nb = (t.double().clamp_min(0) for t in (fa, fb))
        na, nb = (t / (t.square().sum(-1, keepdim=True).sqrt() + 1e-10) for t in (na, nb))
        d = ((na - nb).square() * lin.double()).sum(-1)
        want = start + (d * wy[None, :, None] * wx[None, None, :]).sum((1, 2)) / (H * W)
        ws_bytes = lib.ew_lpips_head_workspace_bytes(F_, h, w, C)

        def run(acc_bytes, ws, prefill):
            acc_bytes.view(torch.float64).copy_(start.view(1, F_))
            _lib.check(lib.ew_lpips_head(P(fa), P(fb), P(lin), P(wy), P(wx), F_, h, w, C, float(H * W), P(acc_bytes), P(ws), None), "ew_lpips_head")
        accs = KC.two_prefills(run, (1, F_ * 8, torch.uint8, {"ld": F_ * 8}), (1, ws_bytes, torch.uint8, {"ld": ws_bytes}))
        got = accs[0].view.view(torch.float64).reshape(F_)
        rel = ((got - want).abs() / (want - start).clamp_min(1e-300))[:2]
        print(f"LPIPS head {h}x{w}x{C}: values {(got - start).tolist()} rel err {rel.tolist()} (bound {HEAD_BOUND:.1e})")
        assert float(rel.max()) <= HEAD_BOUND, (h, w, C, rel)
        assert float(got[2]) == 0.5                                                      # identical features add exactly nothing


def test_kernel_entries_refuse_bad_arguments():
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    x = torch.zeros(1, 8, 8, 8, dtype=torch.float16, device=DEV)
    out = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    d = torch.zeros(64, dtype=torch.float64, device=DEV)
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    affine = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    # the fp16 gather and the pool are the 3-D entries with kt = 1: they take the caller's output size and refuse one whose windows leave the
    # input (an 11th output row of an 8-row image; a 5th pooled row; no pooled row at all), not one that merely differs from floor(...)
    cases = [(lambda: lib.ew_im2col3d_f16(P(x), P(out), 1, 8, 8, 8, 1, 3, 3, 1, 1, 1, 0, 1, 1, 1, 11, 8, 128, 0, None), "has windows that miss"),
             (lambda: lib.ew_im2col3d_f16(P(x), P(out), 1, 8, 8, 8, 1, 3, 3, 1, 1, 1, 0, 1, 1, 1, 8, 8, 64, 0, None), "ldk = 64"),
             (lambda: lib.ew_im2col3d_f16(P(x), P(out), 1, 8, 8, 4, 1, 3, 3, 1, 1, 1, 0, 1, 1, 1, 8, 8, 64, 0, None), "C % 8"),
             (lambda: lib.ew_im2col_frames_f16(P(x), 1, P(out), 1, 8, 8, 3, 1, 1, 7, 8, 64, 0, affine, None), "is not floor"),
             (lambda: lib.ew_im2col_frames_f16(P(x), 1, P(out), 1, 8, 8, 3, 1, 1, 8, 8, 64, 0, None, None), "six scaling constants"),
             (lambda: lib.ew_im2col_frames_f16(P(x), 3, P(out), 1, 8, 8, 3, 1, 1, 8, 8, 128, 0, affine, None), "src_kind 3"),
             (lambda: lib.ew_im2col_frames_f16(P(x), 0, P(out), 1, 8, 8, 3, 1, 1, 8, 8, 128, 0, affine, None), "src_kind 0"),
             (lambda: lib.ew_maxpool3d_relu_f16(P(x), P(out), 1, 8, 8, 8, 1, 3, 3, 1, 2, 2, 0, 0, 0, 1, 5, 3, None), "has windows that miss"),
             (lambda: lib.ew_maxpool3d_relu_f16(P(x), P(out), 1, 2, 8, 8, 1, 3, 3, 1, 2, 2, 0, 0, 0, 1, 0, 3, None), "has windows that miss"),
             (lambda: lib.ew_lpips_head(P(x), P(x), P(f), P(d), P(d), 1, 8, 8, 12, 64.0, P(d), P(d), None), "C = 12"),
             (lambda: lib.ew_lpips_head(P(x), P(x), P(f), P(d), P(d), 1, 8, 8, 8, 0.0, P(d), P(d), None), "n_out"),
             (lambda: lib.ew_lpips_head(P(x), P(x), None, P(d), P(d), 1, 8, 8, 8, 64.0, P(d), P(d), None), "NULL")]
    for call, msg in cases:
        assert call() != 0 and msg in lib.ew_last_error().decode(), (msg, lib.ew_last_error())
    with pytest.raises(TypeError):
        ops.maxpool3d_relu(x.float(), (1, 3, 3), (1, 2, 2), (0, 0, 0), (1, 3, 3))
    with pytest.raises(ValueError):
        ops.lpips_head(x, x, f[:8], d[:8], d[:7], 64, d[:1])


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
    from evoworld_amd import metrics as M
    H, W = 48, 80
    a, b = _pairs(21, H, W, 10, 40, torch.uint8)
    gt, gen = a.reshape(2, 25, H, W, 3).numpy(), b.reshape(2, 25, H, W, 3).numpy()
    _write_tree(str(tmp_path), gt, gen)
    sd = lpips_ref.random_weights(5)
    weights = str(tmp_path / "lpips_alex.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, weights)
    argv = ["--data_path", str(tmp_path), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0"]
    M.main(argv + ["--metrics", "psnr,ssim,lpips", "--lpips_weights", weights, "--result_file", "scores.json"])
    got = json.load(open(tmp_path / "scores.json"))
    assert list(got) == ["ssim", "psnr", "lpips", "not_computed"]
    assert set(got["not_computed"]) == {"fvd", "latent_mse", "loop_closure_latent_mse"}
    lp = got["lpips"]
    assert set(lp) == {"value", "value_mean", "value_std", "video_setting", "video_setting_name"}
    assert lp["video_setting"] == [25, 3, H, W] and lp["video_setting_name"] == "time, channel, heigth, width"
    assert list(lp["value"]) == [str(t) for t in range(25)] and list(lp["value_std"]) == list(lp["value"])
    # the per-frame values are LPIPSAlex.__call__'s, fed B, G, R planes by default, aggregated as PSNR and SSIM are
    model = _model(sd)
    frames = model(a.to(DEV), b.to(DEV), "bgr").cpu().numpy().reshape(2, 25)
    assert lp["value_mean"] == float(np.mean(frames))
    assert [lp["value"][str(t)] for t in range(25)] == [float(np.mean(frames[:, t])) for t in range(25)]
    assert [lp["value_std"][str(t)] for t in range(25)] == [float(np.std(frames[:, t])) for t in range(25)]
    # the BGR default against the restatement fed BGR, on what the CLI reports: the mean over the 50 pairs.  (The relative error of a
    # mean of positive values cannot exceed the worst per-pair one, so REL_BOUND applies; the worst single pair of these 50 at 48 x 80
    # measured 5.77e-4 on the MI355X, printed here as a figure.)
    want = lpips_ref.lpips_alex(_as_ref_input(a), _as_ref_input(b), sd, "bgr").double().numpy()
    rel = np.abs(frames.ravel() - want) / want
    rel_mean = abs(lp["value_mean"] - want.mean()) / want.mean()
    print(f"LPIPS CLI {H}x{W}: value_mean off by {rel_mean:.3e} (bound {REL_BOUND:.2e}); worst single pair {rel.max():.3e}")
    assert rel_mean <= REL_BOUND
    rgb_ref = lpips_ref.lpips_alex(_as_ref_input(a), _as_ref_input(b), sd, "rgb").double().numpy()
    assert abs(lp["value_mean"] - rgb_ref.mean()) / rgb_ref.mean() > 10 * REL_BOUND          # and it is not the RGB number
    # rgb is another number, and calculate_lpips gives the same dict from [B,T,C,H,W] videos
    rgb, _ = M.main(argv + ["--metrics", "lpips", "--lpips_weights", weights, "--lpips_channel_order", "rgb"])
    assert list(rgb) == ["lpips", "not_computed"] and rgb["lpips"]["value_mean"] != lp["value_mean"]
    v1, v2 = (torch.from_numpy(v).permute(0, 1, 4, 2, 3) / 255.0 for v in (gt, gen))
    d = M.calculate_lpips(v1, v2, model, "rgb")
    assert d["value_mean"] == pytest.approx(rgb["lpips"]["value_mean"], rel=1e-5) and d["video_setting"] == v1[0].shape
    # without weights nothing changes: the three keys, all four names not computed, lpips refused
    plain, _ = M.main(argv + ["--result_file", "plain.json"])
    assert list(plain) == ["ssim", "psnr", "not_computed"]
    assert set(plain["not_computed"]) == {"fvd", "lpips", "latent_mse", "loop_closure_latent_mse"}
    plain = json.load(open(tmp_path / "plain.json"))
    assert plain["psnr"] == got["psnr"] and plain["ssim"] == got["ssim"]
    with pytest.raises(ValueError, match="LPIPS"):
        M.main(argv + ["--metrics", "psnr,lpips"])
