"""-m gpu: ew_video_metrics_ws (csrc/metrics.hip) through ops.video_metrics_ws and evoworld_amd.metrics -- the row-weighted squared
error and SSIM behind WS-PSNR / WS-SSIM -- against the fp64 restatement tests/ws_metrics_ref.py, against the planar kernel under unit
weights and against a closed form; WS-LPIPS (LPIPSAlex's row_weights) against the weighted restatement built from tests/lpips_ref.py.
Nothing here is in the reference: the header's definitions are the specification, and parity with an external 360-degree tool is not pinned.

Shapes.  The tile of the kernel holds 24 x 32 SSIM outputs: (11, 11) is one window; (12, 45) two tile columns; (34, 42) valid outputs that
fill one tile exactly while the squared error spans 2 x 2 tiles; (35, 43) one row and one column more; (58, 75) 2 x 3 tiles of outputs.

Bounds are the planar kernel's own (tests/test_gpu_metrics.py): wsse 1e-12 * max(1, value), wssim 1e-9, WS-PSNR 1e-5 dB.

WS-LPIPS bound.  WS_LPIPS_BOUND is a relative error per frame pair, twice the worst value measured on the MI355X over the cases of
test_ws_lpips_against_the_weighted_restatement (the convention of tests/test_gpu_lpips.py); MEASURED_WS_LPIPS holds the measured values:
2.066e-4 at 64 x 96 and 9.914e-5 at 70 x 93, so the bound is 4.132e-4.  The error is that of the fp16 convolutions (plain LPIPS measures
2.7e-4 at these sizes); the weighted average itself is host fp64 arithmetic and the head kernel unchanged.
Measured for the kernel (same box): wsse within 3.8e-16 relative, WS-PSNR within 7.2e-15 dB, wssim within 3.4e-16 of the restatement.
"""
import ctypes

import numpy as np
import pytest
import torch

import lpips_ref
import metrics_ref as MR
import ws_metrics_ref as WR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(11, 11), (12, 45), (34, 42), (35, 43), (58, 75)]

# worst relative error per frame pair on the MI355X (latitude and random row weights, rgb and bgr, one noise and one perturbed pair)
MEASURED_WS_LPIPS = {"64x96": 2.066e-4, "70x93": 9.914e-5}      # both on the perturbed pair (WS-LPIPS 0.066, 0.067), B, G, R order, latitude weights
WS_LPIPS_BOUND = 2 * max(MEASURED_WS_LPIPS.values())             # 4.132e-4; noise pairs (WS-LPIPS 0.87 ... 0.92) stay below 4.4e-5


def _pair(F_, H, W, C, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    a = np.stack([np.stack([(128 + 100 * np.sin(0.013 * x * (c + 1) + 0.021 * y + f)) for c in range(C)], -1) for f in range(F_)])
    a = np.clip(a + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
    return a, b


def _inputs(layout, F_, H, W, C, seed):
    """(device a, device b, float32 [F,C,H,W] numpy a, b as the kernel reads them): uint8 [F,H,W,C], or fp32 [F,C,H,W] off the 8-bit grid"""
    a, b = _pair(F_, H, W, C, seed)
    if layout == "u8":
        fa, fb = (MR.u8_values(v).transpose(0, 3, 1, 2) for v in (a, b))
        return torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), fa, fb
    rng = np.random.default_rng(seed + 1)
    fa, fb = (np.ascontiguousarray(np.clip(MR.u8_values(v).transpose(0, 3, 1, 2) + rng.uniform(-0.002, 0.002, (F_, C, H, W)), 0, 1).astype(np.float32))
              for v in (a, b))
    return torch.from_numpy(fa).to(DEV), torch.from_numpy(fb).to(DEV), fa, fb


def _weights(H, seed):
    """latitude weights, and random positive asymmetric ones: the latter tell a window weighted by its top row from one weighted by its
    centre row, and an image row from a tile-local one"""
    return {"latitude": WR.latitude_weights(H), "random": np.random.default_rng(1000 + seed).random(H) + 0.05}


def _check(fa, fb, w, wsse, wssim):
    from evoworld_amd import metrics as M
    F_, C, H, W = fa.shape
    worst = [0.0, 0.0, 0.0]
    for f in range(F_):
        want = WR.wsse_ref(fa[f], fb[f], w)
        worst[0] = max(worst[0], abs(wsse[f] - want) / max(1.0, want))
        assert abs(wsse[f] - want) <= 1e-12 * max(1.0, want), (f, wsse[f], want)
        dp = abs(M.psnr_from_sse(wsse[f], C * W * float(w.sum())) - WR.ws_psnr_ref(fa[f], fb[f], w))
        worst[1] = max(worst[1], dp)
        assert dp <= 1e-5, (f, dp)
        if wssim is not None:
            ds = abs(wssim[f] - WR.wssim_ref(fa[f], fb[f], w))
            worst[2] = max(worst[2], ds)
            assert ds <= 1e-9, (f, wssim[f], ds)
    return worst


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("layout", ["u8", "f32"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_against_the_restatement(H, W, layout, C):
    from evoworld_amd import ops
    ta, tb, fa, fb = _inputs(layout, 2, H, W, C, H * W + C)
    for name, w in _weights(H, H * W).items():
        wsse, wssim = ops.video_metrics_ws(ta, tb, w)
        assert wsse.dtype == wssim.dtype == torch.float64 and wsse.shape == wssim.shape == (2,) and wsse.is_cuda
        worst = _check(fa, fb, w, wsse.cpu().numpy(), wssim.cpu().numpy())
        print(f"WS {H}x{W} {layout} C={C} {name}: wsse rel {worst[0]:.2e}, WS-PSNR {worst[1]:.2e} dB, wssim {worst[2]:.2e}")


def test_full_size_frames_against_the_restatement():
    from evoworld_amd import ops
    ta, tb, fa, fb = _inputs("u8", 2, 576, 1024, 3, 17)
    for name, w in _weights(576, 17).items():
        wsse, wssim = ops.video_metrics_ws(ta, tb, w)
        worst = _check(fa, fb, w, wsse.cpu().numpy(), wssim.cpu().numpy())
        print(f"WS 576x1024 u8 C=3 {name}: wsse rel {worst[0]:.2e}, WS-PSNR {worst[1]:.2e} dB, wssim {worst[2]:.2e}")


@pytest.mark.parametrize("layout", ["u8", "f32"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_unit_weights_give_the_planar_values(H, W, layout):
    from evoworld_amd import ops
    for C in (1, 3):
        ta, tb, _, _ = _inputs(layout, 2, H, W, C, 3 * H + W + C)
        sse, ssim = (t.cpu().numpy() for t in ops.video_metrics(ta, tb))
        wsse, wssim = (t.cpu().numpy() for t in ops.video_metrics_ws(ta, tb, np.ones(H)))
        assert np.abs(wsse - sse).max() <= 1e-12 * np.abs(sse).max() and (sse > 0).all()
        assert np.abs(wssim - ssim).max() <= 1e-12


def test_polar_error_closed_form():
    """H = 40, W = 64, a = 0, b = 1 on the top four and the bottom four rows and 0 elsewhere: the error covers 20 % of the rows and
    sum(cap weights) / sum(weights) = 0.0489434837 of the weighted area (1 - sin 72 deg = 0.0489434837 of the sphere), so
    WS-PSNR - PSNR = 10 log10(0.2 / 0.0489434837) = 6.113 dB"""
    from evoworld_amd import metrics as M
    H, W = 40, 64
    w = WR.latitude_weights(H)
    frac = (w[:4].sum() + w[-4:].sum()) / w.sum()
    assert abs(frac - 0.0489434837) <= 1e-9
    want = 10 * np.log10(0.2 / 0.0489434837)
    assert abs(want - 6.113) <= 1e-3
    for C in (1, 3):
        a = torch.zeros(1, 1, C, H, W)
        b = torch.zeros(1, 1, C, H, W)
        b[..., :4, :] = 1.0
        b[..., -4:, :] = 1.0
        ws, plain = M.calculate_ws_psnr(a, b), M.calculate_psnr(a, b)
        assert abs(plain["value_mean"] - 10 * np.log10(1 / 0.2)) <= 1e-9
        assert abs((ws["value_mean"] - plain["value_mean"]) - want) <= 1e-5, ws["value_mean"] - plain["value_mean"]
        assert ws["video_setting"] == plain["video_setting"] and ws.keys() == plain.keys()
        u8 = lambda t: (t[0] * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(DEV)          # the CLI's fast path: uint8 [F,H,W,C]
        p_ws, _ = M.video_metrics_ws_u8(u8(a), u8(b), 1)
        assert abs(p_ws[0] - ws["value_mean"]) <= 1e-9


def test_calculate_ws_psnr_and_ws_ssim_dicts():
    from evoworld_amd import metrics as M
    a, b = _pair(6, 35, 43, 3, 5)
    v1, v2 = (torch.from_numpy(v).reshape(2, 3, 35, 43, 3).permute(0, 1, 4, 2, 3) / 255.0 for v in (a, b))
    w = WR.latitude_weights(35)
    fa, fb = (MR.u8_values(v).transpose(0, 3, 1, 2) for v in (a, b))
    want_p = M.aggregate(np.array([WR.ws_psnr_ref(fa[f], fb[f], w) for f in range(6)]).reshape(2, 3), v1[0].shape)
    want_s = M.aggregate(np.array([WR.wssim_ref(fa[f], fb[f], w) for f in range(6)]).reshape(2, 3), v1[0].shape)
    for got, want, tol in ((M.calculate_ws_psnr(v1, v2.to(DEV)), want_p, 1e-5), (M.calculate_ws_ssim(v1.to(DEV), v2), want_s, 1e-9)):
        assert got.keys() == want.keys() and got["video_setting"] == v1[0].shape and got["video_setting_name"] == want["video_setting_name"]
        assert abs(got["value_mean"] - want["value_mean"]) <= tol
        for k in ("value", "value_std"):
            assert max(abs(got[k][t] - want[k][t]) for t in range(3)) <= tol and len(got[k]) == 3
    p, s = M.video_metrics_ws_u8(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert abs(p.mean() - want_p["value_mean"]) <= 1e-5 and abs(s.mean() - want_s["value_mean"]) <= 1e-9
    with pytest.raises(AssertionError):
        M.calculate_ws_psnr(v1, v2[:, :2])


@pytest.mark.parametrize("H,W", [(35, 43), (58, 75)])
def test_vertical_flip_under_latitude_weights(H, W):
    from evoworld_amd import ops
    a, b = _pair(2, H, W, 3, 23)
    w = WR.latitude_weights(H)
    up = ops.video_metrics_ws(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), w)
    down = ops.video_metrics_ws(torch.from_numpy(a[:, ::-1].copy()).to(DEV), torch.from_numpy(b[:, ::-1].copy()).to(DEV), w)
    for u, d in zip(up, down):
        u, d = u.cpu().numpy(), d.cpu().numpy()
        assert np.abs(u - d).max() <= 1e-12 * max(1.0, np.abs(u).max())


def test_guarded_outputs_wsse_only_and_bit_identical_reruns():
    from evoworld_amd import ops
    a, b = _pair(5, 40, 61, 3, 11)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    w = _weights(40, 3)["random"]
    buf = torch.full((5 + 16,), float("nan"), dtype=torch.float64, device=DEV)
    buf2 = torch.full((5 + 16,), -7.25, dtype=torch.float64, device=DEV)
    wsse, wssim = ops.video_metrics_ws(ta, tb, w, wsse=buf[8:13], wssim=buf2[8:13])
    assert wsse.data_ptr() == buf[8:13].data_ptr() and wssim.data_ptr() == buf2[8:13].data_ptr()
    assert torch.isnan(buf[:8]).all() and torch.isnan(buf[13:]).all()
    assert (buf2[:8] == -7.25).all() and (buf2[13:] == -7.25).all()
    assert torch.isfinite(wsse).all() and torch.isfinite(wssim).all()
    s2, m2 = ops.video_metrics_ws(ta, tb, w)
    assert torch.equal(s2.view(torch.int64), wsse.view(torch.int64)) and torch.equal(m2.view(torch.int64), wssim.view(torch.int64))
    # what = 1: no wssim is written, and frames below the 11-pixel window are fine
    keep = torch.full((5,), -1.0, dtype=torch.float64, device=DEV)
    s3, m3 = ops.video_metrics_ws(ta, tb, w, what=ops.METRIC_SSE, wssim=keep)
    assert m3 is None and (keep == -1.0).all() and torch.equal(s3.view(torch.int64), wsse.view(torch.int64))
    keep_s = torch.full((5,), -1.0, dtype=torch.float64, device=DEV)
    s4, m4 = ops.video_metrics_ws(ta, tb, w, what=ops.METRIC_SSIM, wsse=keep_s)
    assert s4 is None and (keep_s == -1.0).all() and torch.equal(m4.view(torch.int64), wssim.view(torch.int64))
    small_a, small_b = a[:, :7, :9].copy(), b[:, :7, :9].copy()
    s5, _ = ops.video_metrics_ws(torch.from_numpy(small_a).to(DEV), torch.from_numpy(small_b).to(DEV), w[:7], what=ops.METRIC_SSE)
    fa, fb = (MR.u8_values(v).transpose(0, 3, 1, 2) for v in (small_a, small_b))
    for f in range(5):
        want = WR.wsse_ref(fa[f], fb[f], w[:7])
        assert abs(float(s5[f]) - want) <= 1e-12 * max(1.0, want)
    # the planar entry point returns what it returned before the weighted launch and after it
    p1 = ops.video_metrics(ta, tb)
    ops.video_metrics_ws(ta, tb, w)
    p2 = ops.video_metrics(ta, tb)
    assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(p1, p2))


def test_refusals():
    from evoworld_amd import _lib, ops
    from evoworld_amd._lib import EvoWorldHipError
    lib = _lib.load()
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    for C in (2, 4):
        with pytest.raises(EvoWorldHipError, match=f"C = {C}"):
            ops.video_metrics_ws(u8(2, 16, 16, C), u8(2, 16, 16, C), np.ones(16))
    for H, W in ((10, 16), (16, 10)):
        with pytest.raises(EvoWorldHipError, match="H, W >= 11"):
            ops.video_metrics_ws(u8(2, H, W, 3), u8(2, H, W, 3), np.ones(H))
    a, out, ws = u8(2, 16, 16, 3), torch.zeros(2, dtype=torch.float64, device=DEV), torch.zeros(4096, dtype=torch.uint8, device=DEV)
    rw = torch.ones(16, dtype=torch.float64, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.ew_video_metrics_ws_workspace_bytes(2, 3, 16, 16) == lib.ew_video_metrics_workspace_bytes(2, 3, 16, 16) <= 4096
    cases = [((0, 0, 3, 16, 16, 3, P(rw), P(out), P(out)), "positive"),
             ((0, 2, 3, 0, 16, 3, P(rw), P(out), P(out)), "positive"),
             ((0, 2, 3, 16, -1, 1, P(rw), P(out), P(out)), "positive"),
             ((0, 2, 2, 16, 16, 3, P(rw), P(out), P(out)), "C = 2"),
             ((0, 2, 3, 10, 16, 2, P(rw), P(out), P(out)), "H, W >= 11"),
             ((0, 2, 3, 16, 16, 3, None, P(out), P(out)), "NULL row_w"),
             ((0, 2, 3, 16, 16, 1, P(rw), None, P(out)), "SSE asked for with a NULL output"),
             ((0, 2, 3, 16, 16, 2, P(rw), P(out), None), "SSIM asked for with a NULL output"),
             ((2, 2, 3, 16, 16, 3, P(rw), P(out), P(out)), "layout 2"),
             ((0, 2, 3, 16, 16, 0, P(rw), P(out), P(out)), "what = 0")]
    for (layout, F_, C, H, W, what, r, s, m), msg in cases:
        st = lib.ew_video_metrics_ws(P(a), P(a), layout, F_, C, H, W, what, r, s, m, P(ws), None)
        err = lib.ew_last_error().decode()
        assert st != 0 and msg in err and "ew_video_metrics_ws" in err, (msg, err)
    # the host checks of the weights, before anything is launched
    edge = np.zeros(16)
    edge[:5] = 1.0
    for bad, what, msg in ((np.ones(15), 3, "expected 16"), (np.full(16, np.nan), 3, "finite"), (-np.ones(16), 1, ">= 0"),
                           (np.zeros(16), 1, "sum to zero"), (edge, 3, "centre rows")):
        with pytest.raises(ValueError, match=msg):
            ops.video_metrics_ws(a, a, bad, what)
    assert ops.video_metrics_ws(a, a, edge, ops.METRIC_SSE)[0].tolist() == [0.0, 0.0]            # zero centre rows are fine without SSIM
    with pytest.raises(ValueError):
        ops.video_metrics_ws(u8(2, 16, 16, 3), u8(2, 16, 17, 3), np.ones(16))
    with pytest.raises(TypeError):
        ops.video_metrics_ws(a.double(), a.double(), np.ones(16))


# ------------------------------------------------------------------ WS-LPIPS
def _lpips_pairs(seed, H, W):
    """uint8 [2,H,W,3] each: one pair of independent noise frames, one smooth textured frame against a copy perturbed by +-24 levels"""
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(H, dtype=torch.float32)[:, None, None]
    x = torch.arange(W, dtype=torch.float32)[None, :, None]
    c = torch.arange(3, dtype=torch.float32)[None, None, :]
    scene = (128 + 70 * torch.sin(0.05 * x * (c + 1) + 0.08 * y + 1.0) + 25 * torch.randn(H, W, 3, generator=g)).round().clamp(0, 255)
    pert = (scene + torch.randint(-24, 25, scene.shape, generator=g)).clamp(0, 255)
    noise = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    return torch.stack([noise[0], scene.to(torch.uint8)]), torch.stack([noise[1], pert.to(torch.uint8)])


def _ws_lpips_ref(a, b, sd, order, w):
    """sum over the taps of sum_yx w[y] up(y,x) / (W sum_y w[y]), one frame pair at a time, in fp64 over the fp32 maps"""
    W = a.shape[2]
    x, y = (t.permute(0, 3, 1, 2).float() / 255.0 for t in (a, b))
    wt = torch.from_numpy(w).view(1, 1, -1, 1)
    out = []
    for i in range(a.shape[0]):
        maps = lpips_ref.tap_maps(x[i:i + 1], y[i:i + 1], sd, order)
        out.append(float(sum((m.double() * wt).sum() for m in maps) / (W * w.sum())))
    return np.array(out)


def _ws_lpips_worst(H, W):
    from evoworld_amd.lpips import LPIPSAlex
    sd = lpips_ref.random_weights(3)
    model = LPIPSAlex.from_state_dict(sd, DEV)
    a, b = _lpips_pairs(H * W, H, W)
    worst = 0.0
    for name, w in _weights(H, 7).items():
        for order in ("rgb", "bgr"):
            got = model(a.to(DEV), b.to(DEV), order, row_weights=w)
            assert got.dtype == torch.float64 and got.shape == (2,) and got.is_cuda
            want = _ws_lpips_ref(a, b, sd, order, w)
            rel = np.abs(got.cpu().numpy() - want) / want
            plain = model(a.to(DEV), b.to(DEV), order).cpu().numpy()
            print(f"WS-LPIPS {H}x{W} {name} {order}: ref {want.tolist()} rel err {rel.tolist()} (plain LPIPS {plain.tolist()})")
            assert (np.abs(got.cpu().numpy() - plain) / plain > 1e-4).any()               # the weights do change the number
            worst = max(worst, float(rel.max()))
    print(f"WS-LPIPS {H}x{W}: worst relative error per frame pair {worst:.3e}")
    return worst


@pytest.mark.parametrize("H,W", [(64, 96), (70, 93)])
def test_ws_lpips_against_the_weighted_restatement(H, W):
    worst = _ws_lpips_worst(H, W)
    assert worst <= WS_LPIPS_BOUND


def test_ws_lpips_under_unit_weights_is_plain_lpips_bit_for_bit():
    from evoworld_amd.lpips import LPIPSAlex
    model = LPIPSAlex.from_state_dict(lpips_ref.random_weights(3), DEV)
    for H, W in ((64, 96), (70, 93)):
        a, b = (t.to(DEV) for t in _lpips_pairs(H + W, H, W))
        plain = model(a, b)
        assert torch.equal(model(a, b, row_weights=np.ones(H)).view(torch.int64), plain.view(torch.int64))
        assert torch.equal(model(a, b, row_weights=torch.ones(H)).view(torch.int64), plain.view(torch.int64))
        assert torch.equal(model(a, a, row_weights=WR.latitude_weights(H)), torch.zeros(2, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="expected 70"):
        model(a, b, row_weights=np.ones(64))


def test_cli_ws_lpips(tmp_path):
    """--metrics lpips,ws_lpips: the CLI's values are LPIPSAlex's under latitude weights, fed B, G, R planes by default, aggregated as
    every other metric; the keys come in the documented order"""
    import os
    from PIL import Image
    from safetensors.torch import save_file
    from evoworld_amd import metrics as M
    from evoworld_amd.lpips import LPIPSAlex
    H, W = 48, 80
    pairs = [_lpips_pairs(40 + i, H, W) for i in range(2)]
    for e, (a, b) in enumerate(pairs):
        for sub, v in (("predictions_gt_0", a), ("predictions_0", b)):
            d = tmp_path / f"ep_{e:03d}" / sub
            os.makedirs(d)
            for t in range(2):
                Image.fromarray(v[t].numpy()).save(d / f"{t + 1:03}.png")
    sd = lpips_ref.random_weights(5)
    weights = str(tmp_path / "lpips_alex.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, weights)
    argv = ["--data_path", str(tmp_path), "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0", "--lpips_weights", weights]
    got, _ = M.main(argv + ["--metrics", "psnr,lpips,ws_psnr,ws_lpips"])
    assert list(got) == ["psnr", "lpips", "ws_psnr", "ws_lpips", "not_computed"]
    assert set(got["not_computed"]) == {"fvd", "latent_mse", "loop_closure_latent_mse"}
    model = LPIPSAlex.from_state_dict(sd, DEV)
    rows = [model(a.to(DEV), b.to(DEV), "bgr", row_weights=WR.latitude_weights(H)).cpu().numpy() for a, b in pairs]
    assert got["ws_lpips"] == M.aggregate(rows, torch.Size([2, 3, H, W])) and got["ws_lpips"]["value_mean"] != got["lpips"]["value_mean"]
    only, _ = M.main(argv + ["--metrics", "ws_lpips"])
    assert list(only) == ["ws_lpips", "not_computed"] and "lpips" in only["not_computed"] and only["ws_lpips"] == got["ws_lpips"]
