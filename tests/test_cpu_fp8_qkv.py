"""-m "not gpu": the host side of the opt-in fp8 (e4m3) q / k / v projections (BASELINE.json configs[4]) -- the CPU reference's
self-checks, the ABI declaration, the command-line flag and the config key."""
import os
import re

import pytest
import torch

import fp8_ref
from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, "include", "evoworld_hip.h")).read()


def test_ref_round_trip_of_representable_values_is_exact():
    """Values exactly representable in e4m3 whose row maximum is 448 (scale exactly 1) survive quantise -> dequantise bit for bit;
    so do the same rows times a power of two (the scale is then that power of two)."""
    grid = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    grid = grid[torch.isfinite(grid)]
    assert grid.numel() == 254 and float(grid.abs().max()) == 448.0
    g = torch.Generator().manual_seed(0)
    x = grid[torch.randint(0, grid.numel(), (37, 64), generator=g)]
    x[:, 5] = 448.0
    for mul in (1.0, 0.125, 4.0):
        q, s = fp8_ref.quant_rows(x * mul)
        assert torch.equal(s, torch.full((37,), mul))
        assert torch.equal(fp8_ref.deq(q, s), x * mul)


def test_ref_zero_row_gets_scale_one():
    x = torch.randn(4, 32, generator=torch.Generator().manual_seed(1))
    x[2] = 0
    q, s = fp8_ref.quant_rows(x)
    assert float(s[2]) == 1.0 and int(q[2].to(torch.int32).abs().sum()) == 0
    assert torch.allclose(s[[0, 1, 3]], x[[0, 1, 3]].abs().amax(1) / 448.0, rtol=1e-6)
    assert torch.isfinite(fp8_ref.deq(q, s)).all()


# ------------------------------------------------------------------------------------------------ the independent e4m3 encoder
def _torch_bytes(x):
    return x.to(torch.float8_e4m3fn).view(torch.uint8)


def test_encoder_equals_torch_on_every_fp16_value_up_to_448():
    t = fp8_ref.fp16_convert_table()
    vals = t[:, 1:].reshape(-1)[:48642].float()
    assert vals.numel() == 48642 and float(vals.abs().max()) == 448.0 and int((vals.view(torch.int32) == -(1 << 31)).sum()) == 1      # -0.0 is in
    fp8_ref.assert_bits(fp8_ref.e4m3_rne_bytes(vals), _torch_bytes(vals), "encoder vs torch on fp16 values")
    assert torch.equal(fp8_ref.e4m3_rne_bytes(t.float()), _torch_bytes(t.float()))


def test_encoder_equals_torch_on_every_midpoint_and_one_ulp_either_side():
    grid = torch.arange(0, 0x7F, dtype=torch.uint8).view(torch.float8_e4m3fn).float()         # 0 .. 448, ascending
    assert grid.numel() == 127 and bool((grid[1:] > grid[:-1]).all())
    mid = (grid[1:] + grid[:-1]) / 2                                                          # exact in fp32
    assert torch.equal(mid.double(), (grid[1:].double() + grid[:-1].double()) / 2)
    inf = torch.tensor(float("inf"))
    pts = torch.cat([mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf)])
    pts = torch.cat([pts, -pts])
    got = fp8_ref.e4m3_rne_bytes(pts)
    fp8_ref.assert_bits(got, _torch_bytes(pts), "encoder vs torch around the midpoints")
    # ties go to the even code; one ulp above / below goes up / down
    n = mid.numel()
    lo = torch.arange(0, 126, dtype=torch.uint8)
    assert torch.equal(got[:n], lo + (lo & 1)) and torch.equal(got[n: 2 * n], lo + 1) and torch.equal(got[2 * n: 3 * n], lo)


def test_encoder_row_maximum_always_encodes_to_0x7e():
    """fl(amax * fl(1 / fl(amax / 448))) lies in [447.99997, 448.00003] for every positive finite fp16 amax: the largest finite code"""
    a = fp8_ref.positive_fp16().float()
    assert a.numel() == 31743
    top = a * (1.0 / (a / 448.0))
    assert 447.99996 < float(top.min()) and float(top.max()) < 448.00004 and float(top.max()) > 448.0
    assert bool((fp8_ref.e4m3_rne_bytes(top) == 0x7E).all()) and bool((fp8_ref.e4m3_rne_bytes(-top) == 0xFE).all())
    q, s = fp8_ref.quant_rows_independent(fp8_ref.amax_sweep_rows())
    assert torch.equal(s, a / 448.0) and bool((q[:, 0] == 0x7E).all()) and bool((q[:, 1] == 0xFE).all()) and not bool(q[:, 3:].any())


def test_encoder_nan_and_overflow():
    """464 is the tie between 448 (even) and the would-be 480 and stays 448; anything above rounds to the NaN code"""
    x = torch.tensor([464.0, 464.00003, 1e9, float("inf"), float("nan"), -464.00003, -464.0])
    assert fp8_ref.e4m3_rne_bytes(x).tolist() == [0x7E, 0x7F, 0x7F, 0x7F, 0x7F, 0xFF, 0xFE]
    assert torch.equal(fp8_ref.e4m3_rne_bytes(x[:3]), _torch_bytes(x[:3]))


def test_independent_quantiser_equals_the_torch_one():
    for x in (fp8_ref.real_rows(1000, 640), fp8_ref.real_rows(9, 2048, seed=3, mul=0.7), fp8_ref.fp16_convert_table()):
        q, s = fp8_ref.quant_rows(x)
        qi, si = fp8_ref.quant_rows_independent(x)
        assert torch.equal(s, si)
        fp8_ref.assert_bits(qi, q, "independent quantiser vs torch's cast")


# ------------------------------------------------------------------------------------------------ emulated faults: the bit checks reject them
def _rejected(got, want, what):
    with pytest.raises(AssertionError, match="differ in their bits"):
        fp8_ref.assert_bits(got, want, what)


@pytest.mark.parametrize("M,N,K", [s for s in fp8_ref.INT_SHAPES if s[0] > 1])
@pytest.mark.parametrize("variant", fp8_ref.INT_VARIANTS)
def test_integer_gemm_check_rejects_dropped_k_tile_and_duplicated_row(M, N, K, variant):
    """The GPU test's inputs and comparison: a kernel that skips the last 64-byte K-tile, or stores row M - 1 into row M - 2 as well,
    does not pass at any shape, variant or c_acc."""
    from evoworld_amd import ops
    c = fp8_ref.int_gemm_case(M, N, K, variant)
    short = fp8_ref.int_gemm_acc(c["aq"][:, : K - 64], c["wq"][:, : K - 64]) if K > 64 else torch.zeros(M, N, dtype=torch.float64)
    for c_acc in (1.0, 0.25, ops.QK_LOG2_PRESCALE):
        want = fp8_ref.int_gemm_expect(c["acc"], c["sa"], c["sw"], c_acc)
        fp8_ref.assert_bits(fp8_ref.int_gemm_expect(fp8_ref.int_gemm_acc(c["aq"], c["wq"]), c["sa"], c["sw"], c_acc), want, "restatement")
        _rejected(fp8_ref.int_gemm_expect(short, c["sa"], c["sw"], c_acc), want, "dropped last K-tile")
        dup = want.clone()
        dup[M - 2] = dup[M - 1]
        _rejected(dup, want, "row M-1 duplicated into row M-2")


def test_integer_gemm_single_row_shape_rejects_dropped_k_tile():
    c = fp8_ref.int_gemm_case(1, 4, 64, "positive")
    want = fp8_ref.int_gemm_expect(c["acc"], c["sa"], c["sw"], 1.0)
    assert float(c["acc"].min()) >= 30 * 64
    _rejected(torch.zeros_like(want), want, "dropped only K-tile")


@pytest.mark.parametrize("M,N,K", fp8_ref.INT_SHAPES)
def test_integer_gemm_check_rejects_swapped_scale_order(M, N, K):
    """((acc * c_acc) * sw) * sa instead of ((acc * sa) * sw) * c_acc, c_acc = QK_LOG2_PRESCALE: the `mixed` variant (scales with full
    fp32 significands and exponents 2^-124 / 2^124 apart) rejects it, and ((acc * sw) * sa) * c_acc too.  With power-of-two scales the
    orders round alike -- which is why that variant exists."""
    from evoworld_amd import ops
    c = fp8_ref.int_gemm_case(M, N, K, "mixed")
    cc = torch.tensor(ops.QK_LOG2_PRESCALE, dtype=torch.float32)
    want = fp8_ref.int_gemm_expect(c["acc"], c["sa"], c["sw"], ops.QK_LOG2_PRESCALE)
    swapped = (((c["acc"].float() * cc) * c["sw"][None, :]) * c["sa"][:, None]).half()
    _rejected(swapped, want, "scales in swapped order")
    _rejected((((c["acc"].float() * c["sw"][None, :]) * c["sa"][:, None]) * cc).half(), want, "w_scale before a_scale")
    assert bool(torch.isfinite(want).all())
    p = fp8_ref.int_gemm_case(M, N, K, "signed")
    same = (((p["acc"].float() * cc) * p["sw"][None, :]) * p["sa"][:, None]).half()
    fp8_ref.assert_bits(same, fp8_ref.int_gemm_expect(p["acc"], p["sa"], p["sw"], ops.QK_LOG2_PRESCALE), "power-of-two scales commute")


def test_integer_gemm_outputs_exercise_the_fp16_rounding():
    """`positive`: most sums need more than 11 significant bits, and some are exact ties of the fp16 grid"""
    for M, N, K in fp8_ref.INT_SHAPES:
        c = fp8_ref.int_gemm_case(M, N, K, "positive")
        y32 = (c["acc"].float() * c["sa"][:, None]) * c["sw"][None, :]
        y16 = y32.half()
        inexact = y16.float() != y32
        assert float(inexact.float().mean()) > 0.25 or M * N < 16, (M, N, K)
        if M * N >= 1000:
            ulp = torch.ldexp(torch.ones_like(y32), torch.frexp(y32)[1] - 11)      # fp16 spacing at y32
            assert bool(((y32 - y16.float()).abs() * 2 == ulp).any()), (M, N, K)


def test_quantiser_check_rejects_division_by_the_scale():
    """bytes = e4m3(x / s) instead of e4m3(x * (1 / s)): 23 bytes of the suite's 1000 x 640 input differ, and the byte comparison sees them"""
    x = fp8_ref.real_rows(1000, 640)
    q, s = fp8_ref.quant_rows_independent(x)
    qd, sd = fp8_ref.quant_rows_by_division(x)
    assert torch.equal(s, sd) and int((q != qd).sum()) == 23
    _rejected(qd, q, "quantiser dividing by the scale")


def test_real_gemm_fp32_accumulation_error_is_negligible():
    """The figure tests/test_gpu_fp8_qkv.py adds to 2^-11 in its per-row bound: a plain fp32 restatement of the scaled sum (no fp16
    rounding) against fp64 on the same dequantised bytes -- worst row below 1e-6 at every shape of that test."""
    from kernel_checks import worst_row
    for M, N, K in fp8_ref.REAL_SHAPES:
        x, w = fp8_ref.real_rows(M, K), fp8_ref.real_weights(N, K)
        (xq, xs), (wq, ws) = fp8_ref.quant_rows(x), fp8_ref.quant_rows(w)
        acc32 = xq.view(torch.float8_e4m3fn).float() @ wq.view(torch.float8_e4m3fn).float().T
        y32 = (acc32 * xs[:, None]) * ws[None, :]
        exact = fp8_ref.deq(xq, xs).double() @ fp8_ref.deq(wq, ws).double().T
        e = worst_row(y32, exact)[0]
        print(f"fp32 restatement {M}x{N}x{K}: worst row {e:.3e}")
        assert e < fp8_ref.FP32_ACC_ERR


def test_ref_fake_quant_unet_hooks_self_attention_only():
    """The hooks sit on attn1's to_q / to_k / to_v of every transformer (tiny config: widths 64, 128, 256), change the output, and leave
    the plain oracle behind when they are removed."""
    from evoworld_amd.unet import DEFAULT_CONFIG, _arch
    from oracle.unet_ref import UNetSpatioTemporalConditionModelRef, tiny_config
    cfg = tiny_config()
    ref = UNetSpatioTemporalConditionModelRef(**cfg).eval()
    handles, names = fp8_ref.fake_quant_unet(ref)
    n_tr = len(_arch({**DEFAULT_CONFIG, **cfg}).trs)
    assert len(names) == 2 * n_tr and all(n.endswith(".attn1") for n in names)       # spatial + temporal block of each transformer
    assert len(handles) == 2 * 3 * len(names)
    lin = dict(ref.named_modules())[names[0]].to_q
    w = lin.weight.data.clone()
    x = torch.randn(3, 5, lin.in_features, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        y_q = lin(x)
        assert torch.equal(lin.weight.data, w)                                        # the weight is swapped for the call only
        assert torch.equal(y_q, torch.nn.functional.linear(fp8_ref.fake_quant(x), fp8_ref.fake_quant(w)))
        for h in handles:
            h.remove()
        assert torch.equal(lin(x), torch.nn.functional.linear(x, w))


def test_header_declares_fp8_pair_with_c_acc():
    hdr = re.sub(r"\s+", " ", _header())
    assert "ew_status ew_quant_rows_fp8(const void* x, void* q, float* scale, int rows, int K, void* stream);" in hdr
    assert ("ew_status ew_gemm_fp8(const void* a, const float* a_scale, const void* w, const float* w_scale, void* out, int M, int N, int K, "
            "long long ld_out, float c_acc, void* stream);") in hdr


def test_abi_version_at_least_15():
    from evoworld_amd import _lib
    version = int(re.search(r"#define EW_ABI_VERSION (\d+)", _header()).group(1))
    assert version >= 15 and version == _lib.ABI_VERSION
    lib = _lib.load()
    for s in ("ew_quant_rows_fp8", "ew_gemm_fp8"):
        assert s in _lib.HEADER.functions, s
        assert (getattr(lib, s).restype, list(getattr(lib, s).argtypes)) == _lib.HEADER.signatures[s], s


def test_cli_flag_defaults_off():
    from unified_loop_consistency import parse_arguments
    assert parse_arguments(["--unet_path", "x"]).qkv_fp8 is False
    assert parse_arguments(["--unet_path", "x", "--qkv_fp8"]).qkv_fp8 is True


def test_config_key(monkeypatch):
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel
    monkeypatch.delenv("EW_QKV_FP8", raising=False)
    assert UNetSpatioTemporalConditionModel(qkv_fp8=True).config.qkv_fp8 is True
    assert UNetSpatioTemporalConditionModel().config.qkv_fp8 is False
    monkeypatch.setenv("EW_QKV_FP8", "1")
    assert UNetSpatioTemporalConditionModel().config.qkv_fp8 is True
    assert UNetSpatioTemporalConditionModel(qkv_fp8=False).config.qkv_fp8 is False      # the keyword wins over the environment
