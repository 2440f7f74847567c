"""-m "not gpu": the host side of the opt-in fp8 (e4m3) q / k / v projections (BASELINE.json configs[4]) -- the CPU reference's
self-checks, the ABI declaration, the command-line flag and the config key."""
import os
import re

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
