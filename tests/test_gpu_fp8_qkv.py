"""-m gpu: the opt-in fp8 (OCP e4m3) q / k / v projection path of BASELINE.json configs[4] (ew_quant_rows_fp8, ew_gemm_fp8,
UNetSpatioTemporalConditionModel(qkv_fp8=True)) against the fp32 CPU reference of tests/fp8_ref.py.

Stated tolerances, none of them taken from what the kernels give:
  * quantiser: scales = amax / 448 to rtol 1e-6 (one fp32 division); rel-L2(dequantised rows, x) <= 1.02 x the same quantity of the
    CPU reference on the same input (2.5e-2 ... 2.7e-2 for these inputs: e4m3 keeps 3 mantissa bits) -- the 2 % covers a handful of
    ties falling the other way in the hardware convert;
  * GEMM against fp32 deq(a) @ deq(w).T of the SAME bytes: rel-L2 <= 5e-4 -- the products and the fp32 accumulation of e4m3 values are
    as good as exact, only the fp16 rounding of the output is left, at most 2^-11 = 4.9e-4 per element (a CPU restatement, fp32 product
    rounded to fp16, measures 2.1e-4);
  * tiny U-Net forward: rel-L2(GPU fp8 forward, plain fp32 oracle) <= 1.5 x E_ref, E_ref = rel-L2(fake-quantised fp32 oracle, plain fp32
    oracle) computed here on the CPU -- the factor covers the fp16 path's own <= 1e-3 added in quadrature and roundings that flip near
    e4m3 boundaries (the product quantises fp16 LayerNorm outputs, the oracle fp32 ones).
    E_ref on the CPU: seed 0: 6.31e-3, seed 1: 7.00e-3, seed 2: 6.74e-3 (the rounds 2-4 device figure was 6.4e-3); the test prints both sides."""
import functools
import math

import pytest
import torch

import fp8_ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(300, 640, 320), (1000, 132, 640), (132, 1280, 1280), (64, 64, 64)]     # ragged M / N tiles, N % 128 == 4, one and many K-tiles
RAGGED = SHAPES[:3]


def _g(s):
    return torch.Generator().manual_seed(s)


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Inputs and CPU references of one GEMM shape, computed once and shared (read-only) by the tests below."""
    x = (torch.randn(M, K, generator=_g(1)) * 1.5).half()
    w = torch.randn(N, K, generator=_g(2)) / math.sqrt(K)
    xq, xs = fp8_ref.quant_rows(x)
    wq, ws = fp8_ref.quant_rows(w)
    exact = fp8_ref.deq(xq, xs) @ fp8_ref.deq(wq, ws).T
    return dict(x=x, xq=xq, xs=xs, wq=wq, ws=ws, exact=exact)


def _dev(c, *names):
    return [c[n].to(DEV).contiguous() for n in names]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_quant_rows_fp8(M, N, K):
    from evoworld_amd import ops
    c = _case(M, N, K)
    x = c["x"]
    q, s = ops.quant_rows_fp8(x.to(DEV))
    assert q.dtype == torch.uint8 and tuple(q.shape) == (M, K) and s.dtype == torch.float32 and tuple(s.shape) == (M,)
    q, s = q.cpu(), s.cpu()
    assert torch.allclose(s, x.float().abs().amax(1) / 448.0, rtol=1e-6, atol=0)
    e_ref = rel_l2(fp8_ref.deq(c["xq"], c["xs"]), x.float())
    e_gpu = rel_l2(fp8_ref.deq(q, s), x.float())
    differ = int((q != c["xq"]).sum())
    print(f"quant_rows_fp8 {M}x{K}: rel-L2 to x: device {e_gpu:.4e}, CPU reference {e_ref:.4e}; {differ} of {q.numel()} bytes differ from the reference's")
    assert torch.isfinite(fp8_ref.deq(q, s)).all()
    assert e_gpu <= 1.02 * e_ref


def test_quant_rows_fp8_zero_row_and_wide_row():
    """An all-zero row gets scale 1 and zero bytes; K = 2048 (the widest row, four vectors per lane) and K = 8 (one lane) quantise as the reference does"""
    from evoworld_amd import ops
    for K in (8, 1280 + 8, 2048):
        x = (torch.randn(9, K, generator=_g(3)) * 0.7).half()
        x[4] = 0
        q, s = ops.quant_rows_fp8(x.to(DEV))
        q, s = q.cpu(), s.cpu()
        rq, rs = fp8_ref.quant_rows(x)
        assert float(s[4]) == 1.0 and int(q[4].to(torch.int32).sum()) == 0
        assert torch.allclose(s, rs, rtol=1e-6, atol=0)
        assert rel_l2(fp8_ref.deq(q, s), x.float()) <= 1.02 * rel_l2(fp8_ref.deq(rq, rs), x.float())


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_fp8_vs_fp32_product_of_same_bytes(M, N, K):
    from evoworld_amd import ops
    c = _case(M, N, K)
    xq, xs, wq, ws = _dev(c, "xq", "xs", "wq", "ws")
    exact = c["exact"]
    out = ops.gemm_fp8(xq, xs, wq, ws)
    assert out.dtype == torch.float16 and tuple(out.shape) == (M, N)
    e = rel_l2(out.float().cpu(), exact)
    # swapped roles = the transposed product (how V^T is produced); needs the new N (= M) % 4 == 0
    eT = rel_l2(ops.gemm_fp8(wq, ws, xq, xs).float().cpu(), exact.T)
    # c_acc multiplies before the fp16 rounding
    ec = rel_l2(ops.gemm_fp8(xq, xs, wq, ws, c_acc=ops.QK_LOG2_PRESCALE).float().cpu(), exact * ops.QK_LOG2_PRESCALE)
    print(f"gemm_fp8 {M}x{N}x{K}: rel-L2 {e:.3e}, swapped {eT:.3e}, c_acc {ec:.3e}")
    assert e <= 5e-4 and eT <= 5e-4 and ec <= 5e-4


def test_gemm_fp8_asymmetric_identity():
    """A = I (exact in e4m3) against an asymmetric W of small integers, all scales 1: the output is W^T bit for bit.  Catches row / column
    or k-slice permutations of the fragment layout."""
    from evoworld_amd import ops
    K = 128
    eye = torch.eye(K).to(torch.float8_e4m3fn).view(torch.uint8).to(DEV).contiguous()
    w = ((torch.arange(192 * K).reshape(192, K) % 13) - 6).float()
    wq = w.to(torch.float8_e4m3fn).view(torch.uint8).to(DEV).contiguous()
    one_m, one_n = torch.ones(K, device=DEV), torch.ones(192, device=DEV)
    out = ops.gemm_fp8(eye, one_m, wq, one_n)
    assert torch.equal(out.float().cpu(), w.T.contiguous())
    outT = ops.gemm_fp8(wq, one_n, eye, one_m)
    assert torch.equal(outT.float().cpu(), w)


@pytest.mark.parametrize("M,N,K", RAGGED)
def test_gemm_fp8_guarded_output(M, N, K):
    """out with ld_out > N and sentinel rows after M: the padding columns and the sentinel rows come back untouched, the inside equals the plain call's bits"""
    from evoworld_amd import ops
    c = _case(M, N, K)
    xq, xs, wq, ws = _dev(c, "xq", "xs", "wq", "ws")
    for (aq, a_s, bq, b_s, m, n) in ((xq, xs, wq, ws, M, N), (wq, ws, xq, xs, N, M)):
        plain = ops.gemm_fp8(aq, a_s, bq, b_s)
        SENT = -777.0
        buf = torch.full((m + 8, n + 8), SENT, dtype=torch.float16, device=DEV)
        ops.gemm_fp8(aq, a_s, bq, b_s, out=buf[:m, :n])
        assert torch.equal(buf[:m, :n], plain)
        assert bool((buf[m:] == SENT).all()) and bool((buf[:, n:] == SENT).all())


def test_gemm_fp8_refuses_bad_shapes():
    from evoworld_amd import _lib, ops
    q = torch.zeros(64, 96, dtype=torch.uint8, device=DEV)
    s = torch.ones(64, device=DEV)
    with pytest.raises(_lib.EvoWorldHipError):
        ops.gemm_fp8(q, s, q, s)                                   # K % 64 != 0
    q2, s2 = torch.zeros(6, 64, dtype=torch.uint8, device=DEV), torch.ones(6, device=DEV)
    q1, s1 = torch.zeros(64, 64, dtype=torch.uint8, device=DEV), torch.ones(64, device=DEV)
    with pytest.raises(_lib.EvoWorldHipError):
        ops.gemm_fp8(q1, s1, q2, s2)                               # N % 4 != 0
    with pytest.raises(_lib.EvoWorldHipError):
        ops.quant_rows_fp8(torch.zeros(4, 2056, dtype=torch.float16, device=DEV))      # K > 2048


# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_inputs(seed):
    """Tiny config, an fp16-representable random checkpoint and the inputs of tests/test_gpu_unet.py (B=2, T=4, 16x32), shared read-only"""
    from evoworld_amd.unet import DEFAULT_CONFIG, random_state_dict
    from oracle.unet_ref import tiny_config
    cfg = tiny_config()
    sd = {k: v.half().float() for k, v in random_state_dict({**DEFAULT_CONFIG, **cfg}, seed).items()}
    B, T, h, w = 2, 4, 16, 32
    g = _g(seed + 1)
    x = torch.randn(B, T, 18, h, w, generator=g)
    ehs = torch.randn(B, 1, cfg["cross_attention_dim"], generator=g)
    ehs[0] = 0
    ids = torch.tensor([[6.0, 127.0, 0.02]] * B)
    return cfg, sd, (x, torch.tensor(1.6377), ehs, ids)


@functools.lru_cache(maxsize=None)
def _oracle(seed):
    """(plain fp32 oracle output, fake-quantised oracle output, names of the hooked Attention modules), computed once per seed on the CPU"""
    from oracle.unet_ref import UNetSpatioTemporalConditionModelRef
    cfg, sd, inp = _tiny_inputs(seed)
    ref = UNetSpatioTemporalConditionModelRef(**cfg).eval()
    ref.load_state_dict(sd, strict=True)
    with torch.no_grad():
        plain = ref(*inp)
        handles, names = fp8_ref.fake_quant_unet(ref)
        fq = ref(*inp)
        for h in handles:
            h.remove()
    return plain, fq, names


def _tiny(seed, **kw):
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel
    cfg, sd, inp = _tiny_inputs(seed)
    return UNetSpatioTemporalConditionModel(**kw, **cfg).load_state_dict(sd, device=DEV), inp


def _run(m, inp):
    x, t, ehs, ids = inp
    return m(x.to(DEV), t, ehs.to(DEV), ids.to(DEV), return_dict=False)[0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_unet_tiny_fp8_qkv_vs_oracle(seed):
    m, inp = _tiny(seed, qkv_fp8=True)
    assert m.config.qkv_fp8 is True
    assert m.fp8_blocks and m.fp8_blocks == [t.p for t in m.arch.trs]         # every tiny-config width (64, 128, 256) is a multiple of 64
    plain, fq, names = _oracle(seed)
    assert len(names) == 2 * len(m.fp8_blocks)                                # the spatial and the temporal attn1 of each block
    e_ref = rel_l2(fq, plain)
    got = _run(m, inp)
    e = rel_l2(got.cpu(), plain)
    print(f"unet tiny forward, seed {seed}: E_ref (fake-quantised oracle vs plain oracle) {e_ref:.3e}; fp8 q/k/v on the device vs plain oracle {e:.3e}; "
          f"device vs fake-quantised oracle {rel_l2(got.cpu(), fq):.3e}")
    assert torch.isfinite(got).all()
    assert e_ref > 1e-3                   # the hooks did something: e4m3 projections sit well above the fp16 path's error
    assert e <= 1.5 * e_ref


def test_qkv_fp8_false_is_the_default_model(monkeypatch):
    """qkv_fp8=False and no key at all: the same packed tensors and bit-identical forwards (the fp16 default does not change)"""
    monkeypatch.delenv("EW_QKV_FP8", raising=False)
    m_off, inp = _tiny(0, qkv_fp8=False)
    m_def, _ = _tiny(0)
    assert m_off.fp8_blocks == [] and m_def.fp8_blocks == [] and m_def.config.qkv_fp8 is False
    a, b = m_off.packed_tensors(), m_def.packed_tensors()
    assert len(a) == len(b) and all(s.dtype == d.dtype and torch.equal(s, d) for s, d in zip(a, b))
    assert not any(t.dtype == torch.uint8 for t in a)
    assert torch.equal(_run(m_off, inp), _run(m_def, inp))


def test_attn_log2_off_still_works_with_fp8():
    """attn_log2 = False (the scale-and-shift attention kernel): the q|k prescale is then 1 on the fp8 path too; same bound as above"""
    m, inp = _tiny(0, qkv_fp8=True)
    m.attn_log2 = False
    plain, fq, _ = _oracle(0)
    got = _run(m, inp)
    e, e_ref = rel_l2(got.cpu(), plain), rel_l2(fq, plain)
    print(f"unet tiny forward, seed 0, attn_log2 off: fp8 q/k/v on the device vs plain oracle {e:.3e} (E_ref {e_ref:.3e})")
    assert torch.isfinite(got).all() and e <= 1.5 * e_ref


def test_fp8_weight_packs_travel_with_packed_tensors():
    """The fp8 q/k/v packs are (bytes, scales) tuples nested in the per-block dicts; `packed_tensors()` (what `broadcast_weights` ships and
    `weights_checksum` sums) must include them, or every rank but 0 keeps all-zero fp8 weights.  Simulates the broadcast in one process:
    copy rank 0's packed tensors into a from_zeros replica, checksums equal and forwards bit-identical."""
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel
    from oracle.unet_ref import tiny_config
    cfg = tiny_config()
    src = UNetSpatioTemporalConditionModel.from_random(seed=3, device=DEV, qkv_fp8=True, **cfg)
    dst = UNetSpatioTemporalConditionModel.from_zeros(device=DEV, qkv_fp8=True, **cfg)
    a, b = src.packed_tensors(), dst.packed_tensors()
    assert len(a) == len(b) and any(t.dtype == torch.uint8 for t in a)          # the e4m3 bytes are in the list
    for s_, d_ in zip(a, b):
        assert s_.shape == d_.shape and s_.dtype == d_.dtype
        d_.copy_(s_)
    for k in src.w:
        if isinstance(src.w[k], dict) and "mix" in src.w[k]:
            dst.w[k]["mix"] = src.w[k]["mix"]
    assert abs(src.weights_checksum() - dst.weights_checksum()) == 0.0
    g = _g(0)
    x = torch.randn(2, cfg["num_frames"], 18, 16, 32, generator=g).to(DEV)
    ehs = torch.randn(2, 1, cfg["cross_attention_dim"], generator=g).to(DEV)
    ids = torch.tensor([[6.0, 127.0, 0.02]] * 2).to(DEV)
    ya = src(x, torch.tensor(1.0), ehs, ids, return_dict=False)[0]
    yb = dst(x, torch.tensor(1.0), ehs, ids, return_dict=False)[0]
    assert torch.equal(ya, yb) and float(ya.abs().mean()) > 0
