"""CPU reference of the opt-in fp8 (OCP e4m3) q / k / v projection path, in fp32 PyTorch (no GPU, no project kernels):
  quant_rows / deq     the row-wise quantiser of ew_quant_rows_fp8 and its inverse;
  fake_quant_unet      the path's arithmetic restated on the fp32 oracle: forward hooks on to_q / to_k / to_v of every
                       self-attention `Attention` module whose width is a multiple of 64 replace the Linear's input and weight by
                       their row-wise e4m3 fake-quantised values (one scale per token row, one per weight row).  The cross-attention
                       modules (attn2: one key/value token, folded away in the product) are left alone.
Shared by tests/test_cpu_fp8_qkv.py and tests/test_gpu_fp8_qkv.py."""
import math

import torch

FP8_MAX = 448.0     # largest finite e4m3fn value


def quant_rows(x):
    """x [rows, K] (any float dtype) -> (uint8 [rows, K] e4m3 bytes, fp32 scale [rows]): s = amax / 448 (1 for an all-zero row),
    bytes = e4m3(x * (1 / s)), round to nearest even."""
    x = x.float()
    amax = x.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (x * (1.0 / s)[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), s


def deq(q, s):
    """e4m3 bytes uint8 [rows, K], fp32 scale [rows] -> fp32 [rows, K]"""
    return q.view(torch.float8_e4m3fn).float() * s.float()[:, None]


def e4m3_rne_bytes(x):
    """fp32 tensor -> uint8 e4m3fn codes, round to nearest even, in fp64 / integer arithmetic only (no torch.float8_e4m3fn):
    the grid has step 2^-9 below 2^-6 (denormals and zero) and 2^(e-3) in [2^e, 2^(e+1)), e = -6 .. 8, up to 448 = 1.75 * 2^8.
    Every scaling below is by a power of two, so exact in fp64; torch.round rounds halves to even.  A magnitude that rounds past
    448 (> 464: 464 itself is a tie and goes to the even 448) and NaN give 0x7F / 0xFF, the format's NaN: e4m3fn has no infinity."""
    assert x.dtype == torch.float32
    a = x.double().abs()
    sign = ((x.view(torch.int32) >> 31) & 1).to(torch.int64) << 7            # the sign BIT: -0.0 keeps it
    _, ex = torch.frexp(a)                                                    # a = m * 2^ex, m in [0.5, 1)
    e = (ex.to(torch.int64) - 1).clamp(min=-6)                                # below 2^-6: the denormal step of exponent -6
    q = torch.round(torch.ldexp(a, (3 - e).to(torch.int32))).to(torch.int64)  # a / 2^(e-3): 0 .. 8 (denormal), 8 .. 16 (normal)
    up = q == 16                                                              # rounded up into the next binade
    e = torch.where(up, e + 1, e)
    q = torch.where(up, torch.full_like(q, 8), q)
    code = torch.where(q < 8, q, ((e + 7) << 3) | (q - 8))                    # q < 8 only in the denormal range (biased exponent 0)
    code = torch.where((code >= 0x7F) | torch.isnan(a) | torch.isinf(a), torch.full_like(code, 0x7F), code)
    return (sign | code).to(torch.uint8)


def quant_rows_independent(x):
    """quant_rows with e4m3_rne_bytes in place of torch's cast: the same three fp32 operations per element (one correctly rounded
    division for the scale, one reciprocal, one product), then the encoder above."""
    x = x.float()
    amax = x.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    return e4m3_rne_bytes(x * (1.0 / s)[:, None]), s


def quant_rows_by_division(x):
    """The quantiser as ops.quant_rows_fp8's docstring once stated it, bytes = e4m3(x / s): an emulated fault for the CPU tests"""
    x = x.float()
    amax = x.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    return e4m3_rne_bytes(x / s[:, None]), s


def real_rows(rows, K, seed=1, mul=1.5):
    """The fp16 input rows of the real-valued tests (the GPU suite's activations)"""
    return (torch.randn(rows, K, generator=torch.Generator().manual_seed(seed)) * mul).half()


def real_weights(N, K, seed=2):
    """The fp32 weight rows of the real-valued tests"""
    return torch.randn(N, K, generator=torch.Generator().manual_seed(seed)) / math.sqrt(K)


# shapes (M, N, K) of the real-valued GEMM tests: ragged M / N tiles, N % 128 == 4, one and many K-tiles; then q|k at level 0 on a ragged
# row count, and (swapped) the V^T call M = C = 320, N = rows = 260
REAL_SHAPES = [(300, 640, 320), (1000, 132, 640), (132, 1280, 1280), (64, 64, 64), (257, 640, 320), (260, 320, 320)]

# worst-row error of a plain fp32 restatement of ew_gemm_fp8's scaled sum against fp64, no fp16 rounding (asserted on the CPU in
# tests/test_cpu_fp8_qkv.py; measured 6.9e-8 ... 7.6e-8 at REAL_SHAPES): what the GPU test's per-row bound adds to the fp16 rounding's 2^-11
FP32_ACC_ERR = 1e-6


def fp16_convert_table():
    """fp16 [rows, 2048]: column 0 of each row holds 448 (so the row's scale is exactly 1), the rest every finite fp16 value in
    [-448, 448], -0.0 included (48 642 of them), padded with zeros"""
    bits = torch.arange(0, 0x5F00 + 1, dtype=torch.int32)                     # 0x5F00 = 448.0
    vals = torch.cat([bits, bits | 0x8000]).to(torch.int16).view(torch.float16)
    assert vals.numel() == 48642
    per = 2047
    rows = -(-vals.numel() // per)
    t = torch.zeros(rows, 2048, dtype=torch.float16)
    t[:, 0] = 448.0
    flat = torch.zeros(rows * per, dtype=torch.float16)
    flat[: vals.numel()] = vals
    t[:, 1:] = flat.view(rows, per)
    return t


def positive_fp16():
    """every positive finite fp16 value (31 743 of them), as fp16"""
    return torch.arange(1, 0x7C00, dtype=torch.int16).view(torch.float16)


def amax_sweep_rows():
    """fp16 [31743, 8]: row i = [amax, -amax, amax / 2, 0, ...] for the i-th positive finite fp16 amax"""
    a = positive_fp16()
    t = torch.zeros(a.numel(), 8, dtype=torch.float16)
    t[:, 0], t[:, 1], t[:, 2] = a, -a, (a.float() / 2).half()
    return t


def assert_bits(got, want, what):
    """THE bit comparison of the fp8 tests (device results in tests/test_gpu_fp8_qkv.py, emulated faults in
    tests/test_cpu_fp8_qkv.py): same shape and dtype, every element equal as an integer; names the first few that differ."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    itype = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[got.dtype.itemsize]
    diff = got.contiguous().view(itype) != want.contiguous().view(itype)
    if bool(diff.any()):
        idx = [tuple(int(v) for v in i) for i in diff.nonzero()[:8]]
        shown = ", ".join(f"{i}: got {got[i].item()!r} want {want[i].item()!r}" for i in idx)
        raise AssertionError(f"{what}: {int(diff.sum())} of {diff.numel()} elements differ in their bits; {shown}")


# ------------------------------------------------------------------------------------------------ the GEMM on small integers
INT_SHAPES = [(1, 4, 64), (127, 132, 64), (129, 124, 128), (257, 640, 320), (320, 260, 320), (130, 8, 2048)]
INT_VARIANTS = ("signed", "positive", "mixed")


def _codes(v):
    """e4m3 codes of a tensor of exactly representable values"""
    q = e4m3_rne_bytes(v.float())
    assert torch.equal(q.view(torch.float8_e4m3fn).float(), v.float())
    return q


def int_gemm_case(M, N, K, variant="signed"):
    """Operands on which ew_gemm_fp8's fp32 sums are exact in any order: A bytes = codes of random integers in [-8, 8], W bytes of
    integers in [-6, 6], |sum| <= 48 K < 2^24.  Variants:
      signed    scales are powers of two, varying per row and per column;
      positive  A in [6, 8], W in [5, 6] (sums >= 30 K >= 1920, mean 38.5 K: more than fp16's 11 significant bits, so the fp16 rounding
                of the output, ties included, decides bits), the same scales;
      mixed     the positive operands; scales = power of two x a random fp32 in [1, 2) (24 significant bits), so each of the three fp32
                products of the epilogue rounds, and a_scale carries a further 2^-124, w_scale 2^124: ((acc * sa) * sw) * c_acc stays
                normal at every step (acc >= 1920), while acc * sw or (acc * c_acc) * sw overflows fp32 for every element.  This pins
                the ORDER of the epilogue, not only its product: with power-of-two scales every order rounds alike.
    The scales keep 48 K * sa * sw (and c_acc <= 1) inside fp16's finite range and every non-zero output above 2^-10.
    Returns dict(aq, wq uint8; sa, sw fp32; acc fp64 [M, N] = the exact integer sums)."""
    assert variant in INT_VARIANTS and 48 * K < 1 << 24
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + INT_VARIANTS.index(variant))
    if variant != "signed":
        a = torch.randint(6, 9, (M, K), generator=g)
        w = torch.randint(5, 7, (N, K), generator=g)
    else:
        a = torch.randint(-8, 9, (M, K), generator=g)
        w = torch.randint(-6, 7, (N, K), generator=g)
    top = 0
    while 48 * K * 2.0 ** (top + 1) <= 65504:
        top += 1
    while 48 * K * 2.0 ** top > 65504:
        top -= 1
    if variant == "mixed":
        top -= 2                                                               # each scale < 2 x its power of two
    sa = torch.ldexp(torch.ones(M), top - torch.randint(0, 3, (M,), generator=g))
    sw = torch.ldexp(torch.ones(N), -torch.randint(0, 4, (N,), generator=g))
    if variant == "mixed":
        sa = torch.ldexp(sa * (1 + torch.rand(M, generator=g)), torch.tensor(-124))
        sw = torch.ldexp(sw * (1 + torch.rand(N, generator=g)), torch.tensor(124))
    acc = a.double() @ w.double().T
    assert float(acc.abs().max()) <= 48 * K
    return dict(aq=_codes(a), wq=_codes(w), sa=sa.float(), sw=sw.float(), acc=acc, M=M, N=N, K=K)


def int_gemm_expect(acc, sa, sw, c_acc):
    """fp16(((acc * sa) * sw) * c_acc), each product one fp32 rounding, c_acc rounded to fp32 first as the C ABI's float is"""
    acc = acc.float()
    assert torch.equal(acc.double(), acc.double().round())
    y = ((acc * sa.float()[:, None]) * sw.float()[None, :]) * torch.tensor(c_acc, dtype=torch.float32)
    assert float(y.abs().max()) <= 65504
    return y.half()


def int_gemm_acc(aq, wq):
    """the exact sums of a pair of byte operands, fp64"""
    return aq.view(torch.float8_e4m3fn).double() @ wq.view(torch.float8_e4m3fn).double().T


def fake_quant(x):
    """Row-wise (last dim) e4m3 fake quantisation of a tensor of any rank, fp32 out"""
    flat = x.reshape(-1, x.shape[-1])
    return deq(*quant_rows(flat)).reshape(x.shape)


def self_attention_modules(ref):
    """(name, module) of every self-attention Attention of the oracle U-Net (attn1: keys and values come from the tokens themselves)"""
    from oracle.unet_ref import Attention
    return [(n, m) for n, m in ref.named_modules()
            if isinstance(m, Attention) and n.endswith(".attn1") and m.to_k.in_features == m.to_q.in_features]


def fake_quant_unet(ref):
    """Register the fake-quantisation hooks on `ref` (an oracle.unet_ref.UNetSpatioTemporalConditionModelRef).  Returns
    (handles, names): remove the handles to get the plain oracle back; names lists the hooked Attention modules."""
    handles, names = [], []

    def pre(mod, args):                  # input rows and weight rows -> their e4m3 fake-quantised values for this call
        mod._fp8_plain_weight = mod.weight.data
        mod.weight.data = mod._fp8_weight
        return (fake_quant(args[0]),) + tuple(args[1:])

    def post(mod, args, out):
        mod.weight.data = mod._fp8_plain_weight
        del mod._fp8_plain_weight

    for name, attn in self_attention_modules(ref):
        if attn.to_q.in_features % 64:
            continue
        names.append(name)
        for lin in (attn.to_q, attn.to_k, attn.to_v):
            lin._fp8_weight = fake_quant(lin.weight.data)
            handles.append(lin.register_forward_pre_hook(pre))
            handles.append(lin.register_forward_hook(post))
    return handles, names
