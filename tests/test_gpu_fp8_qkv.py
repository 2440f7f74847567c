"""-m gpu: the opt-in fp8 (OCP e4m3) q / k / v projection path of BASELINE.json configs[4] (ew_quant_rows_fp8, ew_gemm_fp8,
UNetSpatioTemporalConditionModel(qkv_fp8=True)) against the CPU references of tests/fp8_ref.py.

The two kernels are held to bits (tests/test_cpu_fp8_qkv.py shows on the CPU that these comparisons, on these inputs, reject a dropped
K-tile, a duplicated row, a reordered epilogue and a quantiser that divides by its scale):
  * quantiser: scale == fl(amax / 448) and bytes == e4m3_rne(fl(x * fl(1 / scale))) of an encoder that shares no code with torch's cast
    -- on every finite fp16 value in [-448, 448] at scale 1 (all ties, the e4m3 denormals, underflow, -0.0), on every positive finite
    fp16 row maximum (the row's largest element reaches the convert at up to 448.00003 and must come out 0x7E, not the NaN code), on
    the random rows of the GEMM cases and at every row / vector count at which the kernel takes another path; outputs guarded and twice
    prefilled, each row alone == the row in its batch.  (rel-L2(dequantised rows, x) <= 1.02 x the CPU reference's stays asserted.)
  * GEMM on small integers (fp8_ref.int_gemm_case: the fp32 sums are exact in any order): == fp16(((acc * sa) * sw) * c_acc) at six
    shapes with every ragged-tile form, three c_acc, two output strides; A, W and both scale vectors inside poisoned halos; each
    128-row tile alone == the same rows in the batched call; every refusal leaves its guarded output untouched.
  * GEMM on real-valued operands, per row (kernel_checks.report, `KCHECK` lines) against the fp64 product of the same dequantised
    bytes: the fp16 rounding of the output costs at most 2^-11 = 4.88e-4 per element, hence per row; the fp32 accumulation adds less
    than fp8_ref.FP32_ACC_ERR = 1e-6 (a plain fp32 restatement of the sum against fp64 measures 6.9e-8 ... 7.6e-8 per row on the CPU,
    test_cpu_fp8_qkv.py).  WORST_ROW holds min(that sum, 2 x the worst row measured on an MI355X).  The whole-tensor rel-L2 <= 5e-4
    of the earlier form of this file stays.
  * tiny U-Net forward: rel-L2(GPU fp8 forward, plain fp32 oracle) <= 1.5 x E_ref, E_ref = rel-L2(fake-quantised fp32 oracle, plain fp32
    oracle) computed here on the CPU -- the factor covers the fp16 path's own <= 1e-3 added in quadrature and roundings that flip near
    e4m3 boundaries (the product quantises fp16 LayerNorm outputs, the oracle fp32 ones).
    E_ref on the CPU: seed 0: 6.31e-3, seed 1: 7.00e-3, seed 2: 6.74e-3 (the rounds 2-4 device figure was 6.4e-3); the test prints both sides."""
import ctypes
import functools

import pytest
import torch

import fp8_ref
from conftest import rel_l2
from kernel_checks import Guarded, report, two_prefills

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8, F16, F32 = torch.uint8, torch.float16, torch.float32
SHAPES = fp8_ref.REAL_SHAPES[:4]                                                  # ragged M / N tiles, N % 128 == 4, one and many K-tiles
RAGGED = SHAPES[:3]
ROW_SHAPES = fp8_ref.REAL_SHAPES
ROW_ANALYTIC = 2.0 ** -11 + fp8_ref.FP32_ACC_ERR

# worst-row bounds per case: (bound, value measured on an MI355X, its row); bound = min(ROW_ANALYTIC, 2 x the measurement)
WORST_ROW = {
    'gemm_fp8 300x640x320 plain': (0.000455, 2.278e-04, 120),  # rel-L2 2.080e-04
    'gemm_fp8 300x640x320 c_acc': (0.000451, 2.257e-04, 15),  # rel-L2 2.078e-04
    'gemm_fp8 300x640x320 swapped': (ROW_ANALYTIC, 2.459e-04, 494),  # rel-L2 2.080e-04
    'gemm_fp8 1000x132x640 plain': (ROW_ANALYTIC, 2.713e-04, 264),  # rel-L2 2.074e-04
    'gemm_fp8 1000x132x640 c_acc': (ROW_ANALYTIC, 2.561e-04, 455),  # rel-L2 2.078e-04
    'gemm_fp8 1000x132x640 swapped': (0.000445, 2.227e-04, 33),  # rel-L2 2.074e-04
    'gemm_fp8 132x1280x1280 plain': (0.000440, 2.203e-04, 111),  # rel-L2 2.074e-04
    'gemm_fp8 132x1280x1280 c_acc': (0.000440, 2.200e-04, 68),  # rel-L2 2.078e-04
    'gemm_fp8 132x1280x1280 swapped': (ROW_ANALYTIC, 2.611e-04, 117),  # rel-L2 2.074e-04
    'gemm_fp8 64x64x64 plain': (ROW_ANALYTIC, 2.584e-04, 21),  # rel-L2 2.072e-04
    'gemm_fp8 64x64x64 c_acc': (ROW_ANALYTIC, 2.499e-04, 3),  # rel-L2 2.062e-04
    'gemm_fp8 64x64x64 swapped': (ROW_ANALYTIC, 2.607e-04, 47),  # rel-L2 2.072e-04
    'gemm_fp8 257x640x320 plain': (0.000455, 2.278e-04, 120),  # rel-L2 2.079e-04
    'gemm_fp8 257x640x320 c_acc': (0.000451, 2.257e-04, 15),  # rel-L2 2.080e-04
    'gemm_fp8 260x320x320 plain': (0.000467, 2.335e-04, 198),  # rel-L2 2.082e-04
    'gemm_fp8 260x320x320 c_acc': (0.000478, 2.391e-04, 122),  # rel-L2 2.075e-04
    'gemm_fp8 260x320x320 swapped': (0.000484, 2.424e-04, 49),  # rel-L2 2.082e-04
}


def _g(s):
    return torch.Generator().manual_seed(s)


def _p(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


def _call(name, *args):
    from evoworld_amd import _lib, ops
    _lib.check(getattr(_lib.load(), name)(*args, ops._stream()), name)


def _refused(name, *args):
    from evoworld_amd import _lib
    with pytest.raises(_lib.EvoWorldHipError):
        _call(name, *args)
    torch.cuda.synchronize()


def _spec(rows, width, dtype, ld=None):
    """a Guarded spec whose guard past the last row holds at least 16 Ki elements"""
    ld = width if ld is None else ld
    return rows, width, dtype, dict(ld=ld, pad_rows=max(2, -(-16384 // ld)))


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Inputs and CPU references of one real-valued GEMM shape, computed once and shared (read-only) by the tests below."""
    x = fp8_ref.real_rows(M, K)
    w = fp8_ref.real_weights(N, K)
    xq, xs = fp8_ref.quant_rows(x)
    wq, ws = fp8_ref.quant_rows(w)
    exact = fp8_ref.deq(xq, xs) @ fp8_ref.deq(wq, ws).T
    exact64 = fp8_ref.deq(xq, xs).double() @ fp8_ref.deq(wq, ws).double().T
    return dict(x=x, xq=xq, xs=xs, wq=wq, ws=ws, exact=exact, exact64=exact64)


def _dev(c, *names):
    return [c[n].to(DEV).contiguous() for n in names]


# ------------------------------------------------------------------------------------------------ the quantiser, to the bit
def _quant_abi(x):
    """ew_quant_rows_fp8 through the C ABI on x (fp16, CPU) into guarded, twice-prefilled q / scale; returns them on the CPU"""
    rows, K = x.shape
    d_x = x.to(DEV).contiguous()
    gq, gs = two_prefills(lambda q, s, k: _call("ew_quant_rows_fp8", _p(d_x), _p(q), _p(s), rows, K), _spec(rows, K, U8), _spec(1, rows, F32))
    return gq.view.cpu(), gs.view.cpu().reshape(rows)


def _check_quant(what, x, q, s):
    """device bytes and scales against the independent reference; every differing (input, device byte, reference byte) is printed first"""
    rq, rs = fp8_ref.quant_rows_independent(x)
    q, s = q.cpu(), s.cpu()
    bad = (q != rq).nonzero().tolist()
    for r, c in bad[:48]:
        print(f"QUANT MISMATCH {what}: row {r} col {c}: x {float(x[r, c])!r} (fp16 0x{int(x[r, c].view(torch.int16)) & 0xFFFF:04X}) "
              f"scale {float(s[r])!r} reference scale {float(rs[r])!r}: device byte 0x{int(q[r, c]):02X}, reference 0x{int(rq[r, c]):02X}")
    print(f"quant_rows_fp8 {what}: {len(bad)} of {q.numel()} bytes and {int((s.view(torch.int32) != rs.view(torch.int32)).sum())} of {s.numel()} "
          f"scales differ from the independent reference's")
    fp8_ref.assert_bits(s, rs, f"{what}: scales")
    fp8_ref.assert_bits(q, rq, f"{what}: bytes")
    return rq, rs


def test_quant_convert_table_every_fp16_value_at_scale_one():
    """Every finite fp16 value in [-448, 448] (48 642: all e4m3 ties, the denormal range, underflow to zero, -0.0) in rows whose
    maximum is 448, i.e. scale exactly 1: the bytes are those of the CPU encoder -- what v_cvt_pk_fp8_f32 does over its whole range"""
    x = fp8_ref.fp16_convert_table()
    q, s = _quant_abi(x)
    _check_quant("convert table", x, q, s)
    assert torch.equal(s, torch.ones(x.shape[0]))
    fp8_ref.assert_bits(q, fp8_ref.e4m3_rne_bytes(x.float()), "convert table vs the encoder at scale 1")
    assert not bool(((q & 0x7F) == 0x7F).any())


def test_quant_row_maximum_sweep():
    """One row [amax, -amax, amax / 2, 0 ...] per positive finite fp16 amax (31 743): scale bits == fl(amax / 448); the extremes reach
    the (unclamped) convert at 447.99997 ... 448.00003 and encode to 0x7E / 0xFE, never the NaN code"""
    x = fp8_ref.amax_sweep_rows()
    q, s = _quant_abi(x)
    nan = ((q & 0x7F) == 0x7F).nonzero().tolist()
    for r, c in nan[:16]:
        print(f"QUANT NaN byte: amax {float(x[r, 0])!r} (fp16 0x{int(x[r, 0].view(torch.int16)) & 0xFFFF:04X}) col {c}: 0x{int(q[r, c]):02X}")
    print(f"row-maximum sweep: {len(nan)} NaN bytes")
    assert torch.equal(s, fp8_ref.positive_fp16().float() / 448.0)
    assert torch.equal(q[:, 0], torch.full((x.shape[0],), 0x7E, dtype=U8)) and torch.equal(q[:, 1], torch.full((x.shape[0],), 0xFE, dtype=U8))
    _check_quant("row-maximum sweep", x, q, s)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_quant_rows_fp8(M, N, K):
    from evoworld_amd import ops
    c = _case(M, N, K)
    x = c["x"]
    q, s = ops.quant_rows_fp8(x.to(DEV))
    assert q.dtype == torch.uint8 and tuple(q.shape) == (M, K) and s.dtype == torch.float32 and tuple(s.shape) == (M,)
    q, s = q.cpu(), s.cpu()
    assert torch.equal(s, x.float().abs().amax(1) / 448.0)
    e_ref = rel_l2(fp8_ref.deq(c["xq"], c["xs"]), x.float())
    e_gpu = rel_l2(fp8_ref.deq(q, s), x.float())
    differ = int((q != c["xq"]).sum())
    print(f"quant_rows_fp8 {M}x{K}: rel-L2 to x: device {e_gpu:.4e}, CPU reference {e_ref:.4e}; {differ} of {q.numel()} bytes differ from the reference's")
    assert torch.isfinite(fp8_ref.deq(q, s)).all()
    assert e_gpu <= 1.02 * e_ref
    _check_quant(f"{M}x{K}", x, q, s)
    assert differ == 0 and torch.equal(s, c["xs"])


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
        assert torch.equal(s, rs)
        assert rel_l2(fp8_ref.deq(q, s), x.float()) <= 1.02 * rel_l2(fp8_ref.deq(rq, rs), x.float())
        _check_quant(f"zero row, K={K}", x, q, s)
        assert int((q != rq).sum()) == 0


@pytest.mark.parametrize("K", [8, 512, 520, 1288, 2048])
def test_quant_geometry_guarded_and_row_alone(K):
    """rows in {1, 4, 5, 9} (a workgroup holds 4 rows) x K = one lane / exactly 64 vectors / 64 + 1 / three per lane / four: bytes and
    scales exact, guards intact under both prefills, and each row quantised alone (pointer offsets into one guarded buffer) == the
    same row quantised with its batch"""
    for rows in (1, 4, 5, 9):
        x = fp8_ref.real_rows(rows, K, seed=10 * rows + K, mul=0.7)
        if rows >= 5:
            x[3] = 0
        q, s = _quant_abi(x)
        _check_quant(f"{rows}x{K}", x, q, s)
        d_x = x.to(DEV)
        gq = Guarded(rows, K, U8, prefill=1, device=DEV, **_spec(rows, K, U8)[3])
        gs = Guarded(1, rows, F32, prefill=1, device=DEV, **_spec(1, rows, F32)[3])
        for r in range(rows):
            _call("ew_quant_rows_fp8", _p(d_x, r * K * 2), _p(gq.buf, r * K), _p(gs.buf, r * 4), 1, K)
        torch.cuda.synchronize()
        gq.check()
        gs.check()
        fp8_ref.assert_bits(gq.view, q, f"{rows}x{K}: rows alone vs batched, bytes")
        fp8_ref.assert_bits(gs.view.reshape(rows), s, f"{rows}x{K}: rows alone vs batched, scales")


def test_quant_refusals_leave_the_outputs_untouched():
    x = torch.ones(4, 2056, dtype=F16, device=DEV)
    gq = Guarded(4, 2056, U8, ld=2056, pad_rows=4, device=DEV)
    gs = Guarded(1, 4, F32, ld=4, pad_rows=64, device=DEV)
    a = (_p(x), _p(gq.buf), _p(gs.buf))
    _refused("ew_quant_rows_fp8", *a, 4, 12)                  # K % 8 != 0
    _refused("ew_quant_rows_fp8", *a, 4, 2056)                # K > 2048
    _refused("ew_quant_rows_fp8", *a, 0, 64)                  # rows = 0
    _refused("ew_quant_rows_fp8", *a, 4, 0)                   # K = 0
    _refused("ew_quant_rows_fp8", None, a[1], a[2], 4, 64)
    _refused("ew_quant_rows_fp8", a[0], None, a[2], 4, 64)
    _refused("ew_quant_rows_fp8", a[0], a[1], None, 4, 64)
    for g in (gq, gs):
        g.check()
        assert bool((g.view.view(g.itype) == g.pattern).all())


# ------------------------------------------------------------------------------------------------ the GEMM on small integers, to the bit
@functools.lru_cache(maxsize=None)
def _int_case(M, N, K, variant):
    c = fp8_ref.int_gemm_case(M, N, K, variant)
    c["dev"] = tuple(c[n].to(DEV).contiguous() for n in ("aq", "sa", "wq", "sw"))
    return c


def _c_accs():
    from evoworld_amd import ops
    return (1.0, 0.25, ops.QK_LOG2_PRESCALE)


def _gemm_abi(aq, sa, wq, sw, M, N, K, c_acc, ld_pad):
    """ew_gemm_fp8 through the C ABI into a guarded, twice-prefilled output of row stride N + ld_pad; returns the [M, N] view"""
    run = lambda o, k: _call("ew_gemm_fp8", _p(aq), _p(sa), _p(wq), _p(sw), _p(o), M, N, K, N + ld_pad, c_acc)      # noqa: E731
    return two_prefills(run, _spec(M, N, F16, N + ld_pad))[0].view


@pytest.mark.parametrize("variant", fp8_ref.INT_VARIANTS)
@pytest.mark.parametrize("M,N,K", fp8_ref.INT_SHAPES)
def test_gemm_fp8_integers_exact(M, N, K, variant):
    """== fp16(((acc * sa) * sw) * c_acc) bit for bit: M = 1 / N = 4, ragged M and N tiles either side of 128, N % 128 == 4, q|k at level
    0 (five K-tiles), the swapped V^T form, 32 K-tiles; c_acc 1, 1/4 and QK_LOG2_PRESCALE; ld_out = N + 4 and N + 64"""
    c = _int_case(M, N, K, variant)
    for c_acc in _c_accs():
        want = fp8_ref.int_gemm_expect(c["acc"], c["sa"], c["sw"], c_acc)
        for ld_pad in (4, 64):
            got = _gemm_abi(*c["dev"], M, N, K, c_acc, ld_pad)
            fp8_ref.assert_bits(got, want, f"gemm_fp8 {variant} {M}x{N}x{K} c_acc={c_acc:.4g} ld_out=N+{ld_pad}")


def _haloed(data, before, after, fill):
    """`data` (device, [rows, ...]) inside one larger allocation whose `before` / `after` rows around it hold `fill`; returns the
    inner view (the allocation stays alive through it)"""
    rows = data.shape[0]
    buf = torch.empty((before + rows + after,) + tuple(data.shape[1:]), dtype=data.dtype, device=data.device)
    buf.fill_(fill)
    inner = buf[before: before + rows]
    inner.copy_(data)
    return inner


@pytest.mark.parametrize("variant", ["signed", "mixed"])
@pytest.mark.parametrize("M,N,K", fp8_ref.INT_SHAPES)
def test_gemm_fp8_integers_poisoned_halos(M, N, K, variant):
    """A, W, a_scale and w_scale each inside a larger allocation whose surround (4 rows / values before, 132 after: more than a
    tile's worth of the rows the kernel clamps with min(.., M - 1)) holds 0x7F bytes (the e4m3 NaN) and NaN scales in one run, 0x7E
    (448) bytes and inf scales in the other: a row or scale read past either edge poisons the sums.  Bit-identical to the plain call."""
    from evoworld_amd import ops
    c = _int_case(M, N, K, variant)
    aq, sa, wq, sw = c["dev"]
    c_acc = ops.QK_LOG2_PRESCALE
    want = fp8_ref.int_gemm_expect(c["acc"], c["sa"], c["sw"], c_acc)
    plain = _gemm_abi(aq, sa, wq, sw, M, N, K, c_acc, 4)
    fp8_ref.assert_bits(plain, want, "plain call")
    for byte, scale in ((0x7F, float("nan")), (0x7E, float("inf"))):
        h = (_haloed(aq, 4, 132, byte), _haloed(sa, 4, 132, scale), _haloed(wq, 4, 132, byte), _haloed(sw, 4, 132, scale))
        got = _gemm_abi(*h, M, N, K, c_acc, 4)
        fp8_ref.assert_bits(got, plain, f"gemm_fp8 {variant} {M}x{N}x{K} under 0x{byte:02X} / {scale} halos vs the plain call")


@pytest.mark.parametrize("M,N,K", [(257, 640, 320), (320, 260, 320)])
def test_gemm_fp8_integers_tile_alone_vs_batched(M, N, K):
    """Each 128-row tile, and the ragged last rows, run alone through pointer offsets into a second guarded buffer == the batched call"""
    from evoworld_amd import ops
    for variant in ("signed", "mixed"):
        c = _int_case(M, N, K, variant)
        aq, sa, wq, sw = c["dev"]
        c_acc, ld = ops.QK_LOG2_PRESCALE, N + 4
        batched = _gemm_abi(aq, sa, wq, sw, M, N, K, c_acc, 4)
        fp8_ref.assert_bits(batched, fp8_ref.int_gemm_expect(c["acc"], c["sa"], c["sw"], c_acc), "batched call")
        rows, width, dtype, kw = _spec(M, N, F16, ld)
        g = Guarded(rows, width, dtype, prefill=1, device=DEV, **kw)
        for r0 in range(0, M, 128):
            m = min(128, M - r0)
            _call("ew_gemm_fp8", _p(aq, r0 * K), _p(sa, r0 * 4), _p(wq), _p(sw), _p(g.buf, r0 * ld * 2), m, N, K, ld, c_acc)
        torch.cuda.synchronize()
        g.check()
        fp8_ref.assert_bits(g.view, batched, f"gemm_fp8 {variant} {M}x{N}x{K}: row tiles alone vs batched")


def test_gemm_fp8_refusals_leave_the_output_untouched():
    M, N, K = 8, 8, 128
    aq = torch.zeros(M + 1, K, dtype=U8, device=DEV)
    wq = torch.zeros(N + 1, K, dtype=U8, device=DEV)
    sa, sw = torch.ones(M + 4, device=DEV), torch.ones(N + 4, device=DEV)
    g = Guarded(M, N, F16, ld=N + 4, pad_rows=64, device=DEV)
    a, s_a, w, s_w, o = _p(aq), _p(sa), _p(wq), _p(sw), _p(g.buf)
    ld = N + 4
    _call("ew_gemm_fp8", a, s_a, w, s_w, _p(torch.empty(M, ld, dtype=F16, device=DEV)), M, N, K, ld, 1.0)      # the argument set itself is legal
    _refused("ew_gemm_fp8", _p(aq, 8), s_a, w, s_w, o, M, N, K, ld, 1.0)          # a not 16-byte aligned
    _refused("ew_gemm_fp8", a, s_a, _p(wq, 8), s_w, o, M, N, K, ld, 1.0)          # w not 16-byte aligned
    _refused("ew_gemm_fp8", a, s_a, w, _p(sw, 4), o, M, N, K, ld, 1.0)            # w_scale not 16-byte aligned
    _refused("ew_gemm_fp8", a, s_a, w, s_w, _p(g.buf, 4), M, N, K, ld, 1.0)       # out not 8-byte aligned
    _refused("ew_gemm_fp8", a, s_a, w, s_w, o, M, N, K, N - 4, 1.0)               # ld_out < N
    _refused("ew_gemm_fp8", a, s_a, w, s_w, o, M, N, K, N + 2, 1.0)               # ld_out % 4 != 0
    _refused("ew_gemm_fp8", a, s_a, w, s_w, o, 0, N, K, ld, 1.0)                  # M = 0
    _refused("ew_gemm_fp8", a, s_a, w, s_w, o, M, 0, K, ld, 1.0)                  # N = 0
    _refused("ew_gemm_fp8", a, s_a, w, s_w, o, M, 6, K, ld, 1.0)                  # N % 4 != 0
    _refused("ew_gemm_fp8", a, s_a, w, s_w, o, M, N, 96, ld, 1.0)                 # K % 64 != 0
    _refused("ew_gemm_fp8", a, s_a, w, s_w, o, M, N, 0, ld, 1.0)                  # K = 0
    for i in range(5):                                                             # a NULL pointer, each of the five
        ptrs = [a, s_a, w, s_w, o]
        ptrs[i] = None
        _refused("ew_gemm_fp8", *ptrs, M, N, K, ld, 1.0)
    g.check()
    assert bool((g.view.view(g.itype) == g.pattern).all())


# ------------------------------------------------------------------------------------------------ the GEMM on real-valued operands
def _row_check(key, got, ref):
    """kernel_checks.report under the table's bound, and the whole-tensor rel-L2 < 5e-4"""
    bound = WORST_ROW[key][0]
    assert bound <= ROW_ANALYTIC
    return report(key, got, ref, bound, 5e-4)


@pytest.mark.parametrize("M,N,K", ROW_SHAPES)
def test_gemm_fp8_per_row(M, N, K):
    """Worst row against the fp64 product of the same dequantised bytes: plain, swapped (the transposed product, where the new N = M
    is a multiple of 4) and with c_acc = QK_LOG2_PRESCALE.  Bounds: the module docstring and WORST_ROW."""
    from evoworld_amd import ops
    c = _case(M, N, K)
    xq, xs, wq, ws = _dev(c, "xq", "xs", "wq", "ws")
    exact = c["exact64"]
    cc = float(torch.tensor(ops.QK_LOG2_PRESCALE, dtype=F32))
    failed = []
    runs = [("plain", lambda: _gemm_abi(xq, xs, wq, ws, M, N, K, 1.0, 4), exact),
            ("c_acc", lambda: _gemm_abi(xq, xs, wq, ws, M, N, K, ops.QK_LOG2_PRESCALE, 4), exact * cc)]
    if M % 4 == 0:
        runs.append(("swapped", lambda: _gemm_abi(wq, ws, xq, xs, N, M, K, 1.0, 4), exact.T.contiguous()))
    for form, run, ref in runs:                                 # every figure is printed before the test fails
        try:
            _row_check(f"gemm_fp8 {M}x{N}x{K} {form}", run().cpu(), ref)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


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
