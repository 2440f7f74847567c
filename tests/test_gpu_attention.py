"""-m gpu: the attention cores (attn_spatial_kernel<false/true>, attn_temporal_kernel, attn_temporal64_kernel, attn_temporal_long_kernel,
attn_small_kernel) through ops.attn_* (the C ABI), held to more than a tolerance:

1. one-hot attention is a bit-exact gather (attn_cases.onehot_*): a wrong key order, mask or problem decode is named by key;
2. operand halos (kernel_checks.same_under_halos): what lies past S / T / the row width never reaches a result -- NaN, inf, the largest
   finite value and zero around q, k and v / V^T give bit-identical outputs;
3. every (sequence, head) / (b, pixel, head) problem of a batched call equals the same problem run alone through pointer offsets;
4. the adversarial score profiles on the paths that did not see them (the scale-and-shift form; the T <= 32 and T <= 64 temporal kernels),
   per row against fp64 SDPA on the same fp16 inputs;
5. the entry points' refusals leave o untouched and name themselves in ew_last_error().
Strides are wider than the data and outputs are guarded and twice prefilled, as in test_gpu_ops.py.  The exact tests carry no tolerance."""
import pytest
import torch

import attn_cases as ac
from kernel_checks import Guarded, assert_same_bits, report, same_under_halos, two_prefills

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = ["scale", "log2"]
# worst-row bounds per case: (bound, value measured on an MI355X); the bound is at most 2x the measurement and none is above 1e-3.  The rows
# measured above 5e-4 are the algorithm's own error, not a defect: on ramp and the two shifts attn_cases.attn_tiled (the torch restatement: fp16 P
# rounded toward zero, rounded-sum normaliser) gives the same worst rows to three digits (tests/test_cpu_attn_cases.py prints them; the log2 form's
# cases in test_gpu_ops.py likewise).  overflow (exponents up to 3000: an fp32 score carries 2^-12 .. 2^-9 of rounding there) measures 5.3e-4
# where the restatement gives 4.9e-4 with one rounding per MFMA k-step and 1.2e-3 with a plain fp32 dot product: the MFMA lies between
WORST_ROW = {
    'attn_spatial max profile ramp': (0.001, 0.00052),  # measured worst row; rel-L2 0.000282 row 1379
    'attn_spatial max profile jumps': (0.00093, 0.00047),  # measured worst row; rel-L2 0.000275 row 1281
    'attn_spatial max profile overflow': (0.001, 0.000533),  # measured worst row; rel-L2 0.000286 row 1717
    'attn_spatial max profile flat_below': (0.00096, 0.000484),  # measured worst row; rel-L2 0.000289 row 206
    'attn_spatial max profile flat_above': (0.00094, 0.000472),  # measured worst row; rel-L2 0.000287 row 244
    'attn_spatial max profile late_spike': (0.00096, 0.000485),  # measured worst row; rel-L2 0.00027 row 1217
    'attn_spatial max profile ragged_spike': (0.0009, 0.000454),  # measured worst row; rel-L2 0.000248 row 1686
    'attn_spatial shift 2x512x2 0': (0.00079, 0.000396),  # measured worst row; rel-L2 0.000249 row 102
    'attn_spatial shift 1x1000x1 0': (0.00097, 0.000485),  # measured worst row; rel-L2 0.000249 row 20
    'attn_spatial shift 3x136x5 0': (0.00074, 0.000374),  # measured worst row; rel-L2 0.000284 row 63
    'attn_spatial shift 1x2304x1 -60': (0.001, 0.000509),  # measured worst row; rel-L2 0.000246 row 820
    'attn_spatial shift 1x640x2 40': (0.001, 0.000515),  # measured worst row; rel-L2 0.000239 row 48
    'attn_spatial shift 1x128x1 -60': (0.00083, 0.000418),  # measured worst row; rel-L2 0.000234 row 120
    'attn_spatial shift 2x72x2 40': (0.0008, 0.000401),  # measured worst row; rel-L2 0.000261 row 124
    'attn_temporal spike first T=25': (2.2e-07, 1.14e-07),  # measured worst row; rel-L2 9.44e-09 row 100
    'attn_temporal spike first T=49': (1.1e-07, 5.79e-08),  # measured worst row; rel-L2 4.02e-09 row 137
    'attn_temporal spike last T=25': (2.9e-09, 1.46e-09),  # measured worst row; rel-L2 1.51e-10 row 110
    'attn_temporal spike last T=49': (1.4e-07, 7.28e-08),  # measured worst row; rel-L2 4.98e-09 row 234
    'attn_temporal spike rising T=25': (0.0006, 0.000303),  # measured worst row; rel-L2 0.000209 row 87
    'attn_temporal spike rising T=49': (0.0007, 0.000354),  # measured worst row; rel-L2 0.000219 row 225
}


@pytest.fixture(scope="module")
def ops():
    from evoworld_amd import ops as o
    assert torch.cuda.is_available()
    assert o.QK_LOG2_PRESCALE == ac.QK_LOG2_PRESCALE
    return o


def _wr(case):
    bound = WORST_ROW[case][0]
    assert bound <= 1e-3, case
    return bound


def _spatial(ops, form, q, k, vt, o, n_seq, S, heads, ld_qk, ld_vt, ld_o):
    if form == "log2":
        return ops.attn_spatial_log2(q, k, vt, o, n_seq, S, heads, ld_qk, ld_vt, ld_o)
    return ops.attn_spatial(q, k, vt, o, n_seq, S, heads, ld_qk, ld_vt, ld_o, scale=0.125)


def _spatial_operands(qk, v, n_seq, S, heads):
    """fp16 CPU q|k [rows, 2C], v [rows, C] -> device q|k with ld_qk > 2C, V^T with ld_vt > rows (zero padding), and the strides"""
    C, rows = heads * 64, n_seq * S
    ld_qk, ld_vt, ld_o = 2 * C + 24, rows + 40, C + (8 if heads > 1 else 64)
    qkd = torch.zeros(rows, ld_qk, dtype=torch.float16, device=DEV)
    qkd[:, :2 * C] = qk.to(DEV)
    vt = torch.zeros(C, ld_vt, dtype=torch.float16, device=DEV)
    vt[:, :rows] = v.to(DEV).T
    return qkd, vt, ld_qk, ld_vt, ld_o


def _run_spatial(ops, form, qk, v, n_seq, S, heads):
    """-> guarded, twice-prefilled o view [rows, C] on the device"""
    C, rows = heads * 64, n_seq * S
    qkd, vt, ld_qk, ld_vt, ld_o = _spatial_operands(qk, v, n_seq, S, heads)
    return two_prefills(lambda o, _: _spatial(ops, form, qkd, qkd[:, C:], vt, o, n_seq, S, heads, ld_qk, ld_vt, ld_o),
                        (rows, C, torch.float16, dict(ld=ld_o, pad_rows=64)))[0].view


def _temporal_operands(q, k, v):
    """fp16 CPU rows [B*T*S, C] each -> device q|k|v with ld > 3C"""
    rows, C = q.shape
    ld, ld_o = 3 * C + 16, C + (8 if C > 64 else 64)
    qkv = torch.zeros(rows, ld, dtype=torch.float16, device=DEV)
    for i, x in enumerate((q, k, v)):
        qkv[:, i * C:(i + 1) * C] = x.to(DEV)
    return qkv, ld, ld_o


def _run_temporal(ops, q, k, v, B, T, S, heads):
    C, rows = heads * 64, B * T * S
    qkv, ld, ld_o = _temporal_operands(q, k, v)
    return two_prefills(lambda o, _: ops.attn_temporal(qkv, qkv[:, C:], qkv[:, 2 * C:], o, B, T, S, heads, ld, ld_o),
                        (rows, C, torch.float16, dict(ld=ld_o, pad_rows=64)))[0].view


# ----------------------------------------------------------------------------- 1. one-hot attention is a bit-exact gather
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("perm", ac.PERMS)
@pytest.mark.parametrize("n_seq,S,heads", ac.ONEHOT_SPATIAL)
def test_onehot_spatial_is_a_gather(ops, n_seq, S, heads, perm, form):
    """S = 8: one ragged tile; 72 / 136 / 200: a ragged second / third / fourth tile, 136 and 200 with a second q-tile; 1000: eight q-tiles,
    sixteen key tiles, the last ragged.  The V^T tile order (write_tile slots A / B), mask_tail, the tok0 / pair / qtile decode and the
    XCD remap all move whole V rows: the message names the key that arrived"""
    case, _ = ac.onehot_spatial(n_seq, S, heads, perm, form)
    qk = torch.cat([ac.spatial_rows(case["q"], n_seq, S, heads), ac.spatial_rows(case["k"], n_seq, S, heads)], dim=1)
    o = _run_spatial(ops, form, qk, ac.spatial_rows(case["v"], n_seq, S, heads), n_seq, S, heads)
    ac.check_gather(ac.spatial_problems(o.cpu(), n_seq, S, heads), case, f"attn_spatial {form} {n_seq}x{S}x{heads} {perm}")


@pytest.mark.parametrize("perm", ac.PERMS)
@pytest.mark.parametrize("B,T,S,heads", ac.ONEHOT_TEMPORAL)
def test_onehot_temporal_is_a_gather(ops, B, T, S, heads, perm):
    """T <= 32, <= 64 and streaming, at and beside the block edges; the 16-bit LDS gathers of V^T, the key masks and the (b, pixel, head)
    decode move whole V rows; B * S * heads % 4 != 0 leaves an idle wave in the last block"""
    case, _ = ac.onehot_temporal(B, T, S, heads, perm)
    q, k, v = (ac.temporal_rows(case[n], B, T, S, heads) for n in "qkv")
    o = _run_temporal(ops, q, k, v, B, T, S, heads)
    ac.check_gather(ac.temporal_problems(o.cpu(), B, T, S, heads), case, f"attn_temporal {B}x{T}x{S}x{heads} {perm}")


@pytest.mark.parametrize("perm", ac.PERMS)
@pytest.mark.parametrize("n_seq,S,heads,D", ac.ONEHOT_SMALL)
def test_onehot_small_is_a_gather(ops, n_seq, S, heads, D, perm):
    case, _ = ac.onehot_small(n_seq, S, heads, D, perm)
    C, rows = heads * D, n_seq * S
    ld, ld_o = 3 * C + 8, C + 64
    qkv = torch.zeros(rows, ld, dtype=torch.float16, device=DEV)
    for i, n in enumerate("qkv"):
        qkv[:, i * C:(i + 1) * C] = ac.small_rows(case[n], n_seq, S, heads, D).to(DEV)
    o = two_prefills(lambda o, _: ops.attn_small(qkv, qkv[:, C:], qkv[:, 2 * C:], o, n_seq, S, heads, D, ld, ld_o, D ** -0.5),
                     (rows, C, torch.float16, dict(ld=ld_o, pad_rows=16)))[0].view
    ac.check_gather(ac.small_problems(o.cpu(), n_seq, S, heads, D), case, f"attn_small {n_seq}x{S}x{heads}x{D} {perm}")


# ----------------------------------------------------------------------------- 2. operand halos
def _out(rows, C, ld_o):
    return Guarded(rows, C, torch.float16, ld=ld_o, pad_rows=16, prefill=0, device=DEV)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("S", [136, 128])
def test_spatial_operand_halos(ops, S, form):
    """q|k rows before the first and after the last token, columns >= 2C; V^T columns >= n_seq * S and rows outside heads * 64: K rows are
    clamped to S-1, V^T columns >= S replaced by zero -- nothing of the surround may be weighted, not even by zero"""
    n_seq, heads = 2, 2
    C, rows = heads * 64, n_seq * S
    qk32, v = ac.spatial_random(n_seq, S, heads)
    qk = ac.to_form(qk32 * ac.QK_LOG2_PRESCALE, form)[0]
    ld_o = C + 8

    def run(qkh, vth):
        g = _out(rows, C, ld_o)
        _spatial(ops, form, qkh.view, qkh.view[:, C:], vth.view, g.view, n_seq, S, heads, qkh.ld, vth.ld, ld_o)
        torch.cuda.synchronize()
        g.check()
        return g.view.contiguous()

    qkd, vtd = qk.to(DEV), v.to(DEV).T.contiguous()
    plain = _out(rows, C, ld_o)
    _spatial(ops, form, qkd, qkd[:, C:], vtd, plain.view, n_seq, S, heads, 2 * C, rows, ld_o)
    same_under_halos(run, [(qkd, dict(ld=2 * C + 24)), (vtd, dict(ld=rows + 40))], plain=plain.view.contiguous())


@pytest.mark.parametrize("T", [25, 49, 97, 32, 64, 96])
def test_temporal_operand_halos(ops, T):
    """rows >= T of a problem are zero-filled in the kernels, never loaded: frames past the last (the rows after the operand), the rows before
    it and the columns >= 3C reach no result"""
    B, S, heads = 2, 3, 2
    C, rows = heads * 64, B * T * S
    qkv = torch.randn(rows, 3 * C, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    ld_o = C + 8

    def call(x, ld):
        g = _out(rows, C, ld_o)
        ops.attn_temporal(x, x[:, C:], x[:, 2 * C:], g.view, B, T, S, heads, ld, ld_o)
        torch.cuda.synchronize()
        g.check()
        return g.view.contiguous()

    same_under_halos(lambda h: call(h.view, h.ld), [(qkv, dict(ld=3 * C + 16))], plain=call(qkv, 3 * C))


def test_small_operand_halos(ops):
    n_seq, S, heads, D = 2, 17, 2, 80
    C, rows = heads * D, n_seq * S
    qkv = torch.randn(rows, 3 * C, generator=torch.Generator().manual_seed(2)).half().to(DEV)
    ld_o = C + 8

    def call(x, ld):
        g = _out(rows, C, ld_o)
        ops.attn_small(x, x[:, C:], x[:, 2 * C:], g.view, n_seq, S, heads, D, ld, ld_o, D ** -0.5)
        torch.cuda.synchronize()
        g.check()
        return g.view.contiguous()

    same_under_halos(lambda h: call(h.view, h.ld), [(qkv, dict(ld=3 * C + 8))], plain=call(qkv, 3 * C))


# ----------------------------------------------------------------------------- 3. alone equals batched
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_seq,S,heads", [(3, 136, 3), (2, 200, 2)])
def test_spatial_alone_equals_batched(ops, n_seq, S, heads, form):
    """every (sequence, head) of the batched call against the same problem as an n_seq = 1, heads = 1 call on pointers into the same
    buffers (same strides): the XCD remap and the pair / n_qtiles decode only choose WHERE a problem runs"""
    C, rows = heads * 64, n_seq * S
    qk32, v = ac.spatial_random(n_seq, S, heads)
    qkd, vt, ld_qk, ld_vt, ld_o = _spatial_operands(ac.to_form(qk32 * ac.QK_LOG2_PRESCALE, form)[0], v, n_seq, S, heads)
    both, alone = (Guarded(rows, C, torch.float16, ld=ld_o, pad_rows=16, prefill=0, device=DEV) for _ in range(2))
    _spatial(ops, form, qkd, qkd[:, C:], vt, both.view, n_seq, S, heads, ld_qk, ld_vt, ld_o)
    for seq in range(n_seq):
        for h in range(heads):
            r0, c0 = seq * S, h * 64
            _spatial(ops, form, qkd[r0:, c0:], qkd[r0:, C + c0:], vt[c0:, r0:], alone.view[r0:, c0:], 1, S, 1, ld_qk, ld_vt, ld_o)
    torch.cuda.synchronize()
    both.check()
    alone.check()
    for seq in range(n_seq):
        for h in range(heads):
            blk = (slice(seq * S, (seq + 1) * S), slice(h * 64, (h + 1) * 64))
            assert_same_bits(both.view[blk].contiguous(), alone.view[blk].contiguous(), f"(seq {seq}, head {h}) batched vs alone")


@pytest.mark.parametrize("B,T,S,heads", [(2, 25, 7, 2), (1, 49, 5, 3), (1, 97, 5, 2)])
def test_temporal_alone_equals_batched(ops, B, T, S, heads):
    """every (b, pixel, head) of the batched call against the same problem as a B = 1, S = 1, heads = 1 call with ld = S * ld and
    ld_o = S * ld_o on pointers into the same buffers"""
    C, rows = heads * 64, B * T * S
    x = torch.randn(rows, 3 * C, generator=torch.Generator().manual_seed(1)).half()
    qkv, ld, ld_o = _temporal_operands(x[:, :C], x[:, C:2 * C], x[:, 2 * C:])
    both, alone = (Guarded(rows, C, torch.float16, ld=ld_o, pad_rows=16, prefill=0, device=DEV) for _ in range(2))
    ops.attn_temporal(qkv, qkv[:, C:], qkv[:, 2 * C:], both.view, B, T, S, heads, ld, ld_o)
    for b in range(B):
        for s in range(S):
            for h in range(heads):
                r0, c0 = b * T * S + s, h * 64
                ops.attn_temporal(qkv[r0:, c0:], qkv[r0:, C + c0:], qkv[r0:, 2 * C + c0:], alone.view[r0:, c0:], 1, T, 1, 1, S * ld, S * ld_o)
    torch.cuda.synchronize()
    both.check()
    alone.check()
    got, ref = (ac.temporal_problems(g.view.contiguous(), B, T, S, heads) for g in (both, alone))
    for p, pid in enumerate(ac.temporal_ids(B, S, heads)):
        assert_same_bits(got[p].contiguous(), ref[p].contiguous(), f"(b, pixel, head) = {pid} batched vs alone")


# ----------------------------------------------------------------------------- 4. profiles on every path, per row
def _spatial_profile(ops, case, form, qk_l2, v, n_seq, S, heads):
    qk, _, c = ac.to_form(qk_l2, form)
    o = _run_spatial(ops, form, qk, v, n_seq, S, heads)
    C = heads * 64
    q, k, vv = (ac.spatial_problems(x.to(DEV), n_seq, S, heads) for x in (qk[:, :C], qk[:, C:], v))
    ref = ac.spatial_rows(ac.sdpa64(q, k, vv, c), n_seq, S, heads)
    assert torch.isfinite(o).all()
    report(case, o, ref, _wr(case), 2e-3)


@pytest.mark.parametrize("pattern", ac.LAZY_PATTERNS)
def test_attn_spatial_scale_form_max_profiles(ops, pattern):
    """the seven profiles of test_attn_spatial_log2_lazy_max on ew_attn_spatial_f16 (deferred max, threshold 2^6), the same exponents
    through its scale; flat_below / flat_above put the tile maxima 5.9 / 6.1 above the first tile's"""
    n_seq, S, heads, qk_l2, v = ac.lazy_max_case(pattern, "scale")
    _spatial_profile(ops, f"attn_spatial max profile {pattern}", "scale", qk_l2, v, n_seq, S, heads)


@pytest.mark.parametrize("n_seq,S,heads,shift", ac.SHIFT_CASES)
def test_attn_spatial_scale_form_shifts(ops, n_seq, S, heads, shift):
    _spatial_profile(ops, f"attn_spatial shift {n_seq}x{S}x{heads} {shift:g}", "scale", *ac.shift_case(n_seq, S, heads, shift), n_seq, S, heads)


@pytest.mark.parametrize("T", [25, 49])
@pytest.mark.parametrize("pattern", ["first", "last", "rising"])
def test_attn_temporal_spikes_below_65_frames(ops, pattern, T):
    """the forced-rescale inputs of test_attn_temporal_long_forced_rescale on attn_temporal_kernel (T = 25) and attn_temporal64_kernel
    (T = 49): one maximum over all keys there, ~40 logits above the rest"""
    q, k, v = ac.spike_case(pattern, T=T)
    B, _, S, heads, _ = q.shape
    rows, C = B * T * S, heads * 64
    o = _run_temporal(ops, *(x.reshape(rows, C) for x in (q, k, v)), B, T, S, heads)
    p = lambda x: ac.temporal_problems(x.reshape(rows, C).to(DEV), B, T, S, heads)
    ref = ac.temporal_rows(ac.sdpa64(p(q), p(k), p(v), 0.125 * ac.LOG2E), B, T, S, heads)
    assert torch.isfinite(o).all()
    case = f"attn_temporal spike {pattern} T={T}"
    report(case, o, ref, _wr(case), 2e-3)


# ----------------------------------------------------------------------------- 5. refusals
def _refused(call, name, rows=256):
    """call(o view) must raise, name the entry point in ew_last_error() and leave the guarded o as it was"""
    from evoworld_amd import _lib
    g = Guarded(rows, 128, torch.float16, ld=136, pad_rows=16, prefill=0, device=DEV)
    with pytest.raises(_lib.EvoWorldHipError):
        call(g.view)
    assert name in _lib.load().ew_last_error().decode(), (name, _lib.load().ew_last_error())
    torch.cuda.synchronize()
    assert bool((g.buf.view(torch.int16) == g.pattern).all()), f"{name}: o written by a refused call"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("what", ["S=12", "ld_qk=2C+4", "ld_vt=rows+4", "ld_o=C+2", "n_seq=0"])
def test_spatial_refusals(ops, what, form):
    n_seq, S, heads = 2, 16, 2
    C, rows = heads * 64, n_seq * S
    qk = torch.zeros(rows + 8, 2 * C + 8, dtype=torch.float16, device=DEV)            # large enough for every variant below
    vt = torch.zeros(C + 8, rows + 8, dtype=torch.float16, device=DEV)
    a = dict(n_seq=n_seq, S=S, heads=heads, ld_qk=2 * C, ld_vt=rows, ld_o=136)
    a.update({"S=12": dict(S=12), "ld_qk=2C+4": dict(ld_qk=2 * C + 4), "ld_vt=rows+4": dict(ld_vt=rows + 4), "ld_o=C+2": dict(ld_o=C + 2),
              "n_seq=0": dict(n_seq=0)}[what])
    _refused(lambda o: _spatial(ops, form, qk, qk[:, C:], vt, o, a["n_seq"], a["S"], a["heads"], a["ld_qk"], a["ld_vt"], a["ld_o"]),
             "ew_attn_spatial_log2_f16" if form == "log2" else "ew_attn_spatial_f16")


@pytest.mark.parametrize("what", ["ld=3C+4", "ld_o=C+4"])
def test_temporal_refusals(ops, what):
    B, T, S, heads = 1, 8, 4, 2
    C = heads * 64
    qkv = torch.zeros(B * T * S + 8, 3 * C + 8, dtype=torch.float16, device=DEV)
    ld, ld_o = (3 * C + 4, 136) if what == "ld=3C+4" else (3 * C, C + 4)
    _refused(lambda o: ops.attn_temporal(qkv, qkv[:, C:], qkv[:, 2 * C:], o, B, T, S, heads, ld, ld_o), "ew_attn_temporal_f16")


@pytest.mark.parametrize("what", ["D=60", "D=264", "S=2049", "ld=3C+4"])
def test_small_refusals(ops, what):
    n_seq, S, heads, D = 1, 16, 1, 64
    if what == "S=2049":
        S = 2049
    elif what.startswith("D="):
        D = int(what[2:])
    C = heads * D
    ld = 3 * C + 4 if what == "ld=3C+4" else (3 * C + 7) // 8 * 8
    qkv = torch.zeros(n_seq * S + 8, 3 * C + 16, dtype=torch.float16, device=DEV)
    _refused(lambda o: ops.attn_small(qkv, qkv[:, C:], qkv[:, 2 * C:], o, n_seq, S, heads, D, ld, 136, D ** -0.5), "ew_attn_small_f16",
             rows=max(256, S))          # (an o that the S = 2049 call would fit, if it ran)
