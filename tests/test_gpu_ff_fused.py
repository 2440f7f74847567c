"""-m gpu: the fused level-0 feed-forward kernel (ew_ff_geglu320_f16: GEGLU up-projection + down-projection + residual epilogue in
one launch, the 1280-wide intermediate never written) against (1) the same computation in fp32 torch on the fp16-rounded
operands and (2) the two-GEMM path of ew_gemm_f16 it replaces, in the three epilogue forms the transformer blocks use."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import ff_cases
from conftest import rel_l2
from kernel_checks import Guarded, report, two_prefills, worst_row

pytestmark = pytest.mark.gpu
DEV = "cuda"
# worst-row bounds per case: (bound, value measured on an MI355X); the bound is at most 2x the measurement
WORST_ROW = {
    'ff_geglu320 M=129 split out': (3.7e-06, 1.879e-06),  # measured worst row; rel-L2 9.20e-07 row 39 (logistic gate, before: 1.52e-05 / 6.92e-06)
    'ff_geglu320 M=300 split out': (3.7e-06, 1.879e-06),  # measured worst row; rel-L2 8.85e-07 row 3 (before: 1.55e-05 / 7.04e-06)
    'ff_geglu320 M=51277 split out': (1.3e-05, 6.594e-06),  # measured worst row; rel-L2 9.52e-07 row 1185 (before: 1.64e-05 / 6.95e-06)
}


def _g(s):
    return torch.Generator().manual_seed(s)


def _weights(seed):
    C, H = 320, 1280
    w1 = (torch.rand(2 * H, C, generator=_g(seed)) * 2 - 1) / C ** 0.5
    b1 = (torch.rand(2 * H, generator=_g(seed + 1)) * 2 - 1) / C ** 0.5
    w2 = (torch.rand(C, H, generator=_g(seed + 2)) * 2 - 1) / H ** 0.5
    b2 = (torch.rand(C, generator=_g(seed + 3)) * 2 - 1) / H ** 0.5
    return [t.half().to(DEV) for t in (w1, b1, w2, b2)]


def _two_gemm(x, w1, b1, w2, b2, out, **kw):
    """the path the fused kernel replaces (unet._pack's GEGLU interleave + two ew_gemm_f16 calls)"""
    from evoworld_amd import ops
    n = w1.shape[0] // 2
    idx = torch.arange(2 * n, device=DEV).reshape(2, n // 16, 16).permute(1, 0, 2).reshape(-1)
    ffh = ops.linear(x, w1[idx].contiguous(), b1[idx].contiguous(), act=ops.ACT_GEGLU)
    return ops.linear(ffh, w2, b2, out=out, **kw)


@pytest.mark.parametrize("form,M", [("s_ff", 460800), ("t_ffin", 51200 + 77), ("t_ff", 51200), ("plain", 300)])
def test_fused_ff_matches_torch_and_two_gemm_path(form, M):
    from evoworld_amd import ops
    C = 320
    w1, b1, w2, b2 = _weights(10)
    x = torch.randn(M, C, generator=_g(0)).half().to(DEV)
    pack = ops.ff_pack(w1, b1, w2)
    h = ops.Res.from_float((torch.randn(M, C, generator=_g(1)) * 2).to(DEV))
    hm = (torch.randn(M, C, generator=_g(2)) * 2).half().to(DEV)
    S = 64
    pos = torch.randn((M + S - 1) // S, C, generator=_g(3)).half().to(DEV)
    if form == "s_ff":
        kw = dict(r1=h)
        out_a, out_b = ops.Res.empty(M, C, DEV, True), ops.Res.empty(M, C, DEV, True)
        extra = h.float()
    elif form == "t_ffin":
        kw = dict(r1=h, rowbias=pos, rows_per_group=S, ld_rowbias=C)
        out_a, out_b = torch.empty(M, C, dtype=torch.float16, device=DEV), torch.empty(M, C, dtype=torch.float16, device=DEV)
        extra = h.float() + pos.float().repeat_interleave(S, 0)[:M]
    elif form == "t_ff":
        a = 0.37
        kw = dict(c_acc=1 - a, r1=hm, c_r1=1 - a, r2=h, c_r2=a)
        out_a, out_b = torch.empty(M, C, dtype=torch.float16, device=DEV), torch.empty(M, C, dtype=torch.float16, device=DEV)
        extra = None
    else:
        kw = {}
        out_a, out_b = torch.empty(M, C, dtype=torch.float16, device=DEV), torch.empty(M, C, dtype=torch.float16, device=DEV)
        extra = 0.0
    ops.ff_geglu320(x, pack, b2, out_a, **kw)
    kw2 = dict(kw)
    for k in ("r1", "r2"):
        if k in kw2:
            kw2["ld_" + k] = C
    _two_gemm(x, w1, b1, w2, b2, out_b, **kw2)
    got = out_a.float() if isinstance(out_a, ops.Res) else out_a.float()
    two = out_b.float() if isinstance(out_b, ops.Res) else out_b.float()
    # fp32 reference on a row sample (the full 460800-row reference would need 4.7 GB of fp32 intermediates)
    rows = torch.randperm(M, generator=_g(4))[:4096].to(DEV) if M > 4096 else torch.arange(M, device=DEV)
    pre = x[rows].float() @ w1.float().t() + b1.float()
    hid = (pre[:, :1280] * F.gelu(pre[:, 1280:])).half().float()
    ff = hid @ w2.float().t() + b2.float()
    if form == "t_ff":
        ref = (1 - a) * (ff + hm[rows].float()) + a * h.float()[rows]
    elif form == "t_ffin":
        ref = ff + extra[rows]
    elif form == "s_ff":
        ref = ff + extra[rows]
    else:
        ref = ff
    e_ref = rel_l2(got[rows].cpu(), ref.cpu())
    e_two = rel_l2(got.cpu(), two.cpu())
    print(f"fused feed-forward {form} M={M}: rel-L2 vs fp32 torch {e_ref:.2e}, vs the two-GEMM path {e_two:.2e}")
    assert torch.isfinite(got).all()
    assert e_ref < (3e-4 if form in ("t_ffin", "t_ff", "plain") else 1e-5 + 3e-4) and e_two < 3e-4
    if isinstance(out_a, ops.Res):        # split output: hi + lo8 carries ~19 bits
        assert e_ref < 2e-4


@pytest.mark.parametrize("M", [129, 300, 51277])
def test_fused_ff_ragged_rows_guarded(M):
    """M ragged against the 128-row tile: out and out_lo guarded past the last row (the kernel takes no output stride) and twice
    prefilled; fp64 reference (of the kernel's fp16 hidden operand) on a row sample that includes the last 128 rows"""
    from evoworld_amd import ops
    C = 320
    w1, b1, w2, b2 = _weights(30)
    x = torch.randn(M, C, generator=_g(31)).half().to(DEV)
    pack = ops.ff_pack(w1, b1, w2)
    h = ops.Res.from_float((torch.randn(M, C, generator=_g(32)) * 2).to(DEV))
    spec = dict(ld=C, pad_rows=128)
    hi, lo = two_prefills(lambda o, ol, k: ops.ff_geglu320(x, pack, b2, ops.Res(o, ol), r1=h, c_acc=0.8),
                          (M, C, torch.float16, spec), (M, C, torch.int8, spec))
    rows = torch.cat([torch.arange(0, max(M - 128, 0), 13), torch.arange(max(M - 128, 0), M)]).to(DEV)
    pre = x[rows].double() @ w1.double().t() + b1.double()
    hid = (pre[:, :1280] * F.gelu(pre[:, 1280:])).half().double()
    ref = 0.8 * (hid @ w2.double().t() + b2.double()) + h.float()[rows].double()
    case = f"ff_geglu320 M={M} split out"
    report(case, ops.Res(hi.view, lo.view).float()[rows], ref, WORST_ROW[case][0], 2e-4)


def test_fused_ff_is_deterministic_and_times():
    from evoworld_amd import ops
    M, C = 460800, 320
    w1, b1, w2, b2 = _weights(20)
    x = torch.randn(M, C, generator=_g(5)).half().to(DEV)
    h = ops.Res.from_float(torch.randn(M, C, generator=_g(6)).to(DEV))
    pack = ops.ff_pack(w1, b1, w2)
    o1, o2 = ops.Res.empty(M, C, DEV, True), ops.Res.empty(M, C, DEV, True)
    ops.ff_geglu320(x, pack, b2, o1, r1=h)
    ops.ff_geglu320(x, pack, b2, o2, r1=h)
    assert torch.equal(o1.hi, o2.hi) and torch.equal(o1.lo, o2.lo)

    def t(fn, n=5):
        fn(); torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e) / n
    fused = t(lambda: ops.ff_geglu320(x, pack, b2, o1, r1=h))
    pair = t(lambda: _two_gemm(x, w1, b1, w2, b2, o2, r1=h, ld_r1=C))
    fl = 2.0 * M * C * 2560 + 2.0 * M * 1280 * C
    print(f"level-0 feed-forward (460800 tokens): fused {fused:.3f} ms ({fl / fused / 1e9:.0f} TF/s) vs two GEMMs {pair:.3f} ms ({fl / pair / 1e9:.0f} TF/s)")


# ----------------------------------------------------------------------------------------------------------------------------------
# Per row, every operand form, chained tiles (tests/ff_cases.py; tests/test_cpu_ff_cases.py checks the helpers on the CPU).
# Everything below runs under the default CU budget (G = ew_get_cu_budget()) on the default stream.
@pytest.fixture(scope="module")
def ops():
    from evoworld_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from evoworld_amd import _lib
    L = _lib.load()
    gen = L.ew_get_gemm_generation()
    yield L
    L.ew_set_gemm_generation(gen)


def _planes(M, split, prefill=0):
    return [Guarded(M, ff_cases.C, dt, ld=ff_cases.C, pad_rows=128, prefill=prefill, device=DEV) for dt in ([torch.float16, torch.int8] if split else [torch.float16])]


@pytest.mark.parametrize("cid", list(ff_cases.FF_CASES))
def test_case(ops, lib, cid):
    """One FF_CASES entry: fused kernel and twin (the two-GEMM path under generation 1) each into guarded, twice-prefilled planes;
    both against fp64 on ALL rows by rel-L2 and by worst row (bound: 2 x the TWIN's measured worst row, ff_cases.WORST_ROW); fused
    against twin.

    What this test found: with the fitted logistic gate (ew_vgelu2, 2.6e-5 absolute) the split-output cases F1, F6, F7, F8, F9, F12 missed
    their worst-row bounds against fp64 and against the twin (rel-L2 / worst row: F1 8.62e-6 / 1.34e-5 at row 66, F6 1.48e-4 / 2.36e-4 at
    row 69, F7 7.48e-6 / 9.46e-6, F8 6.28e-6 / 1.20e-5, F9 8.62e-6 / 3.49e-5 at row 13094, F12 7.45e-6 / 1.15e-5; the twin 0.86e-6 ...
    1.0e-6 / 1e-6 ... 8.8e-6, F6 5.65e-6 / 3.77e-5).  The excess lay on all rows -- not one tile, wave or chain position, and the chained
    F9 showed the figures of the single-tile F1 -- and vanished against an fp64 reference with the fitted gate (ref(fitted=True): rel-L2
    1.0e-6 ... 1.2e-6).  ff320_kernel now uses the erf form of the gate (ew_vgelu2_erf), as generation 1 does; the figures of both are in
    ff_cases.WORST_ROW."""
    c = ff_cases.FF_CASES[cid]
    G = lib.ew_get_cu_budget()
    p = ff_cases.problem(ops, c, G)
    M, C = p.M, ff_cases.C
    assert ff_cases.instantiation(c) == (int(p.split or any(isinstance(r, ops.Res) for r in (p.r1, p.r2))), int(p.r2 is not None))
    spec = dict(ld=C, pad_rows=128)
    specs = [(M, C, torch.float16, spec)] + ([(M, C, torch.int8, spec)] if p.split else [])
    gf = two_prefills(lambda *a: p.run(*a[:-1]), *specs)
    gt = two_prefills(lambda *a: p.run_twin(*a[:-1]), *specs)
    dec = lambda gs: ops.Res(gs[0].view, gs[1].view).float() if p.split else gs[0].view.float()
    fused, twin = dec(gf), dec(gt)
    ref = p.ref()
    n_tiles = [len(t) for t in ff_cases.schedule(M, G)]
    print(f"{cid}: M {M} = {sum(n_tiles)} tiles on {len(n_tiles)} workgroups, {min(n_tiles)}-{max(n_tiles)} tiles per workgroup, "
          f"ff320_kernel<{', '.join(map(str, ff_cases.instantiation(c)))}>")
    assert (max(n_tiles) >= 2) == (cid in ff_cases.CHAINED), f"{cid}: chains of {max(n_tiles)} at a CU budget of {G}"
    bound = ff_cases.WORST_ROW[cid][0]
    tol = ff_cases.BOUND_SPLIT if p.split else ff_cases.BOUND
    failed = []                                          # every figure is printed before the test fails

    def check(fn, what):
        try:
            return fn()
        except AssertionError as e:
            failed.append(f"{what}: {e}")

    check(lambda: report(f"{cid} twin", twin, ref, bound, tol), "twin vs fp64")
    r = check(lambda: report(f"{cid} fused", fused, ref, bound, tol), "fused vs fp64")
    if r is None:
        failed.append("fused kernel: " + ff_cases.where_row(worst_row(fused, ref)[1], G))
    check(lambda: report(f"{cid} fused vs twin", fused, twin, 2 * bound, tol), "fused vs twin")
    assert torch.isfinite(fused).all()
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("cid", ff_cases.CHAINED)
def test_piece_identity(ops, lib, cid):
    """A tile's accumulators, hf_old and acc1p start from zero and the chunk order is fixed, so a tile's arithmetic cannot depend on its
    position in a workgroup's chain: the whole launch (chains of 2-3 tiles) and its pieces of at most G tiles, each launched alone on
    row-offset pointers (one tile per workgroup), agree BIT FOR BIT on hi and lo8."""
    c = ff_cases.FF_CASES[cid]
    G = lib.ew_get_cu_budget()
    p = ff_cases.problem(ops, c, G)
    pieces = ff_cases.piece_ranges(p.M, G, p.rpg if p.rb is not None else None)
    assert max(len(t) for t in ff_cases.schedule(p.M, G)) >= 2 and len(pieces) >= 2
    gw = _planes(p.M, p.split)
    p.run(*[g.view for g in gw])
    n_bad, where = 0, []
    for r0, r1 in pieces:
        assert max(len(t) for t in ff_cases.schedule(r1 - r0, G)) == 1
        gp = _planes(r1 - r0, p.split)
        p.run(*[g.view for g in gp], r0=r0, r1_=r1)
        torch.cuda.synchronize()
        for w, g in zip(gw, gp):
            g.check()
            n, s = ff_cases.piece_diff(w.view[r0:r1], g.view, r0, G)
            n_bad += n
            if n:
                where.append(("lo8 " if g.dtype == torch.int8 else "hi ") + s)
    for g in gw:
        g.check()
    print(f"{cid} pieces: {len(pieces)} launches {pieces}, {n_bad} differing elements")
    assert n_bad == 0, f"{cid}: {n_bad} elements of the whole launch differ from its single-tile-per-workgroup pieces: {'; '.join(where)}"


@pytest.mark.parametrize("cid", ["F2", "F10"])
def test_rowbias_group_seams(ops, lib, cid):
    """x = 0, b1 = b2 = 0, residual zeros, row g of the bias = g + 1: the output is m // rows_per_group + 1 EXACTLY on every row (ragged
    groups of 37 crossing fragments, tiles and chain seams, the partial last group), whatever bias columns 320..327 hold"""
    c = ff_cases.FF_CASES[cid]
    G = lib.ew_get_cu_budget()
    p = ff_cases.problem(ops, c, G, zero=True)
    assert not p.split and p.rb is not None and p.ld > ff_cases.C and p.M % p.rpg
    want = (torch.arange(p.M, device=DEV) // p.rpg + 1).half()[:, None].expand(p.M, ff_cases.C)
    for filler in (float("nan"), -3000.0):
        p.rb[:, ff_cases.C:] = filler
        (g,) = _planes(p.M, False)
        p.run(g.view)
        torch.cuda.synchronize()
        g.check()
        bad = (g.view != want).any(1).nonzero()
        assert bad.numel() == 0, (f"{cid} (bias columns 320.. = {filler}): {bad.numel()} rows differ from m // {p.rpg} + 1, first "
                                  f"{ff_cases.where_row(int(bad[0]), G)}: got {g.view[int(bad[0]), :4].tolist()}, want {float(want[int(bad[0]), 0])}")


@pytest.fixture(scope="module")
def gate():
    x, w1, b1, w2s, b2, v, g = ff_cases.gate_problem()
    ref, tol = ff_cases.gate_bound(v, g)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return dict(x=x.to(DEV), w1=w1.to(DEV), b1=b1.to(DEV), w2s=[w.to(DEV) for w in w2s], b2=b2.to(DEV), v=t(v), g=t(g), ref=t(ref), tol=t(tol))


def _check_gates(got, gate, name, unit_of):
    """got [rows, n * 160] (fp16): column n carries the (v, g) pair of column n % 160"""
    reps = got.shape[1] // 160
    v, g, ref, tol = (gate[k].repeat(1, reps) for k in ("v", "g", "ref", "tol"))
    got = got.double()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    small = g.abs() <= 12
    over = ((got - ref).abs() - tol).masked_fill(~small, -1.0)
    m, n = divmod(int(over.argmax()), got.shape[1])
    print(f"{name}: |g| <= 12: largest |err| - bound {float(over[m, n]):.3e} at g = {float(g[m, n])}, v = {float(v[m, n])} ({unit_of(n)}); "
          f"largest |err| {float(((got - ref).abs() * small).max()):.3e}")
    assert float(over[m, n]) <= 0, (f"{name}: v = {float(v[m, n])}, g = {float(g[m, n])}: got {float(got[m, n])}, want {float(ref[m, n])} "
                                   f"+- {float(tol[m, n]):.3e} ({unit_of(n)}, row {m})")
    big = ~small
    want = torch.where(g > 0, (v * g).half().double(), torch.zeros_like(g))
    bad = (big & (got != want)).nonzero()
    assert bad.numel() == 0, (f"{name}: large gates: {bad.shape[0]} wrong, first g = {float(g[tuple(bad[0])])}, v = {float(v[tuple(bad[0])])}: "
                              f"got {float(got[tuple(bad[0])])}, want {float(want[tuple(bad[0])])} ({unit_of(int(bad[0][1]))})")
    assert int(big.sum()) == reps * len(ff_cases.BIG_GATES)


@pytest.mark.parametrize("b", range(4))
def test_gate_range(ops, gate, b):
    """every fp16 gate of [-12, 12] and +-16, +-100, +-2048 through hidden units 320 b ... 320 b + 319 of the fused kernel (all 40
    chunks, both wave halves and every lane slot over the four packs): |out - v gelu(g)| within ff_cases.gate_bound, large gates
    exactly fp16(v g) or 0"""
    pack = ops.ff_pack(gate["w1"], gate["b1"], gate["w2s"][b])
    out = torch.empty(gate["x"].shape[0], ff_cases.C, dtype=torch.float16, device=DEV)
    ops.ff_geglu320(gate["x"], pack, gate["b2"], out)

    def unit_of(n):
        j = 320 * b + n
        kk = j % 32
        return f"hidden unit {j}: chunk {j // 32}, lane slot fks {kk // 8}, wave half wn {(kk % 8) // 4}, e {kk % 4}"
    _check_gates(out, gate, f"ff_geglu320 gate range, pack {b}", unit_of)


def test_gate_range_linear_geglu(ops, lib, gate):
    """the same sweep through ew_gemm_f16's GEGLU epilogue under the default generation (it shares ew_vgelu2), same bound"""
    idx = ff_cases.geglu_interleave(ff_cases.HID)
    hid = ops.linear(gate["x"], gate["w1"][idx].contiguous(), gate["b1"][idx].contiguous(), act=ops.ACT_GEGLU)
    assert tuple(hid.shape) == (gate["x"].shape[0], ff_cases.HID)
    _check_gates(hid, gate, f"linear GEGLU gate range ({lib.ew_gemm_last_kernel().decode()})", lambda n: f"hidden unit {n}")


def test_refusals(ops, lib):
    """The C entry refuses bad arguments with a status, a message naming the entry and no launch; ops.ff_geglu320 raises before any
    launch on planes the strideless ABI would misread.  The guarded output keeps its prefill through all of it."""
    from evoworld_amd import _lib
    M, C = 40, ff_cases.C
    w1, b1, w2, b2 = ff_cases.weights(50)
    pack = ops.ff_pack(w1, b1, w2)
    x = torch.randn(M, C, generator=_g(51)).half().to(DEV)
    res = ops.Res.from_float(torch.randn(M, C, generator=_g(52)).to(DEV))
    rb = torch.randn(M, 328, generator=_g(53)).half().to(DEV)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def c_call(out_, **over):
        a = _lib.FfArgs()
        a.x, a.w1p, a.b1p, a.w2p, a.b2, a.out, a.zero_page = P(x), P(pack[0]), P(pack[1]), P(pack[2]), P(b2), P(out_), P(ops.zero_page(x.device))
        a.M, a.C, a.hidden, a.rows_per_group, a.ld_rowbias = M, C, 1280, 1, C
        a.c_acc = a.c_r1 = a.c_r2 = 1.0
        for k, v in over.items():
            setattr(a, k, P(v) if torch.is_tensor(v) or v is None else v)
        return lib.ew_ff_geglu320_f16(ctypes.byref(a), stream)

    # the argument builder itself is sound: the same call with nothing wrong runs
    ok = torch.empty(M, C, dtype=torch.float16, device=DEV)
    assert c_call(ok, rowbias=rb, ld_rowbias=328, r1=res.hi, r1_lo=res.lo) == 0
    want = torch.empty_like(ok)
    ops.ff_geglu320(x, pack, b2, want, rowbias=rb, ld_rowbias=328, r1=res)
    assert torch.equal(ok, want)

    g = Guarded(M, C, torch.float16, ld=C, pad_rows=128, prefill=1, device=DEV)
    out = g.view

    def untouched():
        torch.cuda.synchronize()
        assert bool((g.buf.view(torch.int16) == g.pattern).all()), "a refused call wrote to the output"

    bad_c = dict(null_x=dict(x=None), null_w1p=dict(w1p=None), null_b1p=dict(b1p=None), null_w2p=dict(w2p=None), null_b2=dict(b2=None),
                 null_out=dict(out=None), null_zero_page=dict(zero_page=None), C=dict(C=328), hidden=dict(hidden=1312), M0=dict(M=0),
                 M_negative=dict(M=-1), rows_per_group=dict(rows_per_group=0), ld_rowbias=dict(rowbias=rb, ld_rowbias=324),
                 r1_lo_alone=dict(r1_lo=res.lo), r2_lo_alone=dict(r2_lo=res.lo))
    for name, over in bad_c.items():
        st = c_call(out, **over)
        msg = (lib.ew_last_error() or b"").decode()
        assert st != 0 and "ew_ff_geglu320_f16" in msg, (name, st, msg)
    assert lib.ew_ff_geglu320_f16(None, stream) != 0 and "ew_ff_geglu320_f16" in (lib.ew_last_error() or b"").decode()
    untouched()

    wide = lambda dt=torch.float16: torch.zeros(M, 384, dtype=dt, device=DEV)[:, :C]
    f16 = lambda *s: torch.zeros(*s, dtype=torch.float16, device=DEV)
    i8 = lambda *s: torch.zeros(*s, dtype=torch.int8, device=DEV)
    Res = ops.Res
    bad_py = dict(
        out_view=dict(out=wide()), r1_view=dict(r1=wide()), r2_view=dict(r2=wide()), out_lo_view=dict(out=Res(f16(M, C), wide(torch.int8))),
        r1_lo_view=dict(r1=Res(f16(M, C), wide(torch.int8))),
        out_row_short=dict(out=f16(M - 1, C)), out_row_long=dict(out=f16(M + 1, C)), r1_rows=dict(r1=f16(M + 1, C)), r2_rows=dict(r2=f16(M - 1, C)),
        out_width=dict(out=f16(M, 328)), r1_width=dict(r1=f16(M, 160)), out_1d=dict(out=f16(M * C)),
        out_dtype=dict(out=torch.zeros(M, C, device=DEV)), r1_dtype=dict(r1=torch.zeros(M, C, dtype=torch.bfloat16, device=DEV)),
        r2_dtype=dict(r2=i8(M, C)), out_lo_dtype=dict(out=Res(f16(M, C), torch.zeros(M, C, dtype=torch.uint8, device=DEV))),
        r1_lo_dtype=dict(r1=Res(f16(M, C), f16(M, C))), r2_lo_dtype=dict(r2=Res(f16(M, C), torch.zeros(M, C, dtype=torch.int16, device=DEV))),
        out_lo_shape=dict(out=Res(f16(M, C), i8(M - 1, C))), r1_lo_shape=dict(r1=Res(f16(M, C), i8(M, 328))), r2_lo_shape=dict(r2=Res(f16(M, C), i8(M + 1, C))),
        b2_dtype=dict(b2=b2.float()), b2_short=dict(b2=b2[:319]), b2_long=dict(b2=f16(328)), b2_2d=dict(b2=b2[None]), b2_strided=dict(b2=f16(2 * C)[::2]),
        rb_dtype=dict(rowbias=rb.float(), ld_rowbias=328), rb_col_stride=dict(rowbias=f16(328, M).t(), ld_rowbias=328),
        rb_row_stride=dict(rowbias=rb, ld_rowbias=C), rb_default_ld=dict(rowbias=rb), rb_rows=dict(rowbias=rb[:M - 1], ld_rowbias=328),
        rb_groups=dict(rowbias=rb[:13], ld_rowbias=328, rows_per_group=3), rb_narrow=dict(rowbias=f16(M, 312), ld_rowbias=312), rb_1d=dict(rowbias=f16(M * C)))
    for name, over in bad_py.items():
        kw = dict(b2=b2, out=out)
        kw.update(over)
        b2_, out_ = kw.pop("b2"), kw.pop("out")
        with pytest.raises((TypeError, ValueError, _lib.EvoWorldHipError)):
            ops.ff_geglu320(x, pack, b2_, out_, **kw)
            pytest.fail(f"{name}: ops.ff_geglu320 accepted it")
    untouched()
    # ... and the forms next to them that are fine
    ops.ff_geglu320(x, pack, b2, out, rowbias=rb[:14], ld_rowbias=328, rows_per_group=3, r1=res, r2=res.hi)
    torch.cuda.synchronize()
    g.check()
    assert torch.isfinite(out).all()
