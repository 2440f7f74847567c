"""-m gpu: the GroupNorm kernels of csrc/norm.hip through the C ABI (stats -> finalize -> apply / apply_split) against the fp64
reference of tests/groupnorm_cases.py, at the shapes, row contents and argument edges that tests/test_gpu_ops.py does not reach;
and a LayerNorm companion.  The cases, their bounds and why each case can bear its bound: groupnorm_cases.py and
test_cpu_groupnorm_cases.py.

Every GroupNorm run goes into kernel_checks.Guarded buffers -- the output (split form: row stride 2 C + 64 > width; the plain
entry point has no stride argument, its rows are C_tot wide and only the sentinel rows guard it) and the workspace -- under
two_prefills, so neither may be written outside its extent and neither's previous contents may matter.

(a) / (b) statistics when rows are atypical, read through the split output (the plain fp16 output hides anything below 2.8e-4),
and with the rows of every slab rolled by one.  MEASURED holds the worst row seen on an MI355X per case next to its bound."""
import pytest
import torch

import groupnorm_cases as gc
from kernel_checks import Guarded, pattern, report, two_prefills

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (shape, dist, kind) -> worst row measured on an MI355X, the largest over plain / split input and rows as built / rolled by one.
# The bound is gc.BOUND_SPLIT[dist] (1e-4 for n75, 1e-5 for n03): derived in groupnorm_cases.py, not taken from this table.
# With the statistics pivoting on row 0 of the slab (before the per-thread pivots) the same run gave, at 2x9216x64: n75 alike
# 2.1e-5, row0_zero 2.5e-3, row0_300 1.6e-3, last_row (rolled) 2.0e-3; n03 alike 1.1e-6, row0_300 1.8e-3; at 2x9216x320 n75
# row0_zero 3.1e-4; at 64x9216x64 n75 alike 2.5e-5, row0_zero 1.1e-3, n03 row0_300 7.2e-4 -- the emulation of
# groupnorm_cases.emulate_row0_pivot_stats had said 2.4e-3 / 5.8e-4 / 9.7e-4 of rstd for the three n75 row0_zero cases.
MEASURED = {
    ('2x9216x64', 'n75', 'alike'): 2.28e-5,
    ('2x9216x64', 'n75', 'row0_zero'): 1.94e-5,
    ('2x9216x64', 'n75', 'row0_300'): 1.51e-5,
    ('2x9216x64', 'n75', 'last_row'): 1.95e-5,
    ('2x9216x64', 'n75', 'interior_row'): 1.98e-5,
    ('2x9216x64', 'n75', 'first_line'): 7.83e-6,
    ('2x9216x64', 'n75', 'border'): 3.13e-6,
    ('2x9216x64', 'n03', 'alike'): 2.10e-7,
    ('2x9216x64', 'n03', 'row0_zero'): 2.03e-7,
    ('2x9216x64', 'n03', 'row0_300'): 6.95e-7,
    ('2x9216x64', 'n03', 'last_row'): 2.10e-7,
    ('2x9216x64', 'n03', 'interior_row'): 2.03e-7,
    ('2x9216x64', 'n03', 'first_line'): 2.15e-7,
    ('2x9216x64', 'n03', 'border'): 2.52e-7,
    ('2x9216x320', 'n75', 'alike'): 1.90e-5,
    ('2x9216x320', 'n75', 'row0_zero'): 1.93e-5,
    ('2x9216x320', 'n75', 'row0_300'): 1.28e-5,
    ('2x9216x320', 'n75', 'last_row'): 1.94e-5,
    ('2x9216x320', 'n75', 'interior_row'): 1.84e-5,
    ('2x9216x320', 'n75', 'first_line'): 3.33e-6,
    ('2x9216x320', 'n75', 'border'): 1.32e-6,
    ('2x9216x320', 'n03', 'alike'): 1.03e-7,
    ('2x9216x320', 'n03', 'row0_zero'): 1.10e-7,
    ('2x9216x320', 'n03', 'row0_300'): 2.99e-7,
    ('2x9216x320', 'n03', 'last_row'): 1.11e-7,
    ('2x9216x320', 'n03', 'interior_row'): 1.17e-7,
    ('2x9216x320', 'n03', 'first_line'): 1.21e-7,
    ('2x9216x320', 'n03', 'border'): 1.18e-7,
    ('64x9216x64', 'n75', 'alike'): 2.54e-5,
    ('64x9216x64', 'n75', 'row0_zero'): 2.23e-5,
    ('64x9216x64', 'n75', 'row0_300'): 1.58e-5,
    ('64x9216x64', 'n75', 'last_row'): 2.48e-5,
    ('64x9216x64', 'n75', 'interior_row'): 2.43e-5,
    ('64x9216x64', 'n75', 'first_line'): 3.29e-6,
    ('64x9216x64', 'n75', 'border'): 1.10e-6,
    ('64x9216x64', 'n03', 'alike'): 1.95e-7,
    ('64x9216x64', 'n03', 'row0_zero'): 2.18e-7,
    ('64x9216x64', 'n03', 'row0_300'): 3.24e-6,
    ('64x9216x64', 'n03', 'last_row'): 2.02e-7,
    ('64x9216x64', 'n03', 'interior_row'): 1.89e-7,
    ('64x9216x64', 'n03', 'first_line'): 1.97e-7,
    ('64x9216x64', 'n03', 'border'): 1.86e-7,
}
# (d): largest worst row over the 27 ABI cases x 4 forms each: split output 3.4e-7 ("40000 rows"; bound 1e-5), plain output
# 4.26e-4 ("C8"; bound 2^-11 + 1e-4 = 5.9e-4).  (f): LayerNorm mean/std 300: 2.36e-4 (C = 320), 2.20e-4 (C = 2048); one row:
# 1.77e-4 ... 2.06e-4 (bound 4.98e-4).
assert set(MEASURED) == set(gc.STAT_CASES)


@pytest.fixture(scope="module")
def ops():
    from evoworld_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def lib():
    from evoworld_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def noise():
    cache = {}

    def get(shape):
        if shape not in cache:
            cache.clear()                                   # one shape at a time on the device
            cache[shape] = gc.stat_noise(shape).to(DEV)
        return cache[shape]
    return get


def _check(lib, status, what):
    from evoworld_amd import _lib
    _lib.check(status, what)


def run_groupnorm(ops, lib, srcs, gh, bh, n, rows, groups, silu, split_out, eps=gc.EPS):
    """stats per source -> finalize -> apply per source through the C ABI.  srcs: [(hi, lo or None)] of [n * rows, C_i].
    Returns the result as fp64 [n * rows, C_tot] (split form: y_hi + y_lo)."""
    p, st = ops._ptr, ops._stream()
    Cs = [h.shape[1] for h, _ in srcs]
    C = sum(Cs)
    nws = lib.ew_groupnorm_workspace_floats(n, rows, C, groups)
    assert nws >= gc.workspace_floats(n, rows, C, groups)
    width, ld_y = (2 * C, 2 * C + 64) if split_out else (C, C)

    def run(y, ws, k):
        off = 0
        for (h, l), c in zip(srcs, Cs):
            _check(lib, lib.ew_groupnorm_stats_f16(p(h), p(l), p(ws), n, rows, c, off, C, groups, st), "stats")
            off += c
        _check(lib, lib.ew_groupnorm_finalize(p(ws), n, rows, C, groups, st), "finalize")
        off = 0
        for (h, l), c in zip(srcs, Cs):
            if split_out:
                _check(lib, lib.ew_groupnorm_apply_split_f16(p(h), p(l), p(ws), p(gh), p(bh), p(y), p(y[:, C:]), ld_y, n, rows, c, off, C,
                                                             groups, eps, int(silu), st), "apply_split")
            else:
                _check(lib, lib.ew_groupnorm_apply_f16(p(h), p(l), p(ws), p(gh), p(bh), p(y), n, rows, c, off, C, groups, eps, int(silu), st),
                       "apply")
            off += c
    y = two_prefills(run, (n * rows, width, torch.float16, dict(ld=ld_y, pad_rows=64)),
                     (1, nws, torch.float32, dict(ld=nws, pad_rows=1)))[0].view
    return (y[:, :C].double() + y[:, C:].double()) if split_out else y.double()


# ----------------------------------------------------------------------------- (a), (b): atypical rows; row order
@pytest.mark.parametrize("shape,dist,kind", gc.STAT_CASES)
def test_groupnorm_atypical_rows(ops, lib, noise, shape, dist, kind):
    n, rows, C = gc.STAT_SHAPES[shape]
    gamma, beta = gc.params(C)
    gh, bh = gamma.to(DEV), beta.to(DEV)
    x = gc.stat_input(noise(shape), shape, dist, kind)
    bound = gc.BOUND_SPLIT[dist]
    failures = []
    for split in (False, True):
        hi, lo, val = gc.operand(x, split)
        ref = gc.reference(val, gh, bh, 32, silu=gc.STAT_SILU)[0]
        del val
        for rolled in (False, True):
            if rolled:
                hi, lo = torch.roll(hi, 1, dims=1), (None if lo is None else torch.roll(lo, 1, dims=1))
            src = (hi.reshape(n * rows, C), None if lo is None else lo.reshape(n * rows, C))
            got = run_groupnorm(ops, lib, [src], gh, bh, n, rows, 32, gc.STAT_SILU, True)
            if rolled:
                got = torch.roll(got.reshape(n, rows, C), -1, dims=1).reshape(n * rows, C)
            case = f"groupnorm {shape} {dist} {kind} {'split' if split else 'fp16'} in{' rolled' if rolled else ''}"
            try:
                report(case, got, ref, bound)
            except AssertionError as e:                      # every form of the case is measured before the test fails
                failures.append(str(e))
            del got
        del ref
    assert not failures, failures


# ----------------------------------------------------------------------------- (d): shapes the ABI admits
@pytest.mark.parametrize("name", list(gc.ABI_CASES))
def test_groupnorm_abi_shapes(ops, lib, name):
    """groups != 32, concat seams inside a group, the thread-layout, row-count and chunking edges.  '40000 rows' pins that a chunk
    past the last row still writes its (empty) partial: the workspace is prefilled with NaNs and with finite values, and the
    two results must agree bit for bit and with the reference."""
    n, rows, groups, Cs = gc.ABI_CASES[name]
    C = sum(Cs)
    gamma, beta = gc.params(C)
    gh, bh = gamma.to(DEV), beta.to(DEV)
    x = gc.abi_input(name).to(DEV)
    if name == "40000 rows":
        assert gc.empty_chunks(n, rows)
    for split_in in (False, True):
        hi, lo, val = gc.operand(x, split_in)
        srcs = list(zip(gc.split_sources(hi, Cs), gc.split_sources(lo, Cs) if split_in else [None] * len(Cs)))
        for silu in (False, True):
            ref = gc.reference(val, gh, bh, groups, silu=silu)[0]
            for split_out in (False, True):
                got = run_groupnorm(ops, lib, srcs, gh, bh, n, rows, groups, silu, split_out)
                case = f"groupnorm abi {name} {'split' if split_in else 'fp16'} in {'split' if split_out else 'fp16'} out silu={int(silu)}"
                report(case, got, ref, gc.BOUND_SPLIT["n03"] if split_out else gc.BOUND_PLAIN)


# ----------------------------------------------------------------------------- (e): refusals
def test_groupnorm_refusals(ops, lib):
    """argument checks on the host: a non-OK status with an ew_last_error text, nothing launched, nothing written.  Every buffer
    is large enough for the arguments as passed, so that even an entry point that failed to refuse would stay inside them."""
    p, st = ops._ptr, ops._stream()
    n, rows = 1, 2
    x = torch.zeros(1 << 16, dtype=torch.float16, device=DEV)
    xl = torch.zeros(1 << 16, dtype=torch.int8, device=DEV)
    gh, bh = torch.ones(1 << 14, dtype=torch.float16, device=DEV), torch.zeros(1 << 14, dtype=torch.float16, device=DEV)
    y = Guarded(16, 1 << 15, torch.float16, ld=1 << 15, pad_rows=1, device=DEV)
    ws = Guarded(1, 1 << 20, torch.float32, ld=1 << 20, pad_rows=1, device=DEV)
    Y, YL, W = p(y.view), p(y.view[8:]), p(ws.view)
    eps = gc.EPS
    calls = {
        "stats C_src % 8": lambda: lib.ew_groupnorm_stats_f16(p(x), p(xl), W, n, rows, 12, 0, 64, 4, st),
        "apply C_src % 8": lambda: lib.ew_groupnorm_apply_f16(p(x), p(xl), W, p(gh), p(bh), Y, n, rows, 12, 0, 64, 4, eps, 1, st),
        "stats C_tot % groups": lambda: lib.ew_groupnorm_stats_f16(p(x), p(xl), W, n, rows, 64, 0, 64, 5, st),
        "finalize C_tot % groups": lambda: lib.ew_groupnorm_finalize(W, n, rows, 64, 5, st),
        "apply C_tot % groups": lambda: lib.ew_groupnorm_apply_f16(p(x), p(xl), W, p(gh), p(bh), Y, n, rows, 64, 0, 64, 5, eps, 1, st),
        "stats c_off + C_src > C_tot": lambda: lib.ew_groupnorm_stats_f16(p(x), p(xl), W, n, rows, 64, 8, 64, 4, st),
        "apply c_off + C_src > C_tot": lambda: lib.ew_groupnorm_apply_f16(p(x), p(xl), W, p(gh), p(bh), Y, n, rows, 64, 8, 64, 4, eps, 1, st),
        "apply_split ld_y < C_tot": lambda: lib.ew_groupnorm_apply_split_f16(p(x), p(xl), W, p(gh), p(bh), Y, YL, 56, n, rows, 64, 0, 64, 4,
                                                                             eps, 1, st),
        "apply_split ld_y % 8": lambda: lib.ew_groupnorm_apply_split_f16(p(x), p(xl), W, p(gh), p(bh), Y, YL, 132, n, rows, 64, 0, 64, 4,
                                                                         eps, 1, st),
        "finalize C_tot / groups > 512": lambda: lib.ew_groupnorm_finalize(W, n, rows, 1032, 2, st),
        "stats C_src > 8192": lambda: lib.ew_groupnorm_stats_f16(p(x), p(xl), W, n, rows, 8200, 0, 8200, 25, st),
        "apply_split null y_lo": lambda: lib.ew_groupnorm_apply_split_f16(p(x), p(xl), W, p(gh), p(bh), Y, None, 128, n, rows, 64, 0, 64, 4,
                                                                          eps, 1, st),
    }
    for what, call in calls.items():
        status = call()
        msg = lib.ew_last_error()
        torch.cuda.synchronize()
        assert status != 0, what
        assert msg and b"ew_groupnorm" in msg, (what, msg)
        for g in (y, ws):
            g.check()
            assert bool((g.view.view(g.itype) == g.pattern).all()), what
    # the same buffers take the accepted form of these calls
    _check(lib, lib.ew_groupnorm_stats_f16(p(x), p(xl), W, n, rows, 64, 0, 64, 4, st), "stats")
    _check(lib, lib.ew_groupnorm_finalize(W, n, rows, 64, 4, st), "finalize")
    _check(lib, lib.ew_groupnorm_apply_split_f16(p(x), p(xl), W, p(gh), p(bh), Y, YL, 128, n, rows, 64, 0, 64, 4, eps, 1, st), "apply_split")
    torch.cuda.synchronize()
    y.check()
    ws.check()
    assert not bool((y.view.reshape(-1)[:64].view(torch.int16) == pattern(torch.float16, 0)).any())


# ----------------------------------------------------------------------------- (f): LayerNorm companion
# worst-row bounds of test_gpu_ops.test_layernorm_guarded at the same C (its WORST_ROW table), rel-L2 4e-4
LN_BOUNDS = {320: 4.9e-4, 2048: 4.4e-4}


def _layernorm_ref(val, gh, bh):
    v = val.double()
    v = v - v.mean(dim=1, keepdim=True)
    return v * (v.square().mean(dim=1, keepdim=True) + 1e-5).rsqrt() * gh.double() + bh.double()


@pytest.mark.parametrize("C", [320, 2048])
@pytest.mark.parametrize("split", [False, True])
def test_layernorm_mean_over_std_300(ops, C, split):
    rows = 263
    x = torch.randn(rows, C, generator=gc._gen(f"ln 300 {C}")) * 0.25 + 75.0
    gamma, beta = gc.params(C, "ln")
    gh, bh = gamma.to(DEV), beta.to(DEV)
    hi, lo, val = gc.operand(x.to(DEV), split)
    y = two_prefills(lambda y, k: ops.layernorm(ops.Res(hi, lo), gh, bh, out=y), (rows, C, torch.float16, dict(ld=C, pad_rows=16)))[0].view
    report(f"layernorm mean/std 300 {rows}x{C} {'split' if split else 'fp16'} in", y, _layernorm_ref(val, gh, bh), LN_BOUNDS[C], 4e-4)


@pytest.mark.parametrize("C", [64, 640, 1280, 2048])
def test_layernorm_one_row(ops, C):
    """rows = 1 for each register layout (1 to 4 vectors per lane).  Bound: the fp16 half-ulp, relative, on every element of the
    row, plus 1e-5 for the fp32 statistics"""
    x = torch.randn(1, C, generator=gc._gen(f"ln one row {C}")) * 2 + 0.5
    gamma, beta = gc.params(C, "ln")
    gh, bh = gamma.to(DEV), beta.to(DEV)
    hi, lo, val = gc.operand(x.to(DEV), True)
    y = two_prefills(lambda y, k: ops.layernorm(ops.Res(hi, lo), gh, bh, out=y), (1, C, torch.float16, dict(ld=C, pad_rows=16)))[0].view
    report(f"layernorm 1x{C}", y, _layernorm_ref(val, gh, bh), 2.0 ** -11 + 1e-5)
