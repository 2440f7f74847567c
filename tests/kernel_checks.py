"""Checks shared by the kernel tests (a plain module, imported like conftest.rel_l2).

- worst_row: the largest per-row relative error, so that one wrong row (a ragged last tile, a partial key block, one lane
  group's rescale) is not averaged away by a whole-tensor rel-L2.
- Guarded: an output view inside a larger backing buffer prefilled with a fixed byte pattern; check() asserts that nothing
  outside [0:rows, 0:width] was written (past the last row, or between the width and the row stride).
- two_prefills: the same call into two sets of guarded buffers prefilled with different patterns must give bit-identical
  results -- catches elements that are never written and kernels that read their own output.

Everything runs on the device of the tensors it is given (some GPU buffers are several GB).
tests/test_cpu_kernel_checks.py shows on the CPU that each check catches what it claims."""
import torch

# integer view used for every bit comparison (NaN != NaN in the float view)
_INT = {torch.float16: torch.int16, torch.float32: torch.int32, torch.int8: torch.int8, torch.uint8: torch.uint8}
# two prefill patterns per dtype: [0] a NaN payload (float types), [1] a finite value; 0x5A / 0xA5 for bytes
_PATTERNS = {torch.float16: (0x7E5A, 0x5A5A), torch.float32: (0x7FC05A5A, 0x5A5A5A5A), torch.int8: (0x5A, 0xA5),
             torch.uint8: (0x5A, 0xA5)}
_BITS = {torch.int16: 16, torch.int32: 32, torch.int8: 8, torch.uint8: 8}


def _signed(v, itype):
    """the pattern as a value of the (signed) integer dtype"""
    bits = _BITS[itype]
    if itype != torch.uint8 and v >= 1 << (bits - 1):
        v -= 1 << bits
    return v


def pattern(dtype, which):
    itype = _INT[dtype]
    return _signed(_PATTERNS[dtype][which], itype)


def fill_pattern(t, which):
    """Fill tensor t (any dtype of _INT, contiguous) with prefill pattern `which` (0 or 1) bit for bit."""
    t.view(_INT[t.dtype]).fill_(pattern(t.dtype, which))
    return t


def worst_row(got, ref, floor=0.1):
    """max over rows r of ||got_r - ref_r|| / max(||ref_r||, floor * RMS row norm), in fp64.
    Returns (value, row index).  A non-finite row counts as infinitely wrong."""
    g = got.double().reshape(got.shape[0], -1)
    r = ref.double().reshape(ref.shape[0], -1).to(g.device)
    assert g.shape == r.shape, (g.shape, r.shape)
    rn = r.norm(dim=1)
    rms = rn.square().mean().sqrt()
    e = (g - r).norm(dim=1) / torch.maximum(rn, floor * rms).clamp_min(1e-300)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    i = int(e.argmax())
    return float(e[i]), i


def rel_l2(got, ref):
    g, r = got.double(), ref.double().to(got.device)
    return float((g - r).norm() / r.norm().clamp_min(1e-30))


def report(case, got, ref, bound, rel_bound=None):
    """rel-L2 and worst row of got against ref (fp64); prints one parseable line and asserts worst row <= bound (0: exact)
    (and rel-L2 < rel_bound when given).  Returns (rel, worst, row)."""
    e = rel_l2(got, ref)
    w, i = worst_row(got, ref)
    print(f"KCHECK {case}: rel-L2 {e:.3e} worst-row {w:.3e} @ row {i} (bound {bound:.1e})")
    if rel_bound is not None:
        assert e < rel_bound, (case, e)
    assert w <= bound, f"{case}: row {i} off by {w:.3e} (bound {bound:.1e}; rel-L2 {e:.3e})"
    return e, w, i


class Guarded:
    """A [rows, width] view with row stride `ld` into a backing buffer of (rows + pad_rows) * ld elements, all of it
    prefilled with pattern `prefill`.  `view` goes to the kernel (pass `ld` as its row stride); check() asserts that every
    element outside the view still holds the pattern."""

    def __init__(self, rows, width, dtype=torch.float16, *, ld=None, pad_rows=256, pad_cols=64, prefill=0, device="cuda"):
        self.rows, self.width, self.dtype = rows, width, dtype
        self.ld = width + pad_cols if ld is None else ld
        assert self.ld >= width
        self.itype = _INT[dtype]
        self.pattern = pattern(dtype, prefill)
        self.buf = torch.empty((rows + pad_rows) * self.ld, dtype=dtype, device=device)
        self.buf.view(self.itype).fill_(self.pattern)
        self.view = self.buf[: rows * self.ld].view(rows, self.ld)[:, :width]

    def check(self, chunk_rows=1 << 16):
        b = self.buf.view(self.itype)
        if self.ld > self.width:
            body = b[: self.rows * self.ld].view(self.rows, self.ld)
            for r0 in range(0, self.rows, chunk_rows):                  # chunked: the side band of a 4 GB buffer is 2 GB of bools at once
                bad = body[r0: r0 + chunk_rows, self.width:] != self.pattern
                if bool(bad.any()):
                    r, c = (int(v) for v in bad.nonzero()[0])
                    raise AssertionError(f"guard: element ({r0 + r}, {self.width + c}) written (width {self.width}, ld {self.ld}); "
                                         f"{int(bad.sum())} such in rows {r0}..{r0 + bad.shape[0] - 1}")
        tail = b[self.rows * self.ld:]
        bad = tail != self.pattern
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f"guard: element ({self.rows + i // self.ld}, {i % self.ld}) past the last row {self.rows - 1} written; "
                                 f"{int(bad.sum())} such")


def assert_same_bits(a, b, what="output"):
    ia, ib = a.view(_INT[a.dtype]), b.view(_INT[b.dtype])
    diff = ia != ib
    if bool(diff.any()):
        idx = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} elements differ between the two prefills, first at {idx} "
                             f"({a[idx].item()} vs {b[idx].item()}): never written, or the kernel reads its own output")


def two_prefills(run, *specs, device="cuda"):
    """specs: (rows, width, dtype, kwargs-for-Guarded) per output.  Calls run(*views, prefill) for prefill 0 and 1, each into
    fresh guarded buffers of that pattern, checks every guard and requires the two runs' outputs to be bit-identical.
    (run gets the prefill index too, so that it can prefill workspaces the same way.)  Returns the first run's Guarded list."""
    runs = []
    for k in (0, 1):
        gs = [Guarded(rows, width, dtype, prefill=k, device=device, **kw) for rows, width, dtype, kw in specs]
        run(*[g.view for g in gs], k)
        if gs[0].buf.is_cuda:
            torch.cuda.synchronize()
        for g in gs:
            g.check()
        runs.append(gs)
    for j, (a, b) in enumerate(zip(*runs)):
        assert_same_bits(a.view, b.view, f"output {j}")
    return runs[0]
