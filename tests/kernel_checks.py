"""Checks shared by the kernel tests (a plain module, imported like conftest.rel_l2).

- worst_row: the largest per-row relative error, so that one wrong row (a ragged last tile, a partial key block, one lane
  group's rescale) is not averaged away by a whole-tensor rel-L2.
- Guarded: an output view inside a larger backing buffer prefilled with a fixed byte pattern; check() asserts that nothing
  outside [0:rows, 0:width] was written (past the last row, or between the width and the row stride).
- two_prefills: the same call into two sets of guarded buffers prefilled with different patterns must give bit-identical
  results -- catches elements that are never written and kernels that read their own output.

- Haloed: the input-side mirror of Guarded -- an operand view inside one larger allocation whose surround (rows before and after,
  columns between the width and the row stride) holds a fill pattern; same_under_halos runs the same call under every fill of
  HALO_FILLS and requires bit-identical outputs: NaN and inf catch 0 * halo, the largest finite value catches a halo element that is
  weighted, zero is what torch.zeros operands give (and must equal the plain, un-haloed call).  The halo is ordinary memory of the
  operand's own allocation: nothing outside it is read.

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


# fp16 bit patterns of an operand's surround: zero, the NaN payload of _PATTERNS, +inf, the largest finite value
HALO_FILLS = {"zero": 0x0000, "nan": _PATTERNS[torch.float16][0], "inf": 0x7C00, "max": 0x7BFF}


class Haloed:
    """`data` (fp16 [rows, width], any device) copied into a view with row stride `ld` of one allocation of
    (pad_before + rows + pad_after) * ld elements; every other element of it holds HALO_FILLS[fill].  `view` goes to the kernel
    (pass `ld` as its row stride); ld and pad_before * ld are multiples of 8 so that the view is 16-byte aligned."""

    def __init__(self, data, *, ld=None, pad_cols=16, pad_before=3, pad_after=5, fill="zero", device=None):
        assert data.dtype == torch.float16 and data.ndim == 2
        rows, width = data.shape
        self.ld = width + pad_cols if ld is None else ld
        assert self.ld >= width and self.ld % 8 == 0, (self.ld, width)
        self.fill = fill
        self.buf = torch.empty((pad_before + rows + pad_after) * self.ld, dtype=torch.float16, device=device or data.device)
        self.buf.view(torch.int16).fill_(_signed(HALO_FILLS[fill], torch.int16))
        self.view = self.buf[pad_before * self.ld: (pad_before + rows) * self.ld].view(rows, self.ld)[:, :width]
        self.view.copy_(data)


def same_under_halos(run, operands, plain=None, fills=tuple(HALO_FILLS), device=None):
    """operands: (fp16 [rows, width] data, kwargs-for-Haloed) per input.  Calls run(*haloed) -- each argument a Haloed, whose .view and
    .ld go to the kernel -- once per fill; run returns the output tensor.  Every output must equal the first fill's bit for bit, and
    `plain` (the output of the un-haloed call) when given.  Returns the first output."""
    first = None
    for fill in fills:
        out = run(*[Haloed(d, fill=fill, device=device, **kw) for d, kw in operands])
        if out.is_cuda:
            torch.cuda.synchronize()
        out = out.clone()
        if first is None:
            first, first_fill = out, fill
            if plain is not None:
                _assert_halo_bits(plain, out, f"the un-haloed call vs the '{fill}' halo")
        else:
            _assert_halo_bits(first, out, f"halo fill '{first_fill}' vs '{fill}'")
    return first


def _assert_halo_bits(a, b, what):
    diff = a.view(_INT[a.dtype]) != b.view(_INT[b.dtype])
    if bool(diff.any()):
        idx = tuple(int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"halo: {what}: {int(diff.sum())} output elements differ, first at {idx} ({a[idx].item()} vs {b[idx].item()}): "
                             f"an element outside the operand reached the result")


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
