"""The checks of tests/kernel_checks.py catch what they claim (CPU only: the "kernels" here are Python writes)."""
import pytest
import torch

from conftest import rel_l2
from kernel_checks import HALO_FILLS, Guarded, Haloed, fill_pattern, same_under_halos, two_prefills, worst_row


def test_worst_row_flags_one_row_that_rel_l2_misses():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(51237, 320, generator=g, dtype=torch.float64)
    got = ref * (1 + 3e-4 * torch.randn(51237, 320, generator=g, dtype=torch.float64))      # fp16-like background noise
    got[40000] *= 1.005                                                                      # one row 0.5 % off
    assert rel_l2(got, ref) < 1e-3                                                           # the whole-tensor norm does not see it
    w, i = worst_row(got, ref)
    assert i == 40000 and w > 4e-3
    w0, _ = worst_row(ref * (1 + 3e-4 * torch.randn(51237, 320, generator=g, dtype=torch.float64)), ref)
    assert w0 < 1e-3


def test_worst_row_floor_and_non_finite():
    ref = torch.ones(4, 8, dtype=torch.float64)
    ref[2] = 0.0                                         # a zero reference row: error relative to 0.1 x RMS row norm
    got = ref.clone()
    got[2, 0] = 1e-3
    w, i = worst_row(got, ref)
    assert i == 2 and abs(w - 1e-3 / (0.1 * (3 * 8 / 4) ** 0.5)) < 1e-12
    got[1, 3] = float("nan")
    assert worst_row(got, ref) == (float("inf"), 1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.int8, torch.uint8])
@pytest.mark.parametrize("where", ["pad_col", "pad_row", "last_byte"])
def test_guard_flags_one_byte_outside(dtype, where):
    g = Guarded(37, 20, dtype, pad_rows=5, pad_cols=8, device="cpu")
    g.view.view(torch.uint8 if dtype.itemsize == 1 else dtype).zero_()    # a well-behaved kernel: writes the whole view
    g.check()
    raw = g.buf.view(torch.uint8)                                          # one BYTE flipped in the padding
    esz = dtype.itemsize
    off = {"pad_col": (36 * g.ld + 20) * esz + esz - 1, "pad_row": (37 * g.ld + 3) * esz, "last_byte": raw.numel() - 1}[where]
    raw[off] ^= 0x01
    with pytest.raises(AssertionError, match="guard"):
        g.check()


def test_guard_nan_pattern_compares_by_bits():
    g = Guarded(3, 4, torch.float16, pad_rows=1, pad_cols=4, prefill=0, device="cpu")
    assert torch.isnan(g.buf).all()                       # the fp16 prefill is a NaN payload ...
    g.check()                                             # ... and still passes: the comparison is on integers
    g.buf.view(torch.int16)[-1] = 0x7E00                  # another NaN is a different payload
    with pytest.raises(AssertionError, match="guard"):
        g.check()


def test_two_prefills_flags_one_element_left_unwritten():
    def good(o, lo, k):
        o.copy_(torch.arange(o.numel(), dtype=torch.float32).reshape(o.shape).half())
        lo.fill_(3)

    def skips_one(o, lo, k):
        keep = o[99, 7].clone()                           # element (99, 7) keeps the prefill
        good(o, lo, k)
        o[99, 7] = keep

    specs = [(100, 16, torch.float16, dict(pad_rows=4, pad_cols=8)), (100, 16, torch.int8, dict(pad_rows=4, pad_cols=8))]
    two_prefills(good, *specs, device="cpu")
    with pytest.raises(AssertionError, match="differ between the two prefills"):
        two_prefills(skips_one, *specs, device="cpu")

    def lo_unwritten(o, lo, k):
        good(o, lo, k)
        lo[0, 0] = 0x5A if k == 0 else -0x5B             # 0x5A / 0xA5: the two int8 prefills
    with pytest.raises(AssertionError, match="output 1"):
        two_prefills(lo_unwritten, *specs, device="cpu")


def test_two_prefills_flags_a_kernel_that_reads_its_output():
    def accumulates(o, k):
        o += 1.0                                          # reads what is there: NaN under one prefill, 203.25 under the other
    with pytest.raises(AssertionError, match="differ"):
        two_prefills(accumulates, (8, 8, torch.float16, dict(pad_rows=1)), device="cpu")


def _emulated(reach):
    """a row-sum 'kernel' over a Haloed [rows, width] operand that also touches one element outside it"""
    def run(x):
        rows, width = x.view.shape
        off = x.view.storage_offset()
        wide = x.buf.as_strided((rows + 2, x.ld), (x.ld, 1), off - x.ld).float()      # the view with one row before and one after
        out = wide[1:-1, :width].sum(dim=1)
        if reach == "column":
            out = out + wide[1:-1, width]                 # the column just past the width
        elif reach == "row_after_x0":
            out[-1] = out[-1] + 0.0 * wide[-1, 0]         # the row after the last, weight zero ("never consumed")
        elif reach == "row_before":
            out[0] = out[0] + wide[0, 2]
        return out
    return run


def test_halo_fills_and_layout():
    data = torch.arange(5 * 24, dtype=torch.float32).reshape(5, 24).half()
    for fill, bits in HALO_FILLS.items():
        h = Haloed(data, pad_cols=8, pad_before=2, pad_after=3, fill=fill)
        assert h.ld == 32 and h.view.data_ptr() % 16 == h.buf.data_ptr() % 16 and torch.equal(h.view, data)
        surround = torch.ones(10, 32, dtype=torch.bool)
        surround[2:7, :24] = False
        assert (h.buf.view(torch.int16).view(10, 32)[surround] == (bits if bits < 0x8000 else bits - 0x10000)).all()
    assert torch.isnan(Haloed(data, fill="nan").buf[0]) and torch.isinf(Haloed(data, fill="inf").buf[0])
    assert Haloed(data, fill="max").buf[0] == 65504.0


def test_same_under_halos_catches_reads_outside_the_operand():
    data = torch.randn(9, 24, generator=torch.Generator().manual_seed(0)).half()
    ops = [(data, dict(pad_cols=8))]
    plain = data.float().sum(dim=1)
    assert torch.equal(same_under_halos(_emulated("none"), ops, plain=plain), plain)
    with pytest.raises(AssertionError, match="halo"):
        same_under_halos(_emulated("column"), ops)
    with pytest.raises(AssertionError, match="halo"):
        same_under_halos(_emulated("row_before"), ops)
    # weight zero: 0 * NaN and 0 * inf are NaN, 0 * 65504 is 0 -- the finite fill alone does not see it
    same_under_halos(_emulated("row_after_x0"), ops, plain=plain, fills=("zero", "max"))
    with pytest.raises(AssertionError, match="'zero' vs 'nan'"):
        same_under_halos(_emulated("row_after_x0"), ops, plain=plain, fills=("zero", "nan"))
    with pytest.raises(AssertionError, match="'zero' vs 'inf'"):
        same_under_halos(_emulated("row_after_x0"), ops, plain=plain, fills=("zero", "inf"))
    # ... and a weighted element is seen by the finite fill alone, too
    with pytest.raises(AssertionError, match="'zero' vs 'max'"):
        same_under_halos(_emulated("column"), ops, fills=("zero", "max"))
    # the result under the zero halo is held to the plain, un-haloed call
    with pytest.raises(AssertionError, match="un-haloed"):
        same_under_halos(_emulated("none"), ops, plain=plain + 1.0, fills=("zero",))


def test_fill_pattern_workspace():
    ws = torch.empty(100, dtype=torch.float32)
    assert torch.isnan(fill_pattern(ws, 0)).all()
    assert (fill_pattern(ws, 1).view(torch.int32) == 0x5A5A5A5A).all()
