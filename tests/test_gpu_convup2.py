"""-m gpu: ew_gemm_f16's upsample=2 form -- the 3x3 conv over a nearest-x2 upsampled image as four 2x2 phase convs over the source image
(gemm3_kernel<3, 17>, weights from ops.pack_convup2_weight) -- against its twin, the upsample=1 call on the same inputs and the nine taps.

- exact agreement: integer inputs in [-4, 4], weights k/64 with k in [-8, 8], bias k/8: every product, every phase sum of taps and every partial
  sum is exact in fp32 (and the phase sums in fp16), so both forms accumulate the same numbers in any order: hi and lo8 planes bit-equal;
- random fp16 data: against fp64 with the same rounded phase weights the split output sits under the split-output bound of the 3x3 conv tests
  (tests/test_gpu_gemm_gen3.py: rel-L2 2e-5 -- fp32 accumulation and the 19-bit output, nothing else), the hi plane alone under their 1e-3;
  against fp64 with the unrounded fp32 weights the rel-L2 is at most 1.10 x the twin's on the same inputs (one rounding of a tap sum instead
  of nine rounded taps: expectation 1, tests/test_cpu_convup2_pack.py);
- guards: both output planes lie between poisoned bands (rows before and after, columns up to the row stride) and are prefilled twice with
  different patterns: the planes agree bit for bit, so every element is written and none is read, and the bands are untouched.  With the exact
  data each output row has one value whichever phase tile writes it, so "bit-equal to the twin" is "every row written with its own result";
- refusals: stride 2, conv_shift, a second source, h_out != 2 h_in, an N the predicate rejects: error status, no launch, output untouched.

Shapes (n_img, h x w source, C -> N): (2, 5x7, 64 -> 320) one ragged tile per phase, all four borders and the image seam inside the tile;
(2, 13x17, 128 -> 640) two K chunks, two tile columns, two tiles per phase; (3, 16x24, 64 -> 320) on a CU budget of 8: 20 tiles on 8
workgroups = one whole-tile round, then 12 tiles as a stream-K tail cut inside tiles (nk = 4, 6 K-tiles per workgroup).  (The budget is 8 and
not 3: ew_set_cu_budget takes multiples of 8 and ignores anything else, and an ignored budget would run the 20 tiles as one round.)"""
import math

import pytest
import torch
import torch.nn.functional as F

from kernel_checks import _INT, fill_pattern, pattern

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEW, PAD_ROWS, PAD_COLS = "gemm3_kernel<3, 17>", 64, 8


@pytest.fixture(scope="module")
def ops():
    from evoworld_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from evoworld_amd import _lib
    return _lib.load()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def operands(ops, n, h, w, C, N, exact):
    """x [n, C, h, w] (fp16-exact), w32 [N, C, 3, 3] fp32, bias fp16 -> device operands of both forms"""
    if exact:
        x = torch.randint(-4, 5, (n, C, h, w), generator=gen(1)).float()
        w32 = torch.randint(-8, 9, (N, C, 3, 3), generator=gen(2)).float() / 64
        b = torch.randint(-8, 9, (N,), generator=gen(3)).float() / 8
    else:
        x = torch.randn(n, C, h, w, generator=gen(1)).half().float()
        w32 = torch.randn(N, C, 3, 3, generator=gen(2)) / math.sqrt(9 * C)
        b = torch.randn(N, generator=gen(3)).half().float()
    a = x.permute(0, 2, 3, 1).reshape(-1, C).half().contiguous().to(DEV)
    return x, w32, b, a, ops.pack_conv_weight(w32).to(DEV), ops.pack_convup2_weight(w32).to(DEV), b.half().to(DEV)


class Banded:
    """[rows, width] view with row stride width + PAD_COLS, PAD_ROWS rows of the backing buffer before and after it, everything prefilled"""

    def __init__(self, rows, width, dtype, which):
        self.ld = width + PAD_COLS
        self.buf = fill_pattern(torch.empty((rows + 2 * PAD_ROWS) * self.ld, dtype=dtype, device=DEV), which)
        self.pat, self.rows, self.width = pattern(dtype, which), rows, width
        self.view = self.buf[PAD_ROWS * self.ld: (PAD_ROWS + rows) * self.ld].view(rows, self.ld)[:, :width]

    def check(self):
        b = self.buf.view(_INT[self.buf.dtype]).view(-1, self.ld)
        assert bool((b[:PAD_ROWS] == self.pat).all()), "rows before the output written"
        assert bool((b[PAD_ROWS + self.rows:] == self.pat).all()), "rows after the output written"
        assert bool((b[PAD_ROWS: PAD_ROWS + self.rows, self.width:] == self.pat).all()), "columns between the width and the row stride written"


def run_planes(ops, lib, a, wp, bias, n, h, w, C, N, up, want=None):
    """one launch of form `up` into banded, twice-prefilled hi / lo8 planes -> (hi, lo) of the first prefill"""
    M = n * 4 * h * w
    outs = []
    for which in (0, 1):
        hi, lo = Banded(M, N, torch.float16, which), Banded(M, N, torch.int8, which)
        ops.gemm(a, wp, ops.Res(hi.view, lo.view), M=M, N=N, c1=C, lda=C, bias=bias, mode=ops.A_CONV3X3, conv=(n, h, w, 2 * h, 2 * w, 1, up), ld_out=hi.ld)
        torch.cuda.synchronize()
        if want is not None:
            assert lib.ew_gemm_last_kernel().decode() == want
        hi.check()
        lo.check()
        outs.append((hi.view, lo.view))
    for p0, p1 in zip(*outs):
        assert torch.equal(p0.contiguous().view(_INT[p0.dtype]), p1.contiguous().view(_INT[p1.dtype])), "the two prefills differ: an element never written, or read"
    return outs[0]


def ref64(x, w_nine):
    """fp64 conv2d(interpolate(x, 2, nearest), w, padding=1) -> [n * 2h * 2w, N] rows in NHWC order, on the device"""
    y = F.conv2d(F.interpolate(x.double().to(DEV), scale_factor=2.0, mode="nearest"), w_nine.double().to(DEV), padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def ref64_phases(x, pack, N):
    """fp64 result of the four-phase form from the fp16 pack [4 N, 4 C] (layout: include/evoworld_hip.h) -> [n * 2h * 2w, N]"""
    n, C, h, w = x.shape
    wt = pack.double().reshape(4, N, C // 64, 4, 64).permute(0, 3, 1, 2, 4).reshape(4, 4, N, C)
    xp = F.pad(x.double().to(DEV), (1, 1, 1, 1))
    out = torch.zeros(n, N, 2 * h, 2 * w, dtype=torch.float64, device=DEV)
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        for t in range(4):
            r, c = t >> 1, t & 1
            out[:, :, a::2, b::2] += torch.einsum("oc,nchw->nohw", wt[ph, t], xp[:, :, a + r: a + r + h, b + c: b + c + w])
    return out.permute(0, 2, 3, 1).reshape(-1, N)


def rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm())


CASES = [(2, 5, 7, 64, 320, None), (2, 13, 17, 128, 640, None), (3, 16, 24, 64, 320, 8)]


@pytest.mark.parametrize("n,h,w,C,N,budget", CASES, ids=["ragged-5x7", "2chunks-2cols-13x17", "rounds-and-tail-16x24"])
def test_exact_data_bit_equal_to_the_nine_tap_twin(ops, lib, n, h, w, C, N, budget):
    _, _, _, a, w9, w4, bias = operands(ops, n, h, w, C, N, exact=True)
    before = lib.ew_get_cu_budget()
    try:
        if budget is not None:
            lib.ew_set_cu_budget(budget)
            assert lib.ew_get_cu_budget() == budget
        new_hi, new_lo = run_planes(ops, lib, a, w4, bias, n, h, w, C, N, up=2, want=NEW)
    finally:
        lib.ew_set_cu_budget(before)
    # plain fp16 output (no lo8 plane: the fp16 residual stream) is the hi plane of the split one
    plain = torch.empty(n * 4 * h * w, N, dtype=torch.float16, device=DEV)
    ops.gemm(a, w4, plain, M=plain.shape[0], N=N, c1=C, lda=C, bias=bias, mode=ops.A_CONV3X3, conv=(n, h, w, 2 * h, 2 * w, 1, 2))
    assert lib.ew_gemm_last_kernel().decode() == NEW and torch.equal(plain, new_hi)
    twin_hi, twin_lo = run_planes(ops, lib, a, w9, bias, n, h, w, C, N, up=1)
    assert float(twin_hi.float().abs().max()) > 1.0
    bad = (new_hi != twin_hi).any(1) | (new_lo != twin_lo).any(1)
    assert not bool(bad.any()), f"{int(bad.sum())} output rows differ from the twin, first {int(bad.nonzero()[0])}"
    assert lib.ew_gemm_streamk_status() == 0


def test_random_data_against_fp64_and_the_twin(ops, lib):
    n, h, w, C, N = 2, 13, 17, 128, 640
    x, w32, b, a, w9, w4, bias = operands(ops, n, h, w, C, N, exact=False)
    new = ops.Res(*run_planes(ops, lib, a, w4, bias, n, h, w, C, N, up=2, want=NEW))
    twin = ops.Res(*run_planes(ops, lib, a, w9, bias, n, h, w, C, N, up=1))
    bd = b.double().to(DEV)
    same_w = ref64_phases(x, w4, N) + bd
    e_split, e_hi = rel_l2(new.float(), same_w), rel_l2(new.hi.float(), same_w)
    print(f"upsample=2 vs fp64 on the same rounded phase weights: split output rel-L2 {e_split:.3e}, hi plane {e_hi:.3e}")
    assert e_split < 2e-5 and e_hi < 1e-3
    exact_w = ref64(x, w32) + bd
    e_new, e_twin = rel_l2(new.float(), exact_w), rel_l2(twin.float(), exact_w)
    print(f"vs fp64 on the fp32 weights: upsample=2 rel-L2 {e_new:.3e}, nine-tap twin {e_twin:.3e}, ratio {e_new / e_twin:.3f}")
    assert e_new <= 1.10 * e_twin


@pytest.mark.parametrize("what", ["stride2", "conv_shift", "a2", "h_out", "N"])
def test_refusals_launch_nothing(ops, lib, what):
    from evoworld_amd import _lib
    n, h, w, C, N = 1, 6, 8, 64, 320
    if what == "N":
        N = 256
        assert not ops.convup2_ok(N, C) and ops.convup2_ok(320, C) and not ops.convup2_ok(320, 96)
    M = n * 4 * h * w
    a = torch.zeros(n * h * w, C, dtype=torch.float16, device=DEV)
    wp = torch.zeros(4 * N, 4 * C, dtype=torch.float16, device=DEV)
    out = fill_pattern(torch.empty(M, N, dtype=torch.float16, device=DEV), 1)
    kw = dict(M=M, N=N, c1=C, lda=C, mode=ops.A_CONV3X3, conv=(n, h, w, 2 * h, 2 * w, 1, 2))
    if what == "stride2":
        kw["conv"] = (n, h, w, 2 * h, 2 * w, 2, 2)
    elif what == "conv_shift":
        kw["conv_shift"] = 1
    elif what == "a2":
        kw.update(a2=a, c2=C, lda2=C)
    elif what == "h_out":
        kw.update(M=n * (2 * h - 1) * 2 * w, conv=(n, h, w, 2 * h - 1, 2 * w, 1, 2))
    ops.linear(torch.zeros(8, 64, dtype=torch.float16, device=DEV), torch.zeros(8, 64, dtype=torch.float16, device=DEV))      # a launch to tell from
    last = lib.ew_gemm_last_kernel()
    with pytest.raises(_lib.EvoWorldHipError):
        ops.gemm(a, wp, out, **kw)
    torch.cuda.synchronize()
    assert lib.ew_gemm_last_kernel() == last
    assert bool((out.view(torch.int16) == pattern(torch.float16, 1)).all())
