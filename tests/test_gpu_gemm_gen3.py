"""-m gpu: the generation-3 GEMM (256x320 tile; taken when N % 320 == 0 and the problem fills the chip) against a plain
PyTorch fp32 reference AND against the independent generation-1 kernels, on problems large enough to be routed to it:
ragged M (edge tiles), every epilogue operand set that occurs in the U-Net, all three A addressing modes (dense, conv3x3 with
stride / upsample / dual source, temporal 3-tap).  Most cases here are sized to about 200 tiles on 256 workgroups, one tile per
workgroup, and the stream-K test compares the kernel with its own whole-tile twin: generation 3's chained tiles (multi-round
schedules, banded order, stream-K tail then data-parallel tile) are covered by test_gpu_gemm_gen3_rounds.py against fp64, generation 1
and single-round pieces.  test_gpu_ops.py's GEMM cases are small and run on generation 2, at most one tile per workgroup;
generation 2's multi-round schedules are covered by test_gpu_gemm_gen2.py.  The helpers shared with those files (guarded, the fp64
conv references) live in gemm_cases.py."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from gemm_cases import _nhwc, _pack3, conv3x3_ref64, convt3_ref64, gen3_plan, guarded, guarded_planes
from kernel_checks import report
from vae_cases import denormal_fraction, softmax_rows_f16

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def ops():
    from evoworld_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from evoworld_amd import _lib
    L = _lib.load()
    yield L
    L.ew_set_gemm_generation(3)


# worst-row bounds per case: (bound, value measured on an MI355X); the bound is at most 2x the measurement
WORST_ROW = {
    'conv small-N 7x64+0->4 24x40 ld+8': (0.00092, 0.000465),  # measured worst row; rel-L2 0.000207 row 774
    'conv small-N 7x64+0->4 24x40 ld+8 (gen-b)': (0.00092, 0.000465),  # measured worst row; rel-L2 0.000207 row 774
    'conv small-N 5x128+64->4 36x64 ld+8': (0.00091, 0.000456),  # measured worst row; rel-L2 0.000207 row 2471
    'conv small-N 5x128+64->4 36x64 ld+8 (gen-b)': (0.00091, 0.000456),  # measured worst row; rel-L2 0.000207 row 2471
    'conv small-N 3x192+0->8 40x48 ld+8': (0.00082, 0.000411),  # measured worst row; rel-L2 0.000207 row 1094
    'conv small-N 3x192+0->8 40x48 ld+8 (gen-b)': (0.00082, 0.000411),  # measured worst row; rel-L2 0.000207 row 1094
    'conv small-N 2x64+64->16 72x128 ld+64': (0.00079, 0.000398),  # measured worst row; rel-L2 0.000207 row 9099
    'conv small-N 2x64+64->16 72x128 ld+64 (gen-b)': (0.00079, 0.000398),  # measured worst row; rel-L2 0.000207 row 9099
    'conv small-N 4x64+0->12 30x41 ld+64': (0.00071, 0.00036),  # measured worst row; rel-L2 0.000207 row 992
    'conv small-N 4x64+0->12 30x41 ld+64 (gen-b)': (0.00071, 0.00036),  # measured worst row; rel-L2 0.000207 row 992
    'dense 51237x320x320 bias ld+8': (0.0005, 0.000251),  # measured worst row; rel-L2 0.000208 row 21735
    'dense 51237x320x320 bias ld+8 (gen-b)': (0.0005, 0.000251),  # measured worst row; rel-L2 0.000208 row 21735
    'dense 26011x640x192 rb+r1 ld+8': (0.00047, 0.000238),  # measured worst row; rel-L2 0.000207 row 7924
    'dense 26011x640x192 rb+r1 ld+8 (gen-b)': (0.00047, 0.000238),  # measured worst row; rel-L2 0.000207 row 7924
    'dense 26000x640x128 r1+r2 ld+64': (0.00048, 0.000242),  # measured worst row; rel-L2 0.000208 row 4391
    'dense 26000x640x128 r1+r2 ld+64 (gen-b)': (0.00048, 0.000242),  # measured worst row; rel-L2 0.000208 row 4391
    'dense 51456x320x64 silu ld+64': (0.00055, 0.000277),  # measured worst row; rel-L2 0.000208 row 26217
    'dense 51456x320x64 silu ld+64 (gen-b)': (0.00055, 0.000277),  # measured worst row; rel-L2 0.000208 row 26217
    'dense 25700x640x448 rb ld+64': (0.00047, 0.000237),  # measured worst row; rel-L2 0.000208 row 24161
    'dense 25700x640x448 rb ld+64 (gen-b)': (0.00047, 0.000237),  # measured worst row; rel-L2 0.000208 row 24161
    'dense 30000x960x64 rb+r1+r2 ld+64': (0.00046, 0.000232),  # measured worst row; rel-L2 0.000208 row 28722
    'dense 30000x960x64 rb+r1+r2 ld+64 (gen-b)': (0.00046, 0.000232),  # measured worst row; rel-L2 0.000208 row 28722
    'dense 51237x320x320 gelu ld+8': (0.00056, 0.00028),  # measured worst row; rel-L2 0.000208 row 18026
    'dense 51237x320x320 gelu ld+8 (gen-b)': (0.00056, 0.00028),  # measured worst row; rel-L2 0.000208 row 18026
    'dense 26011x640x192 split ld+8': (1.9e-06, 9.53e-07),  # measured worst row; rel-L2 8.23e-07 row 441
    'dense 26011x640x192 split ld+8 (gen-b)': (1.9e-06, 9.51e-07),  # measured worst row; rel-L2 8.2e-07 row 441
    'dense 6500x2560x640 bias ld+64': (0.00044, 0.000222),  # measured worst row; rel-L2 0.000208 row 668
    'dense 6500x2560x640 bias ld+64 (gen-b)': (0.00044, 0.000222),  # measured worst row; rel-L2 0.000208 row 668
    'dense 8811x1920x1024 r1 ld+8': (0.00044, 0.000223),  # measured worst row; rel-L2 0.000208 row 3630
    'dense 8811x1920x1024 r1 ld+8 (gen-b)': (0.00044, 0.000223),  # measured worst row; rel-L2 0.000208 row 3630
    'dense 320x32000x320 bias ld+64': (0.00042, 0.000211),  # measured worst row; rel-L2 0.000208 row 38
    'dense 320x32000x320 bias ld+64 (gen-b)': (0.00042, 0.000211),  # measured worst row; rel-L2 0.000208 row 38
    'geglu 25700x640x128 ld+8': (0.00073, 0.000368),  # measured worst row; rel-L2 0.000208 row 20259
    'geglu 25700x640x128 ld+8 (gen-b)': (0.00073, 0.000368),  # measured worst row; rel-L2 0.000207 row 20259
    'geglu 25701x640x128 ld+64': (0.00073, 0.000368),  # measured worst row; rel-L2 0.000208 row 20259
    'geglu 25701x640x128 ld+64 (gen-b)': (0.00073, 0.000368),  # measured worst row; rel-L2 0.000207 row 20259
    'conv3x3 13x64+0->320 61x65 s1 up0 rb ld+8': (0.00049, 0.000248),  # measured worst row; rel-L2 0.000207 row 30016
    'conv3x3 13x64+0->320 61x65 s1 up0 rb ld+8 (gen-b)': (0.00049, 0.000248),  # measured worst row; rel-L2 0.000207 row 30016
    'conv3x3 7x64+64->320 44x170 s1 up0 r1 ld+8': (0.0005, 0.000252),  # measured worst row; rel-L2 0.000207 row 5664
    'conv3x3 7x64+64->320 44x170 s1 up0 r1 ld+8 (gen-b)': (0.0005, 0.000252),  # measured worst row; rel-L2 0.000207 row 5664
    'conv3x3 5x64+0->320 50x52 s1 up1 bias ld+8': (0.0005, 0.000251),  # measured worst row; rel-L2 0.000207 row 26203
    'conv3x3 5x64+0->320 50x52 s1 up1 bias ld+8 (gen-b)': (0.0005, 0.000251),  # measured worst row; rel-L2 0.000207 row 26203
    'conv3x3 20x128+0->640 74x70 s2 up0 bias ld+64': (0.00047, 0.000238),  # measured worst row; rel-L2 0.000207 row 9661
    'conv3x3 20x128+0->640 74x70 s2 up0 bias ld+64 (gen-b)': (0.00047, 0.000238),  # measured worst row; rel-L2 0.000207 row 9661
    'conv temporal 2x25x1031 64->320 r1 ld+8': (0.00051, 0.000255),  # measured worst row; rel-L2 0.000208 row 18641
    'conv temporal 2x25x1031 64->320 r1 ld+8 (gen-b)': (0.00051, 0.000255),  # measured worst row; rel-L2 0.000208 row 18641
    'conv temporal 2x25x1031 64->320 r1 ld+64': (0.00051, 0.000255),  # measured worst row; rel-L2 0.000208 row 18641
    'conv temporal 2x25x1031 64->320 r1 ld+64 (gen-b)': (0.00051, 0.000255),  # measured worst row; rel-L2 0.000208 row 18641
    'stream-K dense_res ld+64': (1.8e-06, 9.5e-07),  # measured worst row; rel-L2 8.18e-07 row 28293
    'stream-K dense_k320 ld+8': (0.00047, 0.000237),  # measured worst row; rel-L2 0.000209 row 109435
    'stream-K half_dense ld+64': (1.8e-06, 9.04e-07),  # measured worst row; rel-L2 8.35e-07 row 1013
    # the 256-wide instance on the half split: (bound, worst row of GENERATION 1 against fp64 measured on an MI355X), bound = 2 x that
    # measurement rounded down to two digits, applied to generation 3, generation 2 and generation 1 (test_gpu_gemm_gen3_rounds.py's rule)
    'stream-K half_b256_min M=1024 ld+64': (1.8e-06, 9.123e-07),  # generation 1 vs fp64: rel-L2 8.15e-07, worst row 459
    'stream-K half_b256_min M=1000 ld+8': (1.8e-06, 9.127e-07),  # generation 1 vs fp64: rel-L2 8.16e-07, worst row 740
    'stream-K half_b256_attn M=9216 ld+64': (0.00047, 0.0002392),  # generation 1 vs fp64: rel-L2 2.07e-04, worst row 2536
    'b256 dense 61237x256x320 bias ld+8': (0.00051, 0.000259),  # measured worst row; rel-L2 0.000208 row 21735
    'b256 dense 61237x256x320 bias ld+8 (gen-b)': (0.00051, 0.000259),  # measured worst row; rel-L2 0.000208 row 21735
    'b256 dense 52011x512x192 rb+r1 ld+8': (0.00048, 0.000243),  # measured worst row; rel-L2 0.000207 row 30010
    'b256 dense 52011x512x192 rb+r1 ld+8 (gen-b)': (0.00048, 0.000243),  # measured worst row; rel-L2 0.000207 row 30010
    'b256 dense 70000x256x1920 r1+r2 ld+64': (0.00051, 0.000256),  # measured worst row; rel-L2 0.000208 row 11743
    'b256 dense 70000x256x1920 r1+r2 ld+64 (gen-b)': (0.00051, 0.000256),  # measured worst row; rel-L2 0.000208 row 11743
    'b256 dense 51456x512x64 silu ld+64': (0.00052, 0.000262),  # measured worst row; rel-L2 0.000208 row 29571
    'b256 dense 51456x512x64 silu ld+64 (gen-b)': (0.00052, 0.000262),  # measured worst row; rel-L2 0.000208 row 29571
    'b256 dense 26000x1024x448 split ld+64': (1.8e-06, 9.35e-07),  # measured worst row; rel-L2 8.3e-07 row 1361
    'b256 dense 26000x1024x448 split ld+64 (gen-b)': (1.8e-06, 9.34e-07),  # measured worst row; rel-L2 8.23e-07 row 1361
    'b256 dense 140000x256x2304 split ld+64': (2.4e-06, 1.24e-06),  # measured worst row; rel-L2 8.66e-07 row 39877
    'b256 dense 140000x256x2304 split ld+64 (gen-b)': (2.3e-06, 1.2e-06),  # measured worst row; rel-L2 8.39e-07 row 39877
    'b256 conv3x3 256->256 96x128 plain ld+8': (0.00053, 0.000266),  # measured worst row; rel-L2 0.000207 row 36312
    'b256 conv3x3 256->256 96x128 plain ld+8 (gen-b)': (0.00053, 0.000266),  # measured worst row; rel-L2 0.000207 row 36312
    'b256 conv3x3 512->512 96x128 res ld+64': (0.00048, 0.000241),  # measured worst row; rel-L2 0.000207 row 39027
    'b256 conv3x3 512->512 96x128 res ld+64 (gen-b)': (0.00048, 0.000241),  # measured worst row; rel-L2 0.000207 row 39027
    'b256 conv3x3 512->256 96x128 up ld+64': (0.00052, 0.000263),  # measured worst row; rel-L2 0.000207 row 128238
    'b256 conv3x3 512->256 96x128 up ld+64 (gen-b)': (0.00052, 0.000263),  # measured worst row; rel-L2 0.000207 row 128238
    'b256 conv3x3 128->256 192x256 shift ld+8': (0.00052, 0.000261),  # measured worst row; rel-L2 0.000207 row 67241
    'b256 conv3x3 128->256 192x256 shift ld+8 (gen-b)': (0.00052, 0.000261),  # measured worst row; rel-L2 0.000207 row 67241
    '32-bit edge M=524287 ld_out=4096': (0.00048, 0.000244),  # measured worst row; rel-L2 0.000207 row 189
    '32-bit edge M=524289 ld_out=4096': (0.00048, 0.000244),  # measured worst row; rel-L2 0.000207 row 189
}


def both(lib, run, M, n_out, ld_pad, split=False, want3="gemm3_kernel", gen_b=1, want_b="gemm_kernel"):
    """run(out, ld_out) under generation 3 (asserting that `want3` took the problem) and under generation `gen_b`, each into its
    own guarded, twice-prefilled output (a tile one generation skips cannot inherit the other's values)."""
    return (guarded(lib, 3, want3, run, M, n_out, ld_pad, split), guarded(lib, gen_b, want_b, run, M, n_out, ld_pad, split))


def check_both(case, g3, gb, ref, rel_bound):
    """generation 3 and the comparison generation each against the fp64 reference: rel-L2 and worst row"""
    report(case, g3, ref, WORST_ROW[case][0], rel_bound)
    report(case + " (gen-b)", gb, ref, WORST_ROW[case + " (gen-b)"][0], rel_bound)


@pytest.mark.parametrize("M,N,K,eps", [(51237, 320, 320, "bias"), (26011, 640, 192, "rb+r1"), (26000, 640, 128, "r1+r2"),
                                               (51456, 320, 64, "silu"), (25700, 640, 448, "rb"), (30000, 960, 64, "rb+r1+r2"),
                                               (51237, 320, 320, "gelu"), (26011, 640, 192, "split"),
                                               # weight matrix > 3 MB: banded tile order (8 tile columns = 2 bands; 6 = one full + one ragged band)
                                               (6500, 2560, 640, "bias"), (8811, 1920, 1024, "r1"),
                                               # round 4: M = C (the swapped-operand V^T projections: W_v rows against all tokens), ragged second row tile
                                               (320, 32000, 320, "bias")])
def test_dense_epilogues(ops, lib, M, N, K, eps):
    ld_pad = 8 if M % 2 else 64                         # ld_out = N + 8 or N + 64
    x, w, b = rnd(M, K, seed=1).half().to(DEV), (rnd(N, K, seed=2) / math.sqrt(K)).half().to(DEV), rnd(N, seed=3).half().to(DEV)
    rpg = 7001
    G = M // rpg + 1
    split = eps == "split"
    rb = rnd(G, N + 64, seed=4).half().to(DEV) if "rb" in eps else None
    r1 = rnd(M, N, seed=5).half().to(DEV) if "r1" in eps else (ops.Res.from_float(rnd(M, N, seed=5).to(DEV)) if split else None)
    r2 = rnd(M, N + 8, seed=6).half().to(DEV) if "r2" in eps else None
    act = {"silu": ops.ACT_SILU, "gelu": ops.ACT_GELU}.get(eps, ops.ACT_NONE)

    def run(out, ld_out):
        ops.gemm(x, w, out, M=M, N=N, c1=K, lda=K, bias=b, rowbias=None if rb is None else rb[:, 64:], ld_rowbias=N + 64,
                 rows_per_group=rpg, r1=r1, ld_r1=N, r2=r2, ld_r2=N + 8, act=act, c_acc=0.7, c_r1=0.6, c_r2=-1.5, ld_out=ld_out)
    g3, g1 = both(lib, run, M, N, ld_pad, split=split)
    y = x.double() @ w.double().T + b.double()
    if rb is not None:
        y = y + rb[:, 64:].double()[torch.arange(M, device=DEV) // rpg]
    if act == ops.ACT_SILU:
        y = F.silu(y)
    if act == ops.ACT_GELU:
        y = F.gelu(y)
    y = 0.7 * y
    if r1 is not None:
        y = y + 0.6 * r1.float().double()
    if r2 is not None:
        y = y - 1.5 * r2[:, :N].double()
    check_both(f"dense {M}x{N}x{K} {eps} ld+{ld_pad}", g3, g1, y, 2e-5 if split else 1e-3)
    assert rel_l2(g3.cpu(), g1.cpu()) < (2e-5 if split else 1e-3)


def test_geglu(ops, lib):
    for M, ld_pad in ((25700, 8), (25701, 64)):       # ld_out = N/2 + 8, N/2 + 64
        _geglu_case(ops, lib, M, ld_pad)


def _geglu_case(ops, lib, M, ld_pad):
    C = 80                                               # N = 8C = 640
    x = rnd(M, C, seed=1).half().to(DEV)
    w, b = (rnd(8 * C, C, seed=2) / 8).half().to(DEV), rnd(8 * C, seed=3).half().to(DEV)
    x = F.pad(x, (0, 48))                                # K padded to 128 (c1 % 64 == 0)
    w = F.pad(w, (0, 48))
    n = 4 * C
    idx = torch.arange(2 * n).reshape(2, n // 16, 16).permute(1, 0, 2).reshape(-1).to(DEV)
    wp, bp = w[idx].contiguous(), b[idx].contiguous()
    g3, g1 = both(lib, lambda out, ld: ops.gemm(x, wp, out, M=M, N=8 * C, c1=128, lda=128, bias=bp, act=ops.ACT_GEGLU, ld_out=ld),
                  M, n, ld_pad)                          # output width N/2
    y = x.double() @ w.double().T + b.double()
    ref = y[:, :n] * F.gelu(y[:, n:])
    check_both(f"geglu {M}x{8 * C}x128 ld+{ld_pad}", g3, g1, ref, 1e-3)
    assert rel_l2(g3.cpu(), g1.cpu()) < 1e-3


@pytest.mark.parametrize("N,C,c2,O,H,W,stride,up,eps", [(13, 64, 0, 320, 61, 65, 1, 0, "rb"), (7, 64, 64, 320, 44, 170, 1, 0, "r1"),
                                                                 (5, 64, 0, 320, 50, 52, 1, 1, "bias"), (20, 128, 0, 640, 74, 70, 2, 0, "bias")])
def test_conv3x3(ops, lib, N, C, c2, O, H, W, stride, up, eps):
    ld_pad = 8 if N % 2 else 64                         # ld_out = O + 8 or O + 64
    x1, x2 = rnd(N, C, H, W, seed=1), (rnd(N, c2, H, W, seed=7) if c2 else None)
    w, b = rnd(O, C + c2, 3, 3, seed=2) / math.sqrt(9 * (C + c2)), rnd(O, seed=3)
    xin = torch.cat([x1, x2], 1) if c2 else x1
    xin = xin.half().float()
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    Ho, Wo = (xin.shape[2] - 1) // stride + 1, (xin.shape[3] - 1) // stride + 1
    M = N * Ho * Wo
    rpg = 3 * Ho * Wo
    rb = rnd(M // rpg + 1, O, seed=4).half().to(DEV) if eps == "rb" else None
    r1 = rnd(M, O, seed=5).half().to(DEV) if eps == "r1" else None
    a1, a2 = _nhwc(x1), (_nhwc(x2) if c2 else None)
    wp, bh = _pack3(w), b.half().to(DEV)

    def run(out, ld):
        ops.gemm(a1, wp, out, M=M, N=O, c1=C, lda=C, a2=a2, c2=c2, lda2=c2, bias=bh, rowbias=rb, ld_rowbias=O,
                 rows_per_group=rpg, r1=r1, ld_r1=O, mode=ops.A_CONV3X3, conv=(N, H, W, Ho, Wo, stride, up), ld_out=ld)
    g3, g1 = both(lib, run, M, O, ld_pad)
    y = conv3x3_ref64(xin, w.half(), b.half(), stride)
    if rb is not None:
        y = y + rb.double()[torch.arange(M, device=DEV) // rpg]
    if r1 is not None:
        y = y + r1.double()
    check_both(f"conv3x3 {N}x{C}+{c2}->{O} {H}x{W} s{stride} up{up} {eps} ld+{ld_pad}", g3, g1, y, 1e-3)
    assert rel_l2(g3.cpu(), g1.cpu()) < 1e-3


@pytest.mark.parametrize("case", ["dense_r1", "dense_rb_r1_r2", "dense_shortk_r1", "conv_r1", "convt_rb_r1"])
@pytest.mark.parametrize("streamk", [False, True])
def test_reslds_epilogue_matches_register_operand_build(ops, lib, case, streamk):
    """generation 3's residual-carrying direct epilogues (<*, 18 / 19 / 22 / 23>) land their r1 / r2 tiles in LDS by LDS-DMA behind COUNTED
    s_waitcnt vmcnt(n) waits whose counts assume how many global_store / DMA instructions hipcc emits per fragment -- wrong output with no error if a
    compiler update ever emits fewer.  This test runs every such variant on problems with full AND edge tiles (ragged M), with and without the
    stream-K tail, through the shipped library and through a build of the same source with the pre-round-5 register-operand epilogue
    (-DEW_G3_RESLDS=0: `make -C evoworld_amd/csrc reslds0`, built by __graft_entry__.build()) and requires the two to agree BIT FOR BIT (to the last fp32 bit where scaling coefficients make the fma contraction order differ)."""
    import os
    from evoworld_amd import _lib
    alt_path = os.path.join(os.path.dirname(_lib.LIB_PATH), "libevoworld_hip_reslds0.so")
    if not os.path.exists(alt_path):
        pytest.fail(f"{alt_path} missing: run `make -C evoworld_amd/csrc reslds0` (or __graft_entry__.build())")
    alt = _lib.bind(ctypes.CDLL(alt_path))
    g = torch.Generator().manual_seed(17)
    r = lambda *sh: (torch.rand(*sh, generator=g) * 2 - 1)
    kw = {}
    if case.startswith("dense"):
        M, N, K = {"dense_r1": (115200 + 77, 640, 2560), "dense_rb_r1_r2": (57600 + 130, 1280, 1280), "dense_shortk_r1": (115200 + 9, 640, 640)}[case]
        a, w = r(M, K).half().to(DEV), (r(N, K) / math.sqrt(K)).half().to(DEV)
        kw = dict(M=M, N=N, c1=K, lda=K)
        if case == "dense_rb_r1_r2":
            kw.update(rowbias=r(M // 5000 + 1, N).half().to(DEV), rows_per_group=5000, ld_rowbias=N, r2=ops.Res.from_float(r(M, N).to(DEV)), ld_r2=N, c_r2=0.4, c_acc=0.6)
        want = {"dense_r1": "<0, 19>", "dense_rb_r1_r2": "<0, 23>", "dense_shortk_r1": "<0, 19>"}[case]
    elif case == "conv_r1":
        Nimg, C, O, H, W = 19, 128, 640, 36, 64
        M, N = Nimg * H * W, O
        a = r(M, C).half().to(DEV)
        w = ops.pack_conv_weight((r(O, C, 3, 3) / math.sqrt(9 * C)).to(DEV))
        kw = dict(M=M, N=N, c1=C, lda=C, mode=ops.A_CONV3X3, conv=(Nimg, H, W, H, W, 1, 0))
        want = "<1, 18>"
    else:
        B, T, P, C, O = 2, 25, 2304 + 3, 128, 640
        M, N = B * T * P, O
        a = r(M, C).half().to(DEV)
        w = ops.pack_conv_weight((r(O, C, 3, 1, 1) / math.sqrt(3 * C)).to(DEV))
        kw = dict(M=M, N=N, c1=C, lda=C, mode=ops.A_CONVT3, tconv=(B, T, P), rowbias=r(B, N).half().to(DEV), rows_per_group=T * P, ld_rowbias=N)
        want = "<2, 19>"
    bias = r(N).half().to(DEV)
    r1 = ops.Res.from_float(r(M, N).to(DEV) * 2)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ops.streamk_init()
    assert alt.ew_gemm_streamk_init(st) == 0

    def run(L):
        out = ops.Res.empty(M, N, DEV, True)
        out.hi.fill_(5.0); out.lo.fill_(1)
        L.ew_set_gemm_debug(0 if streamk else 4)
        try:
            with _lib.using(L):                          # ops.gemm fills the ew_gemm_args struct; the call goes to library L
                ops.gemm(a, w, out, bias=bias, r1=r1, ld_r1=N, **kw)
                name = L.ew_gemm_last_kernel().decode()
        finally:
            L.ew_set_gemm_debug(0)
        torch.cuda.synchronize()
        return out, name
    o1, n1 = run(lib)
    o0, n0 = run(alt)
    assert n1 == n0 == "gemm3_kernel" + want, (n1, n0)
    assert lib.ew_gemm_streamk_status() == 0 and alt.ew_gemm_streamk_status() == 0
    f1, f0 = o1.float(), o0.float()
    nbad = int((o1.hi != o0.hi).sum()) + int((o1.lo != o0.lo).sum())
    dmax = float((f1 - f0).abs().max())
    print(f"RES_LDS 1 vs 0, {case}, stream-K {streamk}: {nbad} differing hi / lo8 words of {2 * M * N}, max |delta| of the decoded values {dmax:.2e}")
    assert torch.isfinite(f1).all() and float(f1.abs().mean()) > 0.1
    if "r2" in case:
        # c_acc / c_r2 != 1: the two epilogues contract acc * c_acc + r1 + c_r2 * r2 into fmas in a different order -- last-bit differences of the fp32
        # value (one lo8 step = 2^-18 relative) are legitimate; a stale LDS tile would be wrong by O(1) on whole 16-row fragments
        assert dmax < 4e-5 and nbad < 0.02 * M * N
    else:
        assert nbad == 0


@pytest.mark.parametrize("N,C,c2,O,H,W,split_rows", [(7, 64, 0, 4, 24, 40, False),     # ragged last workgroup (6720 pixels)
                                                              (5, 128, 64, 4, 36, 64, True),    # conv_out's form: rows [x_hi | x_lo] + the x_hi half again (lda2 != c2)
                                                              (3, 192, 0, 8, 40, 48, False), (2, 64, 64, 16, 72, 128, False),
                                                              (4, 64, 0, 12, 30, 41, False)])
def test_conv3x3_small_n_kernel(ops, lib, N, C, c2, O, H, W, split_rows):
    """Round 6: stride-1 3x3 convs with N <= 16 output channels (the U-Net's conv_out: 320 -> 4 with three split-operand K blocks) run on
    conv_small_n_kernel instead of a 160-wide tile of the generic kernels -- against fp64 and against generation 1."""
    M = N * H * W
    ld_pad = 8 if N % 2 else 64                          # ld_out = O + 8 or O + 64
    if split_rows:
        xs = rnd(N, C, H, W, seed=1)                                     # source 1 = the full 2*c2-wide rows, source 2 = their first c2 channels
        a1 = _nhwc(xs)
        a2, lda2 = a1, C
        xin = torch.cat([xs, xs[:, :c2]], 1)
    else:
        x1, x2 = rnd(N, C, H, W, seed=1), (rnd(N, c2, H, W, seed=7) if c2 else None)
        a1, a2, lda2 = _nhwc(x1), (_nhwc(x2) if c2 else None), c2
        xin = torch.cat([x1, x2], 1) if c2 else x1
    w, b = rnd(O, C + c2, 3, 3, seed=2) / math.sqrt(9 * (C + c2)), rnd(O, seed=3)
    wp, bh = _pack3(w), b.half().to(DEV)

    def run(out, ld):
        ops.gemm(a1, wp, out, M=M, N=O, c1=C, lda=C, a2=a2, c2=c2, lda2=lda2, bias=bh, mode=ops.A_CONV3X3, conv=(N, H, W, H, W, 1, 0), ld_out=ld)
    g3, g1 = both(lib, run, M, O, ld_pad, want3=f"conv_small_n_kernel<{(O + 3) // 4 * 4}>")
    y = conv3x3_ref64(xin.half(), w.half(), b.half())
    check_both(f"conv small-N {N}x{C}+{c2}->{O} {H}x{W} ld+{ld_pad}", g3, g1, y, 4e-4)
    e1 = rel_l2(g3.cpu(), g1.cpu())
    print(f"conv3x3 small-N O={O}: rel-L2 vs generation 1 {e1:.2e}")
    assert e1 < 4e-4


def test_conv_temporal(ops, lib):
    for ld_pad in (8, 64):
        _conv_temporal_case(ops, lib, ld_pad)


def _conv_temporal_case(ops, lib, ld_pad):
    B, T, P, C, O = 2, 25, 1031, 64, 320
    x = rnd(B, T, P, C, seed=1)
    w, b = rnd(O, C, 3, 1, 1, seed=2) / math.sqrt(3 * C), rnd(O, seed=3)
    wp = _pack3(w)                                                     # [O,C,3,1,1] -> chunk-major / tap-minor
    xin = x.reshape(B * T * P, C).half().to(DEV)
    r1 = rnd(B * T * P, O, seed=5).half().to(DEV)
    g3, g1 = both(lib, lambda out, ld: ops.gemm(xin, wp, out, M=B * T * P, N=O, c1=C, lda=C, bias=b.half().to(DEV), r1=r1, ld_r1=O,
                                                 c_acc=0.3, mode=ops.A_CONVT3, tconv=(B, T, P), ld_out=ld), B * T * P, O, ld_pad)
    y = 0.3 * convt3_ref64(x.half(), w.half(), b.half()) + r1.double()
    check_both(f"conv temporal {B}x{T}x{P} {C}->{O} r1 ld+{ld_pad}", g3, g1, y, 1e-3)
    assert rel_l2(g3.cpu(), g1.cpu()) < 1e-3


# ----------------------------------------------------------------------------- stream-K tail
def _half_b256_case(ops, lib, case, M):
    """The HALF split on the 256-wide instance (gemm3b_kernel), which half_dense / half_conv (N = 1280) never reach.
    half_b256_min: M = 1024 / 1000 (ragged last row tile), N = 512, K = 8192 -- 8 tiles on a grid of 16, the smallest problem plan3
    puts there; half_dense's operands (bias + split r1 -> <0, 19>).  half_b256_attn: the VAE attention's P V at 9216 tokens, M = 9216,
    N = 512, K = 9216, no bias (<0, 0>, grid 144, 72 K-tiles per half); A = fp16 softmax rows of 2.3 * randn scores, most of whose
    entries are fp16 denormals, W = randn V^T.
    Guarded, twice-prefilled outputs; the restated plan and the kernel name; against the ew_set_gemm_debug(4) launch (generation 2)
    under 1e-4; generation 3, generation 2 and generation 1 against the fp64 product per row."""
    N = 512
    attn = case == "half_b256_attn"
    if attn:
        K = 9216
        x = softmax_rows_f16(M, K, device=DEV)
        frac = denormal_fraction(x)
        print(f"stream-K {case}: {frac:.3f} of A are non-zero fp16 denormals, row sums {float(x.float().sum(1).mean()):.4f}")
        assert frac > 0.5                                            # a condition on the input
        w = torch.randn(N, K, generator=torch.Generator().manual_seed(12)).half().to(DEV)
        b = r1 = None
        run = lambda out, ld: ops.gemm(x, w, out, M=M, N=N, c1=K, lda=K, ld_out=ld)
        operands, split = set(), False
    else:
        K = 8192
        g = torch.Generator().manual_seed(11)
        rnd_ = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)
        x, w, b = rnd_(M, K).half().to(DEV), (rnd_(N, K) / 64).half().to(DEV), rnd_(N).half().to(DEV)
        r1 = ops.Res.from_float(rnd_(M, N).to(DEV) * 3)
        run = lambda out, ld: ops.gemm(x, w, out, M=M, N=N, c1=K, lda=K, bias=b, r1=r1, ld_r1=N, ld_out=ld)
        operands, split = {"r1", "lo"}, True
    ld_pad = 64 if M % 256 == 0 else 8
    G = lib.ew_get_cu_budget()
    plan = gen3_plan(M, N, K, "dense", operands, G, ld=N + ld_pad)
    assert plan.taken and plan.schedule == "half" and plan.kernel.startswith("gemm3b_kernel<0, ") and plan.grid == 2 * plan.tiles <= G, \
        (plan.kernel, plan.schedule, plan.tiles, G)
    assert all(len(it) == 1 and it[0][2] - it[0][1] == K // 128 for it in plan.items)
    assert not gen3_plan(M, N, K, "dense", operands, G, debug=4, ld=N + ld_pad).taken
    dec = lambda hi, lo: ops.Res(hi, lo).float() if split else hi.float()
    try:
        hi, lo, name = guarded_planes(lib, 3, plan.kernel, run, M, N, ld_pad, split)
        a = dec(hi, lo)
        assert name == plan.kernel, (name, plan.kernel)
        assert lib.ew_gemm_streamk_status() == 0
        lib.ew_set_gemm_debug(4)                                 # no split: generation 2's tiles
        c = guarded(lib, 3, "gemm2_kernel", run, M, N, ld_pad, split)
    finally:
        lib.ew_set_gemm_debug(0)
    g1 = guarded(lib, 1, "gemm_kernel", run, M, N, ld_pad, split)
    assert lib.ew_gemm_streamk_status() == 0
    err = rel_l2(a.cpu(), c.cpu())
    print(f"stream-K {case} M={M}: {name}, grid {plan.grid}; rel-L2 vs generation 2 {err:.2e}, max abs {float((a - c).abs().max()):.3e}")
    y = x.double() @ w.double().T
    if not attn:
        y = y + b.double() + r1.float().double()
    key = f"stream-K {case} M={M} ld+{ld_pad}"
    tol = 2e-5 if split else 1e-3
    failed = []
    for label, got in (("generation 1", g1), ("generation 2", c), ("generation 3", a)):       # every figure is printed before the test fails
        try:
            report(f"{key} {label}", got, y, WORST_ROW[key][0], tol)
        except AssertionError as e:
            failed.append(str(e))
    assert float(a.abs().mean()) > 1e-3
    assert err < 1e-4
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("case", ["dense_res", "conv", "convt", "dense_k320", "half_dense", "half_conv", "half_b256_min", "half_b256_attn"])
def test_streamk_tail_matches_whole_tile_schedule(case):
    """Generation 3 splits the last round of tiles along K (stream-K tail) when whole-tile rounds would idle > 4 % of the chip.
    Same problem with the split switched off (ew_set_gemm_debug bit 2): results may differ only by the fp32 summation order of the
    split tiles, i.e. by rare 1-ulp flips of the fp16 outputs; the split itself is deterministic (two runs bit-identical)."""
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    if case.startswith("half_b256"):
        for M in ((1024, 1000) if case == "half_b256_min" else (9216,)):
            _half_b256_case(ops, lib, case, M)
        return
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)
    if case == "dense_res":                  # level-1 feed-forward down projection: 900 tiles = 3.52 rounds
        M, N, K = 115200, 640, 2560
        x, w, b = rnd(M, K).half().to(DEV), (rnd(N, K) / 32).half().to(DEV), rnd(N).half().to(DEV)
        r1 = ops.Res.from_float(rnd(M, N).to(DEV) * 3)
        run = lambda out, ld: ops.gemm(x, w, out, M=M, N=N, c1=K, lda=K, bias=b, r1=r1, ld_r1=N, ld_out=ld)
        split = True
    elif case == "dense_k320":               # K below the default threshold: must take the whole-tile schedule either way
        M, N, K = 115200, 640, 320
        x, w, b = rnd(M, K).half().to(DEV), (rnd(N, K) / 16).half().to(DEV), rnd(N).half().to(DEV)
        run = lambda out, ld: ops.gemm(x, w, out, M=M, N=N, c1=K, lda=K, bias=b, ld_out=ld)
        split = False
    elif case == "conv":                     # level-0 3x3 conv + row-bias: 1800 tiles = 7.03 rounds, K = 2880 (45 K-tiles, taps inside)
        n, C, H, W = 50, 320, 72, 128
        M = n * H * W
        x, w, b = rnd(M, C).half().to(DEV), (rnd(C, 9 * C) / 40).half().to(DEV), rnd(C).half().to(DEV)
        rb = rnd(n, C).half().to(DEV)
        run = lambda out, ld: ops.gemm(x, w, out, M=M, N=C, c1=C, lda=C, bias=b, mode=ops.A_CONV3X3, conv=(n, H, W, H, W, 1, 0),
                                   rowbias=rb, rows_per_group=H * W, ld_rowbias=C, ld_out=ld)
        split = False
    elif case == "half_dense":               # round 4, HALF split: deepest-level feed-forward down projection, 116 tiles < 256 CUs
        M, N, K = 7200, 1280, 10240          # (the default threshold is K >= 8192)
        x, w, b = rnd(M, K).half().to(DEV), (rnd(N, K) / 64).half().to(DEV), rnd(N).half().to(DEV)
        r1 = ops.Res.from_float(rnd(M, N).to(DEV) * 3)
        run = lambda out, ld: ops.gemm(x, w, out, M=M, N=N, c1=K, lda=K, bias=b, r1=r1, ld_r1=N, ld_out=ld)
        split = True
    elif case == "half_conv":                # deepest-level 3x3 conv + row-bias (K = 11520: 180 K-tiles, 90 per half), ragged M
        n, C, H, W = 50, 1280, 9, 16
        M = n * H * W
        x, w, b = rnd(M, C).half().to(DEV), (rnd(C, 9 * C) / 80).half().to(DEV), rnd(C).half().to(DEV)
        rb = rnd(n, C).half().to(DEV)
        run = lambda out, ld: ops.gemm(x, w, out, M=M, N=C, c1=C, lda=C, bias=b, mode=ops.A_CONV3X3, conv=(n, H, W, H, W, 1, 0),
                                   rowbias=rb, rows_per_group=H * W, ld_rowbias=C, ld_out=ld)
        split = False
    else:                                    # level-1 temporal conv (3 taps) with a split residual
        B, T, P, C = 2, 25, 2304, 640
        M = B * T * P
        x, w, b = rnd(M, C).half().to(DEV), (rnd(C, 3 * C) / 30).half().to(DEV), rnd(C).half().to(DEV)
        r1 = ops.Res.from_float(rnd(M, C).to(DEV))
        run = lambda out, ld: ops.gemm(x, w, out, M=M, N=C, c1=C, lda=C, bias=b, mode=ops.A_CONVT3, tconv=(B, T, P), r1=r1, ld_r1=C, ld_out=ld)
        split = True
    n_out = N if case.startswith(("dense", "half_dense")) else C
    ld_pad = 64 if case in ("dense_res", "conv", "half_dense") else 8
    try:                                                         # split on: two runs into differently prefilled guarded outputs
        a = guarded(lib, 3, "gemm3_kernel", run, M, n_out, ld_pad, split)
        lib.ew_set_gemm_debug(4)                                 # off: whole tiles; half_*: generation 2's 256x160 tiles
        c = guarded(lib, 3, "gemm2_kernel" if case.startswith("half") else "gemm3_kernel", run, M, n_out, ld_pad, split)
    finally:
        lib.ew_set_gemm_debug(0)
    assert lib.ew_gemm_streamk_status() == 0
    err = rel_l2(a.cpu(), c.cpu())
    print(f"stream-K {case}: rel-L2 vs whole-tile schedule {err:.2e}, max abs {float((a - c).abs().max()):.3e}")
    assert err < (2e-5 if not case.startswith("half") else 1e-4)     # half_*: the comparison kernel is generation 2 (another tile order)
    if case == "dense_k320":
        assert torch.equal(a, c)
    if case.startswith(("dense", "half_dense")):                # fp64 reference of the split schedule
        y = x.double() @ w.double().T + b.double()
        if split:
            y = y + r1.float().double()
        report(f"stream-K {case} ld+{ld_pad}", a, y, WORST_ROW[f"stream-K {case} ld+{ld_pad}"][0], 2e-5 if split else 1e-3)


# ----------------------------------------------------------------------------- the 256-wide instance (VAE channel counts)
@pytest.mark.parametrize("M,N,K,eps", [(61237, 256, 320, "bias"), (52011, 512, 192, "rb+r1"), (70000, 256, 1920, "r1+r2"),
                                               (51456, 512, 64, "silu"), (26000, 1024, 448, "split"), (140000, 256, 2304, "split")])
def test_b256_dense_epilogues(ops, lib, M, N, K, eps):
    """gemm3_f16.hip compiled with EW3_BN = 256 (N % 256 == 0 and N % 320 != 0): every epilogue family against fp64 and
    against generation 2, incl. the split residual stream and (last case: 547 x 1 tiles, K = 2304) the stream-K tail."""
    ld_pad = 8 if M % 2 else 64                         # ld_out = N + 8 or N + 64
    x, w, b = rnd(M, K, seed=1).half().to(DEV), (rnd(N, K, seed=2) / math.sqrt(K)).half().to(DEV), rnd(N, seed=3).half().to(DEV)
    rpg = 7001
    G = M // rpg + 1
    rb = rnd(G, N + 64, seed=4).half().to(DEV) if "rb" in eps else None
    split = eps == "split"
    r1f = rnd(M, N, seed=5).to(DEV)
    r1 = (ops.Res.from_float(r1f) if split else r1f.half()) if ("r1" in eps or split) else None
    r2 = rnd(M, N + 8, seed=6).half().to(DEV) if "r2" in eps else None
    act = ops.ACT_SILU if eps == "silu" else ops.ACT_NONE

    def run(out, ld):
        ops.gemm(x, w, out, M=M, N=N, c1=K, lda=K, bias=b, rowbias=None if rb is None else rb[:, 64:], ld_rowbias=N + 64,
                 rows_per_group=rpg, r1=r1, ld_r1=N, r2=r2, ld_r2=N + 8, act=act, c_acc=0.7, c_r1=0.6, c_r2=-1.5, ld_out=ld)
    g3, g2 = both(lib, run, M, N, ld_pad, split=split, want3="gemm3b_kernel", gen_b=2, want_b="gemm2_kernel")
    y = x.double() @ w.double().T + b.double()
    if rb is not None:
        y = y + rb[:, 64:].double()[torch.arange(M, device=DEV) // rpg]
    if act:
        y = F.silu(y)
    y = 0.7 * y
    if r1 is not None:
        y = y + 0.6 * r1.float().double()
    if r2 is not None:
        y = y - 1.5 * r2[:, :N].double()
    tol = 2e-5 if split else 1e-3
    check_both(f"b256 dense {M}x{N}x{K} {eps} ld+{ld_pad}", g3, g2, y, tol)
    assert rel_l2(g3.cpu(), g2.cpu()) < tol
    assert lib.ew_gemm_streamk_status() == 0


@pytest.mark.parametrize("C,O,H,W,mode", [(256, 256, 96, 128, "plain"), (512, 512, 96, 128, "res"), (512, 256, 96, 128, "up"),
                                                  (128, 256, 192, 256, "shift")])
def test_b256_conv3x3(ops, lib, C, O, H, W, mode):
    ld_pad = 8 if mode in ("plain", "shift") else 64       # ld_out = O + 8 or O + 64
    """VAE conv shapes on the 256-wide instance: plain, + residual, nearest-x2 upsample addressing, Downsample2D(padding=0)
    taps (conv_shift) -- against fp64 and against generation 2."""
    n = 6
    x = rnd(n, C, H, W, seed=1).half()
    w = (rnd(O, C, 3, 3, seed=2) / math.sqrt(9 * C)).half()
    b = rnd(O, seed=3).half()
    xin = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous().to(DEV)
    wp = w.permute(0, 2, 3, 1).reshape(O, 9, C // 64, 64).permute(0, 2, 1, 3).reshape(O, 9 * C).contiguous().to(DEV)   # [O, C/64, tap, 64]
    stride, up, shift = 1, 0, 0
    if mode == "up":
        Ho, Wo, up = 2 * H, 2 * W, 1
        ref = conv3x3_ref64(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w, b)
    elif mode == "shift":
        stride, shift = 2, 1
        Ho, Wo = H // 2, W // 2
        ref = conv3x3_ref64(F.pad(x.float(), (0, 1, 0, 1)), w, b, stride=2, pad=0)
    else:
        Ho, Wo = H, W
        ref = conv3x3_ref64(x, w, b)
    M = n * Ho * Wo
    r1 = rnd(M, O, seed=4).half().to(DEV) if mode == "res" else None
    if r1 is not None:
        ref = ref + r1.double()

    def run(out, ld):
        ops.gemm(xin, wp, out, M=M, N=O, c1=C, lda=C, bias=b.to(DEV), mode=ops.A_CONV3X3, conv=(n, H, W, Ho, Wo, stride, up),
                 r1=r1, ld_r1=O, conv_shift=shift, ld_out=ld)
    g3, g2 = both(lib, run, M, O, ld_pad, want3="gemm3b_kernel", gen_b=2, want_b="gemm2_kernel")
    check_both(f"b256 conv3x3 {C}->{O} {H}x{W} {mode} ld+{ld_pad}", g3, g2, ref, 1e-3)
    assert rel_l2(g3.cpu(), g2.cpu()) < 1e-3


# ----------------------------------------------------------------------------- generation 3's 32-bit epilogue offsets
@pytest.mark.parametrize("M,want", [(524287, "gemm3_kernel"), (524289, "gemm2_kernel")])
def test_gen3_32bit_offset_edge(ops, lib, M, want):
    """Generation 3 addresses its epilogue rows as base + unsigned 32-bit byte offset and takes a problem only while
    M * ld_out * 2 < 2^32 (ew_gemm3_wants): ld_out = 4096 puts M = 524287 just under the edge (generation 3 must take it, and its
    last rows must land where they belong) and M = 524289 just over it (generation 2, 64-bit offsets).  Columns 320..4095 of every row
    and one 256-row tile past the end are the guard; each output buffer is ~4.3 GB."""
    N, K, ld = 320, 64, 4096
    assert (M * ld * 2 < 1 << 32) == (want == "gemm3_kernel")
    x, w, b = rnd(M, K, seed=1).half().to(DEV), (rnd(N, K, seed=2) / 8).half().to(DEV), rnd(N, seed=3).half().to(DEV)
    out = guarded(lib, 3, want, lambda o, ldo: ops.gemm(x, w, o, M=M, N=N, c1=K, lda=K, bias=b, ld_out=ldo), M, N, ld - N)
    rows = torch.cat([torch.arange(0, M, 997, device=DEV), torch.arange(M - 512, M, device=DEV)])    # a sample + the last 512 rows
    y = x[rows].double() @ w.double().T + b.double()
    case = f"32-bit edge M={M} ld_out={ld}"
    report(case, out[rows], y, WORST_ROW[case][0], 1e-3)


