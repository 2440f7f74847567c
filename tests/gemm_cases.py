"""GEMM test helpers shared by test_gpu_gemm_gen3.py and test_gpu_gemm_gen2.py (a plain module, imported like kernel_checks.py and
reproject_cases.py).

- guarded / guarded_planes: one ew_gemm_f16 problem under a given generation into guarded, twice-prefilled outputs.
- conv3x3_ref64 / convt3_ref64: fp64 references of the two conv addressing modes.
- gen2_schedule: generation 2's tile family and persistent block sequence restated (csrc/gemm2_f16.hip: dispatch_tile, seq0, n_my).
- GEN2_CASES + problem(): the multi-round generation-2 problems of test_gpu_gemm_gen2.py, each with a run(out, ld_out, r0, r1)
  that launches rows [r0, r1) alone, and piece_ranges / piece_diff for the piece-identity check: a launch cut into tile-aligned
  pieces of at most one tile per workgroup must reproduce the rows of the whole launch bit for bit.
  tests/test_cpu_gemm_gen2_cases.py checks the table's tile counts and that piece_diff catches one stale fragment."""
import math

import torch
import torch.nn.functional as F

from kernel_checks import _INT, two_prefills

DEV = "cuda"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def guarded_planes(lib, gen, want, run, M, n_out, ld_pad, split=False):
    """run(out, ld_out) under generation `gen`, into guarded outputs (one 256-row tile of pad rows, ld_out = n_out + ld_pad; the
    lo8 plane guarded too when `split`) with two prefills; asserts the kernel name starts with `want`.  Returns the first run's
    (hi view, lo view or None) and the kernel name."""
    from evoworld_amd.ops import Res
    ld = n_out + ld_pad
    names = []

    def call(hi, *rest):
        run(Res(hi, rest[0]) if split else hi, ld)
        names.append(lib.ew_gemm_last_kernel().decode())
    specs = [(M, n_out, torch.float16, dict(ld=ld))] + ([(M, n_out, torch.int8, dict(ld=ld))] if split else [])
    lib.ew_set_gemm_generation(gen)
    try:
        gs = two_prefills(call, *specs)
    finally:
        lib.ew_set_gemm_generation(3)
    assert all(n.startswith(want) for n in names), names
    return gs[0].view, (gs[1].view if split else None), names[0]


def guarded(lib, gen, want, run, M, n_out, ld_pad, split=False):
    """guarded_planes, decoded: returns the result as float (hi + lo8 when `split`)."""
    from evoworld_amd.ops import Res
    hi, lo, _ = guarded_planes(lib, gen, want, run, M, n_out, ld_pad, split)
    return Res(hi, lo).float() if split else hi.float()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).half().contiguous().to(DEV)


def _pack3(w):
    from evoworld_amd.ops import pack_conv_weight
    return pack_conv_weight(w.half().float()).to(DEV)


def conv3x3_ref64(xin, w, b, stride=1, pad=1):
    """fp64 3x3 conv of xin [N,C,H,W] (already upsampled / padded as the kernel reads it) by im2col, one image at a time ->
    [N*Ho*Wo, O] rows in the kernel's NHWC order"""
    O = w.shape[0]
    wm = w.reshape(O, -1).double().to(DEV)
    out = [(wm @ F.unfold(xi[None].double().to(DEV), 3, padding=pad, stride=stride)[0]).T for xi in xin]
    y = torch.cat(out)
    return y + b.double().to(DEV) if b is not None else y


def convt3_ref64(x, w, b):
    """fp64 temporal conv, kernel (3,1,1) padding (1,0,0): x [B,T,P,C], w [O,C,3,1,1] -> [B*T*P, O]"""
    xd = F.pad(x.double().to(DEV), (0, 0, 0, 0, 1, 1))                  # zero frames at both ends
    T = x.shape[1]
    wd = w.double().to(DEV).reshape(w.shape[0], w.shape[1], 3)
    y = sum(xd[:, kt: kt + T] @ wd[:, :, kt].T for kt in range(3))
    return y.reshape(-1, w.shape[0]) + b.double().to(DEV)


# ----------------------------------------------------------------------------- generation 2's schedule, restated
def gen2_family(N, geglu):
    """dispatch_tile: (BM, BN, WM, WN) -- 256x160 (4 x 2 waves) when N % 160 == 0 or N <= 160 and not GEGLU, else 128x256 (2 x 4)"""
    if not geglu and (N % 160 == 0 or N <= 160):
        return 256, 160, 64, 80
    return 128, 256, 64, 64


def gen2_schedule(M, N, geglu, G):
    """(BM, BN, tiles_m, tiles_n, min tiles per block, max tiles per block) of a generation-2 launch on G persistent workgroups:
    block b computes tiles i*G + seq0, seq0 = (b & 7) * (G >> 3) + (b >> 3), n_my = (tiles - 1 - seq0) // G + 1 of them."""
    BM, BN, _, _ = gen2_family(N, geglu)
    tiles_m, tiles_n = -(-M // BM), -(-N // BN)
    tiles = tiles_m * tiles_n
    grid = G if tiles >= G else (tiles + 7) // 8 * 8            # launch2: fewer tiles than workgroups shrinks the grid
    n_my = []
    for b in range(grid):
        seq0 = (b & 7) * (grid >> 3) + (b >> 3)
        n_my.append((tiles - 1 - seq0) // grid + 1 if seq0 < tiles else 0)
    assert sum(n_my) == tiles
    return BM, BN, tiles_m, tiles_n, min(n_my), max(n_my)


def piece_ranges(M, N, geglu, G, unit=256, units_per_piece=None):
    """Row ranges [(r0, r1)] covering [0, M): each starts at a multiple of 256 rows and of `unit` (rows of one image / batch
    element; 256 for dense) and holds at most G // tiles_n tile rows, so that it runs as one round of the same tile decomposition."""
    BM, BN, _, tiles_n, _, _ = gen2_schedule(M, N, geglu, G)
    step = unit * 256 // math.gcd(unit, 256)
    rows = (G // tiles_n) * BM // step * step
    if units_per_piece is not None:
        rows = min(rows, units_per_piece * unit)
    assert rows > 0 and rows % 256 == 0 and rows % BM == 0 and (rows // BM) * tiles_n <= G, (rows, BM, tiles_n, G)
    return [(r0, min(r0 + rows, M)) for r0 in range(0, M, rows)]


def piece_diff(whole, pieces, N, geglu, G, limit=6):
    """whole / pieces: lists of same-shaped [M, n_out] planes (hi, then lo8 where present) of the whole launch and of the rows
    assembled from the piece launches.  Returns (number of differing words, description of the first `limit`: row, column, tile id,
    round of its workgroup's sequence, wave tile)."""
    BM, BN, WM, WN = gen2_family(N, geglu)
    tiles_n = -(-N // BN)
    scale = 2 if geglu else 1                            # GEGLU: output column c comes from the tile columns around 2c
    count, where = 0, []
    for k, (a, b) in enumerate(zip(whole, pieces)):
        assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape)
        d = a.contiguous().view(_INT[a.dtype]) != b.contiguous().view(_INT[b.dtype])
        n = int(d.sum())
        count += n
        if n:
            for r, c in d.nonzero()[:limit].tolist():
                tid = (r // BM) * tiles_n + (scale * c) // BN
                where.append(f"{'lo8' if k else 'hi'} ({r}, {c}): tile {tid} = ({r // BM}, {(scale * c) // BN}), round {tid // G}, "
                             f"wave tile ({(r % BM) // WM}, {((scale * c) % BN) // WN}), fragment row {(r % WM) // 16}")
    return count, "; ".join(where)


# ----------------------------------------------------------------------------- the multi-round generation-2 cases
# tiles: tile count at G = 256.  Dense: M, N, K; conv: n images H x W (input), C (+ c2) -> O; temporal: B, T, P, C -> O.
# r1: None / "h" (fp16) / "s" (split hi + lo8); split: split output; gen: generation the whole launch is made under.
GEN2_CASES = {
    # nk = 1: every stream position ends a tile; 5-6 tiles per block, deeper than the ring
    "A1": dict(kind="dense", family=(256, 160), tiles=1290, M=110005, N=480, K=64, rb=True, r1="h"),
    # production forms <0, 19> / <0, 3>, ragged last row tile, under the DEFAULT generation: the name check pins plan3's short-K rule
    "A2s": dict(kind="dense", family=(256, 160), tiles=548, M=70013, N=320, K=320, rb=True, r1="s", split=True, gen=3, epi="0, 19>"),
    "A2h": dict(kind="dense", family=(256, 160), tiles=548, M=70013, N=320, K=320, rb=True, r1="h", gen=3, epi="0, 3>"),
    # nk = 2, one tile column
    "A3": dict(kind="dense", family=(256, 160), tiles=547, M=140021, N=160, K=128, bias=False, r1="h", r2=True, coef=(0.7, 0.6, -1.5)),
    # VAE form: N = 128 < 160, every tile N-ragged, no wave tile of wave column 1 is full
    "A4": dict(kind="conv", family=(256, 160), tiles=550, n=110, H=32, W=40, C=64, O=128, r1="s", split=True),
    # tiles straddle image seams, ragged M
    "A4u": dict(kind="conv", family=(256, 160), tiles=598, n=113, H=33, W=41, C=64, O=128, rb_imgs=3, pieces=False),
    # Downsample2D(padding=0) addressing, nk = 18
    "A5": dict(kind="conv", family=(256, 160), tiles=550, n=110, H=64, W=80, C=128, O=128, stride=2, shift=1),
    # per-row (dy, dx) codes rebuilt at each tile change, a2 switch mid-stream
    "A6": dict(kind="conv", family=(256, 160), tiles=550, n=110, H=16, W=20, C=64, c2=64, O=160, up=1, r1="h"),
    # tap mask per tile, nk = 3
    "A7": dict(kind="temporal", family=(256, 160), tiles=500, B=5, T=4, P=6400, C=64, O=128, rb=True, r1="s", split=True),
    # ragged, seams inside tiles
    "A7u": dict(kind="temporal", family=(256, 160), tiles=501, B=5, T=4, P=6403, C=64, O=128, rb=True, r1="h", pieces=False),
    # full column and N-ragged column (with 256 workgroups and 2 tile columns a block keeps its column: B8c below rotates them)
    "B8": dict(kind="dense", family=(128, 256), tiles=626, M=40005, N=448, K=192, r1="h"),
    # three tile columns (256 + 256 + 64): full and N-ragged columns alternate in each block's sequence, so stores_behind toggles
    "B8c": dict(kind="dense", family=(128, 256), tiles=705, M=30005, N=576, K=192, r1="h"),
    # GEGLU store count, half-width patch (weight rows interleaved in 16s, value | gate)
    "B9": dict(kind="dense", family=(128, 256), tiles=705, M=30001, N=640, K=128, geglu=True),
    # conv loader on the second family
    "B10": dict(kind="conv", family=(128, 256), tiles=560, n=70, H=32, W=32, C=128, O=256),
    # nk = 1, all tiles N-ragged, lo8 plane
    "B11": dict(kind="dense", family=(128, 256), tiles=516, M=66001, N=192, K=64, split=True),
}


def case_dims(c):
    """(M, N, K, geglu, piece unit in rows, units per piece or None) of a GEN2_CASES entry"""
    if c["kind"] == "dense":
        return c["M"], c["N"], c["K"], c.get("geglu", False), 256, None
    if c["kind"] == "conv":
        Ho, Wo = _conv_out_hw(c)
        return c["n"] * Ho * Wo, c["O"], 9 * (c["C"] + c.get("c2", 0)), False, Ho * Wo, None
    return c["B"] * c["T"] * c["P"], c["O"], 3 * c["C"], False, c["T"] * c["P"], 1


def _conv_out_hw(c):
    if c.get("up"):
        return 2 * c["H"], 2 * c["W"]
    if c.get("stride", 1) == 2:
        return c["H"] // 2, c["W"] // 2
    return c["H"], c["W"]


def case_pieces(c, G):
    """piece row ranges of a case, or None where the case does not tile-align (checked by guards, fp64 and generation 1 only)"""
    if not c.get("pieces", True):
        return None
    M, N, _, geglu, unit, upp = case_dims(c)
    return piece_ranges(M, N, geglu, G, unit, upp)


class Problem:
    """M, N, n_out (N / 2 for GEGLU), split (hi + lo8 output), run(out, ld_out, r0=0, r1=M): rows [r0, r1) as one launch
    (out is the view / Res of those rows), ref(): fp64 [M, n_out] on the device"""


def _rows(x, r0, r1):
    from evoworld_amd.ops import Res
    if x is None:
        return None
    return Res(x.hi[r0:r1], x.lo[r0:r1]) if isinstance(x, Res) else x[r0:r1]


def _residual(ops, kind, M, N, seed, scale):
    if kind is None:
        return None
    r = (rnd(M, N, seed=seed) * scale).to(DEV)
    return ops.Res.from_float(r) if kind == "s" else r.half()


def problem(ops, c, G):
    """Build the operands of GEN2_CASES entry c on the device (seeded CPU randn: weights / sqrt(K), residuals x 2 / x 3, row-bias
    groups aligned to the piece starts)."""
    M, N, K, geglu, unit, _ = case_dims(c)
    p = Problem()
    p.M, p.N, p.n_out, p.split = M, N, (N // 2 if geglu else N), c.get("split", False)
    c_acc, c_r1, c_r2 = c.get("coef", (1.0, 1.0, 1.0))
    w0 = rnd(N, *((K,) if c["kind"] == "dense" else (c["C"] + c.get("c2", 0), 3, 3) if c["kind"] == "conv" else (c["C"], 3, 1, 1)),
             seed=2) / math.sqrt(K)
    b0 = rnd(N, seed=3).half() if c.get("bias", True) else None
    bias = None if b0 is None else b0.to(DEV)
    r1 = _residual(ops, c.get("r1"), M, N, 5, 3.0)
    r2 = _residual(ops, "h" if c.get("r2") else None, M, N, 6, 2.0)
    pieces = case_pieces(c, G)
    if c["kind"] == "dense":
        rpg = max(1, (pieces[0][1] - pieces[0][0]) // 2)            # two groups per piece: piece starts are group starts
    elif c["kind"] == "conv":
        rpg = c.get("rb_imgs", 0) * unit
    else:
        rpg = unit                                                  # temporal: one row-bias row per batch element
    rb = rnd(-(-M // rpg), N, seed=4).half().to(DEV) if (c.get("rb") or c.get("rb_imgs")) else None
    common = dict(N=N, bias=bias, ld_rowbias=N, rows_per_group=max(rpg, 1), ld_r1=N, ld_r2=N, c_acc=c_acc, c_r1=c_r1, c_r2=c_r2)

    def operands(r0, r1_):
        assert rb is None or r0 % rpg == 0
        return dict(common, M=r1_ - r0, rowbias=None if rb is None else rb[r0 // rpg:], r1=_rows(r1, r0, r1_), r2=_rows(r2, r0, r1_))

    def finish(y):
        if rb is not None:
            y = y + rb.double()[torch.arange(M, device=DEV) // rpg]
        y = c_acc * y
        if r1 is not None:
            y = y + c_r1 * r1.float().double()
        if r2 is not None:
            y = y + c_r2 * r2.double()
        return y

    if c["kind"] == "dense":
        a, w = rnd(M, K, seed=1).half().to(DEV), w0.half().to(DEV)
        wk, bk = w, bias
        if geglu:                                                   # rows interleaved in 16s: [16 value | 16 gate] (unet._pack)
            n = N // 2
            idx = torch.arange(N).reshape(2, n // 16, 16).permute(1, 0, 2).reshape(-1).to(DEV)
            wk, bk = w[idx].contiguous(), bias[idx].contiguous()

        def run(out, ld, r0=0, r1_=M):
            kw = operands(r0, r1_)
            kw["bias"] = bk
            ops.gemm(a[r0:r1_], wk, out, c1=K, lda=K, act=ops.ACT_GEGLU if geglu else ops.ACT_NONE, ld_out=ld, **kw)

        def ref():
            y = a.double() @ w.double().T
            if bias is not None:
                y = y + bias.double()
            return y[:, :N // 2] * F.gelu(y[:, N // 2:]) if geglu else finish(y)
    elif c["kind"] == "conv":
        n, H, W, C, c2 = c["n"], c["H"], c["W"], c["C"], c.get("c2", 0)
        stride, up, shift = c.get("stride", 1), c.get("up", 0), c.get("shift", 0)
        Ho, Wo = _conv_out_hw(c)
        x1, x2 = rnd(n, C, H, W, seed=1), (rnd(n, c2, H, W, seed=7) if c2 else None)
        a1, a2, wp = _nhwc(x1), (_nhwc(x2) if c2 else None), _pack3(w0)

        def run(out, ld, r0=0, r1_=M):
            assert r0 % unit == 0 and (r1_ == M or r1_ % unit == 0)
            i0, i1 = r0 // unit, r1_ // unit
            ops.gemm(a1[i0 * H * W: i1 * H * W], wp, out, c1=C, lda=C, a2=None if a2 is None else a2[i0 * H * W: i1 * H * W], c2=c2, lda2=c2,
                     mode=ops.A_CONV3X3, conv=(i1 - i0, H, W, Ho, Wo, stride, up), conv_shift=shift, ld_out=ld, **operands(r0, r1_))

        def ref():
            xin = (torch.cat([x1, x2], 1) if c2 else x1).half().float()
            if up:
                xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
            if shift:                                               # Downsample2D(padding=0): pad right / bottom, taps start at oy * stride
                return finish(conv3x3_ref64(F.pad(xin, (0, 1, 0, 1)), w0.half(), b0, stride=stride, pad=0))
            return finish(conv3x3_ref64(xin, w0.half(), b0, stride))
    else:
        B, T, P, C = c["B"], c["T"], c["P"], c["C"]
        x = rnd(B, T, P, C, seed=1)
        xin, wp = x.reshape(M, C).half().to(DEV), _pack3(w0)

        def run(out, ld, r0=0, r1_=M):
            assert r0 % unit == 0 and r1_ % unit == 0
            ops.gemm(xin[r0:r1_], wp, out, c1=C, lda=C, mode=ops.A_CONVT3, tconv=((r1_ - r0) // unit, T, P), ld_out=ld, **operands(r0, r1_))

        def ref():
            return finish(convt3_ref64(x.half(), w0.half(), b0))
    p.run, p.ref = run, ref
    return p
