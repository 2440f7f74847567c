"""GEMM test helpers shared by test_gpu_gemm_gen3.py, test_gpu_gemm_gen2.py and test_gpu_gemm_gen3_rounds.py (a plain module, imported
like kernel_checks.py and reproject_cases.py).

- guarded / guarded_planes: one ew_gemm_f16 problem under a given generation into guarded, twice-prefilled outputs.
- conv3x3_ref64 / convt3_ref64: fp64 references of the two conv addressing modes.
- gen2_schedule: generation 2's tile family and persistent block sequence restated (csrc/gemm2_f16.hip: dispatch_tile, seq0, n_my).
- GEN2_CASES + problem(): the multi-round generation-2 problems of test_gpu_gemm_gen2.py, each with a run(out, ld_out, r0, r1)
  that launches rows [r0, r1) alone, and piece_ranges / piece_diff for the piece-identity check: a launch cut into tile-aligned
  pieces of at most one tile per workgroup must reproduce the rows of the whole launch bit for bit.
  tests/test_cpu_gemm_gen2_cases.py checks the table's tile counts and that piece_diff catches one stale fragment.
- gen3_plan / tile_coords: generation 3's routing decision (csrc/gemm3_f16.hip: plan3), tile order and per-workgroup work-item lists
  (whole-tile schedule, stream-K tail, half split) restated.
- GEN3_CASES + gen3_piece_ranges: the multi-round generation-3 problems of test_gpu_gemm_gen3_rounds.py (problem() builds them too)
  and their single-round pieces; tests/test_cpu_gemm_gen3_cases.py checks that every case has the schedule its comment claims."""
import math
from types import SimpleNamespace

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


def piece_diff(whole, pieces, N, geglu, G, limit=6, family=None, tile_id=None, row0=0):
    """whole / pieces: lists of same-shaped [M, n_out] planes (hi, then lo8 where present) of the whole launch and of the rows
    assembled from the piece launches.  Returns (number of differing words, description of the first `limit`: row, column, tile id,
    round of its workgroup's sequence, wave tile).
    family: (BM, BN, WM, WN) where it is not generation 2's; tile_id(tm, tn): the tile order where it is not tm * tiles_n + tn
    (generation 3's bands); row0: first row of the planes in the whole problem (one piece compared on its own)."""
    BM, BN, WM, WN = family or gen2_family(N, geglu)
    tiles_n = -(-N // BN)
    tile_id = tile_id or (lambda tm, tn: tm * tiles_n + tn)
    scale = 2 if geglu else 1                            # GEGLU: output column c comes from the tile columns around 2c
    count, where = 0, []
    for k, (a, b) in enumerate(zip(whole, pieces)):
        assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape)
        d = a.contiguous().view(_INT[a.dtype]) != b.contiguous().view(_INT[b.dtype])
        n = int(d.sum())
        count += n
        if n:
            for r, c in d.nonzero()[:limit].tolist():
                r += row0
                tid = tile_id(r // BM, (scale * c) // BN)
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


def problem(ops, c, G, rpg=None):
    """Build the operands of GEN2_CASES / GEN3_CASES entry c on the device (seeded CPU randn: weights / sqrt(K), residuals x 2 / x 3,
    row-bias groups aligned to the piece starts; rpg: rows per row-bias group of a dense case where it is not generation 2's rule)."""
    M, N, K, geglu, unit, _ = case_dims(c)
    p = Problem()
    p.M, p.N, p.n_out, p.split = M, N, (N // 2 if geglu else N), c.get("split", False)
    c_acc, c_r1, c_r2 = c.get("coef", (1.0, 1.0, 1.0))
    w0 = rnd(N, *((K,) if c["kind"] == "dense" else (c["C"] + c.get("c2", 0), 3, 3) if c["kind"] == "conv" else (c["C"], 3, 1, 1)),
             seed=2) / math.sqrt(K)
    b0 = rnd(N, seed=3).half() if c.get("bias", True) else None
    bias = None if b0 is None else b0.to(DEV)
    r1 = _residual(ops, c.get("r1"), M, N, 5, 3.0)
    r2 = _residual(ops, {True: "h", False: None}.get(c.get("r2"), c.get("r2")), M, N, 6, 2.0)
    if c["kind"] == "dense" and rpg is not None:
        pass                                                        # GEN3_CASES: gen3_rowbias_rows
    elif c["kind"] == "dense":
        pieces = case_pieces(c, G)
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
            y = y + c_r2 * r2.float().double()
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


# ----------------------------------------------------------------------------- generation 3's plan and schedule, restated
def gen3_family(N):
    """(BM, BN, WM, WN): the 256x320 instance (4 x 2 waves of 64 x 160), or the 256x256 one when only 256 divides N"""
    BN = 256 if N % 256 == 0 and N % 320 != 0 else 320
    return 256, BN, 64, BN // 2


def gen3_epi(mode, operands):
    """ew_gemm_select_epi for generation 3: the EPI of an operand set (bit 0 row-bias, 1 r1, 2 r2, 3 GEGLU, 4 lo8 operands), or
    None where no variant exists.  operands: subset of {"rb", "r1", "r2", "lo", "geglu", "silu", "gelu"}"""
    dense = mode == "dense"
    if "geglu" in operands:
        return 8 if dense else None
    mask = ("rb" in operands) | ("r1" in operands) << 1 | ("r2" in operands) << 2
    if "lo" in operands:
        if mask & 6 == 0:
            return 16 | 1
        if dense:
            return 16 | 3 if mask & 4 == 0 else 16 | 7
        if mask & 5 == 0:
            return 16 | 2
        return 16 | 3 if mask & 4 == 0 else None
    if mask <= 2 or (dense and mask == 3):
        return mask
    return 6 if dense and mask in (4, 6) else 7


def tile_coords(id, tiles_m, tiles_n, band):
    """tile id -> (tm, tn): tn fastest, inside bands of `band` tile columns when there are more columns than that (the last band
    takes what is left)"""
    if band <= 0 or tiles_n <= band:
        return divmod(id, tiles_n)
    nb = -(-tiles_n // band)
    per_band = band * tiles_m
    k = min(id // per_band, nb - 1)
    r = id - k * per_band
    w = tiles_n - k * band if k == nb - 1 else band
    return r // w, k * band + r % w


def gen3_tile_ids(tiles_m, tiles_n, band):
    """[tm][tn] -> tile id (tile_coords inverted)"""
    ids = [[None] * tiles_n for _ in range(tiles_m)]
    for i in range(tiles_m * tiles_n):
        tm, tn = tile_coords(i, tiles_m, tiles_n, band)
        assert ids[tm][tn] is None, (i, tm, tn)
        ids[tm][tn] = i
    return ids


def gen3_plan(M, N, K, mode, operands, G, debug=0, ld=None):
    """plan3 and the kernel's block sequence for one problem on a CU budget of G: mode "dense" / "conv" / "temporal", operands as
    in gen3_epi, debug: ew_set_gemm_debug (bit 2: whole tiles only), ld: the largest of ld_out / ld_r1 / ld_r2 (default N).
    Returns .taken (generation 3 runs it; with a split, given a stream-K workspace), .kernel (name with <MODE, EPI>), .BM / .BN,
    .tiles_m / .tiles_n / .tiles / .nk / .band, .schedule ("whole", "tail" or "half"), .dp_rounds / .sk_tiles, .grid and
    .items[b]: the (tile id, k0, k1) work items of workgroup b in the order it runs them."""
    operands = set(operands)
    BM, BN, _, _ = gen3_family(N)
    dense = mode == "dense"
    rb, r1, r2, lo = ("rb" in operands, "r1" in operands, "r2" in operands, "lo" in operands)
    nk = K // 64
    tiles_m, tiles_n = -(-M // BM), N // BN
    tiles = tiles_m * tiles_n
    epi = gen3_epi(mode, operands)
    pl = SimpleNamespace(taken=False, BM=BM, BN=BN, epi=epi, tiles_m=tiles_m, tiles_n=tiles_n, tiles=tiles, nk=nk, band=0,
                         schedule=None, dp_rounds=0, sk_tiles=0, grid=0, items=[],
                         kernel=f"{'gemm3_kernel' if BN == 320 else 'gemm3b_kernel'}<{('dense', 'conv', 'temporal').index(mode)}, {epi}>")
    if N % BN != 0 or M < 320 or epi is None:
        return pl
    if tiles > G * (8192 // 16 - 4):                                # work-item table of a persistent block
        return pl
    if "gelu" in operands and (not dense or rb or r1 or r2 or lo):
        return pl
    if "silu" in operands and (not dense or r1 or r2 or lo):
        return pl
    if M * (ld or N) * 2 >= 1 << 32 or (rb and (M + 2) * N * 2 >= 1 << 32):          # 32-bit epilogue offsets (row-bias: at most one row per M row)
        return pl
    if dense and N == BN and K <= 1280 and (r1 or r2):              # the short-K rule: generation 2's 256x160 tiles
        return pl
    sk_ok = not (dense and epi == 23) and not debug & 4
    pl.band = 4 if N * K * 2 > 3 * 1024 * 1024 else 0
    if tiles * 256 >= 200 * G:
        pl.grid = G if tiles >= G else (tiles + 7) // 8 * 8
        pl.schedule = "whole"
        sk_shape = mode == "conv" or (tiles_n <= 2 and K >= 1280)
        if sk_shape and sk_ok and tiles > G and tiles % G != 0:
            rounds = -(-tiles // G)
            if 1.0 - tiles / (G * rounds) > 0.04:
                pl.dp_rounds = tiles // G - 1
                pl.sk_tiles = tiles - G * pl.dp_rounds
                pl.schedule = "tail"
    else:
        half_shape = tiles >= 8 and 2 * tiles <= G and (2 * tiles) % 8 == 0 and nk % 2 == 0 and K >= 8192
        if not sk_ok or "geglu" in operands or not half_shape:
            return pl
        pl.grid, pl.sk_tiles, pl.schedule = 2 * tiles, tiles, "half"
    pl.taken = True
    Gk = pl.grid                                                    # the kernel's G is its grid
    for b in range(Gk):
        seq0 = (b & 7) * (Gk >> 3) + (b >> 3)
        items = []
        if pl.sk_tiles:
            U = pl.sk_tiles * nk
            u0, u1 = seq0 * U // Gk, (seq0 + 1) * U // Gk
            (tA, kA), (tB, kB) = divmod(u0, nk), divmod(u1, nk)
            n_sk, n_dp = (tB - tA) + (kB > 0), pl.dp_rounds
            if u1 - u0 + n_dp * nk == 0:
                n_sk = 0
        else:
            n_sk, n_dp = 0, ((tiles - 1 - seq0) // Gk + 1 if seq0 < tiles else 0)
        for w in range(n_sk + n_dp):
            if w < n_sk:
                t = tA + w
                items.append((pl.dp_rounds * Gk + t, kA if w == 0 else 0, kB if t == tB else nk))
            else:
                items.append(((w - n_sk) * Gk + seq0, 0, nk))
        pl.items.append(items)
    return pl


# ----------------------------------------------------------------------------- the multi-round generation-3 cases
# Same keys as GEN2_CASES (r2 may be "s" too).  schedule / band / dp_rounds / sk_tiles / tiles / per_wg (fewest, most work items of
# a workgroup) are what gen3_plan must give at G = 256 (tests/test_cpu_gemm_gen3_cases.py).  Whole-tile schedule unless noted.
GEN3_CASES = {
    # nk = 1: every stream position ends a tile; bias + row-bias enter through init_acc; ragged last row tile
    "G1": dict(kind="dense", tiles=392, per_wg=(1, 2), M=100100, N=320, K=64, rb=True),
    # two tile columns, RES_LDS epilogue (EPI & 6): the next item's first K-tile is staged inside the epilogue; lo8 plane
    "G2": dict(kind="dense", tiles=392, per_wg=(1, 2), M=50013, N=640, K=192, bias=False, rb=True, r1="s", split=True),
    # three tile columns, nk = 2
    "G3": dict(kind="dense", tiles=354, per_wg=(1, 2), M=30005, N=960, K=128, bias=False, r1="h", r2="h", coef=(0.7, 0.6, -1.5)),
    # <0, 23>: the variant compiled without the tail split
    "G4": dict(kind="dense", tiles=352, per_wg=(1, 2), M=45000, N=640, K=128, bias=False, rb=True, r1="s", r2="s", split=True,
               epi="<0, 23>", debug=0),
    # stream-K tail: every workgroup runs stream-K items and then one chained data-parallel tile
    "G5": dict(kind="dense", tiles=548, per_wg=(3, 4), M=70013, N=640, K=1280, r1="s", split=True, schedule="tail", dp_rounds=1, sk_tiles=292),
    # GEGLU: 8 tile columns, W = 1.6 MB (no band), n_out 1280, weight rows interleaved in 16s
    "G6": dict(kind="dense", tiles=376, per_wg=(1, 2), M=12000, N=2560, K=320, geglu=True),
    # banded tile order: one full and one ragged band (6 columns); a workgroup's two tiles lie in different bands
    "G7": dict(kind="dense", tiles=354, per_wg=(1, 2), M=15000, N=1920, K=1024, r1="h", band=4),
    # conv, nk = 9: 500 tiles lose 2.3 % <= 4 % of two rounds, so no tail
    "G8": dict(kind="conv", tiles=500, per_wg=(1, 2), n=125, H=32, W=32, C=64, O=320, rb_imgs=1),
    # ragged M, image seams inside tiles
    "G8u": dict(kind="conv", tiles=500, per_wg=(1, 2), n=125, H=33, W=31, C=64, O=320, rb_imgs=3, pieces=False),
    # per-row (dy, dx) codes and the a2 switch rebuilt at each tile change (100 images: 500 tiles, as G8, keep the plan whole-tile)
    "G9": dict(kind="conv", tiles=500, per_wg=(1, 2), n=100, H=16, W=20, C=64, c2=64, O=320, up=1, r1="h"),
    # conv with the stream-K tail and the RES_LDS epilogue
    "G10": dict(kind="conv", tiles=544, per_wg=(3, 3), n=136, H=32, W=32, C=64, O=320, rb_imgs=1, r1="s", split=True,
                schedule="tail", dp_rounds=1, sk_tiles=288),
    # tap mask per tile, nk = 3
    "G11": dict(kind="temporal", tiles=500, per_wg=(1, 2), B=5, T=4, P=6400, C=64, O=320, rb=True, r1="s", split=True),
    # ragged, seams inside tiles
    "G11u": dict(kind="temporal", tiles=501, per_wg=(1, 2), B=5, T=4, P=6403, C=64, O=320, rb=True, r1="h", pieces=False),
    # the 256-wide instance, Downsample2D(padding=0) addressing, nk = 18, stream-K tail (110 images = 550 tiles: 150 images = 750 tiles
    # lose 2.3 % of three rounds and run whole tiles)
    "G12": dict(kind="conv", tiles=550, per_wg=(3, 4), n=110, H=64, W=80, C=128, O=256, stride=2, shift=1,
                schedule="tail", dp_rounds=1, sk_tiles=294),
    # the 256-wide instance on the VAE attention's score schedule (M = N = 9216 there, c_acc = 1 / sqrt(512)): split output WITHOUT a
    # residual (<0, 17>), 20 x 13 tiles in three full bands of 4 columns and a ragged band of one, ragged last row tile
    "G13": dict(kind="dense", tiles=260, per_wg=(1, 2), M=5000, N=3328, K=512, bias=False, split=True, band=4,
                coef=(512 ** -0.5, 1.0, 1.0), epi="<0, 17>"),
    # the 256-wide instance with TWO tile columns and a stream-K tail: the VAE res-block's conv2 (3x3, split r1, <1, 18>); 68 images
    # of 32 x 32 = 272 x 2 tiles: one data-parallel round, 288 tail tiles
    "G14": dict(kind="conv", tiles=544, per_wg=(3, 3), n=68, H=32, W=32, C=64, O=512, r1="s", split=True, epi="<1, 18>",
                schedule="tail", dp_rounds=1, sk_tiles=288),
}


def case_operands(c):
    """the operand set of a case, as gen3_epi / gen3_plan take it"""
    s = set()
    if c.get("rb") or c.get("rb_imgs"):
        s.add("rb")
    if c.get("r1"):
        s.add("r1")
    if c.get("r2"):
        s.add("r2")
    if c.get("split") or "s" in (c.get("r1"), c.get("r2")):
        s.add("lo")
    if c.get("geglu"):
        s.add("geglu")
    return s


def gen3_case_plan(c, G, debug=0, rows=None):
    """gen3_plan of a GEN3_CASES entry (of its first `rows` rows when given)"""
    M, N, K, _, _, _ = case_dims(c)
    return gen3_plan(M if rows is None else rows, N, K, c["kind"], case_operands(c), G, debug)


def gen3_piece_ranges(c, G):
    """Row ranges [(r0, r1)] covering [0, M), or None for a case that cannot tile-align: each starts at a multiple of 256 rows and of
    the case's unit (rows of one image / batch element) and holds at least 200 * G / 256 and at most G tiles, so that plan3 takes
    it and it runs as one round without a tail.  The last range is the last such window that ends at M: it may overlap the one
    before it."""
    if not c.get("pieces", True):
        return None
    M, N, _, _, unit, _ = case_dims(c)
    BM, BN, _, _ = gen3_family(N)
    tiles_n = N // BN
    step = unit * BM // math.gcd(unit, BM)
    lo_tiles = (200 * G + 255) // 256
    lo_rows = (lo_tiles + tiles_n - 1) // tiles_n                   # fewest tile rows of a piece
    rows = G // (step // BM * tiles_n) * step                       # most rows of a piece
    assert rows > 0 and rows // BM >= lo_rows, (rows, step, lo_rows)
    out, r0 = [], 0
    while -(-(M - r0) // BM) * tiles_n > G:
        out.append((r0, r0 + rows))
        r0 += rows
    if -(-(M - r0) // BM) < lo_rows:
        r0 = (M - (lo_rows - 1) * BM - 1) // step * step
    assert r0 >= 0 and lo_rows <= -(-(M - r0) // BM) <= G // tiles_n, (r0, M)
    out.append((r0, M))
    return out


def gen3_rowbias_rows(c, G):
    """rows per row-bias group of a dense GEN3_CASES entry: every piece start is a group start, and groups change inside tiles
    (32 x the odd part of the starts' common divisor)"""
    g = 0
    for r0, _ in gen3_piece_ranges(c, G):
        g = math.gcd(g, r0)
    assert g > 0
    while g % 64 == 0:
        g //= 2
    return g
