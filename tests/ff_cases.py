"""Fused feed-forward test helpers shared by test_gpu_ff_fused.py and test_cpu_ff_cases.py (a plain module, imported like
gemm_cases.py and kernel_checks.py).

- FF_CASES + problem(): the per-row cases of ew_ff_geglu320_f16 (csrc/ff_fused.hip, ff320_kernel<LO, R2>): every operand state of
  r1 / r2 / out (none, fp16, split hi + lo8), the three forms the transformer blocks launch, ragged row-bias groups with a bias stride
  wider than the row, the fragment edges of M, and workgroups that chain two and three tiles.  problem() gives run(out_hi, out_lo) for
  the fused kernel, run_twin(out_hi, out_lo) for the two-GEMM path it replaces under generation 1 (independent kernels) and ref(): fp64
  on ALL rows, in row chunks on the device.
- instantiation / case_M / schedule: which <LO, R2> the host picks, the row count of a case at a CU budget of G, and the tiles
  each workgroup chains (tile b, b + G, ...), restated from ew_ff_geglu320_f16.
- piece_ranges / piece_diff: a chained launch cut at multiples of lcm(128, rows_per_group) into pieces of at most G tiles, each the
  same problem on row-offset pointers with one tile per workgroup; a tile's arithmetic does not depend on its place in a chain, so
  whole launch and pieces agree bit for bit.
- staged_w1 / staged_w2 / staged_channel / restated_ff: the kernel's W1 / W2 fragment READ addresses restated from the comments and
  code of ff_fused.hip (not from ops.ff_pack), over the packed byte images; the knobs g_table / swap_vg / xor_rows exist so that
  test_cpu_ff_cases.py can show that a drifted restatement fails.
- vgelu_fp32: numpy fp32 restatement of common.h's ew_vgelu2 (the logistic GEGLU gate).
- gate_problem: one-hot selection weights that put every fp16 gate of [-12, 12] (and +-16, +-100, +-2048) on every hidden unit with
  exact single-term pre-activations.
- WORST_ROW: per-case worst-row bounds, derived from the TWIN's measured error (never from the fused kernel's)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

DEV = "cuda"
C, HID, BM, CH, NCH = 320, 1280, 128, 32, 40
# rel-L2 limits against fp64: fp16 output (test_gpu_ff_fused.py's bound) / split output (the GEMM suites' BOUND_SPLIT)
BOUND, BOUND_SPLIT = 3e-4, 2e-5

# M: rows, or (a, b) for a * G * 128 + b at a CU budget of G.  r1 / r2 / out: None, "h" (fp16) or "s" (split hi + lo8).
# rb: (rows_per_group, ld_rowbias) or None.  coef: (c_acc, c_r1, c_r2).  form: the product call it restates (unet._transformer).
FF_CASES = {
    # the spatial block's feed-forward: residual stream in, residual stream out
    "F1": dict(M=129, r1="s", r2=None, out="s", rb=None, coef=(1.0, 1.0, 0.0), form="s_ff"),
    # ff_in: groups of 37 rows start anywhere in a fragment, the last group has 4 rows, the bias stride is wider than the row
    "F2": dict(M=300, r1="s", r2=None, out="h", rb=(37, 328), coef=(1.0, 1.0, 0.0), form="t_ff_in"),
    # the AlphaBlender epilogue; tile 1 holds 72 rows: its waves (wm) 3 are wholly out of range, wm 2 in one fragment of two
    "F3": dict(M=200, r1="h", r2="s", out="h", rb=None, coef=(0.63, 0.63, 0.37), form="t_ff"),
    # <0, 0>; every row of the tile is clamped to row 0
    "F4": dict(M=1, r1=None, r2=None, out="h", rb=None, coef=(1.0, 0.0, 0.0)),
    # <0, 1>: what level 0 launches without split operands; one bias row per token
    "F5": dict(M=127, r1="h", r2="h", out="h", rb=(1, 320), coef=(1.0, 0.5, -2.0)),
    # the lo plane on the output only
    "F6": dict(M=128, r1=None, r2=None, out="s", rb=None, coef=(-1.5, 0.0, 0.0)),
    # r2_lo without r1; one row-bias group larger than M
    "F7": dict(M=16, r1=None, r2="s", out="s", rb=(1000, 320), coef=(1.0, 0.0, 1.0)),
    # both residuals split; 3 tiles + 1 row
    "F8": dict(M=385, r1="s", r2="s", out="s", rb=(48, 640), coef=(0.8, 1.0, 0.25)),
    # chains: workgroups 0-5 own three tiles, the others two; the last tile holds 77 rows
    "F9": dict(M=(2, 5 * 128 + 77), r1="s", r2=None, out="s", rb=None, coef=(1.0, 1.0, 0.0), form="s_ff"),
    # ... with row-bias groups that cross tile and chain seams
    "F10": dict(M=(2, 5 * 128 + 77), r1="s", r2=None, out="h", rb=(37, 328), coef=(1.0, 1.0, 0.0), form="t_ff_in"),
    # the second tile of workgroup 1 holds one row
    "F11": dict(M=(1, 129), r1="h", r2="s", out="h", rb=None, coef=(0.63, 0.63, 0.37), form="t_ff"),
    # fp16 r1 next to a split r2 with a split out (F3's operands, the remaining state inside LO); 1 tile + 2 rows
    "F12": dict(M=130, r1="h", r2="s", out="s", rb=None, coef=(0.63, 0.63, 0.37)),
}
CHAINED = ("F9", "F10", "F11")

# worst-row bounds per case: (bound, worst row of the TWIN -- the two-GEMM path under generation 1 -- against fp64 measured on an
# MI355X); bound = 2 x that measurement rounded down to two digits (the margin covers the different fp32 summation order), applied
# to the fused kernel and to the twin.  The comment carries both measured figures: rel-L2 / worst row of the twin, then of the fused kernel.
# Where 2 x the twin's worst row lies above the case's rel-L2 limit and the twin's worst row itself below it, the bound is that limit: every
# fp16-output case (worst rows of 2.1e-4 ... 2.5e-4 against 3e-4).  F6 has no residual, so its output is the bare feed-forward and the twin's
# own worst row (3.8e-5) lies above the split-output limit of 2e-5, which binds rel-L2 only: its bound is the 2 x.
# (The fused figures are those of the erf gate; with the fitted logistic of ew_vgelu2 the split-output cases measured rel-L2 6.3e-6 ...
# 8.6e-6 and worst rows of 9.5e-6 ... 3.5e-5, F6 1.5e-4 / 2.4e-4 -- every one above its bound.)
WORST_ROW = {
    "F1": (4e-06, 2.028e-06),  # twin: rel-L2 8.76e-07, worst row 2.028e-06 @ 95; fused: rel-L2 9.04e-07, worst row 2.11e-06 @ 123
    "F2": (0.0003, 0.0002357),  # twin: rel-L2 0.000208, worst row 0.0002357 @ 118; fused: rel-L2 0.000208, worst row 0.0002357 @ 118
    "F3": (0.0003, 0.0002381),  # twin: rel-L2 0.000207, worst row 0.0002381 @ 80; fused: rel-L2 0.000207, worst row 0.0002384 @ 80
    "F4": (0.0003, 0.0002073),  # twin: rel-L2 0.000207, worst row 0.0002073 @ 0; fused: rel-L2 0.000207, worst row 0.000207 @ 0
    "F5": (0.0003, 0.0002327),  # twin: rel-L2 0.000209, worst row 0.0002327 @ 103; fused: rel-L2 0.000209, worst row 0.0002329 @ 103
    "F6": (7.5e-05, 3.769e-05),  # twin: rel-L2 5.65e-06, worst row 3.769e-05 @ 95; fused: rel-L2 6.87e-06, worst row 3.77e-05 @ 95
    "F7": (1.9e-06, 9.704e-07),  # twin: rel-L2 8.58e-07, worst row 9.704e-07 @ 2; fused: rel-L2 9.55e-07, worst row 1.79e-06 @ 8
    "F8": (6.1e-06, 3.058e-06),  # twin: rel-L2 9.03e-07, worst row 3.058e-06 @ 369; fused: rel-L2 8.8e-07, worst row 2.97e-06 @ 209
    "F9": (1.7e-05, 8.821e-06),  # twin: rel-L2 1.01e-06, worst row 8.821e-06 @ 32174; fused: rel-L2 1.01e-06, worst row 8.82e-06 @ 32174
    "F10": (0.0003, 0.0002545),  # twin: rel-L2 0.000208, worst row 0.0002545 @ 18987; fused: rel-L2 0.000208, worst row 0.000254 @ 18987
    "F11": (0.0003, 0.0002483),  # twin: rel-L2 0.000207, worst row 0.0002483 @ 18135; fused: rel-L2 0.000207, worst row 0.0002484 @ 18135
    "F12": (3.4e-06, 1.715e-06),  # twin: rel-L2 8.58e-07, worst row 1.715e-06 @ 95; fused: rel-L2 8.79e-07, worst row 1.98e-06 @ 123
}


def case_M(c, G):
    return c["M"] if isinstance(c["M"], int) else c["M"][0] * G * BM + c["M"][1]


def instantiation(c):
    """(LO, R2) of ff320_kernel<LO, R2> as ew_ff_geglu320_f16 picks it: LO = r1_lo || r2_lo || out_lo, R2 = r2 != NULL"""
    return int("s" in (c["r1"], c["r2"], c["out"])), int(c["r2"] is not None)


def schedule(M, G):
    """[tiles of workgroup b] for b < grid: grid = min(tiles, G), workgroup b owns tiles b, b + G, ..."""
    tiles = -(-M // BM)
    grid = min(tiles, G)
    return [list(range(b, tiles, grid)) for b in range(grid)]


def where_row(r, G):
    """row -> its place in the launch: tile, position in its workgroup's chain, wave row (wm: both waves of the pair hold it), fragment"""
    tile = r // BM
    return f"row {r}: tile {tile}, position {tile // G} in the chain of workgroup {tile % G}, waves wm = {(r % BM) // 32}, row fragment {(r % 32) // 16}"


def piece_ranges(M, G, rpg=None):
    """Row ranges [(r0, r1)] tiling [0, M): each starts at a multiple of lcm(128, rows_per_group) (128 without a row bias) and holds at
    most G tiles, so that launched alone it has one tile per workgroup and its row bias starts at a whole group."""
    unit = BM if rpg is None else BM * rpg // math.gcd(BM, rpg)
    rows = G * BM // unit * unit
    assert rows > 0, (G, unit)
    return [(r0, min(r0 + rows, M)) for r0 in range(0, M, rows)]


def piece_diff(whole, piece, r0, G, limit=4):
    """whole / piece: same-shaped planes (rows [r0, r0 + n) of the whole launch, and the piece launched alone).  Returns (number of
    differing elements, description of the first `limit`: (tile, position in its workgroup's chain, wave, row fragment))."""
    assert whole.shape == piece.shape and whole.dtype == piece.dtype, (whole.shape, piece.shape)
    it = {torch.float16: torch.int16, torch.int8: torch.int8}[whole.dtype]
    d = whole.contiguous().view(it) != piece.contiguous().view(it)
    n = int(d.sum())
    where = []
    for r, col in d.nonzero()[:limit].tolist():
        r += r0
        tile = r // BM
        where.append(f"({r}, {col}): tile {tile}, position {tile // G} in the chain of workgroup {tile % G}, wave ({(r % BM) // 32}, {col // 160}), "
                     f"row fragment {(r % 32) // 16}")
    return n, "; ".join(where)


# ----------------------------------------------------------------------------- operands
def _g(s):
    return torch.Generator().manual_seed(s)


def weights(seed, device=DEV):
    """w1 [2560, 320], b1 [2560], w2 [320, 1280], b2 [320] fp16: uniform in +-1 / sqrt(fan-in), as test_gpu_ff_fused.py draws them"""
    w1 = (torch.rand(2 * HID, C, generator=_g(seed)) * 2 - 1) / C ** 0.5
    b1 = (torch.rand(2 * HID, generator=_g(seed + 1)) * 2 - 1) / C ** 0.5
    w2 = (torch.rand(C, HID, generator=_g(seed + 2)) * 2 - 1) / HID ** 0.5
    b2 = (torch.rand(C, generator=_g(seed + 3)) * 2 - 1) / HID ** 0.5
    return [t.half().to(device) for t in (w1, b1, w2, b2)]


def geglu_interleave(n, device=DEV):
    """row order of the GEGLU up-projection for ew_gemm_f16: value / gate rows interleaved in 16s (unet._pack)"""
    return torch.arange(2 * n, device=device).reshape(2, n // 16, 16).permute(1, 0, 2).reshape(-1)


def _rows(t, r0, r1):
    from evoworld_amd.ops import Res
    if t is None:
        return None
    return Res(t.hi[r0:r1], t.lo[r0:r1]) if isinstance(t, Res) else t[r0:r1]


def _dec64(t):
    from evoworld_amd.ops import Res
    return (t.float() if isinstance(t, Res) else t).double()


class Problem:
    """M, split (hi + lo8 output), x, w1, b1, w2, b2, pack, r1, r2, rb, rpg, ld, coef;
    run(out_hi, out_lo, r0=0, r1=M): the fused kernel on rows [r0, r1) as one launch (out_*: the planes of those rows);
    run_twin(out_hi, out_lo): the two-GEMM path under generation 1; ref(): fp64 [M, 320] on the device"""


def problem(ops, c, G, seed=40, zero=False):
    """Build the operands of FF_CASES entry c on the device: x ~ N(0, 1), weights(), residuals N(0, 1) x 2 (the distributions of
    test_gpu_ff_fused.py), row bias N(0, 1) in all `ld` columns.  zero: x, b1, b2 and the residuals are zeros and row g of the bias
    holds g + 1 (test_rowbias_group_seams); the operand STATES stay the case's."""
    from evoworld_amd import _lib
    p = Problem()
    M = p.M = case_M(c, G)
    p.split = c["out"] == "s"
    p.w1, p.b1, p.w2, p.b2 = weights(seed)
    p.x = torch.randn(M, C, generator=_g(seed + 4)).half().to(DEV)
    if zero:
        p.x, p.b1, p.b2 = torch.zeros_like(p.x), torch.zeros_like(p.b1), torch.zeros_like(p.b2)
    p.pack = ops.ff_pack(p.w1, p.b1, p.w2)

    def residual(kind, s):
        if kind is None:
            return None
        r = torch.zeros(M, C, device=DEV) if zero else (torch.randn(M, C, generator=_g(s)) * 2.0).to(DEV)
        return ops.Res.from_float(r) if kind == "s" else r.half()
    p.r1, p.r2 = residual(c["r1"], seed + 5), residual(c["r2"], seed + 6)
    p.rpg, p.ld = c["rb"] or (1, C)
    p.rb = None
    if c["rb"]:
        n_groups = -(-M // p.rpg)
        p.rb = torch.randn(n_groups, p.ld, generator=_g(seed + 7)).half().to(DEV)
        if zero:
            assert n_groups <= 2048                                   # g + 1 is an fp16 integer
            p.rb[:, :C] = torch.arange(1, n_groups + 1, device=DEV, dtype=torch.float32)[:, None].half()
    p.coef = tuple(float(np.float32(v)) for v in c["coef"])          # the ABI carries them as float
    c_acc, c_r1, c_r2 = p.coef

    def epilogue(r0, r1_):
        assert p.rb is None or r0 % p.rpg == 0
        kw = dict(c_acc=c_acc)
        if p.rb is not None:
            kw.update(rowbias=p.rb[r0 // p.rpg:], rows_per_group=p.rpg, ld_rowbias=p.ld)
        if p.r1 is not None:
            kw.update(r1=_rows(p.r1, r0, r1_), c_r1=c_r1)
        if p.r2 is not None:
            kw.update(r2=_rows(p.r2, r0, r1_), c_r2=c_r2)
        return kw

    def out_of(hi, lo):
        assert (lo is not None) == p.split
        return ops.Res(hi, lo) if p.split else hi

    def run(out_hi, out_lo=None, r0=0, r1_=M):
        ops.ff_geglu320(p.x[r0:r1_], p.pack, p.b2, out_of(out_hi, out_lo), **epilogue(r0, r1_))

    def run_twin(out_hi, out_lo=None):
        lib = _lib.load()
        kw = epilogue(0, M)
        for k in ("r1", "r2"):
            if k in kw:
                kw["ld_" + k] = C
        idx = geglu_interleave(HID)
        gen = lib.ew_get_gemm_generation()
        lib.ew_set_gemm_generation(1)
        try:
            ffh = ops.linear(p.x, p.w1[idx].contiguous(), p.b1[idx].contiguous(), act=ops.ACT_GEGLU)
            ops.linear(ffh, p.w2, p.b2, out=out_of(out_hi, out_lo), **kw)
        finally:
            lib.ew_set_gemm_generation(gen)

    def ref(chunk=8192, fitted=False):
        """fitted: the gate is ew_vgelu2's fitted logistic evaluated in fp64 instead of the erf GELU -- a DIAGNOSTIC reference that
        separates the activation's designed absolute error (2.6e-5) from everything else the kernel does"""
        w1, b1, w2, b2 = p.w1.double(), p.b1.double(), p.w2.double(), p.b2.double()
        out = torch.empty(M, C, dtype=torch.float64, device=DEV)
        act = vgelu_gate64 if fitted else F.gelu
        for r0 in range(0, M, chunk):
            r1_ = min(r0 + chunk, M)
            pre = p.x[r0:r1_].double() @ w1.t() + b1
            hid = (pre[:, :HID] * act(pre[:, HID:])).half().double()         # the hidden activation is an fp16 operand: rounded once
            y = hid @ w2.t() + b2
            if p.rb is not None:
                y = y + p.rb[:, :C].double()[torch.arange(r0, r1_, device=DEV) // p.rpg]
            y = c_acc * y
            if p.r1 is not None:
                y = y + c_r1 * _dec64(_rows(p.r1, r0, r1_))
            if p.r2 is not None:
                y = y + c_r2 * _dec64(_rows(p.r2, r0, r1_))
            out[r0:r1_] = y
        return out
    p.run, p.run_twin, p.ref = run, run_twin, ref
    return p


# ----------------------------------------------------------------------------- the pack, as the kernel reads it
G_TABLE = (0, 2, 3, 1)


def staged_w1(w1p, xor_rows=True):
    """W1s[c][R][k], R the staged row (0..63) of chunk c, k the input channel: FF_W1F reads K-tile k // 64 (8 KB), row R (128 bytes),
    16-byte slot ((k % 64) // 8) ^ (R & 7)"""
    w = torch.as_tensor(w1p).detach().cpu().double().reshape(NCH, C // 64, 64, 8, 8)
    c = torch.arange(NCH)[:, None, None]
    R = torch.arange(64)[None, :, None]
    k = torch.arange(C)[None, None, :]
    return w[c, k // 64, R, ((k % 64) // 8) ^ ((R & 7) if xor_rows else 0), k % 8]


def staged_w2(w2p, g_table=G_TABLE):
    """W2s[c][R2][kk], R2 the staged row (0..319), kk the hidden unit inside chunk c: rd2 reads row R2 (64 bytes), 16-byte slot
    (kk // 8) ^ g[(R2 >> 2) & 3]"""
    w = torch.as_tensor(w2p).detach().cpu().double().reshape(NCH, C, 4, 8)
    c = torch.arange(NCH)[:, None, None]
    R = torch.arange(C)[None, :, None]
    kk = torch.arange(CH)[None, None, :]
    g = torch.tensor(g_table)[(R >> 2) & 3]
    return w[c, R, (kk // 8) ^ g, kk % 8]


def staged_channel():
    """staged row R2 = 16 jj + i of the W2 image -> output channel (the epilogue: accumulator pair q of wave half wn, lane slot fks)"""
    r = torch.arange(C)
    jj, i = r // 16, r % 16
    return (jj >> 1) * 32 + (i >> 2) * 8 + (jj & 1) * 4 + (i & 3)


def lane_hidden_map(swap_vg=False):
    """for hidden unit kk = 8 fks + 4 wn + e of a chunk (the A-fragment k of the down-projection): (value staged row, gate staged row)
    = (32 wn + 4 fks + e, 32 wn + 16 + 4 fks + e)"""
    kk = torch.arange(CH)
    fks, wn, e = kk // 8, (kk % 8) // 4, kk % 4
    rv = 32 * wn + 4 * fks + e
    return (rv + 16, rv) if swap_vg else (rv, rv + 16)


def restated_ff(x, pack, g_table=G_TABLE, swap_vg=False, xor_rows=True):
    """GEGLU(x W1^T + b1) W2^T in fp64 with the exact erf GELU (no fp16 rounding of the hidden activation, no b2), computed from
    the PACKED images through the kernel's read addresses.  x: [m, 320]"""
    w1p, b1p, w2p = pack
    x = torch.as_tensor(x).detach().cpu().double()
    W1s, W2s = staged_w1(w1p, xor_rows), staged_w2(w2p, g_table)
    b1s = torch.as_tensor(b1p).detach().cpu().double().reshape(NCH, 64)            # same staged-row order
    pre = torch.einsum("mk,crk->mcr", x, W1s) + b1s
    rv, rg = lane_hidden_map(swap_vg)
    hid = pre[:, :, rv] * F.gelu(pre[:, :, rg])                                      # [m, chunk, kk]: hidden 32 c + kk
    staged = torch.einsum("mck,crk->mr", hid, W2s)
    out = torch.empty_like(staged)
    out[:, staged_channel()] = staged
    return out


def direct_ff(x, w1, b1, w2):
    x, w1, b1, w2 = (torch.as_tensor(t).detach().cpu().double() for t in (x, w1, b1, w2))
    pre = x @ w1.t() + b1
    return (pre[:, :HID] * F.gelu(pre[:, HID:])) @ w2.t()


# ----------------------------------------------------------------------------- the activation
def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in fp64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def vgelu_fp32(v, g):
    """common.h's ew_vgelu2 in numpy fp32: v * g / (1 + exp2(g * p(min(g^2, 64)))), p the fitted quadratic"""
    v, g = np.asarray(v, dtype=np.float32), np.asarray(g, dtype=np.float32)
    k5, k3, k1 = np.float32(0.0010142630), np.float32(-0.10677572), np.float32(-2.3011212)
    with np.errstate(over="ignore"):
        x2 = np.minimum(g * g, np.float32(64.0))
        p = _fma32(x2, np.broadcast_to(k5, x2.shape), np.broadcast_to(k3, x2.shape))
        p = _fma32(p, x2, np.broadcast_to(k1, x2.shape))
        t = g * p
        d = np.exp2(t).astype(np.float32) + np.float32(1.0)
        r = (np.float32(1.0) / d).astype(np.float32)
        return ((v * g) * r).astype(np.float32)


def vgelu_gate64(g):
    """the fitted gate g / (1 + exp2(g p(min(g^2, 64)))) of ew_vgelu2 evaluated in fp64 (torch; its fp32 constants)"""
    k5, k3, k1 = (float(np.float32(k)) for k in (0.0010142630, -0.10677572, -2.3011212))
    x2 = (g * g).clamp_max(64.0)
    return g / (1.0 + torch.exp2(g * ((x2 * k5 + k3) * x2 + k1)))


def gelu64(g):
    """exact erf GELU in fp64 (numpy in, numpy out)"""
    return F.gelu(torch.as_tensor(np.asarray(g, dtype=np.float64))).numpy()


# ----------------------------------------------------------------------------- gate range
GATE_VALUES = (1.0, -0.5, 3.0, 2.0 ** -10)
BIG_GATES = (16.0, -16.0, 100.0, -100.0, 2048.0, -2048.0)


def gate_grid():
    """every fp16 gate of [-12, 12] (both zeros), then BIG_GATES: fp16 numpy"""
    pos = np.arange(0, 0x4A00 + 1, dtype=np.uint16)                  # 0x4A00 = 12.0
    small = np.concatenate([pos, pos | np.uint16(0x8000)]).view(np.float16)
    assert float(np.abs(small.astype(np.float64)).max()) == 12.0
    return np.concatenate([small, np.array(BIG_GATES, dtype=np.float16)])


def gate_problem():
    """x [rows, 320] fp16 (CPU): channels 160.. hold the gate grid in order, channels ..159 the values (GATE_VALUES, the cycle shifted
    by one per row so that a lane slot sees every value); selection weights: hidden unit j has value x[:, j % 160] and gate
    x[:, 160 + j % 160], b1 = b2 = 0, and W2 of pack b copies hidden unit 320 b + n to output channel n.  So
    out[m, n] = fp16(v * gelu(g)) with v = x[m, n % 160], g = x[m, 160 + n % 160] for every pack, each through other hidden units.
    Returns (x, w1, b1, [w2_b for b in 0..3], b2, v [rows, 160] fp64, g [rows, 160] fp64)."""
    gates = gate_grid()
    rows = -(-len(gates) // 160)
    g = np.zeros(rows * 160, dtype=np.float16)
    g[:len(gates)] = gates
    g = g.reshape(rows, 160)
    idx = (np.arange(rows * 160).reshape(rows, 160) + np.arange(rows)[:, None]) % 4
    v = np.array(GATE_VALUES, dtype=np.float16)[idx]
    x = torch.from_numpy(np.concatenate([v, g], axis=1))
    j = torch.arange(HID)
    w1 = torch.zeros(2 * HID, C, dtype=torch.float16)
    w1[j, j % 160] = 1.0
    w1[HID + j, 160 + j % 160] = 1.0
    w2s = []
    n = torch.arange(C)
    for b in range(4):
        w2 = torch.zeros(C, HID, dtype=torch.float16)
        w2[n, 320 * b + n] = 1.0
        w2s.append(w2)
    return (x, w1, torch.zeros(2 * HID, dtype=torch.float16), w2s, torch.zeros(C, dtype=torch.float16),
            v.astype(np.float64), g.astype(np.float64))


def gate_bound(v, g):
    """(reference v * gelu(g), allowed |error|) for |g| <= 12: 3e-5 |v| (the 2.564e-5 of vgelu_fp32 against the erf GELU plus one ulp each
    of v_exp_f32 and v_rcp_f32, <= 3e-6 at |g| <= 12) + 2^-11 |v gelu(g)| (the one fp16 rounding of the hidden value; the output sum
    has one term) + 2^-25 (half a step of an fp16 subnormal)"""
    ref = v * gelu64(g)
    return ref, 3e-5 * np.abs(v) + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
