"""Case tables, input builders, the fp64 reference and two fp32 restatements for the GroupNorm kernels of csrc/norm.hip.
Shared by tests/test_gpu_groupnorm.py (-m gpu: stats -> finalize -> apply / apply_split through the C ABI into guarded buffers)
and tests/test_cpu_groupnorm_cases.py (-m "not gpu": every case bears its bound without the kernel, and the statistics cases
tell a pivot-on-row-0 summation from one that does not depend on row 0).  A plain module, imported like kernel_checks.

Everything here is torch / numpy and runs on the device of the tensors it is given.

Bounds (worst row of the result against the fp64 reference, kernel_checks.worst_row).  None comes from what a kernel gives:
- split output (y_hi + y_lo) of N(75, 0.25) inputs: 1e-4.  An fp32 mean at 75 has a half-ulp of 3.8e-6 = 1.5e-5 sigma, which every
  element of a row carries; times a margin of about 5 for the fp32 apply arithmetic and SiLU.  Under a third of the fp16 output rounding.
- split output of N(0.3, 1.5) inputs: 1e-5 (the fp32 floor is ~4e-7; the margin leaves room for rsqrtf and the fast exp of SiLU).
- plain fp16 output: 2^-11 + 1e-4 (the fp16 half-ulp, relative, on every element of a row, plus the statistics budget).
test_cpu_groupnorm_cases.py requires the fp32 floor of every case (fp64 statistics rounded to fp32, fp32 apply in the kernel's
evaluation order, split output) to stay at or below one fifth of the case's bound."""
import math
import zlib

import numpy as np
import torch

EPS = 1e-5
DISTS = {"n75": (75.0, 0.25), "n03": (0.3, 1.5)}              # name -> (mean, std)
BOUND_SPLIT = {"n75": 1e-4, "n03": 1e-5}
BOUND_PLAIN = 2.0 ** -11 + 1e-4
GRID = (72, 128)                                               # the 9216 rows of a level-0 slab are a 72 x 128 image
# The statistics cases run without SiLU; the ABI cases run with and without.  SiLU divides a row's norm by about 2 and leaves
# the error that the fp32 mean's rounding puts on every element nearly as it is: with it the fp32 floor of the N(75, 0.25) cases at
# C = 64 (2.1e-5) is no longer under a fifth of their bound, without it the worst of them is 1.7e-5.
STAT_SILU = False

# ------------------------------------------------------------------------------------------------ (a) / (b): statistics cases
# name -> (n_slabs, rows, C); 144, 144 and 10 row chunks
STAT_SHAPES = {"2x9216x64": (2, 9216, 64), "2x9216x320": (2, 9216, 320), "64x9216x64": (64, 9216, 64)}
KINDS = ("alike", "row0_zero", "row0_300", "last_row", "interior_row", "first_line", "border")
STAT_CASES = [(s, d, k) for s in STAT_SHAPES for d in DISTS for k in KINDS]


def row0_alone_atypical(dist, kind, rolled=False):
    """whether row 0 of every slab is far (>> std) from the channel means while the other rows are alike.  (In 'first_line' and
    'border' row 0 is atypical too, but so are 128 / 396 rows: they raise the variance itself by three orders of magnitude, and
    an error of the size that a far pivot causes no longer shows against it.)"""
    if rolled:                                                 # rows move down by one: row 0 is the former last row
        return dist == "n75" and kind == "last_row"
    return kind == "row0_300" or (dist == "n75" and kind == "row0_zero")   # 0 is a typical value of N(0.3, 1.5)


def atypical_rows(kind, rows):
    """(row indices, value) that the kind overwrites in every slab"""
    H, W = GRID
    if kind == "alike":
        return torch.zeros(0, dtype=torch.long), 0.0
    if kind == "row0_zero":
        return torch.tensor([0]), 0.0
    if kind == "row0_300":
        return torch.tensor([0]), 300.0
    if kind == "last_row":
        return torch.tensor([rows - 1]), 0.0
    if kind == "interior_row":
        return torch.tensor([rows // 2 + 37]), 0.0
    if kind == "first_line":
        return torch.arange(W), 0.0
    if kind == "border":
        assert rows == H * W
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        edge = (yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)
        return edge.reshape(-1).nonzero().reshape(-1), 0.0
    raise KeyError(kind)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def stat_noise(shape):
    """standard normal noise [2, rows, C] of a statistics shape: slab i of a case is built from noise[i % 2]"""
    n, rows, C = STAT_SHAPES[shape]
    return torch.randn(2, rows, C, generator=_gen("gn stat " + shape))


def stat_input(noise, shape, dist, kind, slabs=None):
    """fp32 [len(slabs), rows, C]: slab i = mean_i + std * noise[i % 2] with mean_i = mean + std * (i // 2) / 32 (every pair of slabs
    has its own mean; all stay inside the binade of `mean`), then the kind's rows overwritten.  `slabs`: slab indices (default all).
    Runs on the device of `noise`."""
    n, rows, C = STAT_SHAPES[shape]
    mu, sd = DISTS[dist]
    idx = torch.arange(n) if slabs is None else torch.as_tensor(slabs)
    means = (mu + sd * (idx // 2).float() / 32).to(noise.device)
    x = noise[(idx % 2).to(noise.device)] * sd + means[:, None, None]
    r, val = atypical_rows(kind, rows)
    if r.numel():
        x[:, r.to(noise.device)] = val
    return x


def params(C, name="gn"):
    """gamma, beta as fp16 [C]"""
    g = torch.randn(C, generator=_gen(name + " gamma")) * 0.2 + 1
    b = torch.randn(C, generator=_gen(name + " beta")) * 0.1
    return g.half(), b.half()


# ------------------------------------------------------------------------------------------------ operand forms
def split_enc(x):
    """fp32 -> (hi fp16, lo int8): bits(x) ~= bits(float(hi)) + 32 * lo (the residual stream's split form, common.h)"""
    x = x.float().contiguous()
    hi = x.half()
    d = (x.view(torch.int32) - hi.float().view(torch.int32) + 16) >> 5
    return hi, d.clamp_(-128, 127).to(torch.int8)


def split_dec(hi, lo):
    return (hi.float().contiguous().view(torch.int32) + (lo.to(torch.int32) << 5)).view(torch.float32)


def operand(x, split):
    """fp32 x -> (hi, lo or None, the fp32 value a kernel reads from them)"""
    if split:
        hi, lo = split_enc(x)
        return hi, lo, split_dec(hi, lo)
    hi = x.half()
    return hi, None, hi.float()


def split_out(f):
    """fp32 result -> the value of the split operand fp16(f) + fp16(f - fp16(f)), in fp64"""
    hi = f.half()
    return hi.double() + (f - hi.float()).half().double()


# ------------------------------------------------------------------------------------------------ reference
def reference(x, gamma, beta, groups, eps=EPS, silu=True):
    """GroupNorm(+SiLU) in fp64 over x [n_slabs, rows, C_tot] (any float dtype; gamma / beta [C_tot]).
    Returns y [n_slabs * rows, C_tot], mean [n_slabs, groups], biased variance [n_slabs, groups]."""
    n, rows, C = x.shape
    assert C % groups == 0
    xg = x.double().reshape(n, rows, groups, C // groups)
    mean = xg.mean(dim=(1, 3))
    xg = xg - mean[:, None, :, None]
    var = xg.square().mean(dim=(1, 3))
    xg *= (var + eps).rsqrt()[:, None, :, None]
    y = xg.reshape(n * rows, C)
    y = y * gamma.double().to(x.device) + beta.double().to(x.device)
    if silu:
        y = y * torch.sigmoid(y)
    return y, mean, var


def apply_fp32(x, mean, var, gamma, beta, groups, eps=EPS, silu=True):
    """the apply in fp32 in the kernel's evaluation order ((x - mean) * rstd) * gamma + beta, x / (1 + exp(-x)) for SiLU,
    from statistics given in any precision (rounded to fp32 here).  x fp32 [n, rows, C] -> fp32 [n * rows, C]."""
    n, rows, C = x.shape
    gs = C // groups
    m = mean.float().repeat_interleave(gs, dim=1)[:, None, :]
    rstd = (var.float() + torch.tensor(eps, dtype=torch.float32)).rsqrt().repeat_interleave(gs, dim=1)[:, None, :]
    f = ((x.float() - m) * rstd) * gamma.float().to(x.device) + beta.float().to(x.device)
    if silu:
        f = f / (1.0 + torch.exp(-f))
    return f.reshape(n * rows, C)


# ------------------------------------------------------------------------------------------------ the launch geometry, restated
def gn_chunks(n_slabs, rows):
    """row chunks per slab of the statistics launch"""
    want = -(-640 // n_slabs)
    return max(1, min(want, (rows + 63) // 64, 512))


def layout(C_src):
    """(VPP, PL): 8-channel vectors per row and row-lanes per block of the statistics and apply kernels"""
    vpp = C_src // 8
    return vpp, (1 if vpp >= 256 else 256 // vpp)


def workspace_floats(n_slabs, rows, C_tot, groups):
    """a lower bound the library's workspace size has to meet: one (two-float) partial per (slab, chunk, channel) and the
    (mean, variance) pair per (slab, group)"""
    return n_slabs * gn_chunks(n_slabs, rows) * C_tot * 2 + n_slabs * groups * 2


# ------------------------------------------------------------------------------------------------ fp32 restatements of the statistics
_F32, _F64 = np.float32, np.float64


def _fma(a, b, c):
    """fp32 fma(a, b, c): the product is exact in fp64, the sum is rounded to fp64 and then to fp32"""
    return (np.asarray(a, _F64) * np.asarray(b, _F64) + np.asarray(c, _F64)).astype(_F32)


def _wave_sum4(v):
    """v [..., 256] fp32 -> the block total the finalize kernel forms: a xor-butterfly inside each wave of 64, then
    w0 + w1 + w2 + w3"""
    w = v.reshape(v.shape[:-1] + (4, 64)).astype(_F32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lanes ^ o]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _thread_rows(rows, chunks, PL):
    """row index [chunks, steps, PL] that row-lane pl of chunk b reads at its step j, and whether that row exists"""
    rpb = -(-rows // chunks)
    steps = -(-rpb // PL)
    off = np.arange(PL)[None, None, :] + np.arange(steps)[None, :, None] * PL
    r = np.arange(chunks)[:, None, None] * rpb + off
    ok = (off < rpb) & (r < rows)
    return np.where(ok, r, 0), ok


def _per_thread_tid(vec, gs):
    """vec [..., gs] -> [..., 256]: thread tid's sequential sum of the entries tid, tid + 256, ..."""
    out = np.zeros(vec.shape[:-1] + (256,), _F32)
    for c0 in range(0, gs, 256):
        w = min(256, gs - c0)
        out[..., :w] = out[..., :w] + vec[..., c0:c0 + w]
    return out


def _group_combine(mean_c, m2_c, n, groups):
    """per-channel (mean, M2) [C] -> per-group (mean, biased variance) [groups], as the finalize kernel combines a group's channels"""
    C = mean_c.shape[0]
    gs = C // groups
    mc, m2 = mean_c.reshape(groups, gs), m2_c.reshape(groups, gs)
    mean = (_wave_sum4(_per_thread_tid(mc, gs)) / _F32(gs)).astype(_F32)
    d = (mc - mean[:, None]).astype(_F32)
    dev = np.zeros((groups, 256), _F32)
    for c0 in range(0, gs, 256):
        w = min(256, gs - c0)
        dev[:, :w] = _fma(d[:, c0:c0 + w], d[:, c0:c0 + w], dev[:, :w])
    # each wave's leader stores m2 + n * dev of ITS wave; the four are added in order
    def waves(v):
        w = v.reshape(groups, 4, 64).astype(_F32)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[..., lanes ^ o]
        return w[..., 0]
    tot = _fma(_F32(n), waves(dev), waves(_per_thread_tid(m2, gs)))
    tot = ((tot[:, 0] + tot[:, 1]) + tot[:, 2]) + tot[:, 3]
    return mean, (tot / (_F32(n) * _F32(gs))).astype(_F32)


def emulate_row0_pivot_stats(x, groups, n_slabs_launch, Cs=None):
    """fp32 restatement, in its summation order, of GroupNorm statistics from sums shifted by ONE pivot per (slab, channel), the
    value in row 0 of the slab: per thread s = sum(x - K), q = sum((x - K)^2) over the rows r0 + pl, r0 + pl + PL, ... of its chunk;
    the PL row-lanes of a block added in order; per channel the chunks kc, kc + KP, ... added by chunk-lane kc and the KP lanes
    added in order; mean_c = K + s / n, M2_c = q - s * (s / n); then the group's channels.  This is how norm.hip computed its
    statistics until the per-thread pivots; it is kept because it shows, without a GPU, that the (a) / (b) cases tell a
    summation that depends on row 0 from one that does not.
    x: fp32 [n, rows, C_tot] (numpy or torch, the values the kernel reads), n_slabs_launch: the n_slabs of the launch (it sets
    the chunking; x may hold only some of its slabs), Cs: widths of the concat's sources (default one source).
    Returns mean, variance as fp32 numpy [n, groups]."""
    x = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=_F32)
    n, rows, C = x.shape
    chunks = gn_chunks(n_slabs_launch, rows)
    gs = C // groups
    cw = min(gs, 256)
    KP = 256 // cw
    means, vars_ = np.zeros((n, groups), _F32), np.zeros((n, groups), _F32)
    for i in range(n):
        S, Q = np.zeros((chunks, C), _F32), np.zeros((chunks, C), _F32)
        off = 0
        for Cw in (Cs or [C]):
            _, PL = layout(Cw)
            xs = x[i, :, off:off + Cw]
            piv = xs[0]
            r, ok = _thread_rows(rows, chunks, PL)
            s, q = np.zeros((chunks, PL, Cw), _F32), np.zeros((chunks, PL, Cw), _F32)
            for j in range(r.shape[1]):
                f = np.where(ok[:, j, :, None], xs[r[:, j]] - piv, _F32(0)).astype(_F32)
                s = s + f
                q = _fma(f, f, q)
            for k in range(PL):
                S[:, off:off + Cw] = S[:, off:off + Cw] + s[:, k]
                Q[:, off:off + Cw] = Q[:, off:off + Cw] + q[:, k]
            off += Cw
        s_l, q_l = np.zeros((KP, C), _F32), np.zeros((KP, C), _F32)
        for k0 in range(0, chunks, KP):
            m = min(KP, chunks - k0)
            s_l[:m] = s_l[:m] + S[k0:k0 + m]
            q_l[:m] = q_l[:m] + Q[k0:k0 + m]
        s2, q2 = np.zeros(C, _F32), np.zeros(C, _F32)
        for k in range(KP):
            s2, q2 = s2 + s_l[k], q2 + q_l[k]
        d = (s2 / _F32(rows)).astype(_F32)
        mean_c = (x[i, 0] + d).astype(_F32)
        m2_c = np.maximum(_fma(-s2, d, q2), _F32(0))
        means[i], vars_[i] = _group_combine(mean_c, m2_c, rows, groups)
    return means, vars_


def _chan(na, ma, Ma, nb, mb, Mb):
    """Chan's combine of (n, mean, M2) pairs in fp32, the first operand being the accumulated one; nb == 0 leaves it unchanged"""
    nab = (na + nb).astype(_F32)
    w = np.where(nab > 0, nb / np.maximum(nab, _F32(1)), _F32(0)).astype(_F32)
    delta = (mb - ma).astype(_F32)
    mean = _fma(delta, w, ma)
    M2 = _fma((delta * delta).astype(_F32), (na * w).astype(_F32), (Ma + Mb).astype(_F32))
    return nab, mean, M2


def _combine_all(nk, mk, Mk, n, relative=True):
    """Chan's combine of K items at once, in order, along axis 1 (nk [B, K, 1], mk / Mk [B, K, C], n [B, 1] = sum of nk):
    mean = ref + sum n_k (m_k - ref) / n with ref = item 0's mean (relative=False: the means are given relative to a reference
    already and the mean is returned so), M2 = sum (M2_k + n_k (m_k - mean)^2).  n == 0 gives (0, 0)."""
    K = mk.shape[1]
    ref = mk[:, 0] if relative else np.zeros_like(mk[:, 0])
    sd = np.zeros_like(ref)
    for k in range(K):
        sd = sd + (nk[:, k] * (mk[:, k] - ref).astype(_F32)).astype(_F32)
    dm = np.where(n > 0, sd / np.maximum(n, _F32(1)), _F32(0)).astype(_F32)
    M2 = np.zeros_like(ref)
    for k in range(K):
        dk = ((mk[:, k] - ref).astype(_F32) - dm).astype(_F32)
        M2 = M2 + (Mk[:, k] + ((nk[:, k] * dk).astype(_F32) * dk).astype(_F32)).astype(_F32)
    return (ref + dm).astype(_F32), M2.astype(_F32)


def emulate_thread_pivot_stats(x, groups, n_slabs_launch, Cs=None):
    """fp32 restatement of the statistics with one pivot PER THREAD (the thread's own first row) and Chan's combine of
    (n, mean, M2): thread -> the PL row-lanes of a block at once (means relative to row-lane 0's) -> per channel the chunks
    kc, kc + KP, ... pairwise in order, then the KP chunk-lanes at once (means relative to chunk 0's) -> the group's channels:
    what norm.hip does.  Same arguments and results as emulate_row0_pivot_stats."""
    x = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=_F32)
    n, rows, C = x.shape
    chunks = gn_chunks(n_slabs_launch, rows)
    rpb = -(-rows // chunks)
    gs = C // groups
    cw = min(gs, 256)
    KP = 256 // cw
    means, vars_ = np.zeros((n, groups), _F32), np.zeros((n, groups), _F32)
    for i in range(n):
        MB, M2B = np.zeros((chunks, C), _F32), np.zeros((chunks, C), _F32)
        off = 0
        for Cw in (Cs or [C]):
            _, PL = layout(Cw)
            xs = x[i, :, off:off + Cw]
            r, ok = _thread_rows(rows, chunks, PL)
            piv = np.where(ok[:, 0, :, None], xs[r[:, 0]], _F32(0)).astype(_F32)
            s, q = np.zeros((chunks, PL, Cw), _F32), np.zeros((chunks, PL, Cw), _F32)
            for j in range(r.shape[1]):
                f = np.where(ok[:, j, :, None], xs[r[:, j]] - piv, _F32(0)).astype(_F32)
                s = s + f
                q = _fma(f, f, q)
            nt = ok.sum(axis=1).astype(_F32)[:, :, None]                          # rows of each thread
            d = np.where(nt > 0, s / np.maximum(nt, _F32(1)), _F32(0)).astype(_F32)
            mt = (piv + d).astype(_F32)
            m2t = np.maximum(_fma(-s, d, q), _F32(0))
            nblk = np.clip(rows - np.arange(chunks) * rpb, 0, rpb).astype(_F32)[:, None]
            MB[:, off:off + Cw], M2B[:, off:off + Cw] = _combine_all(nt, mt, m2t, nblk)
            off += Cw
        nb = np.clip(rows - np.arange(chunks) * rpb, 0, rpb).astype(_F32)[:, None]  # rows of each chunk: the geometry alone
        ln, lm, lM = np.zeros((KP, 1), _F32), np.zeros((KP, C), _F32), np.zeros((KP, C), _F32)
        ref = MB[0]                                                                # means relative to chunk 0's
        for k0 in range(0, chunks, KP):
            m = min(KP, chunks - k0)
            a, b, c = _chan(ln[:m], lm[:m], lM[:m], nb[k0:k0 + m], (MB[k0:k0 + m] - ref).astype(_F32), M2B[k0:k0 + m])
            ln[:m], lm[:m], lM[:m] = a, b, c
        dm, Ma = _combine_all(ln[None], lm[None], lM[None], np.full((1, 1), rows, _F32), relative=False)
        means[i], vars_[i] = _group_combine((ref + dm[0]).astype(_F32), Ma[0], rows, groups)
    return means, vars_


def rstd_error(var, var_ref, eps=EPS):
    """largest relative error of 1 / sqrt(var + eps) over (slab, group), both in fp64"""
    a = 1.0 / np.sqrt(np.asarray(var, _F64) + eps)
    b = 1.0 / np.sqrt(np.asarray(var_ref, _F64) + eps)
    return float(np.abs(a / b - 1).max())


# ------------------------------------------------------------------------------------------------ (d): shapes the ABI admits
# name -> (n_slabs, rows, groups, source widths)
ABI_CASES = {
    # groups != 32
    "g1 C512": (2, 70, 1, [512]),                  # gs = 512: two finalize passes
    "g2 C640": (2, 70, 2, [640]),                  # gs = 320: ragged second pass
    "g4 C64": (3, 70, 4, [64]),
    "g8 C64": (3, 70, 8, [64]),                    # gs = 8: exactly one vector
    "g16 C960": (2, 70, 16, [960]),                # gs = 60: vectors straddle groups
    "g3 C72": (3, 70, 3, [72]),                    # gs = 24
    # concat seam not on a group boundary
    "seam 40+24 g4": (3, 70, 4, [40, 24]),
    "seam 328+312 g32": (2, 70, 32, [328, 312]),
    # thread-layout edges
    "C8": (3, 300, 4, [8]),                        # VPP 1, PL 256
    "C2048": (2, 70, 32, [2048]),                  # VPP 256, PL 1
    "C2056": (2, 70, 8, [2056]),                   # VPP 257: a 257-thread block
    "C8192": (2, 70, 32, [8192]),                  # VPP 1024; the statistics LDS is exactly 64 KB
    # row-count edges: C = 64 has 32 row-lanes, so 5 rows are fewer rows than row-lanes; 63 / 64 / 65 is the chunk-cap seam
    **{f"rows {r} C64": (3, r, 32, [64]) for r in (1, 5, 63, 64, 65, 127, 129)},
    # around 4 * PL and 8 * PL of the apply kernel: PL = 6 at C = 320
    **{f"rows {r} C320": (2, r, 32, [320]) for r in (23, 24, 25, 47, 48, 49)},
    # chunking edges
    "700 slabs": (700, 70, 32, [64]),              # one chunk per slab
    "40000 rows": (1, 40000, 32, [64]),            # 512 chunks of 79 rows: chunk 511 starts past the last row
}


def abi_input(name):
    """fp32 [n_slabs, rows, C_tot] ~ N(0.3, 1.5) of an ABI case"""
    n, rows, groups, Cs = ABI_CASES[name]
    return torch.randn(n, rows, sum(Cs), generator=_gen("gn abi " + name)) * 1.5 + 0.3


def split_sources(x, Cs):
    """[n, rows, C_tot] -> the concat's sources, each contiguous [n * rows, C_i]"""
    n, rows, _ = x.shape
    out, off = [], 0
    for c in Cs:
        out.append(x[:, :, off:off + c].reshape(n * rows, c).contiguous())
        off += c
    return out


def empty_chunks(n_slabs, rows):
    """chunks of the statistics launch whose first row is past the last row"""
    chunks = gn_chunks(n_slabs, rows)
    rpb = -(-rows // chunks)
    return [b for b in range(chunks) if b * rpb >= rows]


assert math.isclose(BOUND_PLAIN, 5.8828125e-4)
