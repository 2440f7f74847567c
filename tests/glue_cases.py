"""Case tables, inputs, references and checks for the "glue" kernels: the layout, Euler / CFG, sinusoid and time_conv3 kernels of
elementwise.hip, the three image kernels of clip.hip (blur_axis, bicubic_resize, vit_patchify) and plucker / depth_unproject of
geometry.hip.  Shared by tests/test_gpu_glue_kernels.py (-m gpu: the kernels through the C ABI into guarded buffers) and
tests/test_cpu_glue_cases.py (-m "not gpu": the tables reach what they claim, the references agree with independent
statements, an fp32 emulation of each kernel passes the checks and deliberately wrong restatements fail them).  A plain module,
imported like kernel_checks.

Everything here runs on the CPU in torch / numpy.  Every check takes what a kernel (or an emulation) produced as CPU tensors,
prints one `KCHECK glue ...` line with the measured error against its bound and raises AssertionError when the bound is missed.
The bounds depend on the inputs and the fp64 reference alone, never on what the code under test gives:

- layout kernels, vit_patchify: bit-exact (one fp32 multiply and round-to-nearest-even conversions, which torch's CPU .half() /
  .float() perform identically).
- time_conv3: 16 u (|b_o| + sum |w| |x|), u = 2^-24: the kernel sums at most 13 fp32 terms, each a true product.
- blur_axis: (ksize + 1) u sum |k| |x|: ksize products, ksize sums.
- bicubic_resize: 64 u (|scale_c| sum |cy| |cx| |x| + |shift_c|).  The kernel evaluates the cubic coefficients in fp32, and the
  outer ones cancel (c0(t) -> 0 as t -> 0 from terms of size 6), so a coefficient carries an ABSOLUTE error of a few u whatever
  its size, and an output one of about 4 of them times |x|.  The bound is relative to sum |cy| |cx| |x| >= min |x| (the absolute
  coefficients sum to >= 1 on each axis), so the inputs are kept in [1, 2): no tap is more than twice another, the bound is at
  least 64 u, and an output whose centre pixel happens to be small next to its neighbours cannot fall out of it.  (On [0, 1) data
  the fp32 emulation itself misses the bound at such pixels; on [1, 2) it stays below half of it, test_cpu_glue_cases.py.)
- Euler step: 16 u (|x| + |e|) max(1, |s' - s| / s) on the latents (about 15 roundings, each relative to |x| + |e|), plus the fp16
  half-ulp 2^-11 |ref| + 2^-25 on the next model input.  The bound is relative to |e| of the CFG-combined eps, so the two eps rows
  are built without cancellation in e = u + g (c - u): c = u (1 + r), r in [0, 1), hence |e| = |u| + g |c - u|.
- sinusoid_embed: 6e-4 absolute for |v| <= 127 (half an fp16 ulp below 1 is 2.4e-4; the rest is the fp32 argument v f_j).
- plucker_embed, depth_unproject: the tolerances of the existing tests (5e-6 absolute; rtol = atol = 2e-5) against the numpy
  oracles; geometry.hip is compiled without FMA contraction."""
import itertools
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                                        # fp32 unit roundoff
THREADS = 256                                         # every launch here uses blocks of 256 threads
_INT = {torch.float16: torch.int16, torch.float32: torch.int32}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def bits(t):
    return t.contiguous().view(_INT[t.dtype])


# ------------------------------------------------------------------------------------------------ checks
def check_bound(case, got, ref, bound):
    """per element |got - ref| <= bound (ref, bound fp64); a non-finite element counts as infinitely wrong.  Returns the worst
    err / bound."""
    g = torch.as_tensor(got).double().reshape(-1)
    r, b = ref.reshape(-1), bound.reshape(-1)
    assert g.shape == r.shape == b.shape, (case, g.shape, r.shape, b.shape)
    err = (g - r).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    i = int(ratio.argmax())
    print(f"KCHECK glue {case}: max err/bound {float(ratio[i]):.3f} (err {float(err[i]):.3e}, bound {float(b[i]):.3e}, ref {float(r[i]):.6g}) "
          f"@ element {i} of {g.numel()}")
    assert float(ratio[i]) <= 1.0, f"{case}: element {i}: got {float(g[i])!r}, reference {float(r[i])!r}, bound {float(b[i]):.3e}; " \
                                   f"{int((ratio > 1).sum())} elements over the bound"
    return float(ratio[i])


def check_bits(case, got, ref):
    """got and ref (same dtype) agree bit for bit"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (case, got.dtype, ref.dtype, got.shape, ref.shape)
    bad = bits(got) != bits(ref)
    n = int(bad.sum())
    print(f"KCHECK glue {case}: {n} of {bad.numel()} elements differ (bound 0: bit-exact)")
    if n:
        idx = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{case}: {n} elements differ, first at {idx}: {got[idx].item()!r} vs {ref[idx].item()!r}")
    return 0.0


def check_untouched(case, rows, written, pattern_bits):
    """rows [R, ld]: every column outside the `written` ranges still holds the prefill pattern"""
    keep = torch.ones(rows.shape[1], dtype=torch.bool)
    for a, b in written:
        keep[a:b] = False
    bad = bits(rows)[:, keep] != pattern_bits
    if bool(bad.any()):
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{case}: column {int(keep.nonzero()[c])} of row {r} was written (outside {written}); {int(bad.sum())} such")


# ------------------------------------------------------------------------------------------------ layout kernels
# N, C, H, W, ldc, c_off, split (lo_off, dup_off) or None, scale.  *_2pass: 5 x 513 x 512 = 1 313 280 pixels; image 4 starts at pixel
# 1 050 624, so the second trip of the grid-stride loop (from pixel 1 048 576) begins in image 3 and crosses into image 4.
LAYOUT_FWD = [
    dict(name="fwd-1x1", N=1, C=1, H=1, W=1, ldc=8, c_off=7, split=None, scale=1.0),
    dict(name="fwd-c18-off0", N=3, C=18, H=7, W=9, ldc=64, c_off=0, split=None, scale=0.5),
    dict(name="fwd-c18-off46", N=3, C=18, H=7, W=9, ldc=64, c_off=46, split=None, scale=0.5),
    dict(name="split-c14", N=3, C=14, H=7, W=9, ldc=64, c_off=4, split=(20, 40), scale=0.5),
    dict(name="fwd_2pass", N=5, C=2, H=513, W=512, ldc=8, c_off=3, split=None, scale=0.18215),
    dict(name="split_2pass", N=5, C=2, H=513, W=512, ldc=12, c_off=1, split=(3, 6), scale=0.18215),
]
LAYOUT_BWD = [
    dict(name="bwd-1x1", N=1, C=1, H=1, W=1, ldc=8),
    dict(name="bwd-c18", N=3, C=18, H=7, W=9, ldc=64),
    dict(name="bwd_2pass", N=5, C=3, H=513, W=512, ldc=8),
]
# values (after the scale) at the edges of the fp16 conversion: +-0, results that round to fp16 subnormals (2^-25 is the tie to
# zero, 2^-24 the smallest subnormal), the round-to-nearest boundary to inf (65519 -> 65504, 65520 -> inf) and beyond it
LAYOUT_SPECIALS = [0.0, -0.0, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -24, -1.5 * 2.0 ** -24, 3.1e-5, -6.0e-5, 6.1e-5, 1e-8, 65519.0, 65520.0,
                   -65519.0, -70000.0, 65504.0, 1.0009765625, 1.00048828125]


def layout_fwd_input(case):
    n = case["N"] * case["C"] * case["H"] * case["W"]
    x = (torch.randn(n, generator=_gen(case["name"])) * 3.0).float()
    sp = torch.tensor(LAYOUT_SPECIALS, dtype=torch.float64)
    if case["scale"] in (1.0, 0.5):                   # a power of two: special / scale is exact, the kernel's product gives the special back
        sp = sp / case["scale"]
    xn = x.numpy()                                     # (shares x's memory; numpy's indexed assignment keeps the last of repeated positions)
    xn[(np.arange(4 * len(sp)) * 37 + 5) % n] = np.tile(sp.float().numpy(), 4)             # each special at several pixels and channels
    return x.reshape(case["N"], case["C"], case["H"], case["W"])


def layout_fwd_blocks(case):
    """[(name, first column)] of the channel blocks the kernel writes"""
    c0 = case["c_off"]
    if case["split"] is None:
        return [("hi", c0)]
    return [("hi", c0), ("lo", case["split"][0] + c0), ("dup", case["split"][1] + c0)]


def layout_fwd_ref(case, x):
    """{hi, lo, dup}: fp16 [N*H*W, C] -- hi = fp16(scale x), lo = fp16(v - hi), dup = fp16(hi 2^-10), in fp32 like the kernel"""
    v = (x * torch.tensor(case["scale"], dtype=torch.float32)).permute(0, 2, 3, 1).reshape(-1, case["C"])
    hi = v.half()
    return {"hi": hi, "lo": (v - hi.float()).half(), "dup": (hi.float() * 2.0 ** -10).half()}


def layout_fwd_emulate(case, x, pattern_bits, lo_ignores_c_off=False):
    """the rows the kernel leaves in a buffer prefilled with pattern_bits; lo_ignores_c_off: the WRONG lo block [lo_off, +C)"""
    ref = layout_fwd_ref(case, x)
    rows = torch.full((x.shape[0] * x.shape[2] * x.shape[3], case["ldc"]), pattern_bits, dtype=torch.int16).view(torch.float16)
    for name, c0 in layout_fwd_blocks(case):
        if name == "lo" and lo_ignores_c_off:
            c0 = case["split"][0]
        rows[:, c0: c0 + case["C"]] = ref[name]
    return rows


def check_layout_fwd(case, rows, x, pattern_bits):
    ref = layout_fwd_ref(case, x)
    C = case["C"]
    blocks = layout_fwd_blocks(case)
    for name, c0 in blocks:
        check_bits(f"layout {case['name']} {name}", rows[:, c0: c0 + C], ref[name])
    check_untouched(f"layout {case['name']}", rows, [(c0, c0 + C) for _, c0 in blocks], pattern_bits)


def finite_f16_patterns():
    p = np.arange(65536, dtype=np.uint32)
    return p[(p & 0x7C00) != 0x7C00].astype(np.uint16)     # 63 488 patterns: exponent 31 (inf, NaN) left out


def layout_bwd_input(case):
    """fp16 [N*H*W, ldc]: columns [0, C) cycle through a fixed shuffle of every finite fp16 bit pattern (subnormals and -0
    included), the columns past C hold other finite values that must not reach the output"""
    rows, C, ldc = case["N"] * case["H"] * case["W"], case["C"], case["ldc"]
    rng = _rng(case["name"])
    pat = rng.permutation(finite_f16_patterns())
    x = rng.permutation(finite_f16_patterns())[np.arange(rows * ldc) % 63488].reshape(rows, ldc)
    x[:, :C] = np.resize(pat, rows * C).reshape(rows, C)
    return torch.from_numpy(x.view(np.int16).copy()).view(torch.float16)


def layout_bwd_ref(case, x):
    N, C, HW = case["N"], case["C"], case["H"] * case["W"]
    return x[:, :C].float().reshape(N, HW, C).permute(0, 2, 1).contiguous()     # [N, C, HW]


# ------------------------------------------------------------------------------------------------ Euler / CFG step
EULER_SIGMAS = [(700.0, 421.569), (421.569, 322.454), (1.3, 0.4), (0.0108, 0.002), (0.002, 0.0)]    # the last one: the final step
EULER_CASES = [dict(name="euler-t1-ld8", T=1, h=3, w=5, ld_eps=8, cpad=4, split=None, sigma=1.3, sigma_next=0.4)]
for _s, _sn in EULER_SIGMAS:
    EULER_CASES.append(dict(name=f"euler-plain-{_s:g}-{_sn:g}", T=5, h=8, w=16, ld_eps=4, cpad=64, split=None, sigma=_s, sigma_next=_sn))
    EULER_CASES.append(dict(name=f"euler-split-{_s:g}-{_sn:g}", T=5, h=8, w=16, ld_eps=4, cpad=64, split=(20, 40), sigma=_s, sigma_next=_sn))
# 5 x 513 x 512 pixels: the second trip (from pixel 1 048 576) begins in frame 3 and crosses into frame 4 (guidance[t], latents plane)
EULER_CASES.append(dict(name="euler-plain_2pass", T=5, h=513, w=512, ld_eps=4, cpad=4, split=None, sigma=421.569, sigma_next=322.454))
EULER_CASES.append(dict(name="euler-split_2pass", T=5, h=513, w=512, ld_eps=4, cpad=12, split=(4, 8), sigma=1.3, sigma_next=0.4))


def euler_input(case):
    """(eps fp16 [2*T*h*w, ld_eps], latents fp32 [T, 4, h*w], guidance fp32 [T]); eps columns past 4 are NaN: they must not be read"""
    T, HW, ld = case["T"], case["h"] * case["w"], case["ld_eps"]
    g = _gen(case["name"])
    u = torch.randn(T * HW, 4, generator=g)
    c = u * (1.0 + torch.rand(T * HW, 4, generator=g))          # same sign, |c| >= |u|: no cancellation in u + g (c - u)
    eps = torch.full((2 * T * HW, ld), float("nan"), dtype=torch.float16)
    eps[: T * HW, :4] = u.half()
    eps[T * HW:, :4] = c.half()
    lat = (torch.randn(T, 4, HW, generator=g) * math.sqrt(case["sigma"] ** 2 + 1.0)).float()
    return eps, lat, torch.linspace(1, 3, T)


def euler_blocks(case):
    return [("hi", 0)] if case["split"] is None else [("hi", 0), ("lo", case["split"][0]), ("dup", case["split"][1])]


def euler_ref(case, eps, lat, guid):
    """fp64: latents_new [T,4,HW], its bound, next_in value [T*HW, 4] (before the fp16 rounding), its bound"""
    T, HW = case["T"], case["h"] * case["w"]
    s, sn = float(np.float32(case["sigma"])), float(np.float32(case["sigma_next"]))     # the kernel receives fp32 sigmas
    e = eps[:, :4].double().reshape(2, T, HW, 4).permute(0, 1, 3, 2)                      # [2, T, 4, HW]
    e = e[0] + guid.double().view(T, 1, 1) * (e[1] - e[0])
    x = lat.double()
    x0 = e * (-s / math.sqrt(s * s + 1.0)) + x / (s * s + 1.0)
    xn = x + (x - x0) / s * (sn - s)
    b_lat = 16 * U * (x.abs() + e.abs()) * max(1.0, abs(sn - s) / s)
    nin = (xn / math.sqrt(sn * sn + 1.0)).permute(0, 2, 1).reshape(T * HW, 4)
    b_nin = 2.0 ** -11 * nin.abs() + 2.0 ** -25 + b_lat.permute(0, 2, 1).reshape(T * HW, 4)
    return xn, b_lat, nin, b_nin


def euler_emulate(case, eps, lat, guid, pattern_bits, guidance_by_pixel=False):
    """numpy fp32 in the kernel's operation order -> (latents_new fp32 [T,4,HW], next_in fp16 [2*T*HW, cpad] in a buffer prefilled
    with pattern_bits).  guidance_by_pixel: the WRONG index guidance[i % T] of the flat pixel index."""
    f32 = np.float32
    T, HW, cpad = case["T"], case["h"] * case["w"], case["cpad"]
    s, sn = f32(case["sigma"]), f32(case["sigma_next"])
    s2p1 = s * s + f32(1)
    c_out = -s / np.sqrt(s2p1)
    dt = sn - s
    in_scale = f32(1) / np.sqrt(sn * sn + f32(1))
    e16 = eps[:, :4].numpy().reshape(2, T, HW, 4)
    u, cn = e16[0].astype(f32), e16[1].astype(f32)
    gv = guid.numpy().astype(f32)
    g = gv[np.arange(T * HW) % T].reshape(T, HW, 1) if guidance_by_pixel else gv.reshape(T, 1, 1)
    e = u + g * (cn - u)
    x = lat.numpy().transpose(0, 2, 1)                                                    # [T, HW, 4]
    x0 = e * c_out + x / s2p1
    d = (x - x0) / s
    xn = x + d * dt
    assert xn.dtype == f32
    v = xn * in_scale
    o = v.astype(np.float16)
    ol = (v - o.astype(f32)).astype(np.float16)
    od = (o.astype(f32) * f32(2.0 ** -10)).astype(np.float16)
    rows = torch.full((2 * T * HW, cpad), pattern_bits, dtype=torch.int16).view(torch.float16)
    for (name, c0), val in zip(euler_blocks(case), (o, ol, od)):
        blk = torch.from_numpy(val.reshape(T * HW, 4))
        rows[: T * HW, c0: c0 + 4] = blk
        rows[T * HW:, c0: c0 + 4] = blk
    return torch.from_numpy(np.ascontiguousarray(xn.transpose(0, 2, 1))), rows


def check_euler(case, lat_new, rows, eps, lat, guid, pattern_bits):
    """returns (worst latents ratio, worst next_in ratio)"""
    T, HW, name = case["T"], case["h"] * case["w"], case["name"]
    xn, b_lat, nin, b_nin = euler_ref(case, eps, lat, guid)
    r_lat = check_bound(f"{name} latents", lat_new, xn, b_lat)
    blocks = dict(euler_blocks(case))
    both = rows.reshape(2, T * HW, case["cpad"])
    check_bits(f"{name} CFG rows", both[0], both[1])                                      # whole rows: prefill columns included
    hi = both[0][:, 0:4]
    r_nin = check_bound(f"{name} next_in", hi, nin, b_nin)
    if case["split"] is not None:
        lo, dup = both[0][:, blocks["lo"]: blocks["lo"] + 4], both[0][:, blocks["dup"]: blocks["dup"] + 4]
        check_bits(f"{name} dup", dup, (hi.float() * 2.0 ** -10).half())
        rel = float(((hi.double() + lo.double()) - nin).norm() / nin.norm())
        print(f"KCHECK glue {name} hi+lo: rel-L2 {rel:.3e} (bound 3.0e-06)")
        assert rel < 3e-6, (name, rel)
    check_untouched(name, rows, [(c0, c0 + 4) for c0 in blocks.values()], pattern_bits)
    return r_lat, r_nin


# ------------------------------------------------------------------------------------------------ time_conv3
TCONV_CASES = [dict(name=f"tconv-b{B}t{T}-c{C}-hw{HW}", B=B, T=T, C=C, HW=HW)
               for (B, T), C, HW in itertools.product([(1, 1), (1, 2), (3, 5)], [1, 2, 3, 4], [4, 36])]
# 21 frames x 210 000 four-pixel groups = 4 410 000 > 16384 x 256 = 4 194 304: the second trip starts at the end of frame 19
# (b = 2, t = 5) and covers frame 20 (b = 2, t = T - 1: the zero padding after the last frame)
TCONV_CASES.append(dict(name="tconv_2pass", B=3, T=7, C=2, HW=840_000))


def tconv_input(case):
    B, T, C, HW = case["B"], case["T"], case["C"], case["HW"]
    g = _gen(case["name"])
    return torch.randn(B, T, C, HW, generator=g), torch.randn(C, C, 3, generator=g) * 0.5, torch.randn(C, generator=g)


def _tconv(x, w, bias):
    """Conv3d(C, C, (3,1,1), padding (1,0,0)) on [B,T,C,HW]"""
    C = x.shape[2]
    y = F.conv3d(x.permute(0, 2, 1, 3).unsqueeze(-1), w.reshape(C, C, 3, 1, 1), bias, padding=(1, 0, 0))
    return y.squeeze(-1).permute(0, 2, 1, 3).contiguous()


def tconv_ref(x, w, bias):
    """fp64 (y, bound); the bound's second term is the same convolution on absolute values"""
    y = _tconv(x.double(), w.double(), bias.double())
    mag = _tconv(x.double().abs(), w.double().abs(), bias.double().abs())               # |b_o| + sum |w| |x|
    return y, 16 * U * mag


def tconv_emulate(x, w, bias, pad_from_neighbour=False):
    """numpy fp32, the kernel's accumulation order (bias, then c outer, kt inner).  pad_from_neighbour: the WRONG padding that
    reads frame bt - 1 / bt + 1 of the flat [B*T] axis across a batch boundary (zero only at the two ends of the buffer)."""
    B, T, C, HW = x.shape
    xn, wn, bn = x.numpy(), w.numpy(), bias.numpy()
    if pad_from_neighbour:
        flat = np.concatenate([np.zeros((1, C, HW), np.float32), xn.reshape(B * T, C, HW), np.zeros((1, C, HW), np.float32)])
        taps = [flat[kt: kt + B * T].reshape(B, T, C, HW) for kt in range(3)]
    else:
        pad = np.zeros((B, T + 2, C, HW), np.float32)
        pad[:, 1: T + 1] = xn
        taps = [pad[:, kt: kt + T] for kt in range(3)]
    y = np.empty_like(xn)
    for o in range(C):
        acc = np.full((B, T, HW), bn[o], np.float32)
        for c in range(C):
            for kt in range(3):
                acc = acc + wn[o, c, kt] * taps[kt][:, :, c]
        y[:, :, o] = acc
    return torch.from_numpy(y)


def check_tconv(case, y, x, w, bias):
    ref, bound = tconv_ref(x, w, bias)
    return check_bound(case["name"], y, ref, bound)


# ------------------------------------------------------------------------------------------------ blur_axis
BLUR_KN = [(1, 1), (2, 2), (3, 2), (4, 3), (7, 4), (8, 5), (7, 30)]      # (ksize, n along the blurred axis); the kernel needs ksize // 2 < n
BLUR_CASES = [dict(name=f"blur-axis{a}-k{k}-n{n}", axis=a, ksize=k, planes=3, H=n if a == 0 else 5, W=5 if a == 0 else n)
              for a in (0, 1) for k, n in BLUR_KN]
# 5 x 650 x 650 = 2 112 500 > 8192 x 256 = 2 097 152: the second trip is rows 626..649 of plane 4, the reflect at a plane's last rows
BLUR_CASES += [dict(name=f"blur-axis{a}_2pass", axis=a, ksize=7, planes=5, H=650, W=650) for a in (0, 1)]


def blur_input(case):
    g = _gen(case["name"])
    x = torch.randn(case["planes"], case["H"], case["W"], generator=g)
    kern = torch.rand(case["ksize"], generator=g) + 0.1 * torch.arange(1, case["ksize"] + 1)     # not symmetric, not normalised
    return x, kern


def blur_apply(x, kern, axis, dtype=torch.float64, flip=False, pad_front=None, mode="reflect"):
    """F.pad(mode, (pad_front, ksize - 1 - pad_front)) then correlation, sequential sum over the taps, in `dtype` -> (out, sum |k| |x|).
    The keyword arguments state the deliberately WRONG variants (flipped kernel, pad_front = ksize // 2, edge repeat)."""
    k = kern.shape[0]
    pf = (k - 1) // 2 if pad_front is None else pad_front
    xs = x.to(dtype).transpose(1, 2) if axis == 0 else x.to(dtype)                        # blurred axis last
    n = xs.shape[-1]
    xp = F.pad(xs, (pf, k - 1 - pf), mode=mode)
    kk = kern.to(dtype).flip(0) if flip else kern.to(dtype)
    out, mag = torch.zeros_like(xs), torch.zeros_like(xs)
    for j in range(k):
        out = out + kk[j] * xp[..., j: j + n]
        mag = mag + kk[j].abs() * xp[..., j: j + n].abs()
    if axis == 0:
        out, mag = out.transpose(1, 2), mag.transpose(1, 2)
    return out.contiguous(), mag.contiguous()


def blur_ref(case, x, kern):
    out, mag = blur_apply(x, kern, case["axis"])
    return out, (case["ksize"] + 1) * U * mag


def blur_double_loop(x, kern, axis):
    """the reference written out index by index (torch 'reflect': no edge repeat)"""
    P, H, W = x.shape
    k = kern.shape[0]
    pf = (k - 1) // 2
    out = np.zeros((P, H, W))
    xn, kn = x.double().numpy(), kern.double().numpy()
    n = H if axis == 0 else W
    for p, y, xw in itertools.product(range(P), range(H), range(W)):
        for j in range(k):
            i = (y if axis == 0 else xw) + j - pf
            i = -i if i < 0 else i
            i = 2 * (n - 1) - i if i >= n else i
            out[p, y, xw] += kn[j] * (xn[p, i, xw] if axis == 0 else xn[p, y, i])
    return torch.from_numpy(out)


def check_blur(case, out, x, kern):
    ref, bound = blur_ref(case, x, kern)
    return check_bound(case["name"], out, ref, bound)


# ------------------------------------------------------------------------------------------------ bicubic_resize
BICUBIC_SHAPES = [(1, 1, 3, 4), (2, 9, 1, 1), (5, 7, 13, 9), (64, 64, 7, 5), (6, 10, 6, 10), (576, 1024, 224, 224)]   # H, W -> Ho, Wo
BICUBIC_CASES = []
for _H, _W, _Ho, _Wo in BICUBIC_SHAPES:
    BICUBIC_CASES.append(dict(name=f"bicubic-{_H}x{_W}-{_Ho}x{_Wo}-c3-affine", N=2, C=3, H=_H, W=_W, Ho=_Ho, Wo=_Wo, affine=True))
    BICUBIC_CASES.append(dict(name=f"bicubic-{_H}x{_W}-{_Ho}x{_Wo}-c1", N=2, C=1, H=_H, W=_W, Ho=_Ho, Wo=_Wo, affine=False))
# 3 x 840 x 840 = 2 116 800 outputs > 2 097 152: the second trip lies in channel 2 (scale[2], shift[2], the last plane's last rows)
BICUBIC_CASES.append(dict(name="bicubic_2pass", N=1, C=3, H=64, W=64, Ho=840, Wo=840, affine=True))


def bicubic_input(case):
    """(x fp32 [N,C,H,W] in [1, 2), scale [C] or None, shift [C] or None); the affine is CLIP's normalisation, per channel"""
    g = _gen(case["name"])
    x = torch.rand(case["N"], case["C"], case["H"], case["W"], generator=g) + 1.0
    if not case["affine"]:
        return x, None, None
    mean, std = torch.tensor([0.48145466, 0.4578275, 0.40821073]), torch.tensor([0.26862954, 0.26130258, 0.27577711])
    return x, (1.0 / std).float()[: case["C"]].contiguous(), (-mean / std).float()[: case["C"]].contiguous()


def bicubic_index(n, no, align_corners=True):
    """torch's fp32 source index: (first tap's centre i = floor(r) as int64 [no], t = r - i as fp32 [no]).  align_corners=False is
    the WRONG variant."""
    f32 = np.float32
    o = np.arange(no, dtype=f32)
    if align_corners:
        s = f32(n - 1) / f32(no - 1) if no > 1 else f32(0)
        r = s * o
    else:
        r = (o + f32(0.5)) * (f32(n) / f32(no)) - f32(0.5)
    assert r.dtype == f32
    i = np.floor(r)
    return i.astype(np.int64), r - i


def cubic_coeffs(t, dtype):
    """torch upsample_bicubic2d coefficients, A = -0.75, in `dtype` in the kernel's expression order -> [len(t), 4]"""
    t = t.astype(dtype)
    A, one, two = dtype(-0.75), dtype(1), dtype(2)
    x1, x2, x3, x4 = t + one, t, one - t, two - t

    def outer(x):
        return ((A * x - dtype(5) * A) * x + dtype(8) * A) * x - dtype(4) * A

    def inner(x):
        return ((A + two) * x - (A + dtype(3))) * x * x + one
    return np.stack([outer(x1), inner(x2), inner(x3), outer(x4)], 1)


def _bicubic_planes(x, iy, cy, ix, cx):
    """x [P,H,W]; taps clamped; inner sum over x, outer over y, each sequential from zero like the kernel, in x's dtype"""
    P, H, W = x.shape
    xx = np.clip(ix[:, None] + np.arange(-1, 3), 0, W - 1)                                # [Wo, 4]
    yy = np.clip(iy[:, None] + np.arange(-1, 3), 0, H - 1)                                # [Ho, 4]
    rows = np.zeros((P, H, len(ix)), x.dtype)
    for b in range(4):
        rows = rows + cx[:, b] * x[:, :, xx[:, b]]
    out = np.zeros((P, len(iy), len(ix)), x.dtype)
    for a in range(4):
        out = out + cy[:, a][None, :, None] * rows[:, yy[:, a], :]
    return out


def bicubic_apply(case, x, scale, shift, dtype=np.float64, align_corners=True, affine_by_image=False):
    """-> (out [N,C,Ho,Wo], sum |cy| |cx| |x|) in `dtype`: fp32 index (bicubic_index), then coefficients, sums and affine in `dtype`.
    dtype = np.float32 is the emulation of the kernel.  align_corners=False and affine_by_image (channel pl // C) are WRONG variants."""
    N, C, H, W, Ho, Wo = (case[k] for k in ("N", "C", "H", "W", "Ho", "Wo"))
    iy, ty = bicubic_index(H, Ho, align_corners)
    ix, tx = bicubic_index(W, Wo, align_corners)
    cy, cx = cubic_coeffs(ty, dtype), cubic_coeffs(tx, dtype)
    xp = x.numpy().reshape(N * C, H, W).astype(dtype)
    out = _bicubic_planes(xp, iy, cy, ix, cx)
    mag = _bicubic_planes(np.abs(xp), iy, np.abs(cy), ix, np.abs(cx))
    if scale is not None:
        pl = np.arange(N * C)
        c = pl // C if affine_by_image else pl % C
        sc, sh = scale.numpy().astype(dtype)[c % C], shift.numpy().astype(dtype)[c % C]
        out = out * sc[:, None, None] + sh[:, None, None]
    assert out.dtype == dtype
    return torch.from_numpy(out.reshape(N, C, Ho, Wo)), torch.from_numpy(mag.reshape(N, C, Ho, Wo))


def bicubic_ref(case, x, scale, shift):
    out, mag = bicubic_apply(case, x, scale, shift)
    C = case["C"]
    sc = scale.double().abs().view(1, C, 1, 1) if scale is not None else 1.0
    sh = shift.double().abs().view(1, C, 1, 1) if shift is not None else 0.0
    return out, 64 * U * (sc * mag + sh)


def check_bicubic(case, out, x, scale, shift):
    ref, bound = bicubic_ref(case, x, scale, shift)
    r = check_bound(case["name"], out, ref, bound)
    if (case["Ho"], case["Wo"]) == (case["H"], case["W"]) and scale is None:              # every coefficient is exactly 0 or 1 in fp32
        assert torch.equal(torch.as_tensor(out).reshape(x.shape), x), f"{case['name']}: the identity resize must return the input exactly"
    return r


# ------------------------------------------------------------------------------------------------ vit_patchify
PATCHIFY_CASES = [dict(name=f"patchify-s{S}-p{P}-ld{ldk}", N=2, S=S, P=P, ldk=ldk)
                  for S, P, ldk in [(4, 4, 48), (8, 1, 8), (28, 14, 592), (28, 14, 640), (224, 14, 640)]]
# 16 x 256 rows x 640 = 2 621 440 > 2 097 152: the second trip starts in row 3276 (image 12) and runs through images 13..15
PATCHIFY_CASES.append(dict(name="patchify_2pass", N=16, S=224, P=14, ldk=640))


def patchify_input(case):
    return (torch.randn(case["N"], 3, case["S"], case["S"], generator=_gen(case["name"])) * 3.0).float()


def patchify_ref(case, x, k_order="c,ky,kx"):
    """fp16 [N*(S/P)^2, ldk]: F.unfold's K order is (c, ky, kx); columns [3 P^2, ldk) are zero.  k_order 'ky,kx,c' is the WRONG one."""
    P, K = case["P"], 3 * case["P"] ** 2
    cols = F.unfold(x, P, stride=P).transpose(1, 2)                                        # [N, G*G, 3*P*P]
    if k_order == "ky,kx,c":
        cols = cols.reshape(cols.shape[0], cols.shape[1], 3, P * P).transpose(2, 3)
    else:
        assert k_order == "c,ky,kx"
    out = torch.zeros(cols.shape[0] * cols.shape[1], case["ldk"], dtype=torch.float16)
    out[:, :K] = cols.reshape(-1, K).half()
    return out


def patchify_explicit(case, x):
    """the same rows by explicit indexing (small cases)"""
    N, S, P, ldk = case["N"], case["S"], case["P"], case["ldk"]
    G = S // P
    out = torch.zeros(N * G * G, ldk, dtype=torch.float16)
    for n, gy, gx, c, ky, kx in itertools.product(range(N), range(G), range(G), range(3), range(P), range(P)):
        out[(n * G + gy) * G + gx, (c * P + ky) * P + kx] = x[n, c, gy * P + ky, gx * P + kx].half()
    return out


def check_patchify(case, out, x):
    return check_bits(case["name"], out, patchify_ref(case, x))


# ------------------------------------------------------------------------------------------------ sinusoid_embed
SINUSOID_VALUES = [0.0, 0.7, -0.7, 1.6377, 6.0, 24.0, 127.0]
SINUSOID_CASES = [dict(name=f"sinusoid-{nv}-{nr}-{dim}", n_vals=nv, n_rows=nr, dim=dim)
                  for nv, nr, dim in [(1, 1, 2), (3, 7, 64), (6, 6, 256), (1, 5, 1280), (4, 3, 320)]]


def sinusoid_input(case):
    k = SINUSOID_CASES.index(case)
    return torch.tensor([SINUSOID_VALUES[(3 * k + 2 * j + 3) % len(SINUSOID_VALUES)] for j in range(case["n_vals"])], dtype=torch.float32)


def sinusoid_ref(case, vals):
    half = case["dim"] // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = vals.double()[torch.arange(case["n_rows"]) % case["n_vals"]].view(-1, 1) * f[None]
    return torch.cat([torch.cos(a), torch.sin(a)], 1)


def check_sinusoid(case, out, vals):
    ref = sinusoid_ref(case, vals)
    return check_bound(case["name"], out, ref, torch.full_like(ref, 6e-4))


# ------------------------------------------------------------------------------------------------ plucker_embed, depth_unproject
# plucker_2pass: 9 x 480 x 512 = 2 211 840 > 2 097 152: the second trip lies in image 8.  unproject_2pass: 5 x 650 x 650 = 2 112 500:
# the second trip lies in view 4 (extr + 4 * 12, intr + 4 * 9)
PLUCKER_CASES = [dict(name="plucker-1x1", N=1, H=1, W=1), dict(name="plucker-5x7", N=3, H=5, W=7), dict(name="plucker_2pass", N=9, H=480, W=512)]
UNPROJECT_CASES = [dict(name="unproject-5x7", S=3, H=5, W=7), dict(name="unproject_2pass", S=5, H=650, W=650)]


def _poses(n, rng):
    """[n, 3, 4] float32: a different rotation and translation each"""
    out = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        out[i, :, :3] = q
        out[i, :, 3] = rng.normal(size=3) * (1.0 + 0.3 * i)
    return out


def plucker_input(case):
    """(rays fp32 [H,W,3] unit directions, c2w fp32 [N,3,4])"""
    rng = _rng(case["name"])
    d = rng.normal(size=(case["H"], case["W"], 3))
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32), _poses(case["N"], rng)


def plucker_ref(rays, c2w):
    """numpy fp32 restatement of the kernel's expression tree (no FMA): out[n] = [R d | t x (R d)] -> [N, 6, H, W]"""
    H, W, _ = rays.shape
    dx, dy, dz = (rays.reshape(-1, 3)[:, i] for i in range(3))
    out = np.empty((c2w.shape[0], 6, H * W), np.float32)
    for n, M in enumerate(c2w):
        wx = M[0, 0] * dx + M[0, 1] * dy + M[0, 2] * dz
        wy = M[1, 0] * dx + M[1, 1] * dy + M[1, 2] * dz
        wz = M[2, 0] * dx + M[2, 1] * dy + M[2, 2] * dz
        tx, ty, tz = M[0, 3], M[1, 3], M[2, 3]
        out[n] = [wx, wy, wz, ty * wz - tz * wy, tz * wx - tx * wz, tx * wy - ty * wx]
    return out.reshape(-1, 6, H, W)


def check_plucker(case, out, rays, c2w):
    ref = torch.from_numpy(plucker_ref(rays, c2w)).double()
    return check_bound(case["name"], out, ref, torch.full_like(ref, 5e-6))               # test_plucker_golden's absolute tolerance


def unproject_input(case):
    """(depth fp32 [S,H,W], extr fp32 [S,3,4], intr fp32 [S,3,3]): another extrinsic and intrinsic for every view"""
    S, H, W = case["S"], case["H"], case["W"]
    rng = _rng(case["name"])
    depth = rng.uniform(1, 20, size=(S, H, W)).astype(np.float32)
    intr = np.zeros((S, 3, 3), np.float32)
    for s in range(S):
        intr[s] = [[259.0 + 17 * s, 0, W / 2 + s], [0, 241.0 - 13 * s, H / 2 - s], [0, 0, 1]]
    return depth, _poses(S, rng), intr


def check_unproject(case, out, depth, extr, intr):
    from oracle.reproject_ref import depth_unproject_ref
    ref = torch.from_numpy(depth_unproject_ref(depth, extr, intr)).double()
    return check_bound(case["name"], out, ref, 2e-5 + 2e-5 * ref.abs())                   # test_depth_unproject_vs_oracle's rtol / atol


# ------------------------------------------------------------------------------------------------ second trips
def second_pass_claims():
    """[(case name, cap kind, work items of the launch, items per unit, unit the second trip must start in, unit it must reach)]:
    kind names the launch whose block cap applies ('ew': elementwise.hip grid_for, 'tconv': ew_time_conv3_f32, 'geom': geometry.hip
    grid_for, 'clip': the three image launches of clip.hip); a unit is an image, frame, plane, channel or view."""
    out = []
    for c in LAYOUT_FWD + LAYOUT_BWD:
        if c["name"].endswith("_2pass"):
            out.append((c["name"], "ew", c["N"] * c["H"] * c["W"], c["H"] * c["W"], 3, 4))
    for c in EULER_CASES:
        if c["name"].endswith("_2pass"):
            out.append((c["name"], "ew", c["T"] * c["h"] * c["w"], c["h"] * c["w"], 3, 4))
    c = TCONV_CASES[-1]
    out.append((c["name"], "tconv", c["B"] * c["T"] * (c["HW"] // 4), c["HW"] // 4, 19, 20))
    for c in BLUR_CASES:
        if c["name"].endswith("_2pass"):
            out.append((c["name"], "clip", c["planes"] * c["H"] * c["W"], c["H"] * c["W"], 4, 4))
    c = BICUBIC_CASES[-1]
    out.append((c["name"], "clip", c["N"] * c["C"] * c["Ho"] * c["Wo"], c["Ho"] * c["Wo"], 2, 2))
    c = PATCHIFY_CASES[-1]
    out.append((c["name"], "clip", c["N"] * (c["S"] // c["P"]) ** 2 * c["ldk"], (c["S"] // c["P"]) ** 2 * c["ldk"], 12, 15))
    c = PLUCKER_CASES[-1]
    out.append((c["name"], "geom", c["N"] * c["H"] * c["W"], c["H"] * c["W"], 8, 8))
    c = UNPROJECT_CASES[-1]
    out.append((c["name"], "geom", c["S"] * c["H"] * c["W"], c["H"] * c["W"], 4, 4))
    return out


def all_cases():
    return (LAYOUT_FWD + LAYOUT_BWD + EULER_CASES + TCONV_CASES + BLUR_CASES + BICUBIC_CASES + PATCHIFY_CASES + SINUSOID_CASES
            + PLUCKER_CASES + UNPROJECT_CASES)
