"""Thin tensor->pointer wrappers over the C ABI (include/evoworld_hip.h).  torch is used only for device
memory and the current HIP stream; every op below is one hand-written HIP kernel launch.  No fallback.
Signatures, argument structs and enum values come from the header through _lib's parse of it; every launch goes through
`_call`, which passes the arguments positionally in the prototype's order with the current stream last."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GemmArgs

A_DENSE, A_CONV3X3, A_CONVT3 = _lib.EW_A_DENSE, _lib.EW_A_CONV3X3, _lib.EW_A_CONVT3
ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_GELU = _lib.EW_ACT_NONE, _lib.EW_ACT_SILU, _lib.EW_ACT_GEGLU, _lib.EW_ACT_GELU

_zero_pages = {}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call(name, *args):
    """The one path into the library for the ew_status entry points: name(*args, current stream), raising on a status != 0.
    The function is looked up on the library object at every call, so that a wrapper set on it (bench.py's per-kernel timers)
    or another build (_lib.using) takes effect."""
    _lib.check(getattr(_lib.load(), name)(*args, _stream()), name)


def _aligned(t, n=16):
    """A contiguous tensor whose data pointer is n-byte aligned: `t` itself when it already is (the usual case: whole
    allocations), otherwise a fresh copy -- a frame-filtered slice such as conf[frames] or xyz[1:] of a tensor with
    H*W % 4 != 0 starts at an odd offset, and the 16-byte vector kernels need an aligned base."""
    t = t.contiguous()
    return t if t.data_ptr() % n == 0 else t.clone(memory_format=torch.contiguous_format)


def _req(t, dtype, name):
    if t.device.type != "cuda":
        raise _lib.EvoWorldHipError(f"{name} must live on the GPU (got {t.device}); evoworld_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def zero_page(device):
    key = str(device)
    if key not in _zero_pages:
        _zero_pages[key] = torch.zeros(4096, dtype=torch.float16, device=device)
    return _zero_pages[key]


class Res:
    """A residual-stream tensor carried split: hi = fp16(x) plus an int8 companion `lo` (one byte per element:
    bits(x) ~= bits(float(hi)) + 32 * lo on the fp32 bit patterns, ~19 mantissa bits in 3 bytes; include/evoworld_hip.h,
    ew_gemm_args), or lo = None when the stream is kept in plain fp16.  The reference runs the stream in fp32
    (unified_loop_consistency.py:188); consumers that need an fp16 MFMA operand read `hi` alone, the residual epilogues and
    the norms read both."""
    __slots__ = ("hi", "lo")

    def __init__(self, hi, lo=None):
        self.hi, self.lo = hi, lo

    @classmethod
    def empty(cls, rows, C, device, split):
        hi = torch.empty(rows, C, dtype=torch.float16, device=device)
        return cls(hi, torch.empty(rows, C, dtype=torch.int8, device=device) if split else None)

    @classmethod
    def from_float(cls, x):
        """fp32 tensor -> split form (host-side twin of the kernels' encoder: tests, debugging taps)."""
        x = x.float().contiguous()
        hi = x.half()
        d = (x.view(torch.int32) - hi.float().view(torch.int32) + 16) >> 5
        return cls(hi, d.clamp_(-128, 127).to(torch.int8))

    def float(self):
        if self.lo is None:
            return self.hi.float()
        return (self.hi.float().contiguous().view(torch.int32) + (self.lo.to(torch.int32) << 5)).view(torch.float32)


def _hl(x):
    """tensor | Res | None -> (hi, lo)"""
    if x is None:
        return None, None
    if isinstance(x, Res):
        return x.hi, x.lo
    return x, None


def gemm(a, w, out, *, M, N, c1, lda, a2=None, c2=0, lda2=0, bias=None, rowbias=None, rows_per_group=1, ld_rowbias=None,
         r1=None, ld_r1=0, r2=None, ld_r2=0, ld_out=None, mode=A_DENSE, conv=None, tconv=None, act=ACT_NONE,
         c_acc=1.0, c_r1=1.0, c_r2=1.0, conv_shift=0):
    """out = c_acc*act(A@W^T + bias + rowbias) + c_r1*r1 + c_r2*r2  (see ew_gemm_f16).
    conv = (n_img, h_in, w_in, h_out, w_out, stride, upsample); tconv = (B, T, P); conv_shift=1: padding (0,1) taps.
    r1 / r2 / out may be `Res` (split-fp16 residual stream): the lo halves ride along (ew_gemm_args.r1_lo ...)."""
    g = GemmArgs()
    r1h, r1l = _hl(r1)
    r2h, r2l = _hl(r2)
    outh, outl = _hl(out)
    g.a, g.a2, g.w, g.bias, g.rowbias = _ptr(a), _ptr(a2), _ptr(w), _ptr(bias), _ptr(rowbias)
    g.r1, g.r2, g.out, g.zero_page = _ptr(r1h), _ptr(r2h), _ptr(outh), _ptr(zero_page(a.device))
    g.r1_lo, g.r2_lo, g.out_lo = _ptr(r1l), _ptr(r2l), _ptr(outl)
    g.M, g.N, g.c1, g.c2, g.lda, g.lda2 = M, N, c1, c2, lda, lda2
    n_out = N // 2 if act == ACT_GEGLU else N
    g.ld_out = ld_out if ld_out is not None else n_out
    g.ld_r1, g.ld_r2, g.mode = ld_r1, ld_r2, mode
    g.ld_rowbias = ld_rowbias if ld_rowbias is not None else N
    if conv is not None:
        g.n_img, g.h_in, g.w_in, g.h_out, g.w_out, g.stride, g.upsample = conv
    if tconv is not None:
        g.tB, g.tT, g.tP = tconv
    g.rows_per_group, g.act = rows_per_group, act
    g.c_acc, g.c_r1, g.c_r2 = c_acc, c_r1, c_r2
    g.conv_shift = conv_shift
    _call("ew_gemm_f16", ctypes.byref(g))
    return out


_sk_ready = set()


def streamk_init():
    """Best effort: allocate generation 3's stream-K workspace for (current device, current stream) once, outside any kernel
    launch path (ew_gemm_streamk_init).  Nothing depends on it succeeding -- a launch without a workspace runs the whole-tile
    schedule -- so a full pool (64 (device, stream) pairs per process) or a failed allocation only warns.  Skipped when the
    tail split cannot be used (generation != 3) and while the current stream is being captured into a graph
    (allocation + memset are illegal there; call it on the capture stream BEFORE the capture to get the tail inside the graph)."""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    if key in _sk_ready:
        return
    if _lib.load().ew_get_gemm_generation() != 3:
        return
    if torch.cuda.is_current_stream_capturing():
        return
    _sk_ready.add(key)
    if _lib.load().ew_gemm_streamk_init(_stream()) != 0:
        import warnings
        msg = _lib.load().ew_last_error()
        warnings.warn("ew_gemm_streamk_init: " + (msg.decode() if msg else "failed") + " (continuing without the stream-K tail on this stream)")


def streamk_check():
    """Raise if a stream-K finisher ever gave up waiting for its partner's partial (the tile it wrote is wrong).  Synchronises:
    call it where results are handed to the caller (end of a denoise loop / U-Net call / bench), not per launch."""
    st = _lib.load().ew_gemm_streamk_status()
    if st != 0:
        msg = _lib.load().ew_last_error()          # names the launch (kernel variant, M / N / K, stream) when the time-out was recorded
        raise _lib.EvoWorldHipError((msg.decode() if msg else "stream-K hand-over timed out in ew_gemm_f16 (generation 3): results of that launch are invalid")
                                    if st > 0 else "ew_gemm_streamk_status: HIP error while reading the status word")


def linear(x, w, bias=None, out=None, split_out=False, **kw):
    """x [M,K] fp16 (row stride = K), w [N,K] fp16 -> [M,N] (a `Res` with a lo half when split_out)."""
    _req(x, torch.float16, "x"); _req(w, torch.float16, "w")
    M, K = x.shape
    N = w.shape[0]
    act = kw.get("act", ACT_NONE)
    if out is None:
        n_out = N // 2 if act == ACT_GEGLU else N
        out = Res.empty(M, n_out, x.device, True) if split_out else torch.empty(M, n_out, dtype=torch.float16, device=x.device)
    return gemm(x, w, out, M=M, N=N, c1=K, lda=K, bias=bias, **kw)


class WorkspacePool:
    """fp32 scratch for the GroupNorm statistics of one forward (partials, stats: all written before they are read, so
    nothing is zeroed).  `reset()` rewinds; `take(n)` hands out the next n floats."""

    def __init__(self, device, floats=8 << 20):
        self.buf = torch.empty(floats, dtype=torch.float32, device=device)
        self.cur = 0

    def reset(self):
        self.cur = 0

    def take(self, n):
        n = (n + 63) // 64 * 64
        if self.cur + n > self.buf.numel():
            return torch.empty(n, dtype=torch.float32, device=self.buf.device)      # overflow: a fresh buffer
        v = self.buf[self.cur: self.cur + n]
        self.cur += n
        return v


def groupnorm(xs, gamma, beta, n_slabs, rows, eps, silu, groups=32, out=None, pool=None, stats_hi_only=False, split_out=False):
    """GroupNorm(+SiLU) over the channel concat of `xs` (list of [n_slabs*rows, C_i] fp16 tensors or `Res`) ->
    [n_slabs*rows, sum C_i] fp16.  Deterministic shifted statistics: stats per source, one finalize, apply per source.
    split_out: the result is the split operand [n_slabs*rows, 2 * sum C_i] = [y_hi | y_lo], y_lo = fp16(y - y_hi) (ew_groupnorm_apply_split_f16)."""
    lib = _lib.load()
    srcs = [_hl(x) for x in xs]
    C_tot = sum(h.shape[-1] for h, _ in srcs)
    dev = srcs[0][0].device
    nws = lib.ew_groupnorm_workspace_floats(n_slabs, rows, C_tot, groups)
    ws = pool.take(nws) if pool is not None else torch.empty(nws, dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty(n_slabs * rows, 2 * C_tot if split_out else C_tot, dtype=torch.float16, device=dev)
    off = 0
    for h, l in srcs:
        # stats_hi_only (off): statistics from the hi half alone would save the lo read of this pass (2.3 ms per forward), but
        # the rounding remainders add ulp^2/12 to the variance -- 0.5 % when a channel's std is ~4 fp16 ulps of its mean
        # (mean/std = 300), i.e. exactly the cancellation-prone inputs the shifted statistics exist for
        _call("ew_groupnorm_stats_f16", _ptr(h), None if stats_hi_only else _ptr(l), _ptr(ws), n_slabs, rows, h.shape[-1], off, C_tot, groups)
        off += h.shape[-1]
    _call("ew_groupnorm_finalize", _ptr(ws), n_slabs, rows, C_tot, groups)
    off = 0
    for h, l in srcs:
        if split_out:
            _call("ew_groupnorm_apply_split_f16", _ptr(h), _ptr(l), _ptr(ws), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(out[:, C_tot:]),
                  2 * C_tot, n_slabs, rows, h.shape[-1], off, C_tot, groups, eps, 1 if silu else 0)
        else:
            _call("ew_groupnorm_apply_f16", _ptr(h), _ptr(l), _ptr(ws), _ptr(gamma), _ptr(beta), _ptr(out), n_slabs, rows,
                  h.shape[-1], off, C_tot, groups, eps, 1 if silu else 0)
        off += h.shape[-1]
    return out


def layernorm(x, gamma, beta, eps=1e-5, addvec=None, rows_per_group=1, x_out=None, out=None):
    """x, x_out: fp16 tensors or `Res` (split-fp16 residual stream)."""
    xh, xl = _hl(x)
    oh, ol = _hl(x_out)
    rows, C = xh.shape
    if out is None:
        out = torch.empty_like(xh)
    _call("ew_layernorm_f16", _ptr(xh), _ptr(xl), _ptr(addvec), rows_per_group, _ptr(oh), _ptr(ol), _ptr(gamma), _ptr(beta), _ptr(out), rows, C, eps)
    return out


def attn_spatial(q, k, vt, o, n_seq, S, heads, ld_qk, ld_vt, ld_o, scale=0.125):
    _call("ew_attn_spatial_f16", _ptr(q), _ptr(k), _ptr(vt), _ptr(o), n_seq, S, heads, ld_qk, ld_vt, ld_o, scale)
    return o


QK_LOG2_PRESCALE = (0.125 * 1.4426950408889634) ** 0.5    # sqrt(head_dim^-0.5 * log2 e), head_dim 64: c_acc of the q|k projection


def attn_spatial_log2(q, k, vt, o, n_seq, S, heads, ld_qk, ld_vt, ld_o):
    """q, k pre-scaled by QK_LOG2_PRESCALE each (projection epilogue): the kernel's MFMA subtracts the running max itself."""
    _call("ew_attn_spatial_log2_f16", _ptr(q), _ptr(k), _ptr(vt), _ptr(o), n_seq, S, heads, ld_qk, ld_vt, ld_o)
    return o


def quant_rows_fp8(x):
    """x fp16 [rows, K] -> (q uint8 [rows, K] holding OCP e4m3 bytes, scale fp32 [rows]): scale = amax(row) / 448 (1 for an all-zero
    row), q = e4m3(x * (1 / scale)), each of the three operations one fp32 rounding, the convert to nearest even (ew_quant_rows_fp8; not
    e4m3(x / scale), which gives other bytes near ties).  K % 8 == 0, K <= 2048."""
    _req(x, torch.float16, "x")
    if x.ndim != 2:
        raise ValueError(f"x: expected fp16 [rows, K], got {tuple(x.shape)}")
    rows, K = x.shape
    q = torch.empty(rows, K, dtype=torch.uint8, device=x.device)
    scale = torch.empty(rows, dtype=torch.float32, device=x.device)
    _call("ew_quant_rows_fp8", _ptr(x), _ptr(q), _ptr(scale), rows, K)
    return q, scale


def gemm_fp8(aq, a_scale, wq, w_scale, out=None, c_acc=1.0):
    """aq [M, K], wq [N, K] e4m3 bytes (uint8), a_scale [M], w_scale [N] fp32 -> fp16 [M, N] = (aq wq^T) * a_scale[m] * w_scale[n] * c_acc
    (ew_gemm_fp8).  `out`: an fp16 [M, N] tensor or view with unit column stride to write into (its row stride is ld_out).
    Swapping the (bytes, scale) pairs gives the transposed product.  K % 64 == 0, N % 4 == 0."""
    _req(aq, torch.uint8, "aq"); _req(wq, torch.uint8, "wq"); _req(a_scale, torch.float32, "a_scale"); _req(w_scale, torch.float32, "w_scale")
    if aq.ndim != 2 or wq.ndim != 2 or aq.shape[1] != wq.shape[1]:
        raise ValueError(f"aq {tuple(aq.shape)} / wq {tuple(wq.shape)}: expected [M, K] and [N, K]")
    M, K = aq.shape
    N = wq.shape[0]
    if a_scale.numel() != M or w_scale.numel() != N:
        raise ValueError(f"a_scale / w_scale hold {a_scale.numel()} / {w_scale.numel()} values for M, N = {M}, {N}")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=aq.device)
    if out.dtype != torch.float16 or out.device != aq.device or tuple(out.shape) != (M, N) or out.stride(1) != 1:
        raise ValueError(f"out: expected an fp16 [{M}, {N}] device tensor with unit column stride, got {out.dtype} {tuple(out.shape)} strides {out.stride()}")
    _call("ew_gemm_fp8", _ptr(aq), _ptr(a_scale), _ptr(wq), _ptr(w_scale), _ptr(out), M, N, K, out.stride(0), float(c_acc))
    return out


def attn_temporal(q, k, v, o, B, T, S, heads, ld, ld_o, scale=0.125):
    _call("ew_attn_temporal_f16", _ptr(q), _ptr(k), _ptr(v), _ptr(o), B, T, S, heads, ld, ld_o, scale)
    return o


def softmax_rows(scores, out=None):
    """scores: fp16 [R, C] tensor or `Res` (hi + lo) -> fp16 softmax over the last dim (fp32 math)."""
    h, l = _hl(scores)
    R, C = h.shape
    if out is None:
        out = torch.empty_like(h)
    _call("ew_softmax_rows_f16", _ptr(h), _ptr(l), _ptr(out), R, C, C)
    return out


def time_conv3(x, w, bias):
    """x fp32 [B,T,C,H,W], w fp32 [C,C,3], bias fp32 [C] -> fp32 [B,T,C,H,W] (Conv3d (3,1,1), zero padding in T)."""
    _req(x, torch.float32, "x"); _req(w, torch.float32, "w"); _req(bias, torch.float32, "bias")
    B, T, C, H, W = x.shape
    y = torch.empty_like(x)
    _call("ew_time_conv3_f32", _ptr(x), _ptr(w), _ptr(bias), _ptr(y), B, T, C, H * W)
    return y


def sinusoid_embed(vals, n_rows, dim):
    """vals fp32 device [n] -> fp16 [n_rows, dim] = [cos | sin] sinusoidal embedding of vals[row % n] (ew_sinusoid_embed_f16)."""
    _req(vals, torch.float32, "vals")
    out = torch.empty(n_rows, dim, dtype=torch.float16, device=vals.device)
    _call("ew_sinusoid_embed_f16", _ptr(vals), vals.numel(), n_rows, dim, _ptr(out))
    return out


def nchw_f32_to_nhwc_f16(x, y, ldc, c_off=0, scale=1.0, split=None):
    """split = (lo_off, dup_off): the row also receives fp16(v - hi) at lo_off + c_off + c and hi again at dup_off + c_off + c
    (ew_nchw_f32_to_nhwc_split_f16: the [x_hi | x_lo | x_hi] A operand of a conv_in packed [W_hi | W_hi | W_lo])."""
    _req(x, torch.float32, "x"); _req(y, torch.float16, "y")
    N, C, H, W = x.shape
    if split:
        _call("ew_nchw_f32_to_nhwc_split_f16", _ptr(x), _ptr(y), N, C, H, W, ldc, c_off, split[0], split[1], scale)
        return y
    _call("ew_nchw_f32_to_nhwc_f16", _ptr(x), _ptr(y), N, C, H, W, ldc, c_off, scale)
    return y


def nhwc_f16_to_nchw_f32(x, N, C, H, W, ldc):
    _req(x, torch.float16, "x")
    y = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    _call("ew_nhwc_f16_to_nchw_f32", _ptr(x), _ptr(y), N, C, H, W, ldc)
    return y


def euler_cfg_step(eps, ld_eps, latents, guidance, sigma, sigma_next, next_in, cpad, T, h, w, split=None):
    _req(latents, torch.float32, "latents"); _req(guidance, torch.float32, "guidance")
    if split:
        _call("ew_euler_cfg_step_split", _ptr(eps), ld_eps, _ptr(latents), _ptr(guidance), float(sigma), float(sigma_next),
              _ptr(next_in), cpad, split[0], split[1], T, h, w)
        return
    _call("ew_euler_cfg_step", _ptr(eps), ld_eps, _ptr(latents), _ptr(guidance), float(sigma), float(sigma_next), _ptr(next_in), cpad, T, h, w)


def plucker_embed(rays, c2w):
    _req(rays, torch.float32, "rays"); _req(c2w, torch.float32, "c2w")
    H, W, _ = rays.shape
    N = c2w.shape[0]
    out = torch.empty(N, 6, H, W, dtype=torch.float32, device=rays.device)
    _call("ew_plucker_embed", _ptr(rays), _ptr(c2w), _ptr(out), N, H, W)
    return out


def cube2equi_gather(faces, lut, H, W):
    """faces uint8 [V,6,res,res,3|4] (order right,left,bottom,top,front,back), lut int16 [H,W,3] -> uint8 [V,H,W,3]."""
    _req(faces, torch.uint8, "faces"); _req(lut, torch.int16, "lut")
    V, res, ch = faces.shape[0], faces.shape[2], faces.shape[-1]
    pano = torch.empty(V, H, W, 3, dtype=torch.uint8, device=faces.device)
    _call("ew_cube2equi_gather", _ptr(faces), ch, _ptr(lut), _ptr(pano), V, H, W, res)
    return pano


def equi2cube(panos, interpolation=True, out=None):
    """Equirectangular panoramas uint8 [V,H,W,3] (W == 2H, W % 4 == 0) -> the reference's cube cross uint8 [V,3W/4,W,3]
    (Navigator.convert_panorama_to_cubemap's transform, navigator_evoworld.py:537-659): bilinear with truncation, or nearest
    with interpolation=False.  One launch for all V.  `out`: a contiguous uint8 [V,3W/4,W,3] tensor to write into."""
    _req(panos, torch.uint8, "panos")
    if panos.ndim != 4 or panos.shape[3] != 3:
        raise ValueError(f"panos: expected uint8 [V,H,W,3], got {tuple(panos.shape)}")
    V, H, W, _ = panos.shape
    if out is None:
        out = torch.empty(V, 3 * (W // 4), W, 3, dtype=torch.uint8, device=panos.device)
    _req(out, torch.uint8, "out")
    if tuple(out.shape) != (V, 3 * (W // 4), W, 3):
        raise ValueError(f"out: expected {(V, 3 * (W // 4), W, 3)}, got {tuple(out.shape)}")
    _call("ew_equi2cube_u8", _ptr(panos), _ptr(out), V, H, W, int(bool(interpolation)))
    return out


def cubemap_faces_to_equi(faces, H, W):
    """Cube faces -> panoramas uint8 [V,H,W,3] through the integer LUT of Navigator.cubemap_to_equirectangular
    (reprojection.build_cubemap2equi_lut, cached per (W,H,res)) and ew_cube2equi_gather.  faces: a dict name -> uint8
    [V,res,res,3] (any key order; a missing face is black, as in the reference, navigator_evoworld.py:806-852) or a stacked
    uint8 [V,6,res,res,3] in FACE_ORDER."""
    from .reprojection import FACE_ORDER, build_cubemap2equi_lut
    if isinstance(faces, dict):
        unknown = set(faces) - set(FACE_ORDER)
        if unknown or not faces:
            raise ValueError(f"faces: expected keys among {FACE_ORDER}, got {sorted(faces)}")
        first = next(iter(faces.values()))
        for n, f in faces.items():
            if f.ndim != 4 or f.shape[1] != f.shape[2] or f.shape[3] != 3 or f.shape != first.shape:
                raise ValueError(f"faces[{n!r}]: expected square uint8 [V,res,res,3] faces of one size, got {tuple(f.shape)}")
        faces = torch.stack([faces[n] if n in faces else torch.zeros_like(first) for n in FACE_ORDER], dim=1)
    lut = build_cubemap2equi_lut(W, H, faces.shape[2]).to(faces.device)
    return cube2equi_gather(faces.contiguous(), lut, H, W)


def select_kth(x, k):
    """x fp32 [n] on the device -> fp32 [2] device tensor (x_(k), x_(k+1)) (0-based, ascending): radix select, no sort."""
    lib = _lib.load()
    x = _aligned(x)
    _req(x, torch.float32, "x")
    ws = torch.empty(lib.ew_select_workspace_bytes() // 4 + 4, dtype=torch.int32, device=x.device)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    _call("ew_select_kth_f32", _ptr(x), x.numel(), int(k), _ptr(ws), _ptr(out))
    return out


def filter_compact(conf, thr, xyz, img, img_nchw_hw=0):
    """conf fp32 [n], xyz fp32 [n,3], img fp32 [n,3] (or [S,3,hw] planes with img_nchw_hw = hw) ->
    (xyz_kept [m,3] fp32, rgbx [m,4] uint8 whose first 3 bytes are (img*255) truncated), order preserved."""
    lib = _lib.load()
    conf, xyz, img = _aligned(conf), _aligned(xyz), _aligned(img)
    _req(conf, torch.float32, "conf"); _req(xyz, torch.float32, "xyz"); _req(img, torch.float32, "img")
    n = conf.numel()
    dev = conf.device
    out_xyz = torch.empty(n, 3, dtype=torch.float32, device=dev)
    out_rgbx = torch.empty(n, 4, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.ew_filter_compact_workspace_bytes(n) // 4 + 1, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("ew_filter_compact", _ptr(conf), n, float(thr), _ptr(xyz), _ptr(img), 1 if img_nchw_hw else 0, int(img_nchw_hw),
          _ptr(out_xyz), _ptr(out_rgbx), _ptr(ws), _ptr(total))
    m = int(total.item())
    return out_xyz[:m], out_rgbx[:m]


def depth_unproject(depth, extr, intr):
    _req(depth, torch.float32, "depth"); _req(extr, torch.float32, "extr"); _req(intr, torch.float32, "intr")
    S, H, W = depth.shape
    xyz = torch.empty(S, H, W, 3, dtype=torch.float32, device=depth.device)
    _call("ew_depth_unproject", _ptr(depth), _ptr(extr), _ptr(intr), _ptr(xyz), S, H, W)
    return xyz


def splat_cubemap(xyz, rgb, w2c, res, fx, fy, cx, cy, z_near, face_channels=3):
    """xyz [N,3] f32, rgb u8 [N,3] (packed) or [N,4] (RGBX words, possibly a [:, :3] view of one), w2c [V,6,3,4] f32 ->
    faces u8 [V,6,res,res,face_channels], zbuf u64-as-int64 [V,6,res,res]."""
    xyz = _aligned(xyz)
    _req(xyz, torch.float32, "xyz"); _req(w2c, torch.float32, "w2c")
    if rgb.dtype != torch.uint8 or rgb.device.type != "cuda":
        raise TypeError("rgb must be a uint8 device tensor")
    if rgb.ndim == 2 and rgb.stride(0) == 4 and rgb.stride(1) == 1:
        stride = 4                                                     # RGBX words (ew_filter_compact output)
    else:
        rgb, stride = rgb.contiguous(), 3
    V = w2c.shape[0]
    zbuf = torch.empty((V, 6, res, res), dtype=torch.int64, device=xyz.device)     # initialised by ew_splat_cubemap itself (0xFFFF... = no fragment)
    _call("ew_splat_cubemap", _ptr(xyz), xyz.shape[0], _ptr(w2c), _ptr(zbuf), V, res, fx, fy, cx, cy, z_near)
    faces = torch.empty(V, 6, res, res, face_channels, dtype=torch.uint8, device=xyz.device)
    _call("ew_splat_resolve", _ptr(zbuf), _ptr(rgb), stride, _ptr(faces), face_channels, V, res)
    return faces, zbuf


def points_bounds(xyz):
    """xyz fp32 [n,3] on the device -> (min fp32 [3], max fp32 [3], n_finite) on the host: the per-axis bounds over the points whose
    three coordinates are all finite, and their count (ew_points_bounds); +inf / -inf and 0 when there is none.  Synchronises."""
    lib = _lib.load()
    xyz = _aligned(xyz)
    _req(xyz, torch.float32, "xyz")
    n = xyz.shape[0]
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must be [n,3], got {tuple(xyz.shape)}")
    ws = torch.empty(lib.ew_points_bounds_workspace_bytes(n) // 8 + 1, dtype=torch.int64, device=xyz.device)
    out6 = torch.empty(6, dtype=torch.float32, device=xyz.device)
    cnt = torch.empty(1, dtype=torch.int64, device=xyz.device)
    _call("ew_points_bounds", _ptr(xyz), n, _ptr(ws), _ptr(out6), _ptr(cnt))
    b = out6.cpu().numpy()
    return b[:3].copy(), b[3:].copy(), int(cnt.item())


VOXEL_GRID_BITS = 21            # bits per axis of a voxel key (ew_voxel_keys)


def voxel_downsample(xyz, rgbx, voxel_size):
    """Voxel-grid downsample on the device, Open3D's voxel_down_sample convention: xyz fp32 [n,3], rgbx uint8 [n,4] (the RGBX words
    of filter_compact; a [n,3] tensor is widened) -> (xyz [m,3] fp32 = the mean of each occupied voxel's points, rgba [m,4] uint8 =
    the per-channel mean rounded half to even with alpha 255, count [m] int32), voxels in ascending key order (x major).  Non-finite
    points are dropped.  ew_points_bounds -> ew_voxel_keys -> torch.sort(stable) -> ew_voxel_reduce; deterministic (no atomics).
    ValueError: voxel_size not a positive finite number, or a cloud that spans more than 2^21 voxels along an axis."""
    try:
        v = float(voxel_size)
    except (TypeError, ValueError):
        raise ValueError(f"voxel_size must be a positive finite number, got {voxel_size!r}") from None
    v32 = np.float32(v)
    if not (np.isfinite(v32) and v32 > 0):
        raise ValueError(f"voxel_size must be a positive finite number (in float32), got {voxel_size!r}")
    if rgbx.dtype != torch.uint8 or rgbx.device.type != "cuda":
        raise TypeError("rgbx must be a uint8 device tensor")
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgbx.ndim != 2 or rgbx.shape[0] != xyz.shape[0] or rgbx.shape[1] not in (3, 4):
        raise ValueError(f"xyz must be [n,3] and rgbx [n,3|4], got {tuple(xyz.shape)} and {tuple(rgbx.shape)}")
    dev = xyz.device

    def empty():
        return (torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 4, dtype=torch.uint8, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))

    n = xyz.shape[0]
    if n == 0:
        return empty()
    lib = _lib.load()
    xyz = _aligned(xyz)
    _req(xyz, torch.float32, "xyz")
    if rgbx.shape[1] == 3:
        rgbx = torch.cat([rgbx, torch.zeros(n, 1, dtype=torch.uint8, device=dev)], dim=1)
    rgbx = _aligned(rgbx)
    lo, hi, n_finite = points_bounds(xyz)
    if n_finite == 0:
        return empty()
    origin = (lo - np.float32(0.5) * v32).astype(np.float32)          # float32 arithmetic, as the kernel's index expects
    origin_d = torch.from_numpy(origin).to(dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("ew_voxel_keys", _ptr(xyz), n, _ptr(origin_d), float(v32), _ptr(keys), _ptr(overflow))
    if int(overflow.item()):
        extent = float(np.max(hi.astype(np.float64) - lo.astype(np.float64)))
        raise ValueError(f"voxel_size {v:g} is too small for a cloud of extent {extent:g}: a voxel key has {VOXEL_GRID_BITS} bits per "
                         f"axis, so the smallest voxel size this cloud admits is about {extent / 2 ** VOXEL_GRID_BITS:g} "
                         f"(extent / 2^{VOXEL_GRID_BITS})")
    skeys, perm = torch.sort(keys, stable=True)                          # plumbing: the sort is torch's
    out_xyz = torch.empty(n, 3, dtype=torch.float32, device=dev)
    out_rgba = torch.empty(n, 4, dtype=torch.uint8, device=dev)
    out_cnt = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.ew_voxel_reduce_workspace_bytes(n) // 16 + 1, 2, dtype=torch.int64, device=dev)
    m_d = torch.empty(1, dtype=torch.int64, device=dev)
    _call("ew_voxel_reduce", _ptr(skeys), _ptr(perm), n, _ptr(xyz), _ptr(rgbx), _ptr(out_xyz), _ptr(out_rgba), _ptr(out_cnt), _ptr(ws),
          _ptr(m_d))
    m = int(m_d.item())
    return out_xyz[:m], out_rgba[:m], out_cnt[:m]


JPEG_SAMPLING = {"4:2:0": (_lib.EW_JPEG_420, 16, 6), "4:4:4": (_lib.EW_JPEG_444, 8, 3)}      # name -> (ABI value, MCU size, blocks per MCU)


def jpeg_dct_quant(frames_u8, quality, subsampling="4:2:0", out=None):
    """frames uint8 [V,H,W,3] on the device -> the quantised DCT coefficients of their baseline JPEGs, int16
    [V, mcu_rows, mcu_cols, blocks_per_mcu, 64] in scan and zigzag order (ew_jpeg_dct_quant).  quality 1..100,
    subsampling "4:2:0" | "4:4:4".  `out`: a contiguous, 16-byte aligned int16 tensor of that shape to write into."""
    _req(frames_u8, torch.uint8, "frames_u8")
    if frames_u8.ndim != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"frames_u8 must be [V,H,W,3], got {tuple(frames_u8.shape)}")
    if subsampling not in JPEG_SAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(JPEG_SAMPLING)}, got {subsampling!r}")
    if not (isinstance(quality, int) and 1 <= quality <= 100):
        raise ValueError(f"quality must be an integer 1..100, got {quality!r}")
    V, H, W, _ = frames_u8.shape
    if not (1 <= V <= 65535 and 1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"V, H and W must be 1..65535, got {V}, {H}, {W}")
    mode, mcu, bpm = JPEG_SAMPLING[subsampling]
    shape = (V, -(-H // mcu), -(-W // mcu), bpm, 64)
    if out is None:
        out = torch.empty(shape, dtype=torch.int16, device=frames_u8.device)
    elif tuple(out.shape) != shape:
        raise ValueError(f"out must be {shape}, got {tuple(out.shape)}")
    _req(out, torch.int16, "out")
    _call("ew_jpeg_dct_quant", _ptr(frames_u8), _ptr(out), V, H, W, quality, mode)
    return out


def jpeg_entropy(coef):
    """coef int16 [V, mcu_rows, mcu_cols, 6 | 3, 64] (jpeg_dct_quant) -> (slots uint8 [V * mcu_rows, slot_bytes], seg_bytes int32
    [V * mcu_rows]) on the device: the Huffman-coded, byte-stuffed restart segment of every MCU row and its length
    (ew_jpeg_entropy).  Slots hold the provable worst case, 416 bytes per block."""
    _req(coef, torch.int16, "coef")
    if coef.ndim != 5 or coef.shape[3] not in (3, 6) or coef.shape[4] != 64 or coef.numel() == 0:
        raise ValueError(f"coef must be [V, mcu_rows, mcu_cols, 6 | 3, 64], got {tuple(coef.shape)}")
    V, mr, mc, bpm, _ = coef.shape
    coef = _aligned(coef)
    slot = _lib.load().ew_jpeg_segment_slot_bytes(mc, bpm)
    slots = torch.empty(V * mr, slot, dtype=torch.uint8, device=coef.device)
    seg_bytes = torch.empty(V * mr, dtype=torch.int32, device=coef.device)
    _call("ew_jpeg_entropy", _ptr(coef), _ptr(slots), _ptr(seg_bytes), V * mr, mc, bpm, slot)
    return slots, seg_bytes


def jpeg_pack(slots, seg_bytes, mcu_rows):
    """The segments of jpeg_entropy -> (stream uint8 [total] on the device, frame_bytes int64 [V] on the host): every frame's scan
    data, contiguous, with the RSTm markers between its MCU rows (ew_jpeg_pack).  The offsets are torch.cumsum of the byte counts
    (plumbing).  Synchronises once, for the stream's length."""
    _req(slots, torch.uint8, "slots"); _req(seg_bytes, torch.int32, "seg_bytes")
    n = seg_bytes.shape[0]
    if slots.ndim != 2 or slots.shape[0] != n or n == 0 or mcu_rows < 1 or n % mcu_rows:
        raise ValueError(f"slots must be [n, slot_bytes] and seg_bytes [n] with n a positive multiple of mcu_rows = {mcu_rows}, "
                         f"got {tuple(slots.shape)} and {tuple(seg_bytes.shape)}")
    sizes = seg_bytes.to(torch.int64).view(-1, mcu_rows) + 2
    sizes[:, -1] -= 2                                                   # no marker behind a frame's last row
    ends = torch.cumsum(sizes.view(-1), 0)
    offsets = (ends - sizes.view(-1)).contiguous()
    frame_bytes = sizes.sum(dim=1).cpu()
    total = int(frame_bytes.sum())
    stream = torch.empty(total, dtype=torch.uint8, device=slots.device)
    _call("ew_jpeg_pack", _ptr(slots), _ptr(seg_bytes), _ptr(offsets), _ptr(stream), n, mcu_rows, slots.shape[1], total)
    return stream, frame_bytes


PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": _lib.EW_PNG_FILTER_ADAPTIVE}
PNG_HIST_COLS = _lib.EW_PNG_HIST_COLS                    # 286 literal/length symbols, then 30 distance codes
PNG_SEGMENT_TARGET = 32768                               # bytes: the default rows_per_segment keeps a segment at or below it


def png_rows_per_segment(H, W, rows_per_segment=None):
    """The rows of one deflate segment: as given (at least 1, at most H), else the most whole filtered rows (1 + 3 W bytes each) that
    stay within 32 KiB, at least 1."""
    if rows_per_segment is None:
        rows_per_segment = max(1, PNG_SEGMENT_TARGET // (1 + 3 * W))
    if not (isinstance(rows_per_segment, int) and rows_per_segment >= 1):
        raise ValueError(f"rows_per_segment must be an integer >= 1, got {rows_per_segment!r}")
    return min(rows_per_segment, H)


def _png_geometry(V, H, W, rows_per_segment):
    """-> (rows per segment, segments per frame, bytes of a full segment) after the checks every PNG entry shares"""
    if not (1 <= V <= 65535 and 1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"V, H and W must be 1..65535, got {V}, {H}, {W}")
    rps = png_rows_per_segment(H, W, rows_per_segment)
    spf = -(-H // rps)
    if V * spf >= 1 << 31:
        raise ValueError(f"n_segments = {V * spf} must be below 2^31")
    if rps * (1 + 3 * W) > _lib.EW_PNG_MAX_SEGMENT_BYTES:
        raise ValueError(f"a segment of {rps} rows of {1 + 3 * W} bytes exceeds {_lib.EW_PNG_MAX_SEGMENT_BYTES} bytes")
    return rps, spf, rps * (1 + 3 * W)


def _png_filtered(filtered):
    if filtered.ndim != 3 or filtered.shape[2] < 4 or (filtered.shape[2] - 1) % 3 or filtered.numel() == 0:
        raise ValueError(f"filtered must be [V,H,1+3W], got {tuple(filtered.shape)}")
    return filtered.shape[0], filtered.shape[1], (filtered.shape[2] - 1) // 3


def png_filter(frames_u8, filter="adaptive", rows_per_segment=None):
    """frames uint8 [V,H,W,3] on the device -> (filtered uint8 [V,H,1+3W]: every row behind its PNG filter type; adler int32
    [n_segments, 2]: the Adler-32 halves of every segment of rows_per_segment rows) (ew_png_filter).  filter: "none" |
    "sub" | "up" | "average" | "paeth" (or 0..4) forces a type, "adaptive" picks per row by the minimum sum of absolute differences."""
    if frames_u8.dtype != torch.uint8:                   # the argument checks come before the device check: they need no GPU
        raise TypeError(f"frames_u8: expected {torch.uint8}, got {frames_u8.dtype}")
    if frames_u8.ndim != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"frames_u8 must be [V,H,W,3], got {tuple(frames_u8.shape)}")
    mode = PNG_FILTERS.get(filter) if isinstance(filter, str) else (filter if isinstance(filter, int) and 0 <= filter <= 4 else None)
    if mode is None:
        raise ValueError(f"filter must be one of {sorted(PNG_FILTERS)} or 0..4, got {filter!r}")
    V, H, W, _ = frames_u8.shape
    rps, spf, _ = _png_geometry(V, H, W, rows_per_segment)
    _req(frames_u8, torch.uint8, "frames_u8")
    filtered = torch.empty(V, H, 1 + 3 * W, dtype=torch.uint8, device=frames_u8.device)
    adler = torch.empty(V * spf, 2, dtype=torch.int32, device=frames_u8.device)
    _call("ew_png_filter", _ptr(frames_u8), _ptr(filtered), _ptr(adler), V, H, W, mode, rps)
    return filtered, adler


def png_lz77(filtered, rows_per_segment=None):
    """filtered uint8 [V,H,1+3W] (png_filter) -> (tokens int32 [n_segments, segment bytes], n_tokens int32 [n_segments], hist int32
    [n_segments, 316]) on the device (ew_png_lz77).  A token's 32 bits: a literal byte, or bit 31 | distance - 1 << 8 | length - 3; a
    token slot holds the worst case of one token per byte."""
    V, H, W = _png_filtered(filtered)
    rps, spf, seg_bytes = _png_geometry(V, H, W, rows_per_segment)
    _req(filtered, torch.uint8, "filtered")
    n = V * spf
    tokens = torch.empty(n, seg_bytes, dtype=torch.int32, device=filtered.device)
    n_tokens = torch.empty(n, dtype=torch.int32, device=filtered.device)
    hist = torch.empty(n, PNG_HIST_COLS, dtype=torch.int32, device=filtered.device)
    _call("ew_png_lz77", _ptr(filtered), _ptr(tokens), _ptr(n_tokens), _ptr(hist), V, H, W, rps, seg_bytes)
    return tokens, n_tokens, hist


def png_emit(tokens, n_tokens, filtered, seg_mode, seg_offsets, seg_bytes, luts, headers, header_bits, out, rows_per_segment=None):
    """The segments' final bytes into `out` uint8 [bytes] (ew_png_emit): segment s to out[seg_offsets[s] : + seg_bytes[s]] (int64), coded
    with its frame's luts int32 [V,316] / headers uint8 [V,n] / header_bits int32 [V] or, where seg_mode int32 says so, as stored
    blocks.  A segment whose range leaves `out` is skipped.  Returns out."""
    V, H, W = _png_filtered(filtered)
    rps, spf, sb = _png_geometry(V, H, W, rows_per_segment)
    _req(filtered, torch.uint8, "filtered")
    n = V * spf
    for t, dt, name, shape in ((tokens, torch.int32, "tokens", None), (n_tokens, torch.int32, "n_tokens", (n,)),
                               (seg_mode, torch.int32, "seg_mode", (n,)), (seg_offsets, torch.int64, "seg_offsets", (n,)),
                               (seg_bytes, torch.int64, "seg_bytes", (n,)), (luts, torch.int32, "luts", (V, PNG_HIST_COLS)),
                               (headers, torch.uint8, "headers", None), (header_bits, torch.int32, "header_bits", (V,)),
                               (out, torch.uint8, "out", None)):
        _req(t, dt, name)
        if shape is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    if tokens.ndim != 2 or tokens.shape[0] != n or tokens.shape[1] < sb:
        raise ValueError(f"tokens must be [{n}, >= {sb}], got {tuple(tokens.shape)}")
    if headers.ndim != 2 or headers.shape[0] != V or headers.shape[1] < 1:
        raise ValueError(f"headers must be [{V}, n], got {tuple(headers.shape)}")
    if out.ndim != 1 or out.numel() < 1:
        raise ValueError(f"out must be a non-empty 1-D tensor, got {tuple(out.shape)}")
    _call("ew_png_emit", _ptr(tokens), _ptr(n_tokens), _ptr(filtered), _ptr(seg_mode), _ptr(seg_offsets), _ptr(seg_bytes), _ptr(luts),
          _ptr(headers), _ptr(header_bits), headers.shape[1], _ptr(out), out.numel(), V, H, W, rps, tokens.shape[1])
    return out


JPEG_SEG_STATUS = {_lib.EW_JPEG_SEG_BAD_CODE: "no Huffman code matches the bits (or an EOBn symbol of a progressive scan)",
                   _lib.EW_JPEG_SEG_INDEX: "a zero run leads past coefficient 63",
                   _lib.EW_JPEG_SEG_SIZE: "a DC category above 11 or an AC size above 10",
                   _lib.EW_JPEG_SEG_EXHAUSTED: "the segment's bytes end before its MCUs",
                   _lib.EW_JPEG_SEG_LEFTOVER: "more than 7 bits are left behind the last MCU",
                   _lib.EW_JPEG_SEG_MARKER: "a marker (FF followed by anything but 00) inside the segment",
                   _lib.EW_JPEG_SEG_RANGE: "the segment lies outside the uploaded bytes"}


def jpeg_huffman_decode(stream, seg_start, seg_bytes, tables, V, mcu_rows, mcu_cols, blocks_per_mcu, restart_interval, out=None):
    """The entropy-coded bytes of V frames with identical headers -> (coef int16 [V, mcu_rows, mcu_cols, blocks_per_mcu, 64] in scan and
    zigzag order, the layout of jpeg_dct_quant; seg_status int32 [n], 0 or a key of JPEG_SEG_STATUS) on the device
    (ew_jpeg_huffman_decode).  stream uint8 [bytes]; seg_start int64 [n] and seg_bytes int32 [n]: every restart segment
    without its RSTm marker, restart_interval MCUs each (0: one segment per frame); tables uint8 [4 * EW_JPEG_HUFF_TABLE_BYTES]
    (video.huffman_device_tables).  `out`: a contiguous int16 tensor of the coefficients' shape to write into."""
    _req(stream, torch.uint8, "stream"); _req(seg_start, torch.int64, "seg_start"); _req(seg_bytes, torch.int32, "seg_bytes")
    _req(tables, torch.uint8, "tables")
    for name, v, lo, hi in (("V", V, 1, 65535), ("mcu_rows", mcu_rows, 1, 8192), ("mcu_cols", mcu_cols, 1, 8192),
                            ("restart_interval", restart_interval, 0, 65535)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer {lo}..{hi}, got {v!r}")
    if blocks_per_mcu not in (3, 6):
        raise ValueError(f"blocks_per_mcu must be 6 (4:2:0) or 3 (4:4:4), got {blocks_per_mcu!r}")
    mcus = mcu_rows * mcu_cols
    interval = mcus if restart_interval == 0 or restart_interval > mcus else restart_interval
    n = V * -(-mcus // interval)
    if stream.ndim != 1 or stream.numel() == 0 or tuple(seg_start.shape) != (n,) or tuple(seg_bytes.shape) != (n,):
        raise ValueError(f"stream must be a non-empty [bytes] and seg_start, seg_bytes [{n}] ({V} frames of {mcus} MCUs at interval "
                         f"{restart_interval}), got {tuple(stream.shape)}, {tuple(seg_start.shape)}, {tuple(seg_bytes.shape)}")
    if tables.numel() != 4 * _lib.EW_JPEG_HUFF_TABLE_BYTES:
        raise ValueError(f"tables must hold 4 x {_lib.EW_JPEG_HUFF_TABLE_BYTES} bytes, got {tables.numel()}")
    shape = (V, mcu_rows, mcu_cols, blocks_per_mcu, 64)
    if out is None:
        out = torch.empty(shape, dtype=torch.int16, device=stream.device)
    elif tuple(out.shape) != shape:
        raise ValueError(f"out must be {shape}, got {tuple(out.shape)}")
    _req(out, torch.int16, "out")
    status = torch.empty(n, dtype=torch.int32, device=stream.device)
    _call("ew_jpeg_huffman_decode", _ptr(stream), stream.numel(), _ptr(seg_start), _ptr(seg_bytes), _ptr(_aligned(tables, 4)), _ptr(out),
          _ptr(status), n, V, mcu_rows, mcu_cols, blocks_per_mcu, restart_interval)
    return out, status


def jpeg_idct(coef, qtables, out=None):
    """coef int16 [V, mcu_rows, mcu_cols, 6 | 3, 64] and qtables uint8 [2,64] (natural order, luminance first), on the device -> the
    sample planes (y uint8 [V, mcu_rows * m, mcu_cols * m] with m = 16 | 8, cb, cr uint8 [V, mcu_rows * 8, mcu_cols * 8]): dequantised,
    inverse DCT, + 128, rounded half to even and clamped to 0..255 (ew_jpeg_idct).  `out`: three such tensors to write into."""
    _req(coef, torch.int16, "coef"); _req(qtables, torch.uint8, "qtables")
    if coef.ndim != 5 or coef.shape[3] not in (3, 6) or coef.shape[4] != 64 or coef.numel() == 0:
        raise ValueError(f"coef must be [V, mcu_rows, mcu_cols, 6 | 3, 64], got {tuple(coef.shape)}")
    if tuple(qtables.shape) != (2, 64):
        raise ValueError(f"qtables must be [2,64], got {tuple(qtables.shape)}")
    V, mr, mc, bpm, _ = coef.shape
    m = 16 if bpm == 6 else 8
    shapes = ((V, mr * m, mc * m), (V, mr * 8, mc * 8), (V, mr * 8, mc * 8))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.uint8, device=coef.device) for s in shapes)
    elif len(out) != 3 or any(tuple(o.shape) != s for o, s in zip(out, shapes)):
        raise ValueError(f"out must be three tensors {shapes}, got {[tuple(o.shape) for o in out]}")
    for o in out:
        _req(o, torch.uint8, "out")
    _call("ew_jpeg_idct", _ptr(_aligned(coef)), _ptr(qtables), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), V, mr, mc, bpm)
    return tuple(out)


def jpeg_planes_to_rgb(planes, H, W, subsampling="4:2:0", out=None):
    """planes (y, cb, cr) of jpeg_idct -> uint8 [V,H,W,3] on the device: cropped to H x W, the 4:2:0 chroma upsampled with the centred
    triangle filter, JFIF YCbCr -> RGB in float32 (ew_jpeg_planes_to_rgb).  `out`: a tensor of that shape to write into."""
    if subsampling not in JPEG_SAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(JPEG_SAMPLING)}, got {subsampling!r}")
    mode, mcu, _ = JPEG_SAMPLING[subsampling]
    if len(planes) != 3:
        raise ValueError("planes must be (y, cb, cr)")
    y, cb, cr = (_req(p, torch.uint8, "planes") for p in planes)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"H and W must be 1..65535, got {H}, {W}")
    V, mr, mc = y.shape[0], -(-H // mcu), -(-W // mcu)
    want = ((V, mr * mcu, mc * mcu), (V, mr * 8, mc * 8), (V, mr * 8, mc * 8))
    if V < 1 or any(tuple(p.shape) != s for p, s in zip((y, cb, cr), want)):
        raise ValueError(f"the planes of {H} x {W} frames at {subsampling} are {want}, got {[tuple(p.shape) for p in planes]}")
    if out is None:
        out = torch.empty(V, H, W, 3, dtype=torch.uint8, device=y.device)
    elif tuple(out.shape) != (V, H, W, 3):
        raise ValueError(f"out must be {(V, H, W, 3)}, got {tuple(out.shape)}")
    _req(out, torch.uint8, "out")
    _call("ew_jpeg_planes_to_rgb", _ptr(y), _ptr(cb), _ptr(cr), _ptr(out), V, H, W, mode)
    return out


def resize_linear_u8(src, h, w, out=None):
    """src uint8 [V,H,W,3] on the device -> uint8 [V,h,w,3]: bilinear sampling at half-pixel centres without antialiasing, neighbours
    clamped to the image, rounded half to even (ew_resize_linear_u8): what cv2.resize(frame, (w, h)) states, unlike resize_aa_u8."""
    _req(src, torch.uint8, "src")
    if src.ndim != 4 or src.shape[3] != 3 or src.numel() == 0:
        raise ValueError(f"src must be a non-empty [V,H,W,3], got {tuple(src.shape)}")
    if not (isinstance(h, (int, np.integer)) and isinstance(w, (int, np.integer)) and 1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"h and w must be integers 1..65535, got {h!r}, {w!r}")
    V, H, W, _ = src.shape
    if out is None:
        out = torch.empty(V, h, w, 3, dtype=torch.uint8, device=src.device)
    elif tuple(out.shape) != (V, h, w, 3):
        raise ValueError(f"out must be {(V, h, w, 3)}, got {tuple(out.shape)}")
    _req(out, torch.uint8, "out")
    _call("ew_resize_linear_u8", _ptr(src), _ptr(out), V, H, W, int(h), int(w))
    return out


def _mvs_out(out, shape, dtype, device, name):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(out.shape)}")
    return _req(out, dtype, name)


def mvs_luma(frames_u8, out=None):
    """frames uint8 [F,H,W,3] on the device -> grey uint8 [F,H,W] = (77 R + 150 G + 29 B + 128) >> 8 (ew_mvs_luma_u8)."""
    if frames_u8.dtype != torch.uint8:
        raise TypeError(f"frames_u8: expected {torch.uint8}, got {frames_u8.dtype}")
    if frames_u8.ndim != 4 or frames_u8.shape[3] != 3 or frames_u8.numel() == 0:
        raise ValueError(f"frames_u8 must be a non-empty [F,H,W,3], got {tuple(frames_u8.shape)}")
    _req(frames_u8, torch.uint8, "frames_u8")
    F_, H, W, _ = frames_u8.shape
    out = _mvs_out(out, (F_, H, W), torch.uint8, frames_u8.device, "out")
    _call("ew_mvs_luma_u8", _ptr(frames_u8), _ptr(out), F_, H, W)
    return out


def _mvs_sources(src_index, F_):
    if src_index.ndim != 2 or src_index.shape[0] != F_ or src_index.shape[1] < 1:
        raise ValueError(f"src_index must be [F = {F_}, S >= 1], got {tuple(src_index.shape)}")
    _req(src_index, torch.int32, "src_index")
    return src_index.shape[1]


def mvs_plane_sweep(grey, homographies, src_index, inv_depth, patch_radius=2, oob_cost=48.0, out=None):
    """grey uint8 [F,H,W], homographies fp32 [F,S,D,3,3] (reference pixel -> source pixel), src_index int32 [F,S] (-1: absent), inv_depth
    fp32 [F,D] -> (depth fp32, conf fp32, winner int32, winner cost fp32), each [F,H,W] (ew_mvs_plane_sweep).
    out: the four output tensors to write into."""
    if grey.ndim != 3 or grey.numel() == 0:
        raise ValueError(f"grey must be a non-empty [F,H,W], got {tuple(grey.shape)}")
    _req(grey, torch.uint8, "grey")
    F_, H, W = grey.shape
    S = _mvs_sources(src_index, F_)
    if inv_depth.ndim != 2 or inv_depth.shape[0] != F_ or inv_depth.shape[1] < 1:
        raise ValueError(f"inv_depth must be [F = {F_}, D >= 1], got {tuple(inv_depth.shape)}")
    D = inv_depth.shape[1]
    if tuple(homographies.shape) != (F_, S, D, 3, 3):
        raise ValueError(f"homographies must be {(F_, S, D, 3, 3)}, got {tuple(homographies.shape)}")
    if patch_radius not in (0, 1, 2, 3):
        raise ValueError(f"patch_radius must be 0 .. 3, got {patch_radius!r}")
    _req(homographies, torch.float32, "homographies"); _req(inv_depth, torch.float32, "inv_depth")
    dev = grey.device
    given = out if out is not None else (None,) * 4
    depth = _mvs_out(given[0], (F_, H, W), torch.float32, dev, "out[0]")
    conf = _mvs_out(given[1], (F_, H, W), torch.float32, dev, "out[1]")
    winner = _mvs_out(given[2], (F_, H, W), torch.int32, dev, "out[2]")
    cost = _mvs_out(given[3], (F_, H, W), torch.float32, dev, "out[3]")
    _call("ew_mvs_plane_sweep", _ptr(grey), _ptr(homographies), _ptr(src_index), _ptr(inv_depth), _ptr(depth), _ptr(conf), _ptr(winner),
          _ptr(cost), F_, H, W, S, D, int(patch_radius), float(oob_cost))
    return depth, conf, winner, cost


def mvs_consistency(depth, rel_pose, src_index, conf, fx, fy, cx, cy, rel_tol=0.02, min_consistent=2):
    """depth fp32 [F,H,W], rel_pose fp32 [F,S,3,4] (reference camera -> source camera), src_index int32 [F,S]; conf fp32 [F,H,W] is set
    to 0 IN PLACE where fewer than min_consistent present sources hold a depth within rel_tol of the lifted pixel's (ew_mvs_consistency).
    Returns conf."""
    if depth.ndim != 3 or depth.numel() == 0:
        raise ValueError(f"depth must be a non-empty [F,H,W], got {tuple(depth.shape)}")
    _req(depth, torch.float32, "depth")
    F_, H, W = depth.shape
    S = _mvs_sources(src_index, F_)
    if tuple(rel_pose.shape) != (F_, S, 3, 4):
        raise ValueError(f"rel_pose must be {(F_, S, 3, 4)}, got {tuple(rel_pose.shape)}")
    if tuple(conf.shape) != (F_, H, W):
        raise ValueError(f"conf must be {(F_, H, W)}, got {tuple(conf.shape)}")
    _req(rel_pose, torch.float32, "rel_pose"); _req(conf, torch.float32, "conf")
    _call("ew_mvs_consistency", _ptr(depth), _ptr(rel_pose), _ptr(src_index), _ptr(conf), F_, H, W, S, float(fx), float(fy), float(cx),
          float(cy), float(rel_tol), int(min_consistent))
    return conf


def mvs_sphere_sweep(grey, rel_pose, src_index, inv_dist, patch_radius=2, out=None):
    """grey uint8 [F,He,We] (equirectangular), rel_pose fp32 [F,S,3,4] (reference panorama camera -> source panorama camera), src_index
    int32 [F,S] (-1: absent), inv_dist fp32 [F,D] -> (radial distance fp32, conf fp32, winner int32, winner cost fp32), each [F,He,We]
    (ew_mvs_sphere_sweep).  out: the four output tensors to write into."""
    if grey.ndim != 3 or grey.numel() == 0:
        raise ValueError(f"grey must be a non-empty [F,He,We], got {tuple(grey.shape)}")
    _req(grey, torch.uint8, "grey")
    F_, H, W = grey.shape
    S = _mvs_sources(src_index, F_)
    if inv_dist.ndim != 2 or inv_dist.shape[0] != F_ or inv_dist.shape[1] < 1:
        raise ValueError(f"inv_dist must be [F = {F_}, D >= 1], got {tuple(inv_dist.shape)}")
    D = inv_dist.shape[1]
    if tuple(rel_pose.shape) != (F_, S, 3, 4):
        raise ValueError(f"rel_pose must be {(F_, S, 3, 4)}, got {tuple(rel_pose.shape)}")
    if patch_radius not in (0, 1, 2, 3):
        raise ValueError(f"patch_radius must be 0 .. 3, got {patch_radius!r}")
    if W < 2 * patch_radius + 1:
        raise ValueError(f"We = {W} is narrower than the window of 2 x {patch_radius} + 1 columns")
    _req(rel_pose, torch.float32, "rel_pose"); _req(inv_dist, torch.float32, "inv_dist")
    dev = grey.device
    given = out if out is not None else (None,) * 4
    dist = _mvs_out(given[0], (F_, H, W), torch.float32, dev, "out[0]")
    conf = _mvs_out(given[1], (F_, H, W), torch.float32, dev, "out[1]")
    winner = _mvs_out(given[2], (F_, H, W), torch.int32, dev, "out[2]")
    cost = _mvs_out(given[3], (F_, H, W), torch.float32, dev, "out[3]")
    _call("ew_mvs_sphere_sweep", _ptr(grey), _ptr(rel_pose), _ptr(src_index), _ptr(inv_dist), _ptr(dist), _ptr(conf), _ptr(winner),
          _ptr(cost), F_, H, W, S, D, int(patch_radius))
    return dist, conf, winner, cost


def mvs_sphere_consistency(dist, rel_pose, src_index, conf, rel_tol=0.02, min_consistent=2):
    """dist fp32 [F,He,We] (radial), rel_pose fp32 [F,S,3,4], src_index int32 [F,S]; conf fp32 [F,He,We] is set to 0 IN PLACE where fewer
    than min_consistent present sources hold, in the lifted pixel's direction, a distance within rel_tol of the pixel's own
    (ew_mvs_sphere_consistency).  Returns conf."""
    if dist.ndim != 3 or dist.numel() == 0:
        raise ValueError(f"dist must be a non-empty [F,He,We], got {tuple(dist.shape)}")
    _req(dist, torch.float32, "dist")
    F_, H, W = dist.shape
    S = _mvs_sources(src_index, F_)
    if tuple(rel_pose.shape) != (F_, S, 3, 4):
        raise ValueError(f"rel_pose must be {(F_, S, 3, 4)}, got {tuple(rel_pose.shape)}")
    if tuple(conf.shape) != (F_, H, W):
        raise ValueError(f"conf must be {(F_, H, W)}, got {tuple(conf.shape)}")
    if not rel_tol >= 0:
        raise ValueError(f"rel_tol = {rel_tol!r} must not be negative")
    _req(rel_pose, torch.float32, "rel_pose"); _req(conf, torch.float32, "conf")
    _call("ew_mvs_sphere_consistency", _ptr(dist), _ptr(rel_pose), _ptr(src_index), _ptr(conf), F_, H, W, S, float(rel_tol),
          int(min_consistent))
    return conf


def pano_unproject(dist, c2w, out=None):
    """dist fp32 [F,He,We] (radial distance per equirectangular pixel), c2w fp32 [F,3,4] (panorama camera -> world) -> world points fp32
    [F,He,We,3] = R (dir dist) + t (ew_pano_unproject): the spherical counterpart of depth_unproject."""
    if dist.ndim != 3 or dist.numel() == 0:
        raise ValueError(f"dist must be a non-empty [F,He,We], got {tuple(dist.shape)}")
    _req(dist, torch.float32, "dist")
    F_, H, W = dist.shape
    if tuple(c2w.shape) != (F_, 3, 4):
        raise ValueError(f"c2w must be {(F_, 3, 4)}, got {tuple(c2w.shape)}")
    _req(c2w, torch.float32, "c2w")
    out = _mvs_out(out, (F_, H, W, 3), torch.float32, dist.device, "out")
    _call("ew_pano_unproject", _ptr(dist), _ptr(c2w), _ptr(out), F_, H, W)
    return out


MVS_COST_MAX, MVS_SGM_MAX_D = _lib.EW_MVS_COST_MAX, _lib.EW_MVS_SGM_MAX_D


def _mvs_view_range(view_begin, n_views, F_):
    """(view_begin, n_views) of the views a volume call writes; n_views None: all from view_begin on"""
    view_begin = int(view_begin)
    n_views = F_ - view_begin if n_views is None else int(n_views)
    if view_begin < 0 or n_views < 1 or view_begin + n_views > F_:
        raise ValueError(f"views {view_begin} .. {view_begin} + {n_views} - 1 must lie in [0, F = {F_})")
    return view_begin, n_views


def _mvs_cost_scale(cost_scale):
    cost_scale = float(cost_scale)
    if not (cost_scale > 0 and np.isfinite(cost_scale)):
        raise ValueError(f"cost_scale = {cost_scale!r} must be positive and finite")
    return cost_scale


def mvs_plane_sweep_volume(grey, homographies, src_index, inv_depth, patch_radius=2, oob_cost=48.0, cost_scale=32.0, view_begin=0,
                           n_views=None, out=None):
    """The inputs of mvs_plane_sweep -> the quantised cost volume uint16 [n_views,H,W,D] of the views view_begin .. view_begin + n_views - 1
    (default: all from view_begin on): q = min(4095, floor(C cost_scale + 0.5)) of the very C(k) mvs_plane_sweep takes its winner from
    (ew_mvs_plane_sweep_volume).  grey holds all F views.  out: the volume to write into."""
    if grey.ndim != 3 or grey.numel() == 0:
        raise ValueError(f"grey must be a non-empty [F,H,W], got {tuple(grey.shape)}")
    _req(grey, torch.uint8, "grey")
    F_, H, W = grey.shape
    S = _mvs_sources(src_index, F_)
    if inv_depth.ndim != 2 or inv_depth.shape[0] != F_ or inv_depth.shape[1] < 1:
        raise ValueError(f"inv_depth must be [F = {F_}, D >= 1], got {tuple(inv_depth.shape)}")
    D = inv_depth.shape[1]
    if tuple(homographies.shape) != (F_, S, D, 3, 3):
        raise ValueError(f"homographies must be {(F_, S, D, 3, 3)}, got {tuple(homographies.shape)}")
    if patch_radius not in (0, 1, 2, 3):
        raise ValueError(f"patch_radius must be 0 .. 3, got {patch_radius!r}")
    cost_scale = _mvs_cost_scale(cost_scale)
    view_begin, n_views = _mvs_view_range(view_begin, n_views, F_)
    _req(homographies, torch.float32, "homographies"); _req(inv_depth, torch.float32, "inv_depth")
    cost = _mvs_out(out, (n_views, H, W, D), torch.uint16, grey.device, "out")
    _call("ew_mvs_plane_sweep_volume", _ptr(grey), _ptr(homographies), _ptr(src_index), _ptr(inv_depth), _ptr(cost), F_, H, W, S, D,
          int(patch_radius), float(oob_cost), cost_scale, view_begin, n_views)
    return cost


def mvs_sphere_sweep_volume(grey, rel_pose, src_index, inv_dist, patch_radius=2, cost_scale=32.0, view_begin=0, n_views=None, out=None):
    """The inputs of mvs_sphere_sweep -> the quantised cost volume uint16 [n_views,He,We,D] of the panoramas view_begin .. view_begin +
    n_views - 1, as mvs_plane_sweep_volume (ew_mvs_sphere_sweep_volume).  out: the volume to write into."""
    if grey.ndim != 3 or grey.numel() == 0:
        raise ValueError(f"grey must be a non-empty [F,He,We], got {tuple(grey.shape)}")
    _req(grey, torch.uint8, "grey")
    F_, H, W = grey.shape
    S = _mvs_sources(src_index, F_)
    if inv_dist.ndim != 2 or inv_dist.shape[0] != F_ or inv_dist.shape[1] < 1:
        raise ValueError(f"inv_dist must be [F = {F_}, D >= 1], got {tuple(inv_dist.shape)}")
    D = inv_dist.shape[1]
    if tuple(rel_pose.shape) != (F_, S, 3, 4):
        raise ValueError(f"rel_pose must be {(F_, S, 3, 4)}, got {tuple(rel_pose.shape)}")
    if patch_radius not in (0, 1, 2, 3):
        raise ValueError(f"patch_radius must be 0 .. 3, got {patch_radius!r}")
    if W < 2 * patch_radius + 1:
        raise ValueError(f"We = {W} is narrower than the window of 2 x {patch_radius} + 1 columns")
    cost_scale = _mvs_cost_scale(cost_scale)
    view_begin, n_views = _mvs_view_range(view_begin, n_views, F_)
    _req(rel_pose, torch.float32, "rel_pose"); _req(inv_dist, torch.float32, "inv_dist")
    cost = _mvs_out(out, (n_views, H, W, D), torch.uint16, grey.device, "out")
    _call("ew_mvs_sphere_sweep_volume", _ptr(grey), _ptr(rel_pose), _ptr(src_index), _ptr(inv_dist), _ptr(cost), F_, H, W, S, D,
          int(patch_radius), cost_scale, view_begin, n_views)
    return cost


def _mvs_zncc_options(patch_radius, var_floor):
    """patch_radius 1 .. 3 (a single tap has no variance) and a finite var_floor >= 0, or ValueError -> (int, float)"""
    if patch_radius not in (1, 2, 3):
        raise ValueError(f"patch_radius must be 1 .. 3 for the zncc cost, got {patch_radius!r}")
    var_floor = float(var_floor)
    if not (var_floor >= 0 and np.isfinite(var_floor)):
        raise ValueError(f"var_floor = {var_floor!r} must be finite and not negative")
    return int(patch_radius), var_floor


def _mvs_plane_inputs(grey, homographies, src_index, inv_depth):
    """the shape and dtype checks of mvs_plane_sweep -> (F, H, W, S, D)"""
    if grey.ndim != 3 or grey.numel() == 0:
        raise ValueError(f"grey must be a non-empty [F,H,W], got {tuple(grey.shape)}")
    _req(grey, torch.uint8, "grey")
    F_, H, W = grey.shape
    S = _mvs_sources(src_index, F_)
    if inv_depth.ndim != 2 or inv_depth.shape[0] != F_ or inv_depth.shape[1] < 1:
        raise ValueError(f"inv_depth must be [F = {F_}, D >= 1], got {tuple(inv_depth.shape)}")
    D = inv_depth.shape[1]
    if tuple(homographies.shape) != (F_, S, D, 3, 3):
        raise ValueError(f"homographies must be {(F_, S, D, 3, 3)}, got {tuple(homographies.shape)}")
    _req(homographies, torch.float32, "homographies"); _req(inv_depth, torch.float32, "inv_depth")
    return F_, H, W, S, D


def _mvs_sphere_inputs(grey, rel_pose, src_index, inv_dist, patch_radius):
    """the shape and dtype checks of mvs_sphere_sweep -> (F, He, We, S, D)"""
    if grey.ndim != 3 or grey.numel() == 0:
        raise ValueError(f"grey must be a non-empty [F,He,We], got {tuple(grey.shape)}")
    _req(grey, torch.uint8, "grey")
    F_, H, W = grey.shape
    S = _mvs_sources(src_index, F_)
    if inv_dist.ndim != 2 or inv_dist.shape[0] != F_ or inv_dist.shape[1] < 1:
        raise ValueError(f"inv_dist must be [F = {F_}, D >= 1], got {tuple(inv_dist.shape)}")
    D = inv_dist.shape[1]
    if tuple(rel_pose.shape) != (F_, S, 3, 4):
        raise ValueError(f"rel_pose must be {(F_, S, 3, 4)}, got {tuple(rel_pose.shape)}")
    if W < 2 * patch_radius + 1:
        raise ValueError(f"We = {W} is narrower than the window of 2 x {patch_radius} + 1 columns")
    _req(rel_pose, torch.float32, "rel_pose"); _req(inv_dist, torch.float32, "inv_dist")
    return F_, H, W, S, D


def _mvs_four_outputs(out, shape, dev):
    given = out if out is not None else (None,) * 4
    return [_mvs_out(g, shape, dt, dev, f"out[{i}]") for i, (g, dt) in enumerate(zip(given, (torch.float32, torch.float32, torch.int32, torch.float32)))]


def mvs_plane_sweep_zncc(grey, homographies, src_index, inv_depth, patch_radius=2, oob_cost=100.0, var_floor=1.0, out=None):
    """The inputs of mvs_plane_sweep -> (depth fp32, conf fp32, winner int32, winner cost fp32 in percent), each [F,H,W], with
    100 (1 - ZNCC) over the window as the matching cost (ew_mvs_plane_sweep_zncc).  patch_radius 1 .. 3; oob_cost: the cost,
    in percent, of a source whose window leaves it; var_floor: grey levels squared.  out: the four output tensors to write into."""
    patch_radius, var_floor = _mvs_zncc_options(patch_radius, var_floor)
    F_, H, W, S, D = _mvs_plane_inputs(grey, homographies, src_index, inv_depth)
    depth, conf, winner, cost = _mvs_four_outputs(out, (F_, H, W), grey.device)
    _call("ew_mvs_plane_sweep_zncc", _ptr(grey), _ptr(homographies), _ptr(src_index), _ptr(inv_depth), _ptr(depth), _ptr(conf), _ptr(winner),
          _ptr(cost), F_, H, W, S, D, patch_radius, float(oob_cost), var_floor)
    return depth, conf, winner, cost


def mvs_plane_sweep_zncc_volume(grey, homographies, src_index, inv_depth, patch_radius=2, oob_cost=100.0, var_floor=1.0, cost_scale=16.0,
                                view_begin=0, n_views=None, out=None):
    """The inputs of mvs_plane_sweep_zncc -> the quantised cost volume uint16 [n_views,H,W,D] of the views view_begin .. view_begin +
    n_views - 1: q = min(4095, floor(C cost_scale + 0.5)) of the very C(k) mvs_plane_sweep_zncc takes its winner from
    (ew_mvs_plane_sweep_zncc_volume).  out: the volume to write into."""
    patch_radius, var_floor = _mvs_zncc_options(patch_radius, var_floor)
    F_, H, W, S, D = _mvs_plane_inputs(grey, homographies, src_index, inv_depth)
    cost_scale = _mvs_cost_scale(cost_scale)
    view_begin, n_views = _mvs_view_range(view_begin, n_views, F_)
    cost = _mvs_out(out, (n_views, H, W, D), torch.uint16, grey.device, "out")
    _call("ew_mvs_plane_sweep_zncc_volume", _ptr(grey), _ptr(homographies), _ptr(src_index), _ptr(inv_depth), _ptr(cost), F_, H, W, S, D,
          patch_radius, float(oob_cost), var_floor, cost_scale, view_begin, n_views)
    return cost


def mvs_sphere_sweep_zncc(grey, rel_pose, src_index, inv_dist, patch_radius=2, var_floor=1.0, out=None):
    """The inputs of mvs_sphere_sweep -> (radial distance fp32, conf fp32, winner int32, winner cost fp32 in percent), each [F,He,We], with
    100 (1 - ZNCC) over the window as the matching cost (ew_mvs_sphere_sweep_zncc).  patch_radius 1 .. 3."""
    patch_radius, var_floor = _mvs_zncc_options(patch_radius, var_floor)
    F_, H, W, S, D = _mvs_sphere_inputs(grey, rel_pose, src_index, inv_dist, patch_radius)
    dist, conf, winner, cost = _mvs_four_outputs(out, (F_, H, W), grey.device)
    _call("ew_mvs_sphere_sweep_zncc", _ptr(grey), _ptr(rel_pose), _ptr(src_index), _ptr(inv_dist), _ptr(dist), _ptr(conf), _ptr(winner),
          _ptr(cost), F_, H, W, S, D, patch_radius, var_floor)
    return dist, conf, winner, cost


def mvs_sphere_sweep_zncc_volume(grey, rel_pose, src_index, inv_dist, patch_radius=2, var_floor=1.0, cost_scale=16.0, view_begin=0,
                                 n_views=None, out=None):
    """The inputs of mvs_sphere_sweep_zncc -> the quantised cost volume uint16 [n_views,He,We,D], as mvs_plane_sweep_zncc_volume
    (ew_mvs_sphere_sweep_zncc_volume).  out: the volume to write into."""
    patch_radius, var_floor = _mvs_zncc_options(patch_radius, var_floor)
    F_, H, W, S, D = _mvs_sphere_inputs(grey, rel_pose, src_index, inv_dist, patch_radius)
    cost_scale = _mvs_cost_scale(cost_scale)
    view_begin, n_views = _mvs_view_range(view_begin, n_views, F_)
    cost = _mvs_out(out, (n_views, H, W, D), torch.uint16, grey.device, "out")
    _call("ew_mvs_sphere_sweep_zncc_volume", _ptr(grey), _ptr(rel_pose), _ptr(src_index), _ptr(inv_dist), _ptr(cost), F_, H, W, S, D,
          patch_radius, var_floor, cost_scale, view_begin, n_views)
    return cost


def _mvs_volume(vol, name):
    if vol.ndim != 4 or vol.numel() == 0:
        raise ValueError(f"{name} must be a non-empty [N,H,W,D], got {tuple(vol.shape)}")
    _req(vol, torch.uint16, name)
    if not 1 <= vol.shape[3] <= MVS_SGM_MAX_D:
        raise ValueError(f"{name}: D = {vol.shape[3]} must be 1 .. {MVS_SGM_MAX_D}")
    return tuple(vol.shape)


def mvs_sgm_check_penalties(P1, P2, paths):
    """0 <= P1 <= P2 <= 4095 as integers and paths in {4, 8}, or ValueError -> (P1, P2, paths) as ints"""
    if int(P1) != P1 or int(P2) != P2 or not 0 <= P1 <= P2 <= MVS_COST_MAX:
        raise ValueError(f"0 <= P1 = {P1!r} <= P2 = {P2!r} <= {MVS_COST_MAX} (integers) does not hold")
    if paths not in (4, 8):
        raise ValueError(f"paths must be 4 or 8, got {paths!r}")
    return int(P1), int(P2), int(paths)


def mvs_sgm_aggregate(cost, P1, P2, paths=4, out=None):
    """cost uint16 [N,H,W,D] with values <= 4095 -> agg uint16 [N,H,W,D]: the sum over 4 or 8 path directions of the semi-global
    recurrence with the penalties 0 <= P1 <= P2 <= 4095, in the volume's units (ew_mvs_sgm_aggregate).  The values are
    not checked: a cost above 4095 can wrap the 16-bit sum.  out: the volume to write into (not `cost`)."""
    shape = _mvs_volume(cost, "cost")
    P1, P2, paths = mvs_sgm_check_penalties(P1, P2, paths)
    agg = _mvs_out(out, shape, torch.uint16, cost.device, "out")
    if agg.data_ptr() == cost.data_ptr():
        raise ValueError("out must not be the cost volume itself")
    N, H, W, D = shape
    _call("ew_mvs_sgm_aggregate", _ptr(cost), _ptr(agg), N, H, W, D, P1, P2, paths)
    return agg


def mvs_sgm_select(agg, inv, src_index, view_begin=0, out=None):
    """agg uint16 [N,H,W,D] of the views view_begin .. view_begin + N - 1, inv fp32 [F,D] (inverse depths or distances), src_index int32
    [F,S] -> (depth or distance fp32, conf fp32, winner int32, winner cost fp32 in aggregated units), each [N,H,W]: mvs_plane_sweep's
    winner, parabola and confidence rules on the aggregated costs (ew_mvs_sgm_select).  out: the four output tensors to write into."""
    N, H, W, D = _mvs_volume(agg, "agg")
    if inv.ndim != 2 or inv.shape[1] != D or inv.shape[0] < 1:
        raise ValueError(f"inv must be [F, D = {D}], got {tuple(inv.shape)}")
    F_ = inv.shape[0]
    S = _mvs_sources(src_index, F_)
    view_begin, _ = _mvs_view_range(view_begin, N, F_)
    _req(inv, torch.float32, "inv")
    dev = agg.device
    given = out if out is not None else (None,) * 4
    depth = _mvs_out(given[0], (N, H, W), torch.float32, dev, "out[0]")
    conf = _mvs_out(given[1], (N, H, W), torch.float32, dev, "out[1]")
    winner = _mvs_out(given[2], (N, H, W), torch.int32, dev, "out[2]")
    cost = _mvs_out(given[3], (N, H, W), torch.float32, dev, "out[3]")
    _call("ew_mvs_sgm_select", _ptr(agg), _ptr(inv), _ptr(src_index), _ptr(depth), _ptr(conf), _ptr(winner), _ptr(cost), F_, H, W, S, D,
          view_begin, N)
    return depth, conf, winner, cost


def equi2pers(equi, rot, Hp, Wp, fov_x):
    _req(equi, torch.uint8, "equi"); _req(rot, torch.float32, "rot")
    F_, He, We, _ = equi.shape
    out = torch.empty(F_, Hp, Wp, 3, dtype=torch.uint8, device=equi.device)
    _call("ew_equi2pers", _ptr(equi), _ptr(rot), _ptr(out), F_, He, We, Hp, Wp, float(fov_x))
    return out


def resize_aa_u8(src, coeffs_h, coeffs_v, Ho, Wo):
    """src uint8 [V,Hi,Wi,3]; coeffs_* = (kk int32 [n_out,ksize], bounds int32 [n_out,2]) device tensors -> uint8 [V,Ho,Wo,3]."""
    _req(src, torch.uint8, "src")
    V, Hi, Wi, _ = src.shape
    tmp = torch.empty(V, Hi, Wo, 3, dtype=torch.uint8, device=src.device)
    dst = torch.empty(V, Ho, Wo, 3, dtype=torch.uint8, device=src.device)
    (kh, bh), (kv, bv) = coeffs_h, coeffs_v
    _call("ew_resize_aa_u8", _ptr(src), _ptr(tmp), _ptr(dst), _ptr(kh), _ptr(bh), kh.shape[1], _ptr(kv), _ptr(bv), kv.shape[1], V, Hi, Wi, Ho, Wo)
    return dst


def u8_hwc_to_f32_chw(src):
    _req(src, torch.uint8, "src")
    V, H, W, _ = src.shape
    dst = torch.empty(V, 3, H, W, dtype=torch.float32, device=src.device)
    _call("ew_u8_hwc_to_f32_chw", _ptr(src), _ptr(dst), V, H, W)
    return dst


def f32_chw_to_u8_hwc(src):
    """fp32 [V,3,H,W] in [-1,1] -> uint8 [V,H,W,3] (round-half-even of clamp(x/2+0.5,0,1)*255: the pipeline's PIL frames)."""
    _req(src, torch.float32, "src")
    V, _, H, W = src.shape
    dst = torch.empty(V, H, W, 3, dtype=torch.uint8, device=src.device)
    _call("ew_f32_chw_to_u8_hwc", _ptr(src), _ptr(dst), V, H, W)
    return dst


def pano_yaw_rotate(src, yaw_deg):
    """Yaw rotation of equirectangular panoramas (Navigator.rotate_panorama, navigator_evoworld.py:466-512), bit-exact:
    src fp32 [V,3,H,W] or uint8 [V,H,W,3] (the 8-bit frames; mapped x/255*2-1 in the same pass), yaw_deg [V] degrees (a float32
    tensor on any device, or numbers rounded to float32 as torch.tensor(..., dtype=float32) does) -> fp32 [V,3,H,W]."""
    if src.dtype == torch.uint8:
        _req(src, torch.uint8, "src")
        if src.ndim != 4 or src.shape[3] != 3:
            raise ValueError(f"src: expected uint8 [V,H,W,3], got {tuple(src.shape)}")
        V, H, W, _ = src.shape
    else:
        _req(src, torch.float32, "src")
        if src.ndim != 4 or src.shape[1] != 3:
            raise ValueError(f"src: expected fp32 [V,3,H,W], got {tuple(src.shape)}")
        V, _, H, W = src.shape
    if isinstance(yaw_deg, torch.Tensor) and yaw_deg.dtype != torch.float32:
        raise TypeError(f"yaw_deg: expected torch.float32, got {yaw_deg.dtype}")
    yaw = torch.as_tensor(yaw_deg, dtype=torch.float32).reshape(-1).to(src.device).contiguous()
    if yaw.numel() != V:
        raise ValueError(f"yaw_deg: expected {V} yaws (one per panorama), got {yaw.numel()}")
    dst = torch.empty(V, 3, H, W, dtype=torch.float32, device=src.device)
    _call("ew_pano_yaw_rotate", _ptr(src), int(src.dtype == torch.uint8), _ptr(yaw), _ptr(dst), V, H, W)
    return dst



METRIC_SSE, METRIC_SSIM = 1, 2


def _metric_frames(a, b):
    """The frame pair of ew_video_metrics / ew_video_metrics_ws, validated -> (layout, F, C, H, W)."""
    if a.dtype == torch.uint8:
        layout = 0
        _req(a, torch.uint8, "a")
        _req(b, torch.uint8, "b")
        if a.ndim != 4:
            raise ValueError(f"a: expected uint8 [F,H,W,C], got {tuple(a.shape)}")
        F_, H, W, C = a.shape
    else:
        layout = 1
        _req(a, torch.float32, "a")
        _req(b, torch.float32, "b")
        if a.ndim != 4:
            raise ValueError(f"a: expected fp32 [F,C,H,W], got {tuple(a.shape)}")
        F_, C, H, W = a.shape
    if b.shape != a.shape or b.device != a.device:
        raise ValueError(f"a {tuple(a.shape)} on {a.device} and b {tuple(b.shape)} on {b.device} differ")
    return layout, F_, C, H, W


def _metric_outputs(what, F_, device, given):
    """fp64 [F] outputs for the bits of `what`: given = ((flag, tensor or None, name), ...) -> [tensor or None per flag]"""
    out = []
    for flag, t, name in given:
        if what & flag and t is None:
            t = torch.empty(F_, dtype=torch.float64, device=device)
        if t is not None:
            _req(t, torch.float64, name)
            if t.numel() != F_:
                raise ValueError(f"{name}: expected {F_} values, got {t.numel()}")
        out.append(t if what & flag else None)
    return out


def video_metrics(a, b, what=METRIC_SSE | METRIC_SSIM, sse=None, ssim=None):
    """Per-frame PSNR / SSIM inputs of frame pairs (ew_video_metrics; calculate_psnr.py:6-15, calculate_ssim.py:6-40): a, b
    uint8 [F,H,W,C] (a pixel is float32(k) / 255.0f) or fp32 [F,C,H,W], C = 1 or 3 -> (sse, ssim), fp64 [F] device tensors
    (None where `what` does not ask for it): sse = the frame's sum of float32 (a - b)^2 in fp64, ssim = the reference's per-frame
    SSIM (mean over the channels).  `sse` / `ssim` may be given as fp64 [F] device views to write into."""
    lib = _lib.load()
    layout, F_, C, H, W = _metric_frames(a, b)
    out = _metric_outputs(what, F_, a.device, ((METRIC_SSE, sse, "sse"), (METRIC_SSIM, ssim, "ssim")))
    ws = torch.empty(max(1, lib.ew_video_metrics_workspace_bytes(F_, C, H, W)), dtype=torch.uint8, device=a.device)
    _call("ew_video_metrics", _ptr(a), _ptr(b), layout, F_, C, H, W, int(what), _ptr(out[0]), _ptr(out[1]), _ptr(ws))
    return out[0], out[1]


def check_row_weights(row_w, H, ssim=False):
    """One weight per image row for ew_video_metrics_ws, validated on the host -> fp64 numpy [H]: finite, >= 0, a positive sum over all
    rows, and with `ssim` over rows 5 .. H-6 too (the centre rows of the 11-row windows)."""
    w = row_w.detach().cpu().numpy() if isinstance(row_w, torch.Tensor) else np.asarray(row_w)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != (H,):
        raise ValueError(f"row_w: expected {H} weights (one per image row), got shape {w.shape}")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("row_w: the weights must be finite and >= 0")
    if not w.sum() > 0:
        raise ValueError("row_w: the weights sum to zero")
    if ssim and H >= 11 and not w[5:H - 5].sum() > 0:
        raise ValueError(f"row_w: the weights of rows 5 .. {H - 6}, the centre rows of the SSIM windows, sum to zero")
    return w


def video_metrics_ws(a, b, row_w, what=METRIC_SSE | METRIC_SSIM, wsse=None, wssim=None):
    """The row-weighted forms of video_metrics (ew_video_metrics_ws): a, b as there; row_w one weight per image row (H values: numpy,
    a sequence or a tensor; metrics.latitude_weights(H) gives WS-PSNR / WS-SSIM of equirectangular frames) -> (wsse, wssim), fp64 [F]
    device tensors (None where `what` does not ask for it): wsse = sum of row_w[y] * float32 (a - b)^2, not normalised; wssim = the SSIM
    map averaged under the weights of its windows' centre rows, then over the channels."""
    lib = _lib.load()
    layout, F_, C, H, W = _metric_frames(a, b)
    w = torch.from_numpy(check_row_weights(row_w, H, ssim=bool(what & METRIC_SSIM))).to(a.device)
    out = _metric_outputs(what, F_, a.device, ((METRIC_SSE, wsse, "wsse"), (METRIC_SSIM, wssim, "wssim")))
    ws = torch.empty(max(1, lib.ew_video_metrics_ws_workspace_bytes(F_, C, H, W)), dtype=torch.uint8, device=a.device)
    _call("ew_video_metrics_ws", _ptr(a), _ptr(b), layout, F_, C, H, W, int(what), _ptr(w), _ptr(out[0]), _ptr(out[1]), _ptr(ws))
    return out[0], out[1]


def gt_dump_map_u8(src):
    """The 8-bit ground-truth frame the reference's episode mode dumps (ew_gt_dump_map_u8: k/255 -> x*2-1 -> tensor_to_pil's
    truncating (x*0.5+0.5)*255, a fixed 256-entry map): uint8 tensor of any shape (device) -> a new one of the same shape."""
    _req(src, torch.uint8, "src")
    dst = torch.empty_like(src)
    _call("ew_gt_dump_map_u8", _ptr(src), _ptr(dst), src.numel())
    return dst


def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _frames_src(t, name, dims="n,H,W"):
    """A batch of frames in [0,1], uint8 [n,H,W,3] or fp32 [n,3,H,W], validated -> (src_kind of the frame entry points, n, H, W);
    `dims` names the three sizes in the message."""
    kind = 1 if t.dtype == torch.uint8 else 2
    _req(t, torch.uint8 if kind == 1 else torch.float32, name)
    if kind == 1:
        n, H, W, C = t.shape if t.ndim == 4 else (0, 0, 0, 0)
    else:
        n, C, H, W = t.shape if t.ndim == 4 else (0, 0, 0, 0)
    if C != 3:
        raise ValueError(f"{name}: expected uint8 [{dims},3] or fp32 [{dims.replace(',', ',3,', 1)}] frames, got {tuple(t.shape)}")
    return kind, n, H, W


def im2col_frames(frames, k, stride, pad, ldk, shift, scale, swap_rb=False):
    """k x k / stride / zero-pad patch rows of a network's first convolution on ew_gemm_f16, straight from the frames
    (ew_im2col_frames_f16): frames in [0,1], uint8 [n,h,w,3] or fp32 [n,3,h,w], mapped 2v - 1 -> (x - shift[c]) / scale[c] on the way
    (network channel c reads frame channel 2 - c when swap_rb) -> fp16 [n*h_out*w_out, ldk], column (ky*k + kx)*3 + c, zero beyond
    k*k*3.  Returns (rows, h_out, w_out)."""
    kind, n, h, w = _frames_src(frames, "src", "n,h,w")
    ho, wo = conv_out_size(h, k, stride, pad), conv_out_size(w, k, stride, pad)
    if ho < 1 or wo < 1:
        raise ValueError(f"im2col: a {k}x{k} window (pad {pad}) does not fit {h}x{w}")
    out = torch.empty(n * ho * wo, ldk, dtype=torch.float16, device=frames.device)
    affine = (ctypes.c_float * 6)(*[float(v) for v in shift], *[float(v) for v in scale])
    _call("ew_im2col_frames_f16", _ptr(frames), kind, _ptr(out), n, h, w, k, stride, pad, ho, wo, ldk, int(bool(swap_rb)), affine)
    return out, ho, wo


def lpips_head(fa, fb, lin, wy, wx, n_out, acc):
    """One LPIPS tap of F frame pairs (ew_lpips_head): fa, fb fp16 [F,h,w,C] pre-ReLU conv outputs, lin fp32 [C], wy [h] / wx [w] fp64
    (lpips.upsample_mean_weights on the device), n_out = H * W of the frames; acc fp64 [F] += the tap's mean over the upsampled map."""
    lib = _lib.load()
    _req(fa, torch.float16, "fa"); _req(fb, torch.float16, "fb"); _req(lin, torch.float32, "lin")
    _req(wy, torch.float64, "wy"); _req(wx, torch.float64, "wx"); _req(acc, torch.float64, "acc")
    if fa.ndim != 4 or fb.shape != fa.shape:
        raise ValueError(f"fa {tuple(fa.shape)} / fb {tuple(fb.shape)}: expected two fp16 [F,h,w,C] tensors of one shape")
    F_, h, w, C = fa.shape
    if lin.numel() != C or wy.numel() != h or wx.numel() != w or acc.numel() != F_:
        raise ValueError(f"lpips_head: lin / wy / wx / acc hold {lin.numel()}, {wy.numel()}, {wx.numel()}, {acc.numel()} values for "
                         f"C, h, w, F = {C}, {h}, {w}, {F_}")
    ws = torch.empty(max(1, lib.ew_lpips_head_workspace_bytes(F_, h, w, C)), dtype=torch.uint8, device=fa.device)
    _call("ew_lpips_head", _ptr(fa), _ptr(fb), _ptr(lin), _ptr(wy), _ptr(wx), F_, h, w, C, float(n_out), _ptr(acc), _ptr(ws))
    return acc


def video_preprocess(clip, h_resized, w_resized, y0, x0, swap_rb=False):
    """styleganv preprocess_single of one clip (ew_video_preprocess_f16): uint8 [T,H,W,3] or fp32 [T,3,H,W] in [0,1] -> fp16
    [T,224,224,8] in [-1,1], channels 3..7 zero: bilinear resize to h_resized x w_resized, 224 x 224 crop at (y0, x0), (x - 0.5) * 2."""
    kind, T, H, W = _frames_src(clip, "clip", "T,H,W")
    out = torch.empty(T, 224, 224, 8, dtype=torch.float16, device=clip.device)
    _call("ew_video_preprocess_f16", _ptr(clip), kind, _ptr(out), T, H, W, h_resized, w_resized, y0, x0, int(bool(swap_rb)))
    return out


def _thwc(x, name):
    _req(x, torch.float16, name)
    if x.ndim != 4:
        raise ValueError(f"{name}: expected fp16 [T,H,W,C], got {tuple(x.shape)}")
    return x.shape


def im2col3d(x, kernel, stride, pads, out_size, ldk, relu=False, out=None):
    """Patch rows of one clip for a 3-D convolution on ew_gemm_f16 (ew_im2col3d_f16): x fp16 [T,H,W,C] (C % 8 == 0; relu: read
    max(x, 0)), kernel / stride / front pads / out_size triples over (t, h, w) -> fp16 [To*Ho*Wo, ldk], column ((dt*kh + dy)*kw + dx)*C + c,
    zero outside the input and beyond kt*kh*kw*C."""
    T, H, W, C = _thwc(x, "x")
    rows = out_size[0] * out_size[1] * out_size[2]
    if out is None:
        out = torch.empty(rows, ldk, dtype=torch.float16, device=x.device)
    else:
        _req(out, torch.float16, "out")
        if out.numel() != rows * ldk:
            raise ValueError(f"out holds {out.numel()} values for {rows} rows of {ldk}")
    _call("ew_im2col3d_f16", _ptr(x), _ptr(out), T, H, W, C, *kernel, *stride, *pads, *out_size, ldk, int(bool(relu)))
    return out


def maxpool3d_relu(x, kernel, stride, pads, out_size):
    """Max pool of max(x, 0) over the taps inside the input (ew_maxpool3d_relu_f16): x fp16 [T,H,W,C] -> [To,Ho,Wo,C]."""
    T, H, W, C = _thwc(x, "x")
    out = torch.empty(*out_size, C, dtype=torch.float16, device=x.device)
    _call("ew_maxpool3d_relu_f16", _ptr(x), _ptr(out), T, H, W, C, *kernel, *stride, *pads, *out_size)
    return out


def i3d_head(x, w, b, out=None):
    """The pre-ReLU Mixed_5c output fp16 [T' >= 2,7,7,1024] -> I3D's 400 logits, fp32 (ew_i3d_head): W @ (mean over the (2,7,7) average
    pool's windows of max(x, 0)) + b, with w fp32 [400,1024] and b fp32 [400]."""
    T, H, W, C = _thwc(x, "x")
    _req(w, torch.float32, "w"); _req(b, torch.float32, "b")
    if tuple(w.shape) != (400, 1024) or tuple(b.shape) != (400,):
        raise ValueError(f"i3d_head: w {tuple(w.shape)} / b {tuple(b.shape)}: expected [400,1024] and [400]")
    if out is None:
        out = torch.empty(400, dtype=torch.float32, device=x.device)
    else:
        _req(out, torch.float32, "out")
        if out.numel() != 400:
            raise ValueError(f"out holds {out.numel()} values, expected 400")
    ws = torch.empty(_lib.load().ew_i3d_head_workspace_bytes(), dtype=torch.uint8, device=x.device)
    _call("ew_i3d_head", _ptr(x), T, H, W, C, _ptr(w), _ptr(b), _ptr(out), _ptr(ws))
    return out


def frames_resize_aa_norm(frames, table_h, table_w, mean, std, swap_rb=False):
    """The Inception-v4 input of a batch of frames (ew_frames_resize_aa_norm_f16): uint8 [F,H,W,3] or fp32 [F,3,H,W] in [0,1] -> fp16
    [F,out_h,out_w,8], channels 3..7 zero: the antialiased bilinear resize of torchvision's Resize on a float tensor, then (x - mean[c]) /
    std[c].  table_h / table_w = (first int32 [n_out], count int32 [n_out], weights fp32 [n_out, taps]) device tensors, as
    latent_mse.resize_table(H, out_h) / (W, out_w) gives them."""
    kind, F_, H, W = _frames_src(frames, "frames", "F,H,W")
    args = []
    for name, (first, count, weights) in (("table_h", table_h), ("table_w", table_w)):
        _req(first, torch.int32, f"{name}[0]"); _req(count, torch.int32, f"{name}[1]"); _req(weights, torch.float32, f"{name}[2]")
        if first.ndim != 1 or count.shape != first.shape or weights.ndim != 2 or weights.shape[0] != first.shape[0]:
            raise ValueError(f"{name}: expected (first [n], count [n], weights [n, taps]), got {tuple(first.shape)}, {tuple(count.shape)}, "
                             f"{tuple(weights.shape)}")
        args += [_ptr(first), _ptr(count), _ptr(weights), weights.shape[1]]
    out_h, out_w = table_h[0].shape[0], table_w[0].shape[0]
    out = torch.empty(F_, out_h, out_w, 8, dtype=torch.float16, device=frames.device)
    mean_std = (ctypes.c_float * 6)(*[float(v) for v in mean], *[float(v) for v in std])
    _call("ew_frames_resize_aa_norm_f16", _ptr(frames), kind, _ptr(out), F_, H, W, out_h, out_w, *args, int(bool(swap_rb)), mean_std)
    return out


def avgpool3x3_relu(x):
    """AvgPool2d(3, stride=1, padding=1, count_include_pad=False) of max(x, 0) (ew_avgpool3x3_relu_f16): fp16 [n,H,W,C] -> the same shape."""
    n, H, W, C = _thwc(x, "x")
    out = torch.empty_like(x)
    _call("ew_avgpool3x3_relu_f16", _ptr(x), _ptr(out), n, H, W, C)
    return out


def global_avgpool_relu(x):
    """fp16 [n,h,w,C] -> fp32 [n,C]: the mean over h * w of max(x, 0), a sequential fp32 sum (ew_global_avgpool_relu_f32)."""
    n, h, w, C = _thwc(x, "x")
    out = torch.empty(n, C, dtype=torch.float32, device=x.device)
    _call("ew_global_avgpool_relu_f32", _ptr(x), _ptr(out), n, h, w, C)
    return out


def blur_axis(x, kern, axis):
    """x fp32 [..., H, W], kern fp32 [k] -> correlation along H (axis 0) or W (axis 1), reflect padding."""
    _req(x, torch.float32, "x"); _req(kern, torch.float32, "kern")
    H, W = x.shape[-2:]
    out = torch.empty_like(x)
    _call("ew_blur_axis_f32", _ptr(x), _ptr(kern), kern.numel(), _ptr(out), x.numel() // (H * W), H, W, axis)
    return out


def bicubic_resize(x, Ho, Wo, scale=None, shift=None):
    """x fp32 [N,C,H,W] -> [N,C,Ho,Wo], bicubic align_corners=True; optional per-channel out = v*scale[c] + shift[c]."""
    _req(x, torch.float32, "x")
    N, C, H, W = x.shape
    out = torch.empty(N, C, Ho, Wo, dtype=torch.float32, device=x.device)
    _call("ew_bicubic_resize_f32", _ptr(x), _ptr(out), N, C, H, W, Ho, Wo, _ptr(scale), _ptr(shift))
    return out


def vit_patchify(x, P, ldk):
    _req(x, torch.float32, "x")
    N, _, S, _ = x.shape
    out = torch.empty(N * (S // P) ** 2, ldk, dtype=torch.float16, device=x.device)
    _call("ew_vit_patchify_f16", _ptr(x), _ptr(out), N, S, P, ldk)
    return out


def attn_small(q, k, v, o, n_seq, S, heads, D, ld, ld_o, scale):
    _call("ew_attn_small_f16", _ptr(q), _ptr(k), _ptr(v), _ptr(o), n_seq, S, heads, D, ld, ld_o, float(scale))
    return o


def ff_pack(w1, b1, w2):
    """Weights of one GEGLU feed-forward (w1 [2*H, C] value rows then gate rows, b1 [2*H], w2 [C, H]; fp32 or fp16, on the
    device) -> (w1p, b1p, w2p) fp16 in the LDS-image packs ew_ff_geglu320_f16 streams (layout: csrc/ff_fused.hip)."""
    dev = w1.device
    H2, C = w1.shape
    H = H2 // 2
    assert C == 320 and H == 1280 and tuple(w2.shape) == (C, H)
    nch = H // 32
    c = torch.arange(nch, device=dev)[:, None]
    r = torch.arange(64, device=dev)[None, :]
    j, i = r // 16, r % 16
    hh, vg = j // 2, j % 2
    src = vg * H + 32 * c + 8 * (i // 4) + 4 * hh + (i % 4)                                 # [nch, 64] proj rows
    sl = torch.arange(8, device=dev)
    w1g = w1.float()[src.reshape(-1)].reshape(nch, 64, C // 64, 8, 8)                       # [c, r, kt, slot, 8]
    perm1 = (sl[None, :] ^ (torch.arange(64, device=dev)[:, None] & 7))                     # packed slot sl <- k-slot sl ^ (r & 7)
    w1g = torch.gather(w1g, 3, perm1[None, :, None, :, None].expand(nch, 64, C // 64, 8, 8))
    w1p = w1g.permute(0, 2, 1, 3, 4).contiguous().to(torch.float16)                         # [c, kt, r, slot, 8]
    b1p = b1.float()[src.reshape(-1)].to(torch.float16).contiguous()
    r2 = torch.arange(C, device=dev)
    jj, i2 = r2 // 16, r2 % 16
    col = (jj // 2) * 32 + (i2 // 4) * 8 + (jj % 2) * 4 + (i2 % 4)                          # staged row -> output channel
    w2g = w2.float()[col].reshape(C, nch, 4, 8)                                              # [r, c, slot, 8]
    gq = torch.tensor([0, 2, 3, 1], device=dev)[(r2 >> 2) & 3]                              # bank-conflict-free slot XOR per row
    perm2 = (torch.arange(4, device=dev)[None, :] ^ gq[:, None])
    w2g = torch.gather(w2g, 2, perm2[:, None, :, None].expand(C, nch, 4, 8))
    w2p = w2g.permute(1, 0, 2, 3).contiguous().to(torch.float16)                             # [c, r, slot, 8]
    return w1p, b1p, w2p


def ff_geglu320(x, pack, b2, out, *, rowbias=None, rows_per_group=1, ld_rowbias=None, r1=None, r2=None, c_acc=1.0, c_r1=1.0, c_r2=1.0):
    """out = c_acc * (GEGLU(x W1^T + b1) W2^T + b2 + rowbias) + c_r1 * r1 + c_r2 * r2 for 320-channel tokens, one kernel
    (ew_ff_geglu320_f16): x fp16 [M, 320] (the LayerNorm output), pack = ff_pack(...); r1 / r2 / out tensors or `Res`, every plane
    a contiguous [M, 320]; b2 fp16 [320]; rowbias fp16 [>= ceil(M / rows_per_group), >= 320] with row stride ld_rowbias."""
    _req(x, torch.float16, "x")
    a = _lib.FfArgs()
    r1h, r1l = _hl(r1)
    r2h, r2l = _hl(r2)
    oh, ol = _hl(out)
    w1p, b1p, w2p = pack
    # the ABI carries no stride for r1 / r2 / out or their lo planes and no extent for b2 / rowbias: anything but dense [M, 320]
    # planes would make the kernel read or write other memory, so it is refused here
    if x.dim() != 2:
        raise ValueError(f"x must be [M, 320] (got {tuple(x.shape)})")
    M = x.shape[0]
    if oh is None:
        raise ValueError("out is required")
    for t, dtype, name in ((oh, torch.float16, "out"), (ol, torch.int8, "out lo plane"), (r1h, torch.float16, "r1"), (r1l, torch.int8, "r1 lo plane"),
                           (r2h, torch.float16, "r2"), (r2l, torch.int8, "r2 lo plane")):
        if t is not None:
            _req(t, dtype, name)
            if tuple(t.shape) != (M, x.shape[1]):
                raise ValueError(f"{name} must be [{M}, {x.shape[1]}] like x (got {tuple(t.shape)})")
    _req(b2, torch.float16, "b2")
    if tuple(b2.shape) != (x.shape[1],):
        raise ValueError(f"b2 must be [{x.shape[1]}] (got {tuple(b2.shape)})")
    if ld_rowbias is None:
        ld_rowbias = x.shape[1]
    if rowbias is not None:
        if rowbias.device.type != "cuda":
            raise _lib.EvoWorldHipError(f"rowbias must live on the GPU (got {rowbias.device}); evoworld_amd has no CPU path")
        if rowbias.dtype != torch.float16:
            raise TypeError(f"rowbias: expected {torch.float16}, got {rowbias.dtype}")
        if rows_per_group < 1:
            raise ValueError(f"rows_per_group must be >= 1 (got {rows_per_group})")
        n_groups = (M + rows_per_group - 1) // rows_per_group
        if rowbias.dim() != 2 or rowbias.shape[1] < x.shape[1] or rowbias.stride(1) != 1 or (rowbias.shape[0] > 1 and rowbias.stride(0) != ld_rowbias):
            raise ValueError(f"rowbias must be [groups, >= {x.shape[1]}] with unit column stride and row stride ld_rowbias = {ld_rowbias} "
                             f"(got shape {tuple(rowbias.shape)}, strides {tuple(rowbias.stride())})")
        if rowbias.shape[0] < n_groups:
            raise ValueError(f"rowbias has {rowbias.shape[0]} rows; {M} rows in groups of {rows_per_group} need {n_groups}")
    a.x, a.w1p, a.b1p, a.w2p, a.b2, a.rowbias = _ptr(x), _ptr(w1p), _ptr(b1p), _ptr(w2p), _ptr(b2), _ptr(rowbias)
    a.r1, a.r1_lo, a.r2, a.r2_lo, a.out, a.out_lo = _ptr(r1h), _ptr(r1l), _ptr(r2h), _ptr(r2l), _ptr(oh), _ptr(ol)
    a.zero_page = _ptr(zero_page(x.device))
    a.M, a.C, a.hidden = x.shape[0], x.shape[1], w2p.shape[0] * 32
    a.rows_per_group = rows_per_group
    a.ld_rowbias = ld_rowbias
    a.c_acc, a.c_r1, a.c_r2 = c_acc, c_r1, c_r2
    _call("ew_ff_geglu320_f16", ctypes.byref(a))
    return out


def pack_conv_weight(w, cpad=None):
    """[O, I, *taps] (Conv2d 3x3 / Conv3d (3,1,1)) fp32 -> fp16 [O, K] in the K order ew_gemm_f16's conv modes read:
    [I/64 chunks][taps][64 channels].  `cpad` zero-pads the input channels first (conv_in: 18 -> 64)."""
    O, I = w.shape[0], w.shape[1]
    wt = w.reshape(O, I, -1).permute(0, 2, 1)                       # [O, taps, I]
    if cpad:
        wt = torch.nn.functional.pad(wt, (0, cpad - I))
        I = cpad
    taps = wt.shape[1]
    wt = wt.reshape(O, taps, I // 64, 64).permute(0, 2, 1, 3)       # [O, chunks, taps, 64]
    return wt.reshape(O, -1).to(torch.float16).contiguous()


# 3x3 conv over a nearest-x2 upsampled image: for output parity a (0 / 1) along one axis, the kernel rows (columns) k that read source pixel
# i + a - 1 + r, r = 0 / 1:  upsampled row 2i + a + k - 1 -> source row (2i + a + k - 1) >> 1
CONVUP2_TAPS = (((0,), (1, 2)), ((0, 1), (2,)))


def convup2_ok(N, C):
    """ew_gemm_f16 runs a 3x3 conv with N output / C input channels as upsample=2 (four 2x2 phase convs, pack_convup2_weight)"""
    return bool(_lib.load().ew_gemm_convup2_ok(int(N), int(C)))


def pack_convup2_weight(w, dtype=torch.float16):
    """[O, I, 3, 3] -> [4 * O, 4 * I]: the weights of ew_gemm_f16's upsample=2 form, [phase 2a+b][O][I/64 chunks][tap 2r+c][64 channels].
    The taps of the 3x3 kernel that read the same source pixel for output parity (a, b) are summed in w's dtype (fp32 from a checkpoint) and
    rounded to `dtype` once."""
    O, I = w.shape[0], w.shape[1]
    if tuple(w.shape[2:]) != (3, 3) or I % 64:
        raise ValueError(f"pack_convup2_weight: expected [O, I % 64 == 0, 3, 3], got {tuple(w.shape)}")
    ph = w.new_zeros(2, 2, O, 2, 2, I)                               # [a, b, O, r, c, I]
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for c in range(2):
                    for ky in CONVUP2_TAPS[a][r]:
                        for kx in CONVUP2_TAPS[b][c]:
                            ph[a, b, :, r, c] += w[:, :, ky, kx]
    ph = ph.reshape(4, O, 4, I // 64, 64).permute(0, 1, 3, 2, 4)     # [phase, O, chunks, taps, 64]
    return ph.reshape(4 * O, 4 * I).to(dtype).contiguous()
