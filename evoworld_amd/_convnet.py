"""The shell of the metric networks (lpips.LPIPSAlex, fvd.I3D, latent_mse.InceptionV4): what a convolutional network on ops.gemm needs
besides its layer table -- reading and validating a state dict, folding BatchNorm, packing a convolution's weight as the patch gathers
order their columns, seeded random weights, the constructors, and the "one GEMM per (unit, piece) into a slice of the concat" loop.

This is not _model.PackedModel: that one needs a CUDA device and a config.json, while everything here up to ConvNet.conv_into runs on
the CPU (packing is tested without a GPU) and the weights are a bare state dict the user supplies.
"""
import math

import torch

K_ALIGN = 64                                           # ew_gemm_f16 takes K in multiples of 64


def load_state_files(paths):
    """One or more weight files (.safetensors, or anything torch.load(..., weights_only=True) reads) merged into one state dict."""
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    sd = {}
    for p in paths:
        if str(p).endswith(".safetensors"):
            from safetensors.torch import load_file
            part = load_file(str(p))
        else:
            part = torch.load(p, map_location="cpu", weights_only=True)
            if isinstance(part, dict) and "state_dict" in part and isinstance(part["state_dict"], dict):
                part = part["state_dict"]
        sd.update(part)
    return sd


def validate(sd, spec, what, accepted=None):
    """State dict -> {key: fp32 CPU tensor} over exactly the keys of `spec` ({key: shape}).  A leading `module.` is stripped, keys outside
    the spec are ignored.  KeyError gives the count and the first three missing keys (and `accepted`, a sentence on what is taken);
    ValueError names the key of the wrong shape."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    missing = [k for k in spec if k not in sd]
    if missing:
        raise KeyError(f"{what} state dict is missing {len(missing)} keys, e.g. {missing[:3]}" + (f"; expected {accepted}" if accepted else ""))
    for k, shape in spec.items():
        if tuple(sd[k].shape) != tuple(shape):
            raise ValueError(f"{k}: expected shape {tuple(shape)}, got {tuple(sd[k].shape)}")
    return {k: sd[k].detach().to("cpu", torch.float32) for k in spec}


def fold_batchnorm(c, name, conv_key, eps):
    """(weight [C_out, C_in, *k], bias [C_out]) in fp64 of unit `name` with its eval-mode BatchNorm folded in: s = gamma / sqrt(var + eps);
    w * s; beta - mean * s.  Reads {name}.{conv_key}.weight and {name}.bn.{weight,bias,running_mean,running_var}."""
    s = c[f"{name}.bn.weight"].double() / (c[f"{name}.bn.running_var"].double() + eps).sqrt()
    w = c[f"{name}.{conv_key}.weight"].double()
    return w * s.view(-1, *([1] * (w.ndim - 1))), c[f"{name}.bn.bias"].double() - c[f"{name}.bn.running_mean"].double() * s


def pack_conv(w, cpad=None):
    """[C_out, C_in, *k] (fp64 or fp32) -> fp16 [C_out, K padded to 64] with K ordered (taps, c_in padded with zeros to `cpad`), as
    ops.im2col3d (cpad = c_in rounded up to 8) and ops.im2col_frames (cpad None: the 3 channels as they are) write their columns."""
    co, ci, taps = w.shape[0], w.shape[1], tuple(w.shape[2:])
    cp = ci if cpad is None else int(cpad)
    if cp < ci:
        raise ValueError(f"pack_conv: cpad = {cp} is less than the {ci} input channels")
    K = math.prod(taps) * cp
    rows = torch.zeros(co, *taps, cp, dtype=w.dtype)
    rows[..., :ci] = w.permute(0, *range(2, w.ndim), 1)
    wk = torch.zeros(co, -(-K // K_ALIGN) * K_ALIGN, dtype=torch.float16)
    wk[:, :K] = rows.reshape(co, K).half()
    return wk


def random_conv_bn(g, sd, name, conv_key, shape):
    """Adds one seeded conv + BatchNorm unit to `sd`, drawn in this order: conv weight [C_out, C_in, *k] ~ N(0, 2 / fan-in), gamma uniform
    in [0.8, 1.2], beta and running mean N(0, 0.1^2), running variance uniform in [0.7, 1.3].  Activations stay O(1)."""
    co = shape[0]
    sd[f"{name}.{conv_key}.weight"] = torch.randn(*shape, generator=g) * (2.0 / math.prod(shape[1:])) ** 0.5
    sd[f"{name}.bn.weight"] = 0.8 + 0.4 * torch.rand(co, generator=g)
    sd[f"{name}.bn.bias"] = 0.1 * torch.randn(co, generator=g)
    sd[f"{name}.bn.running_mean"] = 0.1 * torch.randn(co, generator=g)
    sd[f"{name}.bn.running_var"] = 0.7 + 0.6 * torch.rand(co, generator=g)


class ConvNet:
    """A metric network on the device: self.p holds pack_state_dict's tensors.  A subclass names its module's pack_state_dict,
    load_state_files and random_state_dict (as staticmethods) and takes its own keywords after (packed, device)."""

    def __init__(self, packed, device):
        self.device = torch.device(device)
        self.p = {k: v.to(self.device) if isinstance(v, torch.Tensor) else v for k, v in packed.items()}

    @classmethod
    def from_state_dict(cls, sd, device="cuda", *args, **kw):
        return cls(cls.pack_state_dict(sd), device, *args, **kw)

    @classmethod
    def from_files(cls, paths, device="cuda", *args, **kw):
        return cls.from_state_dict(cls.load_state_files(paths), device, *args, **kw)

    @classmethod
    def from_random(cls, seed=0, device="cuda", *args, **kw):
        """The network's shapes with seeded random weights (timing and tests; the values mean nothing)"""
        return cls.from_state_dict(cls.random_state_dict(seed), device, *args, **kw)

    @staticmethod
    def check_channel_order(channel_order):
        """'rgb' / 'bgr' -> whether network channel c reads frame channel 2 - c"""
        if channel_order not in ("rgb", "bgr"):
            raise ValueError(f"channel_order {channel_order!r}: expected 'rgb' or 'bgr'")
        return channel_order == "bgr"

    @staticmethod
    def frames_hw(frames, name="frames", n="F"):
        """(H, W) of uint8 [n,H,W,3] or fp32 [n,3,H,W] frames"""
        if frames.ndim != 4 or frames.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"{name}: expected uint8 [{n},H,W,3] or fp32 [{n},3,H,W], got {frames.dtype} {tuple(frames.shape)}")
        return (frames.shape[1], frames.shape[2]) if frames.dtype == torch.uint8 else (frames.shape[2], frames.shape[3])

    @staticmethod
    def conv_into(rows, targets):
        """rows fp16 [pieces, m, ldk] patch rows; per target (w [N, ldk], b [N], out [pieces * m pixels, ld channels] in any leading shape,
        channel offset): out[piece, :, offset : offset + N] = rows[piece] @ w^T + b, one GEMM per (target, piece).  A piece is what must not
        depend on its neighbours: one image (LPIPS, Inception-v4) or one slab of output frames (I3D)."""
        from . import ops
        pieces, m, ldk = rows.shape
        for w, b, out, c_off in targets:
            ld = out.shape[-1]
            o = out.view(pieces, m, ld)
            for j in range(pieces):
                ops.gemm(rows[j], w, o[j, :, c_off:], M=m, N=w.shape[0], c1=ldk, lda=ldk, bias=b, ld_out=ld)
