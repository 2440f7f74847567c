"""The shell the packed models share (unet.py, vae.py, clip.py): parameter spec builder, checkpoint / config loading, state-dict validation,
the weight fetcher of the pack routines and the two conv launches.  A model provides DEFAULTS, WEIGHT_FILES, MISSING, `_spec`, `_random`,
a `_pack(sd)` that sets `self.w`, and its forward ("The model shell")."""
import json
import math
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import ops
from .ops import A_CONV3X3, A_CONVT3


class Spec(OrderedDict):
    """name -> (shape, kind) in module-registration order (the checkpoint's key names).  kind: the fan-in (int) of a weight or bias -- what the
    random generators scale by -- or "gamma" / "beta" (norm scale / shift) / "mix" (AlphaBlender factor)."""

    def add(self, name, shape, kind):
        self[name] = (tuple(shape), kind)

    def conv(self, p, o, i, k):
        self.add(p + ".weight", (o, i) + k, i * math.prod(k))
        self.add(p + ".bias", (o,), i * math.prod(k))

    def lin(self, p, o, i, bias=True):
        self.add(p + ".weight", (o, i), i)
        if bias:
            self.add(p + ".bias", (o,), i)

    def norm(self, p, c):
        self.add(p + ".weight", (c,), "gamma")
        self.add(p + ".bias", (c,), "beta")


class Weights:
    """Fetcher of one pack routine: state-dict entries as fp32 on the device (`f32`), fp16 packing (`h`), and the two idioms on top."""

    def __init__(self, sd, device):
        self.sd, self.device = sd, device

    def f32(self, k):
        return self.sd[k].to(device=self.device, dtype=torch.float32)

    @staticmethod
    def h(t):
        return t.to(torch.float16).contiguous()

    def pair(self, p):
        return self.h(self.f32(p + ".weight")), self.h(self.f32(p + ".bias"))

    def conv(self, p, cpad=None):
        """[O, I, 3, 3] or [O, I, 3, 1, 1] -> ([O, K] in ew_gemm_f16's conv order, K = [I/64][taps][64], bias)"""
        return ops.pack_conv_weight(self.f32(p + ".weight"), cpad), self.h(self.f32(p + ".bias"))

    def conv_up(self, p):
        """the conv of a nearest-x2 upsampler -> (w, bias, upsample): the four-phase pack [4 O, 4 I] with upsample = 2 where ew_gemm_f16 runs that
        form for these channel counts (ops.convup2_ok), the nine taps with upsample = 1 otherwise.  One form per layer."""
        w = self.f32(p + ".weight")
        if ops.convup2_ok(w.shape[0], w.shape[1]):
            return ops.pack_convup2_weight(w), self.h(self.f32(p + ".bias")), 2
        return self.conv(p) + (1,)


class PackedModel:
    DEFAULTS = {}           # config keys and their defaults: what config.json is filtered by
    WEIGHT_FILES = ()       # safetensors names tried in order; the first is also named (with a *) when none exists
    MISSING = "state dict is missing"
    _spec = _random = None  # staticmethod(cfg -> Spec), staticmethod((cfg, seed) -> state dict)
    PRETRAINED_KW = ()      # from_pretrained keywords that are config keys (None = not given); every other keyword is ignored

    def __init__(self, cfg, dtype):
        self._cfg = cfg
        self.config = SimpleNamespace(**cfg)
        self.dtype = dtype
        self.device, self.w = None, None

    # ---------------- construction / loading ----------------
    @classmethod
    def _config_from_json(cls, raw):
        return {k: raw[k] for k in cls.DEFAULTS if k in raw}

    @classmethod
    def read_config(cls, root):
        """The constructor keywords <root>/config.json holds ({} without the file)."""
        cj = os.path.join(root, "config.json")
        if not os.path.exists(cj):
            return {}
        with open(cj) as f:
            return cls._config_from_json(json.load(f))

    @classmethod
    def from_pretrained(cls, path, subfolder=None, device="cuda", **kw):
        """diffusers / transformers folder layout: <path>/<subfolder>/config.json + one of WEIGHT_FILES."""
        root = os.path.join(path, subfolder) if subfolder else path
        cfg = cls.read_config(root)
        cfg.update({k: kw[k] for k in cls.PRETRAINED_KW if kw.get(k) is not None})
        m = cls(**cfg)
        from safetensors.torch import load_file
        for fn in cls.WEIGHT_FILES:
            f = os.path.join(root, fn)
            if os.path.exists(f):
                return m.load_state_dict(load_file(f), device=device)
        raise FileNotFoundError(f"no {cls.WEIGHT_FILES[0].replace('.', '*.', 1)} under {root}")

    @classmethod
    def from_random(cls, seed=0, device="cuda", **config):
        m = cls(**config)
        return m.load_state_dict(cls._random(m._cfg, seed), device=device)

    def load_state_dict(self, sd, device="cuda"):
        spec = self._spec(self._cfg)
        missing = [k for k in spec if k not in sd]
        if missing:
            raise KeyError(f"{self.MISSING} {len(missing)} keys, e.g. {missing[:3]}")
        for k, (shape, _) in spec.items():
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"{k}: expected shape {shape}, got {tuple(sd[k].shape)}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"evoworld_amd.{type(self).__name__} needs a GPU device (no CPU path)")
        self._pack(sd)
        return self

    def _require_loaded(self):
        if self.w is None:
            raise RuntimeError("weights not loaded")

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def requires_grad_(self, _flag=False):
        return self

    # ---------------- the conv launches (activations: fp16 [N*H*W, C]; the output is the model's `_res` when res_out) ----------------
    def _conv3x3(self, x, w, b, N, H, W_, Ho, Wo, stride=1, upsample=0, res_out=False, x2=None, c2=None, **kw):
        """x2: second source of a channel concat; c2: its channels when they are fewer than its row width (x2 = the [x_hi | x_lo] rows read
        again for x_hi).  conv_shift=1 (kw): the (0, 1) padding of a stride-2 Downsample2D(padding=0)."""
        c1 = x.shape[-1]
        lda2 = x2.shape[-1] if x2 is not None else 0
        M = N * Ho * Wo
        n_out = w.shape[0] // 4 if upsample == 2 else w.shape[0]      # upsample=2: w is the four-phase pack (Weights.conv_up)
        out = self._res(M, n_out, x.device, head="r1" not in kw) if res_out else torch.empty(M, n_out, dtype=torch.float16, device=x.device)
        return ops.gemm(x, w, out, M=M, N=n_out, c1=c1, lda=c1, a2=x2, c2=lda2 if c2 is None else c2, lda2=lda2, bias=b,
                        mode=A_CONV3X3, conv=(N, H, W_, Ho, Wo, stride, upsample), **kw)

    def _convt(self, x, w, b, B, T, P, res_out=False, **kw):
        C = x.shape[-1]
        M = B * T * P
        out = self._res(M, w.shape[0], x.device) if res_out else torch.empty(M, w.shape[0], dtype=torch.float16, device=x.device)
        return ops.gemm(x, w, out, M=M, N=w.shape[0], c1=C, lda=C, bias=b, mode=A_CONVT3, tconv=(B, T, P), **kw)
