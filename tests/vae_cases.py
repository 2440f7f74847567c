"""Inputs and references for the VAE mid-block attention at production width (C = 512), shared by test_cpu_vae_cases.py and
test_gpu_vae_production.py (a plain module, imported like gemm_cases.py; needs no GPU to import).

- attention_recipe: seeded weights for one oracle.vae_ref.Attention(512), every value fp16-representable.  to_q / to_k are
  1.5 * randn / sqrt(C), so that unit-variance tokens give scores of standard deviation ~2.3: a 9216-key softmax row then has its
  mass on a few hundred keys and 4/5 of its entries below 6.1e-5, the fp16 denormal range.  All four biases are 0.3 * randn:
  the product drops the key bias and folds the value bias into the out-projection bias, so both must be non-zero to matter.
- attention_input: N different frames of S tokens, [N * S, C] fp32.
- branch64: the attention BRANCH, Attention(x) - x, per frame in fp64 -- exact, or (emulate=True) with a rounding to fp16
  at every point where vae._attention stores fp16: the GroupNorm output, q, k (without its bias, as the product computes it),
  V^T (without its bias), P and P V.  The scores stay unrounded: the product carries them as hi + lo8 into an fp32 softmax.  The
  folded bias W_o b_v + b_o is added exactly.
  The residual `+ x` is left out on purpose: it is as large as the branch and exact, and would halve every relative error."""
import math

import torch

C_ATTN = 512
GROUPS = 32
GN_EPS = 1e-6
PREFIX = "decoder.mid_block.attentions.0."


def attention_recipe(C=C_ATTN, seed=0):
    """state dict of oracle.vae_ref.Attention(C) (fp32 tensors holding fp16-representable values)"""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    sd = {"group_norm.weight": 1.0 + 0.1 * r(C), "group_norm.bias": 0.1 * r(C)}
    for name, gain in (("to_q", 1.5), ("to_k", 1.5), ("to_v", 1.0), ("to_out.0", 1.0)):
        sd[name + ".weight"] = gain * r(C, C) / math.sqrt(C)
        sd[name + ".bias"] = 0.3 * r(C)
    return {k: v.half().float() for k, v in sd.items()}


def attention_input(N, S, C=C_ATTN, seed=0):
    """[N * S, C] fp32 tokens (channels last, frame-major): unit-scale, every frame different"""
    return torch.randn(N * S, C, generator=torch.Generator().manual_seed(2000 + seed))


def split_input(x):
    """x as the residual stream holds it: (Res of x, its decoded fp32 value -- what every reference here starts from)"""
    from evoworld_amd.ops import Res
    r = Res.from_float(x)
    return r, r.float()


def _f16(t):
    return t.half().double()


def group_norm64(x, gamma, beta):
    """GroupNorm(32, C, eps 1e-6) of one frame x [S, C] in fp64"""
    S, C = x.shape
    g = x.reshape(S, GROUPS, C // GROUPS)
    mean = g.mean(dim=(0, 2), keepdim=True)
    var = g.var(dim=(0, 2), unbiased=False, keepdim=True)
    return ((g - mean) / torch.sqrt(var + GN_EPS)).reshape(S, C) * gamma + beta


def branch64(sd, x, N, emulate=False, key_bias=True, device="cpu"):
    """x [N * S, C] (any float dtype) -> (branch [N * S, C] fp64 on `device`, standard deviation of the scaled scores).
    emulate: fp16 storage points of vae._attention (module docstring); key_bias=False: the same with to_k.bias = 0."""
    w = {k: v.double().to(device) for k, v in sd.items()}
    C = w["to_q.weight"].shape[0]
    xs = x.double().to(device).reshape(N, -1, C)
    q16 = _f16 if emulate else (lambda t: t)
    out, var = [], []
    for xf in xs:
        h = q16(group_norm64(xf, w["group_norm.weight"], w["group_norm.bias"]))
        q = q16(h @ w["to_q.weight"].T + w["to_q.bias"])
        if emulate:
            k = q16(h @ w["to_k.weight"].T)                              # the key bias is dropped
            v = q16((w["to_v.weight"] @ h.T)).T                          # V^T = W_v X^T, the value bias is folded
            fold = w["to_out.0.weight"] @ w["to_v.bias"] + w["to_out.0.bias"]
        else:
            k = h @ w["to_k.weight"].T + (w["to_k.bias"] if key_bias else 0.0)
            v = h @ w["to_v.weight"].T + w["to_v.bias"]
            fold = w["to_out.0.bias"]
        s = q @ k.T / math.sqrt(C)
        var.append(float(s.var(unbiased=False)))
        p = q16(torch.softmax(s, dim=-1))
        del s
        o = q16(p @ v)
        del p
        out.append(o @ w["to_out.0.weight"].T + fold)
    return torch.cat(out), math.sqrt(sum(var) / len(var))


def softmax_rows_f16(S, cols, seed=0, scale=2.3, device="cpu"):
    """fp16 softmax(scale * randn) rows [S, cols], generated on `device`: the A operand of P V"""
    s = scale * torch.randn(S, cols, generator=torch.Generator(device).manual_seed(3000 + seed), device=device, dtype=torch.float64)
    return torch.softmax(s, dim=-1).half()


def denormal_fraction(p):
    """fraction of the entries of fp16 tensor p that are non-zero denormals (0 < |p| < 2^-14)"""
    a = p.abs()
    return float(((a > 0) & (a < 2.0 ** -14)).double().mean())
