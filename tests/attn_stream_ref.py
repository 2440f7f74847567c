"""Torch restatement of the key-streaming temporal attention (attn_temporal_long_kernel, T > 64) -- a plain module, imported like
kernel_checks.  It states the kernel's NUMERICS, not its layout: fp16 q / k / v, fp32 scores, keys in blocks of 32 with a running maximum m,
P = exp2((s - m) * scale * log2 e) rounded to fp16, the normaliser l summing the same rounded values, fp32 accumulators for l and O, both
multiplied by alpha = exp2((m_old - m_new) * scale * log2 e) in every block, one division and one rounding to fp16 at the end.
tests/test_cpu_attn_stream_ref.py holds it against fp64 SDPA (the forced-rescale inputs, spike_case, live in tests/attn_cases.py)."""
import math

import torch

LOG2E = 1.4426950408889634


def attn_stream(q, k, v, scale=0.125, block=32):
    """q, k, v: fp16 [..., T, 64] -> fp16 [..., T, 64]"""
    T = q.shape[-2]
    c = torch.tensor(scale * LOG2E, dtype=torch.float32)
    qf, kf, vf = q.float(), k.float(), v.float()
    m = torch.full(q.shape[:-1], -math.inf, dtype=torch.float32)
    l = torch.zeros(q.shape[:-1], dtype=torch.float32)
    acc = torch.zeros(q.shape, dtype=torch.float32)
    for k0 in range(0, T, block):
        s = qf @ kf[..., k0:k0 + block, :].transpose(-1, -2)                    # keys >= T simply do not exist here
        m_new = torch.maximum(m, s.amax(dim=-1))
        alpha = torch.exp2((m - m_new) * c)
        p = torch.exp2(s * c - (m_new * c)[..., None]).half()
        l = l * alpha + p.float().sum(dim=-1)
        acc = acc * alpha[..., None] + p.float() @ vf[..., k0:k0 + block, :]
        m = m_new
    return (acc / l[..., None]).half()

