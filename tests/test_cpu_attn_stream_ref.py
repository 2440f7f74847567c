"""The streaming formulation of temporal attention (tests/attn_stream_ref.py: 32-key blocks, fp16 P, rounded-sum normaliser, fp32
accumulators) against fp64 SDPA on the same fp16 inputs, at the op's bound of 2e-3: the shapes and spike patterns of
tests/test_gpu_attn_temporal_long.py, runnable without a GPU.  It pins DESIGN.md's statement that streaming costs no accuracy."""
import pytest
import torch
import torch.nn.functional as F

from attn_cases import spike_case
from attn_stream_ref import attn_stream
from kernel_checks import rel_l2, worst_row


def _sdpa64(q, k, v):
    # [B,T,S,h,64] -> [B,S,h,T,64]
    p = lambda x: x.double().permute(0, 2, 3, 1, 4)
    return F.scaled_dot_product_attention(p(q), p(k), p(v)), attn_stream(*(x.permute(0, 2, 3, 1, 4) for x in (q, k, v)))


@pytest.mark.parametrize("B,T,S,heads", [(1, 65, 7, 1), (2, 96, 5, 3), (1, 97, 21, 2), (1, 128, 3, 1), (1, 129, 5, 1), (1, 200, 9, 1),
                                         (2, 70, 130, 3)])
def test_stream_ref_random(B, T, S, heads):
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, T, S, heads, 64, generator=g).half() for _ in range(3))
    ref, got = _sdpa64(q, k, v)
    e = rel_l2(got, ref)
    w, _ = worst_row(got.reshape(-1, 64), ref.reshape(-1, 64))
    print(f"stream ref {B}x{T}x{S}x{heads}: rel-L2 {e:.2e} worst row {w:.2e}")
    assert e < 2e-3 and w < 1e-3


@pytest.mark.parametrize("pattern", ["first", "last", "rising"])
def test_stream_ref_spikes(pattern):
    ref, got = _sdpa64(*spike_case(pattern))
    assert torch.isfinite(got).all()
    e = rel_l2(got, ref)
    print(f"stream ref spike {pattern}: rel-L2 {e:.2e}")
    assert e < 2e-3
