"""The conditions tests/test_gpu_vae_production.py relies on, checked on the references of tests/vae_cases.py alone (CPU only):
the recipe's scores are spread enough for the softmax to matter, the attention branch is not noise under the residual, the fp16
storage emulation -- from which the GPU test derives its bounds -- stays close to exact, the key bias really is softmax-invariant,
and the fp64 restatement is the oracle's Attention."""
import pytest
import torch

from kernel_checks import rel_l2, worst_row
from vae_cases import C_ATTN, attention_input, attention_recipe, branch64, denormal_fraction, softmax_rows_f16, split_input

SIZES = [(3, 64), (2, 576)]                 # (frames, tokens) of the two small GPU cases


@pytest.fixture(scope="module")
def recipe():
    return attention_recipe()


def test_recipe_is_fp16_representable_and_has_every_bias(recipe):
    for name, v in recipe.items():
        assert torch.equal(v, v.half().float()), name
    for name in ("to_q", "to_k", "to_v", "to_out.0"):
        assert 0.2 < float(recipe[name + ".bias"].std()) < 0.4, name
    assert 0.9 < float(recipe["group_norm.weight"].mean()) < 1.1


@pytest.mark.parametrize("N,S", SIZES)
def test_reference_conditions(recipe, N, S):
    _, x = split_input(attention_input(N, S))
    exact, std = branch64(recipe, x, N)
    emul, _ = branch64(recipe, x, N, emulate=True)
    rms_b, rms_x = float(exact.square().mean().sqrt()), float(x.double().square().mean().sqrt())
    e, (w, row) = rel_l2(emul, exact), worst_row(emul, exact)
    print(f"S {S}: score std {std:.2f}, branch RMS {rms_b:.3f} (input {rms_x:.3f}), emulation rel-L2 {e:.3e} worst row {w:.3e} @ {row}")
    assert 1.5 < std < 3.5
    assert 0.25 * rms_x < rms_b < 2.0 * rms_x
    assert e < 3e-3 and w < 3e-3
    assert e > 1e-5                          # the emulation does round
    # frames differ: a stale per-frame buffer would show
    b = exact.reshape(N, S, C_ATTN)
    assert all(rel_l2(b[i], b[0]) > 0.5 for i in range(1, N))


@pytest.mark.parametrize("N,S", SIZES)
def test_key_bias_is_softmax_invariant(recipe, N, S):
    _, x = split_input(attention_input(N, S))
    with_bias, _ = branch64(recipe, x, N)
    without, _ = branch64(recipe, x, N, key_bias=False)
    assert rel_l2(without, with_bias) < 1e-12
    # ... and the value bias is not: zeroing it moves the branch
    sd = dict(recipe, **{"to_v.bias": torch.zeros(C_ATTN)})
    assert rel_l2(branch64(sd, x, N)[0], with_bias) > 0.1


def test_reference_is_the_oracle_attention(recipe):
    from oracle.vae_ref import Attention
    N, H, W = 2, 8, 8
    att = Attention(C_ATTN).double().eval()
    att.load_state_dict({k: v.double() for k, v in recipe.items()}, strict=True)
    _, x = split_input(attention_input(N, H * W))
    img = x.double().reshape(N, H, W, C_ATTN).permute(0, 3, 1, 2)
    with torch.no_grad():
        want = (att(img) - img).permute(0, 2, 3, 1).reshape(N * H * W, C_ATTN)
    assert rel_l2(branch64(recipe, x, N)[0], want) < 1e-12


def test_softmax_operand_is_mostly_denormal():
    """the A operand of the half_b256_attn GEMM case: at 9216 keys most of a softmax row is an fp16 denormal (a slice of 64 rows)"""
    p = softmax_rows_f16(64, 9216)
    assert denormal_fraction(p) > 0.5
    assert abs(float(p.double().sum(1).mean()) - 1.0) < 1e-2
