"""-m gpu: the temporal VAE at the widths users run (block_out_channels (128, 256, 512, 512), two layers per block), which
test_gpu_vae.py's tiny config never reaches.

1. The mid-block attention as a unit at C = 512 (vae._attention on the recipe of tests/vae_cases.py): the BRANCH, out - x, per frame
   and per row against the fp64 reference -- not the whole image, where the residual hides it.  Bounds come from the reference's own
   fp16-storage emulation (vae_cases.branch64(emulate=True)), never from the product: worst row <= 2 x the emulation's worst row of
   the case, rel-L2 <= 2 x the emulation's and <= 2e-3.  The 2 x covers what the emulation cannot see: MFMA fp32 summation order,
   __expf, the lo8 step of the split streams, the fp16 rounding of the folded bias.  The recipe's key and value biases are non-zero,
   so a wrong fold shows; with N > 1 the frames differ, so a stale per-frame buffer (scores / p / vt) or a wrong frame slice shows as
   one frame failing.  At S = 9216 the kernel of every ew_gemm_f16 launch is recorded: scores and P V must run the gemm3b variants
   and schedules gemm_cases.gen3_plan predicts (<0, 17> whole tiles in bands, <0, 0> on the half split).
   The measured figures stand beside ATTN_CASES below.
2. The production config end to end on small frames against the fp32 oracle: shapes, determinism, the module's stated 3e-3, and
   a bound from the oracle itself (test_production_*)."""
import pytest
import torch

from gemm_cases import gen3_plan
from kernel_checks import rel_l2, report, worst_row
from vae_cases import C_ATTN, PREFIX, attention_input, attention_recipe, branch64

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (frames, H, W) of the attention cases.  Measured on an MI355X, branch against fp64 (rel-L2 / worst row):
#   case          emulation (the bounds are 2 x these)    product
#   3 x  8 x   8  5.308e-4 / 1.076e-3                     5.483e-4 / 1.090e-3   (frames 5.08e-4, 5.77e-4, 5.57e-4)
#   2 x 24 x  24  4.634e-4 / 1.423e-3                     4.880e-4 / 1.428e-3   (frames 4.88e-4, 4.88e-4)
#   1 x 72 x 128  2.607e-4 / 1.218e-3                     3.205e-4 / 1.219e-3
# The test computes the emulation again and takes its bounds from what it computes.
ATTN_CASES = [(3, 8, 8), (2, 24, 24), (1, 72, 128)]


@pytest.fixture(scope="module")
def lib():
    from evoworld_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def attn_vae():
    """a VAE whose mid blocks are 512 wide and whose other blocks are small, with the recipe as its decoder attention"""
    from evoworld_amd.vae import DEFAULT_VAE_CONFIG, AutoencoderKLTemporalDecoder, random_vae_state_dict
    cfg = dict(block_out_channels=(128, C_ATTN), layers_per_block=1)
    sd = {k: v.half().float() for k, v in random_vae_state_dict({**DEFAULT_VAE_CONFIG, **cfg}, 0).items()}
    recipe = attention_recipe()
    for k, v in recipe.items():
        assert sd[PREFIX + k].shape == v.shape, k
        sd[PREFIX + k] = v
    return AutoencoderKLTemporalDecoder(**cfg).load_state_dict(sd, device=DEV), recipe


class GemmLog:
    """records (M, N, K, kernel name) of every ew_gemm_f16 call through a wrapper set on the library object"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __enter__(self):
        self.orig = self.lib.ew_gemm_f16

        def recording(*args):
            g = args[0]._obj                                              # the struct is only alive during the call
            dims = (g.M, g.N, g.c1 + g.c2 if g.mode == 0 else None)
            st = self.orig(*args)
            self.calls.append(dims + (self.lib.ew_gemm_last_kernel().decode(),))
            return st
        self.lib.ew_gemm_f16 = recording
        return self

    def __exit__(self, *exc):
        self.lib.ew_gemm_f16 = self.orig

    def names(self):
        return {c[3].split("<")[0] for c in self.calls}


@pytest.mark.parametrize("N,H,W", ATTN_CASES)
def test_attention_branch_vs_fp64(lib, attn_vae, N, H, W):
    from evoworld_amd import ops
    vae, recipe = attn_vae
    S, C = H * W, C_ATTN
    xr = ops.Res.from_float(attention_input(N, S).to(DEV))
    x = xr.float()                                                        # the decoded split input: what the product reads
    exact, std = branch64(recipe, x, N, device=DEV)
    emul, _ = branch64(recipe, x, N, emulate=True, device=DEV)
    e_rel, (e_worst, e_row) = rel_l2(emul, exact), worst_row(emul, exact)
    rms_b, rms_x = float(exact.square().mean().sqrt()), float(x.double().square().mean().sqrt())
    print(f"attention {N}x{H}x{W}: score std {std:.2f}, branch RMS {rms_b:.3f} (input {rms_x:.3f}); "
          f"emulation vs fp64: rel-L2 {e_rel:.3e} worst row {e_worst:.3e} @ {e_row}")
    assert 1.5 < std < 3.5 and 0.25 * rms_x < rms_b < 2.0 * rms_x         # the conditions of test_cpu_vae_cases.py, on this input
    assert 1e-5 < e_rel < 3e-3 and e_worst < 3e-3
    bound_rel, bound_worst = min(2.0 * e_rel, 2e-3), 2.0 * e_worst
    vae._begin(torch.device(DEV))
    with GemmLog(lib) as log:
        out = vae._attention(vae.w["d_mid"][1], xr, N, H, W)
        torch.cuda.synchronize()
    assert log.lib.ew_gemm_f16 is log.orig
    ops.streamk_check()
    branch = (out.float().double() - x.double()).reshape(N, S, C)
    failed = []
    for f in range(N):                                                    # every figure is printed before the test fails
        try:
            report(f"vae attention {N}x{H}x{W} frame {f}", branch[f], exact.reshape(N, S, C)[f], bound_worst, bound_rel)
        except AssertionError as e:
            failed.append(str(e))
    e_all = rel_l2(branch, exact.reshape(N, S, C))
    print(f"attention {N}x{H}x{W}: product vs fp64 rel-L2 {e_all:.3e} (bound {bound_rel:.3e} = 2 x emulation {e_rel:.3e}, at most 2e-3)")
    assert not failed, "\n".join(failed)
    assert e_all <= bound_rel
    # the launches: q, k, then per frame V^T, scores, P V, then the out projection
    G = lib.ew_get_cu_budget()
    dims = [c[:3] for c in log.calls]
    assert dims == [(N * S, C, C)] * 2 + [(C, S, C), (S, S, C), (S, C, S)] * N + [(N * S, C, C)], dims
    p_scores, p_pv = gen3_plan(S, S, C, "dense", {"lo"}, G), gen3_plan(S, C, S, "dense", set(), G)
    p_vt = gen3_plan(C, S, C, "dense", set(), G)
    for f in range(N):
        vt, sc, pv = (c[3] for c in log.calls[2 + 3 * f: 5 + 3 * f])
        for name, plan in ((vt, p_vt), (sc, p_scores), (pv, p_pv)):
            assert (name == plan.kernel) if plan.taken else name.startswith("gemm2_kernel"), (f, name, plan.kernel, plan.taken)
    if S == 9216:                                                         # production: the routes of the issue's table
        assert G == 256
        assert (p_scores.taken, p_scores.kernel, p_scores.schedule, p_scores.band, p_scores.tiles) == (True, "gemm3b_kernel<0, 17>", "whole", 4, 1296)
        assert sorted({len(it) for it in p_scores.items}) == [5, 6]
        assert (p_pv.taken, p_pv.kernel, p_pv.schedule, p_pv.grid) == (True, "gemm3b_kernel<0, 0>", "half", 144)
        assert not p_vt.taken and log.calls[2][3].startswith("gemm2_kernel")
        assert [c[3] for c in log.calls[3:5]] == ["gemm3b_kernel<0, 17>", "gemm3b_kernel<0, 0>"]


def test_attention_rejects_token_counts_that_are_no_multiple_of_64(attn_vae):
    from evoworld_amd import ops
    vae, _ = attn_vae
    vae._begin(torch.device(DEV))
    x = ops.Res.from_float(attention_input(1, 60).to(DEV))
    with pytest.raises(ValueError, match="multiple of 64"):
        vae._attention(vae.w["d_mid"][1], x, 1, 6, 10)


# ----------------------------------------------------------------------------- the production config end to end
def _round_outputs_to_fp16(ref):
    """forward hooks that round the output of every Conv2d, Conv3d, Linear and GroupNorm of the oracle to fp16: the storage points
    of the product that a module boundary can see (the pattern of fp8_ref.fake_quant_unet).  Returns the handles."""
    import torch.nn as nn
    hook = lambda mod, args, out: out.half().float()
    return [m.register_forward_hook(hook) for m in ref.modules() if isinstance(m, (nn.Conv2d, nn.Conv3d, nn.Linear, nn.GroupNorm))]


@pytest.fixture(scope="module")
def production():
    from evoworld_amd.vae import DEFAULT_VAE_CONFIG, AutoencoderKLTemporalDecoder, random_vae_state_dict
    from oracle.vae_ref import AutoencoderKLTemporalDecoderRef
    sd = {k: v.half().float() for k, v in random_vae_state_dict(DEFAULT_VAE_CONFIG, 0).items()}
    ref = AutoencoderKLTemporalDecoderRef().eval()
    ref.load_state_dict(sd, strict=True)
    vae = AutoencoderKLTemporalDecoder(**DEFAULT_VAE_CONFIG).load_state_dict(sd, device=DEV)
    return ref, vae


def _oracle_pair(ref, fn):
    """fn(ref) on the plain oracle and on the oracle with fp16-rounded module outputs -> (plain, E_emul = rel-L2 between them)"""
    want = fn(ref)
    handles = _round_outputs_to_fp16(ref)
    try:
        hooked = fn(ref)
    finally:
        for h in handles:
            h.remove()
    return want, rel_l2(hooked, want)


def test_production_encode_vs_oracle(lib, production):
    """2 frames of 64 x 64 -> 8 x 8 latents (S = 64, the smallest the attention accepts), every encoder block at its production width.
    Bound from the oracle itself: E_emul = rel-L2 between the oracle with every Conv2d / Conv3d / Linear / GroupNorm output rounded
    to fp16 and the plain oracle; the product may be off by 2 x E_emul (the 2 for the roundings a module hook cannot see: q / k / P /
    V^T, the SiLU'd norm outputs).  Measured on an MI355X: E_emul 1.581e-3, product 1.267e-3.
    On the MI355X every GEMM of this encode ran on generation 2 (the folded conv_out, 512 -> 4, included)."""
    ref, vae = production
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(7)) * 2 - 1
    want, e_emul = _oracle_pair(ref, lambda r: r.encode_mode(x))
    with GemmLog(lib) as log:
        got = vae.encode(x.to(DEV)).latent_dist.mode()
    assert got.shape == (2, 4, 8, 8)
    e = rel_l2(got.cpu(), want)
    print(f"production VAE encode: rel-L2 {e:.3e}; E_emul {e_emul:.3e} (bound 2 x); kernels {sorted(log.names())}")
    assert torch.equal(got, vae.encode(x.to(DEV)).latent_dist.mode())      # deterministic
    assert e < 3e-3
    assert e <= 2.0 * e_emul
    assert "gemm2_kernel" in log.names() and not any(nm.startswith("gemm_kernel") for nm in log.names()), log.names()


@pytest.mark.parametrize("n,T", [(4, 2), (3, 3)])
def test_production_decode_vs_oracle(lib, production, n, T):
    """8 x 8 latents -> n frames of 64 x 64 in chunks of T frames, every decoder block at its production width.
    Same bounds as the encode test.  Measured on an MI355X: (4, 2): E_emul 1.775e-3, product 1.433e-3; (3, 3): E_emul 1.716e-3,
    product 1.413e-3.
    Routes: these frames reach generation 2 (both tile families: 256x160 for the 128-channel blocks) and conv_small_n_kernel
    (conv_out behind the 128-channel norm).  They do NOT reach gemm3b_kernel: plan3 takes a problem from 200 tiles of 256 rows on
    (51200 rows at N = 256, 25600 at N = 512; here at most 4096 and 1024), which on the fp32 oracle would be frames of 256 x 256
    and half a minute per decode.  gemm3b_kernel on the VAE's schedules is covered by test_attention_branch_vs_fp64 at S = 9216,
    by G12 - G14 of test_gpu_gemm_gen3_rounds.py and by the b256 / half_b256 cases of test_gpu_gemm_gen3.py."""
    ref, vae = production
    z = torch.randn(n, 4, 8, 8, generator=torch.Generator().manual_seed(8))
    want, e_emul = _oracle_pair(ref, lambda r: r.decode(z, T))
    with GemmLog(lib) as log:
        got = vae.decode(z.to(DEV), num_frames=T).sample
    assert got.shape == (n, 3, 64, 64)
    e = rel_l2(got.cpu(), want)
    print(f"production VAE decode n={n} T={T}: rel-L2 {e:.3e}; E_emul {e_emul:.3e} (bound 2 x); kernels {sorted(log.names())}")
    assert torch.equal(got, vae.decode(z.to(DEV), num_frames=T).sample)    # deterministic
    assert e < 3e-3
    assert e <= 2.0 * e_emul
    assert {"gemm2_kernel", "conv_small_n_kernel"} <= log.names(), log.names()
    assert not any(nm.startswith("gemm_kernel") for nm in log.names())      # generation 1 is the tests' comparison kernel only
