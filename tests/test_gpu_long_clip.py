"""-m gpu: clips of more than 64 frames through the whole path (tiny U-Net, 16x32 latents): one forward and a 4-step clip against the fp32
CPU oracle, and the pipeline's call surface at 97 frames.  Protocol of test_unet_T49_forward_vs_oracle_fp32_weights (test_gpu_config5.py):
random_state_dict(..., 5), fp32 checkpoint kept by the oracle and packed to fp16 by the HIP loader, ehs[0] = 0, t = 0.8.

Bound: the north_star's 1.0e-3, with one provision because the tiny config sits close to it (README: 8.3e-4 ... 9.8e-4 over seeds): each test
also runs its own protocol at T = 49 (the 64-frame kernel: not code under test) and asserts e_T <= max(1.0e-3, 1.25 x e_49); the 25 % covers
the +-8 % seed-to-seed spread the README records with room for the longer softmax."""
import os

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 16, 32


def _models(T):
    from evoworld_amd.unet import DEFAULT_CONFIG, UNetSpatioTemporalConditionModel, random_state_dict
    from oracle.unet_ref import UNetSpatioTemporalConditionModelRef, tiny_config
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg = tiny_config()
    cfg["num_frames"] = T
    sd = random_state_dict({**DEFAULT_CONFIG, **cfg}, 5)
    ref = UNetSpatioTemporalConditionModelRef(**cfg).eval()
    ref.load_state_dict(sd, strict=True)
    return cfg, ref, UNetSpatioTemporalConditionModel(**cfg).load_state_dict(sd, device=DEV)


def _forward_err(T, B):
    cfg, ref, m = _models(T)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, T, 18, H, W, generator=g)
    ehs = torch.randn(B, 1, cfg["cross_attention_dim"], generator=g)
    ehs[0] = 0
    ids = torch.tensor([[6.0, 127.0, 0.02]] * B)
    t = torch.tensor(0.8)
    with torch.no_grad():
        want = ref(x, t, ehs, ids)
    got = m(x.to(DEV), t, ehs.to(DEV), ids.to(DEV), return_dict=False)[0]
    assert torch.isfinite(got).all()
    return rel_l2(got.cpu(), want)


def _clip_err(T, steps=4):
    from evoworld_amd.pipeline import StableVideoDiffusionPipeline
    from oracle.pipeline_ref import oracle_loop
    cfg, ref, unet = _models(T)
    pipe = StableVideoDiffusionPipeline(unet=unet)
    g = torch.Generator().manual_seed(2)
    lat0, il = torch.randn(1, T, 4, H, W, generator=g), torch.randn(1, T + 1, 4, H, W, generator=g)
    ehs, pl = torch.randn(1, 1, cfg["cross_attention_dim"], generator=g), torch.randn(1, T, 6, H, W, generator=g)
    out = pipe(torch.zeros(1, 3, H * 8, W * 8), height=H * 8, width=W * 8, num_frames=T, num_inference_steps=steps, latents=lat0,
               output_type="latent", plucker_embedding=pl, image_latents=il, image_embeddings=ehs).frames
    with torch.no_grad():
        want = oracle_loop(ref, lat0, il, ehs, pl, T, steps)
    assert torch.isfinite(out).all()
    return rel_l2(out.cpu(), want)


@pytest.fixture(scope="module")
def e49_forward():
    return _forward_err(49, 1)


@pytest.mark.parametrize("T,B", [(65, 1), (97, 2)])
def test_unet_long_clip_forward_vs_oracle(e49_forward, T, B):
    """temporal attention on the key-streaming kernel, T-frame GroupNorm slabs, time_pos_embed over T positions"""
    e = _forward_err(T, B)
    print(f"long clip: tiny U-Net forward, T = {T}, B = {B}, 16x32 latents: rel-L2 vs CPU oracle {e:.3e} (T = 49 twin: {e49_forward:.3e})")
    assert e <= max(1.0e-3, 1.25 * e49_forward)


def test_pipeline_two_steps_T97():
    """the pipeline call surface at T = 97 (guidance ramp, time-id, scheduler) on the tiny U-Net"""
    from evoworld_amd.pipeline import StableVideoDiffusionPipeline
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel
    from oracle.unet_ref import tiny_config
    cfg = tiny_config()
    cfg["num_frames"] = 97
    unet = UNetSpatioTemporalConditionModel.from_random(seed=0, device=DEV, **cfg)
    pipe = StableVideoDiffusionPipeline(unet=unet)
    T = 97
    g = torch.Generator().manual_seed(1)
    out = pipe(torch.zeros(1, 3, H * 8, W * 8), height=H * 8, width=W * 8, num_frames=T, num_inference_steps=2,
               latents=torch.randn(1, T, 4, H, W, generator=g), output_type="latent", plucker_embedding=torch.randn(1, T, 6, H, W, generator=g),
               image_latents=torch.randn(1, T + 1, 4, H, W, generator=g),
               image_embeddings=torch.randn(1, 1, cfg["cross_attention_dim"], generator=g)).frames
    assert out.shape == (1, T, 4, H, W) and torch.isfinite(out).all()


def test_pipeline_4_steps_T65_vs_oracle():
    """a 4-step clip of 65 frames against the fp32 oracle loop; the twin is the same loop at T = 49"""
    e49 = _clip_err(49)
    e65 = _clip_err(65)
    print(f"long clip: 4 steps x 65 frames, tiny U-Net: clip rel-L2 vs CPU oracle loop {e65:.3e} (T = 49 twin: {e49:.3e})")
    assert e65 <= max(1.0e-3, 1.25 * e49)
