"""-m gpu: the device MJPEG encoder (csrc/video.hip: ew_jpeg_dct_quant, ew_jpeg_entropy, ew_jpeg_pack through ops.jpeg_* and
evoworld_amd.video) against the float64 oracle tests/jpeg_ref.py on the inputs of tests/video_cases.py, libjpeg (Pillow) as an
independent decoder, and the paths built on it: write_video, Navigator.save_video / save_gif, process_episode(save_video=).

Coefficients: a device coefficient may differ from the oracle's only by exactly 1 and only where the oracle's quotient c / t lies
within 1e-3 of a half-integer (float32 error through two 8-point passes on values <= 1024 is a few 1e-4); the inputs keep such
quotients at or below 0.2 % (oracle-only precondition, tests/test_cpu_video.py::test_near_tie_precondition).
Entropy coder: the device's bytes of every frame equal the oracle packer's bytes for the device's own coefficients.
Decode: Pillow decodes every frame; its PSNR against the source may fall short of the PSNR of Pillow's own encoder (same quality and
sampling) by at most PSNR_SLACK = twice the largest shortfall measured over the images of this file on an MI355X (floor 0.05 dB).
Measured: -0.458 .. +0.029 dB over the cases of video_cases.py, -0.011 .. +0.021 dB over the episode frames and -0.166 .. +0.138 dB
over the eight 40x72 navigator frames (BICUBIC-upscaled ramps), where the float64 oracle encoder shows the same +0.138: on frames
this small the two encoders (float DCT and box chroma mean here; integer DCT, fixed-point colour transform and biased chroma
rounding in libjpeg) scatter either way by a tenth of a dB.  So the bound is 2 * 0.138 = 0.276 dB."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as J
import video_cases as C
from test_gpu_inference import tiny  # noqa: F401  (the tiny U-Net / pipeline fixture of the episode tests)

pytestmark = pytest.mark.gpu
DEV = "cuda"
PSNR_SLACK = 0.276          # dB: max(2 * the largest measured shortfall (0.138, navigator frame 6), the floor 0.05)
GUARD = 4096                # int16 elements in front of and behind the coefficients (a multiple of 8: the view stays 16-byte aligned)
PATTERN = 0x5A5A
ALL = [(n, s) for n in C.CASES for s in C.SUBSAMPLINGS]
_device = {}


def _pil_sub(subsampling):
    return {"4:2:0": 2, "4:4:4": 0}[subsampling]


def _decode(jpeg):
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))


def _pillow_psnr(frame, quality, subsampling):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", quality=quality, subsampling=_pil_sub(subsampling))
    return J.psnr(_decode(b.getvalue()), frame)


def _check_psnr(label, jpegs, frames, quality, subsampling):
    """every decoded frame against its source: prints each figure, then asserts the worst shortfall against Pillow's own encoder"""
    worst = -np.inf
    for v, (jpeg, frame) in enumerate(zip(jpegs, frames)):
        img = Image.open(io.BytesIO(jpeg))
        assert img.size == (frame.shape[1], frame.shape[0]) and img.mode == "RGB"
        ours, theirs = J.psnr(np.asarray(img), frame), _pillow_psnr(frame, quality, subsampling)
        print(f"PSNR {label} {subsampling} frame {v}: device {ours:.3f} dB, Pillow's encoder {theirs:.3f} dB, shortfall {theirs - ours:+.3f}")
        worst = max(worst, theirs - ours)
    assert worst <= PSNR_SLACK, f"{label}: {worst:.3f} dB below Pillow's encoder"


def _coefficients_guarded(frames, quality, subsampling):
    """ops.jpeg_dct_quant into a view between two prefilled guard bands -> the coefficients on the host"""
    from evoworld_amd import ops
    V, H, W, _ = frames.shape
    mcu, bpm = J.MCU[subsampling], J.BPM[subsampling]
    shape = (V, -(-H // mcu), -(-W // mcu), bpm, 64)
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int16, device=DEV)
    out = buf[GUARD: GUARD + n].view(shape)
    got = ops.jpeg_dct_quant(torch.from_numpy(frames).to(DEV), quality, subsampling, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n:] == PATTERN).all()), "guard band written"
    return got


def device(name, subsampling):
    """(coefficients int16 on the host, [jpeg bytes per frame]) of a case, computed once"""
    from evoworld_amd import video
    key = (name, subsampling)
    if key not in _device:
        frames, quality = C.CASES[name]
        coef = _coefficients_guarded(frames, quality, subsampling)
        jpegs = video.encode_jpeg(torch.from_numpy(frames).to(DEV), quality, subsampling)
        _device[key] = (coef.cpu().numpy(), jpegs)
    return _device[key]


@pytest.mark.parametrize("name,subsampling", ALL)
def test_coefficients_against_the_oracle(name, subsampling):
    quot, want = C.oracle(name, subsampling)
    ties = J.near_ties(quot)
    assert ties.mean() <= 0.002                                            # the precondition, on the oracle alone
    got, _ = device(name, subsampling)
    assert got.shape == want.shape and got.dtype == np.int16
    diff = got.astype(np.int32) - want.astype(np.int32)
    wrong = diff != 0
    print(f"{name} {subsampling}: {int(wrong.sum())} of {wrong.size} coefficients differ, {int(ties.sum())} near ties")
    assert np.abs(diff).max() <= 1, f"a coefficient is off by {np.abs(diff).max()}"
    assert not (wrong & ~ties).any(), f"{int((wrong & ~ties).sum())} coefficients differ away from a tie"
    assert np.abs(got[..., 1:]).max() <= 1023 and got[..., 0].min() >= -1024 and got[..., 0].max() <= 1023


@pytest.mark.parametrize("name,subsampling", ALL)
def test_stream_is_the_oracle_packing_of_the_device_coefficients(name, subsampling):
    from evoworld_amd import video
    frames, quality = C.CASES[name]
    coef, jpegs = device(name, subsampling)
    V, H, W, _ = frames.shape
    assert len(jpegs) == V
    for v in range(V):
        want = J.frame_bytes(coef[v], W, H, quality, subsampling)
        assert jpegs[v] == want, f"frame {v}: {len(jpegs[v])} bytes against {len(want)}"
    again = video.encode_jpeg(torch.from_numpy(frames).to(DEV), quality, subsampling)
    assert again == jpegs                                                  # no atomics on global memory, no data-dependent order


def test_streams_hold_stuffing_zrl_and_the_widest_categories():
    """preconditions of the entropy test: a stuffed FF 00, ZRL, a DC difference of category 11 and an AC coefficient of category 10"""
    stuffed = zrl = 0
    for name, sub in ALL:
        coef, _ = device(name, sub)
        st = {}
        for v in range(len(coef)):
            J.pack_scan(coef[v], sub, st)
        stuffed += st.get("stuffed", 0)
        zrl += st.get("zrl", 0)
    assert stuffed > 0 and zrl > 0
    coef, _ = device("halves_16x32", "4:4:4")
    assert np.abs(np.diff(coef[0, 0, :, 0, 0].astype(np.int32))).max() >= 1024          # category 11
    coef, _ = device("synth_max_16x32", "4:4:4")
    assert np.abs(coef[..., 1:]).max() == 1020                              # the most an image can reach (video_cases.synth_max)


@pytest.mark.parametrize("bpm,mc", [(3, 100), (6, 90)])
def test_entropy_clamps_injected_coefficients(bpm, mc):
    """The entropy coder on coefficients no image produces: every block at the provable worst case (DC differences of +-2047, 63 AC
    coefficients of +-1023: 26 bits each), values beyond the tables' range (clamped to them), and more than two rounds of 256
    blocks, so that the LDS bit buffer is full in every round and a partial byte is carried."""
    from evoworld_amd import ops
    sub = {3: "4:4:4", 6: "4:2:0"}[bpm]
    rng = np.random.default_rng(bpm)
    coef = np.zeros((2, 2, mc, bpm, 64), np.int16)
    coef[0, 0] = rng.choice(np.array([-1023, 1023], np.int16), (mc, bpm, 64))
    coef[0, 0, :, :, 0] = np.where(np.arange(mc)[:, None] % 2 == 0, -1024, 1023)
    coef[0, 1] = rng.integers(-1023, 1024, (mc, bpm, 64))
    coef[1, 0] = rng.integers(-3000, 3000, (mc, bpm, 64))                  # AC out of range: clamped, never overrun
    coef[1, 0, :, :, 0] = rng.integers(-1024, 1024, (mc, bpm))
    coef[1, 1] = rng.integers(-2, 3, (mc, bpm, 64))
    clamped = coef.copy()
    clamped[..., 1:] = np.clip(coef[..., 1:], -1023, 1023)
    d = torch.from_numpy(coef).to(DEV)
    slots, seg_bytes = ops.jpeg_entropy(d)
    stream, frame_bytes = ops.jpeg_pack(slots, seg_bytes, 2)
    data = stream.cpu().numpy().tobytes()
    assert int(seg_bytes.max()) <= slots.shape[1]
    at = 0
    for v in range(2):
        n = int(frame_bytes[v])
        assert data[at: at + n] == J.pack_scan(clamped[v], sub)
        at += n
    assert at == len(data)
    s2, b2 = ops.jpeg_entropy(d)
    assert torch.equal(b2, seg_bytes)
    for i, n in enumerate(seg_bytes.tolist()):
        assert torch.equal(s2[i, :n], slots[i, :n])


@pytest.mark.parametrize("name,subsampling", ALL)
def test_pillow_decodes_and_psnr(name, subsampling):
    frames, quality = C.CASES[name]
    _, jpegs = device(name, subsampling)
    _check_psnr(name, jpegs, frames, quality, subsampling)


def test_refusals():
    from evoworld_amd import _lib, ops, video
    f = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.EvoWorldHipError):
        ops.jpeg_dct_quant(f.cpu(), 90)
    for bad in (0, 101, 90.0):
        with pytest.raises(ValueError):
            ops.jpeg_dct_quant(f, bad)
    with pytest.raises(ValueError):
        ops.jpeg_dct_quant(f, 90, "4:2:2")
    with pytest.raises(ValueError):
        ops.jpeg_dct_quant(f[..., :2].contiguous(), 90)
    odd = torch.zeros(64 * 3 + 8, dtype=torch.int16, device=DEV)[1: 1 + 64 * 3].view(1, 1, 1, 3, 64)      # not 16-byte aligned
    with pytest.raises(_lib.EvoWorldHipError, match="aligned"):
        ops.jpeg_dct_quant(f, 90, "4:4:4", out=odd)
    with pytest.raises(ValueError):
        ops.jpeg_entropy(torch.zeros(1, 1, 1, 4, 64, dtype=torch.int16, device=DEV))
    with pytest.raises(_lib.EvoWorldHipError):
        ops.jpeg_entropy(torch.zeros(1, 1, 1, 3, 64, dtype=torch.int16))
    with pytest.raises(ValueError):
        video.encode_jpeg(f, quality=0)
    assert video.encode_jpeg(f[:0]) == []


def test_write_video_round_trip_and_float_frames(tmp_path):
    from evoworld_amd import ops, video
    frames, _ = C.CASES["ramp_40x72"]
    d = torch.from_numpy(frames).to(DEV)
    path = str(tmp_path / "clip.avi")
    size = video.write_video(path, d, fps=7, quality=90)
    assert size == os.path.getsize(path)
    fps, width, height, jpegs = video.read_avi(path)
    assert (fps, width, height, len(jpegs)) == (7, 72, 40, 3)
    assert jpegs == video.encode_jpeg(d, 90, "4:2:0")
    for j, f in zip(jpegs, frames):
        assert _decode(j).shape == f.shape
    as_float = ops.u8_hwc_to_f32_chw(d)                                    # float [V,3,H,W] in [-1,1] maps back to the same 8-bit frames
    assert video.encode_jpeg(as_float, 90, "4:2:0") == jpegs
    with pytest.raises(ValueError, match="H.264"):
        video.write_video(str(tmp_path / "clip.mp4"), d)


def test_navigator_save_video_and_gif(tmp_path):
    from evoworld_amd import video
    from evoworld_amd.inference import Navigator
    nav = Navigator(None, height=40, width=72, num_frames=5)
    nav.save_video(str(tmp_path / "none.avi"))                             # empty generations: logs, writes nothing
    nav.save_gif(str(tmp_path / "none.gif"))
    assert not os.listdir(tmp_path)
    small = C._ramp(5, 20, 36)                                             # two windows at half the navigator's size: BICUBIC upscale
    pil_window = [[Image.fromarray(f) for f in small]]
    pt_window = torch.from_numpy(small[None]).permute(0, 1, 4, 2, 3).float() / 255
    nav.generations = [(pil_window, 3), (pt_window, 5)]
    want = np.stack([np.asarray(Image.fromarray(f).resize((72, 40), Image.BICUBIC)) for f in list(small[:3]) + list(small)])
    assert np.array_equal(nav.generated_frames_u8().cpu().numpy(), want)   # Pillow's BICUBIC bit for bit, first n frames per window
    nav.save_video(str(tmp_path / "nav.avi"), fps=10)
    fps, width, height, jpegs = video.read_avi(str(tmp_path / "nav.avi"))
    assert (fps, width, height, len(jpegs)) == (10, 72, 40, 8)
    _check_psnr("navigator", jpegs, want, 90, "4:2:0")
    nav.save_gif(str(tmp_path / "nav.gif"), fps=10)
    gif = Image.open(str(tmp_path / "nav.gif"))
    assert gif.n_frames == 8 and gif.size == (72, 40) and gif.info["duration"] == 100 and gif.info["loop"] == 0
    with pytest.raises(ValueError, match="avi"):
        nav.save_video(str(tmp_path / "nav.mp4"))
    nav.generations = [(torch.zeros(1, 5, 4, 5, 9), 5)]                    # latents
    with pytest.raises(NotImplementedError, match="latent"):
        nav.save_video(str(tmp_path / "latent.avi"))
    with pytest.raises(NotImplementedError, match="latent"):
        nav.save_gif(str(tmp_path / "latent.gif"))


def test_process_episode_writes_navigated_avi(tiny, tmp_path):  # noqa: F811
    from evoworld_amd import video
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.stages import SyntheticStages
    from test_gpu_pointcloud import _poses
    cfg, pipe = tiny
    H, W, T = 128, 256, 25
    cam, _ = _poses(60)
    st = SyntheticStages(cross_attention_dim=cfg["cross_attention_dim"], camera_params=cam, depth_hw=(48, 64))
    saved = (pipe.vae, pipe.image_encoder, pipe.vae_scale_factor)
    pipe.set_components(vae=st.vae, image_encoder=st.image_encoder)
    plain_dir, video_dir = tmp_path / "plain", tmp_path / "video"
    try:
        loop = UnifiedLoopConsistencyPipeline(pipe, st.depth_model, height=H, width=W, num_frames=T, num_segments=2,
                                              num_inference_steps=1, pano_size=(64, 128), face_res=32)
        start = (torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
        plain = loop.process_episode(start, cam, save_dir=str(plain_dir), save_video=False)
        frames = loop.process_episode(start, cam, save_dir=str(video_dir), save_video=True, video_fps=12, video_quality=85)
        u8 = loop.last_frames_u8.cpu().numpy()
    finally:
        pipe.vae, pipe.image_encoder, pipe.vae_scale_factor = saved
    assert frames.shape == (49, 3, H, W) and torch.equal(frames, plain)
    assert not [f for f in os.listdir(plain_dir) if f.endswith(".avi")]
    assert sorted(f for f in os.listdir(video_dir) if f.endswith(".avi")) == ["navigated.avi"]      # no panoramas: no original.avi
    fps, width, height, jpegs = video.read_avi(str(video_dir / "navigated.avi"))
    assert (fps, width, height, len(jpegs)) == (12, W, H, 49)
    pick = [0, 24, 25, 48]
    _check_psnr("episode", [jpegs[i] for i in pick], u8[pick], 85, "4:2:0")
