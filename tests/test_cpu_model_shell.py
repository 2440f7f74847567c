"""-m "not gpu": the shell the U-Net, the VAE and CLIP share (evoworld_amd/_model.py).  The spec and random-weight constants were computed on
the commit before the shell existed: key order, shapes and the random generators' bits are what the goldens under tests/golden/ were made
from, so none of them may move.  The behaviour checks pin the loader's exception types and texts, which callers match on."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def _configs():
    from evoworld_amd.clip import DEFAULT_CLIP_CONFIG
    from evoworld_amd.unet import DEFAULT_CONFIG
    from evoworld_amd.vae import DEFAULT_VAE_CONFIG
    from oracle.clip_ref import tiny_clip_config
    from oracle.unet_ref import tiny_config
    from oracle.vae_ref import tiny_vae_config
    return {"unet_default": DEFAULT_CONFIG, "unet_tiny": {**DEFAULT_CONFIG, **tiny_config()},
            "unet_320": {**DEFAULT_CONFIG, **tiny_config(), "block_out_channels": (320, 128, 256, 256), "num_attention_heads": (5, 2, 4, 4)},
            "vae_default": DEFAULT_VAE_CONFIG, "vae_tiny": {**DEFAULT_VAE_CONFIG, **tiny_vae_config()},
            "clip_default": DEFAULT_CLIP_CONFIG, "clip_tiny": {**DEFAULT_CLIP_CONFIG, **tiny_clip_config()}}


def _model(kind):
    from evoworld_amd import clip, unet, vae
    return {"unet": (unet.UNetSpatioTemporalConditionModel, unet.param_spec, unet.random_state_dict, "state dict is missing",
                     "diffusion_pytorch_model.safetensors", "no diffusion_pytorch_model*.safetensors under "),
            "vae": (vae.AutoencoderKLTemporalDecoder, vae.vae_param_spec, vae.random_vae_state_dict, "VAE state dict is missing",
                    "diffusion_pytorch_model.fp16.safetensors", "no diffusion_pytorch_model*.safetensors under "),
            "clip": (clip.CLIPVisionModelWithProjection, clip.clip_param_spec, clip.random_clip_state_dict, "CLIP state dict is missing",
                     "model.safetensors", "no model*.safetensors under ")}[kind]


SPEC_SHA = {
    "unet_default": "a70cf13d855dfbeb4b1a9787c3d15f482ad60a97d2e2e2be726daeccebef86c8",
    "unet_tiny": "c33977b778bcc896f9c91bce05076b69f0683e1491abd3e8dbea9dfd822eaf6a",
    "unet_320": "44b32e398d84793caa64ceec3dd1b86a11d7531bd1f7094051f383b08c8d51b6",
    "vae_default": "051157dd2c6ab7f3943fae3dc47a2aa5b8eb7f2d981dc0cec51d9ee758f0d4f5",
    "vae_tiny": "bd6c105ee442574951500cd8907ebcb99313302fd6acde198fb7e73bb4337e27",
    "clip_default": "f51e68a5ebac5b1bc84a007f266765cd363297b4ce1f3651e23bab3c19358fd2",
    "clip_tiny": "ec97158d29a2b15bc3cbc02826b4d86fc48fca8ef4c379d81f06eeccb03ff5fa",
}
RANDOM_SHA = {
    ("unet_tiny", 0): "0815a5d372e64caf379f63e0a00e6b4c2848e0adc081a1beb61fc0ab34bedea9",
    ("unet_tiny", 3): "02ba1da9316e8041a4c7d5d425258f7371f03e9f5f7a558112baf769b61bead0",
    ("unet_tiny", 5): "0d968f1e6eae0d2547b7129593de3a530b7678cc7f5fdd36be613995fadf6777",
    ("unet_tiny", 7): "bd2a56905c1e84b7d6b9908539458248f174f819a896a3373e91efc955c08569",
    ("unet_tiny", 11): "af097713abf3592ab33a7b723f8163605dd989518a6b73bf7b14596054c9cb48",
    ("unet_320", 11): "d657a54e56f6296e26b756739fdfdddd2bc43336df7dcee4b2cdc31f2e45c297",     # the weights of the fused feed-forward tests
    ("unet_tiny", "golden"): "02ba1da9316e8041a4c7d5d425258f7371f03e9f5f7a558112baf769b61bead0",
    ("vae_tiny", 0): "9c9073bec94089f219ae6d0225e9363393fc0e33eb30ae0acd81d7fe79c7fad1",
    ("clip_tiny", 0): "d643880c6bf8a4fb916a1d7b4eff1e974f7f5ba4d1ef67edc781894688001584",
    ("clip_tiny", 1): "397a0c7c59f6833b3343bf3651d787e69cbd3b3dc526563028b5402785a1b81c",
    ("clip_tiny", 2): "e6cb6aa4c46b641ae6d80b144a4e896c6f4bf041a613034ecd6424bd4180acab",
}


def spec_sha(name):
    spec = _model(name.split("_")[0])[1](_configs()[name])
    return hashlib.sha256("".join(f"{k} {tuple(shape)}\n" for k, (shape, _) in spec.items()).encode()).hexdigest()


def random_sha(name, seed):
    if seed == "golden":
        seed = int(np.load(os.path.join(GOLDEN, "pipeline_glue.npz"))["unet_seed"])
    sd = _model(name.split("_")[0])[2](_configs()[name], seed)
    return hashlib.sha256(b"".join(v.numpy().tobytes() for v in sd.values())).hexdigest()


@pytest.mark.parametrize("name", sorted(SPEC_SHA))
def test_param_spec_keys_and_shapes_are_pinned(name):
    assert spec_sha(name) == SPEC_SHA[name]


@pytest.mark.parametrize("name,seed", sorted(RANDOM_SHA, key=str))
def test_random_state_dict_bits_are_pinned(name, seed):
    assert random_sha(name, seed) == RANDOM_SHA[(name, seed)]


def test_one_kind_vocabulary():
    for name in SPEC_SHA:
        for key, (shape, kind) in _model(name.split("_")[0])[1](_configs()[name]).items():
            assert kind in ("gamma", "beta", "mix") or type(kind) is int and kind >= 1, (name, key, kind)
    from evoworld_amd.clip import clip_param_spec
    spec = clip_param_spec(_configs()["clip_tiny"])
    assert spec["vision_model.embeddings.class_embedding"][1] == 1 and spec["vision_model.embeddings.position_embedding.weight"][1] == 1


KINDS = ("unet", "vae", "clip")


@pytest.fixture(scope="module")
def tiny_sd():
    return {kind: (_configs()[kind + "_tiny"], _model(kind)[2](_configs()[kind + "_tiny"], 0)) for kind in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_load_state_dict_validation(kind, tiny_sd):
    cls, _, _, prefix, _, _ = _model(kind)
    cfg, sd = tiny_sd[kind]
    keys = list(sd)
    gone, bent = keys[3], keys[5]
    with pytest.raises(KeyError) as e:
        cls(**cfg).load_state_dict({k: v for k, v in sd.items() if k != gone}, device="cpu")      # validation comes before the device check
    assert f"{prefix} 1 keys, e.g. ['{gone}']" in str(e.value)
    bad = dict(sd)
    bad[bent] = torch.zeros(*sd[bent].shape, 2)
    with pytest.raises(ValueError) as e:
        cls(**cfg).load_state_dict(bad, device="cpu")
    assert str(e.value) == f"{bent}: expected shape {tuple(sd[bent].shape)}, got {tuple(bad[bent].shape)}"
    with pytest.raises(RuntimeError) as e:
        cls(**cfg).load_state_dict(sd, device="cpu")
    assert str(e.value) == f"evoworld_amd.{cls.__name__} needs a GPU device (no CPU path)"
    with pytest.raises(RuntimeError) as e:
        cls.from_random(seed=0, device="cpu", **cfg)
    assert str(e.value) == f"evoworld_amd.{cls.__name__} needs a GPU device (no CPU path)"


def _write_checkpoint(root, kind, tiny_sd, config):
    from safetensors.torch import save_file
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "config.json"), "w") as f:
        json.dump(config, f)
    save_file({k: v.contiguous() for k, v in tiny_sd[kind][1].items()}, os.path.join(root, _model(kind)[4]))


def _jsonable(cfg):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}


@pytest.mark.parametrize("kind,layout", [("unet", "top"), ("vae", "top"), ("clip", "top"), ("clip", "vision_config")])
def test_from_pretrained_applies_the_config_and_reaches_the_device_check(kind, layout, tiny_sd, tmp_path, monkeypatch):
    """The tiny weights only pass the shape check under the tiny config, so reaching the device error proves config.json was applied."""
    cls = _model(kind)[0]
    cfg = _jsonable(tiny_sd[kind][0])
    raw = {"vision_config": cfg, "model_type": "clip"} if layout == "vision_config" else dict(cfg)
    raw["_class_name"] = "not a config key"
    seen = {}
    real = cls.__init__

    def spy(self, **config):
        seen.update(config)
        real(self, **config)
    monkeypatch.setattr(cls, "__init__", spy)
    _write_checkpoint(str(tmp_path / "sub"), kind, tiny_sd, raw)
    with pytest.raises(RuntimeError) as e:
        cls.from_pretrained(str(tmp_path), subfolder="sub", device="cpu", torch_dtype=torch.float16)       # extra keywords are ignored
    assert str(e.value) == f"evoworld_amd.{cls.__name__} needs a GPU device (no CPU path)"
    assert "_class_name" not in seen and "vision_config" not in seen and "model_type" not in seen
    want = tiny_sd[kind][0]
    assert {k: (tuple(seen[k]) if isinstance(want[k], tuple) else seen[k]) for k in want} == dict(want)
    if kind == "unet":
        assert all(isinstance(seen[k], tuple) for k in ("block_out_channels", "num_attention_heads", "down_block_types", "up_block_types"))
        assert "qkv_fp8" not in seen                         # None: the environment switch decides
        with pytest.raises(RuntimeError):
            cls.from_pretrained(str(tmp_path / "sub"), device="cpu", qkv_fp8=True)
        assert seen["qkv_fp8"] is True


@pytest.mark.parametrize("kind", KINDS)
def test_from_pretrained_without_weights(kind, tmp_path):
    cls, text = _model(kind)[0], _model(kind)[5]
    with pytest.raises(FileNotFoundError) as e:
        cls.from_pretrained(str(tmp_path), device="cpu")
    assert str(e.value) == text + str(tmp_path)
    with pytest.raises(FileNotFoundError) as e:
        cls.from_pretrained(str(tmp_path), subfolder="x", device="cpu")
    assert str(e.value) == text + os.path.join(str(tmp_path), "x")


@pytest.mark.parametrize("kind", KINDS)
def test_calls_before_loading_and_stubs(kind, tiny_sd):
    cls = _model(kind)[0]
    m = cls(**tiny_sd[kind][0])
    calls = {"unet": [lambda: m(torch.zeros(1, 4, 18, 8, 8), 1.0, torch.zeros(1, 1, 64), torch.zeros(1, 3))],
             "vae": [lambda: m.encode(torch.zeros(1, 3, 8, 8)), lambda: m.decode(torch.zeros(1, 4, 8, 8))],
             "clip": [lambda: m(torch.zeros(1, 3, 56, 56))]}[kind]
    for call in calls:
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "weights not loaded"
    assert m.eval() is m and m.requires_grad_(False) is m and m.to("cpu") is m and m.to(dtype=torch.float16) is m


def test_unet_to_refuses_a_device_change():
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel
    m = UNetSpatioTemporalConditionModel(**_configs()["unet_tiny"])
    m.w, m.device = {}, torch.device("cuda:0")           # as after a load
    assert m.to("cuda:0") is m
    with pytest.raises(NotImplementedError):
        m.to("cpu")


def test_config_reader_is_the_shared_one(tmp_path):
    """unified_loop_consistency.py builds the zero-weight ranks' config with the reader from_pretrained uses, not with a filter of its own."""
    import unified_loop_consistency  # noqa: F401  (imports without a filter of its own)
    from evoworld_amd._model import PackedModel
    from evoworld_amd.unet import DEFAULT_CONFIG, UNetSpatioTemporalConditionModel
    assert UNetSpatioTemporalConditionModel.read_config.__func__ is PackedModel.read_config.__func__
    raw = {"block_out_channels": [64, 128], "num_frames": 7, "_diffusers_version": "0.24", "not_a_key": [1]}
    assert UNetSpatioTemporalConditionModel._config_from_json(raw) == {"block_out_channels": (64, 128), "num_frames": 7}
    assert set(UNetSpatioTemporalConditionModel._config_from_json({k: 0 for k in list(DEFAULT_CONFIG) + ["x"]})) == set(DEFAULT_CONFIG)
    assert UNetSpatioTemporalConditionModel.read_config(str(tmp_path)) == {}
    with open(tmp_path / "config.json", "w") as f:
        json.dump(raw, f)
    assert UNetSpatioTemporalConditionModel.read_config(str(tmp_path)) == {"block_out_channels": (64, 128), "num_frames": 7}
