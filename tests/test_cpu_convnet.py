"""-m 'not gpu': the metric networks' shell evoworld_amd._convnet on the host -- the conv packer's column order and paddings on a toy kernel
whose entries say where they came from, the state-dict validator's refusals, and the BatchNorm fold against torch's own eval-mode BatchNorm
in fp64.  (What the three networks make of it is in test_cpu_lpips.py, test_cpu_fvd.py and test_cpu_latent_mse.py.)"""
import itertools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from evoworld_amd import _convnet as C


@pytest.mark.parametrize("taps", [(2, 3), (2, 2, 3)])
@pytest.mark.parametrize("cpad", [None, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pack_conv_orders_k_as_taps_then_padded_channels(taps, cpad, dtype):
    co, ci = 2, 3
    w = torch.zeros(co, ci, *taps, dtype=dtype)
    code = {}
    for n, idx in enumerate(itertools.product(range(co), range(ci), *(range(t) for t in taps))):
        w[idx] = code[idx] = n + 1                                       # small integers: exact in fp16, none of them zero
    cp = ci if cpad is None else cpad
    n_taps = len(list(itertools.product(*(range(t) for t in taps))))
    K = n_taps * cp
    got = C.pack_conv(w, cpad)
    assert got.dtype == torch.float16 and got.shape == (co, 64 * -(-K // 64)) and got.shape[1] % C.K_ALIGN == 0
    want = torch.zeros_like(got)
    for (o, c, *d), v in code.items():
        tap = 0
        for size, i in zip(taps, d):                                     # ((dt * kh + dy) * kw + dx): the last tap axis runs fastest
            tap = tap * size + i
        want[o, tap * cp + c] = v
    assert torch.equal(got, want)
    assert not got[:, K:].any()                                          # columns beyond K
    assert not got[:, :K].view(co, n_taps, cp)[:, :, ci:].any()          # channels beyond c_in
    assert int((got != 0).sum()) == w.numel()
    with pytest.raises(ValueError, match="cpad"):
        C.pack_conv(w, 2)


def test_pack_conv_pads_k_to_64():
    assert C.pack_conv(torch.ones(4, 3, 11, 11)).shape == (4, 384)       # LPIPS' first layer: K = 363
    assert C.pack_conv(torch.ones(4, 3, 7, 7, 7), 8).shape == (4, 2752)  # I3D's stem: K = 343 * 8 = 2744
    assert C.pack_conv(torch.ones(4, 64, 1, 1), 64).shape == (4, 64)     # already a multiple: nothing added


def test_validate_refusals():
    spec = {"a.weight": (2, 3), "a.bias": (2,), "b.weight": (4,), "c.weight": (1,), "d.weight": (1,)}
    sd = {k: torch.zeros(*s, dtype=torch.float64) for k, s in spec.items()}
    got = C.validate({**sd, "extra.weight": torch.zeros(7), "a.num_batches_tracked": torch.tensor(0)}, spec, "Toy")
    assert list(got) == list(spec) and all(t.dtype == torch.float32 and t.device.type == "cpu" for t in got.values())
    wrapped = C.validate({"module." + k: v for k, v in sd.items()}, spec, "Toy")
    assert list(wrapped) == list(spec) and all(torch.equal(wrapped[k], got[k]) for k in spec)
    few = {k: v for k, v in sd.items() if k in ("a.weight", "a.bias")}
    with pytest.raises(KeyError) as e:
        C.validate(few, spec, "Toy")
    assert "Toy state dict is missing 3 keys, e.g. ['b.weight', 'c.weight', 'd.weight']" in str(e.value) and "expected" not in str(e.value)
    del few["a.bias"]
    with pytest.raises(KeyError) as e:
        C.validate(few, spec, "Toy", "a toy layout")
    assert "missing 4 keys, e.g. ['a.bias', 'b.weight', 'c.weight']; expected a toy layout" in str(e.value)      # the first three only
    with pytest.raises(ValueError, match=r"b\.weight: expected shape \(4,\), got \(5,\)"):
        C.validate({**sd, "b.weight": torch.zeros(5)}, spec, "Toy")


@pytest.mark.parametrize("dims,eps", [(2, 1e-3), (3, 1e-5)])
def test_fold_batchnorm_against_eval_mode_batchnorm(dims, eps):
    g = torch.Generator().manual_seed(dims)
    co, ci, k = 5, 4, (3,) * dims
    sd = {}
    C.random_conv_bn(g, sd, "u", "conv", (co, ci, *k))
    assert list(sd) == ["u.conv.weight", "u.bn.weight", "u.bn.bias", "u.bn.running_mean", "u.bn.running_var"]
    bn = (nn.BatchNorm2d if dims == 2 else nn.BatchNorm3d)(co, eps=eps).double().eval()
    bn.load_state_dict({k_[len("u.bn."):]: v.double() for k_, v in sd.items() if k_.startswith("u.bn.")}, strict=False)
    conv = F.conv2d if dims == 2 else F.conv3d
    x = torch.randn(2, ci, *(6,) * dims, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = bn(conv(x, sd["u.conv.weight"].double()))
    w, b = C.fold_batchnorm(sd, "u", "conv", eps)
    assert w.dtype == b.dtype == torch.float64 and w.shape == (co, ci, *k) and b.shape == (co,)
    got = conv(x, w, b)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((conv(x, *C.fold_batchnorm(sd, "u", "conv", 10 * eps)) - want).abs().max()) > 1e-6        # the eps is used
