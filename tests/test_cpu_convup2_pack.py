"""The weight pack of ew_gemm_f16's upsample=2 form (ops.pack_convup2_weight), on the CPU: a 3x3 conv over a nearest-x2 upsampled image is four
2x2 convs over the source image, one per output parity (a, b), whose taps are sums of the 3x3 taps that read the same source pixel.

- identity: the four-phase form evaluated from the pack (restated below from the layout in include/evoworld_hip.h, zero padding on the SOURCE
  image) equals conv2d(interpolate(x, 2, "nearest"), w, padding=1) in fp64 to 1e-12, borders included;
- rounding: with the sums formed in fp32 and rounded to fp16 once, the weight-rounding error of the result is no larger than that of nine
  separately rounded taps (ratio <= 1.10: the expectation is 1 -- fewer, larger roundings -- and the margin covers the seed-to-seed spread);
- the identity check is not vacuous: with the a = 0 and a = 1 row groupings swapped it fails."""
import math

import pytest
import torch
import torch.nn.functional as F

SHAPES = [(2, 64, 48, 5, 7), (1, 320, 64, 9, 16)]      # n, C, O, h, w


def rnd(*shape, seed=0, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def four_phase(x, pack):
    """x [n, C, h, w], pack [4 O, 4 C] = [phase 2a+b][O][C/64][tap 2r+c][64] -> [n, O, 2h, 2w] in fp64: output (2i + a, 2j + b) =
    sum over taps (r, c) of W[phase][tap] . x[i + a - 1 + r, j + b - 1 + c], zero outside the source image"""
    n, C, h, w = x.shape
    O = pack.shape[0] // 4
    wt = pack.double().reshape(4, O, C // 64, 4, 64).permute(0, 3, 1, 2, 4).reshape(4, 4, O, C)      # [phase, tap, O, C]
    xp = F.pad(x.double(), (1, 1, 1, 1))
    out = torch.zeros(n, O, 2 * h, 2 * w, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for c in range(2):
                    src = xp[:, :, a + r: a + r + h, b + c: b + c + w]
                    out[:, :, a::2, b::2] += torch.einsum("oc,nchw->nohw", wt[2 * a + b, 2 * r + c], src)
    return out


def nine_tap(x, w):
    return F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), padding=1)


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def data(request):
    n, C, O, h, w = request.param
    x = rnd(n, C, h, w, seed=1).half().double()
    w32 = (rnd(O, C, 3, 3, seed=2) / math.sqrt(9 * C)).float()
    return x, w32, nine_tap(x, w32)


def test_four_phase_pack_is_the_upsampled_conv(data):
    from evoworld_amd import ops
    x, w32, exact = data
    got = four_phase(x, ops.pack_convup2_weight(w32.double(), dtype=torch.float64))
    err = float((got - exact).abs().max() / exact.abs().max())
    print(f"four-phase identity: max error {err:.2e} of the largest output")
    assert err <= 1e-12


def test_phase_sums_round_no_worse_than_nine_taps(data):
    from evoworld_amd import ops
    x, w32, exact = data
    pack = ops.pack_convup2_weight(w32)
    assert pack.dtype == torch.float16 and pack.shape == (4 * w32.shape[0], 4 * w32.shape[1])
    e_phase = rel_l2(four_phase(x, pack), exact)
    e_nine = rel_l2(nine_tap(x, w32.half()), exact)
    print(f"weight rounding rel-L2: phase pack {e_phase:.3e}, nine taps {e_nine:.3e}, ratio {e_phase / e_nine:.3f}")
    assert e_phase <= 1.10 * e_nine


def test_swapped_row_groupings_fail_the_identity(data, monkeypatch):
    from evoworld_amd import ops
    x, w32, exact = data
    monkeypatch.setattr(ops, "CONVUP2_TAPS", ops.CONVUP2_TAPS[::-1])
    got = four_phase(x, ops.pack_convup2_weight(w32.double(), dtype=torch.float64))
    assert float((got - exact).abs().max() / exact.abs().max()) > 1e-2


def test_pack_refuses_other_kernels():
    from evoworld_amd import ops
    with pytest.raises(ValueError):
        ops.pack_convup2_weight(torch.zeros(8, 64, 3, 1, 1))
    with pytest.raises(ValueError):
        ops.pack_convup2_weight(torch.zeros(8, 48, 3, 3))
