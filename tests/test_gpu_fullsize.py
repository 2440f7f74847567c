"""-m gpu: size-independent properties at BASELINE.json's full sizes (configs[1]: [2,25,18,72,128] latents, 1.52 B-parameter
U-Net; reprojection with ~5 M points into 24 x 6 x 512^2 faces), where the fp32 oracle would take hours:
  * two independent kernel families agree: the default path (generation-3/2 GEMMs) against the generation-1 kernels;
  * batch independence: the CFG halves do not see each other (B=2 forward == two B=1 forwards);
  * the splat is deterministic and order-independent (64-bit atomicMin on depth|index), and idempotent under duplicated points.
Tolerances for the U-Net: 5e-3 rel-L2 = two realisations of the fp16 rounding-noise floor."""
import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def full():
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel
    unet = UNetSpatioTemporalConditionModel.from_random(seed=0, device=DEV)
    B, T, h, w = 2, 25, 72, 128
    g = torch.Generator().manual_seed(0)
    x = torch.zeros(B * T * h * w, 64, dtype=torch.float16)
    x[:, :18] = torch.randn(B * T * h * w, 18, generator=g).half()
    ehs = torch.randn(B, 1, 1024, generator=g).half()
    ids = torch.tensor([[6.0, 127.0, 0.02]] * B)
    return unet, x.to(DEV), ehs.to(DEV), ids.to(DEV), (B, T, h, w)


def test_unet_full_size_two_kernel_families_agree(full):
    from evoworld_amd import _lib
    unet, x, ehs, ids, (B, T, h, w) = full
    lib = _lib.load()
    try:
        lib.ew_set_gemm_generation(3)
        a = unet.forward_nhwc(x, 1.234, ehs, ids, B, T, h, w).float().cpu()
        lib.ew_set_gemm_generation(1)
        b = unet.forward_nhwc(x, 1.234, ehs, ids, B, T, h, w).float().cpu()
    finally:
        lib.ew_set_gemm_generation(3)
    assert a.shape == (B * T * h * w, 4) and torch.isfinite(a).all() and torch.isfinite(b).all()
    assert float(a.abs().mean()) > 1e-3
    assert rel_l2(a, b) < 5e-3


def test_unet_full_size_batch_independence(full):
    unet, x, ehs, ids, (B, T, h, w) = full
    rows = T * h * w
    both = unet.forward_nhwc(x, 1.234, ehs, ids, B, T, h, w).float().cpu()
    for i in range(B):
        one = unet.forward_nhwc(x[i * rows:(i + 1) * rows].contiguous(), 1.234, ehs[i:i + 1], ids[i:i + 1], 1, T, h, w).float().cpu()
        assert rel_l2(one, both[i * rows:(i + 1) * rows]) < 5e-3


def test_splat_full_size_deterministic_order_independent_idempotent():
    from evoworld_amd import ops
    from evoworld_amd import reprojection as RP
    n, V, res = 5_000_000, 24, 512
    g = torch.Generator().manual_seed(1)
    xyz = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([6.0, 2.0, 6.0])
    col = torch.randint(0, 256, (n, 3), generator=g, dtype=torch.uint8)
    ang = torch.linspace(0, 2 * np.pi, V + 1)[:-1]
    c2w = torch.eye(4).repeat(V, 1, 1)
    c2w[:, 0, 3], c2w[:, 2, 3] = 0.5 * torch.cos(ang), 0.5 * torch.sin(ang)
    w2c = torch.tensor(RP.face_w2c(c2w.numpy()), dtype=torch.float32).contiguous()
    fx = fy = cx = cy = res / 2.0

    def splat(p, c):
        return ops.splat_cubemap(p.to(DEV), c.to(DEV), w2c.to(DEV), res, fx, fy, cx, cy, 0.1)[0]
    a = splat(xyz, col)
    assert a.shape == (V, 6, res, res, 3) and a.dtype == torch.uint8
    assert torch.equal(a, splat(xyz, col))                                   # deterministic
    assert int((a.float().sum(-1) > 0).sum()) > V * 6 * res * res // 4       # the cloud really covers the faces
    # duplicated points change nothing; a permutation changes nothing wherever the nearest depth is unique
    assert torch.equal(a, splat(torch.cat([xyz, xyz[:1000]]), torch.cat([col, col[:1000]])))
    perm = torch.randperm(n, generator=g)
    b = splat(xyz[perm], col[perm])
    assert float((a != b).any(-1).float().mean()) < 1e-5
