"""-m gpu: the layer kernels the metric networks share (csrc/convnet.hip) on the geometries a 2-D network gives them -- kt = 1 with the image
batch on the T axis, as evoworld_amd.lpips and evoworld_amd.latent_mse call them -- at the smallest shapes that can go wrong, each exact
against F.unfold / F.max_pool2d, guarded and run over two prefills.  Every case also checks that image j's rows are the rows of image j run
alone: with kt = 1 no window may reach into a neighbouring image.  (The 3-D geometries of I3D are in test_gpu_fvd.py, the average pools in
test_gpu_latent_mse.py, the shapes of a 576 x 1024 frame's LPIPS taps in test_gpu_lpips.py.)
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import kernel_checks as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = lambda t: ctypes.c_void_p(t.data_ptr())


def _x(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).half().to(DEV)


def _pool(x, out_hw):
    """ew_maxpool3d_relu_f16 as MaxPool2d(3, 2) of a batch: kernel (1,3,3), stride (1,2,2), no padding -> [n, ho, wo, C]"""
    from evoworld_amd import _lib
    lib = _lib.load()
    (n, h, w, C), (ho, wo) = x.shape, out_hw

    def run(view, prefill):
        _lib.check(lib.ew_maxpool3d_relu_f16(P(x), P(view), n, h, w, C, 1, 3, 3, 1, 2, 2, 0, 0, 0, n, ho, wo, None), "ew_maxpool3d_relu_f16")
    return KC.two_prefills(run, (n * ho * wo, C, torch.float16, {"ld": C}))[0].view.view(n, ho, wo, C)


@pytest.mark.parametrize("shape,out_hw", [((2, 7, 8, 8), (3, 3)),          # width 8: the last column lies in no window
                                          ((1, 3, 3, 16), (1, 1))])        # a single window
def test_maxpool_of_a_batch_is_exact(shape, out_hw):
    from evoworld_amd import ops
    x = _x(shape, 11 + shape[0])
    want = F.max_pool2d(x.permute(0, 3, 1, 2).float().clamp_min(0), 3, 2).permute(0, 2, 3, 1).half().contiguous()
    assert want.shape == (shape[0], *out_hw, shape[3])
    got = _pool(x, out_hw)
    assert torch.equal(got, want)
    assert torch.equal(ops.maxpool3d_relu(x, (1, 3, 3), (1, 2, 2), (0, 0, 0), (shape[0], *out_hw)), want)
    for j in range(shape[0]):
        assert torch.equal(_pool(x[j:j + 1].clone(), out_hw)[0], got[j]), j


def _gather(x, kernel, pads, ldk, relu):
    """ew_im2col3d_f16 as a stride-1 2-D gather of a batch: kernel (1,kh,kw), front pads (0,ph,pw), the output the input's size"""
    from evoworld_amd import _lib
    lib = _lib.load()
    n, h, w, C = x.shape

    def run(view, prefill):
        _lib.check(lib.ew_im2col3d_f16(P(x), P(view), n, h, w, C, 1, *kernel, 1, 1, 1, 0, *pads, n, h, w, ldk, relu, None), "ew_im2col3d_f16")
    return KC.two_prefills(run, (n * h * w, ldk, torch.float16, {"ld": ldk}))[0].view


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape,kernel,pads,ldk", [((2, 6, 7, 8), (5, 5), (2, 2), 256),        # K = 200: 56 zero columns
                                                   ((3, 5, 5, 16), (1, 7), (0, 3), 128)])      # Inception-B: a window wider than the image
def test_gather_of_a_batch_is_exact(shape, kernel, pads, ldk, relu):
    from evoworld_amd import ops
    n, h, w, C = shape
    x = _x(shape, 23 + n)
    taps, K = kernel[0] * kernel[1], kernel[0] * kernel[1] * C
    assert K < ldk
    cols = F.unfold((x.clamp_min(0) if relu else x).permute(0, 3, 1, 2).float(), kernel, padding=pads)       # [n, C*taps, h*w], rows (c, dy, dx)
    want = torch.zeros(n * h * w, ldk, dtype=torch.float16, device=DEV)
    want[:, :K] = cols.view(n, C, taps, h * w).permute(0, 3, 2, 1).reshape(n * h * w, K).half()
    got = _gather(x, kernel, pads, ldk, relu)
    assert torch.equal(got, want) and not got[:, K:].any()
    assert torch.equal(ops.im2col3d(x, (1, *kernel), (1, 1, 1), (0, *pads), (n, h, w), ldk, relu), want)
    for j in range(n):
        assert torch.equal(_gather(x[j:j + 1].clone(), kernel, pads, ldk, relu), got[j * h * w:(j + 1) * h * w]), j
