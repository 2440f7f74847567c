"""LPIPS (AlexNet backbone) restated in plain PyTorch from its definition (a helper module, not collected): what
lpips.LPIPS(net='alex', spatial=True).forward(img1, img2).mean() computes per frame pair on frames in [0,1] mapped to [-1,1]
(the reference's evoworld/metrics/other_metrics/calculate_lpips.py).  Neither the lpips package nor its weights exist here, so this
restatement with seeded random weights is the oracle of tests/test_gpu_lpips.py; it runs in the dtype of its inputs (fp32 or fp64)."""
import torch
import torch.nn.functional as F

# (torchvision features index, out channels, in channels, kernel, stride, padding)
CONVS = ((0, 64, 3, 11, 4, 2), (3, 192, 64, 5, 1, 2), (6, 384, 192, 3, 1, 1), (8, 256, 384, 3, 1, 1), (10, 256, 256, 3, 1, 1))
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def random_weights(seed):
    """The seeded lpips.LPIPS-layout state dict the tests load into both sides: the package's one maker (AlexNet's shapes, conv
    weights N(0, 1 / fan-in) so activations stay O(1), biases N(0, 0.1^2), lin weights uniform in [0, 1), i.e. non-negative).
    Only the values come from there; the network below is restated independently."""
    from evoworld_amd.lpips import random_state_dict
    return random_state_dict(seed)


def features(x, sd):
    """x [N,3,H,W] in [-1,1] (channels as the network sees them) -> the five taps (after each ReLU)."""
    dt = x.dtype
    shift = torch.tensor(SHIFT, dtype=dt).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=dt).view(1, 3, 1, 1)
    h = (x - shift) / scale
    taps = []
    for i, (idx, _, _, _, s, p) in enumerate(CONVS):
        if i in (1, 2):
            h = F.max_pool2d(h, kernel_size=3, stride=2)
        h = F.relu(F.conv2d(h, sd[f"net.slice{i + 1}.{idx}.weight"].to(dt), sd[f"net.slice{i + 1}.{idx}.bias"].to(dt), stride=s, padding=p))
        taps.append(h)
    return taps


def normalize(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + eps)


def tap_maps(a, b, sd, channel_order="rgb"):
    """a, b [N,3,H,W] in [0,1], channels R, G, B -> the five upsampled distance maps [N,1,H,W] (channel_order 'bgr': the network
    is handed B, G, R planes)."""
    if channel_order == "bgr":
        a, b = a.flip(1), b.flip(1)
    H, W = a.shape[-2:]
    fa, fb = features(a * 2 - 1, sd), features(b * 2 - 1, sd)
    maps = []
    for i, (ta, tb) in enumerate(zip(fa, fb)):
        d = (normalize(ta) - normalize(tb)) ** 2
        m = F.conv2d(d, sd[f"lin{i}.model.1.weight"].to(d.dtype))
        maps.append(F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False))
    return maps


def lpips_alex(a, b, sd, channel_order="rgb"):
    """a, b [N,3,H,W] in [0,1] -> [N]: the mean over the H x W map of the sum of the five upsampled maps, one frame pair at a time."""
    out = []
    for i in range(a.shape[0]):
        maps = tap_maps(a[i:i + 1], b[i:i + 1], sd, channel_order)
        out.append(sum(maps[1:], maps[0]).mean())
    return torch.stack(out)
