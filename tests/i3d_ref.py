"""fp32 PyTorch restatement of what evoworld_amd.fvd computes, for the tests: styleganv's clip preprocessing, the I3D network
(Inception-v1 inflated to 3-D, 400 classes) from a state dict in InceptionI3d's key layout, and the Frechet distance.  Written from the
architecture's definition with F.conv3d, BatchNorm spelled out and F.max_pool3d on zero-padded input; nothing here shares code with the
package (the layer tables are restated too), so that a wrong table entry there shows as a difference."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
INCEPTION = {"Mixed_3b": (64, 96, 128, 16, 32, 32), "Mixed_3c": (128, 128, 192, 32, 96, 64), "Mixed_4b": (192, 96, 208, 16, 48, 64),
             "Mixed_4c": (160, 112, 224, 24, 64, 64), "Mixed_4d": (128, 128, 256, 24, 64, 64), "Mixed_4e": (112, 144, 288, 32, 64, 64),
             "Mixed_4f": (256, 160, 320, 32, 128, 128), "Mixed_5b": (256, 160, 320, 32, 128, 128), "Mixed_5c": (384, 192, 384, 48, 128, 128)}
ORDER = ("Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "Conv3d_2b_1x1", "Conv3d_2c_3x3", "MaxPool3d_3a_3x3", "Mixed_3b", "Mixed_3c", "MaxPool3d_4a_3x3",
         "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f", "MaxPool3d_5a_2x2", "Mixed_5b", "Mixed_5c")
POOLS = {"MaxPool3d_2a_3x3": ((1, 3, 3), (1, 2, 2)), "MaxPool3d_3a_3x3": ((1, 3, 3), (1, 2, 2)), "MaxPool3d_4a_3x3": ((3, 3, 3), (2, 2, 2)),
         "MaxPool3d_5a_2x2": ((2, 2, 2), (2, 2, 2))}
STEM_STRIDE = {"Conv3d_1a_7x7": 2, "Conv3d_2b_1x1": 1, "Conv3d_2c_3x3": 1}


def pad_total(n, k, s):
    """the total "SAME" padding along one axis of n samples for a window k at stride s"""
    r = n % s
    return max(k - (s if r == 0 else r), 0)


def pad_same(x, kernel, stride):
    """x [N,C,T,H,W] zero-padded so that a window `kernel` at `stride` gives ceil(n / stride) outputs; the smaller half goes in front"""
    pads = []
    for n, k, s in zip(reversed(x.shape[2:]), reversed(kernel), reversed(stride)):
        p = pad_total(n, k, s)
        pads += [p // 2, p - p // 2]
    return F.pad(x, pads)


def preprocess(video, size=224):
    """video fp32 [3,T,H,W] in [0,1] -> [3,T,224,224] in [-1,1]: shorter side to `size` (bilinear, align_corners=False, no antialias),
    centre crop, (x - 0.5) * 2"""
    _, _, h, w = video.shape
    scale = size / min(h, w)
    target = (size, math.ceil(w * scale)) if h < w else (math.ceil(h * scale), size)
    v = F.interpolate(video, size=target, mode="bilinear", align_corners=False)
    y0, x0 = (v.shape[2] - size) // 2, (v.shape[3] - size) // 2
    return ((v[:, :, y0:y0 + size, x0:x0 + size] - 0.5) * 2).contiguous()


def clip_input(clip, channel_order="rgb"):
    """uint8 [T,H,W,3] or fp32 [T,3,H,W] in [0,1] -> the network's input fp32 [1,3,T,224,224]"""
    v = clip.permute(0, 3, 1, 2).float() / 255.0 if clip.dtype == torch.uint8 else clip.float()
    if channel_order == "bgr":
        v = v.flip(1)
    return preprocess(v.permute(1, 0, 2, 3).contiguous())[None]


def unit(x, sd, name, stride=1, relu_in=True):
    """conv3d (no bias, SAME) + BatchNorm3d in eval mode, WITHOUT the ReLU that follows: the input's ReLU is applied here instead"""
    w = sd[f"{name}.conv3d.weight"].float()
    k, s = tuple(w.shape[2:]), (stride,) * 3
    y = F.conv3d(pad_same(F.relu(x) if relu_in else x, k, s), w, stride=s)
    g, b, m, v = (sd[f"{name}.bn.{p}"].float().view(1, -1, 1, 1, 1) for p in ("weight", "bias", "running_mean", "running_var"))
    return (y - m) / torch.sqrt(v + EPS) * g + b


def pool(x, kernel, stride):
    return F.max_pool3d(pad_same(F.relu(x), kernel, stride), kernel, stride)


def inception(x, sd, name):
    b0 = unit(x, sd, f"{name}.b0")
    b1 = unit(unit(x, sd, f"{name}.b1a"), sd, f"{name}.b1b")
    b2 = unit(unit(x, sd, f"{name}.b2a"), sd, f"{name}.b2b")
    b3 = unit(pool(x, (3, 3, 3), (1, 1, 1)), sd, f"{name}.b3b")
    return torch.cat([b0, b1, b2, b3], 1)


@torch.no_grad()
def endpoints(x, sd):
    """x fp32 [N,3,T,224,224] -> {endpoint: [N,C,T,H,W]} (pre-ReLU for convolutions and modules) and 'Logits' [N,400]"""
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    out = {}
    for name in ORDER:
        if name in POOLS:
            x = pool(x, *POOLS[name])
        elif name in INCEPTION:
            x = inception(x, sd, name)
        else:
            x = unit(x, sd, name, STEM_STRIDE[name], relu_in=name != "Conv3d_1a_7x7")
        out[name] = x
    a = F.avg_pool3d(F.relu(x), (2, 7, 7), 1)
    y = F.conv3d(a, sd["logits.conv3d.weight"].float(), sd["logits.conv3d.bias"].float())
    out["Logits"] = y[:, :, :, 0, 0].mean(2)
    return out


def logits(clip, sd, channel_order="rgb", n_frames=None):
    """uint8 [T,H,W,3] or fp32 [T,3,H,W] clip -> fp32 [400]"""
    return endpoints(clip_input(clip if n_frames is None else clip[:n_frames], channel_order), sd)["Logits"][0]


def frechet(a, b):
    """float64 Frechet distance between the Gaussians fitted to two feature sets [N,d]; N = 1: the squared distance of the means"""
    from scipy.linalg import sqrtm
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = float(np.sum((a.mean(0) - b.mean(0)) ** 2))
    if a.shape[0] == 1:
        return d
    ca, cb = np.cov(a, rowvar=False), np.cov(b, rowvar=False)
    root, _ = sqrtm(ca @ cb, disp=False)
    return float(np.real(d + np.trace(ca + cb - 2 * root)))
