"""An fp32 PyTorch restatement of the network the reference's latent MSE runs (evoworld/metrics/other_metrics/calculate_latent_mse.py:11-79):
timm 1.0.14 `inception_v4` in eval mode with the classifier removed, in timm's key layout (features.{i}.....conv.weight,
features.{i}.....bn.{weight,bias,running_mean,running_var}; BatchNorm eps 1e-3), with the reference's transform (torchvision's Resize((299,
299)) on a float tensor, i.e. F.interpolate(bilinear, antialias=True), then Normalize) and a restatement of its aggregation.
timm, torchvision and the pretrained weights do not exist where these tests run, so parity with timm itself is unpinned: this file, written
from the architecture's description, is the oracle of tests/test_cpu_latent_mse.py and tests/test_gpu_latent_mse.py."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


class ConvNormAct(nn.Module):
    def __init__(self, ci, co, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(ci, co, kernel_size, stride, padding, bias=False)
        self.bn = nn.BatchNorm2d(co, eps=1e-3)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class FoldedConvAct(nn.Module):
    """the same unit with its BatchNorm folded into a biased convolution (set by fold_batchnorm)"""

    def __init__(self, unit, weight, bias):
        super().__init__()
        c = unit.conv
        self.conv = nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, bias=True)
        self.conv.weight.data.copy_(weight)
        self.conv.bias.data.copy_(bias)

    def forward(self, x):
        return F.relu(self.conv(x))


class Mixed3a(nn.Module):
    def __init__(self):
        super().__init__()
        self.maxpool = nn.MaxPool2d(3, stride=2)
        self.conv = ConvNormAct(64, 96, 3, 2)

    def forward(self, x):
        return torch.cat((self.maxpool(x), self.conv(x)), 1)


class Mixed4a(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = nn.Sequential(ConvNormAct(160, 64, 1), ConvNormAct(64, 96, 3))
        self.branch1 = nn.Sequential(ConvNormAct(160, 64, 1), ConvNormAct(64, 64, (1, 7), padding=(0, 3)),
                                     ConvNormAct(64, 64, (7, 1), padding=(3, 0)), ConvNormAct(64, 96, 3))

    def forward(self, x):
        return torch.cat((self.branch0(x), self.branch1(x)), 1)


class Mixed5a(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = ConvNormAct(192, 192, 3, 2)
        self.maxpool = nn.MaxPool2d(3, stride=2)

    def forward(self, x):
        return torch.cat((self.conv(x), self.maxpool(x)), 1)


class InceptionA(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = ConvNormAct(384, 96, 1)
        self.branch1 = nn.Sequential(ConvNormAct(384, 64, 1), ConvNormAct(64, 96, 3, padding=1))
        self.branch2 = nn.Sequential(ConvNormAct(384, 64, 1), ConvNormAct(64, 96, 3, padding=1), ConvNormAct(96, 96, 3, padding=1))
        self.branch3 = nn.Sequential(nn.AvgPool2d(3, stride=1, padding=1, count_include_pad=False), ConvNormAct(384, 96, 1))

    def forward(self, x):
        return torch.cat((self.branch0(x), self.branch1(x), self.branch2(x), self.branch3(x)), 1)


class ReductionA(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = ConvNormAct(384, 384, 3, 2)
        self.branch1 = nn.Sequential(ConvNormAct(384, 192, 1), ConvNormAct(192, 224, 3, padding=1), ConvNormAct(224, 256, 3, 2))
        self.branch2 = nn.MaxPool2d(3, stride=2)

    def forward(self, x):
        return torch.cat((self.branch0(x), self.branch1(x), self.branch2(x)), 1)


class InceptionB(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = ConvNormAct(1024, 384, 1)
        self.branch1 = nn.Sequential(ConvNormAct(1024, 192, 1), ConvNormAct(192, 224, (1, 7), padding=(0, 3)),
                                     ConvNormAct(224, 256, (7, 1), padding=(3, 0)))
        self.branch2 = nn.Sequential(ConvNormAct(1024, 192, 1), ConvNormAct(192, 192, (7, 1), padding=(3, 0)),
                                     ConvNormAct(192, 224, (1, 7), padding=(0, 3)), ConvNormAct(224, 224, (7, 1), padding=(3, 0)),
                                     ConvNormAct(224, 256, (1, 7), padding=(0, 3)))
        self.branch3 = nn.Sequential(nn.AvgPool2d(3, stride=1, padding=1, count_include_pad=False), ConvNormAct(1024, 128, 1))

    def forward(self, x):
        return torch.cat((self.branch0(x), self.branch1(x), self.branch2(x), self.branch3(x)), 1)


class ReductionB(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = nn.Sequential(ConvNormAct(1024, 192, 1), ConvNormAct(192, 192, 3, 2))
        self.branch1 = nn.Sequential(ConvNormAct(1024, 256, 1), ConvNormAct(256, 256, (1, 7), padding=(0, 3)),
                                     ConvNormAct(256, 320, (7, 1), padding=(3, 0)), ConvNormAct(320, 320, 3, 2))
        self.branch2 = nn.MaxPool2d(3, stride=2)

    def forward(self, x):
        return torch.cat((self.branch0(x), self.branch1(x), self.branch2(x)), 1)


class InceptionC(nn.Module):
    def __init__(self):
        super().__init__()
        self.branch0 = ConvNormAct(1536, 256, 1)
        self.branch1_0 = ConvNormAct(1536, 384, 1)
        self.branch1_1a = ConvNormAct(384, 256, (1, 3), padding=(0, 1))
        self.branch1_1b = ConvNormAct(384, 256, (3, 1), padding=(1, 0))
        self.branch2_0 = ConvNormAct(1536, 384, 1)
        self.branch2_1 = ConvNormAct(384, 448, (3, 1), padding=(1, 0))
        self.branch2_2 = ConvNormAct(448, 512, (1, 3), padding=(0, 1))
        self.branch2_3a = ConvNormAct(512, 256, (1, 3), padding=(0, 1))
        self.branch2_3b = ConvNormAct(512, 256, (3, 1), padding=(1, 0))
        self.branch3 = nn.Sequential(nn.AvgPool2d(3, stride=1, padding=1, count_include_pad=False), ConvNormAct(1536, 256, 1))

    def forward(self, x):
        x1 = self.branch1_0(x)
        x2 = self.branch2_2(self.branch2_1(self.branch2_0(x)))
        return torch.cat((self.branch0(x), self.branch1_1a(x1), self.branch1_1b(x1), self.branch2_3a(x2), self.branch2_3b(x2), self.branch3(x)), 1)


class InceptionV4Features(nn.Module):
    """inception_v4(num_classes=0): features, then the global average pool -> [N,1536]"""

    def __init__(self):
        super().__init__()
        self.features = nn.Sequential(ConvNormAct(3, 32, 3, 2), ConvNormAct(32, 32, 3), ConvNormAct(32, 64, 3, padding=1), Mixed3a(), Mixed4a(),
                                      Mixed5a(), *(InceptionA() for _ in range(4)), ReductionA(), *(InceptionB() for _ in range(7)),
                                      ReductionB(), *(InceptionC() for _ in range(3)))

    def forward(self, x, endpoints=None):
        for i, m in enumerate(self.features):
            x = m(x)
            if endpoints is not None:
                endpoints[f"features.{i}"] = x
        return x.mean((2, 3))


def build(sd):
    """the network in eval mode with `sd` loaded strictly"""
    net = InceptionV4Features().eval()
    net.load_state_dict(sd, strict=True)
    return net


def units(net):
    """[(dotted name, ConvNormAct)] in the network's order"""
    return [(n, m) for n, m in net.named_modules() if isinstance(m, ConvNormAct)]


def fold_batchnorm(net, folded):
    """replace every conv + BatchNorm of `net` by a biased convolution; folded(name) -> (weight, bias)"""
    for name, unit in units(net):
        parent = net
        *path, leaf = name.split(".")
        for p in path:
            parent = getattr(parent, p)
        w, b = folded(name)
        setattr(parent, leaf, FoldedConvAct(unit, w.float(), b.float()))
    return net


def preprocess(frames, channel_order="rgb", size=(299, 299)):
    """uint8 [F,H,W,3] or fp32 [F,3,H,W] frames in [0,1] -> fp32 [F,3,*size]: k / 255, Resize on a float tensor (bilinear, antialias),
    Normalize.  'bgr': the network sees B, G, R planes; the mean and std stay in their own order, as in the reference."""
    x = frames.permute(0, 3, 1, 2).float() / 255.0 if frames.dtype == torch.uint8 else frames.float()
    if channel_order == "bgr":
        x = x.flip(1)
    x = F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=True)
    return (x - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)


@torch.no_grad()
def features(net, frames, channel_order="rgb", endpoints=None):
    return net(preprocess(frames, channel_order), endpoints)


def aggregate(features1, features2, batch_size, n_frames, video_setting):
    """what calculate_latent_mse.py:56-79 does with the two [B*T,C] feature arrays, spelled out per timestamp in float64: the squared
    differences of all B videos and C features at timestamp t, their mean (`value`) and population standard deviation (`value_std`), and
    the mean of the per-timestamp means (`value_mean`)"""
    a = np.asarray(features1, dtype=np.float64).reshape(batch_size, n_frames, -1)
    b = np.asarray(features2, dtype=np.float64).reshape(batch_size, n_frames, -1)
    value, value_std = {}, {}
    for t in range(n_frames):
        d2 = ((a[:, t] - b[:, t]) ** 2).ravel()
        m = d2.sum() / d2.size
        value[t] = float(m)
        value_std[t] = float(np.sqrt(((d2 - m) ** 2).sum() / d2.size))
    return {"value": value, "value_mean": float(sum(value.values()) / n_frames), "value_std": value_std, "video_setting": video_setting,
            "video_setting_name": "time, channel, heigth, width"}
