"""Latent MSE and loop-closure latent MSE on the device, from Inception-v4 weights the user supplies: the counterpart of the reference's
evoworld/metrics/other_metrics/calculate_latent_mse.py:11-79 (run by calculate_all_metrics.py:220-221), i.e. the mean squared difference of
the 1536 pooled features of timm's `inception_v4` (pretrained, num_classes=0, eval mode) on frames resized to 299 x 299 and normalised with
the ImageNet mean and std.  Despite the metric's name no VAE is involved.

ops.frames_resize_aa_norm resizes and normalises; the 149 BatchNorm-folded convolutions run on ops.gemm (dense mode, bias vector, writing
straight into their module's concat) over the patch rows of ops.im2col3d with kt = 1; ops.maxpool3d_relu, ops.avgpool3x3_relu and
ops.global_avgpool_relu do the rest (csrc/convnet.hip, csrc/inception.hip); the loader, packer and constructors are _convnet's.  Conv
outputs stay pre-ReLU in memory: every reader applies max(x, 0) itself.  Every frame goes through the GEMMs on its own (M = one frame's pixels), so a frame's features depend on that frame alone:
identical frames give exactly 0, and the loop-closure value reuses the last frame's features of the same pass.  The aggregation is the
reference's numpy arithmetic on the host, in float64.  This project ships no weights.
"""
import functools

import numpy as np
import torch

from ._convnet import K_ALIGN, ConvNet, load_state_files, pack_conv, random_conv_bn, validate  # noqa: F401 (K_ALIGN, load_state_files: this module's names too)
from ._convnet import fold_batchnorm as _fold_batchnorm

SIDE = 299                                             # Resize((299, 299))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BN_EPS = 1e-3                                          # timm's inception_v4 BatchNorm
N_FEATURES = 1536
ACCEPTED = ("a state dict in timm inception_v4's key layout (features.0.conv.weight, features.0.bn.{weight,bias,running_mean,running_var}, "
            "..., features.21.branch3.1.bn.running_var; last_linear.* is ignored), as .safetensors or a checkpoint "
            "torch.load(weights_only=True) reads")
MAXPOOL, AVGPOOL = ("maxpool",), ("avgpool",)          # MaxPool2d(3, 2) / AvgPool2d(3, 1, 1, count_include_pad=False)


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def U(ci, co, k, s=1, p=0):
    """conv (no bias) + BatchNorm + ReLU: ("conv", in channels, out channels, (kh, kw), stride, (ph, pw))"""
    return ("conv", ci, co, _pair(k), s, _pair(p))


# A module is a list of steps (key under features.{i}, source, op): source None is the module's input, else an earlier step's key.  The
# outputs no later step reads are concatenated over the channels in step order.
_INCEPTION_A = [("branch0", None, U(384, 96, 1)),
                ("branch1.0", None, U(384, 64, 1)), ("branch1.1", "branch1.0", U(64, 96, 3, 1, 1)),
                ("branch2.0", None, U(384, 64, 1)), ("branch2.1", "branch2.0", U(64, 96, 3, 1, 1)), ("branch2.2", "branch2.1", U(96, 96, 3, 1, 1)),
                ("branch3.0", None, AVGPOOL), ("branch3.1", "branch3.0", U(384, 96, 1))]
_REDUCTION_A = [("branch0", None, U(384, 384, 3, 2)),
                ("branch1.0", None, U(384, 192, 1)), ("branch1.1", "branch1.0", U(192, 224, 3, 1, 1)), ("branch1.2", "branch1.1", U(224, 256, 3, 2)),
                ("branch2", None, MAXPOOL)]
_INCEPTION_B = [("branch0", None, U(1024, 384, 1)),
                ("branch1.0", None, U(1024, 192, 1)), ("branch1.1", "branch1.0", U(192, 224, (1, 7), 1, (0, 3))),
                ("branch1.2", "branch1.1", U(224, 256, (7, 1), 1, (3, 0))),
                ("branch2.0", None, U(1024, 192, 1)), ("branch2.1", "branch2.0", U(192, 192, (7, 1), 1, (3, 0))),
                ("branch2.2", "branch2.1", U(192, 224, (1, 7), 1, (0, 3))), ("branch2.3", "branch2.2", U(224, 224, (7, 1), 1, (3, 0))),
                ("branch2.4", "branch2.3", U(224, 256, (1, 7), 1, (0, 3))),
                ("branch3.0", None, AVGPOOL), ("branch3.1", "branch3.0", U(1024, 128, 1))]
_REDUCTION_B = [("branch0.0", None, U(1024, 192, 1)), ("branch0.1", "branch0.0", U(192, 192, 3, 2)),
                ("branch1.0", None, U(1024, 256, 1)), ("branch1.1", "branch1.0", U(256, 256, (1, 7), 1, (0, 3))),
                ("branch1.2", "branch1.1", U(256, 320, (7, 1), 1, (3, 0))), ("branch1.3", "branch1.2", U(320, 320, 3, 2)),
                ("branch2", None, MAXPOOL)]
_INCEPTION_C = [("branch0", None, U(1536, 256, 1)),
                ("branch1_0", None, U(1536, 384, 1)), ("branch1_1a", "branch1_0", U(384, 256, (1, 3), 1, (0, 1))),
                ("branch1_1b", "branch1_0", U(384, 256, (3, 1), 1, (1, 0))),
                ("branch2_0", None, U(1536, 384, 1)), ("branch2_1", "branch2_0", U(384, 448, (3, 1), 1, (1, 0))),
                ("branch2_2", "branch2_1", U(448, 512, (1, 3), 1, (0, 1))), ("branch2_3a", "branch2_2", U(512, 256, (1, 3), 1, (0, 1))),
                ("branch2_3b", "branch2_2", U(512, 256, (3, 1), 1, (1, 0))),
                ("branch3.0", None, AVGPOOL), ("branch3.1", "branch3.0", U(1536, 256, 1))]
FEATURES = (
    [("", None, U(3, 32, 3, 2))], [("", None, U(32, 32, 3))], [("", None, U(32, 64, 3, 1, 1))],
    [("maxpool", None, MAXPOOL), ("conv", None, U(64, 96, 3, 2))],                                                         # Mixed3a
    [("branch0.0", None, U(160, 64, 1)), ("branch0.1", "branch0.0", U(64, 96, 3)),                                         # Mixed4a
     ("branch1.0", None, U(160, 64, 1)), ("branch1.1", "branch1.0", U(64, 64, (1, 7), 1, (0, 3))),
     ("branch1.2", "branch1.1", U(64, 64, (7, 1), 1, (3, 0))), ("branch1.3", "branch1.2", U(64, 96, 3))],
    [("conv", None, U(192, 192, 3, 2)), ("maxpool", None, MAXPOOL)],                                                       # Mixed5a
    *([_INCEPTION_A] * 4), _REDUCTION_A, *([_INCEPTION_B] * 7), _REDUCTION_B, *([_INCEPTION_C] * 3))


def _name(i, key):
    return f"features.{i}.{key}" if key else f"features.{i}"


def units():
    """[(name, c_in, c_out, (kh, kw), stride, (ph, pw))] of the 149 conv + BatchNorm + ReLU units, in the network's order"""
    return [(_name(i, key), *op[1:]) for i, steps in enumerate(FEATURES) for key, _, op in steps if op[0] == "conv"]


def _out_hw(h, w, op):
    """(h, w) after one step's window; ValueError where it does not fit"""
    if op is AVGPOOL:
        return h, w
    (kh, kw), s, (ph, pw) = ((3, 3), 2, (0, 0)) if op is MAXPOOL else op[3:]
    ho, wo = (h + 2 * ph - kh) // s + 1, (w + 2 * pw - kw) // s + 1
    if ho < 1 or wo < 1:
        raise ValueError(f"a {kh} x {kw} window (stride {s}, pad {ph}, {pw}) does not fit {h} x {w}")
    return ho, wo


def module_shapes(i, h, w, c):
    """features.{i} on an h x w x c input -> ({key: (h, w, c) of every step}, [keys that are concatenated], (h, w, c) of the module)"""
    steps = FEATURES[i]
    read = {src for _, src, _ in steps if src is not None}
    shapes = {None: (h, w, c)}
    for key, src, op in steps:
        sh, sw, sc = shapes[src]
        if op[0] == "conv" and op[1] != sc:
            raise ValueError(f"{_name(i, key)} takes {op[1]} channels, its input has {sc}")
        shapes[key] = (*_out_hw(sh, sw, op), op[2] if op[0] == "conv" else sc)
    finals = [key for key, _, _ in steps if key not in read]
    sizes = {shapes[k][:2] for k in finals}
    if len(sizes) != 1:
        raise ValueError(f"features.{i}: the concatenated branches differ in size: {sorted(sizes)}")
    return shapes, finals, (*sizes.pop(), sum(shapes[k][2] for k in finals))


def stage_shapes(side=SIDE):
    """[(h, w, c)] of the 22 features.{i} outputs for side x side input frames"""
    out, shape = [], (side, side, 3)
    for i in range(len(FEATURES)):
        shape = module_shapes(i, *shape)[2]
        out.append(shape)
    return out


def _spec():
    spec = {}
    for name, ci, co, (kh, kw), _, _ in units():
        spec[f"{name}.conv.weight"] = (co, ci, kh, kw)
        for part in ("weight", "bias", "running_mean", "running_var"):
            spec[f"{name}.bn.{part}"] = (co,)
    return spec


def canonical_state_dict(sd):
    """A timm inception_v4 state dict -> {key: fp32 CPU tensor} over exactly the keys the feature network has, validated
    (_convnet.validate).  A leading `module.` is stripped; num_batches_tracked, last_linear.* and anything else is ignored.  KeyError lists
    the first missing keys; ValueError names a key of the wrong shape."""
    return validate(sd, _spec(), "Inception-v4", ACCEPTED)


def fold_batchnorm(c, name):
    """(weight [C_out, C_in, kh, kw], bias [C_out]) in fp64 of unit `name` with its eval-mode BatchNorm (eps 1e-3) folded in"""
    return _fold_batchnorm(c, name, "conv", BN_EPS)


def pack_state_dict(sd):
    """State dict -> the tensors the kernels read, on the CPU.  Per unit: BatchNorm folded in fp64 (fold_batchnorm), `{name}.w` fp16
    [C_out, K padded to 64] with K ordered (dy, dx, c_in) as ops.im2col3d writes its columns (the stem's 3 input channels padded to 8),
    `{name}.b` fp16 [C_out]."""
    c = canonical_state_dict(sd)
    packed = {}
    for name, ci, *_rest in units():
        w, b = fold_batchnorm(c, name)
        packed[f"{name}.w"] = pack_conv(w, -(-ci // 8) * 8)
        packed[f"{name}.b"] = b.half().contiguous()
    return packed


def random_state_dict(seed=0):
    """A seeded inception_v4-layout state dict (timing and tests; the values mean nothing): every unit as _convnet.random_conv_bn draws it,
    plus num_batches_tracked as timm's file has it (the loader ignores it).  Activations stay O(1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, ci, co, (kh, kw), _, _ in units():
        random_conv_bn(g, sd, name, "conv", (co, ci, kh, kw))
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(0)
    return sd


@functools.lru_cache(maxsize=None)
def resize_table(n_in, n_out):
    """One axis of F.interpolate(mode="bilinear", align_corners=False, antialias=True) from n_in to n_out samples, in float32 as torch
    computes it: (first int32 [n_out], count int32 [n_out], weights fp32 [n_out, taps]) numpy arrays, rows zero-padded.  Per output
    index i: scale = n_in / n_out, support = max(scale, 1), center = scale * (i + 0.5), first = max(int(center - support + 0.5), 0),
    end = min(int(center + support + 0.5), n_in), w_j = max(0, 1 - |(j - center + 0.5) * (1 / max(scale, 1))|) for j in [first, end), divided
    by their sum (added in order).  The reciprocal is rounded before the product, as in torch: with the kernel's fma chains these tables
    reproduce F.interpolate bit for bit on an x86 host.  With antialias an upscale is not plain bilinear either: every size goes through
    this table."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_table: n_in, n_out = {n_in}, {n_out} must be positive")
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    support = max(scale, f32(1.0))
    inv = f32(1.0) / scale if scale >= 1 else f32(1.0)
    first, rows = np.zeros(n_out, np.int32), []
    for i in range(n_out):
        center = scale * (f32(i) + f32(0.5))
        lo = max(int(center - support + f32(0.5)), 0)
        hi = min(int(center + support + f32(0.5)), n_in)
        j = np.arange(lo, hi, dtype=np.float32)
        w = np.maximum(f32(0.0), f32(1.0) - np.abs((j - center + f32(0.5)) * inv)).astype(np.float32)
        total = f32(0.0)
        for v in w:                                    # torch adds the weights one after the other
            total = f32(total + v)
        first[i] = lo
        rows.append(w / total)
    count = np.array([len(r) for r in rows], np.int32)
    weights = np.zeros((n_out, int(count.max())), np.float32)
    for i, r in enumerate(rows):
        weights[i, :len(r)] = r
    for a in (first, count, weights):
        a.setflags(write=False)
    return first, count, weights


def latent_mse_result(f1, f2, video_setting):
    """calculate_latent_mse.py:56-79 from the features: f1, f2 [B,T,1536] -> the reference's result dict, in numpy float64"""
    f1, f2 = (np.asarray(f.cpu() if isinstance(f, torch.Tensor) else f, dtype=np.float64) for f in (f1, f2))
    if f1.shape != f2.shape or f1.ndim != 3:
        raise ValueError(f"features: expected two [B,T,C] arrays of one shape, got {f1.shape} and {f2.shape}")
    d2 = (f1 - f2) ** 2
    mse_result, std_result = np.mean(d2, axis=(0, 2)), np.std(d2, axis=(0, 2))
    return {"value": {t: mse_result[t].tolist() for t in range(len(mse_result))},
            "value_mean": float(np.mean(mse_result)),
            "value_std": {t: std_result[t].tolist() for t in range(len(std_result))},
            "video_setting": video_setting,
            "video_setting_name": "time, channel, heigth, width"}


class InceptionV4(ConvNet):
    """timm's inception_v4 (num_classes=0, eval mode) behind Resize((299, 299)) + Normalize, on the device: frames -> 1536 features each.
    `chunk` frames share the gathers and pools of one pass; the GEMMs run frame by frame."""
    pack_state_dict, load_state_files, random_state_dict = map(staticmethod, (pack_state_dict, load_state_files, random_state_dict))

    def __init__(self, packed, device, chunk=5):
        super().__init__(packed, device)
        self.chunk = int(chunk)
        self._tables = {}

    # ---- layers
    def _table(self, n_in, n_out):
        key = (n_in, n_out)
        if key not in self._tables:
            self._tables[key] = tuple(torch.from_numpy(np.array(a)).to(self.device) for a in resize_table(n_in, n_out))
        return self._tables[key]

    def _module(self, i, x, relu=True):
        """features.{i} of x fp16 [n,H,W,C] -> [n,H',W',C'], the convolutions' part pre-ReLU.  Units that read the same tensor through the
        same window share one patch-row gather; the GEMMs write into the concat, the pooled branches are copied into their slice."""
        from . import ops
        n, H, W, C = x.shape
        steps = FEATURES[i]
        shapes, finals, (Ho, Wo, Co) = module_shapes(i, H, W, 3 if i == 0 else C)          # the frames' 3 channels arrive padded to 8
        y = torch.empty(n, Ho, Wo, Co, dtype=torch.float16, device=x.device)
        offset, off = {}, 0
        for k in finals:
            offset[k] = off
            off += shapes[k][2]
        vals, done = {None: x}, set()
        for key, src, op in steps:
            if key in done:
                continue
            h, w, c = shapes[key]
            if op[0] != "conv":
                t = ops.maxpool3d_relu(vals[src], (1, 3, 3), (1, 2, 2), (0, 0, 0), (n, h, w)) if op is MAXPOOL else ops.avgpool3x3_relu(vals[src])
                if key in offset:
                    y[..., offset[key]:offset[key] + c].copy_(t)
                else:
                    vals[key] = t
                done.add(key)
                continue
            _, _, _, (kh, kw), s, (ph, pw) = op
            group = [(k2, o2) for k2, s2, o2 in steps if s2 == src and o2[0] == "conv" and o2[3:] == op[3:] and k2 not in done]
            ldk = self.p[f"{_name(i, key)}.w"].shape[1]
            rows = ops.im2col3d(vals[src], (1, kh, kw), (1, s, s), (0, ph, pw), (n, h, w), ldk, relu).view(n, h * w, ldk)
            targets = []
            for k2, o2 in group:
                name = _name(i, k2)
                if k2 in offset:
                    out, c_off = y, offset[k2]
                else:
                    out, c_off = torch.empty(n, h, w, o2[2], dtype=torch.float16, device=x.device), 0
                    vals[k2] = out
                targets.append((self.p[f"{name}.w"], self.p[f"{name}.b"], out, c_off))
                done.add(k2)
            self.conv_into(rows, targets)              # one frame per GEMM: its values do not depend on the rest of the batch
        return y

    # ---- the network
    def preprocess(self, frames, channel_order="rgb"):
        """frames uint8 [F,H,W,3] or fp32 [F,3,H,W] in [0,1] on the device (channels R, G, B) -> fp16 [F,299,299,8]: the reference's
        transform.  channel_order 'bgr' hands the network B, G, R planes, as the reference's cv2.imread frames reach it; the ImageNet
        mean and std stay indexed by the network's channel."""
        from . import ops
        swap = self.check_channel_order(channel_order)
        H, W = self.frames_hw(frames)
        return ops.frames_resize_aa_norm(frames, self._table(H, SIDE), self._table(W, SIDE), MEAN, STD, swap)

    def forward(self, x, endpoints=None):
        """x = preprocess(...) -> fp32 [F,1536].  `endpoints`: a dict that receives every features.{i} output, fp16 [F,h,w,C] (the
        convolutions' channels pre-ReLU, the pooled ones as they are)."""
        from . import ops
        for i in range(len(FEATURES)):
            x = self._module(i, x, relu=i > 0)
            if endpoints is not None:
                endpoints[f"features.{i}"] = x
        return ops.global_avgpool_relu(x)

    def features(self, frames, channel_order="rgb", endpoints=None):
        """The features the metric compares: fp32 [F,1536] on the device, `chunk` frames per pass"""
        from . import ops
        frames = frames.contiguous()
        out, eps = [], []
        for f0 in range(0, frames.shape[0], max(1, self.chunk)):
            e = {} if endpoints is not None else None
            out.append(self.forward(self.preprocess(frames[f0:f0 + max(1, self.chunk)], channel_order), e))
            eps.append(e)
        if endpoints is not None:
            endpoints.update({k: torch.cat([e[k] for e in eps]) for k in eps[0]})
        ops.streamk_check()                        # results leave here: a timed-out stream-K hand-over in a convolution must not pass silently
        return torch.cat(out) if out else torch.empty(0, N_FEATURES, dtype=torch.float32, device=frames.device)


def calculate_latent_mse(videos1, videos2, model, channel_order="rgb"):
    """calculate_latent_mse(image1_tensor, image2_tensor) of calculate_latent_mse.py:34-79: [B,T,3,H,W] in [0,1] -> the reference's result
    dict, with `model` an evoworld_amd.latent_mse.InceptionV4.  The loop-closure value is this function on videos[:, -1:]."""
    if videos1.shape != videos2.shape:
        raise AssertionError(f"video shapes differ: {tuple(videos1.shape)} vs {tuple(videos2.shape)}")
    if videos1.ndim != 5 or videos1.shape[2] != 3:
        raise ValueError(f"videos: expected [B,T,3,H,W], got {tuple(videos1.shape)}")
    B, T, C, H, W = videos1.shape
    f1, f2 = (model.features(v.reshape(B * T, C, H, W).to(model.device, torch.float32), channel_order).cpu().view(B, T, N_FEATURES)
              for v in (videos1, videos2))
    return latent_mse_result(f1, f2, torch.Size([B * T, C, SIDE, SIDE]))
