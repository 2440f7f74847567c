"""FVD (the styleganv method) on the device, from I3D weights the user supplies: the counterpart of the reference's
evoworld/metrics/calculate_all_metrics.py calculate_fvd_batch with evoworld/metrics/fvd/styleganv/fvd.py (preprocess_single, get_fvd_feats,
frechet_distance), over the network evoworld/metrics/fvd/videogpt/pytorch_i3d.py defines: InceptionI3d(400, in_channels=3), Inception-v1
inflated to 3-D, whose 400 Kinetics logits are the features.

ops.video_preprocess resizes, crops and maps a clip to [-1,1]; the 57 BatchNorm-folded convolutions run on ops.gemm (dense mode, bias
vector, writing straight into their module's concat) over the patch rows of ops.im2col3d; ops.maxpool3d_relu (csrc/convnet.hip) and
ops.i3d_head (csrc/i3d.hip) do the rest; the loader, packer and constructors are _convnet's.  Conv outputs stay pre-ReLU in memory: every
reader applies max(x, 0) itself.  One clip goes through the network per call, so its logits do not depend on what else is evaluated.  Patch rows are written in slabs of output frames of at most WORKSPACE_BYTES.
The Frechet distance is the reference's float64 numpy / scipy arithmetic on the host.  This project ships no weights.
"""
import math
import zipfile

import numpy as np
import torch

from ._convnet import K_ALIGN, ConvNet, fold_batchnorm, pack_conv, random_conv_bn, validate  # noqa: F401 (K_ALIGN: this module's name too)
from ._convnet import load_state_files as _load_state_files

SIDE = 224                                             # preprocess_single's resolution
WORKSPACE_BYTES = 256 << 20                            # cap on the patch rows alive at once (the stem's at T = 25 would be 0.9 GB)
MIN_FRAMES = 9                                         # fewer frames leave Mixed_5c a single frame: the (2,7,7) average pool has no window
BN_EPS = 1e-5
N_CLASSES = 400

# (name, in channels, out channels, kernel, stride) of the stem's convolutions; ("pool", kernel, stride) between them
STEM = (("Conv3d_1a_7x7", 3, 64, 7, 2), ("MaxPool3d_2a_3x3", (1, 3, 3), (1, 2, 2)), ("Conv3d_2b_1x1", 64, 64, 1, 1),
        ("Conv3d_2c_3x3", 64, 192, 3, 1), ("MaxPool3d_3a_3x3", (1, 3, 3), (1, 2, 2)))
# Inception modules: (name, in channels, (b0, b1a, b1b, b2a, b2b, b3b) out channels); pools ("name", kernel, stride) between them
MIXED = (("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
         ("MaxPool3d_4a_3x3", (3, 3, 3), (2, 2, 2)),
         ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
         ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
         ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)),
         ("MaxPool3d_5a_2x2", (2, 2, 2), (2, 2, 2)),
         ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)), ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)))
ENDPOINTS = tuple(e[0] for e in STEM + MIXED)
ACCEPTED = ("a state dict in InceptionI3d's key layout (Conv3d_1a_7x7.conv3d.weight, Conv3d_1a_7x7.bn.{weight,bias,running_mean,running_var}, "
            "Mixed_3b.b0.conv3d.weight, ..., logits.conv3d.{weight,bias}; e.g. the i3d_pretrained_400.pt of the videogpt method), as "
            ".safetensors or a checkpoint torch.load(weights_only=True) reads")


def units():
    """[(name, c_in, c_out, kernel)] of the 57 conv + BatchNorm + ReLU units, in the network's order"""
    out = [(e[0], e[1], e[2], e[3]) for e in STEM if len(e) == 5]
    for e in MIXED:
        if isinstance(e[1], tuple):
            continue
        name, ci, (c0, c1a, c1b, c2a, c2b, c3) = e
        out += [(f"{name}.b0", ci, c0, 1), (f"{name}.b1a", ci, c1a, 1), (f"{name}.b1b", c1a, c1b, 3), (f"{name}.b2a", ci, c2a, 1),
                (f"{name}.b2b", c2a, c2b, 3), (f"{name}.b3b", ci, c3, 1)]
    return out


def same_pad(size, k, s):
    """TensorFlow "SAME" along one axis as Unit3D / MaxPool3dSamePadding compute it per call: (output size, front pad, back pad) with
    output = ceil(size / s), total = max(k - s, 0) when s divides size, else max(k - size % s, 0); front = total // 2."""
    if size < 1 or k < 1 or s < 1:
        raise ValueError(f"same_pad: size, k, s = {size}, {k}, {s} must be positive")
    total = max(k - s, 0) if size % s == 0 else max(k - size % s, 0)
    return -(-size // s), total // 2, total - total // 2


def preprocess_geometry(H, W):
    """preprocess_single's sizes for H x W frames, in the reference's Python arithmetic: (resized height, resized width, crop row, crop
    column).  The shorter side goes to 224 (smaller frames are upsampled), the longer one to ceil(long * (224 / short))."""
    if H < 1 or W < 1:
        raise ValueError(f"preprocess_geometry: frames of {H} x {W}")
    scale = SIDE / min(H, W)
    hr, wr = (SIDE, math.ceil(W * scale)) if H < W else (math.ceil(H * scale), SIDE)
    return hr, wr, (hr - SIDE) // 2, (wr - SIDE) // 2


def _spec():
    spec = {}
    for name, ci, co, k in units():
        spec[f"{name}.conv3d.weight"] = (co, ci, k, k, k)
        for part in ("weight", "bias", "running_mean", "running_var"):
            spec[f"{name}.bn.{part}"] = (co,)
    spec["logits.conv3d.weight"] = (N_CLASSES, 1024, 1, 1, 1)
    spec["logits.conv3d.bias"] = (N_CLASSES,)
    return spec


def canonical_state_dict(sd):
    """An InceptionI3d state dict -> {key: fp32 CPU tensor} over exactly the keys the network has, validated (_convnet.validate).  A leading
    `module.` is stripped, num_batches_tracked and anything else is ignored.  KeyError lists the first missing keys; ValueError names a
    key of the wrong shape."""
    return validate(sd, _spec(), "I3D", ACCEPTED)


def pack_state_dict(sd):
    """State dict -> the tensors the kernels read, on the CPU.  Per unit: BatchNorm folded into the convolution in fp64 (s = gamma /
    sqrt(var + 1e-5); w * s; beta - mean * s), `{name}.w` fp16 [C_out, K padded to 64] with K ordered (dt, dy, dx, c_in) as ops.im2col3d
    writes its columns (the stem's 3 input channels padded to 8), `{name}.b` fp16 [C_out]; logits.w fp32 [400,1024], logits.b fp32 [400]."""
    c = canonical_state_dict(sd)
    packed = {}
    for name, ci, _, _ in units():
        w, b = fold_batchnorm(c, name, "conv3d", BN_EPS)
        packed[f"{name}.w"] = pack_conv(w, -(-ci // 8) * 8)
        packed[f"{name}.b"] = b.half().contiguous()
    packed["logits.w"] = c["logits.conv3d.weight"].reshape(N_CLASSES, 1024).contiguous()
    packed["logits.b"] = c["logits.conv3d.bias"].contiguous()
    return packed


def is_torchscript_archive(path):
    """True for a file torch.jit.save wrote: a zip whose entries include TorchScript's code/ folder or constants.pkl"""
    try:
        if not zipfile.is_zipfile(path):
            return False
        with zipfile.ZipFile(path) as z:
            return any("/code/" in n or n.endswith("constants.pkl") for n in z.namelist())
    except OSError:
        return False


def load_state_files(paths):
    """One or more weight files merged into one state dict (_convnet.load_state_files); a TorchScript archive is refused."""
    if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__"):
        paths = [paths]
    for p in paths:
        if not str(p).endswith(".safetensors") and is_torchscript_archive(p):
            raise ValueError(f"{p} is a TorchScript archive (such as styleganv's i3d_torchscript.pt): its parameters cannot be read as a "
                             f"state dict.  Accepted: {ACCEPTED}")
    return _load_state_files(paths)


def random_state_dict(seed=0):
    """A seeded InceptionI3d-layout state dict (timing and tests; the values mean nothing): every unit as _convnet.random_conv_bn draws it,
    logits weight N(0, 2 / 1024), logits bias N(0, 0.1^2).  Activations stay O(1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, ci, co, k in units():
        random_conv_bn(g, sd, name, "conv3d", (co, ci, k, k, k))
    sd["logits.conv3d.weight"] = torch.randn(N_CLASSES, 1024, 1, 1, 1, generator=g) * (2.0 / 1024) ** 0.5
    sd["logits.conv3d.bias"] = 0.1 * torch.randn(N_CLASSES, generator=g)
    return sd


class I3D(ConvNet):
    """InceptionI3d(400) in eval mode behind styleganv's preprocess_single, one clip per call, on the device.
    workspace_bytes caps the patch rows alive at once; every slab of output frames is one GEMM call, so the cap decides the GEMM shapes and
    is part of the result's definition: logits are bit-for-bit reproducible for a fixed cap, and equal up to summation order across caps."""
    pack_state_dict, load_state_files, random_state_dict = map(staticmethod, (pack_state_dict, load_state_files, random_state_dict))

    def __init__(self, packed, device, workspace_bytes=WORKSPACE_BYTES):
        super().__init__(packed, device)
        self.workspace_bytes = int(workspace_bytes)

    # ---- layers
    def _conv(self, x, targets, k, s, relu=True):
        """x [T,H,W,C] -> for every (unit name, out [To,Ho,Wo,ld], channel offset) of `targets` (units that share x, kernel and stride)
        the unit's pre-ReLU output into out[..., offset : offset + C_out].  The patch rows are written once per slab of output frames."""
        from . import ops
        T, H, W, _ = x.shape
        (To, pt, _), (Ho, ph, _), (Wo, pw, _) = same_pad(T, k, s), same_pad(H, k, s), same_pad(W, k, s)
        ldk = self.p[f"{targets[0][0]}.w"].shape[1]
        per_frame = Ho * Wo
        slab = max(1, self.workspace_bytes // (per_frame * ldk * 2))
        for o0 in range(0, To, slab):
            o1 = min(To, o0 + slab)
            first = o0 * s - pt                                                # input frame of the slab's first tap (negative: padding)
            lo, hi = max(0, first), min(T, (o1 - 1) * s - pt + k)
            rows = ops.im2col3d(x[lo:hi], (k, k, k), (s, s, s), (lo - first, ph, pw), (o1 - o0, Ho, Wo), ldk, relu)
            self.conv_into(rows.view(1, -1, ldk), [(self.p[f"{name}.w"], self.p[f"{name}.b"], out[o0:o1], c_off) for name, out, c_off in targets])
        return To, Ho, Wo

    def _unit(self, x, name, co, k, s, relu=True):
        sizes = [same_pad(n, k, s)[0] for n in x.shape[:3]]
        out = torch.empty(*sizes, co, dtype=torch.float16, device=x.device)
        self._conv(x, [(name, out, 0)], k, s, relu)
        return out

    @staticmethod
    def _pool(x, kernel, stride):
        from . import ops
        geo = [same_pad(n, k, s) for n, k, s in zip(x.shape[:3], kernel, stride)]
        return ops.maxpool3d_relu(x, kernel, stride, [g[1] for g in geo], [g[0] for g in geo])

    def _mixed(self, x, name, outs):
        c0, c1a, c1b, c2a, c2b, c3 = outs
        T, H, W, _ = x.shape
        y = torch.empty(T, H, W, c0 + c1b + c2b + c3, dtype=torch.float16, device=x.device)
        t1 = torch.empty(T, H, W, c1a, dtype=torch.float16, device=x.device)
        t2 = torch.empty(T, H, W, c2a, dtype=torch.float16, device=x.device)
        self._conv(x, [(f"{name}.b0", y, 0), (f"{name}.b1a", t1, 0), (f"{name}.b2a", t2, 0)], 1, 1)
        self._conv(t1, [(f"{name}.b1b", y, c0)], 3, 1)
        self._conv(t2, [(f"{name}.b2b", y, c0 + c1b)], 3, 1)
        self._conv(self._pool(x, (3, 3, 3), (1, 1, 1)), [(f"{name}.b3b", y, c0 + c1b + c2b)], 1, 1)
        return y

    # ---- the network
    def preprocess(self, clip, channel_order="rgb"):
        """clip uint8 [T,H,W,3] or fp32 [T,3,H,W] in [0,1] on the device (channels R, G, B) -> fp16 [T,224,224,8]: preprocess_single.
        channel_order 'bgr' hands the network B, G, R planes, as the reference's cv2.imread frames reach it."""
        from . import ops
        swap = self.check_channel_order(channel_order)
        return ops.video_preprocess(clip, *preprocess_geometry(*self.frames_hw(clip, "clip", "T")), swap_rb=swap)

    def forward(self, x, n_frames=None, endpoints=None):
        """x = preprocess(...) -> the 400 logits, fp32, of its first n_frames frames (all by default).  `endpoints`: a dict that receives
        every endpoint's tensor, fp16 [T,H,W,C]: pre-ReLU for the convolutions and modules, the pooled values for the pools."""
        from . import ops
        T = x.shape[0] if n_frames is None else int(n_frames)
        if not MIN_FRAMES <= T <= x.shape[0]:
            raise ValueError(f"I3D needs {MIN_FRAMES} <= n_frames <= the clip's {x.shape[0]} frames, got {T}")
        x = x[:T]
        keep = (lambda n, t: endpoints.__setitem__(n, t)) if endpoints is not None else (lambda n, t: None)
        for e in STEM:
            x = self._unit(x, e[0], e[2], e[3], e[4], relu=e[0] != "Conv3d_1a_7x7") if len(e) == 5 else self._pool(x, e[1], e[2])
            keep(e[0], x)
        for e in MIXED:
            x = self._pool(x, e[1], e[2]) if isinstance(e[1], tuple) else self._mixed(x, e[0], e[2])
            keep(e[0], x)
        return ops.i3d_head(x, self.p["logits.w"], self.p["logits.b"])

    def logits(self, clip, n_frames=None, channel_order="rgb"):
        """The features FVD compares: InceptionI3d's 400 logits of the clip's first n_frames frames, fp32 [400] on the device."""
        from . import ops
        clip = clip if n_frames is None else clip[:int(n_frames)]
        out = self.forward(self.preprocess(clip.contiguous(), channel_order))
        ops.streamk_check()                        # results leave here: a timed-out stream-K hand-over in a convolution must not pass silently
        return out

    def endpoints(self, clip, n_frames=None, channel_order="rgb"):
        """{endpoint name: fp16 [T,H,W,C]} plus 'Logits' (fp32 [400]), for tests"""
        from . import ops
        eps = {}
        clip = clip if n_frames is None else clip[:int(n_frames)]
        eps["Logits"] = self.forward(self.preprocess(clip.contiguous(), channel_order), endpoints=eps)
        ops.streamk_check()
        return eps


def frechet_distance(feats_fake, feats_real):
    """frechet_distance of styleganv/fvd.py on the host in float64: [N,d] features each -> float.  With N = 1 only the squared distance
    of the means, as there."""
    from scipy.linalg import sqrtm
    a, b = (np.asarray(f.cpu() if isinstance(f, torch.Tensor) else f, dtype=np.float64) for f in (feats_fake, feats_real))
    mu_a, mu_b = a.mean(axis=0), b.mean(axis=0)
    m = np.square(mu_a - mu_b).sum()
    if a.shape[0] > 1:
        sigma_a, sigma_b = np.cov(a, rowvar=False), np.cov(b, rowvar=False)
        s, _ = sqrtm(np.dot(sigma_a, sigma_b), disp=False)
        return float(np.real(m + np.trace(sigma_a + sigma_b - s * 2)))
    return float(np.real(m))


def fvd_result(feats1, feats2, video_setting):
    """{clip length: [N,400] features} of both sets -> calculate_fvd_batch's result dict; videos1 (the ground truth) goes first into
    frechet_distance, as in the reference"""
    value = {L: frechet_distance(feats1[L], feats2[L]) for L in sorted(feats1)}
    return {"value": value, "value_mean": float(np.mean(list(value.values()))), "fvd_setting": "styleganv", "video_setting": video_setting,
            "video_setting_name": "batch_size, channel, time, height, width"}


def clip_features(model, clip, channel_order="rgb", first=10):
    """{L: fp64 numpy [400]} for every clip length L = first..T: the clip is preprocessed once, each length is one pass"""
    from . import ops
    x = model.preprocess(clip.contiguous(), channel_order)
    out = {L: model.forward(x, L) for L in range(first, x.shape[0] + 1)}
    ops.streamk_check()                            # results leave here
    return {L: v.double().cpu().numpy() for L, v in out.items()}


def calculate_fvd(videos1, videos2, model, channel_order="rgb"):
    """calculate_fvd_batch(videos1, videos2, device, method="styleganv") of calculate_all_metrics.py: [B,T,3,H,W] in [0,1] -> the
    reference's result dict, the distance at every clip length from 10 to T, with `model` an evoworld_amd.fvd.I3D."""
    if videos1.shape != videos2.shape:
        raise AssertionError(f"video shapes differ: {tuple(videos1.shape)} vs {tuple(videos2.shape)}")
    if videos1.ndim != 5 or videos1.shape[2] != 3:
        raise ValueError(f"videos: expected [B,T,3,H,W], got {tuple(videos1.shape)}")
    B, T, C, H, W = videos1.shape
    feats = ({}, {})
    for f, videos in zip(feats, (videos1, videos2)):
        for v in videos:
            for L, x in clip_features(model, v.to(model.device, torch.float32), channel_order).items():
                f.setdefault(L, []).append(x)
    return fvd_result(*({L: np.stack(v) for L, v in f.items()} for f in feats), torch.Size([B, C, T, H, W]))
