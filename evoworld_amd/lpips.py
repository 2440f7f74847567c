"""LPIPS with the AlexNet backbone on the device, from weights the user supplies: the counterpart of the reference's
evoworld/metrics/other_metrics/calculate_lpips.py (run by calculate_all_metrics.py:195-221), i.e. per frame pair
lpips.LPIPS(net='alex', spatial=True).forward(img1, img2).mean() on frames mapped from [0,1] to [-1,1].

The five convolutions run on ops.gemm (dense mode, bias vector) over the patch rows of ops.im2col_frames (the first, csrc/lpips.hip) and
ops.im2col3d with kt = 1; ops.maxpool3d_relu (csrc/convnet.hip) and ops.lpips_head (csrc/lpips.hip) do the rest; the loader, packer and
constructors are _convnet's.  Conv outputs stay pre-ReLU in memory: every reader applies max(x, 0) itself.  The mean
over the bilinearly upsampled distance map is a weighted sum over the tap's own pixels (upsample_mean_weights), so no full-size map
exists.  This project ships no weights: they come from a lpips.LPIPS state dict, or from torchvision's AlexNet plus the lpips
package's alex.pth.
"""
import numpy as np
import torch

from ._convnet import K_ALIGN, ConvNet, load_state_files, pack_conv, validate  # noqa: F401 (K_ALIGN, load_state_files: this module's names too)

# (torchvision features index, out channels, in channels, kernel, stride, padding); a tap follows each convolution's ReLU
CONVS = ((0, 64, 3, 11, 4, 2), (3, 192, 64, 5, 1, 2), (6, 384, 192, 3, 1, 1), (8, 256, 384, 3, 1, 1), (10, 256, 256, 3, 1, 1))
POOL_AFTER = (True, True, False, False, False)         # MaxPool2d(3, 2) between conv1 / conv2 and conv2 / conv3
SHIFT = (-.030, -.088, -.188)                          # lpips ScalingLayer
SCALE = (.458, .448, .450)
MIN_SIZE = 31                                          # smallest H, W that leave every tap at least 1 x 1


def upsample_mean_weights(n_in, n_out, out_weights=None):
    """float64 [n_in]: how often F.interpolate(size=n_out, mode='bilinear', align_corners=False) counts each of n_in input samples
    along one axis, so that mean(upsample(m)) = sum_yx wy[y] wx[x] m[y,x] / (H W).  torch's index arithmetic:
    src = max(0, (i + 0.5) * n_in / n_out - 0.5), i0 = floor(src), i1 = min(i0 + 1, n_in - 1).  The weights sum to n_out.
    out_weights (float64 [n_out], optional): output sample i counts out_weights[i] times instead of once, so that
    sum_i out_weights[i] upsample(m)[i] = sum_y w[y] m[y]; the weights then sum to sum(out_weights)."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"upsample_mean_weights: n_in, n_out = {n_in}, {n_out} must be positive")
    if out_weights is not None:
        out_weights = np.asarray(out_weights, dtype=np.float64)
        if out_weights.shape != (n_out,):
            raise ValueError(f"upsample_mean_weights: expected {n_out} output weights, got shape {out_weights.shape}")
    i = np.arange(n_out, dtype=np.float64)
    src = np.maximum(0.0, (i + 0.5) * (float(n_in) / float(n_out)) - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0
    w = np.zeros(n_in, dtype=np.float64)
    np.add.at(w, i0, (1.0 - l1) if out_weights is None else (1.0 - l1) * out_weights)
    np.add.at(w, i1, l1 if out_weights is None else l1 * out_weights)
    return w


def tap_sizes(H, W):
    """[(h, w)] of the five taps for H x W frames; ValueError when a tap would be empty."""
    if H < MIN_SIZE or W < MIN_SIZE:
        raise ValueError(f"LPIPS (AlexNet) needs frames of at least {MIN_SIZE} x {MIN_SIZE}: at {H} x {W} a feature map is empty")
    out, h, w = [], H, W
    for (_, _, _, k, s, p), pool in zip(CONVS, POOL_AFTER):
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out.append((h, w))
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return out


def canonical_state_dict(sd):
    """Either accepted key layout -> {conv{i}.weight, conv{i}.bias, lin{i} (i = 0..4), optional shift / scale}, validated.
    Layouts: a full lpips.LPIPS.state_dict() (net.slice{i+1}.{idx}.weight|bias, lin{i}.model.1.weight, optional scaling_layer.shift|scale;
    the duplicate lins.* entries are ignored), or torchvision AlexNet's features.{idx}.weight|bias merged with the lpips package's
    alex.pth (lin{i}.model.1.weight).  KeyError lists the first missing keys; ValueError names a key of the wrong shape."""
    source, spec = {}, {}                                  # canonical name -> the key it is read from (the alternatives where none is there)
    for i, (idx, co, ci, k, _, _) in enumerate(CONVS):
        for part, shape in (("weight", (co, ci, k, k)), ("bias", (co,))):
            names = (f"net.slice{i + 1}.{idx}.{part}", f"features.{idx}.{part}")
            source[f"conv{i}.{part}"] = next((n for n in names if n in sd), " | ".join(names))
            spec[source[f"conv{i}.{part}"]] = shape
        source[f"lin{i}"] = f"lin{i}.model.1.weight"
        spec[source[f"lin{i}"]] = (1, co, 1, 1)
    c = validate(sd, spec, "LPIPS")
    out = {k: c[n] for k, n in source.items()}
    for k in ("shift", "scale"):
        n = f"scaling_layer.{k}"
        if n in sd:
            if sd[n].numel() != 3:
                raise ValueError(f"{n}: expected shape (1, 3, 1, 1), got {tuple(sd[n].shape)}")
            out[k] = sd[n].detach().to("cpu", torch.float32)
    return out


def pack_state_dict(sd):
    """State dict (either layout) -> the tensors the kernels read, on the CPU: w{i} fp16 [C_out, K padded to 64] with K ordered
    (ky, kx, c_in) as ops.im2col_frames / ops.im2col3d write their columns (the first layer's 3 channels are not padded: K = 363 -> 384),
    b{i} fp16 [C_out], lin{i} fp32 [C_out], shift / scale (tuples of 3 floats)."""
    c = canonical_state_dict(sd)
    packed = {}
    for i, (_, co, *_rest) in enumerate(CONVS):
        packed[f"w{i}"] = pack_conv(c[f"conv{i}.weight"])
        packed[f"b{i}"] = c[f"conv{i}.bias"].half().contiguous()
        packed[f"lin{i}"] = c[f"lin{i}"].reshape(co).contiguous()
    packed["shift"] = tuple(float(v) for v in c["shift"].reshape(3)) if "shift" in c else SHIFT
    packed["scale"] = tuple(float(v) for v in c["scale"].reshape(3)) if "scale" in c else SCALE
    return packed


def random_state_dict(seed=0):
    """A seeded lpips.LPIPS-layout state dict with AlexNet's shapes: conv weights scaled by 1 / sqrt(fan-in) so activations stay
    O(1), biases N(0, 0.1^2), lin weights uniform in [0, 1) (non-negative, as the trained ones are)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, (idx, co, ci, k, _, _) in enumerate(CONVS):
        sd[f"net.slice{i + 1}.{idx}.weight"] = torch.randn(co, ci, k, k, generator=g) / float(ci * k * k) ** 0.5
        sd[f"net.slice{i + 1}.{idx}.bias"] = 0.1 * torch.randn(co, generator=g)
        sd[f"lin{i}.model.1.weight"] = torch.rand(1, co, 1, 1, generator=g)
    return sd


class LPIPSAlex(ConvNet):
    """lpips.LPIPS(net='alex', spatial=True) followed by the mean over the map, per frame pair, on the device."""
    pack_state_dict, load_state_files, random_state_dict = map(staticmethod, (pack_state_dict, load_state_files, random_state_dict))

    def __init__(self, packed, device, chunk=4):
        super().__init__(packed, device)
        self.chunk = int(chunk)                    # frame pairs whose activations are alive at once
        self.shift, self.scale = self.p["shift"], self.p["scale"]
        self.w, self.b, self.lin = ([self.p[f"{k}{i}"] for i in range(5)] for k in ("w", "b", "lin"))
        self._mean_w = {}

    def _weights_for(self, h, w, H, W):
        key = (h, w, H, W)
        if key not in self._mean_w:
            self._mean_w[key] = (torch.from_numpy(upsample_mean_weights(h, H)).to(self.device),
                                 torch.from_numpy(upsample_mean_weights(w, W)).to(self.device))
        return self._mean_w[key]

    def features(self, frames, channel_order="rgb"):
        """frames uint8 [n,H,W,3] or fp32 [n,3,H,W] in [0,1] -> the five pre-ReLU conv outputs, fp16 [n,h,w,C] each.  Every image goes
        through ew_gemm_f16 on its own, so its features do not depend on what else is in the batch."""
        from . import ops
        swap = self.check_channel_order(channel_order)
        n, sizes = frames.shape[0], tap_sizes(*self.frames_hw(frames))
        taps, x = [], frames
        for i, (_, co, ci, k, s, p) in enumerate(CONVS):
            (ho, wo), ldk = sizes[i], self.w[i].shape[1]
            if i == 0:
                rows = ops.im2col_frames(x, k, s, p, ldk, self.shift, self.scale, swap)[0]
            else:
                rows = ops.im2col3d(x, (1, k, k), (1, s, s), (0, p, p), (n, ho, wo), ldk, relu=i >= 3)
            y = torch.empty(n, ho, wo, co, dtype=torch.float16, device=rows.device)
            self.conv_into(rows.view(n, ho * wo, ldk), [(self.w[i], self.b[i], y, 0)])
            taps.append(y)
            x = ops.maxpool3d_relu(y, (1, 3, 3), (1, 2, 2), (0, 0, 0), (n, (ho - 3) // 2 + 1, (wo - 3) // 2 + 1)) if POOL_AFTER[i] else y
        return taps

    def __call__(self, a, b, channel_order="rgb", chunk=None, row_weights=None):
        """a, b: uint8 [F,H,W,3] or fp32 [F,3,H,W] in [0,1] on the device (channels R, G, B) -> fp64 [F] on the device.
        channel_order 'bgr' hands the network B, G, R planes, as the reference's cv2.imread frames reach it.
        row_weights (H values, optional; metrics.latitude_weights(H) gives WS-LPIPS of equirectangular frames): every tap's upsampled
        map is averaged under one weight per image row, sum_taps sum_yx w[y] up(y,x) / (W sum_y w[y]), instead of uniformly."""
        from . import ops
        if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
            raise ValueError(f"a {tuple(a.shape)} {a.dtype} on {a.device} and b {tuple(b.shape)} {b.dtype} on {b.device} differ")
        F_, (H, W) = a.shape[0], self.frames_hw(a)
        sizes = tap_sizes(H, W)
        n_out = H * W
        if row_weights is not None:
            row_weights = ops.check_row_weights(row_weights, H)
            n_out = W * float(row_weights.sum())
            wy_rows = [torch.from_numpy(upsample_mean_weights(h, H, row_weights)).to(self.device) for h, _ in sizes]
        chunk = max(1, int(chunk or self.chunk))
        acc = torch.zeros(F_, dtype=torch.float64, device=a.device)
        for f0 in range(0, F_, chunk):
            n = min(chunk, F_ - f0)
            taps = self.features(torch.cat([a[f0:f0 + n], b[f0:f0 + n]]).contiguous(), channel_order)
            for i, t in enumerate(taps):
                wy, wx = self._weights_for(*sizes[i], H, W)
                if row_weights is not None:
                    wy = wy_rows[i]
                ops.lpips_head(t[:n], t[n:], self.lin[i], wy, wx, n_out, acc[f0:f0 + n])
        ops.streamk_check()                        # results leave here: a timed-out stream-K hand-over in a convolution must not pass silently
        return acc
