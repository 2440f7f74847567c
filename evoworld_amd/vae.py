"""AutoencoderKLTemporalDecoder on the HIP kernels: the temporal VAE either side of the denoise loop.

Call surface of the diffusers class the reference pipeline drives (evoworld/pipeline/pipeline_evoworld.py:307-328,358-385):
    vae = AutoencoderKLTemporalDecoder.from_pretrained(path, subfolder="vae")        # or .from_random(seed)
    vae.config.{block_out_channels, scaling_factor, force_upcast, latent_channels}; vae.dtype
    vae.encode(x[N,3,H,W] in [-1,1]).latent_dist.mode()   -> [N,4,H/8,W/8]
    vae.decode(z[N,4,h,w], num_frames=k).sample           -> [N,3,8h,8w]
State-dict keys are the diffusers keys (oracle/vae_ref.py lists the tree), so the SVD-XT VAE checkpoint loads.

Execution plan (same as the U-Net): fp16 channels-last activations, split-fp16 residual stream, every conv an
implicit-GEMM ew_gemm_f16 (3x3, stride-2 with the (0,1) padding of Downsample2D(padding=0) as `conv_shift`, nearest-x2
upsample as DMA addressing, frame-axis 3-tap), GroupNorm / SiLU as the deterministic two-stage kernels.  The single-head
512-wide attention of the mid blocks is two GEMMs around ew_softmax_rows_f16 per frame (scores leave the GEMM as hi + lo, so
the exponential sees fp32 scores); exact algebra removes work: the key bias shifts every score of a query row equally
(softmax-invariant, dropped), the value bias passes through the row-stochastic P unchanged (folded into the out-projection
bias), quant_conv (1x1, 8->8) is folded into the encoder's conv_out and only the 4 mean channels mode() returns are computed.
"""
import math
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import ops
from ._model import PackedModel, Spec, Weights
from .ops import Res

DEFAULT_VAE_CONFIG = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=4,
                          scaling_factor=0.18215, force_upcast=True)
CPAD = 64


def vae_param_spec(cfg):
    """name -> (shape, kind) in module-registration order (_model.Spec; diffusers key names)."""
    boc = tuple(cfg["block_out_channels"])
    L, lat = cfg["layers_per_block"], cfg["latent_channels"]
    spec = Spec()
    conv, lin, norm = spec.conv, spec.lin, spec.norm

    def res2d(p, ci, co):
        norm(p + ".norm1", ci); conv(p + ".conv1", co, ci, (3, 3)); norm(p + ".norm2", co); conv(p + ".conv2", co, co, (3, 3))
        if ci != co:
            conv(p + ".conv_shortcut", co, ci, (1, 1))

    def st_res(p, ci, co):
        res2d(p + ".spatial_res_block", ci, co)
        t = p + ".temporal_res_block"
        norm(t + ".norm1", co); conv(t + ".conv1", co, co, (3, 1, 1)); norm(t + ".norm2", co); conv(t + ".conv2", co, co, (3, 1, 1))
        spec.add(p + ".time_mixer.mix_factor", (1,), "mix")

    def attn(p, c):
        norm(p + ".group_norm", c)
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            lin(p + "." + n, c, c)

    conv("encoder.conv_in", boc[0], 3, (3, 3))
    out = boc[0]
    for i, c in enumerate(boc):
        cin, out = out, c
        for l in range(L):
            res2d(f"encoder.down_blocks.{i}.resnets.{l}", cin if l == 0 else out, out)
        if i < len(boc) - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", out, out, (3, 3))
    res2d("encoder.mid_block.resnets.0", boc[-1], boc[-1]); attn("encoder.mid_block.attentions.0", boc[-1])
    res2d("encoder.mid_block.resnets.1", boc[-1], boc[-1])
    norm("encoder.conv_norm_out", boc[-1]); conv("encoder.conv_out", 2 * lat, boc[-1], (3, 3))
    conv("decoder.conv_in", boc[-1], lat, (3, 3))
    st_res("decoder.mid_block.resnets.0", boc[-1], boc[-1]); attn("decoder.mid_block.attentions.0", boc[-1])
    st_res("decoder.mid_block.resnets.1", boc[-1], boc[-1])
    rev = boc[::-1]
    out = rev[0]
    for i, c in enumerate(rev):
        prev, out = out, c
        for l in range(L + 1):
            st_res(f"decoder.up_blocks.{i}.resnets.{l}", prev if l == 0 else out, out)
        if i < len(rev) - 1:
            conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", out, out, (3, 3))
    norm("decoder.conv_norm_out", boc[0]); conv("decoder.conv_out", 3, boc[0], (3, 3))
    conv("decoder.time_conv_out", 3, 3, (3, 1, 1))
    conv("quant_conv", 2 * lat, 2 * lat, (1, 1))
    return spec


def random_vae_state_dict(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict()
    for name, (shape, kind) in vae_param_spec(cfg).items():
        if kind == "gamma":
            sd[name] = torch.ones(shape)
        elif kind == "beta":
            sd[name] = torch.zeros(shape)
        elif kind == "mix":
            sd[name] = torch.full(shape, 0.3)
        else:
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(kind)
    return sd


class AutoencoderKLTemporalDecoder(PackedModel):
    DEFAULTS = DEFAULT_VAE_CONFIG
    WEIGHT_FILES = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.fp16.safetensors")
    MISSING = "VAE state dict is missing"
    _spec, _random = staticmethod(vae_param_spec), staticmethod(random_vae_state_dict)

    def __init__(self, **config):
        cfg = dict(DEFAULT_VAE_CONFIG)
        cfg.update(config)
        cfg["block_out_channels"] = tuple(cfg["block_out_channels"])
        for c in cfg["block_out_channels"]:
            if c % 64:
                raise ValueError("evoworld_amd VAE: block_out_channels must be multiples of 64")
        super().__init__(cfg, torch.float32)  # API dtype: fp32 tensors in and out (the reference keeps the VAE in fp32, force_upcast)
        self.split_residual = os.environ.get("EW_RESIDUAL", "split") != "fp16"
        self.chunk = 8                      # frames per encoder pass (the encoder has no frame-axis op: chunking is exact)

    # ---------------- weight packing ----------------
    def _pack(self, sd):
        f = Weights(sd, self.device)
        f32, h, conv, dev = f.f32, f.h, f.conv, self.device
        boc, L, lat = self._cfg["block_out_channels"], self._cfg["layers_per_block"], self._cfg["latent_channels"]

        def res2d(p, ci, co):
            d = {"n1": f.pair(p + ".norm1"), "c1": conv(p + ".conv1"), "n2": f.pair(p + ".norm2"), "c2": conv(p + ".conv2"), "ci": ci, "co": co}
            if ci != co:
                d["sc"] = (h(f32(p + ".conv_shortcut.weight")[:, :, 0, 0]), h(f32(p + ".conv_shortcut.bias")))
            return d

        def st_res(p, ci, co):
            d = res2d(p + ".spatial_res_block", ci, co)
            t = p + ".temporal_res_block"
            d["tn1"], d["t1"], d["tn2"], d["t2"] = f.pair(t + ".norm1"), conv(t + ".conv1"), f.pair(t + ".norm2"), conv(t + ".conv2")
            d["mix"] = float(torch.sigmoid(f32(p + ".time_mixer.mix_factor")).item())
            return d

        def attn(p, c):
            wo, bo = f32(p + ".to_out.0.weight"), f32(p + ".to_out.0.bias")
            return {"gn": f.pair(p + ".group_norm"), "q": f.pair(p + ".to_q"),
                    "k": h(f32(p + ".to_k.weight")),                       # key bias: constant per query row -> softmax-invariant
                    "v": h(f32(p + ".to_v.weight")),                       # value bias: rows of P sum to 1 -> moves to the out bias
                    "o": (h(wo), h(wo @ f32(p + ".to_v.bias") + bo)), "c": c}

        W = {}
        W["e_in"] = conv("encoder.conv_in", CPAD)
        W["e_down"] = []
        out = boc[0]
        for i, c in enumerate(boc):
            cin, out = out, c
            blk = {"res": [res2d(f"encoder.down_blocks.{i}.resnets.{l}", cin if l == 0 else out, out) for l in range(L)]}
            if i < len(boc) - 1:
                blk["down"] = conv(f"encoder.down_blocks.{i}.downsamplers.0.conv")
            W["e_down"].append(blk)
        W["e_mid"] = (res2d("encoder.mid_block.resnets.0", boc[-1], boc[-1]), attn("encoder.mid_block.attentions.0", boc[-1]),
                      res2d("encoder.mid_block.resnets.1", boc[-1], boc[-1]))
        W["e_no"] = f.pair("encoder.conv_norm_out")
        # quant_conv (1x1) folded into conv_out; only the `lat` mean channels
        wq, bq = f32("quant_conv.weight")[:lat, :, 0, 0], f32("quant_conv.bias")[:lat]
        wo, bo = f32("encoder.conv_out.weight"), f32("encoder.conv_out.bias")
        W["e_out"] = (ops.pack_conv_weight(torch.einsum("qo,oikl->qikl", wq, wo)), h(wq @ bo + bq))
        W["d_in"] = conv("decoder.conv_in", CPAD)
        W["d_mid"] = (st_res("decoder.mid_block.resnets.0", boc[-1], boc[-1]), attn("decoder.mid_block.attentions.0", boc[-1]),
                      st_res("decoder.mid_block.resnets.1", boc[-1], boc[-1]))
        W["d_up"] = []
        rev = boc[::-1]
        out = rev[0]
        for i, c in enumerate(rev):
            prev, out = out, c
            blk = {"res": [st_res(f"decoder.up_blocks.{i}.resnets.{l}", prev if l == 0 else out, out) for l in range(L + 1)]}
            if i < len(rev) - 1:
                blk["up"] = conv(f"decoder.up_blocks.{i}.upsamplers.0.conv")
            W["d_up"].append(blk)
        W["d_no"] = f.pair("decoder.conv_norm_out")
        wc, bc = f32("decoder.conv_out.weight"), f32("decoder.conv_out.bias")
        W["d_out"] = (ops.pack_conv_weight(torch.cat([wc, torch.zeros_like(wc[:1])])), h(torch.cat([bc, torch.zeros(1, device=dev)])))  # 3 -> 4 rows
        W["d_time"] = (f32("decoder.time_conv_out.weight")[:, :, :, 0, 0].contiguous(), f32("decoder.time_conv_out.bias").contiguous())
        self.w = W

    # ---------------- building blocks (activations: fp16 [N*H*W, C], residual stream: Res) ----------------
    def _res(self, rows, C, dev, head=False):      # `head` (the U-Net's second policy) does not apply: one stream format
        return Res.empty(rows, C, dev, self.split_residual)

    def _resnet2d(self, d, x, N, H, W_):
        """ResnetBlock2D without time embedding: x + conv2(silu(gn(conv1(silu(gn(x))))))  (x: Res) -> Res"""
        HW = H * W_
        dev = x.hi.device
        hN = ops.groupnorm([x], *d["n1"], N, HW, 1e-6, True, pool=self._pool)
        h1 = self._conv3x3(hN, *d["c1"], N, H, W_, H, W_)
        h2 = ops.groupnorm([h1], *d["n2"], N, HW, 1e-6, True, pool=self._pool)
        if "sc" in d:
            sc = self._res(N * HW, d["co"], dev)
            ops.gemm(x.hi, d["sc"][0], sc, M=N * HW, N=d["co"], c1=d["ci"], lda=d["ci"], bias=d["sc"][1])
        else:
            sc = x
        return self._conv3x3(h2, *d["c2"], N, H, W_, H, W_, res_out=True, r1=sc, ld_r1=d["co"])

    def _st_resblock(self, d, x, B, T, H, W_):
        """SpatioTemporalResBlock of the decoder: AlphaBlender 'learned' with switch_spatial_to_temporal_mix=True:
        out = (1-a)*xsp + a*(xsp + conv2(..)) = xsp + a*conv2(..), a = sigmoid(mix_factor)."""
        HW = H * W_
        xsp = self._resnet2d(d, x, B * T, H, W_)
        g1 = ops.groupnorm([xsp], *d["tn1"], B, T * HW, 1e-5, True, pool=self._pool)
        t1 = self._convt(g1, *d["t1"], B, T, HW)
        g2 = ops.groupnorm([t1], *d["tn2"], B, T * HW, 1e-5, True, pool=self._pool)
        return self._convt(g2, *d["t2"], B, T, HW, res_out=True, r1=xsp, ld_r1=d["co"], c_acc=d["mix"], c_r1=1.0)

    def _attention(self, d, x, N, H, W_):
        """single-head attention over the H*W tokens of each frame, residual outside (diffusers Attention)"""
        C, S = d["c"], H * W_
        dev = x.hi.device
        if S % 64:
            raise ValueError("VAE attention needs (H/8)*(W/8) to be a multiple of 64")
        hn = ops.groupnorm([x], *d["gn"], N, S, 1e-6, False, pool=self._pool)
        q = ops.linear(hn, *d["q"])
        k = ops.linear(hn, d["k"])
        o = torch.empty(N * S, C, dtype=torch.float16, device=dev)
        vt = torch.empty(C, S, dtype=torch.float16, device=dev)
        scores = Res.empty(S, S, dev, True)                                 # hi + lo: the exponential sees fp32 scores
        p = torch.empty(S, S, dtype=torch.float16, device=dev)
        for f in range(N):
            sl = slice(f * S, (f + 1) * S)
            ops.gemm(d["v"], hn[sl], vt, M=C, N=S, c1=C, lda=C)             # V^T = W_v X^T (swapped operands), this frame
            ops.gemm(q[sl], k[sl], scores, M=S, N=S, c1=C, lda=C, c_acc=1.0 / math.sqrt(C))
            ops.softmax_rows(scores, out=p)
            ops.gemm(p, vt, o[sl], M=S, N=C, c1=S, lda=S)
        return ops.linear(o, *d["o"], out=self._res(N * S, C, dev), r1=x, ld_r1=C)

    def _begin(self, dev):
        if getattr(self, "_pool", None) is None or self._pool.buf.device != dev:
            self._pool = ops.WorkspacePool(dev, floats=16 << 20)
        self._pool.reset()

    # ---------------- encode ----------------
    def _encode_chunk(self, x):
        """x fp32 [n,3,H,W] -> fp32 [n,latent,H/8,W/8] (mean of the latent distribution)"""
        Wt = self.w
        n, _, H, W_ = x.shape
        dev = x.device
        self._begin(dev)
        xin = torch.zeros(n * H * W_, CPAD, dtype=torch.float16, device=dev)
        ops.nchw_f32_to_nhwc_f16(x.contiguous(), xin, CPAD)
        h = self._conv3x3(xin, *Wt["e_in"], n, H, W_, H, W_, res_out=True)
        for blk in Wt["e_down"]:
            for d in blk["res"]:
                h = self._resnet2d(d, h, n, H, W_)
            if "down" in blk:
                h = self._conv3x3(h.hi, *blk["down"], n, H, W_, H // 2, W_ // 2, res_out=True, stride=2, conv_shift=1)
                H, W_ = H // 2, W_ // 2
        r0, at, r1 = Wt["e_mid"]
        h = self._resnet2d(r0, h, n, H, W_)
        h = self._attention(at, h, n, H, W_)
        h = self._resnet2d(r1, h, n, H, W_)
        hn = ops.groupnorm([h], *Wt["e_no"], n, H * W_, 1e-6, True, pool=self._pool)
        lat = self._cfg["latent_channels"]
        z = self._conv3x3(hn, *Wt["e_out"], n, H, W_, H, W_)
        return ops.nhwc_f16_to_nchw_f32(z, n, lat, H, W_, lat)

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        self._require_loaded()
        if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"encode expects [N,3,H,W] with H, W multiples of 8, got {tuple(x.shape)}")
        x = x.to(device=self.device, dtype=torch.float32)
        mean = torch.cat([self._encode_chunk(x[i:i + self.chunk]) for i in range(0, x.shape[0], self.chunk)], dim=0)

        def _no_sample(*_a, **_k):
            raise NotImplementedError("only latent_dist.mode() (what the pipeline uses, pipeline_evoworld.py:311) is computed")
        dist = SimpleNamespace(mode=lambda: mean, mean=mean, sample=_no_sample)
        return SimpleNamespace(latent_dist=dist) if return_dict else (dist,)

    # ---------------- decode ----------------
    @torch.no_grad()
    def decode(self, z, num_frames=1, return_dict=True):
        """z fp32 [N,4,h,w] (already divided by scaling_factor by the caller, pipeline_evoworld.py:360); N % num_frames == 0."""
        self._require_loaded()
        if z.ndim != 4 or z.shape[1] != self._cfg["latent_channels"] or z.shape[0] % num_frames:
            raise ValueError(f"decode expects [N,{self._cfg['latent_channels']},h,w] with N a multiple of num_frames, got {tuple(z.shape)}")
        Wt = self.w
        z = z.to(device=self.device, dtype=torch.float32).contiguous()
        N, _, H, W_ = z.shape
        B, T = N // num_frames, num_frames
        dev = z.device
        self._begin(dev)
        zin = torch.zeros(N * H * W_, CPAD, dtype=torch.float16, device=dev)
        ops.nchw_f32_to_nhwc_f16(z, zin, CPAD)
        h = self._conv3x3(zin, *Wt["d_in"], N, H, W_, H, W_, res_out=True)
        r0, at, r1 = Wt["d_mid"]
        h = self._st_resblock(r0, h, B, T, H, W_)
        h = self._attention(at, h, N, H, W_)
        h = self._st_resblock(r1, h, B, T, H, W_)
        for blk in Wt["d_up"]:
            for d in blk["res"]:
                h = self._st_resblock(d, h, B, T, H, W_)
            if "up" in blk:
                h = self._conv3x3(h.hi, *blk["up"], N, H, W_, 2 * H, 2 * W_, res_out=True, upsample=1)
                H, W_ = 2 * H, 2 * W_
        hn = ops.groupnorm([h], *Wt["d_no"], N, H * W_, 1e-6, True, pool=self._pool)
        y = self._conv3x3(hn, *Wt["d_out"], N, H, W_, H, W_)                               # [N*H*W, 4] (3 real channels)
        img = ops.nhwc_f16_to_nchw_f32(y, N, 3, H, W_, 4).reshape(B, T, 3, H, W_)
        out = ops.time_conv3(img, *Wt["d_time"]).reshape(N, 3, H, W_)
        return SimpleNamespace(sample=out) if return_dict else (out,)
