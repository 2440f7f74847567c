"""UNetSpatioTemporalConditionModel on hand-written HIP kernels (gfx950).

Call surface of the reference's U-Net shell, evoworld/trainer/unet_plucker.py:30-488 (itself a copy of
diffusers' UNetSpatioTemporalConditionModel with conv_in widened to 18 channels,
evoworld/trainer/trainer_utils.py:17-64):
    unet = UNetSpatioTemporalConditionModel.from_pretrained(path, subfolder="unet")      # or (**config)
    unet.config.in_channels / .addition_time_embed_dim / .num_frames / .sample_size
    unet.add_embedding.linear_1.in_features
    unet(sample[B,T,18,h,w], timestep, encoder_hidden_states=[B,1,1024], added_time_ids=[B,3],
         return_dict=False) -> (Tensor[B,T,4,h,w],)
State-dict keys are the diffusers keys, so a real SVD-Xtend/EvoWorld checkpoint loads.

MI355X-first execution plan:
  * activations live in HBM as fp16 channels-last [B*T*h*w, C]; conv <-> transformer hand-offs need no permute;
  * every contraction is ew_gemm_f16 (MFMA, LDS-DMA staged); im2col / skip-concat / nearest-upsample / frame-axis
    taps are DMA addressing modes; bias, time-embedding add, GEGLU, residual adds and AlphaBlender are epilogues;
  * the single-KV-token cross attention is the exact identity out = to_out(to_v(ctx)); the two
    weight matrices are folded at load time and the result enters the self-attention out-proj epilogue as a
    per-batch-row bias -- the reference's q-proj / QK^T / out-proj work on it is dead and not executed;
  * all time-embedding projections (44) and all cross-attention vectors (32) are two batched tiny GEMMs per forward.
No torch.nn compute: torch provides device memory, the HIP stream and trivially small host-side glue only.
"""
import math
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import ops
from ._model import PackedModel, Spec, Weights
from .ops import ACT_GEGLU, ACT_SILU, Res

DEFAULT_CONFIG = dict(  # evoworld/trainer/unet_plucker.py:69-94 with in_channels=18 (trainer_utils.py:19)
    sample_size=None, in_channels=18, out_channels=4,
    down_block_types=("CrossAttnDownBlockSpatioTemporal",) * 3 + ("DownBlockSpatioTemporal",),
    up_block_types=("UpBlockSpatioTemporal",) + ("CrossAttnUpBlockSpatioTemporal",) * 3,
    block_out_channels=(320, 640, 1280, 1280), addition_time_embed_dim=256,
    projection_class_embeddings_input_dim=768, layers_per_block=2, cross_attention_dim=1024,
    transformer_layers_per_block=1, num_attention_heads=(5, 10, 20, 20), num_frames=25)

CPAD_IN = 64  # conv_in input channels padded to one 64-wide K tile
SPLIT_DUP_LOG2 = 10  # conv_in with exact operands (round 5): the duplicate block of the input row holds x_hi * 2^-10 and its weight rows W_lo * 2^10,
#                      so that W_lo (~2^-12 |W|) is a NORMAL fp16 number whatever the MFMA does with denormals (csrc/elementwise.hip uses the same constant)


def split_in_offsets(in_channels):
    """(lo_off, dup_off) of the split model-input row [x_hi | x_lo | x_hi 2^-10] inside CPAD_IN channels, or None when three blocks do not fit."""
    s = (in_channels + 3) // 4 * 4
    return (s, 2 * s) if 3 * s <= CPAD_IN else None


def hi_lo(w):
    """fp32 tensor -> (its fp16-representable part, the remainder), both fp32: w == hi + lo exactly."""
    w_hi = w.to(torch.float16).to(torch.float32)
    return w_hi, w - w_hi


def split_conv_in_weight(w, in_split):
    """conv_in weight [O, I, 3, 3] fp32 -> fp32 [O, CPAD_IN, 3, 3] whose input-channel blocks [0, I) | [lo_off, +I) | [dup_off, +I) hold
    W_hi | W_hi | W_lo 2^10: against the row [x_hi | x_lo | x_hi 2^-10] the conv forms x_hi W_hi + x_lo W_hi + x_hi W_lo = x W - x_lo W_lo."""
    w_hi, w_lo = hi_lo(w)
    ci, (lo_off, dup_off) = w.shape[1], in_split
    wp = torch.zeros(w.shape[0], CPAD_IN, 3, 3, dtype=torch.float32, device=w.device)
    wp[:, :ci], wp[:, lo_off:lo_off + ci], wp[:, dup_off:dup_off + ci] = w_hi, w_hi, w_lo * float(2 ** SPLIT_DUP_LOG2)
    return wp


def split_input_row(x, in_split):
    """Host twin of ew_nchw_f32_to_nhwc_split_f16 (tests): x fp32 [N, I, H, W] -> fp16 [N, CPAD_IN, H, W] = [x_hi | x_lo | x_hi 2^-10] channel blocks."""
    lo_off, dup_off = in_split
    ci = x.shape[1]
    row = torch.zeros(x.shape[0], CPAD_IN, *x.shape[2:], dtype=torch.float16, device=x.device)
    hi = x.to(torch.float16)
    row[:, :ci], row[:, lo_off:lo_off + ci] = hi, (x - hi.float()).to(torch.float16)
    row[:, dup_off:dup_off + ci] = (hi.float() * 2.0 ** -SPLIT_DUP_LOG2).to(torch.float16)
    return row


def _pad64(c):
    return (c + 63) // 64 * 64


# ------------------------------------------------------------------------------------------------
# architecture walk: one place that knows the module tree (names = diffusers state-dict keys)
# ------------------------------------------------------------------------------------------------
def _arch(cfg):
    boc = tuple(cfg["block_out_channels"])
    heads = tuple(cfg["num_attention_heads"])
    n = len(boc)
    L = cfg["layers_per_block"]
    res, trs, plan = [], [], []

    def R(prefix, cin, cout, eps):
        d = SimpleNamespace(p=prefix, cin=cin, cout=cout, eps=eps)
        res.append(d)
        return d

    def TR(prefix, ch, nh):
        d = SimpleNamespace(p=prefix, ch=ch, heads=nh)
        trs.append(d)
        return d

    out = boc[0]
    downs = []
    for i in range(n):
        cin, out = out, boc[i]
        last = i == n - 1
        blk = SimpleNamespace(res=[], attn=[], down=None)
        for l in range(L):
            blk.res.append(R(f"down_blocks.{i}.resnets.{l}", cin if l == 0 else out, out, 1e-5 if last else 1e-6))
            if not last:
                blk.attn.append(TR(f"down_blocks.{i}.attentions.{l}", out, heads[i]))
        if not last:
            blk.down = SimpleNamespace(p=f"down_blocks.{i}.downsamplers.0.conv", ch=out)
        downs.append(blk)
    mid = SimpleNamespace(res=[R("mid_block.resnets.0", boc[-1], boc[-1], 1e-5), R("mid_block.resnets.1", boc[-1], boc[-1], 1e-5)],
                          attn=[TR("mid_block.attentions.0", boc[-1], heads[-1])])
    rev, rheads = boc[::-1], heads[::-1]
    ups = []
    out = rev[0]
    for i in range(n):
        prev, out = out, rev[i]
        cin = rev[min(i + 1, n - 1)]
        blk = SimpleNamespace(res=[], attn=[], up=None)
        for l in range(L + 1):
            skip = cin if l == L else out
            rin = prev if l == 0 else out
            r = R(f"up_blocks.{i}.resnets.{l}", rin + skip, out, 1e-6)
            r.split = (rin, skip)
            blk.res.append(r)
            if i > 0:
                blk.attn.append(TR(f"up_blocks.{i}.attentions.{l}", out, rheads[i]))
        if i < n - 1:
            blk.up = SimpleNamespace(p=f"up_blocks.{i}.upsamplers.0.conv", ch=out)
        ups.append(blk)
    return SimpleNamespace(downs=downs, mid=mid, ups=ups, res=res, trs=trs)


def param_spec(cfg):
    """name -> (shape, kind) in module-registration order (_model.Spec)."""
    spec = Spec()
    lin, conv, norm = spec.lin, spec.conv, spec.norm
    boc = tuple(cfg["block_out_channels"])
    temb = boc[0] * 4
    X = cfg["cross_attention_dim"]

    def resblock(r):
        s, t = r.p + ".spatial_res_block", r.p + ".temporal_res_block"
        norm(s + ".norm1", r.cin); conv(s + ".conv1", r.cout, r.cin, (3, 3)); lin(s + ".time_emb_proj", r.cout, temb)
        norm(s + ".norm2", r.cout); conv(s + ".conv2", r.cout, r.cout, (3, 3))
        if r.cin != r.cout:
            conv(s + ".conv_shortcut", r.cout, r.cin, (1, 1))
        norm(t + ".norm1", r.cout); conv(t + ".conv1", r.cout, r.cout, (3, 1, 1)); lin(t + ".time_emb_proj", r.cout, temb)
        norm(t + ".norm2", r.cout); conv(t + ".conv2", r.cout, r.cout, (3, 1, 1))
        spec.add(r.p + ".time_mixer.mix_factor", (1,), "mix")

    def attn(p, c, ctx):
        lin(p + ".to_q", c, c, False); lin(p + ".to_k", c, ctx or c, False); lin(p + ".to_v", c, ctx or c, False)
        lin(p + ".to_out.0", c, c)

    def ff(p, c):
        lin(p + ".net.0.proj", 8 * c, c); lin(p + ".net.2", c, 4 * c)

    def transformer(t):
        c = t.ch
        norm(t.p + ".norm", c); lin(t.p + ".proj_in", c, c)
        b = t.p + ".transformer_blocks.0"
        norm(b + ".norm1", c); attn(b + ".attn1", c, None); norm(b + ".norm2", c); attn(b + ".attn2", c, X)
        norm(b + ".norm3", c); ff(b + ".ff", c)
        b = t.p + ".temporal_transformer_blocks.0"
        norm(b + ".norm_in", c); ff(b + ".ff_in", c); norm(b + ".norm1", c); attn(b + ".attn1", c, None)
        norm(b + ".norm2", c); attn(b + ".attn2", c, X); norm(b + ".norm3", c); ff(b + ".ff", c)
        lin(t.p + ".time_pos_embed.linear_1", 4 * c, c); lin(t.p + ".time_pos_embed.linear_2", c, 4 * c)
        spec.add(t.p + ".time_mixer.mix_factor", (1,), "mix")
        lin(t.p + ".proj_out", c, c)

    conv("conv_in", boc[0], cfg["in_channels"], (3, 3))
    lin("time_embedding.linear_1", temb, boc[0]); lin("time_embedding.linear_2", temb, temb)
    lin("add_embedding.linear_1", temb, cfg["projection_class_embeddings_input_dim"]); lin("add_embedding.linear_2", temb, temb)
    a = _arch(cfg)
    for blk in a.downs:
        for r in blk.res:
            resblock(r)
        for t in blk.attn:
            transformer(t)
        if blk.down:
            conv(blk.down.p, blk.down.ch, blk.down.ch, (3, 3))
    resblock(a.mid.res[0]); resblock(a.mid.res[1]); transformer(a.mid.attn[0])
    for blk in a.ups:
        for r in blk.res:
            resblock(r)
        for t in blk.attn:
            transformer(t)
        if blk.up:
            conv(blk.up.p, blk.up.ch, blk.up.ch, (3, 3))
    norm("conv_norm_out", boc[0]); conv("conv_out", cfg["out_channels"], boc[0], (3, 3))
    return spec


def random_state_dict(cfg, seed=0, device="cpu"):
    """PyTorch-default-style initialisation (U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases, norm
    gamma=1 beta=0, mix_factor=0.5) drawn from one generator in spec order."""
    g = torch.Generator(device=device).manual_seed(seed)
    sd = OrderedDict()
    for name, (shape, kind) in param_spec(cfg).items():
        if isinstance(kind, int):      # fan-in
            bound = 1.0 / math.sqrt(kind)
            sd[name] = (torch.rand(shape, generator=g, device=device) * 2 - 1) * bound
        elif kind == "gamma":
            sd[name] = torch.ones(shape, device=device)
        elif kind == "beta":
            sd[name] = torch.zeros(shape, device=device)
        else:
            sd[name] = torch.full(shape, 0.5, device=device)
    return sd


class UNetSpatioTemporalConditionModel(PackedModel):
    """from_pretrained: diffusers folder layout, <path>/<subfolder>/config.json + diffusion_pytorch_model.safetensors
    (unified_loop_consistency.py:190-192); its qkv_fp8 keyword is the config key of the same name (None: EW_QKV_FP8 decides)."""
    DEFAULTS = DEFAULT_CONFIG
    WEIGHT_FILES = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.fp16.safetensors")
    PRETRAINED_KW = ("qkv_fp8",)
    _spec, _random = staticmethod(param_spec), staticmethod(random_state_dict)

    def __init__(self, **config):
        cfg = dict(DEFAULT_CONFIG)
        cfg["qkv_fp8"] = os.environ.get("EW_QKV_FP8", "0") == "1"      # a keyword argument overrides the environment switch
        cfg.update(config)
        cfg["qkv_fp8"] = bool(cfg["qkv_fp8"])
        super().__init__(cfg, torch.float16)
        self.arch = _arch(cfg)
        self.add_embedding = SimpleNamespace(linear_1=SimpleNamespace(
            in_features=cfg["projection_class_embeddings_input_dim"]))
        # residual stream: split fp16 (hi + lo, ~21 bits; default) or plain fp16 (EW_RESIDUAL=fp16: -15 % HBM traffic,
        # +30 % rel-L2 distance to the fp32 reference -- DESIGN.md section 4)
        mode = os.environ.get("EW_RESIDUAL", "split")
        self.split_residual = mode != "fp16"
        self.split_heads = mode == "split"     # also split the stream tensors produced WITHOUT a residual operand
        # qkv_fp8 (config key, default False; EW_QKV_FP8=1 sets it): BASELINE.json configs[4]'s "fp8 MFMA QKV".  The attn1 q / k / v projections of
        # every transformer whose width is a multiple of 64 (`fp8_blocks`, filled at load time) run on ew_gemm_fp8: per-row-scaled e4m3 operands
        # (one fp32 scale per token row, quantised once per LayerNorm output by ew_quant_rows_fp8, and one per weight row, quantised at load time),
        # fp32 accumulation, fp16 out.  It halves the projections' operand bytes, not their MFMA time, carries its own tolerance
        # (tests/test_gpu_fp8_qkv.py) and makes no speed claim; the fp16 default is untouched by it.
        self.fp8_blocks = []
        # round 4: q|k projections carry sqrt(scale * log2 e) in their epilogue and the attention kernel's MFMA subtracts the running max
        # (ew_attn_spatial_log2_f16); attn_log2 = False (attribute, A/B only) restores the scale-and-shift form on ew_attn_spatial_f16
        self.attn_log2 = True
        # conv1 output of every resblock (the GroupNorm input between the two 3x3 convs) carried split too: in the per-tensor
        # ablation (tests/analysis_fp16_floor.py --per-tensor, tag res_h1) its fp16 rounding was the largest storage term left
        # (0.15e-6 of squared rel-L2 against 0.56e-6 for fp16 MFMA operands alone; 8.9e-4 -> 8.2e-4 per forward for +1.0 ms)
        self.split_h1 = self.split_heads
        # EW_FUSED_FF: the level-0 feed-forwards (GEGLU pair + residual epilogue) through ONE kernel, ew_ff_geglu320_f16: 0 = LayerNorm
        # + two GEMMs (A/B baseline), 1 = LayerNorm kernel + fused kernel (default).  Mode 1 keeps the 1.18 GB GEGLU intermediate of each
        # of the 15 level-0 feed-forwards out of HBM (-35 GB per forward) and measures -1.9 ms per forward in place (A/B in one process).
        # (Modes 2 / 3 -- LayerNorm in the fused kernel's prologue, +9 ms; LayerNorm folded into the pack, +1.1 ms -- were removed in round 6.)
        self.fused_ff = 1 if os.environ.get("EW_FUSED_FF", "1") != "0" else 0
        # Round 5: fp16 operand rounding removed where it is (nearly) free.  An fp32 checkpoint (what the reference runs, unified_loop_consistency.py:188)
        # rounded to fp16 once costs as much squared distance to the fp32 oracle as all activation operands together, and per layer group (tiny
        # config, tests/analysis_fp16_floor.py --per-group) conv_in + conv_out + the level-0 proj_in / proj_out carry ~40 % of it for < 1 % of the flops:
        #   * conv_in: BOTH operands split inside the 64-channel K tile its 18 input channels are padded to anyway -- the model-input row is
        #     [x_hi | x_lo | x_hi 2^-10] (in_split; written by ew_nchw_f32_to_nhwc_split_f16 / ew_euler_cfg_step_split) against weight rows
        #     [W_hi | W_hi | W_lo 2^10]: zero extra MFMA work;
        #   * conv_out and the proj_in / proj_out GEMMs of the 320-channel transformers: W = W_hi + W_lo as a second K block over the SAME A
        #     operand (the dual-source addressing mode of the skip concat: a2 = a), K doubles on ~14 small launches.
        # Round 6: the ACTIVATION side of conv_out and of the level-0 proj_in as well -- their A operand is a GroupNorm output, which
        # ew_groupnorm_apply_split_f16 writes as the row [y_hi | y_lo]; the weights become three K blocks [W_hi | W_hi | W_lo] (source 2 = the
        # y_hi half again), i.e. x W to ~2^-21 in both operands: -16 % of the activation-rounding term (per-group shares: conv_out 7.8 %,
        # level-0 proj_in ~8 %) for one more 320-wide K block on 6 small launches.
        # EW_SPLIT_OPERANDS=0 restores single-rounded operands everywhere, =1 the round-5 set (weights only outside conv_in) (A/B).
        so = int(os.environ.get("EW_SPLIT_OPERANDS", "2"))
        self.split_operands = so != 0
        self.split_acts = so >= 2
        self.in_split = split_in_offsets(cfg["in_channels"]) if self.split_operands else None
        self._pos_cache = {}
        for hd, c in zip(cfg["num_attention_heads"], cfg["block_out_channels"]):
            if c // hd != 64:
                raise ValueError("evoworld_amd attention kernels are specialised to head_dim 64")

    # ---------------- construction / loading ----------------
    @classmethod
    def _config_from_json(cls, raw):
        return {k: (tuple(v) if isinstance(v, list) else v) for k, v in raw.items() if k in DEFAULT_CONFIG}

    @classmethod
    def from_zeros(cls, device="cuda", **config):
        """Same packed layout with all-zero weights: what a rank that does NOT read the checkpoint builds before
        `broadcast_weights` fills it over RCCL."""
        m = cls(**config)
        return m.load_state_dict(OrderedDict((k, torch.zeros(shape)) for k, (shape, _) in param_spec(m._cfg).items()), device=device)

    def packed_tensors(self):
        """Every device tensor of the packed weight set, in a fixed order (3.04 GB fp16 for the full U-Net)."""
        out = []

        def walk(v):      # dicts in key order, tuples / lists in position order, at any nesting depth
            if isinstance(v, torch.Tensor):
                out.append(v)
            elif isinstance(v, dict):
                for n in sorted(v, key=str):
                    walk(v[n])
            elif isinstance(v, (tuple, list)):
                for t in v:
                    walk(t)
        walk(self.w)
        return out

    def broadcast_weights(self, src=0):
        """One-time RCCL broadcast of the packed weights (and the AlphaBlender scalars) from rank `src` (SURVEY.md §8e:
        the rank that read the checkpoint serves the others over xGMI instead of N disk reads).  No-op single-process."""
        from . import distributed as D
        D.broadcast_tensors(self.packed_tensors(), src=src)
        keys = [k for k in sorted(self.w, key=str) if isinstance(self.w[k], dict) and "mix" in self.w[k]]
        mix = torch.tensor([self.w[k]["mix"] for k in keys], dtype=torch.float64, device=self.device)
        D.broadcast_tensors([mix], src=src)
        for k, v in zip(keys, mix.tolist()):
            self.w[k]["mix"] = v
        self._pos_cache = {}
        return self

    def weights_checksum(self):
        """fp64 sum of all packed weights (cheap equality check across ranks after the broadcast)."""
        return float(sum(t.double().sum() for t in self.packed_tensors()))

    def to(self, device=None, dtype=None):
        if device is not None and self.w is not None and torch.device(device) != self.device:
            raise NotImplementedError("weights are packed on the device given at load time")
        return self

    # ---------------- weight packing (once) ----------------
    def _pack(self, sd):
        f = Weights(sd, self.device)
        f32, h = f.f32, f.h
        self._pos_cache = {}   # time_pos_embed outputs depend on the weights being replaced
        W = {}

        def lin2(k, c, acts=False):  # [O, I] -> [O, 2 I] = [W_hi | W_lo] for the level-0 projections (a2 = a), plain fp16 otherwise;
            w = f32(k + ".weight")    # acts: [O, 3 I] = [W_hi | W_hi | W_lo] against the split A operand [x_hi | x_lo] + x_hi again
            if not (self.split_operands and c == self._cfg["block_out_channels"][0]):
                return h(w), h(f32(k + ".bias"))
            w_hi, w_lo = hi_lo(w)
            return h(torch.cat([w_hi, w_hi, w_lo] if acts else [w_hi, w_lo], dim=1)), h(f32(k + ".bias"))

        def geglu(k):              # interleave value/gate rows in blocks of 16 (see ew_gemm_f16)
            w, b = f32(k + ".weight"), f32(k + ".bias")
            n = w.shape[0] // 2
            idx = torch.arange(2 * n, device=self.device).reshape(2, n // 16, 16).permute(1, 0, 2).reshape(-1)
            return h(w[idx]), h(b[idx])

        def ff(k, norm, c):        # one GEGLU feed-forward behind its LayerNorm: what `_ff` issues
            d = {"norm": f.pair(norm), "up": geglu(k + ".net.0.proj"), "down": f.pair(k + ".net.2")}
            if c == 320 and 4 * c == sd[k + ".net.2.weight"].shape[1]:
                # level 0: the GEGLU feed-forward pair runs as ONE kernel (ew_ff_geglu320_f16) on LDS-image packs
                d["pack"] = ops.ff_pack(f32(k + ".net.0.proj.weight"), f32(k + ".net.0.proj.bias"), f32(k + ".net.2.weight"))
            return d

        def fp8(w):                # [O, I] fp32 -> (e4m3 bytes uint8 [O, I], fp32 scale [O]), one scale per output row, on the device
            return ops.quant_rows_fp8(h(w))

        self.fp8_blocks = []
        temb_w, temb_b, self._temb_off = [], [], {}
        off = 0
        for r in self.arch.res:
            s, t = r.p + ".spatial_res_block", r.p + ".temporal_res_block"
            d = {"n1": f.pair(s + ".norm1"), "c1": f.conv(s + ".conv1"), "n2": f.pair(s + ".norm2"), "c2": f.conv(s + ".conv2"),
                 "tn1": f.pair(t + ".norm1"), "t1": f.conv(t + ".conv1"), "tn2": f.pair(t + ".norm2"), "t2": f.conv(t + ".conv2"),
                 "mix": float(torch.sigmoid(f32(r.p + ".time_mixer.mix_factor")).item())}
            if r.cin != r.cout:
                d["sc"] = (h(f32(s + ".conv_shortcut.weight")[:, :, 0, 0]), h(f32(s + ".conv_shortcut.bias")))
            for which in (s, t):
                temb_w.append(f32(which + ".time_emb_proj.weight"))
                temb_b.append(f32(which + ".time_emb_proj.bias"))
                self._temb_off[which] = off
                off += r.cout
            W[r.p] = d
        W["temb"] = (h(torch.cat(temb_w)), h(torch.cat(temb_b)))
        self._temb_total = off

        cv_w, cv_b, self._cv_off = [], [], {}
        off = 0
        for t in self.arch.trs:
            c = t.ch
            use_fp8 = self._cfg["qkv_fp8"] and c % 64 == 0      # ew_gemm_fp8 needs K % 64 == 0: other widths keep fp16 projections
            if use_fp8:
                self.fp8_blocks.append(t.p)
            d = {"norm": f.pair(t.p + ".norm"), "proj_in": lin2(t.p + ".proj_in", c, self.split_acts), "proj_out": lin2(t.p + ".proj_out", c),
                 "mix": float(torch.sigmoid(f32(t.p + ".time_mixer.mix_factor")).item()),
                 "pe1": f.pair(t.p + ".time_pos_embed.linear_1"), "pe2": f.pair(t.p + ".time_pos_embed.linear_2")}
            for tag, b in (("s", t.p + ".transformer_blocks.0"), ("t", t.p + ".temporal_transformer_blocks.0")):
                q, k_, v = f32(b + ".attn1.to_q.weight"), f32(b + ".attn1.to_k.weight"), f32(b + ".attn1.to_v.weight")
                # qkv_fp8: (bytes, scales) packs in place of the fp16 matrices: they travel through packed_tensors() like any other tuple
                if tag == "s":
                    d["s_qk"], d["s_v"] = (fp8(torch.cat([q, k_])), fp8(v)) if use_fp8 else (h(torch.cat([q, k_])), h(v))
                else:
                    d["t_qkv"] = fp8(torch.cat([q, k_, v])) if use_fp8 else h(torch.cat([q, k_, v]))
                    d["t_ff_in"] = ff(b + ".ff_in", b + ".norm_in", c)
                d[tag + "_norm1"], d[tag + "_out"] = f.pair(b + ".norm1"), f.pair(b + ".attn1.to_out.0")
                d[tag + "_ff"] = ff(b + ".ff", b + ".norm3", c)
                # cross attention with ONE key/value token: out = to_out(to_v(ctx)) -> fold the two matrices
                cv_w.append(f32(b + ".attn2.to_out.0.weight") @ f32(b + ".attn2.to_v.weight"))
                cv_b.append(f32(b + ".attn2.to_out.0.bias"))
                self._cv_off[(t.p, tag)] = off
                off += c
            W[t.p] = d
        W["cv"] = (h(torch.cat(cv_w)), h(torch.cat(cv_b)))
        self._cv_total = off

        for blk in self.arch.downs:
            if blk.down:
                W[blk.down.p] = f.conv(blk.down.p)
        for blk in self.arch.ups:
            if blk.up:              # (w, bias, upsample): four 2x2 phase convs (upsample = 2) where the channel counts allow, nine taps otherwise
                W[blk.up.p] = f.conv_up(blk.up.p)
        if self.in_split:
            W["conv_in"] = (ops.pack_conv_weight(split_conv_in_weight(f32("conv_in.weight"), self.in_split)), h(f32("conv_in.bias")))
        else:
            W["conv_in"] = f.conv("conv_in", CPAD_IN)
        if self.split_operands:     # [W_hi | W_lo] over the input channels: the second block reads the same tensor again (a2 = a);
            w_hi, w_lo = hi_lo(f32("conv_out.weight"))      # split_acts: [W_hi | W_hi | W_lo] against the [x_hi | x_lo] rows of conv_norm_out
            W["conv_out"] = (ops.pack_conv_weight(torch.cat([w_hi, w_hi, w_lo] if self.split_acts else [w_hi, w_lo], dim=1)), h(f32("conv_out.bias")))
        else:
            W["conv_out"] = f.conv("conv_out")
        W["norm_out"], W["te1"], W["ae1"] = f.pair("conv_norm_out"), f.pair("time_embedding.linear_1"), f.pair("add_embedding.linear_1")
        # emb = time_embedding.linear_2(.) + add_embedding.linear_2(.): one GEMM over the K-concat
        W["e2"] = (h(torch.cat([f32("time_embedding.linear_2.weight"), f32("add_embedding.linear_2.weight")], dim=1)),
                   h(f32("time_embedding.linear_2.bias") + f32("add_embedding.linear_2.bias")))
        self.w = W

    # ---------------- building blocks ----------------
    def _res(self, rows, C, dev, head=False):
        return Res.empty(rows, C, dev, self.split_heads if head else self.split_residual)

    def _lin2(self, x, w, b, out, **kw):
        """Linear whose weight may be packed [W_hi | W_lo] (twice the input width): the second K block reads x again (a2 = a); or
        [W_hi | W_hi | W_lo] against split rows x = [x_hi | x_lo] (1.5 x the row width): the third block reads the x_hi half again."""
        C = x.shape[-1]
        if w.shape[1] == C:
            return ops.linear(x, w, b, out=out, **kw)
        c2 = w.shape[1] - C         # = C (plain rows) or C / 2 (split rows)
        return ops.gemm(x, w, out, M=x.shape[0], N=w.shape[0], c1=C, lda=C, a2=x, c2=c2, lda2=C, bias=b, **kw)

    def _resblock(self, r, xs, tembs, B, T, H, W_):
        """SpatioTemporalResBlock = ResnetBlock2D -> TemporalResnetBlock -> AlphaBlender.
        xs: one or two `Res` (the up-block skip concat is addressing); returns a `Res`."""
        d = self.w[r.p]
        N, HW = B * T, H * W_
        rows = N * HW
        s, t = r.p + ".spatial_res_block", r.p + ".temporal_res_block"
        x1 = xs[0]
        x2 = xs[1] if len(xs) > 1 else None
        dev = x1.hi.device
        tb_s = tembs[:, self._temb_off[s]:]
        tb_t = tembs[:, self._temb_off[t]:]
        hN = ops.groupnorm(xs, *d["n1"], N, HW, r.eps, True, pool=self._gn_pool)
        h1 = self._conv3x3(hN, *d["c1"], N, H, W_, H, W_, rowbias=tb_s, rows_per_group=T * HW,
                           ld_rowbias=self._temb_total, res_out=self.split_h1)
        h2 = ops.groupnorm([h1], *d["n2"], N, HW, r.eps, True, pool=self._gn_pool)
        if "sc" in d:
            sc = self._res(rows, r.cout, dev, head=True)
            c1 = x1.hi.shape[-1]
            c2 = x2.hi.shape[-1] if x2 is not None else 0
            ops.gemm(x1.hi, d["sc"][0], sc, M=rows, N=r.cout, c1=c1, lda=c1, a2=x2.hi if x2 is not None else None, c2=c2,
                     lda2=c2, bias=d["sc"][1])
        else:
            sc = x1
        xsp = self._conv3x3(h2, *d["c2"], N, H, W_, H, W_, r1=sc, ld_r1=r.cout, res_out=True)
        g1 = ops.groupnorm([xsp], *d["tn1"], B, T * HW, r.eps, True, pool=self._gn_pool)
        t1 = self._convt(g1, *d["t1"], B, T, HW, rowbias=tb_t, rows_per_group=T * HW,
                         ld_rowbias=self._temb_total)
        g2 = ops.groupnorm([t1], *d["tn2"], B, T * HW, r.eps, True, pool=self._gn_pool)
        # x_temporal = xsp + conv2(..); AlphaBlender (switch_spatial_to_temporal_mix=False, the SpatioTemporalResBlock
        # default the U-Net blocks use): out = a*xsp + (1-a)*x_temporal = xsp + (1-a)*conv2(..), a = sigmoid(mix)
        return self._convt(g2, *d["t2"], B, T, HW, r1=xsp, ld_r1=r.cout, c_acc=1.0 - d["mix"], c_r1=1.0,
                           res_out=True)

    def _pos_emb(self, t, B, T):
        key = (t.p, B, T)
        if key not in self._pos_cache:
            d = self.w[t.p]
            sin = ops.sinusoid_embed(torch.arange(T, device=self.device, dtype=torch.float32), T, t.ch)
            e = ops.linear(ops.linear(sin, *d["pe1"], act=ACT_SILU), *d["pe2"])
            self._pos_cache[key] = e.repeat(B, 1).contiguous()
        return self._pos_cache[key]

    def _ff(self, ff, x, out, ln_kw={}, **epi):
        """One GEGLU feed-forward: out = epilogue(down(GEGLU(up(LayerNorm(x))))), `epi` = the residual / row-bias operands both forms share.
        Level 0 (the block has the LDS-image pack) with fused_ff: one kernel after the LayerNorm; otherwise two GEMMs."""
        n = ops.layernorm(x, *ff["norm"], **ln_kw)
        if self.fused_ff and "pack" in ff:
            return ops.ff_geglu320(n, ff["pack"], ff["down"][1], out, **epi)
        C = n.shape[-1]
        return ops.linear(ops.linear(n, *ff["up"], act=ACT_GEGLU), *ff["down"], out=out, ld_r1=C, ld_r2=C if "r2" in epi else 0, **epi)

    def _transformer(self, t, x, cvecs, B, T, H, W_):
        """TransformerSpatioTemporalModel.  x and the result are `Res`; every tensor of the block's
        residual stream (h, hm) is a `Res`, the GEMM operands (norm outputs, q/k/v, attention output, GEGLU output, the
        blended hb) are plain fp16."""
        d = self.w[t.p]
        C, N, S = t.ch, B * T, H * W_
        rows = N * S
        dev = x.hi.device
        fp8 = isinstance(d["s_qk"], tuple)      # qkv_fp8: (bytes, scales) packs
        cv_s = cvecs[:, self._cv_off[(t.p, "s")]:]
        cv_t = cvecs[:, self._cv_off[(t.p, "t")]:]
        hn = ops.groupnorm([x], *d["norm"], N, S, 1e-6, False, pool=self._gn_pool, split_out=d["proj_in"][0].shape[1] == 3 * C)
        h = self._lin2(hn, *d["proj_in"], self._res(rows, C, dev, head=True))
        # --- spatial BasicTransformerBlock ---
        n1 = ops.layernorm(h, *d["s_norm1"])
        prescale = ops.QK_LOG2_PRESCALE if self.attn_log2 else 1.0
        if fp8:                   # qkv_fp8: n1 is quantised once (one scale per token) and feeds both projections
            n1q, n1s = ops.quant_rows_fp8(n1)
            qk = ops.gemm_fp8(n1q, n1s, *d["s_qk"], c_acc=prescale)
            vt = ops.gemm_fp8(*d["s_v"], n1q, n1s)                    # V^T = W_v X^T (swapped roles) -> [C, rows]
            del n1q, n1s
        else:
            qk = ops.linear(n1, d["s_qk"], c_acc=prescale)
            vt = torch.empty(C, rows, dtype=torch.float16, device=dev)
            ops.gemm(d["s_v"], n1, vt, M=C, N=rows, c1=C, lda=C)      # V^T = W_v X^T (swapped operands)
        ao = torch.empty(rows, C, dtype=torch.float16, device=dev)
        (ops.attn_spatial_log2 if self.attn_log2 else ops.attn_spatial)(qk, qk[:, C:], vt, ao, N, S, t.heads, 2 * C, rows, C)
        del qk, vt
        # attn1 out-proj + residual + folded single-token cross attention (per batch row)
        h = ops.linear(ao, *d["s_out"], out=self._res(rows, C, dev), rowbias=cv_s, rows_per_group=T * S,
                       ld_rowbias=self._cv_total, r1=h, ld_r1=C)
        h = self._ff(d["s_ff"], h, self._res(rows, C, dev), r1=h)
        # --- TemporalBasicTransformerBlock on frame-major tokens (regroup = addressing) ---
        # x_temporal stream starts as h + time_pos_embed: the sum is formed inside the LayerNorm (for norm_in) and again in
        # the ff_in epilogue (r1 = h, row-bias = the frame's embedding) -- it is never written to HBM
        pos = self._pos_emb(t, B, T)
        # hm after ff_in and after the temporal attention are the two stream tensors whose fp16 rounding matters least
        # (tests/analysis_fp16_floor.py per-tensor ablation: +0.036e-6 and +0.021e-6 of squared rel-L2 against 0.25e-6 for a
        # resblock output): they are kept as plain fp16, which saves their lo halves' write + two reads
        hm = self._ff(d["t_ff_in"], h, Res.empty(rows, C, dev, False), dict(addvec=pos, rows_per_group=S), r1=h, rowbias=pos,
                      rows_per_group=S, ld_rowbias=C)
        n1 = ops.layernorm(hm, *d["t_norm1"])
        qkv = ops.gemm_fp8(*ops.quant_rows_fp8(n1), *d["t_qkv"]) if fp8 else ops.linear(n1, d["t_qkv"])
        ops.attn_temporal(qkv, qkv[:, C:], qkv[:, 2 * C:], ao, B, T, S, t.heads, 3 * C, C)
        del qkv
        hm = ops.linear(ao, *d["t_out"], out=Res.empty(rows, C, dev, False), rowbias=cv_t, rows_per_group=T * S,
                        ld_rowbias=self._cv_total, r1=hm, ld_r1=C)
        a = d["mix"]  # AlphaBlender: a*x_spatial + (1-a)*x_temporal, x_temporal = hm + ff(..); hb is only a GEMM operand
        hb = self._ff(d["t_ff"], hm, torch.empty(rows, C, dtype=torch.float16, device=dev), c_acc=1.0 - a, r1=hm, c_r1=1.0 - a, r2=h, c_r2=a)
        return self._lin2(hb, *d["proj_out"], self._res(rows, C, dev), r1=x, ld_r1=C)

    # ---------------- forward ----------------
    def forward_nhwc(self, x, timestep, encoder_hidden_states, added_time_ids, B, T, H, W_, taps=None):
        """x: fp16 [B*T*H*W, 64] channels-last (18 real channels, zero padded; with `self.in_split` = (lo_off, dup_off) the row is the split
        operand [x_hi | x_lo | x_hi 2^-10] that ops.nchw_f32_to_nhwc_f16(split=...) / ops.euler_cfg_step(split=...) write) -> fp16 [B*T*H*W, 4]."""
        cfg, Wt = self._cfg, self.w
        dev = x.device
        ops.streamk_init()      # stream-K workspace of this (device, stream): allocated here, never inside a launch / graph capture
        if getattr(self, "_gn_pool", None) is None or self._gn_pool.buf.device != dev:
            self._gn_pool = ops.WorkspacePool(dev)
        self._gn_pool.reset()
        boc = cfg["block_out_channels"]
        N = B * T
        # timestep / added-time-id embeddings: one ew_sinusoid_embed_f16 launch each (diffusers Timesteps; no torch elementwise kernels in a forward)
        ts = torch.as_tensor(timestep, dtype=torch.float32, device=dev).reshape(-1)
        t_emb = ops.sinusoid_embed(ts, B, boc[0])                          # one timestep broadcast over the batch rows, or one per row
        ids = added_time_ids if (added_time_ids.device == dev and added_time_ids.dtype == torch.float32) else added_time_ids.to(device=dev, dtype=torch.float32)
        a_emb = ops.sinusoid_embed(ids.reshape(-1).contiguous(), B * ids.shape[-1], cfg["addition_time_embed_dim"]).reshape(B, -1)
        h1 = ops.linear(t_emb, *Wt["te1"], act=ACT_SILU)
        h2 = ops.linear(a_emb, *Wt["ae1"], act=ACT_SILU)
        td = boc[0] * 4
        semb = torch.empty(B, td, dtype=torch.float16, device=dev)   # silu(emb): the only form emb is consumed in
        ops.gemm(h1, Wt["e2"][0], semb, M=B, N=td, c1=td, lda=td, a2=h2, c2=td, lda2=td, bias=Wt["e2"][1], act=ACT_SILU)
        tembs = ops.linear(semb, *Wt["temb"])         # all 44 time_emb_proj at once
        ehs = encoder_hidden_states.to(device=dev, dtype=torch.float16).reshape(B, -1).contiguous()
        cvecs = ops.linear(ehs, *Wt["cv"])            # all 32 cross-attention vectors at once

        h = self._conv3x3(x, *Wt["conv_in"], N, H, W_, H, W_, res_out=True)
        if taps is not None:
            taps["conv_in"] = (h.float(), H, W_)
        skips = [(h, H, W_)]
        for bi, blk in enumerate(self.arch.downs):
            for l, r in enumerate(blk.res):
                h = self._resblock(r, [h], tembs, B, T, H, W_)
                if blk.attn:
                    h = self._transformer(blk.attn[l], h, cvecs, B, T, H, W_)
                skips.append((h, H, W_))
            if blk.down:
                h = self._conv3x3(h.hi, *Wt[blk.down.p], N, H, W_, H // 2, W_ // 2, stride=2, res_out=True)
                H, W_ = H // 2, W_ // 2
                skips.append((h, H, W_))
            if taps is not None:
                taps[f"down{bi}"] = (h.float(), H, W_)
        m = self.arch.mid
        h = self._resblock(m.res[0], [h], tembs, B, T, H, W_)
        h = self._transformer(m.attn[0], h, cvecs, B, T, H, W_)
        h = self._resblock(m.res[1], [h], tembs, B, T, H, W_)
        if taps is not None:
            taps["mid"] = (h.float(), H, W_)
        for bi, blk in enumerate(self.arch.ups):
            for l, r in enumerate(blk.res):
                sk, sh, sw = skips.pop()
                assert (sh, sw) == (H, W_)
                h = self._resblock(r, [h, sk], tembs, B, T, H, W_)   # cat([hidden, skip], dim=1) by addressing
                if blk.attn:
                    h = self._transformer(blk.attn[l], h, cvecs, B, T, H, W_)
            if blk.up:
                wu, bu, form = Wt[blk.up.p]
                h = self._conv3x3(h.hi, wu, bu, N, H, W_, 2 * H, 2 * W_, upsample=form, res_out=True)
                H, W_ = 2 * H, 2 * W_
            if taps is not None:
                taps[f"up{bi}"] = (h.float(), H, W_)
        wco, bco = Wt["conv_out"]       # packed [W_hi | W_lo] (twice the input channels): the second block reads hn again;
        C0 = h.hi.shape[-1]             # or [W_hi | W_hi | W_lo] against the split rows [hn_hi | hn_lo] + hn_hi again
        blocks = wco.shape[1] // (9 * C0)
        hn = ops.groupnorm([h], *Wt["norm_out"], N, H * W_, 1e-5, True, pool=self._gn_pool, split_out=blocks == 3)
        return self._conv3x3(hn, wco, bco, N, H, W_, H, W_, x2=hn if blocks > 1 else None, c2=C0 if blocks > 1 else None)

    @torch.no_grad()
    def __call__(self, sample, timestep, encoder_hidden_states, added_time_ids, return_dict=True, taps=None):
        self._require_loaded()
        if sample.ndim != 5 or sample.shape[2] != self._cfg["in_channels"]:
            raise ValueError(f"sample must be [B,T,{self._cfg['in_channels']},h,w], got {tuple(sample.shape)}")
        B, T, C, H, W_ = sample.shape
        if H % 8 or W_ % 8:
            raise ValueError("latent height/width must be multiples of 8 (three stride-2 levels)")
        x = torch.zeros(B * T * H * W_, CPAD_IN, dtype=torch.float16, device=self.device)
        ops.nchw_f32_to_nhwc_f16(sample.to(device=self.device, dtype=torch.float32).reshape(B * T, C, H, W_).contiguous(),
                                 x, CPAD_IN, split=self.in_split)
        eps = self.forward_nhwc(x, timestep, encoder_hidden_states, added_time_ids, B, T, H, W_, taps=taps)
        oc = self._cfg["out_channels"]
        out = ops.nhwc_f16_to_nchw_f32(eps, B * T, oc, H, W_, oc).reshape(B, T, oc, H, W_)
        ops.streamk_check()     # a stream-K hand-over that timed out leaves a wrong tile: never return that silently
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)
