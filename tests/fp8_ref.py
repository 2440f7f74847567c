"""CPU reference of the opt-in fp8 (OCP e4m3) q / k / v projection path, in fp32 PyTorch (no GPU, no project kernels):
  quant_rows / deq     the row-wise quantiser of ew_quant_rows_fp8 and its inverse;
  fake_quant_unet      the path's arithmetic restated on the fp32 oracle: forward hooks on to_q / to_k / to_v of every
                       self-attention `Attention` module whose width is a multiple of 64 replace the Linear's input and weight by
                       their row-wise e4m3 fake-quantised values (one scale per token row, one per weight row).  The cross-attention
                       modules (attn2: one key/value token, folded away in the product) are left alone.
Shared by tests/test_cpu_fp8_qkv.py and tests/test_gpu_fp8_qkv.py."""
import torch

FP8_MAX = 448.0     # largest finite e4m3fn value


def quant_rows(x):
    """x [rows, K] (any float dtype) -> (uint8 [rows, K] e4m3 bytes, fp32 scale [rows]): s = amax / 448 (1 for an all-zero row),
    bytes = e4m3(x * (1 / s)), round to nearest even."""
    x = x.float()
    amax = x.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax))
    q = (x * (1.0 / s)[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), s


def deq(q, s):
    """e4m3 bytes uint8 [rows, K], fp32 scale [rows] -> fp32 [rows, K]"""
    return q.view(torch.float8_e4m3fn).float() * s.float()[:, None]


def fake_quant(x):
    """Row-wise (last dim) e4m3 fake quantisation of a tensor of any rank, fp32 out"""
    flat = x.reshape(-1, x.shape[-1])
    return deq(*quant_rows(flat)).reshape(x.shape)


def self_attention_modules(ref):
    """(name, module) of every self-attention Attention of the oracle U-Net (attn1: keys and values come from the tokens themselves)"""
    from oracle.unet_ref import Attention
    return [(n, m) for n, m in ref.named_modules()
            if isinstance(m, Attention) and n.endswith(".attn1") and m.to_k.in_features == m.to_q.in_features]


def fake_quant_unet(ref):
    """Register the fake-quantisation hooks on `ref` (an oracle.unet_ref.UNetSpatioTemporalConditionModelRef).  Returns
    (handles, names): remove the handles to get the plain oracle back; names lists the hooked Attention modules."""
    handles, names = [], []

    def pre(mod, args):                  # input rows and weight rows -> their e4m3 fake-quantised values for this call
        mod._fp8_plain_weight = mod.weight.data
        mod.weight.data = mod._fp8_weight
        return (fake_quant(args[0]),) + tuple(args[1:])

    def post(mod, args, out):
        mod.weight.data = mod._fp8_plain_weight
        del mod._fp8_plain_weight

    for name, attn in self_attention_modules(ref):
        if attn.to_q.in_features % 64:
            continue
        names.append(name)
        for lin in (attn.to_q, attn.to_k, attn.to_v):
            lin._fp8_weight = fake_quant(lin.weight.data)
            handles.append(lin.register_forward_pre_hook(pre))
            handles.append(lin.register_forward_hook(post))
    return handles, names
