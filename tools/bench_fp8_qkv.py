#!/usr/bin/env python3
"""Times the opt-in fp8 (e4m3) q / k / v projections (UNet(qkv_fp8=True), BASELINE.json configs[4]) against the fp16 default.

  projections   per U-Net level (widths 320 / 640 / 1280 at the token counts of a B = 2, 25-frame, 72x128-latent forward): the spatial
                q|k projection (log2 prescale in the epilogue), V^T through swapped operands and the temporal fused qkv projection --
                fp16: three ew_gemm_f16 launches; fp8: two ew_quant_rows_fp8 passes (the spatial and the temporal LayerNorm output,
                COUNTED) + three ew_gemm_fp8 launches.  Device events around the group, the two variants alternating.
  forward       one full-size forward (real architecture, random weights, B = 2) at 72x128 latents x 25 frames and, unless
                --no-config5 or the allocation fails, configs[4]'s 128x256 x 49: host clock around a synchronised forward_nhwc, fp16 and
                fp8 models alternating, plus the rel-L2 distance between their outputs.

Nothing here is a speed claim: the non-scaled fp8 MFMA runs at the fp16 rate on gfx950, the path halves operand bytes only.

Usage:  python tools/bench_fp8_qkv.py [--out profiles/fp8_qkv_bench.json] [--iters 10] [--no-config5]
Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda"


def alternate_ms(fns, iters, warmup=2):
    """Median / min device-event milliseconds of each callable, the callables taking turns (A B A B ...) so that drift hits both"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [{"ms_median": float(np.median(t)), "ms_min": float(np.min(t))} for t in times]


def bench_projections(rows, C, iters):
    from evoworld_amd import ops
    g = torch.Generator(device=DEV).manual_seed(C)
    n1 = torch.randn(rows, C, generator=g, device=DEV).half()            # LayerNorm outputs: unit variance
    n1t = torch.randn(rows, C, generator=g, device=DEV).half()
    w = {k: (torch.randn(n * C, C, generator=g, device=DEV) / C ** 0.5).half() for k, n in (("qk", 2), ("v", 1), ("qkv", 3))}
    w8 = {k: ops.quant_rows_fp8(v) for k, v in w.items()}
    qk = torch.empty(rows, 2 * C, dtype=torch.float16, device=DEV)
    vt = torch.empty(C, rows, dtype=torch.float16, device=DEV)
    qkv = torch.empty(rows, 3 * C, dtype=torch.float16, device=DEV)

    def fp16():
        ops.linear(n1, w["qk"], out=qk, c_acc=ops.QK_LOG2_PRESCALE)
        ops.gemm(w["v"], n1, vt, M=C, N=rows, c1=C, lda=C)
        ops.linear(n1t, w["qkv"], out=qkv)

    def fp8():
        q, s = ops.quant_rows_fp8(n1)
        ops.gemm_fp8(q, s, *w8["qk"], out=qk, c_acc=ops.QK_LOG2_PRESCALE)
        ops.gemm_fp8(*w8["v"], q, s, out=vt)
        q, s = ops.quant_rows_fp8(n1t)
        ops.gemm_fp8(q, s, *w8["qkv"], out=qkv)

    def fp8_gemms_only(q=ops.quant_rows_fp8(n1), qt=ops.quant_rows_fp8(n1t)):
        ops.gemm_fp8(*q, *w8["qk"], out=qk, c_acc=ops.QK_LOG2_PRESCALE)
        ops.gemm_fp8(*w8["v"], *q, out=vt)
        ops.gemm_fp8(*qt, *w8["qkv"], out=qkv)

    r16, r8, r8g = alternate_ms([fp16, fp8, fp8_gemms_only], iters)
    flops = 2.0 * rows * C * 6 * C
    return {"rows": rows, "C": C, "fp16": r16, "fp8_with_quantisation": r8, "fp8_gemms_only": r8g,
            "fp16_TFps": flops / r16["ms_median"] / 1e9, "fp8_TFps": flops / r8["ms_median"] / 1e9,
            "fp8_over_fp16": r8["ms_median"] / r16["ms_median"]}


def bench_forward(models, B, T, h, w, iters):
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.zeros(B * T * h * w, 64, dtype=torch.float16, device=DEV)
    x[:, :18] = torch.randn(B * T * h * w, 18, generator=g, device=DEV).half()
    ehs = torch.randn(B, 1, 1024, generator=g, device=DEV).half()
    ehs[0] = 0
    ids = torch.tensor([[6.0, 127.0, 0.02]] * B, device=DEV)
    outs, times = {}, {k: [] for k in models}
    for it in range(iters + 1):                     # the first round is the warm-up
        for k, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = m.forward_nhwc(x, 1.234, ehs, ids, B, T, h, w)
            torch.cuda.synchronize()
            if it:
                times[k].append((time.perf_counter() - t0) * 1e3)
            outs[k] = o
    a, b = outs["fp16"].double(), outs["fp8"].double()
    rec = {"B": B, "T": T, "latent": [h, w], "finite": bool(torch.isfinite(outs["fp8"]).all()),
           "fp8_vs_fp16_rel_l2": float((b - a).norm() / a.norm())}
    for k, t in times.items():
        rec[k] = {"ms_median": float(np.median(t)), "ms_min": float(np.min(t))}
    rec["fp8_over_fp16"] = rec["fp8"]["ms_median"] / rec["fp16"]["ms_median"]
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-config5", action="store_true")
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args(argv)
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel, random_state_dict
    rec = {"device": torch.cuda.get_device_name(0), "projections": []}
    rows0 = 2 * 25 * 72 * 128
    for lvl, C in enumerate((320, 640, 1280)):
        rec["projections"].append(bench_projections(rows0 >> (2 * lvl), C, args.iters))
    if not args.no_forward:
        models = {}
        for k, flag in (("fp16", False), ("fp8", True)):
            m = UNetSpatioTemporalConditionModel(qkv_fp8=flag, num_frames=49)     # num_frames sizes nothing: one pair serves both shapes
            models[k] = m.load_state_dict(random_state_dict(m._cfg, 0, device=DEV), device=DEV)
        rec["fp8_blocks"] = len(models["fp8"].fp8_blocks)
        rec["forward_72x128x25"] = bench_forward(models, 2, 25, 72, 128, max(3, args.iters // 2))
        if not args.no_config5:
            try:
                rec["forward_128x256x49"] = bench_forward(models, 2, 49, 128, 256, 2)
            except torch.cuda.OutOfMemoryError as e:
                rec["forward_128x256x49"] = {"skipped": "out of memory: " + str(e).splitlines()[0]}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
