#!/usr/bin/env python3
"""Times the panorama -> cubemap conversion on the device next to a host numpy + PIL run of the same method.

  kernel   ew_equi2cube_u8 alone at 4096x2048 -> edge-1024 cross, V = 25 (bilinear and nearest); GB/s counts the input read once
           and the cross written once, against the 8 TB/s HBM peak
  method   Navigator.convert_panorama_to_cubemap on a 25-frame 2048x1024 clip at scale_factor 2 (LANCZOS up, cross, LANCZOS down)
  host     the reference's method for ONE 2048x1024 frame at scale_factor 2 on this machine's CPU, restated with numpy + PIL
           (tools/make_goldens_cubemap.py's own-words formula; the reference tree is not needed), so device and host times come
           from the same run on the same box

Usage:  python tools/bench_cubemap.py [--out FILE.json] [--iters 10] [--no-host]
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
HBM_PEAK = 8.0e12


def device_ms(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def host_convert(img, scale_factor):
    """convert_panorama_to_cubemap (bilinear) of one frame with numpy + PIL on the host"""
    from PIL import Image
    from tools.make_goldens_cubemap import source_coords
    h0, w0 = img.shape[:2]
    W = w0 * scale_factor
    px = np.asarray(Image.fromarray(img).resize((W, W // 2), Image.LANCZOS))
    uf, vf, used = source_coords(W)
    u0, v0 = np.floor(uf).astype(int), np.floor(vf).astype(int)
    mu, nu = (uf - u0)[..., None], (vf - v0)[..., None]
    cu, cv = (lambda t: np.clip(t, 0, W - 1)), (lambda t: np.clip(t, 0, W // 2 - 1))
    A, B, C, D = px[cv(v0), cu(u0)], px[cv(v0), cu(u0 + 1)], px[cv(v0 + 1), cu(u0)], px[cv(v0 + 1), cu(u0 + 1)]
    cross = (A * (1 - mu) * (1 - nu) + B * mu * (1 - nu) + C * (1 - mu) * nu + D * mu * nu).astype(np.uint8)
    cross[~used] = 0
    return np.asarray(Image.fromarray(cross).resize((w0, int(w0 * 3 / 4)), Image.LANCZOS)), cross


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args(argv)
    from evoworld_amd import ops
    from evoworld_amd import reprojection as RP
    rec = {"device": torch.cuda.get_device_name(0)}
    V, H, W = 25, 2048, 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty(V, 3 * W // 4, W, 3, dtype=torch.uint8, device="cuda")
    nbytes = x.numel() + out.numel()
    for name, interp in (("bilinear", True), ("nearest", False)):
        med, best = device_ms(lambda: ops.equi2cube(x, interp, out=out), args.iters)
        rec[f"kernel_{name}"] = {"shape": [V, H, W], "edge": W // 4, "ms_median": med, "ms_min": best, "bytes": nbytes,
                                 "GBps": nbytes / med / 1e6, "share_of_8TBps": nbytes / (med * 1e-3) / HBM_PEAK}
    del x, out
    clip = torch.randint(0, 256, (V, 1024, 2048, 3), dtype=torch.uint8, device="cuda", generator=g)
    med, best = device_ms(lambda: RP.panorama_to_cubemap(clip, True, 2), max(3, args.iters // 2), warmup=2)
    rec["method_clip25_2048x1024_s2"] = {"ms_median": med, "ms_min": best, "ms_per_frame": med / V}
    if not args.no_host:
        frame = clip[0].cpu().numpy()
        t0 = time.perf_counter()
        small, cross = host_convert(frame, 2)
        rec["host_numpy_one_frame_2048x1024_s2_s"] = time.perf_counter() - t0
        dev_small, dev_faces = RP.panorama_to_cubemap(clip[:1], True, 2)
        d = np.abs(dev_faces["front"][0].cpu().numpy().astype(int) - cross[1024:2048, 2048:3072].astype(int))
        rec["front_face_pixels_differing_from_host"] = int((d.max(-1) > 0).sum())
        rec["front_face_largest_difference"] = int(d.max())
        rec["speedup_per_frame"] = rec["host_numpy_one_frame_2048x1024_s2_s"] * 1e3 / (med / V)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
