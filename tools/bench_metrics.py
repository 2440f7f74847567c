#!/usr/bin/env python3
"""PSNR / SSIM evaluation on the MI355X: kernel time per 25-frame 576x1024 pair and the CLI end to end.

  python tools/bench_metrics.py kernel [--iters N]        ew_video_metrics on 25 seeded uint8 frame pairs (event-timed; run under
                                                           `rocprofv3 --kernel-trace --stats` for the per-kernel split); input
                                                           GB/s = 2 x 25 x 576 x 1024 x 3 bytes over the call time, against 8 TB/s
  python tools/bench_metrics.py cli --root DIR [--episodes 20]   writes DIR/ep_NNN/{predictions_gt_0,predictions_0}/001..025.png and
                                                           times evoworld_amd.metrics over them: PNG decode vs device seconds
  python tools/bench_metrics.py episode --root DIR [--poses 80]  writes a seeded episode tree DIR/case_000 (camera_poses.txt and
                                                           panorama/NNN.png, 500x1000) for run_unified_pipeline.sh BASE_FOLDER=DIR
  python tools/bench_metrics.py --lpips [--iters N] [--cpu_baseline]   LPIPS (AlexNet, seeded random weights) of the same 25 pairs through
                                                           evoworld_amd.lpips: ms per clip, host clock around a synchronised call; with
                                                           --cpu_baseline the same clip once through the fp32 PyTorch restatement
                                                           (tests/lpips_ref.py) on this machine's CPU, and the two results compared
  python tools/bench_metrics.py --fvd [--iters N]          FVD's I3D (seeded random weights) on one 25-frame 576x1024 uint8 clip through
                                                           evoworld_amd.fvd: ms for the clip's 16 clip lengths 10..25 (one preprocess, 16
                                                           passes: what the CLI spends per episode and set) and ms for the 25-frame pass
                                                           alone, host clock around synchronised calls
  python tools/bench_metrics.py --latent_mse [--iters N]   the latent MSE's Inception-v4 (seeded random weights) on the same 25 pairs through
                                                           evoworld_amd.latent_mse: ms for the features of both clips (50 frames: what the
                                                           CLI spends per episode for latent_mse and loop_closure_latent_mse together),
                                                           host clock around synchronised calls
  python tools/bench_metrics.py --ws [--iters N]           ew_video_metrics_ws (latitude weights) and ew_video_metrics on the same 25 uint8
                                                           pairs in one process, event-timed as `kernel` is; writes both to
                                                           profiles/ws_metrics_bench.json.  No speed gate
Each mode prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F, H, W = 25, 576, 1024
HBM_TBS = 8.0


def seeded_pair(seed, F_=F, H_=H, W_=W):
    """ground truth: smooth moving pattern; generated: the same plus noise of a few levels (device uint8 [F,H,W,3] each)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.arange(H_, device="cuda", dtype=torch.float32)[:, None, None]
    x = torch.arange(W_, device="cuda", dtype=torch.float32)[None, :, None]
    c = torch.arange(3, device="cuda", dtype=torch.float32)[None, None, :]
    frames = [(128 + 100 * torch.sin(0.011 * x * (c + 1) + 0.017 * y + 0.3 * f + seed)).round().clamp(0, 255) for f in range(F_)]
    gt = torch.stack(frames).to(torch.uint8)
    noise = torch.randint(-8, 9, gt.shape, device="cuda", generator=g, dtype=torch.int16)
    gen = (gt.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
    return gt.contiguous(), gen.contiguous()


def bench_kernel(iters):
    from evoworld_amd import ops
    gt, gen = seeded_pair(0)
    sse = torch.empty(F, dtype=torch.float64, device="cuda")
    ssim = torch.empty(F, dtype=torch.float64, device="cuda")
    for _ in range(5):
        ops.video_metrics(gt, gen, sse=sse, ssim=ssim)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.video_metrics(gt, gen, sse=sse, ssim=ssim)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    nbytes = 2 * F * H * W * 3
    return {"mode": "kernel", "frames": F, "shape": [H, W, 3], "us_per_call": round(us, 1), "us_per_frame": round(us / F, 2),
            "input_GBps": round(nbytes / us / 1e3, 1), "hbm_fraction": round(nbytes / us / 1e6 / HBM_TBS, 4), "iters": iters,
            "note": "event-timed call (both kernels + the workspace allocation); kernel time: rocprofv3 --kernel-trace --stats"}


def bench_ws(iters):
    from evoworld_amd import metrics as M, ops
    gt, gen = seeded_pair(0)
    w = M.latitude_weights(H)
    out = [torch.empty(F, dtype=torch.float64, device="cuda") for _ in range(2)]

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters
    us = {}
    for rnd in range(2):                                                       # planar, weighted, planar, weighted: the second round is reported
        us["planar"] = timed(lambda: ops.video_metrics(gt, gen, sse=out[0], ssim=out[1]))
        us["weighted"] = timed(lambda: ops.video_metrics_ws(gt, gen, w, wsse=out[0], wssim=out[1]))
    rec = {"mode": "ws", "frames": F, "shape": [H, W, 3], "iters": iters,
           "ew_video_metrics_us_per_call": round(us["planar"], 1), "ew_video_metrics_ws_us_per_call": round(us["weighted"], 1),
           "ratio": round(us["weighted"] / us["planar"], 3),
           "note": "event-timed calls through ops (both kernels + the workspace allocation; the weighted call also validates its 576 "
                   "weights on the host and uploads them, per call)"}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ws_metrics_bench.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return rec


def bench_lpips(iters, cpu_baseline):
    from evoworld_amd.lpips import LPIPSAlex, random_state_dict
    sd = random_state_dict(0)
    model = LPIPSAlex.from_state_dict(sd, "cuda")
    gt, gen = seeded_pair(0)
    for _ in range(2):
        out = model(gt, gen, "bgr")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = model(gt, gen, "bgr")
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    rec = {"mode": "lpips", "frames": F, "shape": [H, W, 3], "ms_per_clip": round(ms, 2), "ms_per_pair": round(ms / F, 3), "iters": iters,
           "lpips_mean": float(out.mean()), "weights": "random (seed 0)", "chunk_pairs": model.chunk,
           "note": "host clock around the whole call (uint8 frames already on the device), synchronised"}
    if cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import lpips_ref
        a, b = (t.cpu().permute(0, 3, 1, 2).float() / 255.0 for t in (gt, gen))
        t0 = time.perf_counter()
        ref = lpips_ref.lpips_alex(a, b, sd, channel_order="bgr")
        rec["cpu_restatement_ms_per_clip"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["cpu_threads"] = torch.get_num_threads()
        rec["max_rel_err_vs_cpu"] = float(((out.cpu() - ref.double()).abs() / ref.double().abs()).max())
    return rec


def bench_fvd(iters):
    from evoworld_amd import fvd as V
    model = V.I3D.from_random(0, "cuda")
    clip, _ = seeded_pair(0)

    def timed(fn):
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / iters, out
    ms_all, feats = timed(lambda: V.clip_features(model, clip, "bgr"))
    ms_one, logits = timed(lambda: model.logits(clip, channel_order="bgr"))
    return {"mode": "fvd", "frames": F, "shape": [H, W, 3], "clip_lengths": [min(feats), max(feats)], "ms_per_clip_all_lengths": round(ms_all, 2),
            "ms_per_25_frame_pass": round(ms_one, 2), "iters": iters, "logits_abs_mean": float(logits.abs().mean()), "weights": "random (seed 0)",
            "patch_row_cap_MiB": model.workspace_bytes >> 20,
            "note": "host clock around the whole call (uint8 frames already on the device), synchronised; the all-lengths figure includes "
                    "the 16 device-to-host copies of 400 logits"}


def bench_latent_mse(iters):
    from evoworld_amd import latent_mse as L
    model = L.InceptionV4.from_random(0, "cuda")
    gt, gen = seeded_pair(0)

    def both():
        return model.features(gt, "bgr"), model.features(gen, "bgr")
    for _ in range(2):
        f1, f2 = both()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        f1, f2 = both()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    res = L.latent_mse_result(f1.cpu()[None], f2.cpu()[None], torch.Size([F, 3, L.SIDE, L.SIDE]))
    return {"mode": "latent_mse", "frames": F, "shape": [H, W, 3], "ms_per_clip_pair": round(ms, 2), "ms_per_frame": round(ms / (2 * F), 3),
            "iters": iters, "latent_mse_mean": res["value_mean"], "loop_closure_latent_mse": res["value"][F - 1], "weights": "random (seed 0)",
            "chunk_frames": model.chunk,
            "note": "host clock around the features of both clips (uint8 frames already on the device; each call ends in streamk_check, "
                    "which synchronises)"}


def write_cli_tree(root, episodes):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    jobs = []
    for e in range(episodes):
        gt, gen = (t.cpu().numpy() for t in seeded_pair(e + 1))
        for sub, v in (("predictions_gt_0", gt), ("predictions_0", gen)):
            d = os.path.join(root, f"ep_{e:03d}", sub)
            os.makedirs(d, exist_ok=True)
            jobs += [(v[t], os.path.join(d, f"{t + 1:03}.png")) for t in range(F)]
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(lambda j: Image.fromarray(j[0]).save(j[1], compress_level=1), jobs))


def bench_cli(root, episodes):
    from evoworld_amd import metrics as M
    t0 = time.perf_counter()
    write_cli_tree(root, episodes)
    t_write = time.perf_counter() - t0
    argv = ["--data_path", root, "--gt_subdir", "predictions_gt_0", "--gen_subdir", "predictions_0", "--num_videos", str(episodes)]
    M.evaluate(M.parse_args(argv + ["--num_videos", "1"]))                    # warm-up: library load, first launches
    t0 = time.perf_counter()
    res, timing = M.evaluate(M.parse_args(argv))
    total = time.perf_counter() - t0
    return {"mode": "cli", "episodes": timing["episodes"], "frame_pairs": timing["frames"], "seconds_total": round(total, 3),
            "seconds_png_decode": round(timing["decode_s"], 3), "seconds_device": round(timing["device_s"], 3),
            "decode_fraction": round(timing["decode_s"] / total, 3), "psnr_mean": res["psnr"]["value_mean"],
            "ssim_mean": res["ssim"]["value_mean"], "seconds_writing_tree": round(t_write, 1),
            "note": "device = host->device copy + both kernels + the per-frame results back, per episode"}


def write_episode(root, poses):
    from PIL import Image
    ep = os.path.join(root, "case_000")
    os.makedirs(os.path.join(ep, "panorama"), exist_ok=True)
    with open(os.path.join(ep, "camera_poses.txt"), "w") as f:                # Unity convention, one straight walk with a slow turn
        f.write("Frame,PosX,PosY,PosZ,RotX,RotY,RotZ\n")
        x = z = 0.0
        for i in range(poses):
            yaw = 10.0 + 0.5 * i
            if i:
                x, z = x + 0.4 * np.sin(np.deg2rad(yaw)), z + 0.4 * np.cos(np.deg2rad(yaw))
            f.write(f"{i + 1},{float(x)!r},1.78,{float(z)!r},0.0,{yaw!r},0.0\n")
    yy, xx = np.mgrid[0:500, 0:1000]
    for i in range(1, poses + 1):
        img = np.stack([(128 + 100 * np.sin(0.013 * (xx + 9 * i) * (c + 1) + 0.02 * yy)) for c in range(3)], -1)
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(ep, "panorama", f"{i:03}.png"), compress_level=1)
    return {"mode": "episode", "episode": ep, "poses": poses}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", nargs="?", choices=["kernel", "cli", "episode"])
    p.add_argument("--lpips", action="store_true", help="time LPIPS (random weights) on a 25-pair 576x1024 clip")
    p.add_argument("--fvd", action="store_true", help="time FVD's I3D (random weights) on a 25-frame 576x1024 clip")
    p.add_argument("--latent_mse", action="store_true", help="time the latent MSE's Inception-v4 (random weights) on a 25-pair 576x1024 clip")
    p.add_argument("--ws", action="store_true", help="time ew_video_metrics_ws against ew_video_metrics on a 25-pair 576x1024 clip")
    p.add_argument("--cpu_baseline", action="store_true", help="with --lpips: also run the clip through tests/lpips_ref.py on the CPU")
    p.add_argument("--iters", type=int, default=None, help="timed calls (default: 50 for kernel and --ws, 5 for --lpips, --fvd and --latent_mse)")
    p.add_argument("--root", help="directory the cli / episode modes write their PNG trees to")
    p.add_argument("--episodes", type=int, default=20)
    p.add_argument("--poses", type=int, default=80)
    a = p.parse_args()
    if (a.lpips + a.fvd + a.latent_mse + a.ws + (a.mode is not None)) != 1:
        p.error("give one of kernel / cli / episode, or --lpips, or --fvd, or --latent_mse, or --ws")
    if a.ws:
        rec = bench_ws(a.iters or 50)
    elif a.latent_mse:
        rec = bench_latent_mse(a.iters or 5)
    elif a.fvd:
        rec = bench_fvd(a.iters or 5)
    elif a.lpips:
        rec = bench_lpips(a.iters or 5, a.cpu_baseline)
    elif a.mode == "kernel":
        rec = bench_kernel(a.iters or 50)
    elif a.mode == "cli":
        rec = bench_cli(a.root, a.episodes)
    else:
        rec = write_episode(a.root, a.poses)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
