"""Times the device PNG encoder (csrc/png.hip, evoworld_amd/png.py) kernel by kernel on the frames tools/bench_video.py uses, Pillow's PNG
writer on the same frames, and -- with --episode -- one --save_frames episode with and without --device_png.

  python tools/bench_png.py [--iters 10] [--frames 25] [--height 576] [--width 1024] [--episode] [--out profiles/png_bench.json]

The clip: bench_video.synthetic_clip (gradients, a texture of sinusoids, noise of sigma 4).  Device events around `iters` calls of each
entry (ew_png_filter with its Adler kernel, ew_png_lz77, ew_png_emit) with the bytes each must move at the least and that figure against
the 8 TB/s of HBM; a host clock around the synchronised png.encode_png call, split into the kernels (their event times), the host's table
building (timed alone) and the rest (torch plumbing, two synchronisations, copies, CRC-32 and framing); the file sizes.  Then the same
frames through Pillow's Image.save as PNG on this machine's CPU, one thread.  `ratios`: file size over Pillow's on the three 256 x 512
frames of tests/test_gpu_png.py.  --episode: the 3-segment synthetic episode of unified_loop_consistency.py (--random_init --curve_path
--save_frames) in this process, once with Pillow and once with --device_png after a short warm-up run: wall time of each and the
number of PNG files written.  Prints one JSON line and, with --out, writes it there.  No gate and no speed claim: these are
measurements."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_video import HBM_TBS, stage, synthetic_clip, timed  # noqa: E402


def pillow_png(frames):
    from PIL import Image
    t0 = time.perf_counter()
    nbytes = 0
    for f in frames:
        b = io.BytesIO()
        Image.fromarray(f).save(b, "PNG")
        nbytes += b.tell()
    return {"ms": round((time.perf_counter() - t0) * 1e3, 1), "bytes": nbytes}


def ratios():
    """the three measured ratios of tests/test_gpu_png.py (256 x 512 gradient / texture / sigma-4 noise)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import png_cases as C
    from evoworld_amd import png
    out = {}
    for name in ("gradient", "texture", "noise4"):
        frame = C.CONTENTS[name](256, 512)
        ours = len(png.encode_png(torch.from_numpy(frame).cuda())[0])
        theirs = pillow_png([frame])["bytes"]
        out[name] = {"bytes": ours, "pillow_bytes": theirs, "ratio": round(ours / theirs, 4)}
    return out


def count_png(root):
    return sum(1 for _, _, files in os.walk(root) for f in files if f.endswith(".png"))


def episode_ab(segments, steps):
    import unified_loop_consistency as cli
    from evoworld_amd.pipeline import StableVideoDiffusionPipeline
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel
    dev = "cuda:0"
    unet = UNetSpatioTemporalConditionModel.from_random(seed=42, device=dev, num_frames=25)
    pipe = StableVideoDiffusionPipeline(unet=unet)
    out = {"segments": segments, "num_inference_steps": steps, "height": 576, "width": 1024}
    with tempfile.TemporaryDirectory() as tmp:
        base = ["--unet_path", "none", "--random_init", "--curve_path", "--base_folder", os.path.join(tmp, "no_such_folder")]
        warm = cli.parse_arguments(base + ["--num_segments", "1", "--num_inference_steps", "1", "--save_dir", os.path.join(tmp, "warm")])
        cli.run_episode(warm, "synthetic_000", pipe, unet, dev, os.path.join(tmp, "warm"), True)
        for key, flags in (("pillow", []), ("device_png", ["--device_png"])):
            d = os.path.join(tmp, key)
            os.makedirs(d)
            args = cli.parse_arguments(base + ["--num_segments", str(segments), "--num_inference_steps", str(steps), "--save_frames",
                                               "--save_dir", d] + flags)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec = cli.run_episode(args, "synthetic_000", pipe, unet, dev, d, True)
            torch.cuda.synchronize()
            out[key] = {"wall_s": round(time.perf_counter() - t0, 3), "process_episode_s": rec["seconds"], "png_files": count_png(d),
                        "png_bytes": sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(d) for f in fs if f.endswith(".png"))}
    out["saved_s"] = round(out["pillow"]["wall_s"] - out["device_png"]["wall_s"], 3)
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--frames", type=int, default=25)
    p.add_argument("--height", type=int, default=576)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--episode", action="store_true", help="also run the 3-segment --save_frames episode with and without --device_png")
    p.add_argument("--episode_segments", type=int, default=3)
    p.add_argument("--episode_steps", type=int, default=25)
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args(argv)
    from evoworld_amd import ops, png
    V, H, W, it = args.frames, args.height, args.width, args.iters
    clip = synthetic_clip(V, H, W)
    P = ops._ptr
    pixels = V * H * W * 3
    rps = ops.png_rows_per_segment(H, W)
    spf = -(-H // rps)
    filtered, adler = ops.png_filter(clip, "adaptive", rps)
    tokens, n_tokens, hist = ops.png_lz77(filtered, rps)
    t0 = time.perf_counter()
    tables = [png.FrameTables(h) for h in hist.view(V, spf, -1).sum(dim=1).cpu().numpy()]
    tables_ms = (time.perf_counter() - t0) * 1e3
    luts, headers, header_bits = png.upload_tables(tables, clip.device)
    mode, seg_bytes, offsets, frame_bytes = png.segment_sizes(hist, tables, V, H, W, rps)
    total = int(frame_bytes.sum())
    out = torch.empty(total, dtype=torch.uint8, device=clip.device)
    n_tok = int(n_tokens.sum())
    stride = tokens.shape[1]
    stages = [
        stage("filter+adler", timed(lambda: ops._call("ew_png_filter", P(clip), P(filtered), P(adler), V, H, W, ops.PNG_FILTERS["adaptive"], rps), it),
              pixels + 2 * filtered.numel(), "pixels in, filtered rows out, filtered rows in again for the Adler halves"),
        stage("lz77", timed(lambda: ops._call("ew_png_lz77", P(filtered), P(tokens), P(n_tokens), P(hist), V, H, W, rps, stride), it),
              filtered.numel() + 4 * n_tok + hist.numel() * 4, "filtered rows in, tokens and histograms out"),
        stage("emit", timed(lambda: ops._call("ew_png_emit", P(tokens), P(n_tokens), P(filtered), P(mode), P(offsets), P(seg_bytes), P(luts),
                                              P(headers), P(header_bits), headers.shape[1], P(out), total, V, H, W, rps, stride), it),
              4 * n_tok + total, "tokens in, the final stream out"),
    ]
    torch.cuda.synchronize()
    wall = []
    for _ in range(max(3, it // 2)):
        t0 = time.perf_counter()
        files = png.encode_png(clip)
        wall.append(time.perf_counter() - t0)
    kernels_ms = sum(s["us"] for s in stages) / 1e3
    best = min(wall) * 1e3
    rec = {"tool": "bench_png", "device": torch.cuda.get_device_name(0), "frames": V, "height": H, "width": W, "iters": it,
           "pixel_bytes": pixels, "hbm_TBps": HBM_TBS, "rows_per_segment": rps, "segments": V * spf,
           "segment_bytes": rps * (1 + 3 * W), "stored_segments": int(mode.sum()), "tokens": n_tok,
           "token_workspace_bytes": tokens.numel() * 4, "stages": stages, "kernels_ms": round(kernels_ms, 2),
           "encode_png_wall_ms": round(best, 2), "host_tables_ms": round(tables_ms, 2),
           "rest_ms": round(best - kernels_ms - tables_ms, 2), "png_bytes": sum(len(f) for f in files),
           "ratio_to_pixels": round(sum(len(f) for f in files) / pixels, 4), "pillow_cpu_png": pillow_png(clip.cpu().numpy()),
           "ratios_256x512": ratios(),
           "note": "device events around whole entry calls; encode_png_wall_ms is the best synchronised call with its allocations, the host's "
                   "Huffman tables (host_tables_ms, timed alone), torch's sums and scans, two synchronisations, the device-to-host copy, "
                   "CRC-32 and framing (rest_ms = wall - kernels - tables); lz77 and emit run one lane per segment, so their time is the "
                   "serial walk of a segment (dependent loads), not bandwidth; pillow_cpu_png is one single-threaded pass over the same "
                   "frames on the host.  No gate."}
    rec["ratio_to_pillow"] = round(rec["png_bytes"] / rec["pillow_cpu_png"]["bytes"], 4)
    if args.episode:
        rec["episode_ab"] = episode_ab(args.episode_segments, args.episode_steps)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
