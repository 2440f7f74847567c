"""Times the device MJPEG encoder (csrc/video.hip) kernel by kernel on one clip of the episode's size, and Pillow's encoders on the same
frames for comparison.

  python tools/bench_video.py [--iters N] [--frames 25] [--height 576] [--width 1024] [--quality 90] [--out profiles/video_bench.json]

The clip: `frames` uint8 frames already on the device, synthetic (smooth gradients, a texture of sinusoids and noise of sigma 4: about
the compressibility of a rendered panorama).  Per sampling (4:2:0, 4:4:4): device events around `iters` calls of each kernel
(ew_jpeg_dct_quant, ew_jpeg_entropy, ew_jpeg_pack) with the bytes each must move at the least and that figure against the 8 TB/s of HBM;
a host clock around the synchronised video.encode_jpeg call, device-to-host copy and header assembly included; the compressed size.
Then the same frames through Pillow's Image.save as JPEG (same quality and sampling) and as PNG on this machine's CPU.  Prints one JSON
line and, with --out, writes it there.  No gate: these are measurements.

  python tools/bench_video.py --decode [--out profiles/video_decode_bench.json]

times the way back on the same clip: the clip's own JPEGs through ew_jpeg_huffman_decode, ew_jpeg_idct, ew_jpeg_planes_to_rgb
and ew_resize_linear_u8 (to 64 x 64), the synchronised video.decode_jpeg call, and Pillow's decode of the same bytes on the CPU."""
import argparse
import io
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0


def synthetic_clip(V, H, W, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.linspace(0, 1, H, device="cuda")[None, :, None]
    x = torch.linspace(0, 1, W, device="cuda")[None, None, :]
    t = torch.arange(V, device="cuda")[:, None, None] / max(V, 1)
    chans = []
    for c in range(3):
        base = 120 + 80 * torch.sin(6.3 * (x + 0.3 * c + t)) * torch.cos(3.1 * (y + 0.2 * c))
        tex = 25 * torch.sin(90 * x + 40 * y * (c + 1)) * torch.sin(70 * y - 20 * t)
        chans.append(base + tex + 4 * torch.randn(V, H, W, device="cuda", generator=g))
    return torch.stack(chans, dim=-1).clamp(0, 255).round().to(torch.uint8).contiguous()


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters            # microseconds per call


def stage(name, us, nbytes, note):
    return {"stage": name, "us": round(us, 1), "min_bytes": int(nbytes), "GBps": round(nbytes / us / 1e3, 1),
            "hbm_fraction": round(nbytes / us / 1e6 / HBM_TBS, 4), "note": note}


def decode_runs(clip, q, it):
    """--decode: the four decoder kernels (csrc/video_decode.hip) and the synchronised video.decode_jpeg call on the clip's own JPEGs, per
    sampling, next to Pillow's decode of the same bytes on this machine's CPU"""
    import numpy as np
    from PIL import Image

    from evoworld_amd import ops, video
    V, H, W, _ = clip.shape
    P = ops._ptr
    pixels = V * H * W * 3
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    runs = []
    for sub in video.SUBSAMPLINGS:
        mode, mcu, bpm = ops.JPEG_SAMPLING[sub]
        jpegs = video.encode_jpeg(clip, q, sub)
        info = video.parse_jpeg(jpegs[0])
        scan, starts, lengths = video.scan_batch(jpegs, info)
        base = len(scan)
        stream, seg_start, seg_bytes = dev(scan), dev(starts), dev(lengths)
        tables, qt = dev(video.huffman_device_tables(info["huffman"])), dev(np.stack(info["qtables"]).astype(np.uint8))
        mr, mc = -(-H // mcu), -(-W // mcu)
        coef, status = ops.jpeg_huffman_decode(stream, seg_start, seg_bytes, tables, V, mr, mc, bpm, info["restart_interval"])
        assert not bool(status.any())
        planes = ops.jpeg_idct(coef, qt)
        rgb = ops.jpeg_planes_to_rgb(planes, H, W, sub)
        small = ops.resize_linear_u8(rgb, 64, 64)
        n_seg, plane_bytes = len(lengths), sum(p.numel() for p in planes)
        stages = [
            stage("huffman_decode", timed(lambda: ops._call("ew_jpeg_huffman_decode", P(stream), base, P(seg_start), P(seg_bytes), P(tables), P(coef),
                                                            P(status), n_seg, V, mr, mc, bpm, info["restart_interval"]), it),
                  base + 2 * coef.numel() * 2, "scan bytes in; coefficients zeroed (memset), then written"),
            stage("idct", timed(lambda: ops._call("ew_jpeg_idct", P(coef), P(qt), P(planes[0]), P(planes[1]), P(planes[2]), V, mr, mc, bpm), it),
                  coef.numel() * 2 + plane_bytes, "int16 coefficients in, uint8 sample planes out"),
            stage("planes_to_rgb", timed(lambda: ops._call("ew_jpeg_planes_to_rgb", P(planes[0]), P(planes[1]), P(planes[2]), P(rgb), V, H, W, mode), it),
                  plane_bytes + pixels, "sample planes in, pixels out"),
            stage("resize_linear_64", timed(lambda: ops._call("ew_resize_linear_u8", P(rgb), P(small), V, H, W, 64, 64), it),
                  4 * small.numel() + small.numel(), "four taps per output value in, 64 x 64 out"),
        ]
        torch.cuda.synchronize()
        wall = []
        for _ in range(max(3, it // 2)):
            t0 = time.perf_counter()
            video.decode_jpeg(jpegs)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for j in jpegs:
            Image.open(io.BytesIO(j)).convert("RGB").load()
        pillow_ms = (time.perf_counter() - t0) * 1e3
        us = stages[0]["us"]
        runs.append({"subsampling": sub, "stages": stages, "kernels_us": round(sum(s["us"] for s in stages[:3]), 1),
                     "decode_jpeg_wall_ms": round(min(wall) * 1e3, 2), "pillow_decode_cpu_ms": round(pillow_ms, 1), "scan_bytes": base,
                     "segments": n_seg, "longest_segment_bytes": int(lengths.max()), "mean_segment_bytes": round(float(lengths.mean()), 1),
                     "huffman_ns_per_byte_of_the_longest_segment": round(us * 1e3 / int(lengths.max()), 2),
                     "huffman_lanes_in_flight": n_seg, "coef_bytes": coef.numel() * 2})
    return runs


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--frames", type=int, default=25)
    p.add_argument("--height", type=int, default=576)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--out", type=str, default=None)
    p.add_argument("--decode", action="store_true", help="time the decoder (csrc/video_decode.hip) on the same clip instead of the encoder")
    args = p.parse_args(argv)
    from PIL import Image

    from evoworld_amd import ops, video
    V, H, W, q, it = args.frames, args.height, args.width, args.quality, args.iters
    clip = synthetic_clip(V, H, W)
    if args.decode:
        rec = {"tool": "bench_video --decode", "device": torch.cuda.get_device_name(0), "frames": V, "height": H, "width": W, "quality": q,
               "iters": it, "pixel_bytes": V * H * W * 3, "hbm_TBps": HBM_TBS, "device_runs": decode_runs(clip, q, it),
               "note": "device events around whole kernel calls; decode_jpeg_wall_ms is the best synchronised call with the host's header parse "
                       "and segment table, the upload of the scan bytes and the status read-back; pillow_decode_cpu_ms is one single-threaded "
                       "pass over the same bytes on the host.  The Huffman kernel runs one lane per restart segment, 4 lanes per workgroup: "
                       "its time is the serial walk of the longest segment's bits (dependent byte loads, a table lookup and a scattered 2-byte "
                       "store per symbol), not bandwidth; huffman_ns_per_byte_of_the_longest_segment states that latency.  No gate."}
        line = json.dumps(rec)
        print(line)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(line + "\n")
        return
    P = ops._ptr
    pixels = V * H * W * 3
    runs = []
    for sub in video.SUBSAMPLINGS:
        mode = ops.JPEG_SAMPLING[sub][0]
        coef = ops.jpeg_dct_quant(clip, q, sub)
        _, mr, mc, bpm, _ = coef.shape
        slots, seg_bytes = ops.jpeg_entropy(coef)
        stream, frame_bytes = ops.jpeg_pack(slots, seg_bytes, mr)
        scan = int(stream.numel())
        sizes = seg_bytes.to(torch.int64).view(-1, mr) + 2
        sizes[:, -1] -= 2
        offsets = (torch.cumsum(sizes.view(-1), 0) - sizes.view(-1)).contiguous()
        n_seg, slot = slots.shape
        stages = [
            stage("dct_quant", timed(lambda: ops._call("ew_jpeg_dct_quant", P(clip), P(coef), V, H, W, q, mode), it),
                  pixels + coef.numel() * 2, "pixels in, int16 coefficients out"),
            stage("entropy", timed(lambda: ops._call("ew_jpeg_entropy", P(coef), P(slots), P(seg_bytes), n_seg, mc, bpm, slot), it),
                  coef.numel() * 2 * 2 + scan, "coefficients twice (length pass, coding pass), stuffed bytes out"),
            stage("pack", timed(lambda: ops._call("ew_jpeg_pack", P(slots), P(seg_bytes), P(offsets), P(stream), n_seg, mr, slot, scan), it),
                  2 * scan, "segments in, stream out"),
        ]
        torch.cuda.synchronize()
        wall = []
        for _ in range(max(3, it // 2)):
            t0 = time.perf_counter()
            jpegs = video.encode_jpeg(clip, q, sub)
            wall.append(time.perf_counter() - t0)
        runs.append({"subsampling": sub, "stages": stages, "kernels_us": round(sum(s["us"] for s in stages), 1),
                     "encode_jpeg_wall_ms": round(min(wall) * 1e3, 2), "coef_bytes": coef.numel() * 2, "slot_workspace_bytes": n_seg * slot,
                     "scan_bytes": scan, "jpeg_bytes": sum(len(j) for j in jpegs), "ratio_to_pixels": round(sum(len(j) for j in jpegs) / pixels, 4)})
    host = clip.cpu().numpy()
    cpu = {}
    for name, kw in (("jpeg_420", dict(format="JPEG", quality=q, subsampling=2)), ("jpeg_444", dict(format="JPEG", quality=q, subsampling=0)),
                     ("png", dict(format="PNG"))):
        t0 = time.perf_counter()
        nbytes = 0
        for f in host:
            b = io.BytesIO()
            Image.fromarray(f).save(b, **kw)
            nbytes += b.tell()
        cpu[name] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "bytes": nbytes}
    rec = {"tool": "bench_video", "device": torch.cuda.get_device_name(0), "frames": V, "height": H, "width": W, "quality": q, "iters": it,
           "pixel_bytes": pixels, "hbm_TBps": HBM_TBS, "device_runs": runs, "pillow_cpu": cpu,
           "note": "device events around whole kernel calls; encode_jpeg_wall_ms is the best synchronised call with its allocations, the cumsum, "
                   "the device-to-host copy and the header assembly; the split between kernels and launch gaps inside it, and the saving in "
                   "a real episode, are not measured; pillow_cpu is one pass over the same frames on the host, single-threaded"}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
