"""Times the plane-sweep stereo stage (csrc/mvs.hip, evoworld_amd/mvs.py) entry by entry at the sizes the N-segment loop
hands it: 25 and 73 perspective views of 384 x 512 (the hand-offs after segments 0 and 2).

  python tools/bench_mvs.py [--iters 3] [--views 25 73] [--planes 64] [--sources 4] [--patch_radius 2] [--out profiles/mvs_bench.json]
  python tools/bench_mvs.py --sphere [...]      the sphere-sweep stage (csrc/mvs_sphere.hip) on 25 and 73 PANORAMAS of
                                                576 x 1024: ew_mvs_sphere_sweep, ew_mvs_sphere_consistency, ew_pano_unproject
                                                (default --out profiles/mvs_sphere_bench.json)
  python tools/bench_mvs.py --sgm [--sphere] [--sgm_paths 4]    the opt-in semi-global path (csrc/mvs_sgm.hip) at the same
                                                shapes, in the chunks of views the stage classes use: ew_mvs_*_sweep_volume,
                                                ew_mvs_sgm_aggregate, ew_mvs_sgm_select, and their sum against the fused sweep timed in
                                                the same run (default --out profiles/mvs_sgm_bench.json, one entry per sweep kind)
  python tools/bench_mvs.py --zncc              the opt-in ZNCC matching cost (csrc/mvs_zncc.hip): its four entries next to
                                                their SAD twins, in one process and on the same inputs -- 25 views of 384 x 512 and 25
                                                panoramas of 288 x 512, 64 hypotheses, 4 sources, patch radius 2 (default --out
                                                profiles/mvs_zncc_bench.json)

The views: bench_video.synthetic_clip (gradients, a texture of sinusoids, noise of sigma 4) -- the timing does not depend on what the
sweep finds -- at the poses view_poses gives for the curved synthetic episode of unified_loop_consistency.py.  Device events around
`iters` calls of each entry (ew_mvs_luma_u8, ew_mvs_plane_sweep, ew_mvs_consistency) with the bytes each must move at the least and,
for the sweep, the warped samples it evaluates (views x pixels x planes x present sources, the tile halos not counted); a host clock
around the synchronised PlaneSweepDepth call, which adds sweep_setup's float64 homographies on the host and the uploads.  Prints one
JSON line and, with --out, writes it there.  No gate and no speed claim: these are measurements."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_video import HBM_TBS, stage, synthetic_clip, timed  # noqa: E402


def run(V, H, W, D, S, r, it):
    import unified_loop_consistency as cli
    from evoworld_amd import mvs, ops
    seg = max(0, (V - 25) // 24)
    cam = cli.synthetic_episode(max(V, 24 * (seg + 2) + 8))
    clip = synthetic_clip(V, H, W)
    w2c = mvs.view_poses(cam, V, seg)
    K = mvs.pinhole(H, W)
    t0 = time.perf_counter()
    st = mvs.sweep_setup(w2c, K, S, D)
    setup_ms = (time.perf_counter() - t0) * 1e3
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    homog, src, invd, pose = up(st.homographies_f32), up(st.src_index), up(st.inv_depth_f32), up(st.rel_pose_f32)
    grey = ops.mvs_luma(clip)
    depth, conf, win, cost = ops.mvs_plane_sweep(grey, homog, src, invd, r, 48.0)
    P = ops._ptr
    px = V * H * W
    samples = int((st.src_index >= 0).sum(1).astype(np.int64).sum()) * H * W * D
    stages = [
        stage("luma", timed(lambda: ops._call("ew_mvs_luma_u8", P(clip), P(grey), V, H, W), it), 4 * px, "RGB in, grey out"),
        stage("plane_sweep", timed(lambda: ops._call("ew_mvs_plane_sweep", P(grey), P(homog), P(src), P(invd), P(depth), P(conf), P(win), P(cost),
                                                     V, H, W, S, D, r, 48.0), it),
              px + 16 * px + homog.numel() * 4, "grey in once, four planes out, the homographies; the gathers from the sources hit the caches"),
        stage("consistency", timed(lambda: ops._call("ew_mvs_consistency", P(depth), P(pose), P(src), P(conf), V, H, W, S, float(K[0, 0]), float(K[1, 1]),
                                                     float(K[0, 2]), float(K[1, 2]), 0.02, 2), it),
              8 * px, "depth and confidence in, confidence out; one gathered depth per present source"),
    ]
    sweep_us = stages[1]["us"]
    stage_obj = mvs.PlaneSweepDepth(n_src=S, planes=D, patch_radius=r)
    wall = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stage_obj(clip, view_w2c=w2c)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    return {"views": V, "height": H, "width": W, "planes": D, "sources": S, "patch_radius": r, "segment": seg, "stages": stages,
            "warped_samples": samples, "sweep_Gsamples_per_s": round(samples / sweep_us / 1e3, 2), "kernels_ms": round(sum(s["us"] for s in stages) / 1e3, 2),
            "host_setup_ms": round(setup_ms, 1), "stage_call_wall_ms": round(min(wall) * 1e3, 1), "homography_bytes": homog.numel() * 4}


def run_sphere(V, H, W, D, S, r, it):
    import unified_loop_consistency as cli
    from evoworld_amd import mvs, ops
    seg = max(0, (V - 25) // 24)
    cam = cli.synthetic_episode(max(V, 24 * (seg + 2) + 8))
    clip = synthetic_clip(V, H, W)
    w2c = mvs.pano_poses(cam, V, seg)
    t0 = time.perf_counter()
    st = mvs.sphere_setup(w2c, W, S, D)
    setup_ms = (time.perf_counter() - t0) * 1e3
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src, invd, pose = up(st.src_index), up(st.inv_dist_f32), up(st.rel_pose_f32)
    c2w = up(np.linalg.inv(mvs._w2c_4x4(w2c))[:, :3, :4].astype(np.float32))
    grey = ops.mvs_luma(clip)
    dist, conf, win, cost = ops.mvs_sphere_sweep(grey, pose, src, invd, r)
    xyz = ops.pano_unproject(dist, c2w)
    P = ops._ptr
    px = V * H * W
    samples = int((st.src_index >= 0).sum(1).astype(np.int64).sum()) * H * W * D
    stages = [
        stage("sphere_sweep", timed(lambda: ops._call("ew_mvs_sphere_sweep", P(grey), P(pose), P(src), P(invd), P(dist), P(conf), P(win), P(cost),
                                                      V, H, W, S, D, r), it),
              px + 16 * px, "grey in once, four planes out; the gathers from the sources hit the caches"),
        stage("sphere_consistency", timed(lambda: ops._call("ew_mvs_sphere_consistency", P(dist), P(pose), P(src), P(conf), V, H, W, S, 0.02, 2), it),
              8 * px, "distance and confidence in, confidence out; one gathered distance per present source"),
        stage("pano_unproject", timed(lambda: ops._call("ew_pano_unproject", P(dist), P(c2w), P(xyz), V, H, W), it), 16 * px,
              "distance in, three coordinates out"),
    ]
    sweep_us = stages[0]["us"]
    stage_obj = mvs.SphereSweepDepth(n_src=S, planes=D, patch_radius=r)
    wall = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stage_obj(clip, pano_w2c=w2c)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    return {"panoramas": V, "height": H, "width": W, "hypotheses": D, "sources": S, "patch_radius": r, "segment": seg, "stages": stages,
            "warped_samples": samples, "sweep_Gsamples_per_s": round(samples / sweep_us / 1e3, 2), "kernels_ms": round(sum(s["us"] for s in stages) / 1e3, 2),
            "host_setup_ms": round(setup_ms, 1), "stage_call_wall_ms": round(min(wall) * 1e3, 1)}


def run_sgm(V, H, W, D, S, r, it, sphere, paths, p1=1.0, p2=8.0, cost_scale=32.0, workspace_bytes=2 << 30):
    """volume -> aggregate -> select over all V views in the chunks sgm_sweep uses, each stage timed over all its chunks; the fused sweep
    of the same inputs is timed in the same run.  Least bytes: the volume is written once (2 B per cell) next to the grey image read;
    the aggregation must read the cost and write agg once (2 B + 2 B per cell: the floor DESIGN.md 4.10 sets its passes against); the
    select reads agg once and writes four planes."""
    import unified_loop_consistency as cli
    from evoworld_amd import mvs, ops
    seg = max(0, (V - 25) // 24)
    cam = cli.synthetic_episode(max(V, 24 * (seg + 2) + 8))
    clip = synthetic_clip(V, H, W)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = ops._ptr
    grey = ops.mvs_luma(clip)
    opt = mvs.sgm_options("sgm", p1, p2, paths, cost_scale, workspace_bytes)
    n = min(V, mvs.sgm_chunk_views(workspace_bytes, H, W, D))
    chunks = [(b, min(n, V - b)) for b in range(0, V, n)]
    cost = torch.empty((n, H, W, D), dtype=torch.uint16, device="cuda")
    agg = torch.empty_like(cost)
    outs = [torch.empty((V, H, W), dtype=dt, device="cuda") for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]
    if sphere:
        st = mvs.sphere_setup(mvs.pano_poses(cam, V, seg), W, S, D)
        src, inv, pose = up(st.src_index), up(st.inv_dist_f32), up(st.rel_pose_f32)
        fused = lambda: ops._call("ew_mvs_sphere_sweep", P(grey), P(pose), P(src), P(inv), *[P(o) for o in outs], V, H, W, S, D, r)
        vol = lambda b, m: ops._call("ew_mvs_sphere_sweep_volume", P(grey), P(pose), P(src), P(inv), P(cost), V, H, W, S, D, r, cost_scale, b, m)
    else:
        st = mvs.sweep_setup(mvs.view_poses(cam, V, seg), mvs.pinhole(H, W), S, D)
        src, inv, homog = up(st.src_index), up(st.inv_depth_f32), up(st.homographies_f32)
        fused = lambda: ops._call("ew_mvs_plane_sweep", P(grey), P(homog), P(src), P(inv), *[P(o) for o in outs], V, H, W, S, D, r, 48.0)
        vol = lambda b, m: ops._call("ew_mvs_plane_sweep_volume", P(grey), P(homog), P(src), P(inv), P(cost), V, H, W, S, D, r, 48.0, cost_scale, b, m)
    each = lambda f: [f(b, m) for b, m in chunks]
    vol(*chunks[-1])                                       # the aggregation is timed on real costs (the last chunk's)
    cells, px = V * H * W * D, V * H * W
    fused_us = timed(fused, it)
    stages = [
        stage("sweep_volume", timed(lambda: each(vol), it), px + 2 * cells, "grey in once, the uint16 volume out; the gathers from the sources hit the caches"),
        stage("sgm_aggregate", timed(lambda: each(lambda b, m: ops._call("ew_mvs_sgm_aggregate", P(cost), P(agg), m, H, W, D, opt.P1, opt.P2, paths)), it),
              4 * cells, f"the floor: cost read once, agg written once; the {paths} passes move {4 + 6 * (paths - 1)} B per cell"),
        stage("sgm_select", timed(lambda: each(lambda b, m: ops._call("ew_mvs_sgm_select", P(agg), P(inv), P(src), *[P(o[b:b + m]) for o in outs],
                                                                      V, H, W, S, D, b, m)), it),
              2 * cells + 16 * px, "agg in once, four planes out"),
    ]
    total = sum(s["us"] for s in stages)
    return {"views": V, "height": H, "width": W, "planes": D, "sources": S, "patch_radius": r, "paths": paths, "P1": opt.P1, "P2": opt.P2,
            "cost_scale": cost_scale, "views_per_chunk": n, "chunks": len(chunks), "volume_bytes_per_chunk": 2 * n * H * W * D, "stages": stages,
            "sgm_path_ms": round(total / 1e3, 2), "fused_sweep_ms": round(fused_us / 1e3, 2), "ratio_to_fused_sweep": round(total / fused_us, 3)}


def run_zncc(V, H, W, D, S, r, it, sphere, cost_scale=16.0):
    """The fused sweep and the volume entry of one sweep kind with the SAD cost and with the ZNCC cost, all V views in one call each"""
    import unified_loop_consistency as cli
    from evoworld_amd import mvs, ops
    seg = max(0, (V - 25) // 24)
    cam = cli.synthetic_episode(max(V, 24 * (seg + 2) + 8))
    clip = synthetic_clip(V, H, W)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    P = ops._ptr
    grey = ops.mvs_luma(clip)
    vol = torch.empty((V, H, W, D), dtype=torch.uint16, device="cuda")
    outs = [torch.empty((V, H, W), dtype=dt, device="cuda") for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]
    if sphere:
        st = mvs.sphere_setup(mvs.pano_poses(cam, V, seg), W, S, D)
        src, inv, pose = up(st.src_index), up(st.inv_dist_f32), up(st.rel_pose_f32)
        head, dims = (P(grey), P(pose), P(src), P(inv)), (V, H, W, S, D, r)
        calls = {"sad": lambda: ops._call("ew_mvs_sphere_sweep", *head, *[P(o) for o in outs], *dims),
                 "zncc": lambda: ops._call("ew_mvs_sphere_sweep_zncc", *head, *[P(o) for o in outs], *dims, 1.0),
                 "sad_volume": lambda: ops._call("ew_mvs_sphere_sweep_volume", *head, P(vol), *dims, 32.0, 0, V),
                 "zncc_volume": lambda: ops._call("ew_mvs_sphere_sweep_zncc_volume", *head, P(vol), *dims, 1.0, cost_scale, 0, V)}
    else:
        st = mvs.sweep_setup(mvs.view_poses(cam, V, seg), mvs.pinhole(H, W), S, D)
        src, inv, homog = up(st.src_index), up(st.inv_depth_f32), up(st.homographies_f32)
        head, dims = (P(grey), P(homog), P(src), P(inv)), (V, H, W, S, D, r)
        calls = {"sad": lambda: ops._call("ew_mvs_plane_sweep", *head, *[P(o) for o in outs], *dims, 48.0),
                 "zncc": lambda: ops._call("ew_mvs_plane_sweep_zncc", *head, *[P(o) for o in outs], *dims, 100.0, 1.0),
                 "sad_volume": lambda: ops._call("ew_mvs_plane_sweep_volume", *head, P(vol), *dims, 48.0, 32.0, 0, V),
                 "zncc_volume": lambda: ops._call("ew_mvs_plane_sweep_zncc_volume", *head, P(vol), *dims, 100.0, 1.0, cost_scale, 0, V)}
    us = {name: round(timed(fn, it), 1) for name, fn in calls.items()}
    samples = int((st.src_index >= 0).sum(1).astype(np.int64).sum()) * H * W * D
    return {"views": V, "height": H, "width": W, "hypotheses": D, "sources": S, "patch_radius": r, "us": us, "warped_samples": samples,
            "zncc_Gsamples_per_s": round(samples / us["zncc"] / 1e3, 2), "sad_Gsamples_per_s": round(samples / us["sad"] / 1e3, 2),
            "ratio_fused_zncc_to_sad": round(us["zncc"] / us["sad"], 3), "ratio_volume_zncc_to_sad": round(us["zncc_volume"] / us["sad_volume"], 3)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--views", type=int, nargs="+", default=[25, 73])
    p.add_argument("--sphere", action="store_true", help="time the sphere-sweep stage on panoramas (576 x 1024 unless --height / --width say otherwise)")
    p.add_argument("--height", type=int, default=None, help="default 384 (576 with --sphere)")
    p.add_argument("--width", type=int, default=None, help="default 512 (1024 with --sphere)")
    p.add_argument("--planes", type=int, default=64)
    p.add_argument("--sources", type=int, default=4)
    p.add_argument("--patch_radius", type=int, default=2)
    p.add_argument("--out", type=str, default=None)
    p.add_argument("--sgm", action="store_true", help="time the semi-global path (volume, aggregate, select) against the fused sweep of the same shape")
    p.add_argument("--sgm_paths", type=int, choices=(4, 8), default=4)
    p.add_argument("--zncc", action="store_true", help="time the four ZNCC entries next to their SAD twins, on 25 views of 384 x 512 and 25 panoramas of 288 x 512")
    args = p.parse_args(argv)
    if args.zncc:
        V = args.views[0]
        rec = {"tool": "bench_mvs --zncc", "device": torch.cuda.get_device_name(0), "iters": args.iters,
               "note": "device events around whole entry calls, SAD and ZNCC entries in one process on the same inputs; us per call over all "
                       "views.  Per (hypothesis, source) the ZNCC sweep runs its own box filter of three sums behind two workgroup barriers, "
                       "where the SAD sweep runs one filter of one sum per hypothesis.  No gate and no speed claim.",
               "plane": run_zncc(V, args.height or 384, args.width or 512, args.planes, args.sources, args.patch_radius, args.iters, False),
               "sphere": run_zncc(V, args.height or 288, args.width or 512, args.planes, args.sources, args.patch_radius, args.iters, True)}
        return _emit(rec, args.out or os.path.join(ROOT, "profiles", "mvs_zncc_bench.json"))
    if args.sgm:
        H, W = (args.height or 576, args.width or 1024) if args.sphere else (args.height or 384, args.width or 512)
        kind = "sphere" if args.sphere else "plane"
        out = args.out or os.path.join(ROOT, "profiles", "mvs_sgm_bench.json")
        rec = {}
        if os.path.exists(out):                            # one file, one entry per sweep kind: keep the other kind's
            with open(out) as fh:
                rec = json.loads(fh.read())
        rec.update({"tool": "bench_mvs --sgm", "device": torch.cuda.get_device_name(0), "hbm_TBps": HBM_TBS,
                    "note": "device events around whole entry calls, each stage over all its chunks of views; min_bytes is the least a stage must "
                            "move, GBps and hbm_fraction are that over the time; ratio_to_fused_sweep = (volume + aggregate + select) / the fused "
                            "sweep of the same inputs in the same run.  No gate.",
                    kind: {"iters": args.iters,
                           "runs": [run_sgm(V, H, W, args.planes, args.sources, args.patch_radius, args.iters, args.sphere, args.sgm_paths) for V in args.views]}})
        return _emit(rec, out)
    if args.sphere:
        H, W = args.height or 576, args.width or 1024
        rec = {"tool": "bench_mvs --sphere", "device": torch.cuda.get_device_name(0), "iters": args.iters, "hbm_TBps": HBM_TBS,
               "runs": [run_sphere(V, H, W, args.planes, args.sources, args.patch_radius, args.iters) for V in args.views],
               "note": "device events around whole entry calls; stage_call_wall_ms is the best of two synchronised SphereSweepDepth calls with "
                       "the host set-up (host_setup_ms, timed alone), the uploads, the luma pass and the lift.  Per warped sample the sweep "
                       "evaluates an atan2f, an asinf, a square root and a division besides the bilinear blend and the LDS box filter.  No gate."}
        return _emit(rec, args.out or os.path.join(ROOT, "profiles", "mvs_sphere_bench.json"))
    args.height, args.width = args.height or 384, args.width or 512
    rec = {"tool": "bench_mvs", "device": torch.cuda.get_device_name(0), "iters": args.iters, "hbm_TBps": HBM_TBS,
           "runs": [run(V, args.height, args.width, args.planes, args.sources, args.patch_radius, args.iters) for V in args.views],
           "note": "device events around whole entry calls; stage_call_wall_ms is the best of two synchronised PlaneSweepDepth calls with the "
                   "host's float64 homographies (host_setup_ms, timed alone) and their upload.  The sweep is compute-bound: per warped sample two "
                   "IEEE divisions, a bilinear blend of four gathered bytes and the LDS box filter.  No gate."}
    _emit(rec, args.out)


def _emit(rec, out):
    line = json.dumps(rec)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
