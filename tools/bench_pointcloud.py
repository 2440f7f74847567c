"""Times the device voxel-grid downsample (csrc/pointcloud.hip) stage by stage on a synthetic cloud of the episode's size, and the
point splat with and without it.

  python tools/bench_pointcloud.py [--iters N] [--points N] [--voxels 0.02,0.05] [--out profiles/pointcloud_bench.json]

The cloud: 73 x 384 x 512 lifted pixels at 50 % confidence = 7 176 192 points, drawn as 73 overlapping views of a few noisy planes
(consecutive frames see the same surfaces, so most points are near-duplicates).  Stages, device events around `iters` calls each:
bounds (ew_points_bounds), keys (ew_voxel_keys), sort (torch.sort(stable=True): torch's kernel, not ours), reduce (ew_voxel_reduce), with
the bytes each must move at the least and that figure against the 8 TB/s of HBM; then ew_splat_cubemap + ew_splat_resolve (24 views, 512
faces) on the full cloud and on the cloud thinned at each voxel size.  Prints one JSON line and, with --out, writes it there.  No gate:
these are measurements."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 8.0
EPISODE_POINTS = 73 * 384 * 512 // 2


def synthetic_cloud(n, seed=0):
    """n points on three noisy planes of a 10 x 4 x 10 room, seen again and again (device fp32 [n,3], uint8 [n,4])"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.rand(n, 2, device="cuda", generator=g)
    which = torch.randint(0, 3, (n,), device="cuda", generator=g)
    noise = torch.randn(n, device="cuda", generator=g) * 0.01
    xyz = torch.empty(n, 3, device="cuda")
    xyz[:, 0] = torch.where(which == 0, noise, u[:, 0] * 10)
    xyz[:, 1] = torch.where(which == 1, noise, torch.where(which == 0, u[:, 0] * 4, u[:, 1] * 4))
    xyz[:, 2] = torch.where(which == 2, noise, torch.where(which == 1, u[:, 1] * 10, u[:, 1] * 10))
    rgbx = torch.randint(0, 256, (n, 4), device="cuda", generator=g, dtype=torch.uint8)
    return xyz.contiguous(), rgbx.contiguous()


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


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--points", type=int, default=EPISODE_POINTS)
    p.add_argument("--voxels", type=str, default="0.02,0.05", help="two voxel sizes for the splat comparison (scene units)")
    p.add_argument("--out", type=str, default=None)
    args = p.parse_args(argv)
    from evoworld_amd import _lib, ops
    from evoworld_amd.reprojection import face_w2c
    lib = _lib.load()
    n = args.points
    voxels = [float(v) for v in args.voxels.split(",")]
    xyz, rgbx = synthetic_cloud(n)
    P = ops._ptr

    ws_b = torch.empty(lib.ew_points_bounds_workspace_bytes(n) // 8 + 1, dtype=torch.int64, device="cuda")
    out6, cnt = torch.empty(6, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    lo, _, _ = ops.points_bounds(xyz)
    v0 = voxels[0]
    origin = torch.from_numpy((lo - np.float32(0.5) * np.float32(v0)).astype(np.float32)).cuda()
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops._call("ew_voxel_keys", P(xyz), n, P(origin), v0, P(keys), P(flag))
    skeys, perm = torch.sort(keys, stable=True)
    o_xyz, o_rgba = torch.empty(n, 3, device="cuda"), torch.empty(n, 4, dtype=torch.uint8, device="cuda")
    o_cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    ws_r = torch.empty(lib.ew_voxel_reduce_workspace_bytes(n) // 16 + 1, 2, dtype=torch.int64, device="cuda")
    m_d = torch.empty(1, dtype=torch.int64, device="cuda")
    ops._call("ew_voxel_reduce", P(skeys), P(perm), n, P(xyz), P(rgbx), P(o_xyz), P(o_rgba), P(o_cnt), P(ws_r), P(m_d))
    m = int(m_d.item())
    it = args.iters
    stages = [
        stage("bounds", timed(lambda: ops._call("ew_points_bounds", P(xyz), n, P(ws_b), P(out6), P(cnt)), it), n * 12, "xyz once"),
        stage("keys", timed(lambda: ops._call("ew_voxel_keys", P(xyz), n, P(origin), v0, P(keys), P(flag)), it), n * 20, "xyz in, keys out"),
        stage("sort", timed(lambda: torch.sort(keys, stable=True), it), n * 32, "torch.sort(stable): keys in, keys + permutation out, one pass "
              "counted (a radix sort makes several)"),
        stage("reduce", timed(lambda: ops._call("ew_voxel_reduce", P(skeys), P(perm), n, P(xyz), P(rgbx), P(o_xyz), P(o_rgba), P(o_cnt),
                                                 P(ws_r), P(m_d)), it), n * (8 + 8 + 8 + 12 + 4) + m * 20,
              "keys twice, permutation, gathered xyz + colour; voxels out"),
    ]
    whole = timed(lambda: ops.voxel_downsample(xyz, rgbx, v0), max(2, it // 2))

    V, res = 24, 512
    ang = np.arange(V) * (2 * np.pi / V)
    c2w = np.tile(np.eye(4), (V, 1, 1))
    c2w[:, 0, 3], c2w[:, 1, 3], c2w[:, 2, 3] = 5 + 2 * np.cos(ang), 2.0, 5 + 2 * np.sin(ang)
    w2c = torch.from_numpy(face_w2c(c2w)).cuda()
    f = res / 2

    def splat(v, c):
        return ops.splat_cubemap(v, c, w2c, res, f, f, f, f, 0.1, 4)
    splats = [{"cloud": "full", "points": n, "splat_us": round(timed(lambda: splat(xyz, rgbx), it), 1)}]
    for v in voxels:
        dv, dc, _ = ops.voxel_downsample(xyz, rgbx, v)
        splats.append({"cloud": f"voxel {v:g}", "points": int(dv.shape[0]), "splat_us": round(timed(lambda: splat(dv, dc), it), 1),
                       "downsample_us": round(timed(lambda: ops.voxel_downsample(xyz, rgbx, v), max(2, it // 2)), 1)})
    rec = {"tool": "bench_pointcloud", "device": torch.cuda.get_device_name(0), "points": n, "voxel": v0, "voxels_out": m, "iters": it,
           "hbm_TBps": HBM_TBS, "stages": stages, "voxel_downsample_us": round(whole, 1), "splat": splats,
           "note": "device events around whole calls; voxel_downsample_us is the ops call with its allocations and its three host reads"}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
