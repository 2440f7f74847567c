#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden vectors of the reference's non-curve navigation mode (runs ONLY where the reference tree is).

Imports the reference with the stubs of oracle/make_goldens_pipeline.py (read-only, nothing copied) and runs its own
`Navigator.split_path_into_segments`, `rotate_panorama` and `navigate_path` (evoworld/inference/navigator_evoworld.py:276-301,
335-392, 466-512), with `.to('cuda...')` redirected to the CPU and a recording stub pipe, as `navigator_goldens()` does.

  (a) split_path_into_segments on three paths (case_000's scaled poses, a loop of straight runs with in-place 90-degree turns,
      consecutive single-step turns): the segments, and the input tensor as the call leaves it (the reference writes into it)
  (b) rotate_panorama at 576x1024: per-column source index ui and per-row vi for a set of yaws (the map is separable)
  (c) navigate_path at 64x128, segment_id 0..3 with infer_segment=True and one chained call (infer_segment=False): per pipe call
      the rotated image, the Plucker embedding of the window, mask_mem, the re-seeded generator, the frame count, current_pose

Usage:  python tools/make_goldens_navigate_path.py   (from the repo root)  ->  tests/golden/navigate_path.npz
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "navigate_path.npz")

H_ROT, W_ROT = 576, 1024
YAWS = [0.0, 90.0, -90.0, 180.0, -37.5, 12.3456, 0.001, 270.0]
H, W = 64, 128
N_CALLS_INFER = 4


def straight(start_xyz, yaw, n, step=0.04):
    """n rows walking along `yaw` (degrees) from start_xyz (exclusive) with a constant rotation."""
    x, y, z = start_xyz
    rows = []
    for _ in range(n):
        x, z = x + step * np.sin(np.deg2rad(yaw)), z + step * np.cos(np.deg2rad(yaw))
        rows.append([x, y, z, 0.0, yaw, 0.0])
    return rows


def runs_path(spec, start=(0.3, -0.178, -0.2)):
    """[(yaw, n_rows), ...] -> float32 [P,6]: straight runs joined by in-place turns."""
    rows = [[*start, 0.0, spec[0][0], 0.0]]
    for i, (yaw, n) in enumerate(spec):
        rows += straight(rows[-1][:3], yaw, n - 1 if i == 0 else n)
    return np.asarray(rows, np.float32)


def loop_path():
    return runs_path([(95.0, 25), (185.0, 24), (275.0, 24), (5.0, 24)])


def single_step_turns_path():
    rows = [[0.0, 0.0, 0.0, 0.0, 10.0, 0.0]]
    for yaw in [10.0, 10.0, 20.0, 30.0, 45.0, 45.0, -15.0, -15.0, -15.0, 60.0, 75.0, 75.0, 75.0]:
        rows += straight(rows[-1][:3], yaw, 1)
    return np.asarray(rows, np.float32)


def navigate_path_case():
    """runs of 30 (> 25: trimmed to the pipeline's 25), 8, 1 (a 2-pose segment), 12 and 5 rows; turns +90, -37.5, +12.3456,
    +0.001 degrees"""
    return runs_path([(10.0, 30), (100.0, 8), (62.5, 1), (74.8456, 12), (74.8466, 5)])


def case_000_scaled():
    from evoworld_amd.geometry import UNITY_TO_OPENCV
    g = np.load(os.path.join(ROOT, "tests", "golden", "plucker.npz"))
    cam = g["poses_unity"].astype(np.float64) * np.asarray(UNITY_TO_OPENCV, np.float64)
    cam[:, :3] *= 0.1                                                     # dataset/CameraTrajDataset.py:223,348
    return cam.astype(np.float32)


def pattern_u8(h, w, a, b, c0):
    """a deterministic, well-compressible 8-bit image whose columns and rows are mostly distinct"""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(a * x + b * y + c0 + 70 * c) % 256 for c in range(3)], -1).astype(np.uint8)


def stub_frame(call, i):
    return pattern_u8(H, W, 5, 11, 17 * i + 31 * call)


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from oracle.make_goldens_pipeline import _patch_reference
    _patch_reference()
    import evoworld.inference.navigator_evoworld as NV
    from PIL import Image
    from utils.plucker_embedding import equirectangular_to_ray
    real_to = torch.Tensor.to

    def to_cpu(self, *a, **k):
        a = tuple("cpu" if (isinstance(x, str) and x.startswith("cuda")) else x for x in a)
        return real_to(self, *a, **k)

    def new_nav():
        nav = NV.Navigator.__new__(NV.Navigator)
        nav.logger = SimpleNamespace(info=lambda *a, **k: None)
        nav.step_size, nav.position_scale, nav.generations = 0.4, 0.1, []
        nav.previous_images = torch.zeros(0, 3, H, W)
        nav.previous_trajectoies = torch.tensor([])
        nav.current_pose = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        nav.rays = torch.tensor(equirectangular_to_ray(target_H=H // 8, target_W=W // 8)).to(torch.float32)
        nav.transform = lambda im: torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).float() / 255.0 * 2 - 1
        nav.model_width, nav.model_height, nav.num_frames, nav.fps = W, H, 25, 7
        return nav

    gold = {}
    torch.Tensor.to = to_cpu
    try:
        # (a) segmentation, and what the call does to its input
        for tag, path in (("case000", case_000_scaled()), ("loop", loop_path()), ("turns", single_step_turns_path())):
            t = torch.from_numpy(path.copy())
            segs = new_nav().split_path_into_segments(t)
            gold[f"a_{tag}_path"] = path
            gold[f"a_{tag}_path_after"] = t.numpy()
            gold[f"a_{tag}_lengths"] = np.array([len(s) for s in segs], np.int64)
            gold[f"a_{tag}_segments"] = torch.cat([torch.stack(s) for s in segs]).numpy()
            print(tag, "segments", [len(s) for s in segs], "input modified:", not np.array_equal(path, t.numpy()))

        # (b) rotate_panorama's gather indices: pixel value = y*W + x (exact in fp32)
        nav = new_nav()
        enc = (torch.arange(H_ROT)[:, None] * W_ROT + torch.arange(W_ROT)[None, :]).float()
        img = enc[None].repeat(3, 1, 1)
        ui, vi = [], []
        for d in YAWS:
            out = nav.rotate_panorama(img, torch.tensor(d, dtype=torch.float32), scale_factor=1)[0].long()
            u, v = out % W_ROT, out // W_ROT
            assert (u == u[:1]).all() and (v == v[:, :1]).all()                 # separable
            ui.append(u[0].numpy())
            vi.append(v[:, 0].numpy())
        gold["b_yaws"] = np.asarray(YAWS, np.float32)
        gold["b_hw"] = np.array([H_ROT, W_ROT], np.int64)
        gold["b_ui"] = np.stack(ui).astype(np.int16)
        gold["b_vi"] = np.stack(vi).astype(np.int16)
        print("rows != y at 0 deg:", int((vi[0] != np.arange(H_ROT)).sum()), " columns != x at 0 deg:", int((ui[0] != np.arange(W_ROT)).sum()))

        # (c) navigate_path with a recording pipe
        path = navigate_path_case()
        start_u8 = pattern_u8(H, W, 7, 3, 0)
        start = torch.from_numpy(start_u8).permute(2, 0, 1).float() / 255.0 * 2 - 1
        g = torch.Generator().manual_seed(31)
        memory = torch.rand(1, 25, 3, H, W, generator=g) * 2 - 1
        ref_state = torch.manual_seed(-1).get_state()
        calls = []
        plucker = {}

        def run(segment_id, infer_segment):
            nav = new_nav()

            def pipe(image, **kw):
                c = len(calls)
                calls.append(dict(image=image.clone(), plucker=kw["plucker_embedding"].clone(), mask_mem=kw["mask_mem"],
                                  reseeded=kw["generator"] is torch.default_generator and torch.equal(kw["generator"].get_state(), ref_state),
                                  segment_id=-1 if segment_id is None else segment_id, infer=infer_segment))
                return SimpleNamespace(frames=[[Image.fromarray(stub_frame(c, i)) for i in range(25)]])
            nav.pipe = pipe
            n0 = len(calls)
            gens = nav.navigate_path(torch.from_numpy(path.copy()), start.clone(), width=W, height=H, fps=7, num_inference_steps=7,
                                     memorized_images=memory, infer_segment=infer_segment, segment_id=segment_id)
            for c, mv in zip(calls[n0:], gens):
                c["n_frames"] = len(mv)
            calls[-1]["current_pose"] = nav.current_pose.clone()

        for k in range(N_CALLS_INFER):
            run(k, True)
        run(None, False)
        seg_of_call = list(range(N_CALLS_INFER)) + list(range(len(calls) - N_CALLS_INFER))
        for c, k in zip(calls, seg_of_call):
            if k in plucker:
                assert torch.equal(plucker[k], c["plucker"])                    # same window in both kinds of call
            plucker[k] = c["plucker"]
        imgs = torch.stack([c["image"][0] for c in calls])
        u8 = torch.round((imgs + 1) / 2 * 255).to(torch.uint8)
        assert torch.equal(u8.float() / 255.0 * 2 - 1, imgs)                      # every image handed over is on the 8-bit grid
        gold.update({
            "c_path": path, "c_start_u8": start_u8, "c_hw": np.array([H, W], np.int64),
            "c_call_segment": np.array(seg_of_call, np.int64),
            "c_call_infer": np.array([c["infer"] for c in calls]),
            "c_call_segment_id": np.array([c["segment_id"] for c in calls], np.int64),
            "c_image_u8_hwc": u8.permute(0, 2, 3, 1).contiguous().numpy(),
            "c_mask_mem": np.array([c["mask_mem"] for c in calls]),
            "c_reseeded": np.array([c["reseeded"] for c in calls]),
            "c_n_frames": np.array([c["n_frames"] for c in calls], np.int64),
            "c_current_pose": np.stack([c["current_pose"].numpy() if "current_pose" in c else np.full(6, np.nan, np.float32) for c in calls]),
        })
        for k, pl in plucker.items():
            gold[f"c_plucker_seg{k}"] = pl[0].numpy()                             # [25,6,8,16]
        print("navigate_path calls:", len(calls), "frames", gold["c_n_frames"].tolist(), "mask_mem", gold["c_mask_mem"].tolist())
    finally:
        torch.Tensor.to = real_to
    np.savez_compressed(OUT, **gold)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
