#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden vectors of the reference's FVD pieces (runs ONLY where the reference tree is).

Loads two files of the reference by path (read-only, nothing copied; calculate_all_metrics.py is NOT imported, it needs cv2):
evoworld/metrics/fvd/videogpt/pytorch_i3d.py for InceptionI3d, Unit3D and MaxPool3dSamePadding, and evoworld/metrics/fvd/styleganv/fvd.py
for preprocess_single and frechet_distance.  evoworld_amd.fvd.random_state_dict(0) is loaded into the reference's InceptionI3d(400).

  sd_names / sd_shapes     the reference network's state-dict keys (num_batches_tracked left out) and their shapes, zero-padded to 5
  clip{i}                  two uint8 clips: landscape [10,45,80,3] and portrait [13,60,52,3] (the h >= w branch), noise over a texture
  pre_idx{i} / pre_val{i}  preprocess_single's output [3,T,224,224] at ~2000 fixed flat positions; pre_sum{i} its float64 sum
  logits{i}                the 400 logits of the clip (R, G, B order)
  fd_*                     seeded feature pairs [64,8], [16,400], [1,400] and frechet_distance of each
  pad_ks / pad_table       compute_pad for sizes 1..16 at the four (kernel, stride) pairs in use, from Unit3D and MaxPool3dSamePadding
  geo_hw / geo_target      the size preprocess_single hands to F.interpolate for a list of frame sizes

Usage:  python tools/make_goldens_fvd.py   (from the repo root)  ->  tests/golden/fvd.npz
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "fvd.npz")
CLIPS = ((10, 45, 80), (13, 60, 52))
PAD_KS = ((7, 2), (3, 1), (3, 2), (2, 2))
GEO_HW = ((45, 80), (60, 52), (224, 224), (576, 1024), (64, 96), (96, 160), (100, 100), (300, 224), (7, 9), (500, 1000), (225, 224))
FD_SHAPES = ((64, 8), (16, 400), (1, 400))


def load_reference(rel, name):
    from oracle.make_goldens import REF
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_clip(seed, T, H, W):
    """uint8 [T,H,W,3]: a drifting smooth texture under noise of +-40 levels"""
    rng = np.random.default_rng(seed)
    t, y, x, c = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    base = 128 + 70 * np.sin(0.21 * x * (c + 1) + 0.17 * y + 0.4 * t + seed)
    return np.clip(np.rint(base + rng.integers(-40, 41, base.shape)), 0, 255).astype(np.uint8)


def main():
    from evoworld_amd.fvd import random_state_dict
    i3d = load_reference("evoworld/metrics/fvd/videogpt/pytorch_i3d.py", "ref_pytorch_i3d")
    sg = load_reference("evoworld/metrics/fvd/styleganv/fvd.py", "ref_styleganv_fvd")
    net = i3d.InceptionI3d(400, in_channels=3).eval()
    ref_sd = {k: v for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    gold = {"sd_names": np.array(list(ref_sd)), "sd_shapes": np.array([list(v.shape) + [0] * (5 - v.ndim) for v in ref_sd.values()], np.int64)}
    res = net.load_state_dict(random_state_dict(0), strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys), res
    rng = np.random.default_rng(2024)
    with torch.no_grad():
        for i, (T, H, W) in enumerate(CLIPS):
            clip = make_clip(i + 1, T, H, W)
            video = (torch.from_numpy(clip).permute(3, 0, 1, 2).float() / 255.0).contiguous()          # CTHW in [0,1]
            pre = sg.preprocess_single(video)
            assert tuple(pre.shape) == (3, T, 224, 224)
            idx = np.unique(np.concatenate([rng.choice(pre.numel(), 2000, replace=False), [0, 223, 224 * 223, pre.numel() - 1]]))
            gold[f"clip{i}"] = clip
            gold[f"pre_idx{i}"] = idx.astype(np.int64)
            gold[f"pre_val{i}"] = pre.reshape(-1)[torch.from_numpy(idx)].numpy()
            gold[f"pre_sum{i}"] = np.float64(pre.double().sum())
            gold[f"logits{i}"] = net(pre[None])[0].numpy()
            assert gold[f"logits{i}"].shape == (400,)
    for n, d in FD_SHAPES:
        a, b = rng.standard_normal((n, d)), 0.3 + 1.2 * rng.standard_normal((n, d))
        gold[f"fd_a_{n}x{d}"], gold[f"fd_b_{n}x{d}"] = a, b
        gold[f"fd_{n}x{d}"] = np.float64(sg.frechet_distance(a, b))
    table = np.zeros((2, len(PAD_KS), 16), np.int64)
    for j, (k, s) in enumerate(PAD_KS):
        u = i3d.Unit3D(8, 8, kernel_shape=(k, k, k), stride=(s, s, s))
        m = i3d.MaxPool3dSamePadding(kernel_size=(k, k, k), stride=(s, s, s), padding=0)
        for size in range(1, 17):
            table[0, j, size - 1], table[1, j, size - 1] = u.compute_pad(1, size), m.compute_pad(2, size)
    assert np.array_equal(table[0], table[1])
    gold["pad_ks"], gold["pad_table"] = np.array(PAD_KS, np.int64), table[0]
    # the loaded module's own name `F` is pointed at a recorder for these calls; torch.nn.functional itself is not touched
    targets, real = [], sg.F
    try:
        sg.F = SimpleNamespace(interpolate=lambda v, size, **kw: (targets.append(tuple(size)), real.interpolate(v, size=size, **kw))[1])
        for H, W in GEO_HW:
            sg.preprocess_single(torch.zeros(3, 1, H, W))
    finally:
        sg.F = real
    gold["geo_hw"], gold["geo_target"] = np.array(GEO_HW, np.int64), np.array(targets, np.int64)
    np.savez_compressed(OUT, **gold)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; logits |mean| {[float(np.abs(gold[f'logits{i}']).mean()) for i in range(len(CLIPS))]}")


if __name__ == "__main__":
    main()
