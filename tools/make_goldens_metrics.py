#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden vectors of the reference's PSNR / SSIM evaluation and of its ground-truth dump map (runs ONLY
where the reference tree is).

Imports the reference read-only (nothing copied) and runs its own code:
  * calculate_psnr / img_psnr (evoworld/metrics/other_metrics/calculate_psnr.py) as they are: numpy, torch, tqdm, math only.
  * calculate_ssim / calculate_ssim_function (other_metrics/calculate_ssim.py) and main / read_video_our of
    evoworld/metrics/calculate_all_metrics.py, with stub modules for what this machine lacks:
      cv2.getGaussianKernel   restated: cv2's double path for sigma > 0 (t_i = exp(-0.5/sigma^2 * x_i^2), times 1/sum)
      cv2.filter2D            restated: float64 correlation with BORDER_REFLECT_101 (scipy.ndimage.correlate, mode 'mirror')
      cv2.imread              PIL, returned as BGR uint8 like cv2's IMREAD_COLOR
      lpips, torchvision(.utils), the FVD, LPIPS and latent-MSE functions: placeholders (main's other metrics)
    The cv2 filter is the one unpinned piece: OpenCV itself evaluates an 11x11 float64 filter2D through its own (DFT or direct)
    path, whose roundings this restatement does not reproduce (the SSIM values agree to ~1e-15, far inside the tests' 1e-9).
  * the 256-entry map of the predictions_gt_{seg} dumps: the reference's own tensor_to_pil (unified_loop_consistency.py:87-93)
    when its module imports under the stubs of oracle/make_goldens.py; otherwise its two lines are restated here on torch's CPU
    (ToTensor k/255 -> x*2-1 -> (x*0.5+0.5).clamp(0,1).mul(255).byte()).  The fixture records which (gt_map_source).

Contents: seeded uint8 videos, 3 episodes x 25 frames at 29x41 (2 x 2 tiles of the kernel) (C = 3; C = 1 is channel 0 of the same data), their per-frame
PSNR / SSIM, the dicts calculate_psnr, calculate_ssim and main return, the PSNR 100-rule edge (11 vs 12 one-level differences in
a 576x1024x3 frame: only the coordinates are stored), main's failure on 24 generated vs 25 ground-truth frames, and the map.

Usage:  python tools/make_goldens_metrics.py   (from the repo root)  ->  tests/golden/metrics.npz
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_goldens import REF  # noqa: E402  (the reference checkout the oracle tools import)
OUT = os.path.join(ROOT, "tests", "golden", "metrics.npz")

N_EP, T, H, W = 3, 25, 29, 41
EDGE_SHAPE = (3, 576, 1024)
EDGE_MOD = 251                    # edge base frame: (arange(3*576*1024) % 251) as uint8, [3,576,1024]


def seeded_videos(seed=0):
    """gt, gen uint8 [N_EP,T,H,W,3]: smooth moving patterns; the generated side adds noise of a few levels,
    a blur-like shift in some frames, and is identical to the ground truth in two frames (PSNR 100)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gt = np.empty((N_EP, T, H, W, 3), np.uint8)
    for e in range(N_EP):
        for t in range(T):
            for c in range(3):
                v = 128 + 90 * np.sin(0.11 * x * (c + 1) + 0.07 * y + 0.3 * t + e) * np.cos(0.05 * y - 0.2 * c)
                gt[e, t, :, :, c] = np.clip(np.rint(v), 0, 255)
    gen = gt.astype(np.int16) + rng.integers(-6, 7, gt.shape)
    gen[1, 5:9] = np.roll(gt[1, 5:9], 1, axis=2)
    gen[2, 20] = 255 - gt[2, 20]
    gen = np.clip(gen, 0, 255).astype(np.uint8)
    gen[0, 3] = gt[0, 3]
    gen[2, 24] = gt[2, 24]
    return gt, gen


def edge_coords(n, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(int(np.prod(EDGE_SHAPE)), size=n, replace=False)).astype(np.int64)


def _stub_modules():
    from PIL import Image
    from scipy import ndimage

    def getGaussianKernel(ksize, sigma):
        x = np.arange(ksize, dtype=np.float64) - (ksize - 1) * 0.5
        t = np.exp((-0.5 / (sigma * sigma)) * x * x)
        return (t * (1.0 / t.sum())).reshape(ksize, 1)

    def filter2D(src, ddepth, kernel):
        assert src.dtype == np.float64 and ddepth == -1
        return ndimage.correlate(src, np.asarray(kernel, np.float64), mode="mirror")

    def imread(path):
        return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1])

    cv2 = types.ModuleType("cv2")
    cv2.getGaussianKernel, cv2.filter2D, cv2.imread = getGaussianKernel, filter2D, imread
    sys.modules["cv2"] = cv2
    tv = types.ModuleType("torchvision")
    tvu = types.ModuleType("torchvision.utils")
    tvu.save_image = lambda *a, **k: None
    tv.utils = tvu
    sys.modules.update({"torchvision": tv, "torchvision.utils": tvu, "lpips": types.ModuleType("lpips")})
    for name, fn in (("calculate_lpips", "calculate_lpips"), ("calculate_latent_mse", "calculate_latent_mse")):
        m = types.ModuleType(f"evoworld.metrics.other_metrics.{name}")
        setattr(m, fn, lambda *a, _fn=fn, **k: {"placeholder": _fn})
        sys.modules[m.__name__] = m


def import_reference_metrics():
    _stub_modules()
    sys.path.insert(0, REF)
    import evoworld.metrics.calculate_all_metrics as CAM
    import evoworld.metrics.other_metrics.calculate_psnr as CP
    import evoworld.metrics.other_metrics.calculate_ssim as CS
    CAM.calculate_fvd_batch = lambda *a, **k: {"placeholder": "fvd"}
    return CAM, CP, CS


def gt_dump_map():
    k = torch.arange(256, dtype=torch.uint8)
    frame = (k.float() / 255.0) * 2 - 1                                  # ToTensor, CustomRescale (CameraTrajDataset.py:41-50)
    img = frame.reshape(1, 16, 16).repeat(3, 1, 1)
    try:
        from oracle.make_goldens import _import_reference
        cwd = os.getcwd()
        _import_reference()
        os.chdir(cwd)
        import unified_loop_consistency as U
        out = np.asarray(U.tensor_to_pil(img))[:, :, 0].reshape(256)
        return out.astype(np.uint8), "reference tensor_to_pil"
    except Exception as e:                                               # noqa: BLE001
        print(f"tensor_to_pil not importable ({type(e).__name__}: {e}); restating its two lines", file=sys.stderr)
        out = (img * 0.5 + 0.5).clamp(0, 1).mul(255).byte()[0].reshape(256)
        return out.numpy(), "restated"


def write_tree(root, gt, gen, gen_frames=None):
    """data_path/ep_XXX/{predictions_gt_0, predictions_0}/NNN.png (NNN from 001); gen_frames: generated frames per episode."""
    from PIL import Image
    for e in range(gt.shape[0]):
        for sub, v, n in (("predictions_gt_0", gt, gt.shape[1]), ("predictions_0", gen, gen_frames or gen.shape[1])):
            d = os.path.join(root, f"ep_{e:03d}", sub)
            os.makedirs(d, exist_ok=True)
            for t in range(n):
                Image.fromarray(v[e, t]).save(os.path.join(d, f"{t + 1:03}.png"))


def run_main(CAM, root):
    import argparse
    args = argparse.Namespace(data_path=root, gt_subdir="predictions_gt_0", gen_subdir="predictions_0",
                              result_file=os.path.join(root, "eval_score.json"), num_videos=100, test_length=25)
    CAM.args = args                                                      # read_video_our lists the global args.data_path (:185)
    CAM.main(args)
    return json.load(open(args.result_file))


def main():
    gt_map, gt_map_src = gt_dump_map()                                   # first: it installs oracle/make_goldens.py's stubs
    CAM, CP, CS = import_reference_metrics()
    gt, gen = seeded_videos()
    v1 = torch.tensor(gt).permute(0, 1, 4, 2, 3) / 255.0                 # [B,T,C,H,W] in [0,1], uint8 / 255.0 as main does
    v2 = torch.tensor(gen).permute(0, 1, 4, 2, 3) / 255.0
    out = {"gt": gt, "gen": gen}
    for tag, a, b in (("c3", v1, v2), ("c1", v1[:, :, :1], v2[:, :, :1])):
        out[f"psnr_frames_{tag}"] = np.array([[CP.img_psnr(a[e, t].numpy(), b[e, t].numpy()) for t in range(T)] for e in range(N_EP)],
                                             np.float64)
        out[f"ssim_frames_{tag}"] = np.array([[CS.calculate_ssim_function(a[e, t].numpy(), b[e, t].numpy()) for t in range(T)]
                                              for e in range(N_EP)], np.float64)
        out[f"psnr_dict_{tag}"] = json.dumps(CP.calculate_psnr(a, b))
        out[f"ssim_dict_{tag}"] = json.dumps(CS.calculate_ssim(a, b))
    with tempfile.TemporaryDirectory() as d:
        write_tree(d, gt, gen)
        out["main_result"] = json.dumps(run_main(CAM, d))
    with tempfile.TemporaryDirectory() as d:
        write_tree(d, gt, gen, gen_frames=T - 1)
        try:
            run_main(CAM, d)
            out["main_mismatch_error"] = "none"
        except Exception as e:                                           # noqa: BLE001
            out["main_mismatch_error"] = f"{type(e).__name__}"
    base = (np.arange(int(np.prod(EDGE_SHAPE))) % EDGE_MOD).astype(np.uint8)
    for n in (11, 12):
        idx = edge_coords(n, n)
        other = base.copy()
        other[idx] += 1                                                  # base < 251: one level up never wraps
        a = (torch.tensor(base).reshape(EDGE_SHAPE) / 255.0).numpy()
        b = (torch.tensor(other).reshape(EDGE_SHAPE) / 255.0).numpy()
        out[f"edge_idx_{n}"] = idx
        out[f"edge_psnr_{n}"] = np.float64(CP.img_psnr(a, b))
    out["gt_map"], out["gt_map_source"] = gt_map, src = gt_map, gt_map_src
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); gt map: {src}, lowered levels: {int((out['gt_map'] != np.arange(256)).sum())}; "
          f"edge psnr 11/12: {out['edge_psnr_11']} / {out['edge_psnr_12']}; mismatch: {out['main_mismatch_error']}")


if __name__ == "__main__":
    main()
