"""PSNR / SSIM of generated against ground-truth videos on the device: the counterpart of the reference's
evoworld/metrics/calculate_all_metrics.py (main :209-236, read_video_our :178-207, arguments :229-258) with
other_metrics/calculate_psnr.py and calculate_ssim.py.

Per-frame values come from one kernel pass over each frame pair (ops.video_metrics, csrc/metrics.hip); the per-timestamp mean
and std and the overall mean are the reference's numpy aggregation over those fp64 values.  FVD, LPIPS and the latent MSEs need
pretrained networks (I3D, LPIPS/AlexNet, Inception-v4) that this project does not ship: they are listed under `not_computed`.
LPIPS is computed as well (evoworld_amd/lpips.py, csrc/lpips.hip) when the user names a file with its weights, and so is FVD
(evoworld_amd/fvd.py, csrc/i3d.hip: the styleganv method over I3D's 400 logits) when the user names a file with the I3D weights, and so
are latent_mse and loop_closure_latent_mse (evoworld_amd/latent_mse.py, csrc/inception.hip: calculate_latent_mse.py:11-79 as
calculate_all_metrics.py:220-221 calls it, over timm inception_v4's 1536 pooled features) when the user names the Inception-v4 weights.

    python -m evoworld_amd.metrics --data_path OUT --gt_subdir predictions_gt_2 --gen_subdir predictions_2 [--pair_by_name]
                                   [--metrics psnr,ssim,lpips --lpips_weights lpips_alex.safetensors]
                                   [--metrics psnr,ssim,fvd --fvd_weights i3d_pretrained_400.pt]
                                   [--metrics psnr,ssim,latent_mse,loop_closure_latent_mse --latent_mse_weights inception_v4.safetensors]
                                   [--metrics psnr,ssim,ws_psnr,ws_ssim[,ws_lpips --lpips_weights ...]]
                                   [--projection cube [--viewport_size 256]]

The frames are equirectangular panoramas, which the metrics above score as flat images.  Two additions, neither of them in the
reference, account for the sphere: the latitude-weighted WS-PSNR / WS-SSIM / WS-LPIPS (a row counts with the cosine of its latitude:
ops.video_metrics_ws, LPIPSAlex's row_weights), and --projection cube, which scores six 90-degree perspective viewports of every clip
(cube_viewports, through reprojection.Equi2Pers) with the unchanged planar metrics.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

from .frames import read_frames

SEQUENCE = 25                  # read_video_our keeps the last 25 frames of each folder (:191)
NOT_COMPUTED = {
    "fvd": "needs the I3D network (styleganv i3d_torchscript weights) and its code, absent from this project; no network access",
    "lpips": "needs the LPIPS network (AlexNet backbone and linear-layer weights) and its package, absent; no network access",
    "latent_mse": "needs Inception-v4 (timm inception_v4) weights passed with --latent_mse_weights, which this project does not ship; "
                  "despite the metric's name its features are not latents of the SVD VAE",
    "loop_closure_latent_mse": "needs the same Inception-v4 (timm inception_v4) weights as latent_mse, passed with --latent_mse_weights; "
                               "despite the metric's name it does not use the SVD VAE",
}
SUPPORTED = ("psnr", "ssim")
SPHERICAL = ("ws_psnr", "ws_ssim", "ws_lpips")      # latitude-weighted forms for equirectangular frames; ws_lpips needs --lpips_weights
PROJECTIONS = ("equirect", "cube")
CUBE_FACES = ("front", "right", "back", "left", "up", "down")
# Equi2Pers rotations of the faces, radians: a positive yaw turns the view to the left, a positive pitch turns it up
CUBE_ROTS = ({}, {"yaw": -math.pi / 2}, {"yaw": math.pi}, {"yaw": math.pi / 2}, {"pitch": math.pi / 2}, {"pitch": -math.pi / 2})


def psnr_from_sse(sse, n):
    """img_psnr of calculate_psnr.py:6-15 from the frame's squared-error sum over n = C*H*W elements.  WS-PSNR is the same rule on the
    weighted sum with n = C * W * sum_y w[y]."""
    mse = float(sse) / n
    if mse < 1e-10:
        return 100
    return 20 * math.log10(1 / math.sqrt(mse))


def latitude_weights(H):
    """fp64 [H]: the cosine of the latitude of each row's centre of an equirectangular frame, cos((y + 0.5 - H/2) pi / H): the share
    of the sphere a pixel of that row covers, up to a constant (the WS-PSNR weights of 360-degree video evaluation)."""
    if H < 1:
        raise ValueError(f"latitude_weights: H = {H} must be positive")
    return np.cos((np.arange(H, dtype=np.float64) + 0.5 - H / 2) * np.pi / H)


def aggregate(results, video_setting):
    """The reference's aggregation (calculate_psnr.py / calculate_ssim.py, after the per-frame loop): results [B,T] -> dict."""
    results = np.array(results)
    value, value_std = {}, {}
    for t in range(results.shape[1]):
        value[t] = np.mean(results[:, t])
        value_std[t] = np.std(results[:, t])
    return {
        "value": value,
        "value_mean": float(np.mean(results)),
        "value_std": value_std,
        "video_setting": video_setting,
        "video_setting_name": "time, channel, heigth, width",
    }


def _per_frame(videos1, videos2, what):
    """[B,T,C,H,W] float in [0,1] (CPU or device) -> per-frame (sse, ssim) numpy fp64 [B,T] (None where not asked)."""
    from . import ops
    if videos1.shape != videos2.shape:
        raise AssertionError(f"video shapes differ: {tuple(videos1.shape)} vs {tuple(videos2.shape)}")
    B, T, C, H, W = videos1.shape
    a = videos1.reshape(B * T, C, H, W).to("cuda", torch.float32).contiguous()
    b = videos2.reshape(B * T, C, H, W).to("cuda", torch.float32).contiguous()
    sse, ssim = ops.video_metrics(a, b, what)
    cpu = lambda x: None if x is None else x.cpu().numpy().reshape(B, T)
    return cpu(sse), cpu(ssim)


def calculate_psnr(videos1, videos2):
    """calculate_psnr(videos1, videos2) of calculate_psnr.py:18-65: [B,T,C,H,W] in [0,1] -> the reference's result dict."""
    from . import ops
    sse, _ = _per_frame(videos1, videos2, ops.METRIC_SSE)
    n = int(np.prod(videos1.shape[2:]))
    return aggregate([[psnr_from_sse(s, n) for s in row] for row in sse], videos1[0].shape)


def calculate_ssim(videos1, videos2):
    """calculate_ssim(videos1, videos2) of calculate_ssim.py:48-95 (C = 1 or 3; H, W >= 11) -> the reference's result dict."""
    from . import ops
    _, ssim = _per_frame(videos1, videos2, ops.METRIC_SSIM)
    return aggregate(ssim, videos1[0].shape)


def _per_frame_ws(videos1, videos2, what, row_w):
    """_per_frame under row weights (default: latitude_weights(H)) -> (wsse, wssim, the weights)"""
    from . import ops
    if videos1.shape != videos2.shape:
        raise AssertionError(f"video shapes differ: {tuple(videos1.shape)} vs {tuple(videos2.shape)}")
    B, T, C, H, W = videos1.shape
    row_w = latitude_weights(H) if row_w is None else ops.check_row_weights(row_w, H)
    a = videos1.reshape(B * T, C, H, W).to("cuda", torch.float32).contiguous()
    b = videos2.reshape(B * T, C, H, W).to("cuda", torch.float32).contiguous()
    wsse, wssim = ops.video_metrics_ws(a, b, row_w, what)
    cpu = lambda x: None if x is None else x.cpu().numpy().reshape(B, T)
    return cpu(wsse), cpu(wssim), row_w


def calculate_ws_psnr(videos1, videos2, row_w=None):
    """WS-PSNR of equirectangular videos: [B,T,C,H,W] in [0,1] -> calculate_psnr's result dict, every squared error weighted by the
    cosine of its row's latitude (row_w: other weights, one per row)."""
    from . import ops
    wsse, _, w = _per_frame_ws(videos1, videos2, ops.METRIC_SSE, row_w)
    n_w = videos1.shape[2] * videos1.shape[4] * float(w.sum())
    return aggregate([[psnr_from_sse(s, n_w) for s in row] for row in wsse], videos1[0].shape)


def calculate_ws_ssim(videos1, videos2, row_w=None):
    """WS-SSIM of equirectangular videos (C = 1 or 3; H, W >= 11): calculate_ssim's result dict, every window of the SSIM map
    weighted by the cosine of its centre row's latitude (row_w: other weights, one per row)."""
    from . import ops
    _, wssim, _ = _per_frame_ws(videos1, videos2, ops.METRIC_SSIM, row_w)
    return aggregate(wssim, videos1[0].shape)


def video_metrics_ws_u8(gt, gen, what=3, row_w=None):
    """uint8 [F,H,W,3] device tensors -> (ws_psnr, ws_ssim) numpy fp64 [F] (None where `what`, ops.METRIC_SSE | ops.METRIC_SSIM, does
    not ask for it) under latitude_weights(H), or row_w."""
    from . import ops
    F_, H, W, C = gt.shape
    row_w = latitude_weights(H) if row_w is None else ops.check_row_weights(row_w, H)
    wsse, wssim = ops.video_metrics_ws(gt.contiguous(), gen.contiguous(), row_w, what)
    n_w = C * W * float(row_w.sum())
    p = None if wsse is None else np.array([psnr_from_sse(s, n_w) for s in wsse.cpu().numpy()], dtype=np.float64)
    return p, None if wssim is None else wssim.cpu().numpy()


def cube_viewports(frames_u8, size=None):
    """Equirectangular frames uint8 [T,H,W,3] on the device -> their six 90-degree perspective viewports, uint8 [6,T,S,S,3] on the
    device in the order of CUBE_FACES (S = size, default W // 4): reprojection.Equi2Pers(S, S, 90) at CUBE_ROTS, one launch per face
    over the same panoramas."""
    from .reprojection import Equi2Pers
    if frames_u8.ndim != 4 or frames_u8.shape[-1] != 3 or frames_u8.dtype != torch.uint8:
        raise ValueError(f"cube_viewports: expected uint8 [T,H,W,3] frames, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
    T, _, W, _ = frames_u8.shape
    S = int(size) if size else W // 4
    if S < 1:
        raise ValueError(f"cube_viewports: viewport size {S} must be positive")
    frames_u8 = frames_u8.contiguous()
    e2p = Equi2Pers(height=S, width=S, fov_x=90.0)
    out = torch.empty(6, T, S, S, 3, dtype=torch.uint8, device=frames_u8.device)
    for k, rots in enumerate(CUBE_ROTS):
        out[k] = e2p.batch(frames_u8, [rots] * T)
    return out


def calculate_lpips(videos1, videos2, model, channel_order="rgb"):
    """calculate_lpips(videos1, videos2, device) of calculate_lpips.py: [B,T,3,H,W] in [0,1] -> the reference's result dict, with
    `model` an evoworld_amd.lpips.LPIPSAlex.  channel_order 'bgr' feeds the network B, G, R planes as the reference's main does."""
    if videos1.shape != videos2.shape:
        raise AssertionError(f"video shapes differ: {tuple(videos1.shape)} vs {tuple(videos2.shape)}")
    B, T, C, H, W = videos1.shape
    a = videos1.reshape(B * T, C, H, W).to(model.device, torch.float32).contiguous()
    b = videos2.reshape(B * T, C, H, W).to(model.device, torch.float32).contiguous()
    return aggregate(model(a, b, channel_order).cpu().numpy().reshape(B, T), videos1[0].shape)


def video_metrics_u8(gt, gen):
    """uint8 [F,H,W,3] device tensors -> (psnr, ssim) numpy fp64 [F]: the per-frame values of the reference's main on frames
    read as uint8 and divided by 255.0."""
    from . import ops
    sse, ssim = ops.video_metrics(gt.contiguous(), gen.contiguous())
    n = int(np.prod(gt.shape[1:]))
    return np.array([psnr_from_sse(s, n) for s in sse.cpu().numpy()], dtype=np.float64), ssim.cpu().numpy()


# ------------------------------------------------------------------ the evaluation CLI
def parse_args(argv=None):
    p = argparse.ArgumentParser(description="PSNR / SSIM of generated against ground-truth frame folders on the GPU "
                                            "(calculate_all_metrics.py)")
    p.add_argument("--data_path", type=str, default="data/Segment_Consistency/test")
    p.add_argument("--gt_subdir", type=str, default="predictions_gt_1")
    p.add_argument("--gen_subdir", type=str, default="predictions_1")
    p.add_argument("--result_file", type=str, default="eval_score.json", help="written under --data_path")
    p.add_argument("--num_videos", type=int, default=100)
    p.add_argument("--test_length", type=int, default=25, help="parsed and ignored, as in the reference")
    p.add_argument("--metrics", type=str, default="psnr,ssim",
                   help="comma-separated; psnr and ssim are computed, and so are their latitude-weighted forms ws_psnr and ws_ssim (and "
                        "ws_lpips with --lpips_weights); the others need networks this project lacks")
    p.add_argument("--pair_by_name", action="store_true",
                   help="pair the last 25 file names both folders share (segments >= 1 hold 24 generated and 25 GT frames)")
    p.add_argument("--lpips_weights", type=str, nargs="+", default=None, metavar="PATH",
                   help="LPIPS (AlexNet) weights, .safetensors or a torch checkpoint: a lpips.LPIPS state dict, or torchvision's AlexNet "
                        "and the lpips package's alex.pth as two files; allows lpips in --metrics")
    p.add_argument("--lpips_channel_order", type=str, choices=("bgr", "rgb"), default="bgr",
                   help="bgr (default): the network sees B, G, R planes as in the reference, whose cv2.imread frames are never "
                        "swapped; rgb: LPIPS as its authors define it")
    p.add_argument("--fvd_weights", type=str, nargs="+", default=None, metavar="PATH",
                   help="I3D (Kinetics-400) weights, .safetensors or a torch checkpoint: a state dict in InceptionI3d's key layout, such "
                        "as the i3d_pretrained_400.pt of the reference's videogpt method (a TorchScript archive is refused); allows fvd "
                        "in --metrics")
    p.add_argument("--fvd_channel_order", type=str, choices=("bgr", "rgb"), default="bgr",
                   help="bgr (default): the network sees B, G, R planes as in the reference, whose cv2.imread frames are never "
                        "swapped; rgb: the order I3D was trained on")
    p.add_argument("--latent_mse_weights", type=str, nargs="+", default=None, metavar="PATH",
                   help="Inception-v4 weights, .safetensors or a torch checkpoint: a state dict in timm inception_v4's key layout "
                        "(last_linear.* is ignored); allows latent_mse and loop_closure_latent_mse in --metrics")
    p.add_argument("--latent_mse_channel_order", type=str, choices=("bgr", "rgb"), default="bgr",
                   help="bgr (default): the network sees B, G, R planes under the ImageNet mean and std of R, G, B, as in the reference, "
                        "whose cv2.imread frames are never swapped; rgb: the order Inception-v4 was trained on")
    p.add_argument("--projection", type=str, choices=PROJECTIONS, default="equirect",
                   help="equirect (default): the frames as they are; cube: every clip is scored on its six 90-degree perspective "
                        "viewports (front, right, back, left, up, down), each (episode, face) one video of every selected metric")
    p.add_argument("--viewport_size", type=int, default=None, metavar="N", help="side of a cube viewport (default: frame width / 4)")
    args = p.parse_args(argv)
    args.result_file = os.path.join(args.data_path, args.result_file)
    return args


LATENT_METRICS = ("latent_mse", "loop_closure_latent_mse")


def selected_metrics(spec, lpips_weights=False, fvd_weights=False, latent_mse_weights=False, projection="equirect"):
    """The metric names of --metrics.  lpips_weights / fvd_weights / latent_mse_weights: the user supplied LPIPS / I3D / Inception-v4
    weights, which lifts the refusal of `lpips` and `ws_lpips` / `fvd` / both latent MSEs.  projection 'cube' refuses the ws_* names."""
    if projection not in PROJECTIONS:
        raise ValueError(f"projection {projection!r}: expected one of {', '.join(PROJECTIONS)}")
    names = [m.strip() for m in spec.split(",") if m.strip()]
    for m in names:
        if m in SPHERICAL:
            if projection == "cube":
                raise ValueError(f"metric {m!r} weights the rows of an equirectangular frame by latitude, which means nothing on a "
                                 f"perspective cube face: drop it or --projection cube")
            if m == "ws_lpips" and not lpips_weights:
                raise ValueError(f"metric {m!r} cannot be computed: it {NOT_COMPUTED['lpips']}")
            continue
        if (m == "lpips" and lpips_weights) or (m == "fvd" and fvd_weights) or (m in LATENT_METRICS and latent_mse_weights):
            continue
        if m in NOT_COMPUTED:
            raise ValueError(f"metric {m!r} cannot be computed: it {NOT_COMPUTED[m]}")
        if m not in SUPPORTED:
            raise ValueError(f"unknown metric {m!r} (computed: {', '.join(SUPPORTED + SPHERICAL[:2])}; not available: {', '.join(NOT_COMPUTED)})")
    if not names:
        raise ValueError("--metrics selects nothing")
    return names


def list_episode_folders(data_path, num_videos=None):
    """read_video_our's episode list (:185-190): the sorted sub-directories of data_path, the first num_videos of them."""
    eps = sorted(d for d in os.listdir(data_path) if os.path.isdir(os.path.join(data_path, d)))
    return eps[:num_videos] if num_videos else eps


def frame_pairs(data_path, episode, gt_subdir, gen_subdir, pair_by_name=False):
    """(gt paths, gen paths) of one episode: sorted(listdir)[-25:] of each folder (:191), or with pair_by_name the last 25 file
    names both folders hold.  ValueError naming the episode when the two counts differ (the reference fails its shape assert)."""
    gd, nd = os.path.join(data_path, episode, gt_subdir), os.path.join(data_path, episode, gen_subdir)
    gt, gen = sorted(os.listdir(gd)), sorted(os.listdir(nd))
    if pair_by_name:
        gt = gen = sorted(set(gt) & set(gen))[-SEQUENCE:]
        if not gt:
            raise ValueError(f"episode {episode}: {gt_subdir} and {gen_subdir} share no file name")
    else:
        gt, gen = gt[-SEQUENCE:], gen[-SEQUENCE:]
        if len(gt) != len(gen):
            raise ValueError(f"episode {episode}: {gt_subdir} holds {len(gt)} frames and {gen_subdir} holds {len(gen)}; the "
                             f"reference's shape assertion fails here (pair the shared frame names with --pair_by_name)")
    return [os.path.join(gd, f) for f in gt], [os.path.join(nd, f) for f in gen]


def evaluate(args, device="cuda"):
    """main(args) of calculate_all_metrics.py:209-236 for PSNR / SSIM: one episode at a time is decoded (thread pool) and streamed
    to the device as uint8.  Returns (result dict, timing dict)."""
    weights, fvd_weights = getattr(args, "lpips_weights", None), getattr(args, "fvd_weights", None)
    latent_weights = getattr(args, "latent_mse_weights", None)
    projection, viewport_size = getattr(args, "projection", "equirect"), getattr(args, "viewport_size", None)
    names = selected_metrics(args.metrics, lpips_weights=bool(weights), fvd_weights=bool(fvd_weights), latent_mse_weights=bool(latent_weights),
                             projection=projection)
    ws_what = 1 * ("ws_psnr" in names) | 2 * ("ws_ssim" in names)                # ops.METRIC_SSE | ops.METRIC_SSIM
    lpips_model, lpips_order, lpips, ws_lpips = None, getattr(args, "lpips_channel_order", "bgr"), [], []
    if "lpips" in names or "ws_lpips" in names:
        from .lpips import LPIPSAlex
        lpips_model = LPIPSAlex.from_files(weights, device)
    fvd_model, fvd_order, fvd_feats = None, getattr(args, "fvd_channel_order", "bgr"), ({}, {})     # {clip length: [logits per episode]}
    if "fvd" in names:
        from . import fvd as fvd_mod
        fvd_model = fvd_mod.I3D.from_files(fvd_weights, device)
    latent_model, latent_order, latent_feats = None, getattr(args, "latent_mse_channel_order", "bgr"), ([], [])   # [T,1536] per episode
    if any(m in names for m in LATENT_METRICS):
        from . import latent_mse as latent_mod
        latent_model = latent_mod.InceptionV4.from_files(latent_weights, device)
    episodes = list_episode_folders(args.data_path, args.num_videos)
    if not episodes:
        raise ValueError(f"no episode folders under {args.data_path}")
    psnr, ssim, ws_psnr, ws_ssim, shape, n_videos = [], [], [], [], None, 0
    t_decode = t_device = 0.0
    for ep in episodes:
        gp, np_ = frame_pairs(args.data_path, ep, args.gt_subdir, args.gen_subdir, args.pair_by_name)
        t0 = time.perf_counter()
        gt_d, gen_d = read_frames(gp, device), read_frames(np_, device)      # decode (thread pool) + upload, timed as decode
        t1 = time.perf_counter()
        gt_shape = tuple(gt_d.shape)
        if gt_d.shape != gen_d.shape:
            raise ValueError(f"episode {ep}: ground-truth frames {gt_shape} and generated frames {tuple(gen_d.shape)} differ")
        if shape is not None and gt_shape != shape:
            raise ValueError(f"episode {ep}: frames {gt_shape} differ from the first episode's {shape}")
        shape = gt_shape
        clips = [(gt_d, gen_d)]
        if projection == "cube":                                             # every (episode, face) is one video of every metric
            clips = list(zip(cube_viewports(gt_d, viewport_size), cube_viewports(gen_d, viewport_size)))
        for gt_c, gen_c in clips:
            p, s = video_metrics_u8(gt_c, gen_c)
            psnr.append(p)
            ssim.append(s)
            if ws_what:
                wp, wsm = video_metrics_ws_u8(gt_c, gen_c, ws_what)
                ws_psnr.append(wp)
                ws_ssim.append(wsm)
            if "lpips" in names:
                lpips.append(lpips_model(gt_c, gen_c, lpips_order).cpu().numpy())
            if "ws_lpips" in names:
                ws_lpips.append(lpips_model(gt_c, gen_c, lpips_order, row_weights=latitude_weights(gt_c.shape[1])).cpu().numpy())
            if fvd_model is not None:
                if shape[0] < 10:
                    raise ValueError(f"episode {ep}: FVD compares clips of 10 frames and more, the folders hold {shape[0]}")
                for feats, clip in zip(fvd_feats, (gt_c, gen_c)):            # ground truth first, as the reference's main
                    for L, v in fvd_mod.clip_features(fvd_model, clip, fvd_order).items():
                        feats.setdefault(L, []).append(v)
            if latent_model is not None:                                     # one pass per clip serves both metrics
                for feats, clip in zip(latent_feats, (gt_c, gen_c)):
                    feats.append(latent_model.features(clip, latent_order).cpu().numpy())
        n_videos += len(clips)
        t_device += time.perf_counter() - t1
        t_decode += t1 - t0
    T, H, W, C = shape
    if projection == "cube":
        H = W = int(viewport_size) if viewport_size else W // 4
    setting = torch.Size([T, C, H, W])
    result = {}
    if fvd_model is not None:
        from .ops import streamk_check
        streamk_check()                            # results leave here
        result["fvd"] = fvd_mod.fvd_result(*({L: np.stack(v) for L, v in f.items()} for f in fvd_feats),
                                           torch.Size([n_videos, C, T, H, W]))
    if "ssim" in names:
        result["ssim"] = aggregate(ssim, setting)
    if "psnr" in names:
        result["psnr"] = aggregate(psnr, setting)
    if "lpips" in names:
        result["lpips"] = aggregate(lpips, setting)
    if latent_model is not None:
        f_gt, f_gen = (np.stack(f) for f in latent_feats)                        # [B,T,1536], ground truth first as the reference's main
        side = latent_mod.SIDE
        if "latent_mse" in names:
            result["latent_mse"] = latent_mod.latent_mse_result(f_gt, f_gen, torch.Size([n_videos * T, C, side, side]))
        if "loop_closure_latent_mse" in names:                                   # video[:, -1:]: does the last frame come back to the start?
            result["loop_closure_latent_mse"] = latent_mod.latent_mse_result(f_gt[:, -1:], f_gen[:, -1:],
                                                                             torch.Size([n_videos, C, side, side]))
    for name, rows in (("ws_psnr", ws_psnr), ("ws_ssim", ws_ssim), ("ws_lpips", ws_lpips)):
        if name in names:
            result[name] = aggregate(rows, setting)
    if projection == "cube":
        result["projection"], result["viewport_size"] = "cube", H
    computed = {"lpips": "lpips" in result, "fvd": fvd_model is not None, **{m: m in result for m in LATENT_METRICS}}
    result["not_computed"] = {k: v for k, v in NOT_COMPUTED.items() if not computed.get(k, False)}
    return result, {"episodes": len(episodes), "frames": len(episodes) * T, "decode_s": t_decode, "device_s": t_device}


def main(argv=None):
    args = parse_args(argv)
    os.makedirs(os.path.dirname(args.result_file) or ".", exist_ok=True)
    result, timing = evaluate(args)
    print(json.dumps(result, indent=4))
    with open(args.result_file, "w") as f:
        json.dump(result, f, indent=4)
    print(f"metrics: {timing['episodes']} episodes, {timing['frames']} frame pairs; PNG decode {timing['decode_s']:.3f} s, "
          f"device {timing['device_s']:.3f} s -> {args.result_file}", file=sys.stderr)
    return result, timing


if __name__ == "__main__":
    main()
