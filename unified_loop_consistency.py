#!/usr/bin/env python
"""Drop-in entry point for the reference's `unified_loop_consistency.py` (CLI flags of :542-571, `main` :574-581) on the
MI355X-native hot path: U-Net denoising loop + reprojection on the device, one process per GPU, episodes sharded over ranks.

Same flags as the reference.  Additions (all optional):
  --stages pkg.mod:factory   provider of the out-of-scope networks (VAE, CLIP image encoder, VGGT); default = the synthetic,
                             weight-free stand-ins of `evoworld_amd.stages` so the script runs without checkpoints
  --random_init              random U-Net weights of the full architecture instead of loading --unet_path
  --num_inference_steps N    (reference fixes 25)
  --height/--width           (reference fixes 576x1024)
  --save_video               navigated.avi / original.avi per episode (Motion-JPEG, encoded on the device); --video_fps, --video_quality
  --device_png               the --save_frames PNG files are encoded on the device (evoworld_amd.png): same names and pixels, other bytes
  --qkv_fp8                  fp8 (e4m3) q / k / v projections in the U-Net's self-attention (BASELINE.json configs[4]); default off = fp16

Launch on N GPUs:  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 unified_loop_consistency.py ...
"""
import argparse
import json
import os
import time

import numpy as np
import torch


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(description="Unified Loop Consistency Pipeline (MI355X-native hot path)")
    p.add_argument("--unet_path", type=str, required=True, help="Path to UNet model")
    p.add_argument("--svd_path", type=str, default="stabilityai/stable-video-diffusion-img2vid-xt-1-1", help="Path to SVD model")
    p.add_argument("--base_folder", type=str, default="data/Curve_Loop/test", help="Base folder containing episodes")
    p.add_argument("--save_dir", type=str, default="unified_output", help="Output directory")
    p.add_argument("--dataset_name", type=str, default="CameraTrajDataset", help="Dataset name")
    p.add_argument("--num_data", type=int, default=1, help="Number of episodes to process")
    p.add_argument("--start_idx", type=int, default=0, help="Start index")
    p.add_argument("--num_segments", type=int, default=3, help="Number of segments to process")
    p.add_argument("--num_frames", type=int, default=25, help="Frames per segment")
    p.add_argument("--save_frames", action="store_true", help="Save intermediate frames")
    p.add_argument("--curve_path", action="store_true", help="Use curve path navigation")
    p.add_argument("--seed", type=int, default=42, help="Random seed")
    p.add_argument("--single_segment", action="store_true", help="Use single segment fast path")
    # additions
    p.add_argument("--stages", type=str, default=None)
    p.add_argument("--random_init", action="store_true")
    p.add_argument("--num_inference_steps", type=int, default=25)
    p.add_argument("--height", type=int, default=576)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--qkv_fp8", action="store_true", help="fp8 (e4m3) q/k/v projections in the U-Net self-attention (opt-in; default fp16)")
    p.add_argument("--export_glb", action="store_true",
                   help="write every hand-off's 3D memory as glbscene_{seg}.glb under the episode's output directory (with its memory panoramas)")
    p.add_argument("--memory_voxel_size", type=float, default=None,
                   help="voxel-grid downsample of the 3D memory before the splat and the export (opt-in; scene units)")
    p.add_argument("--save_video", action="store_true",
                   help="write navigated.avi (and original.avi for an episode with panoramas): Motion-JPEG encoded on the device")
    p.add_argument("--video_fps", type=float, default=10, help="frame rate of the --save_video files")
    p.add_argument("--video_quality", type=int, default=90, help="JPEG quality (1..100) of the --save_video files")
    p.add_argument("--device_png", action="store_true",
                   help="encode the --save_frames PNG files on the device (same names, same pixels, file bytes other than Pillow's)")
    p.add_argument("--depth_stage", choices=("synthetic", "mvs", "mvs_pano"), default="synthetic",
                   help="depth source of the memory hand-off: the stand-in's fixed room, plane-sweep stereo on the 90-degree views cut from the "
                        "generated frames (mvs, opt-in), or sphere-sweep stereo on the generated panoramas themselves (mvs_pano, opt-in)")
    p.add_argument("--mvs_planes", type=int, default=64, help="depth planes (mvs) / distance hypotheses (mvs_pano) of --depth_stage")
    p.add_argument("--mvs_sources", type=int, default=4, help="source views per reference view of --depth_stage mvs / mvs_pano")
    p.add_argument("--mvs_aggregate", choices=("box", "sgm"), default="box",
                   help="--depth_stage mvs / mvs_pano: the winner of the box-filtered cost (box), or after semi-global aggregation of the cost volume (sgm, opt-in)")
    p.add_argument("--mvs_p1", type=float, default=1.0,
                   help="--mvs_aggregate sgm: the penalty of a one-step change of hypothesis, in the cost's units: grey levels (--mvs_cost sad), percent of 1 - ZNCC (--mvs_cost zncc)")
    p.add_argument("--mvs_p2", type=float, default=8.0, help="--mvs_aggregate sgm: the penalty of a larger jump, in the same units; with --mvs_cost zncc a larger one, 32, recovered more of a weak, noisy, flickering scene than 8 (DESIGN.md 4.11)")
    p.add_argument("--mvs_paths", type=int, choices=(4, 8), default=4, help="--mvs_aggregate sgm: path directions")
    p.add_argument("--mvs_cost", choices=("sad", "zncc"), default="sad",
                   help="--depth_stage mvs / mvs_pano: match by the absolute difference of grey levels (sad), or by zero-mean normalised cross-correlation "
                        "over the same window (zncc, opt-in), which does not move when a frame's exposure or tone drifts")
    return p.parse_args(argv)


def load_camera_poses(episode_path):
    """camera_poses.txt -> [P,6] UNSCALED poses in the OpenCV convention (unified_loop_consistency.py:370-395)."""
    from evoworld_amd.dataset import load_camera_poses as _load
    return _load(episode_path)


def list_episodes(base_folder):
    """A folder holding camera_poses.txt is one episode; otherwise each sub-folder that holds one is
    (unified_loop_consistency.py `determine_data_config`)."""
    if os.path.isfile(os.path.join(base_folder, "camera_poses.txt")):
        return [base_folder]
    if not os.path.isdir(base_folder):
        return []
    return sorted(os.path.join(base_folder, d) for d in os.listdir(base_folder)
                  if os.path.isfile(os.path.join(base_folder, d, "camera_poses.txt")))


def synthetic_episode(n_poses=80):
    i = np.arange(n_poses, dtype=np.float64)
    return np.stack([0.04 * i * np.sin(i / 9), 0 * i, 0.04 * i * np.cos(i / 9), 0 * i, 95 + 3.6 * i, 0 * i], 1)


def synthetic_path_episode(num_segments, extra=8, step=0.4):
    """The episode of runs without --curve_path: straight runs of 25, 24, 24, ... poses joined by in-place 90-degree turns, the
    last run `extra` poses longer.  synthetic_episode turns at every pose, which the non-curve mode splits into 2-pose runs
    whose first hand-off has a single frame to align on (refused by evoworld_amd.inference.check_path_episode)."""
    rows, x, z = [], 0.0, 0.0
    for k in range(num_segments):
        yaw = 95.0 + 90.0 * k
        for _ in range((25 if k == 0 else 24) + (extra if k == num_segments - 1 else 0)):
            if rows:
                x, z = x + step * np.sin(np.deg2rad(yaw)), z + step * np.cos(np.deg2rad(yaw))
            rows.append([x, 0.0, z, 0.0, yaw, 0.0])
    return np.asarray(rows, np.float64)


def run_single_segment(args, ep, pipe, unet, dev, out_dir, synthetic):
    """The reference's single-segment fast path (`run_single_segment`, unified_loop_consistency.py:513-535): the dataset in
    'reprojection' mode hands out the episode's LAST 25 frames / poses (positions x pos_scale) with the PRE-RENDERED memory
    panoramas [panorama/001.png] + rendered_panorama_vggt_open3d/*.png, and the batch goes through forward_evoworld.process_batch
    with mask_mem=False.  Counterparts: evoworld_amd.dataset.load_single_segment_batch -> evoworld_amd.inference.process_batch."""
    from evoworld_amd import ops
    from evoworld_amd.dataset import load_single_segment_batch
    from evoworld_amd.frames import write_numbered
    from evoworld_amd.inference import process_batch
    from evoworld_amd.plucker import equirectangular_to_ray
    from evoworld_amd.stages import load_stages
    if synthetic:
        cam = synthetic_episode(max(args.num_frames, 25))
        traj = torch.tensor(cam[-args.num_frames:], dtype=torch.float32)
        traj[:, :3] *= 0.1
        g = torch.Generator().manual_seed(0)
        pix = (torch.rand(args.num_frames, 3, args.height, args.width, generator=g) * 2 - 1).to(dev)
        batch = {"pixel_values": pix[None], "cam_traj": traj[None], "memorized_pixel_values": torch.zeros_like(pix)[None]}
    else:
        cam = load_camera_poses(ep)
        batch = load_single_segment_batch(ep, args.height, args.width, dev, sequence_length=args.num_frames)
    stages = load_stages(args.stages, args, cross_attention_dim=unet._cfg["cross_attention_dim"], camera_params=cam)
    rays = torch.tensor(equirectangular_to_ray(args.height // 8, args.width // 8)).float().to(dev)
    args.mask_mem = False                                                                   # :532
    pipe.set_components(vae=stages.vae, image_encoder=stages.image_encoder, feature_extractor=stages.feature_extractor)
    torch.cuda.synchronize()
    t0 = time.time()
    # the pipeline encodes [first frame | memory] itself (aug-noise draw, VAE mode, CLIP) as the reference's does
    latents = process_batch(batch, args, pipe, rays, torch.float32, None, os.path.basename(ep), output_type="latent",
                            num_inference_steps=args.num_inference_steps)
    dec = pipe.decode_latents(latents, args.num_frames, 8)[0].permute(1, 0, 2, 3)                  # [T,3,H,W] in [-1,1]
    frames_u8 = ops.f32_chw_to_u8_hwc(dec.float().contiguous())
    torch.cuda.synchronize()
    dt = time.time() - t0
    if args.save_frames:
        write_numbered(os.path.join(out_dir, "predictions"), frames_u8, on_device=args.device_png)     # forward_evoworld.save_frames
        write_numbered(os.path.join(out_dir, "predictions_gt"), ops.f32_chw_to_u8_hwc(batch["pixel_values"][0].float().contiguous()),
                       on_device=args.device_png)
    if args.save_video:                                                                   # the clip and its ground truth, as process_episode names them
        from evoworld_amd.video import write_video
        write_video(os.path.join(out_dir, "navigated.avi"), frames_u8, fps=args.video_fps, quality=args.video_quality)
        write_video(os.path.join(out_dir, "original.avi"), batch["pixel_values"][0].float().to(dev), fps=args.video_fps, quality=args.video_quality)
    return {"episode": os.path.basename(ep), "frames": int(frames_u8.shape[0]), "seconds": round(dt, 3), "mode": "single_segment"}


def run_episode(args, ep, pipe, unet, dev, out_dir, synthetic):
    """N segments with evolving 3D memory (`process_episode`, unified_loop_consistency.py:398-492)."""
    from evoworld_amd.dataset import load_complete_episode_batch
    from evoworld_amd.frames import write_numbered
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.stages import load_stages
    if synthetic:                                                                                    # UNSCALED
        cam = synthetic_episode(24 * args.num_segments + 8) if args.curve_path else synthetic_path_episode(args.num_segments)
    else:
        cam = load_camera_poses(ep)
    stages = load_stages(args.stages, args, depth_stage=getattr(args, "depth_stage", None), cross_attention_dim=unet._cfg["cross_attention_dim"], camera_params=cam)
    start = None if synthetic else load_complete_episode_batch(ep, args.height, args.width, dev, cam=cam)["first_frame"]
    if start is None:
        g = torch.Generator().manual_seed(0)
        start = (torch.rand(3, args.height, args.width, generator=g) * 2 - 1).to(dev)
    pipe.set_components(vae=stages.vae, image_encoder=stages.image_encoder, feature_extractor=stages.feature_extractor)
    loop = UnifiedLoopConsistencyPipeline(pipe, stages.depth_model, height=args.height,
                                          width=args.width, num_frames=args.num_frames, num_segments=args.num_segments,
                                          num_inference_steps=args.num_inference_steps, curve_path=args.curve_path)
    torch.cuda.synchronize()
    t0 = time.time()
    # the unscaled poses go in; process_episode derives the pos-scaled Navigator / Plücker path itself (pos_scale = 0.1);
    # --save_frames also writes the reference's per-segment dumps predictions_{seg}/ and perspective_look_at_center_{seg}/
    # ... and, for an episode folder with panoramas, the ground-truth windows predictions_gt_{seg}/ (:437-439)
    frames = loop.process_episode(start, cam, save_dir=out_dir if args.save_frames or args.export_glb or args.save_video else None,
                                  save_segment_frames=args.save_frames, episode_path=None if synthetic else ep,
                                  export_memory=args.export_glb, memory_voxel_size=args.memory_voxel_size,
                                  save_video=args.save_video, video_fps=args.video_fps, video_quality=args.video_quality,
                                  png_on_device=args.device_png)
    torch.cuda.synchronize()
    dt = time.time() - t0
    if args.save_frames:
        write_numbered(os.path.join(out_dir, "predictions"), loop.last_frames_u8, on_device=args.device_png)
    return {"episode": os.path.basename(ep), "frames": int(frames.shape[0]), "seconds": round(dt, 3)}


def main(argv=None):
    args = parse_arguments(argv)
    from evoworld_amd import distributed as D
    from evoworld_amd.pipeline import StableVideoDiffusionPipeline
    from evoworld_amd.unet import UNetSpatioTemporalConditionModel

    rank, world, local = D.init()
    dev = f"cuda:{local}"
    torch.cuda.set_device(local)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    os.makedirs(args.save_dir, exist_ok=True)
    # rank 0 reads (or draws) the weights; the other ranks receive the packed set once over RCCL / xGMI
    sub = "unet" if os.path.isdir(os.path.join(args.unet_path, "unet")) else None
    fp8 = {"qkv_fp8": True} if args.qkv_fp8 else {}      # absent: the model's own default (fp16, or what EW_QKV_FP8 says); every rank builds the same layout
    if rank == 0 or world == 1:
        if args.random_init:
            unet = UNetSpatioTemporalConditionModel.from_random(seed=args.seed, device=dev, num_frames=args.num_frames, **fp8)
        else:
            unet = UNetSpatioTemporalConditionModel.from_pretrained(args.unet_path, subfolder=sub, device=dev, **fp8)
    else:
        cfg = {"num_frames": args.num_frames}
        root = os.path.join(args.unet_path, sub or "")
        if not args.random_init and os.path.exists(os.path.join(root, "config.json")):
            cfg = UNetSpatioTemporalConditionModel.read_config(root)
        unet = UNetSpatioTemporalConditionModel.from_zeros(device=dev, **cfg, **fp8)
    if world > 1:
        unet.broadcast_weights(src=0)
    pipe = StableVideoDiffusionPipeline(unet=unet)

    episodes = list_episodes(args.base_folder)[args.start_idx: args.start_idx + args.num_data]
    synthetic = not episodes
    if synthetic:
        episodes = [f"synthetic_{i:03d}" for i in range(args.start_idx, args.start_idx + args.num_data)]
    mine = D.shard_clips(len(episodes), rank, world)
    report = []
    for idx in mine:
        ep = episodes[idx]
        out_dir = os.path.join(args.save_dir, os.path.basename(ep.rstrip("/")))
        os.makedirs(out_dir, exist_ok=True)
        if args.single_segment:
            rec = run_single_segment(args, ep, pipe, unet, dev, out_dir, synthetic)
        else:
            rec = run_episode(args, ep, pipe, unet, dev, out_dir, synthetic)
        rec["rank"] = rank
        report.append(rec)
        print(json.dumps(rec), flush=True)
    D.barrier()
    D.shutdown()
    return report


if __name__ == "__main__":
    main()
