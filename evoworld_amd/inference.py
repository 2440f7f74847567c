"""Inference drivers of the hot path -- the build's counterparts of the reference callers:

  prepare_batch_data / process_batch     <- evoworld/inference/forward_evoworld.py:119-211          (C1, single clip)
  Navigator.move_forward / navigate_curve_path / split_curve_into_segments / extend_segment
                                         <- evoworld/inference/navigator_evoworld.py:146-154,173-231,303-318,394-448  (C2)
  Navigator.navigate_path / split_path_into_segments / rotate_panorama
                                         <- evoworld/inference/navigator_evoworld.py:276-301,335-392,466-512  (C2, non-curve mode)
  Navigator.convert_panorama_to_cubemap / precompute_rotation_matrix / cubemap_to_equirectangular
                                         <- evoworld/inference/navigator_evoworld.py:514-705,707-743,745-864  (C2, skybox export)
  Navigator.save_video / save_gif        <- evoworld/inference/navigator_evoworld.py:233-274               (C2, clip export)
  UnifiedLoopConsistencyPipeline.process_episode / convert_pano_to_pers
                                         <- unified_loop_consistency.py:299-334,398-492               (C3, N-segment loop)

Same tensor preparation and pipeline kwargs (decode_chunk_size=8, motion_bucket_id=127, fps=7, noise_aug_strength=0.02,
mask_mem, per-window generator re-seeded with torch.manual_seed(-1)).  Differences, all device-side: frames stay tensors
(no PIL / PNG / numpy round-trips between the stages, SURVEY.md §3.2 'a native design keeps all of this on-device'); the
depth network (VGGT-1B, out of scope) is a duck-typed callable `depth_model(perspective_frames_u8) -> predictions dict`.
File output (PNG dumps) is optional and off the hot path.
"""
import logging
import os

import numpy as np
import torch

from . import ops
from . import reprojection as RP
from .dataset import load_gt_window_u8
from .frames import numbered_paths, pil_to_rgb, write_numbered
from .geometry import UNITY_TO_OPENCV, xyz_euler_to_four_by_four_matrix_batch, xyz_euler_to_three_by_four_matrix_batch
from .mvs import call_depth_model
from .plucker import equirectangular_to_ray, ray_c2w_to_plucker

logger = logging.getLogger(__name__)


# ------------------------------------------------------------------ C1: single clip
def prepare_batch_data(batch, args, rays, weight_dtype=torch.float32):
    """batch: pixel_values [B,T,3,H,W] in [-1,1], cam_traj [B,T,6] (RDF, pos-scaled), memorized_pixel_values [B,T,3,H,W]
    -> (first_frame, camera_traj [B,T,3,4], plucker_embedding [B,T,6,H/8,W/8], memorized_pixel_values, images)."""
    images = batch["pixel_values"]
    first_frame = images[:, 0].cuda()
    raw = batch["cam_traj"].cuda()
    B = raw.shape[0]
    camera_traj = torch.zeros(B, args.num_frames, 3, 4, dtype=weight_dtype, device="cuda")
    plucker = torch.zeros(B, args.num_frames, 6, args.height // 8, args.width // 8, dtype=weight_dtype, device="cuda")
    for i in range(B):
        camera_traj[i] = xyz_euler_to_three_by_four_matrix_batch(raw[i], relative=True)
        plucker[i] = ray_c2w_to_plucker(rays, camera_traj[i])
    return first_frame, camera_traj, plucker, batch["memorized_pixel_values"].cuda(), images


def process_batch(batch, args, pipeline, rays, weight_dtype=torch.float32, output_path=None, episode="episode", **pipe_kw):
    """One clip through the pipeline with the reference's fixed kwargs; returns the pipeline's frames (and saves PNGs when
    output_path is given and the frames are PIL images)."""
    first_frame, _traj, plucker, memory, images = prepare_batch_data(batch, args, rays, weight_dtype)
    frames = pipeline(first_frame, height=args.height, width=args.width, num_frames=args.num_frames, decode_chunk_size=8,
                      motion_bucket_id=127, fps=7, noise_aug_strength=0.02, plucker_embedding=plucker,
                      memorized_pixel_values=memory, mask_mem=args.mask_mem, **pipe_kw).frames
    if output_path and isinstance(frames, list):
        d = os.path.join(output_path, episode, "predictions")
        os.makedirs(d, exist_ok=True)
        for f, path in zip(frames[0], numbered_paths(d, len(frames[0]))):
            f.save(path)
    return frames


# ------------------------------------------------------------------ C2: windowed navigation
class Navigator:
    def __init__(self, pipe, height=576, width=1024, num_frames=25, fps=7, step_size=0.4, position_scale=0.1):
        self.pipe, self.model_height, self.model_width, self.num_frames, self.fps = pipe, height, width, num_frames, fps
        self.step_size, self.position_scale = step_size, position_scale            # navigator_evoworld.py:49-52
        self.rays = torch.tensor(equirectangular_to_ray(height // 8, width // 8)).float().cuda()
        self.memorized_images = None
        self.generations = []

    split_curve_into_segments = staticmethod(RP.split_curve_into_segments)

    def extend_segment(self, segment, n):
        """Extrapolate a short window to n poses (navigator_evoworld.py:132-172): a 1-pose window steps forward by
        step_size*position_scale along its yaw; a longer one continues with the last xyz increment, rotation held (the
        reference asserts the last two rotations agree)."""
        if len(segment) == 0:
            return segment
        seg = segment if isinstance(segment, torch.Tensor) else torch.stack(list(segment), dim=0)
        if len(seg) == 1:
            roty = seg[0][4]
            dz = self.step_size * torch.cos(torch.deg2rad(roty)) * self.position_scale
            dx = self.step_size * torch.sin(torch.deg2rad(roty)) * self.position_scale
            step = torch.stack([dx, torch.zeros_like(dx), dz, torch.zeros_like(dx), torch.zeros_like(dx), torch.zeros_like(dx)]).to(seg)
            return torch.cat([seg] + [seg[-1:] + step[None] * (i + 1) for i in range(n - 1)], dim=0)
        if len(seg) < n:
            last, prev = seg[-1], seg[-2]
            if not torch.allclose(last[3:], prev[3:]):
                raise AssertionError("The rotation of the last two steps are not the same.")
            delta = last - prev
            extra = torch.stack([last + delta * (i + 1) for i in range(n - len(seg))], dim=0)
            return torch.cat([seg, extra], dim=0)
        return seg

    def move_forward(self, image, segment, num_model_frames=25, num_inference_steps=25, noise_aug_strength=0.02,
                     use_memory=False, **pipe_kw):
        """One 25-pose window (navigator_evoworld.py:173-231): relative c2w -> Plücker -> pipeline with a CPU generator
        re-seeded per window (every segment starts from identical noise), mask_mem = not use_memory."""
        n = len(segment)
        if n < num_model_frames:
            segment = self.extend_segment(segment, num_model_frames)
        raw = segment if isinstance(segment, torch.Tensor) else torch.stack(list(segment), dim=0)
        raw = raw.cuda().float()
        c2w = xyz_euler_to_three_by_four_matrix_batch(raw, relative=True)
        pl = ray_c2w_to_plucker(self.rays, c2w)
        generator = torch.manual_seed(-1)                                   # navigator_evoworld.py:198
        frames = self.pipe(image.unsqueeze(0), num_frames=self.num_frames, width=self.model_width, height=self.model_height,
                           decode_chunk_size=8, generator=generator, motion_bucket_id=127, fps=self.fps,
                           num_inference_steps=num_inference_steps, noise_aug_strength=noise_aug_strength,
                           plucker_embedding=pl[:25].unsqueeze(0), memorized_pixel_values=self.memorized_images.clone(),
                           mask_mem=not use_memory, **pipe_kw).frames
        return frames, n

    @staticmethod
    def _last_frame_tensor(frames, n):
        """the window's last generated frame as the next window's start image (navigator :436-437: movement[-1] through
        the ToTensor + rescale transform)"""
        if isinstance(frames, list):                      # PIL clips [[img]*T]
            return (torch.from_numpy(pil_to_rgb(frames[0][n - 1])).permute(2, 0, 1).float() / 255.0 * 2 - 1).cuda()
        raise NotImplementedError("chaining windows needs decoded frames (output_type='pil'); with output_type='latent' "
                                  "run one window per call (infer_segment=True), as process_episode does")

    def generated_frames_u8(self):
        """The frames save_video / save_gif export: of every window in self.generations its first n frames (the poses the window was
        asked for), as uint8 [N,H,W,3] on the device, resized to the navigator's image size with Pillow's BICUBIC
        (navigator_evoworld.py:241, :263) -- on the device through reprojection.resize_u8, skipped when the size already matches.
        A window is a PIL clip list (output_type='pil'), a uint8 array [B,T,H,W,3] ('np') or a tensor [B,T,3,H,W] in [0,1] ('pt').
        None when there is no generation."""
        parts = []
        for frames, n in self.generations:
            if isinstance(frames, list):
                u8 = torch.from_numpy(np.stack([pil_to_rgb(f) for f in frames[0][:n]])).cuda()
            elif isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.ndim == 5:
                u8 = torch.from_numpy(np.ascontiguousarray(frames[0][:n])).cuda()
            elif isinstance(frames, torch.Tensor) and frames.ndim == 5 and frames.shape[2] == 3:
                u8 = (frames[0, :n].float().clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cuda()
            elif isinstance(frames, torch.Tensor):
                raise NotImplementedError(f"a generation of shape {tuple(frames.shape)} holds latents (output_type='latent'), not images: "
                                          "decode them first (pipe.decode_latents, or process_episode(save_video=True), which "
                                          "writes the decoded episode)")
            else:
                raise TypeError(f"cannot export a generation of type {type(frames).__name__}")
            if len(u8):
                parts.append(RP.resize_u8(u8, self.model_height, self.model_width, filter="pillow_bicubic"))
        return torch.cat(parts, dim=0) if parts else None

    def save_video(self, save_path, fps=10):
        """The generated windows as one video file (navigator_evoworld.py:233-257).  The reference hands the frames to imageio /
        ffmpeg; here they are encoded on the device as Motion-JPEG and wrapped in an AVI (evoworld_amd.video.write_video: quality
        90, 4:2:0), so save_path must end in .avi.  Nothing is written (and that is logged) when there is no generation."""
        from .video import write_video
        frames = self.generated_frames_u8()
        if frames is None:
            logger.info("No Movement to Export.")
            return
        write_video(save_path, frames, fps=fps)
        logger.info("Video saved as %s", save_path)

    def save_gif(self, save_path, fps=10):
        """The generated windows as an animated GIF (navigator_evoworld.py:259-274): Pillow on the host, save_all with
        duration = int(1000 / fps) ms and loop = 0, exactly as the reference does.  GIF is an LZW-coded palette format of
        thumbnail-sized use; it is not worth a kernel, only the BICUBIC resize in front of it runs on the device."""
        from PIL import Image
        frames = self.generated_frames_u8()
        if frames is None:
            logger.info("No Movement to Export.")
            return
        imgs = [Image.fromarray(f) for f in frames.cpu().numpy()]
        imgs[0].save(save_path, save_all=True, append_images=imgs[1:], duration=int(1000 / fps), loop=0)
        logger.info("GIF saved as %s", save_path)

    @staticmethod
    def split_path_into_segments(path):
        """Straight runs between turns (navigator_evoworld.py:276-301): a row whose rotation differs from the previous one
        (torch.allclose, atol = rtol = 1e-5) starts a new segment whose first pose is the previous position with the new
        rotation.  -> list of [n,6] float32 tensors on the host.
        The reference writes into its input when two consecutive rows each turn (`last_step = step` is a row view that the
        next `last_step[3:6] = ...` writes through); its episode flow never sees that, since every call gets a fresh device
        copy of the poses.  This runs the same steps on a private copy, so the caller's tensor is never modified."""
        p = torch.as_tensor(path).detach().to("cpu", torch.float32, copy=True)
        segments, current = [], []
        last = p[0]
        for step in p:
            if torch.allclose(step[3:6], last[3:6], atol=1e-5):
                current.append(step.clone())
                last = step.clone()
                continue
            segments.append(current)
            last[3:6] = step[3:6]
            current = [last.clone(), step.clone()]
            last = step
        if current:
            segments.append(current)
        return [torch.stack(s) for s in segments]

    @staticmethod
    def rotate_panorama(image, rotation_degrees):
        """Yaw rotation of one panorama (navigator_evoworld.py:466-512), bit-exact, one kernel (ew_pano_yaw_rotate): image fp32
        [3,H,W] or the 8-bit frame uint8 [H,W,3] (converted x/255*2-1 in the same pass) -> fp32 [3,H,W].  Unlike a plain
        integer roll the map is not the identity even at 0 degrees: callers rotate only for a non-zero turn, as the reference."""
        return ops.pano_yaw_rotate(image[None].contiguous(), torch.as_tensor(rotation_degrees, dtype=torch.float32).reshape(1))[0]

    @staticmethod
    def _clip_u8(x, what):
        """(uint8 [V,H,W,3] device tensor, kind) of a PIL image, a device [H,W,3] frame or a [V,H,W,3] clip."""
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.uint8 or x.ndim not in (3, 4) or x.shape[-1] != 3:
                raise TypeError(f"{what}: expected a PIL image or a device uint8 [H,W,3] / [V,H,W,3] tensor, got {x.dtype} {tuple(x.shape)}")
            return (x[None] if x.ndim == 3 else x), ("frame" if x.ndim == 3 else "clip")
        return torch.from_numpy(pil_to_rgb(x))[None].cuda(), "pil"

    @staticmethod
    def _like(t, kind):
        if kind == "clip":
            return t
        if kind == "frame":
            return t[0]
        from PIL import Image
        return Image.fromarray(t[0].cpu().numpy())

    @classmethod
    def convert_panorama_to_cubemap(cls, panorama_image, interpolation=True, scale_factor=2):
        """Panorama -> (cubemap, faces) as navigator_evoworld.py:514-705, on the device: LANCZOS x scale_factor, the cube cross
        (ew_equi2cube_u8: bilinear, or nearest with interpolation=False), LANCZOS back to (W0, int(W0*3/4)).  `cubemap` is the
        downscaled cross; `faces` is a dict in the reference's key order right, left, top, bottom, front, back, cut from the
        SCALED cross (edge scale_factor*W0/4).  A PIL image gives PIL images; a device uint8 [H,W,3] frame or [V,H,W,3] clip gives
        device tensors (faces [E,E,3] / [V,E,E,3], views of the scaled cross), a whole clip in one launch per stage.
        The panorama must be 2:1 (AssertionError otherwise, as the reference): the model's 1024x576 frames are not -- resize them
        first, e.g. reprojection.resize_u8(frames, 512, 1024) (ops.resize_aa_u8 with Pillow's bilinear tables).
        Reference behaviour kept: the bilinear blend is truncated, not rounded (a flat area of value A can come out A - 1), and
        the neighbours are clipped, not wrapped, at the seam; nearest mode leaves the seam pixel whose column rounds to W black."""
        x, kind = cls._clip_u8(panorama_image, "panorama_image")
        cubemap, faces = RP.panorama_to_cubemap(x, interpolation, scale_factor)
        return cls._like(cubemap, kind), {n: cls._like(f, kind) for n, f in faces.items()}

    precompute_rotation_matrix = staticmethod(RP.precompute_rotation_matrix)

    @classmethod
    def cubemap_to_equirectangular(cls, cubemap_faces, output_width, output_height, scale_factor=2):
        """Faces dict -> panorama as navigator_evoworld.py:745-864, on the device: the reference's integer gather at scale_factor
        x the output size (host LUT in float64, ew_cube2equi_gather), then LANCZOS down when scale_factor > 1.  The dict's key
        order does not matter; a face that is missing renders black.  PIL faces give a PIL image; device uint8 [res,res,3] /
        [V,res,res,3] faces give a device [H,W,3] / [V,H,W,3] tensor.  The faces of one call must be square and of one size
        (the reference also takes faces of mixed sizes; ValueError here)."""
        conv = {n: cls._clip_u8(f, f"cubemap_faces[{n!r}]") for n, f in cubemap_faces.items()}
        kind = next(iter(conv.values()))[1] if conv else "pil"
        pano = RP.cubemap_to_panorama({n: t.contiguous() for n, (t, _) in conv.items()}, output_width, output_height, scale_factor)
        return cls._like(pano, kind)

    @classmethod
    def turn_start_image(cls, image, rotation_degrees):
        """The start image of a run after a turn of `rotation_degrees` (navigator_evoworld.py:368-370): rotated when the turn is
        non-zero, as it is; fp32 [3,H,W] or uint8 [H,W,3] (rotated and converted in one pass) -> fp32 [3,H,W]."""
        if rotation_degrees != 0:
            return cls.rotate_panorama(image, rotation_degrees)
        if image.dtype == torch.uint8:
            return ops.u8_hwc_to_f32_chw(image[None].contiguous())[0]
        return image

    @classmethod
    def path_turn(cls, path, segment_id):
        """The turn navigate_path applies before segment `segment_id`: seg_k[0].yaw - seg_{k-1}[-1].yaw (0 for the first)."""
        segs = cls.split_path_into_segments(path)
        return segs[segment_id][0][4] - segs[segment_id - 1][-1][4] if segment_id else torch.zeros(())

    def navigate_path(self, path, start_image, num_inference_steps=25, memorized_images=None, infer_segment=False,
                      segment_id=None, **pipe_kw):
        """The non-curve mode (navigator_evoworld.py:335-392): one window per straight run of split_path_into_segments; at
        each turn the current panorama is rotated in place by seg_k[0].yaw - seg_{k-1}[-1].yaw (only when that is non-zero),
        then move_forward walks the run (extended to 25 poses when shorter; a longer run yields the pipeline's 25 frames).
        With infer_segment only segment `segment_id` is generated (the skipped ones still advance the heading); otherwise
        every segment starts from the previous one's last frame.  start_image: fp32 [3,H,W] in [-1,1] or the 8-bit frame
        uint8 [H,W,3] (turned and converted in one kernel pass).  Leaves current_pose = the last pose of the last generated
        segment."""
        self.memorized_images = memorized_images.clone()
        segments = self.split_path_into_segments(path)
        generations, current = [], 0
        angle = segments[0][0][4]
        image = start_image
        for k, segment in enumerate(segments):
            rotation = segment[0][4] - angle
            angle = segment[-1][4]
            if segment_id is not None and current < segment_id and infer_segment:
                current += 1
                continue
            image = self.turn_start_image(image, rotation)
            frames, n = self.move_forward(image, segment, num_inference_steps=num_inference_steps,
                                          use_memory=(segment_id != 0), **pipe_kw)
            generations.append((frames, n))
            self.current_pose = segment[-1].clone()                      # move_forward's camera_trajectory_raw[n - 1] (:229)
            current += 1
            if (infer_segment and current > segment_id) or k == len(segments) - 1:
                break
            image = self._last_frame_tensor(frames, min(n, self.num_frames))     # movement[-1] of frames[:n] (:223,383)
        self.generations = generations
        return generations

    def navigate_curve_path(self, path, start_image, num_inference_steps=25, memorized_images=None, infer_segment=False,
                            segment_id=None, **pipe_kw):
        """Windows [0:25],[24:49],... ; with infer_segment only window `segment_id` is generated (navigator :394-448);
        otherwise every window starts from the previous window's last frame."""
        self.memorized_images = memorized_images.clone()
        segments = self.split_curve_into_segments(path)
        generations, current = [], 0
        image = start_image
        for segment in segments:
            if segment_id is not None and current < segment_id and infer_segment:
                current += 1
                continue
            if len(segment) != 0:
                frames, n = self.move_forward(image, segment, num_inference_steps=num_inference_steps,
                                              use_memory=(segment_id != 0), **pipe_kw)
                generations.append((frames, n))
                last_window = (infer_segment and current + 1 > segment_id) or segment is segments[-1]
                if not last_window:
                    image = self._last_frame_tensor(frames, n)
            current += 1
            if infer_segment and current > segment_id:
                break
        self.generations = generations
        return generations


# ------------------------------------------------------------------ C3: N-segment loop with evolving 3D memory
class UnifiedLoopConsistencyPipeline:
    """process_episode of unified_loop_consistency.py:398-492 with every stage on the device.
    `frames_from_latents(latents[1,T,4,h,w]) -> float [T,3,H,W] in [-1,1]` stands for the VAE decode (row N1);
    `depth_model(persp_u8 [F,384,512,3]) -> dict(depth, depth_conf, images, extrinsic, intrinsic)` stands for VGGT (row N4); one that
    declares `wants_view_poses = True` (evoworld_amd.mvs.PlaneSweepDepth) is called with `view_w2c=mvs.view_poses(...)` as well, and one
    that declares `wants_panoramas = True` (evoworld_amd.mvs.SphereSweepDepth) with the panoramas so far and `pano_w2c=mvs.pano_poses(...)`
    instead of the views."""

    def __init__(self, pipeline, depth_model, frames_from_latents=None, height=576, width=1024, num_frames=25, num_segments=3,
                 num_inference_steps=25, pano_size=(1000, 2000), face_res=512, curve_path=True):
        self.nav = Navigator(pipeline, height, width, num_frames)
        self.curve_path = curve_path                    # --curve_path: navigate_curve_path; False: navigate_path (:255,285)
        self.depth_model, self.frames_from_latents = depth_model, frames_from_latents
        self.height, self.width, self.num_frames, self.num_segments = height, width, num_frames, num_segments
        self.steps = num_inference_steps
        self.equi2pers = RP.Equi2Pers(height=384, width=512, fov_x=90.0, mode="bilinear")      # :178-183
        self.pano_size, self.renderer = pano_size, RP.CubemapRenderer(face_res=face_res)

    def convert_pano_to_pers(self, frames_u8, camera_params, segment_id):
        """frames uint8 [F,H,W,3] (device; the 8-bit frames the reference holds as PIL images) -> uint8 [F,384,512,3] +
        target yaws in degrees (:299-334).  camera_params: UNSCALED poses (camera_poses.txt)."""
        yaws = RP.calculate_target_yaws(camera_params, frames_u8.shape[0], segment_id)
        pers = self.equi2pers.batch(frames_u8, [{"pitch": 0, "roll": 0, "yaw": float(y)} for y in yaws])
        return pers, yaws / np.pi * 180.0

    def process_episode(self, start_image, camera_params, image_latents_fn=None, save_dir=None, pos_scale=0.1,
                        save_segment_frames=False, episode_path=None, export_memory=False, memory_voxel_size=None,
                        save_video=False, video_fps=10, video_quality=90, png_on_device=False, **pipe_kw):
        """start_image float [3,H,W] in [-1,1]; camera_params [P,6] numpy: the UNSCALED RDF poses of camera_poses.txt
        (unified_loop_consistency.py:370-395), used as they are for the target yaws and the reprojection alignment; the
        Navigator / Plücker path gets the copy with xyz * pos_scale that the dataset hands out as batch['cam_traj']
        (dataset/CameraTrajDataset.py:223,348).

        Default (image_latents_fn=None, the reference's flow): the PIPELINE owns `vae` and `image_encoder` and every window
        is one `pipe(image, generator=torch.manual_seed(-1), memorized_pixel_values=...)` call, so the generator's first draw
        is the [1+T,3,H,W] augmentation noise and its second the latents (pipeline_evoworld.py:596-600, then :663-673 ->
        :401-435; navigator_evoworld.py:198) -- same seed, same noise as the reference.  Frames are decoded by the
        pipeline's `decode_latents` (chunks of 8).
        With `image_latents_fn(first_frame, memory [T,3,H,W]) -> dict(image_latents=[1,1+T,4,h,w], image_embeddings=[1,1,X])`
        (stand-ins for VAE-encode + CLIP; decode through `frames_from_latents`) the conditioning is injected; the pipeline
        still consumes draw #1 from the generator so that the latents stay the generator's second draw.
        Every generated frame is carried as the 8-bit image the reference's PIL frames hold (:418-419, navigator :214-226).
        With save_dir and save_segment_frames, the per-segment dumps of :432-453 are written: predictions_{seg}/NNN.png
        (the segment's new frames, NNN continuing at seg*(T-1)+1) and perspective_look_at_center_{seg}/NNN.png (the
        pano->pers views fed to the depth network).  Returns all generated frames float [N,3,H,W] in [-1,1] (25 -> 49 -> 73 ...) on the 8-bit grid.
        With curve_path=False segment k is the k-th straight run of Navigator.split_path_into_segments (navigate_path): its start
        image is the last 8-bit frame rotated by the turn, and only the run's first n frames are kept (frames[:n], so the
        counts follow the runs' lengths); ValueError when the path or the episode cannot carry num_segments segments.
        With save_segment_frames and an `episode_path` whose panorama/NNN.png exist, predictions_gt_{seg}/NNN.png is written too
        (:437-439): the window's ground-truth panoramas (ids start_idx+1 .. end_idx of calculate_segment_indices), Pillow-exact
        resized and passed through the reference's tensor_to_pil round trip (ops.gt_dump_map_u8), numbered like predictions_{seg}.
        With export_memory and a save_dir, every hand-off also writes its 3D memory as glbscene_{seg}.glb (memory.SceneMemory: the very
        cloud the panoramas are rendered from, with the depth network's cameras; reproject_vggt_open3d.py:245-265).  memory_voxel_size
        (opt-in) thins that cloud by a voxel-grid downsample before the splat (and the export); None leaves the path as it is.
        With save_video and a save_dir, navigated.avi holds all generated frames -- the very uint8 tensor that is returned -- as
        Motion-JPEG encoded on the device (evoworld_amd.video; video_fps, video_quality), and, for an `episode_path` with ground-truth
        panoramas, original.avi holds the frames load_gt_window_u8 yields for the same poses (panorama ids 1 .. N, frame for frame
        beside navigated.avi): the pair calculate_scores.py loads per episode (there as .mp4).  The returned frames do not depend on it.
        With png_on_device (opt-in) every PNG named above -- the per-segment dumps and the memory panoramas -- is encoded on the device
        (evoworld_amd.png): same names, the same pixels for any decoder, other file bytes than Pillow's."""
        dev = start_image.device
        camera_params = np.asarray(camera_params, dtype=np.float64)
        cam_t = torch.tensor(camera_params, dtype=torch.float32, device=dev)
        cam_t[:, :3] *= pos_scale
        gt_window = lambda a, b: None if episode_path is None else load_gt_window_u8(episode_path, a, b, self.height, self.width, dev,
                                                                                     len(camera_params))
        out = _EpisodeOutputs(save_dir, save_segment_frames, export_memory, save_video and {"fps": video_fps, "quality": video_quality},
                              png_on_device, stride=self.num_frames - 1, gt_window=gt_window)
        all_u8 = None
        memory = torch.zeros(self.num_frames, 3, self.height, self.width, device=dev)       # 'empty_with_traj' memory
        if not self.curve_path:
            runs = self.nav.split_path_into_segments(cam_t)
            check_path_episode([len(r) for r in runs], len(camera_params), self.num_segments, self.num_frames)
        for seg in range(self.num_segments):
            start_idx, end_idx, _ = RP.calculate_segment_indices(seg)
            if self.curve_path:
                first = start_image if seg == 0 else ops.u8_hwc_to_f32_chw(all_u8[-1:])[0]    # pil_to_tensor(tensor_to_pil(.)) (:418-419)
                cond = image_latents_fn(first, memory) if image_latents_fn is not None else {}
                gens = self.nav.navigate_curve_path(cam_t, first, num_inference_steps=self.steps, memorized_images=memory[None],
                                                    infer_segment=True, segment_id=seg, output_type="latent", **cond, **pipe_kw)
            else:
                # the last 8-bit frame: navigate_path turns it by the heading change between the two runs and converts it in
                # one kernel pass (navigator :365-370); injected conditioning sees the same turned image
                first = start_image if seg == 0 else all_u8[-1]
                cond = {}
                if image_latents_fn is not None:
                    cond = image_latents_fn(self.nav.turn_start_image(first, self.nav.path_turn(cam_t, seg)), memory)
                gens = self.nav.navigate_path(cam_t, first, num_inference_steps=self.steps, memorized_images=memory[None],
                                              infer_segment=True, segment_id=seg, output_type="latent", **cond, **pipe_kw)
            latents, n = gens[-1]
            if self.frames_from_latents is None:                                          # the pipeline's own VAE decodes (chunks of 8)
                pipe = self.nav.pipe
                dec = pipe.decode_latents(latents, self.num_frames, 8)[0].permute(1, 0, 2, 3)      # [T,3,H,W] in [-1,1]
            else:
                dec = self.frames_from_latents(latents)
            frames_u8 = ops.f32_chw_to_u8_hwc(dec.float().contiguous())
            if not self.curve_path:
                frames_u8 = frames_u8[:n]                                               # frames[:num_frames] (navigator :223)
            if all_u8 is not None:
                frames_u8 = frames_u8[1:]                                               # drop the duplicated first frame (:427-429)
            out.segment(seg, frames_u8, start_idx, end_idx)                             # :432-439
            all_u8 = frames_u8 if all_u8 is None else torch.cat([all_u8, frames_u8], dim=0)
            if seg < self.num_segments - 1:
                pers, target_yaws = self.convert_pano_to_pers(all_u8, camera_params, seg)
                out.perspective(seg, pers)                                                # :449-453
                temp_cam = camera_params.copy()
                s = max(0, end_idx - len(target_yaws))
                temp_cam[s:end_idx, 4] = target_yaws[: end_idx - s]                        # :456-459
                if getattr(self.depth_model, "wants_panoramas", False):                   # opt-in: the stage reads the panoramas, not the crops
                    preds = call_depth_model(self.depth_model, pers, camera_params, seg, panos_u8=all_u8)
                else:
                    preds = call_depth_model(self.depth_model, pers, camera_params, seg)    # a stage that wants them also gets the views' poses
                poses = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(temp_cam, dtype=torch.float32), relative=True)
                outdir, glb, save_png = out.memory(seg)
                panos = RP.predictions_to_target_view(preds, poses.numpy(), conf_thres=50.0, prediction_mode="depth_unproject",
                                                      num_target_view=24, outdir=outdir, cubemap_renderer=_Sized(self.renderer, self.pano_size),
                                                      return_device_tensor=True, save_png=save_png, voxel_size=memory_voxel_size,
                                                      export_glb=glb, png_on_device=png_on_device)
                mem24 = RP.memory_to_pixel_values(panos, self.height, self.width)           # [24,3,H,W]
                memory = torch.cat([start_image[None], mem24], dim=0)                      # [episode frame 1] + 24 reprojected (:277-279)
        self.last_frames_u8 = all_u8
        out.finish(all_u8)
        return ops.u8_hwc_to_f32_chw(all_u8)


def check_path_episode(run_lengths, n_poses, num_segments, num_frames=25):
    """States of the non-curve episode loop that the reference cannot get through, refused before any work (ValueError naming
    the segment): a segment beyond the path's last straight run (navigate_path generates nothing for it); a memory hand-off
    that has fewer than 2 generated frames (segment k keeps min(run, T) frames, minus the shared first one for k > 0; one
    frame leaves the first-and-last-point alignment without a direction, reproject_vggt_open3d_utils.py:1126-1213, and the
    target poses singular); or one whose 24 target views (poses (seg+1)*24+1 ... +24, :487-492) run past the episode."""
    have = 0
    for seg in range(num_segments):
        if seg >= len(run_lengths):
            raise ValueError(f"segment {seg}: the path splits into only {len(run_lengths)} straight run(s) between turns")
        have += min(run_lengths[seg], num_frames) - (1 if seg else 0)
        if seg == num_segments - 1:
            break
        if have < 2:
            raise ValueError(f"segment {seg}: the memory hand-off would align on {have} generated frame(s) (straight runs "
                             f"of {run_lengths[:seg + 1]} poses); it needs at least 2")
        need = (seg + 2) * 24 + 1
        if n_poses < need:
            raise ValueError(f"segment {seg}: the memory for segment {seg + 1} renders target poses {need - 24}..{need - 1}, "
                             f"but the episode has {n_poses} poses")


# What an episode leaves under save_dir (unified_loop_consistency.py:432-453, 487-492; T frames per segment); nothing without one:
#   predictions_{seg}/NNN.png                   the segment's new frames, NNN going on at seg * (T - 1) + 1          save_segment_frames
#   predictions_gt_{seg}/NNN.png                their ground truth, numbered alike, where the episode has panoramas  save_segment_frames
#   perspective_look_at_center_{seg}/NNN.png    the views handed to the depth stage, from 001                        save_segment_frames
#   rendered_panorama_vggt_open3d_{seg}/NN.png  the 24 memory panoramas of the hand-off, from 00                     any save_dir
#   glbscene_{seg}.glb                          the 3D memory of the hand-off                                        export_memory
#   navigated.avi, original.avi                 all generated frames; their ground truth, where there is one         save_video
class _EpisodeOutputs:
    """Every file name and every `if save_dir` of process_episode.  video: write_video's keywords or None; stride: T - 1;
    gt_window(first, end): the ground-truth frames uint8 [n,H,W,3] of poses first .. end - 1, or None."""

    def __init__(self, save_dir, segment_frames, export_memory, video, png_on_device, stride, gt_window):
        self.dir, self.png_on_device, self.stride, self.gt_window = save_dir, png_on_device, stride, gt_window
        self.dumps, self.glb, self.video = bool(save_dir and segment_frames), bool(save_dir and export_memory), save_dir and video

    def segment(self, seg, frames_u8, start_idx, end_idx):
        if self.dumps:
            write_numbered(os.path.join(self.dir, f"predictions_{seg}"), frames_u8, seg * self.stride, self.png_on_device)
            gt = self.gt_window(start_idx, end_idx)
            if gt is not None:
                write_numbered(os.path.join(self.dir, f"predictions_gt_{seg}"), ops.gt_dump_map_u8(gt), seg * self.stride, self.png_on_device)

    def perspective(self, seg, pers):
        if self.dumps:
            write_numbered(os.path.join(self.dir, f"perspective_look_at_center_{seg}"), pers, 0, self.png_on_device)

    def memory(self, seg):
        """(outdir, glb path or None, save_png) of predictions_to_target_view.  outdir is more than a destination: its _{seg} suffix selects
        the target poses (SceneBuilder.align_extrinsics), so it is named even when nothing is saved."""
        if self.glb:
            os.makedirs(self.dir, exist_ok=True)
        return (os.path.join(self.dir or "", f"rendered_panorama_vggt_open3d_{seg}"),
                os.path.join(self.dir, f"glbscene_{seg}.glb") if self.glb else None, bool(self.dir))

    def finish(self, all_u8):
        if self.video:
            from .video import write_video
            os.makedirs(self.dir, exist_ok=True)
            write_video(os.path.join(self.dir, "navigated.avi"), all_u8, **self.video)
            gt = self.gt_window(0, all_u8.shape[0])
            if gt is not None:
                write_video(os.path.join(self.dir, "original.avi"), gt, **self.video)


class _Sized:
    def __init__(self, cr, pano_size):
        self.cr, self.pano_size = cr, pano_size

    def render_cubemaps_to_panoramas(self, v, c, target, n, outdir, **kw):
        return self.cr.render_cubemaps_to_panoramas(v, c, target, n, outdir, width=self.pano_size[1], height=self.pano_size[0], **kw)
