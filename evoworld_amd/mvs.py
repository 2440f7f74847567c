"""Plane-sweep multi-view stereo: a weight-free depth stage for the N-segment loop.

The reference gets depth, confidence and cameras from VGGT-1B (unified_loop_consistency.py:336-368).  In this loop the cameras are
known -- the perspective views fed to the depth stage are cut from the generated panoramas at poses the episode file states -- so depth
can come from geometry instead of a network: every view is swept against its neighbours over planes of constant depth
(ew_mvs_plane_sweep), the winners are cross-checked between views (ew_mvs_consistency), and the result has the duck type of the
depth network's predictions.  It is opt-in (`--depth_stage mvs`); how it compares with VGGT is not measured.

  view_poses       the world->camera matrices of the views `UnifiedLoopConsistencyPipeline.convert_pano_to_pers` produces
  sweep_setup      sources per view, inverse depths, homographies (host, float64)
  PlaneSweepDepth  the callable: uint8 views [F,H,W,3] on the device -> predictions dict (device tensors)
  python -m evoworld_amd.mvs cloud --frames DIR --poses camera_poses.txt --segment K --output scene.ply|.glb

The same stage on the panoramas themselves (`--depth_stage mvs_pano`): the views above are 90-degree crops cut near the
direction of motion, where parallax is least; the sphere sweep reads the whole equirectangular frame (ew_mvs_sphere_sweep,
ew_mvs_sphere_consistency) and lifts spherically (ew_pano_unproject), so the cloud covers every direction.

  pano_poses        the world->camera matrices of the panorama cameras, in the frame view_poses(..., relative=True) defines
  sphere_setup      sources per panorama, inverse distances, relative poses (host, float64)
  SphereSweepDepth  the callable: uint8 panoramas [F,He,We,3] on the device -> predictions dict with world_points_from_depth
  python -m evoworld_amd.mvs cloud --stage sphere [--sweep_size H W] ...

Both stages take the winner of a box-filtered cost; `aggregate="sgm"` (opt-in) puts semi-global aggregation between the
cost and the winner, for surfaces with little texture: the sweep stores its quantised cost volume (ew_mvs_*_sweep_volume), 1-D dynamic
programmes along 4 or 8 path directions are summed (ew_mvs_sgm_aggregate), and the sweeps' winner, parabola and confidence rules run on
the sum (ew_mvs_sgm_select), in chunks of views that fit a workspace.

  sgm_options / sgm_chunk_views / sgm_sweep    the checked options, the views per chunk, the chunked volume -> aggregate -> select path
  python -m evoworld_amd.mvs cloud --aggregate sgm [--sgm_p1 1 --sgm_p2 8 --sgm_paths 4] ...

Both match views by the absolute difference of grey levels; `cost="zncc"` (opt-in) matches by zero-mean normalised
cross-correlation over the same window instead (ew_mvs_*_sweep_zncc, ew_mvs_*_sweep_zncc_volume), which does not move when a frame's
exposure, contrast or tone drifts against its neighbours'.  Winner, parabola, confidence, consistency and the semi-global path are unchanged.

  cost_options    the checked options
  python -m evoworld_amd.mvs cloud --cost zncc ...
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

from .geometry import xyz_euler_to_four_by_four_matrix_batch


def pinhole(height, width):
    """float64 [3,3]: the 90-degree pinhole of the views (f = W / 2, centre (W / 2, H / 2)), as the stand-in states it and
    ew_equi2pers renders it (pixel index x <-> ray ((x - W / 2) / f, (y - H / 2) / f, 1))."""
    f = width / 2.0
    return np.array([[f, 0, width / 2.0], [0, f, height / 2.0], [0, 0, 1]], np.float64)


def view_poses(camera_params, n_frames, segment_id, relative=True):
    """float64 [F,3,4] world->camera of the perspective views convert_pano_to_pers cuts from the first n_frames panoramas, in the
    convention ew_depth_unproject expects (x right, y down, z forward; Xc = R Xw + t).  camera_params: the UNSCALED [P,6] poses of
    camera_poses.txt, as the alignment uses them.  A view's camera is its panorama's camera (xyz_euler_to_four_by_four_matrix_batch)
    turned by the view's own rotation, Equi2Pers.rotation at the yaw calculate_target_yaws gives -- the float32 camera->panorama
    matrix ew_equi2pers is handed.  relative: in the frame of the first VIEW (its matrix is the identity), which is what a depth
    network reports; otherwise in the frame the poses are given in."""
    from . import reprojection as RP
    cam = np.asarray(camera_params, dtype=np.float64)
    if n_frames < 1 or n_frames > len(cam):
        raise ValueError(f"n_frames = {n_frames} must be 1 .. {len(cam)} (the poses of the episode)")
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(cam[:n_frames], dtype=torch.float64), relative=False).numpy()
    yaws = RP.calculate_target_yaws(cam, n_frames, segment_id)
    for i, y in enumerate(yaws):
        turn = np.eye(4)
        turn[:3, :3] = RP.Equi2Pers.rotation({"pitch": 0, "roll": 0, "yaw": float(y)}).astype(np.float64)
        c2w[i] = c2w[i] @ turn
    if relative:
        c2w = np.linalg.inv(c2w[0])[None] @ c2w
    return np.linalg.inv(c2w)[:, :3, :4]


def pano_poses(camera_params, n_frames, segment_id):
    """float64 [F,3,4] world->camera of the panorama cameras of the first n_frames frames (x right, y down, z forward: the frame in which
    ew_equi2pers' direction <-> pixel map is stated).  The panorama camera is xyz_euler_to_four_by_four_matrix_batch on the UNSCALED
    poses; world = the frame of the first perspective VIEW, exactly as view_poses(..., relative=True) defines it -- so a sphere cloud and
    a plane-sweep cloud of one episode share a frame, and the camera centres equal those of the views (a view only turns its panorama's
    camera on the spot)."""
    from . import reprojection as RP
    cam = np.asarray(camera_params, dtype=np.float64)
    if n_frames < 1 or n_frames > len(cam):
        raise ValueError(f"n_frames = {n_frames} must be 1 .. {len(cam)} (the poses of the episode)")
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(cam[:n_frames], dtype=torch.float64), relative=False).numpy()
    yaw0 = RP.calculate_target_yaws(cam, n_frames, segment_id)[0]
    first_view = c2w[0].copy()
    turn = np.eye(4)
    turn[:3, :3] = RP.Equi2Pers.rotation({"pitch": 0, "roll": 0, "yaw": float(yaw0)}).astype(np.float64)
    first_view = first_view @ turn
    c2w = np.linalg.inv(first_view)[None] @ c2w
    return np.linalg.inv(c2w)[:, :3, :4]


def _w2c_4x4(w2c):
    w = np.asarray(w2c.detach().cpu() if isinstance(w2c, torch.Tensor) else w2c, dtype=np.float64)
    if w.ndim != 3 or w.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError(f"w2c must be [F,3,4] or [F,4,4], got {w.shape}")
    E = np.tile(np.eye(4), (len(w), 1, 1))
    E[:, :3, :4] = w[:, :3, :4]
    return E


def choose_sources(centres, n_src, min_baseline=1e-6):
    """int32 [F, n_src]: per view the n_src nearest views by index distance (i-1, i+1, i-2, i+2, ...) whose camera centre is more
    than min_baseline away; a slot that cannot be filled is -1.  At an end of the sequence the slots fill from the one side there is."""
    F = len(centres)
    out = np.full((F, n_src), -1, np.int32)
    for i in range(F):
        got = 0
        for d in range(1, F):
            for j in (i - d, i + d):
                if 0 <= j < F and got < n_src and np.linalg.norm(centres[j] - centres[i]) > min_baseline:
                    out[i, got] = j
                    got += 1
    return out


def sweep_setup(w2c, K, n_src, D, z_near=None, z_far=None, min_baseline=1e-6):
    """What ew_mvs_plane_sweep and ew_mvs_consistency need, computed on the host in float64 (the *_f32 members are the uploads):
      src_index [F,n_src] int32 (choose_sources); baseline [F,n_src]; z_near, z_far [F]; inv_depth [F,D], uniform in inverse depth from
      1 / z_far (plane 0) to 1 / z_near (plane D - 1); homographies [F,n_src,D,3,3], reference pixel -> source pixel:
      K_s (R + t e3^T / z) K_r^-1 for the plane of depth z in the reference camera; rel_pose [F,n_src,3,4], reference camera -> source
      camera.  Default range per view: z_far = f b_max -- one pixel of disparity over the view's widest baseline -- and z_near = z_far / D,
      so that one plane step is one pixel of disparity at that baseline.  A view without a source sweeps the single depth z_far of the
      nearest view that has one (1.0 when none has)."""
    E = _w2c_4x4(w2c)
    F = len(E)
    K = np.asarray(K, np.float64)
    K = np.broadcast_to(K, (F, 3, 3)) if K.ndim == 2 else K
    if n_src < 1 or D < 1:
        raise ValueError(f"n_src = {n_src} and D = {D} must be positive")
    c2w = np.linalg.inv(E)
    centres = c2w[:, :3, 3]
    src = choose_sources(centres, n_src, min_baseline)
    base = np.where(src >= 0, np.linalg.norm(centres[np.maximum(src, 0)] - centres[:, None], axis=-1), 0.0)
    has = (src >= 0).any(1)
    far = np.where(has, K[:, 0, 0] * base.max(1), 0.0) if z_far is None else np.broadcast_to(np.asarray(z_far, np.float64), (F,)).copy()
    for i in np.flatnonzero(~has):                 # nothing to sweep against: the neighbour's far plane
        with_src = np.flatnonzero(has)
        far[i] = far[with_src[np.argmin(np.abs(with_src - i))]] if len(with_src) else 1.0
    near = far / D if z_near is None else np.broadcast_to(np.asarray(z_near, np.float64), (F,)).copy()
    near = np.where(has, near, far)
    t = np.linspace(0.0, 1.0, D) if D > 1 else np.zeros(1)
    inv_depth = 1.0 / far[:, None] + t[None] * (1.0 / near - 1.0 / far)[:, None]
    rel = np.zeros((F, n_src, 4, 4))
    Hs = np.zeros((F, n_src, D, 3, 3))
    e3 = np.array([0.0, 0.0, 1.0])
    for i in range(F):
        Kinv = np.linalg.inv(K[i])
        for s in range(n_src):
            j = src[i, s]
            if j < 0:
                rel[i, s] = np.eye(4)
                Hs[i, s] = np.eye(3)
                continue
            T = E[j] @ c2w[i]
            rel[i, s] = T
            Hs[i, s] = K[j] @ (T[:3, :3][None] + np.outer(T[:3, 3], e3)[None] * inv_depth[i][:, None, None]) @ Kinv
    return SimpleNamespace(src_index=src, baseline=base, z_near=near, z_far=far, inv_depth=inv_depth, homographies=Hs,
                           rel_pose=rel[:, :, :3, :4].copy(), K=K.copy(), has_source=has,
                           inv_depth_f32=inv_depth.astype(np.float32), homographies_f32=Hs.astype(np.float32),
                           rel_pose_f32=rel[:, :, :3, :4].astype(np.float32))


def sphere_setup(pano_w2c, We, n_src, D, d_near=None, d_far=None, min_baseline=1e-6):
    """What ew_mvs_sphere_sweep and ew_mvs_sphere_consistency need, computed on the host in float64 (the *_f32 members are the uploads):
      src_index [F,n_src] int32 (choose_sources); baseline [F,n_src]; d_near, d_far [F]; inv_dist [F,D], uniform in inverse distance from
      1 / d_far (hypothesis 0) to 1 / d_near (hypothesis D - 1); rel_pose [F,n_src,3,4], reference panorama camera -> source panorama
      camera.  Default range per view: d_far = b_max We / (2 pi) -- one pixel of angular disparity over the view's widest baseline -- and
      d_near = d_far / D.  A view without a source sweeps the single distance d_far of the nearest view that has one (1.0 when none has),
      as sweep_setup does."""
    E = _w2c_4x4(pano_w2c)
    F = len(E)
    if n_src < 1 or D < 1 or We < 1:
        raise ValueError(f"n_src = {n_src}, D = {D} and We = {We} must be positive")
    c2w = np.linalg.inv(E)
    centres = c2w[:, :3, 3]
    src = choose_sources(centres, n_src, min_baseline)
    base = np.where(src >= 0, np.linalg.norm(centres[np.maximum(src, 0)] - centres[:, None], axis=-1), 0.0)
    has = (src >= 0).any(1)
    far = np.where(has, base.max(1) * We / (2 * np.pi), 0.0) if d_far is None else np.broadcast_to(np.asarray(d_far, np.float64), (F,)).copy()
    for i in np.flatnonzero(~has):                 # nothing to sweep against: the neighbour's far sphere
        with_src = np.flatnonzero(has)
        far[i] = far[with_src[np.argmin(np.abs(with_src - i))]] if len(with_src) else 1.0
    near = far / D if d_near is None else np.broadcast_to(np.asarray(d_near, np.float64), (F,)).copy()
    near = np.where(has, near, far)
    t = np.linspace(0.0, 1.0, D) if D > 1 else np.zeros(1)
    inv_dist = 1.0 / far[:, None] + t[None] * (1.0 / near - 1.0 / far)[:, None]
    rel = np.tile(np.eye(4), (F, n_src, 1, 1))
    for i in range(F):
        for s in range(n_src):
            if src[i, s] >= 0:
                rel[i, s] = E[src[i, s]] @ c2w[i]
    return SimpleNamespace(src_index=src, baseline=base, d_near=near, d_far=far, inv_dist=inv_dist, rel_pose=rel[:, :, :3, :4].copy(),
                           has_source=has, inv_dist_f32=inv_dist.astype(np.float32), rel_pose_f32=rel[:, :, :3, :4].astype(np.float32))


AGGREGATES = ("box", "sgm")
COSTS = ("sad", "zncc")
COST_SCALES = {"sad": 32.0, "zncc": 16.0}          # volume units per grey level (sad: 127.97 grey levels clip) / per percent (zncc: 200 % -> 3200)


def cost_options(cost="sad", patch_radius=2, var_floor=1.0, cost_scale=None):
    """The checked matching-cost options of the two stages -> SimpleNamespace(cost, var_floor, cost_scale): cost_scale
    None resolves to COST_SCALES[cost].  A cost outside COSTS, patch_radius 0 with "zncc" (a single tap has no variance), a var_floor that
    is negative or not finite: ValueError naming the value."""
    if cost not in COSTS:
        raise ValueError(f"cost must be one of {COSTS}, got {cost!r}")
    if cost == "zncc" and patch_radius == 0:
        raise ValueError(f"cost = 'zncc' takes patch_radius 1 .. 3 (a single tap has no variance), got {patch_radius!r}")
    try:
        vf = float(var_floor)
    except (TypeError, ValueError):
        raise ValueError(f"var_floor = {var_floor!r} must be a number") from None
    if not (vf >= 0 and np.isfinite(vf)):
        raise ValueError(f"var_floor = {var_floor!r} must be finite and not negative")
    return SimpleNamespace(cost=cost, var_floor=vf, cost_scale=COST_SCALES[cost] if cost_scale is None else cost_scale)


def sgm_options(aggregate="box", sgm_p1=1.0, sgm_p2=8.0, sgm_paths=4, cost_scale=32.0, workspace_bytes=2 << 30):
    """The checked semi-global options of the two stages -> SimpleNamespace(aggregate, sgm_p1, sgm_p2 in the cost's own
    units -- grey levels for the sad cost, percent of 1 - ZNCC for the zncc cost;
    P1, P2 = int(round(p cost_scale)), the penalties in the units of the quantised volume; paths; cost_scale; workspace_bytes).
    aggregate outside ("box", "sgm"), 0 <= P1 <= P2 <= 4095 violated, paths outside {4, 8}, a cost_scale that is not positive and
    finite or a workspace below one byte: ValueError."""
    if aggregate not in AGGREGATES:
        raise ValueError(f"aggregate must be one of {AGGREGATES}, got {aggregate!r}")
    cost_scale = float(cost_scale)
    if not (cost_scale > 0 and np.isfinite(cost_scale)):
        raise ValueError(f"cost_scale = {cost_scale!r} must be positive and finite")
    if not (np.isfinite(sgm_p1) and np.isfinite(sgm_p2)):
        raise ValueError(f"sgm_p1 = {sgm_p1!r} and sgm_p2 = {sgm_p2!r} must be finite")
    P1, P2 = int(round(float(sgm_p1) * cost_scale)), int(round(float(sgm_p2) * cost_scale))
    if not 0 <= P1 <= P2 <= 4095:
        raise ValueError(f"0 <= P1 <= P2 <= 4095 does not hold for sgm_p1 = {sgm_p1!r}, sgm_p2 = {sgm_p2!r} at cost_scale = {cost_scale!r} "
                         f"(P1 = {P1}, P2 = {P2})")
    if sgm_paths not in (4, 8):
        raise ValueError(f"sgm_paths must be 4 or 8, got {sgm_paths!r}")
    if int(workspace_bytes) < 1:
        raise ValueError(f"workspace_bytes = {workspace_bytes!r} must be positive")
    return SimpleNamespace(aggregate=aggregate, sgm_p1=float(sgm_p1), sgm_p2=float(sgm_p2), P1=P1, P2=P2, paths=int(sgm_paths),
                           cost_scale=cost_scale, workspace_bytes=int(workspace_bytes))


def sgm_chunk_views(workspace_bytes, H, W, D):
    """Views per chunk of the semi-global path: the cost volume and the aggregated one, uint16 [n,H,W,D] each, fit workspace_bytes --
    max(1, workspace_bytes // (4 H W D))."""
    return max(1, int(workspace_bytes) // (4 * int(H) * int(W) * int(D)))


def sgm_sweep(volume, inv, src_index, F, H, W, D, opt):
    """The semi-global path of both stages, in chunks of sgm_chunk_views views: volume(view_begin, n_views, out) -> the chunk's cost
    volume, then ops.mvs_sgm_aggregate, then ops.mvs_sgm_select into the chunk's slice of the four outputs.  Views are aggregated
    independently, so the chunk size does not change a bit of the result.  -> (depth, conf, winner, winner cost), each [F,H,W]."""
    from . import ops
    dev = inv.device
    n = min(F, sgm_chunk_views(opt.workspace_bytes, H, W, D))
    cost = torch.empty((n, H, W, D), dtype=torch.uint16, device=dev)
    agg = torch.empty((n, H, W, D), dtype=torch.uint16, device=dev)
    outs = [torch.empty((F, H, W), dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]
    for b in range(0, F, n):
        m = min(n, F - b)
        volume(b, m, cost[:m])
        ops.mvs_sgm_aggregate(cost[:m], opt.P1, opt.P2, opt.paths, out=agg[:m])
        ops.mvs_sgm_select(agg[:m], inv, src_index, view_begin=b, out=[o[b:b + m] for o in outs])
    return tuple(outs)


def call_depth_model(depth_model, pers_u8, camera_params, segment_id, panos_u8=None):
    """How process_episode calls its depth stage: a stage that declares `wants_panoramas` is called with the episode's panoramas so far
    (panos_u8) and their world->camera matrices (pano_poses) instead of the views; one that declares `wants_view_poses` gets the views and
    their world->camera matrices (view_poses); any other callable is called with the views alone, exactly as before."""
    if getattr(depth_model, "wants_panoramas", False):
        if panos_u8 is None:
            raise ValueError("a depth stage that declares wants_panoramas needs panos_u8, the panoramas the views were cut from")
        return depth_model(panos_u8, pano_w2c=pano_poses(camera_params, len(panos_u8), segment_id))
    if getattr(depth_model, "wants_view_poses", False):
        return depth_model(pers_u8, view_w2c=view_poses(camera_params, len(pers_u8), segment_id))
    return depth_model(pers_u8)


class PlaneSweepDepth:
    """The depth stage: `__call__(views uint8 [F,H,W,3] on the device, view_w2c [F,3,4])` -> the predictions dict of the depth network's
    duck type, as device tensors: depth [F,H,W,1], depth_conf [F,H,W], images [F,3,H,W] (the frames / 255), extrinsic [F,3,4] (view_w2c),
    intrinsic [F,3,3] (pinhole).  n_src sources per view, `planes` depth planes (sweep_setup); patch_radius and oob_cost as
    ew_mvs_plane_sweep; a pixel keeps its confidence when at least min_consistent sources hold a depth within rel_tol of its own
    (min_consistent is capped at the number of sources a view has; 0 switches the check off).  Without view_w2c the poses come from
    view_poses(camera_params, F, segment_id), the segment inferred from F = 25 + 24 k when it is not given.
    aggregate="sgm" (opt-in; "box", the default, is the fused sweep as before): the winner is taken after semi-global aggregation of the
    quantised cost volume (sgm_options, sgm_sweep) -- sgm_p1 / sgm_p2 the penalties in grey levels, sgm_paths 4 or 8,
    cost_scale the volume's units per grey level, workspace_bytes what the two volumes of a chunk of views may take.
    cost="zncc" (opt-in; "sad", the default, is the sweep as before): the matching cost is 100 (1 - ZNCC) over the window instead of the
    mean absolute difference, for views whose exposure, contrast or tone drift (cost_options) -- var_floor in grey levels
    squared, zncc_oob_cost the cost in percent of a source whose window leaves it (oob_cost stays the sad cost's, in grey levels);
    sgm_p1 / sgm_p2 are then in percent, and cost_scale (None: 32 for sad, 16 for zncc) in volume units per percent."""
    wants_view_poses = True

    def __init__(self, camera_params=None, n_src=4, planes=64, patch_radius=2, oob_cost=48.0, min_consistent=2, rel_tol=0.02,
                 z_near=None, z_far=None, min_baseline=1e-6, segment_id=None, aggregate="box", sgm_p1=1.0, sgm_p2=8.0, sgm_paths=4,
                 cost_scale=None, workspace_bytes=2 << 30, cost="sad", var_floor=1.0, zncc_oob_cost=100.0):
        self.match = cost_options(cost, patch_radius, var_floor, cost_scale)
        self.cost, self.var_floor, self.zncc_oob_cost = cost, self.match.var_floor, float(zncc_oob_cost)
        self.sgm = sgm_options(aggregate, sgm_p1, sgm_p2, sgm_paths, self.match.cost_scale, workspace_bytes)
        self.aggregate = aggregate
        if aggregate == "sgm" and not 1 <= planes <= 256:
            raise ValueError(f"aggregate = 'sgm' takes 1 .. 256 planes, got {planes!r}")
        if patch_radius not in (0, 1, 2, 3):
            raise ValueError(f"patch_radius must be 0 .. 3, got {patch_radius!r}")
        if n_src < 1 or planes < 1:
            raise ValueError(f"n_src = {n_src} and planes = {planes} must be positive")
        self.camera_params = None if camera_params is None else np.asarray(camera_params, np.float64)
        self.n_src, self.planes, self.patch_radius, self.oob_cost = int(n_src), int(planes), int(patch_radius), float(oob_cost)
        self.min_consistent, self.rel_tol = int(min_consistent), float(rel_tol)
        self.z_near, self.z_far, self.min_baseline, self.segment_id = z_near, z_far, min_baseline, segment_id
        self.last_setup = None

    def _poses(self, n):
        if self.camera_params is None:
            raise ValueError("PlaneSweepDepth needs view_w2c, or camera_params to derive it from")
        seg = self.segment_id
        if seg is None:
            if n < 25 or (n - 25) % 24:
                raise ValueError(f"cannot infer the segment from {n} views (25 + 24 k expected): pass segment_id or view_w2c")
            seg = (n - 25) // 24
        return view_poses(self.camera_params, n, seg)

    def __call__(self, pers_u8, view_w2c=None):
        from . import ops
        if not isinstance(pers_u8, torch.Tensor) or pers_u8.dtype != torch.uint8 or pers_u8.ndim != 4 or pers_u8.shape[3] != 3:
            raise TypeError("PlaneSweepDepth: the views must be a device uint8 [F,H,W,3] tensor")
        F, H, W, _ = pers_u8.shape
        dev = pers_u8.device
        w2c = self._poses(F) if view_w2c is None else view_w2c
        K = pinhole(H, W)
        st = sweep_setup(w2c, K, self.n_src, self.planes, self.z_near, self.z_far, self.min_baseline)
        self.last_setup = st
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        src = up(st.src_index)
        grey = ops.mvs_luma(pers_u8.contiguous())
        if self.aggregate == "sgm":
            homog, inv = up(st.homographies_f32), up(st.inv_depth_f32)
            if self.cost == "zncc":
                volume = lambda b, m, out: ops.mvs_plane_sweep_zncc_volume(grey, homog, src, inv, self.patch_radius, self.zncc_oob_cost,
                                                                           self.var_floor, self.sgm.cost_scale, b, m, out=out)
            else:
                volume = lambda b, m, out: ops.mvs_plane_sweep_volume(grey, homog, src, inv, self.patch_radius, self.oob_cost,
                                                                      self.sgm.cost_scale, b, m, out=out)
            depth, conf, _, _ = sgm_sweep(volume, inv, src, F, H, W, self.planes, self.sgm)
        elif self.cost == "zncc":
            depth, conf, _, _ = ops.mvs_plane_sweep_zncc(grey, up(st.homographies_f32), src, up(st.inv_depth_f32), self.patch_radius,
                                                         self.zncc_oob_cost, self.var_floor)
        else:
            depth, conf, _, _ = ops.mvs_plane_sweep(grey, up(st.homographies_f32), src, up(st.inv_depth_f32), self.patch_radius, self.oob_cost)
        need = min(self.min_consistent, int((st.src_index >= 0).sum(1).max()))
        if need > 0:
            ops.mvs_consistency(depth, up(st.rel_pose_f32), src, conf, K[0, 0], K[1, 1], K[0, 2], K[1, 2], self.rel_tol, need)
        E = _w2c_4x4(w2c)[:, :3, :4]
        return {"depth": depth[..., None], "depth_conf": conf, "images": pers_u8.permute(0, 3, 1, 2).float() / 255,
                "extrinsic": up(E.astype(np.float32)), "intrinsic": up(np.repeat(K[None].astype(np.float32), F, 0))}


class SphereSweepDepth:
    """The depth stage on the panoramas: `__call__(panoramas uint8 [F,He,We,3] on the device, pano_w2c [F,3,4])` -> the predictions dict
    predictions_to_target_view(..., prediction_mode="depth_unproject") consumes, as device tensors: world_points_from_depth [F,h,w,3]
    (ew_pano_unproject, in the frame pano_w2c is given in), depth_conf [F,h,w], depth [F,h,w,1] (the RADIAL distance), images [F,3,h,w]
    (the swept frames / 255), extrinsic [F,3,4] (pano_w2c).  There is no `intrinsic`: the lift is spherical and already done.  n_src
    sources per panorama, `planes` distance hypotheses (sphere_setup); patch_radius as ew_mvs_sphere_sweep; a pixel keeps its confidence
    when at least min_consistent sources hold a distance within rel_tol of its own (capped at the number of sources a view has; 0
    switches the check off).  sweep_size = (h, w): the panoramas are first resized on the device (ops.resize_linear_u8); default: native
    size.  Without pano_w2c the poses come from pano_poses(camera_params, F, segment_id), the segment inferred from F = 25 + 24 k.
    aggregate, sgm_p1, sgm_p2, sgm_paths, cost_scale, workspace_bytes: as PlaneSweepDepth (the paths do not wrap across the seam).
    cost, var_floor: as PlaneSweepDepth (every direction lands in a source panorama: there is no out-of-image cost)."""
    wants_panoramas = True

    def __init__(self, camera_params=None, n_src=4, planes=64, patch_radius=2, min_consistent=2, rel_tol=0.02, d_near=None, d_far=None,
                 sweep_size=None, segment_id=None, min_baseline=1e-6, aggregate="box", sgm_p1=1.0, sgm_p2=8.0, sgm_paths=4,
                 cost_scale=None, workspace_bytes=2 << 30, cost="sad", var_floor=1.0):
        self.match = cost_options(cost, patch_radius, var_floor, cost_scale)
        self.cost, self.var_floor = cost, self.match.var_floor
        self.sgm = sgm_options(aggregate, sgm_p1, sgm_p2, sgm_paths, self.match.cost_scale, workspace_bytes)
        self.aggregate = aggregate
        if aggregate == "sgm" and not 1 <= planes <= 256:
            raise ValueError(f"aggregate = 'sgm' takes 1 .. 256 planes, got {planes!r}")
        if patch_radius not in (0, 1, 2, 3):
            raise ValueError(f"patch_radius must be 0 .. 3, got {patch_radius!r}")
        if n_src < 1 or planes < 1:
            raise ValueError(f"n_src = {n_src} and planes = {planes} must be positive")
        if sweep_size is not None and (len(sweep_size) != 2 or min(sweep_size) < 1):
            raise ValueError(f"sweep_size must be (h, w), got {sweep_size!r}")
        self.camera_params = None if camera_params is None else np.asarray(camera_params, np.float64)
        self.n_src, self.planes, self.patch_radius = int(n_src), int(planes), int(patch_radius)
        self.min_consistent, self.rel_tol = int(min_consistent), float(rel_tol)
        self.d_near, self.d_far, self.min_baseline, self.segment_id = d_near, d_far, min_baseline, segment_id
        self.sweep_size = None if sweep_size is None else (int(sweep_size[0]), int(sweep_size[1]))
        self.last_setup = None

    def _poses(self, n):
        if self.camera_params is None:
            raise ValueError("SphereSweepDepth needs pano_w2c, or camera_params to derive it from")
        seg = self.segment_id
        if seg is None:
            if n < 25 or (n - 25) % 24:
                raise ValueError(f"cannot infer the segment from {n} panoramas (25 + 24 k expected): pass segment_id or pano_w2c")
            seg = (n - 25) // 24
        return pano_poses(self.camera_params, n, seg)

    def __call__(self, panos_u8, pano_w2c=None):
        from . import ops
        if not isinstance(panos_u8, torch.Tensor) or panos_u8.dtype != torch.uint8 or panos_u8.ndim != 4 or panos_u8.shape[3] != 3:
            raise TypeError("SphereSweepDepth: the panoramas must be a device uint8 [F,He,We,3] tensor")
        F = panos_u8.shape[0]
        dev = panos_u8.device
        w2c = self._poses(F) if pano_w2c is None else pano_w2c
        frames = panos_u8.contiguous()
        if self.sweep_size is not None and self.sweep_size != tuple(frames.shape[1:3]):
            frames = ops.resize_linear_u8(frames, *self.sweep_size)
        He, We = frames.shape[1:3]
        st = sphere_setup(w2c, We, self.n_src, self.planes, self.d_near, self.d_far, self.min_baseline)
        self.last_setup = st
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        src, rel = up(st.src_index), up(st.rel_pose_f32)
        if self.aggregate == "sgm":
            grey, inv = ops.mvs_luma(frames), up(st.inv_dist_f32)
            if self.cost == "zncc":
                volume = lambda b, m, out: ops.mvs_sphere_sweep_zncc_volume(grey, rel, src, inv, self.patch_radius, self.var_floor,
                                                                            self.sgm.cost_scale, b, m, out=out)
            else:
                volume = lambda b, m, out: ops.mvs_sphere_sweep_volume(grey, rel, src, inv, self.patch_radius, self.sgm.cost_scale, b, m, out=out)
            dist, conf, _, _ = sgm_sweep(volume, inv, src, F, He, We, self.planes, self.sgm)
        elif self.cost == "zncc":
            dist, conf, _, _ = ops.mvs_sphere_sweep_zncc(ops.mvs_luma(frames), rel, src, up(st.inv_dist_f32), self.patch_radius, self.var_floor)
        else:
            dist, conf, _, _ = ops.mvs_sphere_sweep(ops.mvs_luma(frames), rel, src, up(st.inv_dist_f32), self.patch_radius)
        need = min(self.min_consistent, int((st.src_index >= 0).sum(1).max()))
        if need > 0:
            ops.mvs_sphere_consistency(dist, rel, src, conf, self.rel_tol, need)
        E = _w2c_4x4(w2c)
        pts = ops.pano_unproject(dist, up(np.linalg.inv(E)[:, :3, :4].astype(np.float32)))
        return {"world_points_from_depth": pts, "depth_conf": conf, "depth": dist[..., None],
                "images": frames.permute(0, 3, 1, 2).float() / 255, "extrinsic": up(E[:, :3, :4].astype(np.float32))}


# ------------------------------------------------------------------ command line
def _load_frames(folder, n, device):
    from .frames import list_images, read_frames
    names = list_images(folder, (".png", ".jpg"))
    if not names:
        raise SystemExit(f"no .png / .jpg frames under {folder}")
    return read_frames([os.path.join(folder, f) for f in (names[:n] if n else names)], device)


def _cloud_main(args):
    from . import reprojection as RP
    from .dataset import load_camera_poses
    from .memory import SceneMemory
    poses = args.poses
    cam = load_camera_poses(os.path.dirname(os.path.abspath(poses)) if os.path.isfile(poses) else poses)
    n = 25 + 24 * args.segment
    frames = _load_frames(args.frames, n, "cuda")
    n = min(n, len(frames), len(cam))
    frames = frames[:n]
    sgm = dict(aggregate=args.aggregate, sgm_p1=args.sgm_p1, sgm_p2=args.sgm_p2, sgm_paths=args.sgm_paths, cost=args.cost)
    if args.stage == "sphere":
        stage = SphereSweepDepth(cam, n_src=args.sources, planes=args.planes, patch_radius=args.patch_radius, sweep_size=args.sweep_size, **sgm)
        preds = stage(frames, pano_w2c=pano_poses(cam, n, args.segment))
    else:
        yaws = RP.calculate_target_yaws(cam, n, args.segment)
        views = RP.Equi2Pers(height=args.view_height, width=args.view_width, fov_x=90.0).batch(
            frames, [{"pitch": 0, "roll": 0, "yaw": float(y)} for y in yaws])
        stage = PlaneSweepDepth(cam, n_src=args.sources, planes=args.planes, patch_radius=args.patch_radius, **sgm)
        preds = stage(views, view_w2c=view_poses(cam, n, args.segment))
    mem = SceneMemory.from_predictions(preds, conf_thres=args.conf_thres, show_cam=args.show_cam, prediction_mode="depth_unproject")
    n_in = len(mem)
    if args.voxel_size is not None:
        mem = mem.voxel_downsample(args.voxel_size)
    if args.output.lower().endswith(".ply"):
        mem.to_ply(args.output)
    elif args.output.lower().endswith(".glb"):
        mem.to_glb(args.output)
    else:
        raise SystemExit(f"--output must end in .glb or .ply (got {args.output})")
    print(json.dumps({"output": args.output, "views": int(n), "points_in": n_in, "points_out": len(mem), "scene_scale": mem.scene_scale,
                      "planes": args.planes, "sources": args.sources, "stage": args.stage, "aggregate": args.aggregate, "sgm_p1": args.sgm_p1,
                      "sgm_p2": args.sgm_p2, "sgm_paths": args.sgm_paths, "cost": args.cost}))


def build_parser():
    p = argparse.ArgumentParser(prog="python -m evoworld_amd.mvs", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="command", required=True)
    c = sub.add_parser("cloud", help="panorama frames + poses -> plane-sweep depth on perspective views, or sphere-sweep depth on the panoramas -> filtered cloud (.ply | .glb)")
    c.add_argument("--frames", required=True, help="folder of panorama frames (NNN.png, sorted by name), e.g. an episode's predictions/")
    c.add_argument("--poses", required=True, help="camera_poses.txt (or the folder that holds it)")
    c.add_argument("--segment", type=int, default=0, help="segment K: the first 25 + 24 K frames, looking at the segment's target pose")
    c.add_argument("--output", required=True, help="scene.ply or scene.glb")
    c.add_argument("--planes", type=int, default=64)
    c.add_argument("--sources", type=int, default=4)
    c.add_argument("--patch_radius", type=int, default=2)
    c.add_argument("--conf_thres", type=float, default=50.0, help="confidence percentile below which points are dropped")
    c.add_argument("--voxel_size", type=float, default=None, help="voxel-grid downsample on the device before the export")
    c.add_argument("--show_cam", action="store_true", help="add one pyramid marker per camera (GLB)")
    c.add_argument("--view_height", type=int, default=384)
    c.add_argument("--view_width", type=int, default=512)
    c.add_argument("--stage", choices=("plane", "sphere"), default="plane",
                   help="plane: plane sweep on the 90-degree views (DESIGN.md 4.8); sphere: sphere sweep on the panoramas themselves (4.9)")
    c.add_argument("--sweep_size", type=int, nargs=2, metavar=("H", "W"), default=None,
                   help="--stage sphere: resize the panoramas to H x W on the device before the sweep (default: native size)")
    c.add_argument("--aggregate", choices=AGGREGATES, default="box",
                   help="box: the winner of the box-filtered cost (default); sgm: after semi-global aggregation of the cost volume (DESIGN.md 4.10)")
    c.add_argument("--sgm_p1", type=float, default=1.0,
                   help="--aggregate sgm: the penalty of a one-step change of hypothesis, in the cost's units: grey levels (--cost sad), percent of 1 - ZNCC (--cost zncc)")
    c.add_argument("--sgm_p2", type=float, default=8.0, help="--aggregate sgm: the penalty of a larger jump, in the same units; with --cost zncc a larger one, 32, recovered more of a weak, noisy, flickering scene than 8 (DESIGN.md 4.11)")
    c.add_argument("--sgm_paths", type=int, choices=(4, 8), default=4, help="--aggregate sgm: path directions")
    c.add_argument("--cost", choices=COSTS, default="sad",
                   help="sad: the mean absolute difference of grey levels (default); zncc: 100 (1 - ZNCC) over the window, for frames whose exposure or tone drifts (DESIGN.md 4.11)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    _cloud_main(args)


if __name__ == "__main__":
    sys.exit(main())
