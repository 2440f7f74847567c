"""-m gpu: the device voxel-grid downsample (csrc/pointcloud.hip: ew_points_bounds, ew_voxel_keys, ew_voxel_reduce through
ops.points_bounds / ops.voxel_downsample) against the numpy oracle tests/pointcloud_ref.py, and the 3D-memory export built on it
(evoworld_amd/memory.py, predictions_to_target_view(voxel_size=), process_episode(export_memory=)).
Dyadic inputs (integers / 64) make every fp64 sum exact, so positions are compared bit for bit; for general float32 positions the two
fp64 association orders may round differently and the bound is 1 float32 ulp of the expected value.  Colours (integer arithmetic) and
counts are exact everywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pointcloud_ref as PR
from test_gpu_inference import tiny  # noqa: F401  (the tiny U-Net / pipeline fixture of the episode tests)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _down(xyz, rgb, voxel):
    from evoworld_amd import ops
    v, c, k = ops.voxel_downsample(torch.from_numpy(xyz).to(DEV), torch.from_numpy(rgb).to(DEV), voxel)
    assert v.dtype == torch.float32 and c.dtype == torch.uint8 and k.dtype == torch.int32
    assert v.shape == (len(k), 3) and c.shape == (len(k), 4)
    return v.cpu().numpy(), c.cpu().numpy(), k.cpu().numpy()


def _assert_exact(got, want):
    v, c, k = got
    assert len(k) == len(want["keys"])
    assert np.array_equal(k, want["count"])
    assert v.tobytes() == want["xyz"].tobytes()
    assert np.array_equal(c, want["rgba"]) and (c[:, 3] == 255).all()


def _keys(xyz, voxel):
    """ew_voxel_keys on its own -> (keys int64 [n], overflow flag), origin from the oracle's bounds"""
    from evoworld_amd import ops
    lo, _, _ = PR.points_bounds_ref(xyz)
    origin = torch.from_numpy((lo - np.float32(0.5) * np.float32(voxel)).astype(np.float32)).to(DEV)
    d = torch.from_numpy(xyz).to(DEV)
    keys = torch.empty(len(xyz), dtype=torch.int64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops._call("ew_voxel_keys", ops._ptr(d), len(xyz), ops._ptr(origin), float(voxel), ops._ptr(keys), ops._ptr(flag))
    return keys.cpu().numpy(), int(flag.item())


def test_main_downsample_case():
    xyz, rgb = PR.main_case(4097)
    want = PR.voxel_downsample_ref(xyz, rgb, 2.0)
    assert len(want["keys"]) == 715 and want["run_max"] == 19 and want["ties"] == 251        # what the case was chosen for
    keys, flag = _keys(xyz, 2.0)
    assert flag == 0 and np.array_equal(keys, PR.voxel_keys_ref(xyz, 2.0))
    got = _down(xyz, rgb, 2.0)
    _assert_exact(got, want)
    assert np.array_equal(np.unique(keys), want["keys"])                                     # one output per key, ascending
    rgbx = np.concatenate([rgb, np.full((len(rgb), 1), 77, np.uint8)], axis=1)              # the X byte is ignored
    _assert_exact(_down(xyz, rgbx, 2.0), want)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513])
def test_edge_sizes(n):
    xyz, rgb = PR.main_case(n)
    got = _down(xyz, rgb, 2.0)
    _assert_exact(got, PR.voxel_downsample_ref(xyz, rgb, 2.0))
    if n == 0:
        assert got[0].shape == (0, 3) and got[1].shape == (0, 4) and got[2].shape == (0,)


@pytest.mark.parametrize("n,voxel", [(5000, 0.37), (5000, 3.0), (300, 0.01)])
def test_non_dyadic_positions(n, voxel):
    rng = np.random.default_rng(7)
    xyz = rng.standard_normal((n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    want = PR.voxel_downsample_ref(xyz, rgb, voxel)
    v, c, k = _down(xyz, rgb, voxel)
    assert np.array_equal(k, want["count"]) and np.array_equal(c, want["rgba"])
    err = np.abs(v.astype(np.float64) - want["xyz"].astype(np.float64))
    ulp = np.spacing(np.abs(want["xyz"])).astype(np.float64)
    print(f"non-dyadic n={n} voxel={voxel}: {len(k)} voxels, max error {float((err / ulp).max()):.3f} ulp")
    assert (err <= ulp).all()


def test_one_voxel_holds_everything():
    """the long run: 2^20 points in one voxel (4096 chunk pieces folded by the carry stage), mean exact"""
    n = 1 << 20
    xyz, rgb = PR.main_case(n)
    v, c, k = _down(xyz, rgb, 32.0)                                                          # extent < 16 < voxel
    assert k.tolist() == [n]
    want_xyz = (xyz.astype(np.float64).sum(axis=0) / n).astype(np.float32)                   # exact sums of multiples of 1/64
    assert v.tobytes() == want_xyz[None].tobytes()
    s = rgb.astype(np.int64).sum(axis=0)
    assert c[0].tolist() == PR.half_even_div(s, np.int64(n)).tolist() + [255]


def test_non_finite_points():
    from evoworld_amd import ops
    xyz, rgb = PR.main_case(4097)
    rng = np.random.default_rng(11)
    bad = rng.choice(4097, 300, replace=False)
    xyz[bad[:100], rng.integers(0, 3, 100)] = np.nan
    xyz[bad[100:200], rng.integers(0, 3, 100)] = np.inf
    xyz[bad[200:], rng.integers(0, 3, 100)] = -np.inf
    lo, hi, nf = ops.points_bounds(torch.from_numpy(xyz).to(DEV))
    wlo, whi, wnf = PR.points_bounds_ref(xyz)
    assert nf == wnf == 4097 - 300 and np.array_equal(lo, wlo) and np.array_equal(hi, whi)
    keys, flag = _keys(xyz, 2.0)
    assert flag == 0 and np.array_equal(keys, PR.voxel_keys_ref(xyz, 2.0)) and (keys[bad] == 2 ** 63 - 1).all()
    want = PR.voxel_downsample_ref(xyz, rgb, 2.0)
    assert want["count"].sum() == 4097 - 300
    _assert_exact(_down(xyz, rgb, 2.0), want)
    only = np.full((130, 3), np.nan, np.float32)
    only[::2, 1] = np.inf
    lo, hi, nf = ops.points_bounds(torch.from_numpy(only).to(DEV))
    assert nf == 0 and np.isposinf(lo).all() and np.isneginf(hi).all()
    v, c, k = _down(only, rgb[:130], 2.0)
    assert v.shape == (0, 3) and c.shape == (0, 4) and k.shape == (0,)
    lo, hi, nf = ops.points_bounds(torch.empty(0, 3, device=DEV))
    assert nf == 0 and np.isposinf(lo).all() and np.isneginf(hi).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_grid_limit_of_21_bits(axis):
    rgb = np.array([[10, 20, 30], [50, 60, 70]], np.uint8)
    xyz = np.zeros((2, 3), np.float32)
    xyz[1, axis] = 2 ** 21 - 1                                  # (p - origin) / voxel = 2^21 - 0.5: the last cell
    v, c, k = _down(xyz, rgb, 1.0)
    assert k.tolist() == [1, 1] and v.tobytes() == xyz.tobytes() and np.array_equal(c[:, :3], rgb)
    assert _keys(xyz, 1.0)[0][1] == (2 ** 21 - 1) << (42 - 21 * axis)
    xyz[1, axis] = 2 ** 21                                      # one step further
    assert _keys(xyz, 1.0)[1] == 1
    with pytest.raises(ValueError) as e:
        _down(xyz, rgb, 1.0)
    assert "extent" in str(e.value) and f"{2 ** 21:g}" in str(e.value) and "2^21" in str(e.value)
    v, c, k = _down(xyz, rgb, 1.5)                              # the size the message admits works
    assert k.tolist() == [1, 1]


def test_voxel_size_is_validated():
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, "x", None):
        with pytest.raises(ValueError):
            _down(*PR.main_case(5), bad)


@pytest.mark.parametrize("n", [1, 65, 100003])
def test_points_bounds(n):
    from evoworld_amd import ops
    rng = np.random.default_rng(n)
    xyz = (rng.standard_normal((n, 3)) * [1.0, 50.0, 1e-3]).astype(np.float32)
    if n > 1000:
        xyz[rng.choice(n, 50, replace=False), rng.integers(0, 3, 50)] = [np.nan, np.inf] * 25
    lo, hi, nf = ops.points_bounds(torch.from_numpy(xyz).to(DEV))
    wlo, whi, wnf = PR.points_bounds_ref(xyz)
    assert nf == wnf and np.array_equal(lo, wlo) and np.array_equal(hi, whi) and lo.dtype == np.float32


def test_determinism():
    from evoworld_amd import ops
    rng = np.random.default_rng(5)
    xyz = torch.from_numpy(rng.standard_normal((200_000, 3)).astype(np.float32)).to(DEV)
    rgb = torch.from_numpy(rng.integers(0, 256, (200_000, 4), dtype=np.uint8)).to(DEV)
    a = ops.voxel_downsample(xyz, rgb, 0.25)
    b = ops.voxel_downsample(xyz, rgb, 0.25)
    assert 1000 < len(a[2]) < 200_000 and int(a[2].sum()) == 200_000
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_exact_scene_scale():
    from evoworld_amd import memory as M
    rng = np.random.default_rng(2)
    v = (rng.standard_normal((50_001, 3)) * [1.0, 3.0, 0.2]).astype(np.float32)
    want = np.linalg.norm(np.percentile(v, 95, axis=0) - np.percentile(v, 5, axis=0))
    assert M.exact_scene_scale(torch.from_numpy(v).to(DEV)) == float(want)


# ------------------------------------------------------------------------------------------------ the memory object and the episode path
def _poses(n):
    from evoworld_amd.geometry import xyz_euler_to_four_by_four_matrix_batch
    i = np.arange(n, dtype=np.float64)
    cam = np.stack([0.04 * i * np.sin(i / 9), 0 * i, 0.04 * i * np.cos(i / 9), 0 * i, 95 + 3.6 * i, 0 * i], 1)
    return cam, xyz_euler_to_four_by_four_matrix_batch(torch.tensor(cam, dtype=torch.float32), relative=True).double().numpy()


@pytest.fixture(scope="module")
def preds():
    """synthetic VGGT predictions: S = 3 frames of 24 x 32"""
    S, H, W = 3, 24, 32
    g = torch.Generator().manual_seed(21)
    _, poses = _poses(S)
    return {"depth": (torch.rand(S, H, W, 1, generator=g) * 6 + 1).numpy(), "depth_conf": torch.rand(S, H, W, generator=g).numpy(),
            "images": torch.rand(S, 3, H, W, generator=g).numpy(), "extrinsic": np.linalg.inv(poses)[:, :3, :4].astype(np.float32),
            "intrinsic": np.repeat(np.array([[[W / 2, 0, W / 2], [0, W / 2, H / 2], [0, 0, 1]]], np.float32), S, 0)}


@pytest.fixture(scope="module")
def filtered(preds):
    """the existing filter's output on the lifted predictions (host copies): the reference of everything below"""
    from evoworld_amd import reprojection as RP
    p = dict(preds)
    p["world_points_from_depth"] = RP.depth_to_world_points(p["depth"], p["extrinsic"], p["intrinsic"])
    v, c, _ = RP.PointCloudProcessor().filter_predictions(p, 50.0, prediction_mode="depth_unproject")
    return v.cpu().numpy(), c.cpu().numpy()


VOXEL = 0.4


def test_scene_memory_and_glb(preds, filtered, tmp_path):
    from evoworld_amd import memory as M
    from evoworld_amd import reprojection as RP
    v, c = filtered
    assert len(v) == 3 * 24 * 32 // 2
    mem = RP.predictions_to_glb(preds, prediction_mode="depth_unproject")
    assert isinstance(mem, M.SceneMemory) and mem.vertices.is_cuda and len(mem) == len(v)
    assert mem.vertices.cpu().numpy().tobytes() == v.tobytes() and np.array_equal(mem.colors.cpu().numpy(), c)
    assert mem.scene_scale == float(np.linalg.norm(np.percentile(v, 95, axis=0) - np.percentile(v, 5, axis=0)))
    assert np.array_equal(mem.extrinsic, preds["extrinsic"])
    got = M.read_glb(mem.export(file_obj=str(tmp_path / "full.glb")))
    assert got["points"].tobytes() == v.tobytes() and np.array_equal(got["colors"][:, :3], c) and (got["colors"][:, 3] == 255).all()
    acc = got["json"]["accessors"][0]
    assert np.array_equal(np.array(acc["min"], np.float32), v.min(0)) and np.array_equal(np.array(acc["max"], np.float32), v.max(0))
    cv, cf, cc = M.camera_markers(preds["extrinsic"], mem.scene_scale)
    assert np.array_equal(got["camera_vertices"], cv) and np.array_equal(got["camera_faces"], cf) and np.array_equal(got["camera_colors"], cc)
    assert "camera_vertices" not in M.read_glb(mem.to_glb(str(tmp_path / "nocam.glb"), show_cam=False))
    want = PR.voxel_downsample_ref(v, c, VOXEL)
    small = mem.voxel_downsample(VOXEL)
    assert 1 < len(small) == len(want["keys"]) < len(mem) and small.scene_scale == mem.scene_scale
    got = M.read_glb(small.to_glb(str(tmp_path / "small.glb")))
    assert got["points"].tobytes() == want["xyz"].tobytes() and np.array_equal(got["colors"], want["rgba"])
    p, col = M.read_ply(small.to_ply(str(tmp_path / "small.ply")))
    assert p.tobytes() == got["points"].tobytes() and np.array_equal(col, want["rgba"][:, :3])
    with pytest.raises(NotImplementedError):
        RP.predictions_to_glb(preds, mask_sky=True)
    # the command line writes the same file
    np.savez(tmp_path / "preds.npz", **preds)
    small2 = M.SceneMemory.from_predictions(preds, show_cam=True, prediction_mode="Pointmap Regression").voxel_downsample(VOXEL)
    ref_file = small2.to_glb(str(tmp_path / "api.glb"), opengl_align=True)
    r = subprocess.run([sys.executable, "-m", "evoworld_amd.memory", "export", "--predictions", str(tmp_path / "preds.npz"), "--output",
                        str(tmp_path / "cli.glb"), "--show_cam", "--voxel_size", str(VOXEL), "--opengl_align"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tmp_path / "cli.glb", "rb").read() == open(ref_file, "rb").read()
    assert open(ref_file, "rb").read()[20:].startswith(b'{"asset"') and "matrix" in M.read_glb(ref_file)


def test_target_view_with_voxel_size(preds, filtered):
    from evoworld_amd import reprojection as RP
    from evoworld_amd.inference import _Sized
    v, c = filtered
    _, poses = _poses(60)
    cr = _Sized(RP.CubemapRenderer(face_res=32), (64, 128))
    kw = dict(conf_thres=50.0, prediction_mode="depth_unproject", num_target_view=24, outdir="rendered_0", cubemap_renderer=cr,
              return_device_tensor=True, save_png=False)
    base = RP.predictions_to_target_view(preds, poses, **kw)
    assert base.shape == (24, 64, 128, 3) and base.any()
    assert torch.equal(RP.predictions_to_target_view(preds, poses, voxel_size=None, **kw), base)
    want = PR.voxel_downsample_ref(v, c, VOXEL)
    assert (want["count"] > 1).any()
    target = RP.SceneBuilder().align_extrinsics(poses, preds["extrinsic"], 24, "rendered_0", False)
    got = RP.predictions_to_target_view(preds, poses, voxel_size=VOXEL, **kw)
    # downsample (oracle) -> the existing splat path
    ref = cr.render_cubemaps_to_panoramas(torch.from_numpy(want["xyz"]).to(DEV), torch.from_numpy(want["rgba"][:, :3].copy()).to(DEV),
                                          target, 24, None)
    assert torch.equal(got, ref) and not torch.equal(got, base)


def test_process_episode_exports_the_memory(tiny, tmp_path):  # noqa: F811
    from evoworld_amd import memory as M
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.stages import SyntheticStages
    cfg, pipe = tiny
    H, W, T = 128, 256, 25
    cam, _ = _poses(60)
    st = SyntheticStages(cross_attention_dim=cfg["cross_attention_dim"], camera_params=cam, depth_hw=(48, 64))
    saved = (pipe.vae, pipe.image_encoder, pipe.vae_scale_factor)
    pipe.set_components(vae=st.vae, image_encoder=st.image_encoder)
    seen = []

    def depth_model(pers):
        seen.append(st.depth_model(pers))
        return seen[-1]
    try:
        loop = UnifiedLoopConsistencyPipeline(pipe, depth_model, height=H, width=W, num_frames=T, num_segments=2,
                                              num_inference_steps=1, pano_size=(64, 128), face_res=32)
        start = (torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
        plain = loop.process_episode(start, cam)
        frames = loop.process_episode(start, cam, save_dir=str(tmp_path), export_memory=True, memory_voxel_size=None)
    finally:
        pipe.vae, pipe.image_encoder, pipe.vae_scale_factor = saved
    assert frames.shape == (49, 3, H, W) and torch.equal(frames, plain)
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith(".glb")) == ["glbscene_0.glb"]       # one hand-off in two segments
    got = M.read_glb(str(tmp_path / "glbscene_0.glb"))
    ref = M.SceneMemory.from_predictions(seen[-1], prediction_mode="depth_unproject")
    assert got["points"].tobytes() == ref.vertices.cpu().numpy().tobytes() and len(got["points"]) > 100
    assert np.array_equal(got["colors"][:, :3], ref.colors.cpu().numpy())
    assert len(got["camera_vertices"]) == 25 * M.MARKER_VERTS                                         # the 25 cameras of the hand-off
