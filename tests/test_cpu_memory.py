"""-m 'not gpu': the host side of the 3D-memory export (evoworld_amd/memory.py): the hand-written glTF 2.0 binary writer and its reader,
the PLY writer / reader (binary and the reference's text layout, utils/plucker_embedding.py:334-358), the camera markers' geometry
(reproject_vggt_open3d_utils.py:364-455: apex at the camera centre, base cam_height along the viewing axis, gist_rainbow colours), the
numpy oracle of the voxel downsample on its own stated input, and the header's declarations (ABI 19)."""
import json
import struct

import numpy as np
import pytest

import pointcloud_ref as PR


def _cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)).astype(np.float32), rng.integers(0, 256, (n, 4), dtype=np.uint8)


def _extrinsics():
    """two hand-made world->camera matrices [2,3,4]: a yaw of 30 degrees at (1, 2, 3) and a pitch of -20 degrees at (-2, 0.5, 4)"""
    def rt(R, c):
        return np.concatenate([R, (-R @ np.asarray(c, float))[:, None]], axis=1)
    a, b = np.radians(30), np.radians(-20)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return np.stack([rt(Ry, (1, 2, 3)), rt(Rx, (-2, 0.5, 4))])


@pytest.mark.parametrize("n,show_cam", [(1, False), (5, True), (1000, True)])
def test_glb_round_trip(tmp_path, n, show_cam):
    from evoworld_amd import memory as M
    xyz, rgbx = _cloud(n)
    E = _extrinsics()
    path = M.write_glb(str(tmp_path / "s.glb"), xyz, rgbx, E, scene_scale=2.0, show_cam=show_cam)
    blob = open(path, "rb").read()
    magic, version, total = struct.unpack_from("<III", blob, 0)
    assert magic == 0x46546C67 and version == 2 and total == len(blob)
    jlen, jtype = struct.unpack_from("<II", blob, 12)
    assert jtype == 0x4E4F534A and jlen % 4 == 0
    jtext = blob[20:20 + jlen]
    doc = json.loads(jtext.decode())
    assert jtext.rstrip(b" ") == json.dumps(doc, separators=(",", ":")).encode()       # padded with spaces only
    blen, btype = struct.unpack_from("<II", blob, 20 + jlen)
    assert btype == 0x004E4942 and blen % 4 == 0 and 28 + jlen + blen == len(blob)
    assert doc["asset"]["version"] == "2.0" and doc["buffers"] == [{"byteLength": blen}]
    views = doc["bufferViews"]
    assert all(v["byteOffset"] % 4 == 0 for v in views)
    assert sum(v["byteLength"] + (-v["byteLength"] % 4) for v in views) == blen
    for v, nxt in zip(views, views[1:]):
        assert nxt["byteOffset"] == v["byteOffset"] + v["byteLength"] + (-v["byteLength"] % 4)
    prim = doc["meshes"][0]["primitives"][0]
    assert prim["mode"] == 0 and "indices" not in prim
    pos, col = doc["accessors"][prim["attributes"]["POSITION"]], doc["accessors"][prim["attributes"]["COLOR_0"]]
    assert (pos["componentType"], pos["type"], pos["count"]) == (5126, "VEC3", n)
    assert (col["componentType"], col["type"], col["count"], col["normalized"]) == (5121, "VEC4", n, True)
    assert np.array_equal(np.array(pos["min"], np.float32), xyz.min(0)) and np.array_equal(np.array(pos["max"], np.float32), xyz.max(0))
    assert len(doc["meshes"]) == (2 if show_cam else 1) and len(doc["nodes"]) == len(doc["meshes"])
    got = M.read_glb(path)
    assert got["points"].dtype == np.float32 and got["points"].tobytes() == xyz.tobytes()
    assert np.array_equal(got["colors"][:, :3], rgbx[:, :3]) and (got["colors"][:, 3] == 255).all()
    if show_cam:
        p1 = doc["meshes"][1]["primitives"][0]
        assert p1["mode"] == 4
        idx = doc["accessors"][p1["indices"]]
        assert (idx["componentType"], idx["type"], idx["count"]) == (5125, "SCALAR", 2 * M.MARKER_TRIS * 3)
        cv, cf, cc = M.camera_markers(E, 2.0)
        assert np.array_equal(got["camera_vertices"], cv) and np.array_equal(got["camera_faces"], cf) and np.array_equal(got["camera_colors"], cc)
        cpos = doc["accessors"][p1["attributes"]["POSITION"]]
        assert cpos["count"] == 2 * M.MARKER_VERTS and np.array_equal(np.array(cpos["min"], np.float32), cv.min(0))
        assert cf.max() < len(cv)
    assert "matrix" not in doc["nodes"][0] and "matrix" not in got


def test_glb_bounds_skip_non_finite_and_alignment(tmp_path):
    from evoworld_amd import memory as M
    xyz, rgbx = _cloud(9, seed=3)
    xyz[2, 1], xyz[5, 0] = np.nan, np.inf
    E = _extrinsics()
    got = M.read_glb(M.write_glb(str(tmp_path / "a.glb"), xyz, rgbx[:, :3], E, 1.0, show_cam=False, opengl_align=True))
    keep = np.isfinite(xyz).all(1)
    acc = got["json"]["accessors"][0]
    assert np.array_equal(np.array(acc["min"], np.float32), xyz[keep].min(0)) and np.array_equal(np.array(acc["max"], np.float32), xyz[keep].max(0))
    assert got["points"].tobytes() == xyz.tobytes()                                     # the points are not touched
    E0 = np.eye(4)
    E0[:3] = E[0]
    want = np.linalg.inv(E0) @ np.diag([1.0, -1.0, -1.0, 1.0])
    assert np.array_equal(got["matrix"], want)
    assert got["json"]["nodes"][0]["matrix"] == [float(x) for x in want.T.reshape(-1)]  # column-major
    with pytest.raises(ValueError):
        M.write_glb(str(tmp_path / "e.glb"), xyz[:0], rgbx[:0])
    with pytest.raises(ValueError):
        M.write_glb(str(tmp_path / "e.glb"), xyz, rgbx, None, opengl_align=True)


def test_ply_round_trips(tmp_path):
    from evoworld_amd import memory as M
    xyz, rgbx = _cloud(257, seed=5)
    pb = M.write_ply(str(tmp_path / "b.ply"), xyz, rgbx)
    blob = open(pb, "rb").read()
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 257\nproperty float x\nproperty float y\nproperty float z\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert blob.startswith(head) and len(blob) == len(head) + 257 * 15
    p, c = M.read_ply(pb)
    assert p.tobytes() == xyz.tobytes() and np.array_equal(c, rgbx[:, :3])
    pa = M.write_ply(str(tmp_path / "a.ply"), xyz, rgbx[:, :3], ascii=True)
    p, c = M.read_ply(pa)
    assert p.tobytes() == xyz.tobytes() and np.array_equal(c, rgbx[:, :3])


def test_ply_ascii_is_the_reference_layout(tmp_path):
    """save_point_cloud_to_ply on the (N, 6) float64 array [x, y, z, R, G, B] the reference builds, written out by hand for 3 points"""
    from evoworld_amd import memory as M
    xyz = np.array([[0.5, -1.25, 3.0], [0.1, 2.0, -0.75], [1e-3, 100.0, 0.0]], dtype=np.float32)
    rgb = np.array([[255, 0, 7], [12, 128, 200], [1, 2, 3]], dtype=np.uint8)
    text = open(M.write_ply(str(tmp_path / "t.ply"), xyz, rgb, ascii=True)).read()
    want = ("ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
            "0.5 -1.25 3.0 255 0 7\n"
            "0.10000000149011612 2.0 -0.75 12 128 200\n"
            "0.0010000000474974513 100.0 0.0 1 2 3\n")
    assert text == want
    pc = np.concatenate([xyz.astype(np.float64), rgb.astype(np.float64)], axis=1)       # the reference's loop, restated
    lines = "".join(f"{x} {y} {z} {int(r)} {int(g)} {int(b)}\n" for x, y, z, r, g, b in pc)
    assert text.endswith("end_header\n" + lines)


def test_camera_markers():
    import matplotlib
    from evoworld_amd import memory as M
    E = _extrinsics()
    scale = 3.0
    v, f, c = M.camera_markers(E, scale)
    S, h, w = 2, 0.1 * scale, 0.05 * scale
    assert v.shape == (S * M.MARKER_VERTS, 3) and v.dtype == np.float32 and f.shape == (S * M.MARKER_TRIS, 3) and f.dtype == np.uint32
    assert c.shape == (S * M.MARKER_VERTS, 4) and c.dtype == np.uint8
    cmap = matplotlib.colormaps["gist_rainbow"]
    for i in range(S):
        E4 = np.eye(4)
        E4[:3] = E[i]
        c2w = np.linalg.inv(E4)
        vi = v[i * M.MARKER_VERTS:(i + 1) * M.MARKER_VERTS].astype(np.float64)
        assert np.abs(vi[4] - c2w[:3, 3]).max() < 1e-6                                  # apex at the camera centre
        base = (c2w @ np.array([0, 0, h, 1.0]))[:3]                                     # cam_height along the camera's +z
        assert np.abs(vi[:4].mean(0) - base).max() < 1e-6
        assert np.abs(np.linalg.norm(vi[:4] - base, axis=1) - w).max() < 1e-6           # corners on the circle of radius cam_width
        assert np.abs((vi[:4] - base) @ c2w[:3, 2]).max() < 1e-6                        # the base is perpendicular to the viewing axis
        assert np.abs(vi[9] - c2w[:3, 3]).max() < 0.06 * h and np.abs(vi[14] - c2w[:3, 3]).max() < 1e-6
        want = [int(255 * x) for x in cmap(i / S)[:3]] + [255]
        assert (c[i * M.MARKER_VERTS:(i + 1) * M.MARKER_VERTS] == np.array(want, np.uint8)).all()
        fi = f[i * M.MARKER_TRIS:(i + 1) * M.MARKER_TRIS]
        assert fi.min() >= i * M.MARKER_VERTS and fi.max() < (i + 1) * M.MARKER_VERTS
        half = fi[:M.MARKER_TRIS // 2]
        assert np.array_equal(fi[M.MARKER_TRIS // 2:], half[:, ::-1])                   # every triangle in both windings
    assert np.array_equal(M.camera_colors(2), c.reshape(S, M.MARKER_VERTS, 4)[:, 0, :3])
    E44 = np.zeros((2, 4, 4))
    E44[:, :3], E44[:, 3, 3] = E, 1
    assert np.array_equal(M.camera_markers(E44, scale)[0], v)                           # [S,4,4] extrinsics too


def test_oracle_on_the_main_case():
    """what the numpy oracle gives on the main GPU case: the figures the case was chosen for"""
    xyz, rgb = PR.main_case()
    r = PR.voxel_downsample_ref(xyz, rgb, 2.0)
    idx, _ = PR.voxel_indices_ref(xyz, 2.0)
    q = (xyz - (xyz.min(0) - np.float32(1.0))) / np.float32(2.0)
    assert len(r["keys"]) == 715 and int((r["count"] == 1).sum()) == 48 and r["run_max"] == 19 and r["ties"] == 251
    assert int((q == np.floor(q)).sum()) == 95                                          # coordinates exactly on a voxel face
    assert (np.diff(r["keys"]) > 0).all() and r["count"].sum() == 4097 and (r["rgba"][:, 3] == 255).all()
    assert np.array_equal(PR.half_even_div(np.array([5, 7, 9, 2, 0]), np.array([2, 2, 2, 4, 3])), [2, 4, 4, 0, 0])
    lo, hi, nf = PR.points_bounds_ref(np.array([[np.nan, 0, 0], [1, 2, 3], [-1, np.inf, 0], [0, 5, -2]], np.float32))
    assert nf == 2 and lo.tolist() == [0, 2, -2] and hi.tolist() == [1, 5, 3]
    with pytest.raises(ValueError):
        PR.voxel_downsample_ref(np.array([[0, 0, 0], [2 ** 21, 0, 0]], np.float32), np.zeros((2, 3), np.uint8), 1.0)
    assert len(PR.voxel_downsample_ref(np.array([[0, 0, 0], [2 ** 21 - 1, 0, 0]], np.float32), np.zeros((2, 3), np.uint8), 1.0)["keys"]) == 2


def test_header_declares_the_pointcloud_entry_points():
    from evoworld_amd import _lib
    H = _lib.HEADER
    assert H.constants["EW_ABI_VERSION"] == _lib.ABI_VERSION >= 19
    assert H.functions["ew_points_bounds_workspace_bytes"] == ("size_t", ["size_t"])
    assert H.functions["ew_voxel_reduce_workspace_bytes"] == ("size_t", ["size_t"])
    assert H.functions["ew_points_bounds"] == ("ew_status", ["const float*", "size_t", "void*", "float*", "unsigned long long*", "void*"])
    assert H.functions["ew_voxel_keys"] == ("ew_status", ["const float*", "size_t", "const float*", "float", "long long*", "int*", "void*"])
    ret, params = H.functions["ew_voxel_reduce"]
    assert ret == "ew_status" and params == ["const long long*", "const long long*", "size_t", "const float*", "const uint8_t*", "float*",
                                              "uint8_t*", "int*", "void*", "unsigned long long*", "void*"]


def test_entry_points_take_the_export_flags():
    import inspect
    import unified_loop_consistency as cli
    from evoworld_amd import memory as M
    from evoworld_amd import reprojection as RP
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    a = cli.parse_arguments(["--unet_path", "x"])
    assert a.export_glb is False and a.memory_voxel_size is None
    a = cli.parse_arguments(["--unet_path", "x", "--export_glb", "--memory_voxel_size", "0.05"])
    assert a.export_glb is True and a.memory_voxel_size == 0.05
    sig = inspect.signature(UnifiedLoopConsistencyPipeline.process_episode).parameters
    assert sig["export_memory"].default is False and sig["memory_voxel_size"].default is None
    assert inspect.signature(RP.predictions_to_target_view).parameters["voxel_size"].default is None
    assert RP.predictions_to_glb is M.predictions_to_glb
    want = ["predictions", "conf_thres", "filter_by_frames", "mask_black_bg", "mask_white_bg", "show_cam", "mask_sky", "target_dir",
            "image_subdir", "prediction_mode", "only_render_last_24_frame"]
    p = inspect.signature(M.predictions_to_glb).parameters
    assert list(p) == want and p["conf_thres"].default == 50.0 and p["prediction_mode"].default == "Predicted Pointmap"
    with pytest.raises(ValueError):
        M.predictions_to_glb([1, 2, 3])
