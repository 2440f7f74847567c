"""The 3D memory as an object a user can keep: the filtered point cloud of a hand-off, its cameras and its scale, on the device, with
a voxel-grid downsample and GLB / PLY export.

Call surface of the reference's export path: predictions_to_glb -> SceneBuilder.build_scene / _add_cameras_to_scene /
_integrate_camera_into_scene (evoworld/reprojection/reproject_vggt_open3d_utils.py:713-766, 349-455), apply_scene_alignment (:819-845),
the `--export_glb` branch of reproject_vggt_open3d.py:245-265 and save_point_cloud_to_ply (utils/plucker_embedding.py:334-358).  The
reference builds a trimesh.Scene on the host; here the cloud stays in HBM (ops.filter_compact's output, optionally thinned by
ops.voxel_downsample: csrc/pointcloud.hip) and crosses to the host once per array when a file is written.  The glTF 2.0 binary is
written by hand (no trimesh): mesh 0 is the cloud as POINTS, an optional mesh 1 holds one pyramid marker per camera.  The marker's
vertex order is this module's own (trimesh's cone is unpinned); its geometry -- apex at the camera centre, base
cam_height in front of the camera, colour gist_rainbow(i / num_cameras) -- is the reference's.

    python -m evoworld_amd.memory export --predictions preds.npz --output scene.glb [--voxel_size 0.02] [--show_cam] ...
"""
import argparse
import json
import math
import struct
import sys

import numpy as np
import torch

GLB_MAGIC, GLB_VERSION, CHUNK_JSON, CHUNK_BIN = 0x46546C67, 2, 0x4E4F534A, 0x004E4942
GL_FLOAT, GL_UBYTE, GL_UINT, GL_ARRAY_BUFFER, GL_ELEMENT_ARRAY_BUFFER = 5126, 5121, 5125, 34962, 34963
MODE_POINTS, MODE_TRIANGLES = 0, 4
MARKER_VERTS, MARKER_TRIS = 15, 48              # per camera: 3 copies of (4 base corners + apex); 4 sides x 6 triangles x 2 windings
OPENGL = np.diag([1.0, -1.0, -1.0, 1.0])        # _get_opengl_conversion_matrix (:415-420)


def _host(x, dtype=None):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a if dtype is None else np.ascontiguousarray(a, dtype=dtype)


def extrinsics_4x4(extrinsic):
    """[S,3,4] or [S,4,4] world->camera -> float64 [S,4,4] (:367-371)"""
    e = _host(extrinsic).astype(np.float64)
    if e.ndim != 3 or e.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError(f"extrinsic must be [S,3,4] or [S,4,4], got {e.shape}")
    out = np.zeros((len(e), 4, 4))
    out[:, :3, :4] = e[:, :3, :4]
    out[:, 3, 3] = 1
    return out


def camera_colors(num_cameras):
    """uint8 [S,3]: int(255 * x) of gist_rainbow(i / num_cameras) (:376-377).  matplotlib is imported here, on first use."""
    import matplotlib
    cmap = matplotlib.colormaps["gist_rainbow"]
    return np.array([[int(255 * x) for x in cmap(i / num_cameras)[:3]] for i in range(num_cameras)], dtype=np.uint8).reshape(-1, 3)


def camera_markers(extrinsic, scene_scale):
    """One pyramid per camera (:364-455): -> (vertices float32 [S*15,3], triangles uint32 [S*48,3], colours uint8 [S*15,4]).
    Local cone: 4 base corners on a circle of radius cam_width = 0.05 * scene_scale at z = 0, apex at z = cam_height = 0.1 * scene_scale;
    three copies (as it is, scaled 0.95, turned 2 degrees about z) give the edges some thickness, as in the reference; transform
    c2w @ diag(1,-1,-1,1) @ [Rz(45 deg), z -= cam_height]: the apex lands on the camera centre and the base cam_height along the
    camera's viewing axis.  Per camera the vertices are copy-major: copy k holds corners at 5k .. 5k+3 and the apex at 5k+4."""
    E = extrinsics_4x4(extrinsic)
    S = len(E)
    w, h = 0.05 * float(scene_scale), 0.1 * float(scene_scale)
    ang = np.arange(4) * (np.pi / 2)
    cone = np.concatenate([np.stack([w * np.cos(ang), w * np.sin(ang), np.zeros(4)], axis=1), [[0.0, 0.0, h]]])       # [5,3]

    def rot_z(deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        m = np.eye(4)
        m[:2, :2] = [[c, -s], [s, c]]
        return m

    local = np.concatenate([cone, 0.95 * cone, cone @ rot_z(2)[:3, :3].T])                                            # [15,3]
    rot45 = rot_z(45)
    rot45[2, 3] = -h
    tris = []
    for k in range(4):                             # the side (apex, corner k, corner k+1) joined to its two companions (:433-455)
        v1, v2, v3 = 4, k, (k + 1) % 4
        for off in (5, 10):
            tris += [(v1, v2, v2 + off), (v1, v1 + off, v3), (v3 + off, v2, v3)]
    tris += [(c, b, a) for a, b, c in tris]
    tris = np.array(tris, dtype=np.uint32)
    col = camera_colors(S)
    verts = np.zeros((S, MARKER_VERTS, 3))
    for i in range(S):
        T = np.linalg.inv(E[i]) @ OPENGL @ rot45
        verts[i] = local @ T[:3, :3].T + T[:3, 3]
    faces = (tris[None] + (np.arange(S, dtype=np.uint32) * MARKER_VERTS)[:, None, None]).reshape(-1, 3)
    colors = np.full((S, MARKER_VERTS, 4), 255, dtype=np.uint8)
    colors[:, :, :3] = col[:, None]
    return verts.reshape(-1, 3).astype(np.float32), faces.astype(np.uint32), colors.reshape(-1, 4)


def scene_alignment(extrinsic):
    """inv(E0) @ diag(1,-1,-1,1): the node transform of apply_scene_alignment (:837)"""
    return np.linalg.inv(extrinsics_4x4(extrinsic)[0]) @ OPENGL


def _finite_bounds(xyz):
    """per-axis (min, max) over the finite points: ew_points_bounds for a device tensor, numpy for a host array"""
    if isinstance(xyz, torch.Tensor) and xyz.device.type == "cuda":
        from . import ops
        lo, hi, _ = ops.points_bounds(xyz)
        return lo, hi
    p = _host(xyz, np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if len(p) == 0:
        return np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    return p.min(axis=0), p.max(axis=0)


def _rgba_host(colors):
    """[n,3|4] uint8 (host or device; a fourth byte is padding) -> host uint8 [n,4] with alpha 255, one transfer"""
    if isinstance(colors, torch.Tensor):
        c = colors if colors.shape[1] == 4 else torch.cat([colors, colors[:, :1]], dim=1)
        c = c.clone()
        c[:, 3] = 255
        return c.cpu().numpy()
    c = np.asarray(colors, dtype=np.uint8)
    out = np.full((len(c), 4), 255, dtype=np.uint8)
    out[:, :3] = c[:, :3]
    return out


def write_glb(path, vertices, colors, extrinsic=None, scene_scale=1.0, show_cam=True, opengl_align=False):
    """glTF 2.0 binary: 12-byte header, JSON chunk (space padded to 4 bytes), BIN chunk (zero padded).  Mesh 0: POINTS with POSITION
    (float VEC3, min / max over the finite points) and COLOR_0 (normalised unsigned byte VEC4).  With show_cam and extrinsics, mesh 1:
    TRIANGLES of `camera_markers`.  opengl_align stores `scene_alignment` as every node's matrix; the points are not touched.
    vertices [n,3] float32 and colors [n,3|4] uint8 may be host arrays or device tensors (each crosses to the host once)."""
    lo, hi = _finite_bounds(vertices)
    pos = _host(vertices, np.float32).reshape(-1, 3)
    rgba = _rgba_host(colors)
    if len(pos) == 0 or len(pos) != len(rgba):
        raise ValueError(f"write_glb needs a non-empty cloud with one colour per point (got {len(pos)} points, {len(rgba)} colours)")
    blobs, views, accessors = [], [], []

    def add(arr, target, ctype, kind, normalized=False, minmax=None):
        data = np.ascontiguousarray(arr).tobytes()
        offset = sum(len(b) for b in blobs)
        assert offset % 4 == 0
        blobs.append(data + b"\0" * (-len(data) % 4))
        views.append({"buffer": 0, "byteOffset": offset, "byteLength": len(data), "target": target})
        acc = {"bufferView": len(views) - 1, "componentType": ctype, "count": int(arr.size if kind == "SCALAR" else len(arr)), "type": kind}
        if normalized:
            acc["normalized"] = True
        if minmax is not None:
            acc["min"], acc["max"] = [float(x) for x in minmax[0]], [float(x) for x in minmax[1]]
        accessors.append(acc)
        return len(accessors) - 1

    meshes = [{"name": "points", "primitives": [{"mode": MODE_POINTS, "attributes": {
        "POSITION": add(pos, GL_ARRAY_BUFFER, GL_FLOAT, "VEC3", minmax=(lo, hi)),
        "COLOR_0": add(rgba, GL_ARRAY_BUFFER, GL_UBYTE, "VEC4", normalized=True)}}]}]
    if show_cam and extrinsic is not None and len(_host(extrinsic)):
        cv, cf, cc = camera_markers(extrinsic, scene_scale)
        meshes.append({"name": "cameras", "primitives": [{"mode": MODE_TRIANGLES, "attributes": {
            "POSITION": add(cv, GL_ARRAY_BUFFER, GL_FLOAT, "VEC3", minmax=(cv.min(axis=0), cv.max(axis=0))),
            "COLOR_0": add(cc, GL_ARRAY_BUFFER, GL_UBYTE, "VEC4", normalized=True)},
            "indices": add(cf.reshape(-1), GL_ELEMENT_ARRAY_BUFFER, GL_UINT, "SCALAR")}]})
    nodes = [{"mesh": i, "name": m["name"]} for i, m in enumerate(meshes)]
    if opengl_align:
        if extrinsic is None:
            raise ValueError("opengl_align needs the extrinsics (the first camera defines the alignment)")
        mat = [float(x) for x in scene_alignment(extrinsic).T.reshape(-1)]                 # glTF matrices are column-major
        for nd in nodes:
            nd["matrix"] = mat
    binary = b"".join(blobs)
    doc = {"asset": {"version": "2.0", "generator": "evoworld_amd.memory"}, "scene": 0, "scenes": [{"nodes": list(range(len(nodes)))}],
           "nodes": nodes, "meshes": meshes, "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(binary)}]}
    js = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    js += b" " * (-len(js) % 4)
    total = 12 + 8 + len(js) + 8 + len(binary)
    with open(path, "wb") as f:
        f.write(struct.pack("<III", GLB_MAGIC, GLB_VERSION, total))
        f.write(struct.pack("<II", len(js), CHUNK_JSON) + js)
        f.write(struct.pack("<II", len(binary), CHUNK_BIN) + binary)
    return path


_COMPONENT = {GL_FLOAT: np.dtype("<f4"), GL_UBYTE: np.dtype("u1"), GL_UINT: np.dtype("<u4"), 5123: np.dtype("<u2")}
_WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def read_glb(path):
    """-> dict(json, points float32 [n,3], colors uint8 [n,4], and with a camera mesh: camera_vertices float32 [k,3], camera_faces
    uint32 [t,3], camera_colors uint8 [k,4]; matrix float64 [4,4] of node 0 when it has one).  Reads the files `write_glb` writes and
    any glTF 2.0 binary with tightly packed accessors in one BIN chunk."""
    with open(path, "rb") as f:
        blob = f.read()
    magic, version, total = struct.unpack_from("<III", blob, 0)
    if magic != GLB_MAGIC or version != GLB_VERSION or total != len(blob):
        raise ValueError(f"{path}: not a glTF 2.0 binary (magic {magic:#x}, version {version}, length {total} of {len(blob)})")
    jlen, jtype = struct.unpack_from("<II", blob, 12)
    if jtype != CHUNK_JSON:
        raise ValueError(f"{path}: the first chunk is not JSON")
    doc = json.loads(blob[20:20 + jlen].decode("utf-8"))
    blen, btype = struct.unpack_from("<II", blob, 20 + jlen)
    if btype != CHUNK_BIN:
        raise ValueError(f"{path}: the second chunk is not BIN")
    binary = blob[28 + jlen:28 + jlen + blen]

    def accessor(i):
        a = doc["accessors"][i]
        v = doc["bufferViews"][a["bufferView"]]
        dt, w = _COMPONENT[a["componentType"]], _WIDTH[a["type"]]
        off = v.get("byteOffset", 0) + a.get("byteOffset", 0)
        arr = np.frombuffer(binary, dtype=dt, count=a["count"] * w, offset=off)
        return arr.reshape(a["count"], w).copy() if w > 1 else arr.copy()

    out = {"json": doc}
    p0 = doc["meshes"][0]["primitives"][0]
    out["points"], out["colors"] = accessor(p0["attributes"]["POSITION"]), accessor(p0["attributes"]["COLOR_0"])
    if len(doc["meshes"]) > 1:
        p1 = doc["meshes"][1]["primitives"][0]
        out["camera_vertices"], out["camera_colors"] = accessor(p1["attributes"]["POSITION"]), accessor(p1["attributes"]["COLOR_0"])
        out["camera_faces"] = accessor(p1["indices"]).reshape(-1, 3)
    if "matrix" in doc["nodes"][0]:
        out["matrix"] = np.array(doc["nodes"][0]["matrix"], dtype=np.float64).reshape(4, 4).T
    return out


_PLY_PROPS = (("x", "float"), ("y", "float"), ("z", "float"), ("red", "uchar"), ("green", "uchar"), ("blue", "uchar"))
_PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_ply(path, vertices, colors, ascii=False):
    """PLY with the reference's properties (x y z float, red green blue uchar; utils/plucker_embedding.py:334-358): binary
    little-endian, or with ascii=True the reference's text: one `x y z r g b` line per point, the coordinates printed as Python prints
    the float64 they widen to, the colours as integers."""
    pos = _host(vertices, np.float32).reshape(-1, 3)
    rgb = _host(colors, np.uint8)[:, :3]
    head = ["ply", f"format {'ascii' if ascii else 'binary_little_endian'} 1.0", f"element vertex {len(pos)}"]
    head += [f"property {t} {n}" for n, t in _PLY_PROPS] + ["end_header"]
    header = "".join(line + "\n" for line in head)
    if ascii:
        with open(path, "w") as f:
            f.write(header)
            for (x, y, z), (r, g, b) in zip(pos.astype(np.float64).tolist(), rgb.tolist()):
                f.write(f"{x} {y} {z} {int(r)} {int(g)} {int(b)}\n")
        return path
    rec = np.empty(len(pos), dtype=_PLY_DTYPE)
    rec["x"], rec["y"], rec["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
    return path


def read_ply(path):
    """-> (points float32 [n,3], colors uint8 [n,3]) of a PLY with exactly the six properties `write_ply` writes, ascii or binary
    little-endian"""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    if lines[0] != "ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt = lines[1].split()[1]
    n = int(next(ln for ln in lines if ln.startswith("element vertex")).split()[2])
    props = tuple((ln.split()[2], ln.split()[1]) for ln in lines if ln.startswith("property"))
    if props != _PLY_PROPS:
        raise ValueError(f"{path}: properties {props} are not {_PLY_PROPS}")
    if fmt == "ascii":
        rows = np.array([ln.split() for ln in blob[end:].decode("ascii").split("\n") if ln.strip()], dtype=object).reshape(n, 6)
        return rows[:, :3].astype(np.float64).astype(np.float32), rows[:, 3:].astype(np.int64).astype(np.uint8)
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: format {fmt} is not supported")
    rec = np.frombuffer(blob, dtype=_PLY_DTYPE, count=n, offset=end)
    return (np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32),
            np.stack([rec["red"], rec["green"], rec["blue"]], axis=1).astype(np.uint8))


def exact_scene_scale(vertices):
    """|| P95 - P5 || over the three axes with numpy's linear percentile, exactly (_calculate_scene_scale, :330-337): each contiguous
    axis column goes through the radix select (ew_select_kth_f32) and numpy's float32 interpolation (reprojection.percentile_threshold)."""
    from .reprojection import percentile_threshold
    cols = vertices.t().contiguous()                                      # [3,n]: one contiguous column per axis
    lo = np.array([percentile_threshold(cols[a], 5) for a in range(3)], dtype=np.float32)
    hi = np.array([percentile_threshold(cols[a], 95) for a in range(3)], dtype=np.float32)
    return float(np.linalg.norm(hi - lo))


class SceneMemory:
    """The memory of one hand-off: `vertices` fp32 [n,3] and `rgbx` uint8 [n,4] (RGB + one padding byte; alpha 255 after a downsample)
    on the device, `extrinsic` [S,3,4] or [S,4,4] world->camera (host), `scene_scale` (the exact 5 / 95 percentile diagonal)."""

    def __init__(self, vertices, rgbx, extrinsic=None, scene_scale=1.0, show_cam=True):
        if rgbx.shape[1] == 3:                                            # widen packed RGB to words
            pad = torch.zeros_like(rgbx[:, :1]) if isinstance(rgbx, torch.Tensor) else np.zeros_like(rgbx[:, :1])
            rgbx = torch.cat([rgbx, pad], dim=1) if isinstance(rgbx, torch.Tensor) else np.concatenate([rgbx, pad], axis=1)
        self.vertices, self.rgbx, self.extrinsic, self.scene_scale, self.show_cam = vertices, rgbx, extrinsic, float(scene_scale), show_cam

    def __len__(self):
        return int(self.vertices.shape[0])

    @property
    def colors(self):
        return self.rgbx[:, :3]

    @classmethod
    def from_predictions(cls, predictions, conf_thres=50.0, filter_by_frames="all", mask_black_bg=False, mask_white_bg=False,
                         show_cam=True, mask_sky=False, target_dir=None, image_subdir=None, prediction_mode="Predicted Pointmap",
                         only_render_last_24_frame=False, point_processor=None):
        """The arguments of the reference's predictions_to_glb (:713-725).  The cloud is PointCloudProcessor.filter_predictions'
        output as it is (mask_sky=True raises there); with only `depth` in the predictions the depth lift runs first, as in
        predictions_to_target_view."""
        from . import reprojection as RP
        if not isinstance(predictions, dict):
            raise ValueError("predictions must be a dictionary")
        pp = point_processor or RP.PointCloudProcessor()
        if "world_points_from_depth" not in predictions and "world_points" not in predictions:
            predictions = dict(predictions)
            predictions["world_points_from_depth"] = RP.depth_to_world_points(predictions["depth"], predictions["extrinsic"],
                                                                              predictions["intrinsic"], device=pp.device)
        v, c, _ = pp.filter_predictions(predictions, conf_thres, filter_by_frames, mask_black_bg, mask_white_bg, mask_sky, target_dir,
                                        image_subdir, prediction_mode, only_render_last_24_frame)
        return cls.from_cloud(v, c, predictions.get("extrinsic"), show_cam)

    @classmethod
    def from_cloud(cls, vertices, colors, extrinsic=None, show_cam=True):
        """From a filtered cloud that already exists on the device (the one a hand-off renders): nothing is filtered twice."""
        return cls(vertices, colors, None if extrinsic is None else _host(extrinsic), exact_scene_scale(vertices), show_cam)

    def voxel_downsample(self, voxel_size):
        """A new SceneMemory with one averaged point per occupied voxel (ops.voxel_downsample); cameras and scale are kept."""
        from . import ops
        v, rgba, _ = ops.voxel_downsample(self.vertices, self.rgbx, voxel_size)
        return SceneMemory(v, rgba, self.extrinsic, self.scene_scale, self.show_cam)

    def to_glb(self, path, show_cam=None, opengl_align=False):
        return write_glb(path, self.vertices, self.rgbx, self.extrinsic, self.scene_scale,
                         self.show_cam if show_cam is None else show_cam, opengl_align)

    def export(self, file_obj, **kw):
        """trimesh.Scene.export's spelling, so that the reference's `glbscene.export(file_obj=glbfile)` works unchanged"""
        return self.to_glb(file_obj, **kw)

    def to_ply(self, path, ascii=False):
        return write_ply(path, self.vertices, self.rgbx, ascii)

    def render(self, target_extrinsic, num_target_view=24, outdir=None, width=2000, height=1000, cubemap_renderer=None):
        """The memory seen from the target cameras (camera-to-world [V,4,4]): uint8 [V,height,width,3] panoramas on the device"""
        from .reprojection import CubemapRenderer
        cr = cubemap_renderer or CubemapRenderer()
        return cr.render_cubemaps_to_panoramas(self.vertices, self.colors, target_extrinsic, num_target_view, outdir, width, height)


def predictions_to_glb(predictions, conf_thres=50.0, filter_by_frames="all", mask_black_bg=False, mask_white_bg=False, show_cam=True,
                       mask_sky=False, target_dir=None, image_subdir=None, prediction_mode="Predicted Pointmap",
                       only_render_last_24_frame=False):
    """The reference's predictions_to_glb (:713-766): returns the SceneMemory, whose .export(file_obj=path) writes the GLB."""
    return SceneMemory.from_predictions(predictions, conf_thres, filter_by_frames, mask_black_bg, mask_white_bg, show_cam, mask_sky,
                                        target_dir, image_subdir, prediction_mode, only_render_last_24_frame)


def _export_main(args):
    with np.load(args.predictions) as z:
        predictions = {k: z[k] for k in z.files}
    mem = predictions_to_glb(predictions, conf_thres=args.conf_thres, filter_by_frames=args.frame_filter, mask_black_bg=args.mask_black_bg,
                             mask_white_bg=args.mask_white_bg, show_cam=args.show_cam, prediction_mode=args.prediction_mode)
    n_in = len(mem)
    if args.voxel_size is not None:
        mem = mem.voxel_downsample(args.voxel_size)
    if args.output.lower().endswith(".ply"):
        mem.to_ply(args.output)
    elif args.output.lower().endswith(".glb"):
        mem.to_glb(args.output, opengl_align=args.opengl_align)
    else:
        raise SystemExit(f"--output must end in .glb or .ply (got {args.output})")
    print(json.dumps({"output": args.output, "points_in": n_in, "points_out": len(mem), "scene_scale": mem.scene_scale,
                      "voxel_size": args.voxel_size}))


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m evoworld_amd.memory", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="command", required=True)
    e = sub.add_parser("export", help="VGGT predictions (.npz with the keys of the predictions dict) -> scene.glb | scene.ply")
    e.add_argument("--predictions", required=True, help=".npz: images, extrinsic, and world_points(+_conf) or depth(+_conf) + intrinsic")
    e.add_argument("--output", required=True, help="scene.glb or scene.ply")
    e.add_argument("--conf_thres", type=float, default=50.0, help="confidence percentile below which points are dropped")
    e.add_argument("--frame_filter", type=str, default="All")
    e.add_argument("--mask_black_bg", action="store_true")
    e.add_argument("--mask_white_bg", action="store_true")
    e.add_argument("--show_cam", action="store_true", help="add one pyramid marker per camera")
    e.add_argument("--prediction_mode", type=str, default="Pointmap Regression")
    e.add_argument("--voxel_size", type=float, default=None, help="voxel-grid downsample on the device before the export")
    e.add_argument("--opengl_align", action="store_true", help="store inv(E0) @ diag(1,-1,-1,1) as the node matrix")
    args = p.parse_args(argv)
    _export_main(args)


if __name__ == "__main__":
    sys.exit(main())
