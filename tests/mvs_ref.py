"""numpy oracle of the plane-sweep stereo stage (evoworld_amd/csrc/mvs.hip, evoworld_amd/mvs.py; include/evoworld_hip.h states the rules).

  luma_ref            the integer grey conversion
  cost_volume         C(k) per pixel in float64 (the truth) or in float32 in the kernel's written operation order, plus the (pixel, plane)
                      pairs whose window holds an ambiguous tap
  winner_ref / parabola_inverse_depth / confidence_ref     the rules behind depth and confidence, on any cost volume
  consistency_ref     the cross-view check
  BoxScene            the inside of an axis-aligned box with a smooth, non-periodic texture that is a function of the 3D point, ray-cast
                      into perspective views (with true depth) and into equirectangular panoramas
  sweep_case / GPU_CASES    the inputs of tests/test_gpu_mvs.py, shared with the CPU tests that measure the margin on them
"""
import math
from types import SimpleNamespace

import numpy as np

# The largest |float32-order cost - float64 cost| over the inputs of the GPU tests (ambiguous taps left out), in grey levels, measured by
# tests/test_cpu_mvs.py::test_margin_constant_covers_the_measured_float32_error (2.2e-4 when this was written), rounded up.  The GPU tests
# allow COST_TOL = COST_TOL_FACTOR x this; the factor is for library-level differences in the bilinear weights (a division that is not
# correctly rounded moves a sample by an ulp of a coordinate), not for kernel changes.
F32_ORDER_MARGIN = 3.0e-4
COST_TOL_FACTOR = 2.0
COST_TOL = COST_TOL_FACTOR * F32_ORDER_MARGIN
BORDER_EPS = 1e-3          # a sample this close (px) to the source's border may fall on either side
Q2_EPS = 1e-6              # and so may one whose q2 is this close to 0
MAX_AMBIGUOUS_SHARE = 0.005


def luma_ref(rgb):
    rgb = rgb.astype(np.int64)
    return ((77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + 128) >> 8).astype(np.uint8)


def _warp(ref, src, Hm, oob, dt):
    """per-pixel AD of one (reference, source, plane) in dtype dt, in the header's order; also (q2, sx, sy)"""
    H, W = ref.shape
    y, x = np.meshgrid(np.arange(H, dtype=dt), np.arange(W, dtype=dt), indexing="ij")
    h = np.asarray(Hm, dtype=dt).reshape(9)
    q0 = (h[0] * x + h[1] * y) + h[2]
    q1 = (h[3] * x + h[4] * y) + h[5]
    q2 = (h[6] * x + h[7] * y) + h[8]
    with np.errstate(all="ignore"):
        sx, sy = q0 / q2, q1 / q2
        inb = (q2 > 0) & (sx >= 0) & (sx <= dt(W - 1)) & (sy >= 0) & (sy <= dt(H - 1))
    sxc, syc = np.where(inb, sx, dt(0)), np.where(inb, sy, dt(0))
    x0f, y0f = np.floor(sxc), np.floor(syc)
    ax, ay = sxc - x0f, syc - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    s = src.astype(dt)
    one = dt(1)
    top = s[y0, x0] * (one - ax) + s[y0, x1] * ax
    bot = s[y1, x0] * (one - ax) + s[y1, x1] * ax
    ad = np.abs(ref.astype(dt) - (top * (one - ay) + bot * ay))
    out = np.where(inb, ad, dt(oob))
    assert out.dtype == dt
    return out, q2, sx, sy


def _box(a, r, dt):
    """rows of taps left to right, then the row sums top to bottom; taps outside the image add 0"""
    H, W = a.shape
    p = np.zeros((H + 2 * r, W + 2 * r), dt)
    p[r:r + H, r:r + W] = a
    rs = np.zeros((H + 2 * r, W), dt)
    for d in range(2 * r + 1):
        rs = rs + p[:, d:d + W]
    c = np.zeros((H, W), dt)
    for d in range(2 * r + 1):
        c = c + rs[d:d + H]
    assert c.dtype == dt
    return c


def window_taps(H, W, r):
    ys, xs = np.arange(H), np.arange(W)
    cy = np.minimum(ys + r, H - 1) - np.maximum(ys - r, 0) + 1
    cx = np.minimum(xs + r, W - 1) - np.maximum(xs - r, 0) + 1
    return cy[:, None] * cx[None]


def present(src_index, F):
    s = np.asarray(src_index)
    return (s >= 0) & (s < F)


def cost_volume(grey, homographies, src_index, r, oob, dtype=np.float64):
    """grey uint8 [F,H,W]; homographies [F,S,D,3,3] -- the float32 values the device gets; src_index [F,S] -> (C [F,D,H,W] in dtype,
    ambiguous bool [F,D,H,W]).  float64: the truth.  float32: every operation rounded once, in the order the header writes down."""
    dt = np.float32 if dtype == np.float32 else np.float64
    F, H, W = grey.shape
    S, D = homographies.shape[1:3]
    ok = present(src_index, F)
    C = np.zeros((F, D, H, W), dt)
    amb = np.zeros((F, D, H, W), bool)
    taps = window_taps(H, W, r)
    for f in range(F):
        n = int(ok[f].sum())
        denom = (taps * max(n, 1)).astype(np.float32).astype(dt)
        for k in range(D):
            A = np.zeros((H, W), dt)
            flag = np.zeros((H, W), bool)
            for s in range(S):
                if not ok[f, s]:
                    continue
                Hm = np.asarray(homographies[f, s, k], np.float32)
                ad, _, _, _ = _warp(grey[f], grey[src_index[f, s]], Hm, oob, dt)
                A = A + ad
                _, q2, sx, sy = _warp(grey[f], grey[src_index[f, s]], Hm, oob, np.float64)
                with np.errstate(all="ignore"):
                    near_x = ((np.abs(sx) < BORDER_EPS) | (np.abs(sx - (W - 1)) < BORDER_EPS)) & (sy > -BORDER_EPS) & (sy < H - 1 + BORDER_EPS)
                    near_y = ((np.abs(sy) < BORDER_EPS) | (np.abs(sy - (H - 1)) < BORDER_EPS)) & (sx > -BORDER_EPS) & (sx < W - 1 + BORDER_EPS)
                    flag |= (np.abs(q2) < Q2_EPS) | near_x | near_y | ~np.isfinite(q2)
            C[f, k] = _box(A, r, dt) / denom
            amb[f, k] = _box(flag.astype(np.float64), r, np.float64) > 0
    return C, amb


def winner_ref(C):
    """[..., D, H, W] -> the plane of the lowest cost, ties to the lowest plane"""
    return np.argmin(C, axis=-3)


def _at(C, k):
    return np.take_along_axis(C, k[None], axis=0)[0]


def parabola_offset(C, k):
    """C [D,H,W], k int [H,W] -> (off [H,W], refined bool [H,W], curv [H,W]): the sub-plane offset in [-0.5, 0.5] where 0 < k < D - 1
    and the parabola through the three costs is convex; 0 and False elsewhere"""
    D = C.shape[0]
    inner = (k > 0) & (k < D - 1)
    c = _at(C, k)
    cl, cr = _at(C, np.maximum(k - 1, 0)), _at(C, np.minimum(k + 1, D - 1))
    curv = (cl + cr) - 2 * c
    refined = inner & (curv > 0)
    with np.errstate(all="ignore"):
        off = np.where(refined, np.clip(0.5 * (cl - cr) / np.where(refined, curv, 1), -0.5, 0.5), 0.0)
    return off, refined, np.where(inner, curv, 0.0)


def inverse_depth_at(inv_depth, k, off):
    """inv_depth [D], k [H,W], off [H,W] -> inverse depth moved |off| of the way to the neighbour on off's side"""
    D = len(inv_depth)
    base = inv_depth[k]
    nb = np.where(off >= 0, inv_depth[np.minimum(k + 1, D - 1)], inv_depth[np.maximum(k - 1, 0)])
    return base + np.abs(off) * (nb - base)


def confidence_ref(C, k, n_present):
    """-> (conf [H,W], has_runner_up bool [H,W]): (C2 - C1) / max(C2, 1e-6), C2 the lowest cost more than one plane from k; 0 without one
    or without a source"""
    D = C.shape[0]
    far = np.abs(np.arange(D)[:, None, None] - k[None]) > 1
    has = far.any(0) & (n_present > 0)
    c2 = np.where(far, C, np.inf).min(0)
    c1 = _at(C, k)
    with np.errstate(all="ignore"):
        conf = np.where(has, (c2 - c1) / np.maximum(c2, 1e-6), 0.0)
    return conf, has


def sweep_ref(C, inv_depth, n_present):
    """The kernel's four outputs for one view from its cost volume C [D,H,W]: (depth, conf, winner, winner cost)"""
    k = winner_ref(C)
    off, _, _ = parabola_offset(C, k)
    conf, _ = confidence_ref(C, k, n_present)
    return 1.0 / inverse_depth_at(np.asarray(inv_depth, np.float64), k, off), conf, k, _at(C, k)


def consistency_ref(depth, rel_pose, src_index, conf, fx, fy, cx, cy, rel_tol, min_consistent):
    """float32 in the kernel's order -> (conf with the rejected pixels zeroed, agree counts int [F,H,W], borderline bool [F,H,W]: a present
    source's verdict hangs on the last bits -- the depth difference within 1e-4 Z of the tolerance, the projection within 1e-3 px of a
    rounding or image boundary, or Z within 1e-6 of 0)"""
    f32 = np.float32
    depth = np.asarray(depth, f32)
    F, H, W = depth.shape
    ok = present(src_index, F)
    fx, fy, cx, cy, rel_tol = f32(fx), f32(fy), f32(cx), f32(cy), f32(rel_tol)
    y, x = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing="ij")
    out = np.array(conf, f32, copy=True)
    agree = np.zeros((F, H, W), np.int64)
    border = np.zeros((F, H, W), bool)
    for f in range(F):
        z = depth[f]
        xc, yc = (x - cx) * z / fx, (y - cy) * z / fy
        for s in range(src_index.shape[1]):
            if not ok[f, s]:
                continue
            T = np.asarray(rel_pose[f, s], f32)
            X = ((T[0, 0] * xc + T[0, 1] * yc) + T[0, 2] * z) + T[0, 3]
            Y = ((T[1, 0] * xc + T[1, 1] * yc) + T[1, 2] * z) + T[1, 3]
            Z = ((T[2, 0] * xc + T[2, 1] * yc) + T[2, 2] * z) + T[2, 3]
            with np.errstate(all="ignore"):
                pu, pv = (fx * X / Z + cx) + f32(0.5), (fy * Y / Z + cy) + f32(0.5)
                u, v = np.floor(pu), np.floor(pv)
                inb = (Z > 0) & (u >= 0) & (u <= f32(W - 1)) & (v >= 0) & (v <= f32(H - 1))
                ui, vi = np.where(inb, u, 0).astype(np.int64), np.where(inb, v, 0).astype(np.int64)
                zs = depth[src_index[f, s]][vi, ui]
                agree[f] += inb & (np.abs(zs - Z) <= rel_tol * Z)
                edge = (np.abs(pu - np.rint(pu)) < 1e-3) | (np.abs(pv - np.rint(pv)) < 1e-3) | (np.abs(Z) < 1e-6) | ~np.isfinite(pu + pv)
                border[f] |= edge | (inb & (np.abs(np.abs(zs - Z) - rel_tol * Z) < 1e-4 * np.abs(Z)))
        out[f][agree[f] < min_consistent] = 0
    return out, agree, border


# ------------------------------------------------------------------ the analytic scene
def look_at_w2c(eye, target):
    """float64 [3,4] world->camera of a camera at `eye` looking at `target`: x right, y down, z forward, no roll (world y is down)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ eye)[:, None]], 1)


class BoxScene:
    """The inside of the box lo .. hi (world x right, y down, z forward).  The texture is a sum of sinusoids over fixed, mutually
    irrational directions and wavelengths of the 3D point -- smooth, non-periodic, with gradient at the scale of a stereo patch -- so a
    pixel's grey level is a continuous function of the surface point it sees, also across the box's edges."""
    WAVES = (  # (direction, wavelength in scene units, amplitude in grey levels, phase)
        ((1.0, 0.31, 0.17), 1.9, 11.0, 0.3), ((-0.23, 1.0, 0.41), 1.3, 8.0, 1.1), ((0.37, -0.19, 1.0), 1.6, 10.0, 2.3),
        ((1.0, 1.0, -0.53), 3.1, 22.0, 0.7), ((-0.71, 0.43, 1.0), 4.3, 26.0, 1.9), ((0.59, -1.0, 0.29), 2.7, 18.0, 4.1),
    )

    def __init__(self, lo=(-5.0, -2.6, -4.5), hi=(5.5, 1.6, 8.0), wavelength_scale=1.0):
        self.lo, self.hi, self.wavelength_scale = np.asarray(lo, np.float64), np.asarray(hi, np.float64), float(wavelength_scale)

    def texture(self, P):
        g = np.full(P.shape[:-1], 128.0)
        for d, lam, amp, ph in self.WAVES:
            d = np.asarray(d) / np.linalg.norm(d)
            g = g + amp * np.sin(P @ d * (2 * math.pi / (lam * self.wavelength_scale)) + ph)
        return g

    def cast(self, origin, dirs):
        """rays origin + t dirs from inside the box -> (t, face id 0..5) of the wall they hit"""
        with np.errstate(all="ignore"):
            wall = np.where(dirs > 0, self.hi, self.lo)
            t = np.where(dirs != 0, (wall - origin) / dirs, np.inf)
        axis = np.argmin(t, axis=-1)
        tt = np.take_along_axis(t, axis[..., None], -1)[..., 0]
        return tt, axis * 2 + (np.take_along_axis(dirs, axis[..., None], -1)[..., 0] > 0)

    def wall_distance(self, P):
        """distance of points to the nearest wall plane (for points on or near the box's surface)"""
        return np.minimum(np.abs(P - self.lo), np.abs(P - self.hi)).min(-1)

    def render_views(self, w2c, K, H, W):
        """w2c [F,3,4] scene->camera, K [3,3] -> (grey uint8 [F,H,W], depth float64 [F,H,W], face id [F,H,W], unrounded grey)"""
        K = np.asarray(K, np.float64)
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        dc = np.stack([(x - K[0, 2]) / K[0, 0], (y - K[1, 2]) / K[1, 1], np.ones_like(x)], -1)
        grey, depth, face = [], [], []
        for E in np.asarray(w2c, np.float64):
            R, t = E[:3, :3], E[:3, 3]
            o = -R.T @ t
            tt, fid = self.cast(o, dc @ R)
            grey.append(self.texture(o + tt[..., None] * (dc @ R)))
            depth.append(tt)
            face.append(fid)
        g = np.stack(grey)
        return np.clip(np.rint(g), 0, 255).astype(np.uint8), np.stack(depth), np.stack(face), g

    def render_panos(self, c2w, He, We):
        """c2w [F,4,4] panorama camera->scene -> uint8 [F,He,We,3] (R = G = B): the inverse of ew_equi2pers' direction <-> pixel map as
        oracle/reproject_ref.py restates it: column i <-> lon = (i - We / 2 - 0.5) 2 pi / We, row j <-> lat = (j - He / 2 - 0.5) pi / He,
        direction (cos lat sin lon, sin lat, cos lat cos lon) in the camera's x right, y down, z forward frame"""
        j, i = np.meshgrid(np.arange(He, dtype=np.float64), np.arange(We, dtype=np.float64), indexing="ij")
        lon, lat = (i - We * 0.5 - 0.5) * (2 * math.pi / We), (j - He * 0.5 - 0.5) * (math.pi / He)
        d = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], -1)
        out = []
        for M in np.asarray(c2w, np.float64):
            dw = d @ M[:3, :3].T
            tt, _ = self.cast(M[:3, 3], dw)
            g = np.clip(np.rint(self.texture(M[:3, 3] + tt[..., None] * dw)), 0, 255).astype(np.uint8)
            out.append(np.repeat(g[..., None], 3, -1))
        return np.stack(out)


def near_face_edge(face):
    """[F,H,W] face ids -> bool: the pixel or one of its 8 neighbours sees another wall (within one pixel of a box edge)"""
    F, H, W = face.shape
    p = np.pad(face, ((0, 0), (1, 1), (1, 1)), mode="edge")
    out = np.zeros(face.shape, bool)
    for dy in range(3):
        for dx in range(3):
            out |= p[:, dy:dy + H, dx:dx + W] != face
    return out


def arc_path(n, radius=9.0, sweep_deg=16.0, centre=(0.3, -0.4, 6.5), height=-0.4, climb=0.9):
    """n cameras on an arc around `centre` that also climbs (no two at one height, so that no image row maps onto a source's border row for
    a whole view), all looking at the centre: a curved path with high overlap -> w2c float64 [n,3,4]"""
    out = []
    for a in np.linspace(-sweep_deg / 2, sweep_deg / 2, n) if n > 1 else [0.0]:
        a = math.radians(a)
        eye = np.array([centre[0] + radius * math.sin(a), height + climb * a, centre[2] - radius * math.cos(a)])
        out.append(look_at_w2c(eye, centre))
    return np.stack(out)


def sweep_case(F, H, W, S, D, r, oob=48.0, absent=(), no_source_view=None, push_out=False, scene=None, sweep_deg=16.0):
    """One input of the GPU tests: F views of the box scene on the arc, sweep_setup's tables for them (evoworld_amd.mvs), then the edits the
    case asks for: `absent` = (view, slot) pairs set to -1, no_source_view = a view whose slots are all -1, push_out = the homographies of
    slot 0 shifted 3 W / 4 to the right on the odd planes (whole tiles leave the source) and those of the last slot negated on plane 0
    (q2 < 0 everywhere)."""
    from evoworld_amd import mvs
    scene = scene or BoxScene()
    K = mvs.pinhole(H, W)
    w2c = arc_path(F, sweep_deg=sweep_deg)
    grey, depth, face, _ = scene.render_views(w2c, K, H, W)
    st = mvs.sweep_setup(w2c, K, S, D)
    src = st.src_index.copy()
    for f, s in absent:
        src[f, s] = -1
    if no_source_view is not None:
        src[no_source_view] = -1
    Hm = st.homographies_f32.copy()
    if push_out:
        shift = np.array([[1, 0, 0.75 * W], [0, 1, 0], [0, 0, 1]], np.float64)
        Hm[:, 0, 1::2] = (shift @ st.homographies[:, 0, 1::2]).astype(np.float32)
        Hm[:, -1, 0] = -Hm[:, -1, 0]
    return SimpleNamespace(F=F, H=H, W=W, S=S, D=D, r=r, oob=oob, grey=grey, true_depth=depth, face=face, w2c=w2c, K=K, setup=st,
                           src_index=src, homographies=Hm, inv_depth=st.inv_depth_f32.copy(), rel_pose=st.rel_pose_f32.copy(),
                           id=f"F{F}_{H}x{W}_S{S}_D{D}_r{r}" + ("_out" if push_out else ""))


# F = 3 at 37 x 53 is ragged against any tile, F = 2 at 8 x 8 smaller than one, F = 5 at 48 x 64 whole tiles; S in {1, 4} with absent slots
# (F - 1 < 4 leaves some, others are struck out), D in {2, 3, 32}, r in {0, 2, 3}; one input pushes whole tiles out of the source
GPU_CASES = (
    dict(F=3, H=37, W=53, S=1, D=2, r=0),
    dict(F=3, H=37, W=53, S=4, D=3, r=3, absent=((1, 0),)),
    dict(F=3, H=37, W=53, S=4, D=32, r=2, no_source_view=2),
    dict(F=3, H=37, W=53, S=1, D=32, r=3),
    dict(F=3, H=37, W=53, S=4, D=32, r=2, push_out=True),
    dict(F=2, H=8, W=8, S=1, D=3, r=3),
    dict(F=2, H=8, W=8, S=4, D=32, r=2),
    dict(F=2, H=8, W=8, S=4, D=2, r=0, absent=((0, 0),)),
    dict(F=5, H=48, W=64, S=4, D=32, r=0, absent=((2, 1), (4, 3))),
    dict(F=5, H=48, W=64, S=1, D=32, r=2),
    dict(F=5, H=48, W=64, S=1, D=2, r=3),
)
RECOVERY_CASE = dict(F=5, H=48, W=64, S=4, D=32, r=2)

# the episode of the pose tests: a curved path whose cameras also turn, tilted a little about both other axes; pose 48 is what segment 0 looks at
POSE_CAM = np.stack([3.0 * np.sin(np.arange(50) / 6), np.full(50, -0.3), -3.5 + 0.2 * np.arange(50), np.full(50, 2.0),
                     95 + 3.6 * np.arange(50), np.full(50, -1.5)], 1)


def pose_scene():
    """The box of the pose tests: so large that the first five views of POSE_CAM see one wall (6 - 11 units away) and at most a strip of a
    second one, with the texture's wavelengths stretched until a 128 x 256 panorama resolves it (a bilinear cut then stays within the
    8-bit rounding of the direct render)."""
    return BoxScene(lo=(-14.0, -9.0, -14.0), hi=(15.0, 9.0, 4.0), wavelength_scale=4.5)


_case_cache = {}


def cached_case(**kw):
    """sweep_case plus its two cost volumes, computed once per process and never modified by a test"""
    key = tuple(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in kw.items()))
    if key not in _case_cache:
        c = sweep_case(**kw)
        c.C64, c.ambiguous = cost_volume(c.grey, c.homographies, c.src_index, c.r, c.oob, np.float64)
        c.C64.setflags(write=False)
        c.ambiguous.setflags(write=False)
        _case_cache[key] = c
    return _case_cache[key]


def kept_and_correct(conf, depth, true_depth, inv_depth_step):
    """The recovery figure: among the pixels the pipeline would keep (confidence >= its 50th percentile over all views), the share whose
    inverse depth is within 1.5 plane steps of the truth.  inv_depth_step [F]. -> (share, number kept)"""
    keep = conf >= np.percentile(conf, 50.0)
    err = np.abs(1.0 / depth - 1.0 / true_depth) / np.asarray(inv_depth_step)[:, None, None]
    return float((err[keep] <= 1.5).mean()), int(keep.sum())
