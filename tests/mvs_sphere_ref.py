"""numpy oracle of the sphere-sweep stereo stage (evoworld_amd/csrc/mvs_sphere.hip, evoworld_amd/mvs.py; include/evoworld_hip.h states the
rules).  The winner, parabola and confidence rules are those of the plane sweep and are taken from tests/mvs_ref.py, as are the scene, the
paths and the recovery figure.

  pixel_dir / dir_pixel     the two sides of ew_equi2pers' direction <-> pixel map, in float64 or in float32 in the header's order
  cost_volume               C(k) per pixel in float64 (the truth) or in float32 with every operation rounded once, plus the (pixel,
                            hypothesis) pairs whose window holds a tap that lands on a source's centre
  consistency_ref           the cross-view check in float32 order, with the pixels whose verdict hangs on the last bits
  unproject_ref             R (dir dist) + t in float64
  sphere_case / GPU_CASES   the inputs of tests/test_gpu_mvs_sphere.py, shared with the CPU tests that measure the margin on them
"""
import math
from types import SimpleNamespace

import numpy as np

from mvs_ref import BoxScene, arc_path, present

# The largest |float32-order cost - float64 cost| over the inputs of the GPU tests (no ambiguous pair exists on them), in grey levels,
# measured by tests/test_cpu_mvs_sphere.py::test_margin_constant_covers_the_measured_float32_error (2.1e-3 when this was written, at a
# point that lands within a pixel of a source's pole, where asinf and atan2f are ill-conditioned; 3e-4 is exceeded by 7e-5 of the pairs
# of one case and by none of the others), rounded up.  The GPU tests allow COST_TOL = COST_TOL_FACTOR x this; the factor is for the device's sinf / cosf / atan2f / asinf against numpy's
# (each moves a sample by ulps of an angle), not for kernel changes: the rule of mvs_ref.COST_TOL.
SPHERE_F32_MARGIN = 2.5e-3
COST_TOL_FACTOR = 2.0
COST_TOL = COST_TOL_FACTOR * SPHERE_F32_MARGIN
CENTRE_EPS = 1e-6          # a source point this close to the source's centre has no direction: the pair is ambiguous
MAX_AMBIGUOUS_SHARE = 0.005
PI32 = np.float32(3.14159265358979323846)


def pixel_dir(He, We, dt=np.float64):
    """-> [He,We,3] unit directions of the pixels (x right, y down, z forward), the header's dir(x, y)"""
    dt = np.float32 if dt == np.float32 else np.float64
    pi = PI32 if dt == np.float32 else dt(math.pi)
    Wf, Hf, half = dt(We), dt(He), dt(0.5)
    y, x = np.meshgrid(np.arange(He, dtype=dt), np.arange(We, dtype=dt), indexing="ij")
    lon = ((x - Wf * half) - half) * ((dt(2) * pi) / Wf)
    lat = ((y - Hf * half) - half) * (pi / Hf)
    cl = np.cos(lat)
    d = np.stack([cl * np.sin(lon), np.sin(lat), cl * np.cos(lon)], -1)
    assert d.dtype == dt
    return d


def dir_pixel(X, Y, Z, He, We, dt=np.float64):
    """points in a panorama camera -> (u unwrapped, v unclamped, nrm), the header's pix(X, Y, Z)"""
    dt = np.float32 if dt == np.float32 else np.float64
    pi = PI32 if dt == np.float32 else dt(math.pi)
    Wf, Hf, half = dt(We), dt(He), dt(0.5)
    nrm = np.sqrt((X * X + Y * Y) + Z * Z)
    with np.errstate(all="ignore"):
        lon = np.arctan2(X, Z)
        lat = np.arcsin(np.clip(Y / nrm, dt(-1), dt(1)))
    u = ((lon * Wf) / (dt(2) * pi) + Wf * half) + half
    v = ((lat * Hf) / pi + Hf * half) + half
    assert u.dtype == dt and v.dtype == dt
    return u, v, nrm


def _move(T, px, py, pz):
    X = ((T[0, 0] * px + T[0, 1] * py) + T[0, 2] * pz) + T[0, 3]
    Y = ((T[1, 0] * px + T[1, 1] * py) + T[1, 2] * pz) + T[1, 3]
    Z = ((T[2, 0] * px + T[2, 1] * py) + T[2, 2] * pz) + T[2, 3]
    return X, Y, Z


def _warp(ref, src, T, inv, d, dt):
    """per-pixel AD of one (reference, source, hypothesis) in dtype dt, in the header's order; also |Ps|"""
    He, We = ref.shape
    T = np.asarray(T, dt)
    rad = dt(1) / dt(inv)
    X, Y, Z = _move(T, d[..., 0] * rad, d[..., 1] * rad, d[..., 2] * rad)
    u, v, nrm = dir_pixel(X, Y, Z, He, We, dt)
    ok = (nrm > 0) & np.isfinite(nrm)
    Wf = dt(We)
    u, v = np.where(ok, u, dt(0)), np.where(ok, v, dt(0))
    u = u - np.floor(u / Wf) * Wf
    v = np.minimum(np.maximum(v, dt(0)), dt(He - 1))
    x0f, y0f = np.floor(u), np.floor(v)
    ax, ay = u - x0f, v - y0f
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x0 = np.where(x0 >= We, x0 - We, x0)
    x1 = np.where(x0 + 1 >= We, 0, x0 + 1)
    y1 = np.minimum(y0 + 1, He - 1)
    s = src.astype(dt)
    one = dt(1)
    top = s[y0, x0] * (one - ax) + s[y0, x1] * ax
    bot = s[y1, x0] * (one - ax) + s[y1, x1] * ax
    ad = np.where(ok, np.abs(ref.astype(dt) - (top * (one - ay) + bot * ay)), dt(0))
    assert ad.dtype == dt
    return ad, nrm


def _box(a, r, dt):
    """rows of taps left to right with the columns wrapping across the seam, then the row sums top to bottom; rows outside add 0"""
    He, We = a.shape
    p = np.zeros((He + 2 * r, We + 2 * r), dt)
    p[r:r + He] = a[:, np.arange(-r, We + r) % We]
    rs = np.zeros((He + 2 * r, We), dt)
    for k in range(2 * r + 1):
        rs = rs + p[:, k:k + We]
    c = np.zeros((He, We), dt)
    for k in range(2 * r + 1):
        c = c + rs[k:k + He]
    assert c.dtype == dt
    return c


def window_rows(He, r):
    ys = np.arange(He)
    return np.minimum(ys + r, He - 1) - np.maximum(ys - r, 0) + 1


def cost_volume(grey, rel_pose, src_index, inv_dist, r, dtype=np.float64):
    """grey uint8 [F,He,We]; rel_pose [F,S,3,4] and inv_dist [F,D] -- the float32 values the device gets; src_index [F,S] -> (C [F,D,He,We]
    in dtype, ambiguous bool [F,D,He,We]).  float64: the truth.  float32: every operation rounded once, in the order the header writes."""
    dt = np.float32 if dtype == np.float32 else np.float64
    F, He, We = grey.shape
    S, D = rel_pose.shape[1], inv_dist.shape[1]
    ok = present(src_index, F)
    C = np.zeros((F, D, He, We), dt)
    amb = np.zeros((F, D, He, We), bool)
    d, d64 = pixel_dir(He, We, dt), pixel_dir(He, We, np.float64)
    rows = window_rows(He, r)
    for f in range(F):
        n = int(ok[f].sum())
        denom = ((2 * r + 1) * rows * max(n, 1)).astype(np.float32).astype(dt)[:, None]
        for k in range(D):
            A = np.zeros((He, We), dt)
            flag = np.zeros((He, We), bool)
            for s in range(S):
                if not ok[f, s]:
                    continue
                T = np.asarray(rel_pose[f, s], np.float32)
                inv = np.float32(inv_dist[f, k])
                ad, nrm = _warp(grey[f], grey[src_index[f, s]], T, inv, d, dt)
                A = A + ad
                if dt == np.float32:
                    _, nrm = _warp(grey[f], grey[src_index[f, s]], T, inv, d64, np.float64)
                flag |= ~(nrm >= CENTRE_EPS)
            C[f, k] = _box(A, r, dt) / denom
            amb[f, k] = _box(flag.astype(np.float64), r, np.float64) > 0
    return C, amb


def consistency_ref(dist, rel_pose, src_index, conf, rel_tol, min_consistent):
    """float32 in the kernel's order -> (conf with the rejected pixels zeroed, agree counts int [F,He,We], borderline bool [F,He,We]: a
    present source's verdict hangs on the last bits -- the distance difference within 1e-4 |Ps| of the tolerance, the direction's pixel
    within 1e-3 px of a rounding boundary, or |Ps| within 1e-6 of 0)"""
    f32 = np.float32
    dist = np.asarray(dist, f32)
    F, He, We = dist.shape
    ok = present(src_index, F)
    rel_tol = f32(rel_tol)
    d = pixel_dir(He, We, f32)
    out = np.array(conf, f32, copy=True)
    agree = np.zeros((F, He, We), np.int64)
    border = np.zeros((F, He, We), bool)
    for f in range(F):
        px, py, pz = d[..., 0] * dist[f], d[..., 1] * dist[f], d[..., 2] * dist[f]
        for s in range(src_index.shape[1]):
            if not ok[f, s]:
                continue
            X, Y, Z = _move(np.asarray(rel_pose[f, s], f32), px, py, pz)
            u, v, nrm = dir_pixel(X, Y, Z, He, We, f32)
            with np.errstate(all="ignore"):
                good = (nrm > 0) & np.isfinite(nrm)
                pu, pv = np.where(good, u, 0) + f32(0.5), np.where(good, v, 0) + f32(0.5)
                xi = np.floor(pu).astype(np.int64) % We
                yi = np.clip(np.floor(pv).astype(np.int64), 0, He - 1)
                ds = dist[src_index[f, s]][yi, xi]
                agree[f] += good & (np.abs(ds - nrm) <= rel_tol * nrm)
                edge = (np.abs(pu - np.rint(pu)) < 1e-3) | (np.abs(pv - np.rint(pv)) < 1e-3) | ~(nrm >= 1e-6) | ~np.isfinite(pu + pv)
                border[f] |= edge | (good & (np.abs(np.abs(ds - nrm) - rel_tol * nrm) < 1e-4 * nrm))
        out[f][agree[f] < min_consistent] = 0
    return out, agree, border


def unproject_ref(dist, c2w):
    """float64: dist [F,He,We], c2w [F,3,4] -> [F,He,We,3] = R (dir dist) + t"""
    dist, c2w = np.asarray(dist, np.float64), np.asarray(c2w, np.float64)
    d = pixel_dir(dist.shape[1], dist.shape[2])
    return np.einsum("fij,fhwj->fhwi", c2w[:, :, :3], d[None] * dist[..., None]) + c2w[:, None, None, :, 3]


# ------------------------------------------------------------------ the scene seen by panorama cameras
def _four(w):
    w = np.asarray(w, np.float64)
    E = np.tile(np.eye(4), (len(w), 1, 1))
    E[:, :3, :4] = w[:, :3, :4]
    return E


def turned(w2c, yaw_step_deg):
    """arc_path's cameras, camera i turned on the spot by i x yaw_step_deg about its own y axis -> w2c float64 [n,3,4]: panorama cameras
    of different yaw, so that a source's seam falls mid-image of the reference"""
    E = _four(w2c)
    for i in range(len(E)):
        a = math.radians(yaw_step_deg * i)
        Ry = np.array([[math.cos(a), 0, math.sin(a), 0], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1.0]])
        E[i] = np.linalg.inv(np.linalg.inv(E[i]) @ Ry)
    return E[:, :3, :4]


def true_distance(scene, w2c, He, We):
    """float64 [F,He,We]: the distance along each pixel's direction to the wall it sees"""
    d = pixel_dir(He, We)
    out = []
    for M in np.linalg.inv(_four(w2c)):
        out.append(scene.cast(M[:3, 3], d @ M[:3, :3].T)[0])
    return np.stack(out)


def sphere_case(F, He, We, S, D, r, absent=(), no_source_view=None, yaw_step=0.0, scene=None):
    """One input of the GPU tests: F panoramas of the box scene on the arc (camera i turned by i x yaw_step degrees), sphere_setup's tables
    for them (evoworld_amd.mvs), then the edits the case asks for: `absent` = (view, slot) pairs set to -1, no_source_view = a view whose
    slots are all -1."""
    from evoworld_amd import mvs
    scene = scene or BoxScene()
    w2c = turned(arc_path(F), yaw_step)
    grey = scene.render_panos(np.linalg.inv(_four(w2c)), He, We)[..., 0]
    st = mvs.sphere_setup(w2c, We, S, D)
    src = st.src_index.copy()
    for f, s in absent:
        src[f, s] = -1
    if no_source_view is not None:
        src[no_source_view] = -1
    return SimpleNamespace(F=F, H=He, W=We, S=S, D=D, r=r, grey=grey, true_dist=true_distance(scene, w2c, He, We), w2c=w2c, setup=st,
                           src_index=src, inv_dist=st.inv_dist_f32.copy(), rel_pose=st.rel_pose_f32.copy(),
                           id=f"F{F}_{He}x{We}_S{S}_D{D}_r{r}" + (f"_yaw{yaw_step:g}" if yaw_step else ""))


# F = 3 at 20 x 40: two tile columns, ragged, both halos cross the seam; F = 2 at 8 x 16: smaller than one tile, the halo wraps onto the
# tile itself; F = 5 at 48 x 96: whole tiles.  S in {1, 4} with absent slots (F - 1 < 4 leaves some, others are struck out) and one view
# without sources, D in {2, 3, 32}, r in {0, 2, 3}; yaw_step turns the cameras against each other (130 degrees: a source's seam falls mid-image)
GPU_CASES = (
    dict(F=3, He=20, We=40, S=1, D=2, r=0),
    dict(F=3, He=20, We=40, S=4, D=3, r=3, absent=((1, 0),), yaw_step=130.0),
    dict(F=3, He=20, We=40, S=4, D=32, r=2, no_source_view=2),
    dict(F=3, He=20, We=40, S=1, D=32, r=3, yaw_step=130.0),
    dict(F=2, He=8, We=16, S=1, D=3, r=3),
    dict(F=2, He=8, We=16, S=4, D=32, r=2, yaw_step=130.0),
    dict(F=2, He=8, We=16, S=4, D=2, r=0, absent=((0, 0),)),
    dict(F=5, He=48, We=96, S=4, D=32, r=0, absent=((2, 1), (4, 3)), yaw_step=130.0),
    dict(F=5, He=48, We=96, S=1, D=32, r=2),
    dict(F=5, He=48, We=96, S=1, D=2, r=3),
)
RECOVERY_CASE = dict(F=5, He=48, We=96, S=4, D=32, r=2)

_case_cache = {}


def cached_case(**kw):
    """sphere_case plus its float64 cost volume, computed once per process and never modified by a test"""
    key = tuple(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in kw.items()))
    if key not in _case_cache:
        c = sphere_case(**kw)
        c.C64, c.ambiguous = cost_volume(c.grey, c.rel_pose, c.src_index, c.inv_dist, c.r, np.float64)
        c.C64.setflags(write=False)
        c.ambiguous.setflags(write=False)
        _case_cache[key] = c
    return _case_cache[key]
