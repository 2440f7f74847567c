"""numpy oracle of the ZNCC matching cost of the two sweeps (evoworld_amd/csrc/mvs_zncc.hip, evoworld_amd/mvs.py; include/evoworld_hip.h
states the rules).  A helper module, not a test.  The scene, the cases, the box filters, the pixel <-> direction maps and
the winner, parabola and confidence rules are those of tests/mvs_ref.py and tests/mvs_sphere_ref.py; only the sample (their warps return
the absolute difference, not the sample itself) and the correlation are stated here.

  zncc_volume        C(k) per pixel in float64 (the truth) or in float32 in the header's order, plus the ambiguous (pixel, hypothesis) pairs:
                     those whose window holds a tap the SAD oracles flag (BORDER_EPS, Q2_EPS, CENTRE_EPS) -- which are also the windows
                     whose validity hangs on such a tap
  flicker            a fixed gain, offset and gamma per view on unrounded grey levels, then rounded to uint8
  plane_unrounded / sphere_unrounded      the unrounded grey levels of a case's views
  PLANE_CASES / SPHERE_CASES / cached     the inputs of tests/test_gpu_mvs_zncc.py (R.GPU_CASES / S.GPU_CASES with r >= 1), with their
                                          float64 volumes computed once per process
  recovery           the figure of R.kept_and_correct for a cost volume
"""
import numpy as np

import mvs_ref as R
import mvs_sphere_ref as S

# The largest |float32-order cost - float64 cost| over the inputs of the GPU tests (ambiguous pairs left out), in PERCENT (the cost runs
# from 0 to 200), measured by tests/test_cpu_mvs_zncc.py::test_margin_constant_covers_the_measured_float32_error and rounded up: plane
# 8.6e-3, sphere 7.9e-2 when this was written (the 99.99th percentile of the worst case: 3.0e-3 and 2.5e-2).  Both are far below the 0.5 at
# which the cancellation in n Saa - Sa Sa would have to be written differently.  The sphere's is larger for the reason its SAD margin is
# (S.SPHERE_F32_MARGIN): float32 atan2f / asinf move a sample that lands near a source's pole, and a correlation divides that by the
# window's contrast.  ZNCC_F32_MARGIN is the larger of the two; the GPU tests allow COST_TOL[kind] = COST_TOL_FACTOR x the kind's own
# margin.  The factor is for the device's sinf / cosf / atan2f / asinf against numpy's (each moves a sample by ulps of a coordinate), not
# for kernel changes: the rule of mvs_ref.COST_TOL.
F32_MARGIN = {"plane": 1.0e-2, "sphere": 1.0e-1}
ZNCC_F32_MARGIN = max(F32_MARGIN.values())
COST_TOL_FACTOR = 2.0
COST_TOL = {kind: COST_TOL_FACTOR * m for kind, m in F32_MARGIN.items()}
MAX_AMBIGUOUS_SHARE = 0.005                                 # R.MAX_AMBIGUOUS_SHARE and S.MAX_AMBIGUOUS_SHARE, unchanged
VAR_FLOOR, OOB_COST, COST_SCALE = 1.0, 100.0, 16.0          # the stage defaults
MID = 128.0

FLICKER_GAIN = (1.0, 0.7, 1.3, 0.75, 1.25)                  # about grey level 128
FLICKER_OFFSET = (0.0, 20.0, -25.0, 15.0, -10.0)
FLICKER_GAMMA = (1.0, 0.8, 1.25, 1.2, 0.85)


def flicker(grey):
    """unrounded grey levels [F,...] -> uint8: view i gets gain, offset and gamma number i mod 5 -- v = 128 + gain (g - 128) + offset,
    clipped to [0, 255], then 255 (v / 255) ^ gamma, rounded"""
    g = np.asarray(grey, np.float64)
    out = np.empty(g.shape, np.uint8)
    for i in range(len(g)):
        j = i % len(FLICKER_GAIN)
        v = np.clip(MID + FLICKER_GAIN[j] * (g[i] - MID) + FLICKER_OFFSET[j], 0.0, 255.0)
        out[i] = np.clip(np.rint(255.0 * (v / 255.0) ** FLICKER_GAMMA[j]), 0, 255).astype(np.uint8)
    return out


def plane_unrounded(c, scene=None):
    """the unrounded grey levels [F,H,W] of a R.sweep_case"""
    return (scene or R.BoxScene()).render_views(c.w2c, c.K, c.H, c.W)[3]


def sphere_unrounded(c, scene=None):
    """the unrounded grey levels [F,He,We] of a S.sphere_case: BoxScene.render_panos without the rounding"""
    scene = scene or R.BoxScene()
    d = S.pixel_dir(c.H, c.W)
    out = []
    for M in np.linalg.inv(S._four(c.w2c)):
        dw = d @ M[:3, :3].T
        tt, _ = scene.cast(M[:3, 3], dw)
        out.append(scene.texture(M[:3, 3] + tt[..., None] * dw))
    return np.stack(out)


def _plane_sample(src, Hm, H, W, dt):
    """b = bilinear(src, H (x, y, 1)) - 128 per reference pixel in dtype dt, in the header's order (0 where invalid); valid; (q2, sx, sy)"""
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
    b = np.where(inb, (top * (one - ay) + bot * ay) - dt(MID), dt(0))
    assert b.dtype == dt
    return b, inb, (q2, sx, sy)


def _sphere_sample(a, src, T, inv, d, dt):
    """b per reference pixel in dtype dt, in the header's order: bilinear(src, pix(R (dir rad) + t)) - 128, and a where |Ps| is 0 or not
    finite; also |Ps|"""
    He, We = src.shape
    T = np.asarray(T, dt)
    rad = dt(1) / dt(inv)
    X, Y, Z = S._move(T, d[..., 0] * rad, d[..., 1] * rad, d[..., 2] * rad)
    u, v, nrm = S.dir_pixel(X, Y, Z, He, We, dt)
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
    b = np.where(ok, (top * (one - ay) + bot * ay) - dt(MID), a)
    assert b.dtype == dt
    return b, nrm


def correlation_cost(n, Sa, Saa, Sb, Sbb, Sab, var_floor, dt):
    """the header's correlation on the five window sums, every operation in dtype dt: -> (100 (1 - zncc), va, vb)"""
    nf = np.asarray(n).astype(np.float32).astype(dt)
    cov = nf * Sab - Sa * Sb
    va = np.maximum(nf * Saa - Sa * Sa, dt(0))
    vb = np.maximum(nf * Sbb - Sb * Sb, dt(0))
    fl = dt(var_floor) * (nf * nf)
    den = np.sqrt(va * vb + fl * fl)
    with np.errstate(all="ignore"):
        z = np.where(den > 0, cov / np.where(den > 0, den, dt(1)), dt(0))
    cost = dt(100) * (dt(1) - z)
    assert cost.dtype == dt
    return cost, va, vb


def zncc_volume(kind, c, var_floor=VAR_FLOOR, oob=OOB_COST, dtype=np.float64, grey=None, with_variances=False):
    """kind "plane": c a R.sweep_case (grey, homographies, src_index, r); "sphere": c a S.sphere_case (grey, rel_pose, inv_dist, src_index,
    r); grey: other frames than the case's own (uint8 [F,H,W]) -> (C [F,D,H,W] in dtype, ambiguous bool [F,D,H,W]).  float64: the truth.
    float32: every operation rounded once, in the order the header writes down.  with_variances: also (va [F,H,W], vb_min [F,D,H,W]), the
    reference window's variance term and the lowest source term of a pair (inf without a present source)."""
    dt = np.float32 if dtype == np.float32 else np.float64
    assert kind in ("plane", "sphere") and c.r >= 1
    grey = c.grey if grey is None else grey
    F, H, W = grey.shape
    r, D = c.r, c.D
    ok = R.present(c.src_index, F)
    box = (lambda a, t=dt: R._box(a, r, t)) if kind == "plane" else (lambda a, t=dt: S._box(a, r, t))
    n = R.window_taps(H, W, r) if kind == "plane" else np.broadcast_to(((2 * r + 1) * S.window_rows(H, r))[:, None], (H, W))
    if kind == "sphere":
        d, d64 = S.pixel_dir(H, W, dt), S.pixel_dir(H, W, np.float64)
    C = np.zeros((F, D, H, W), dt)
    amb = np.zeros((F, D, H, W), bool)
    VA, VB = np.zeros((F, H, W), dt), np.full((F, D, H, W), np.inf)
    for f in range(F):
        slots = dt(np.float32(max(int(ok[f].sum()), 1)))
        a = grey[f].astype(dt) - dt(MID)
        Sa, Saa = box(a), box(a * a)
        for k in range(D):
            acc = np.zeros((H, W), dt)
            flag = np.zeros((H, W), bool)
            for s in range(c.S):
                if not ok[f, s]:
                    continue
                src = grey[c.src_index[f, s]]
                if kind == "plane":
                    Hm = np.asarray(c.homographies[f, s, k], np.float32)
                    b, valid, _ = _plane_sample(src, Hm, H, W, dt)
                    _, _, (q2, sx, sy) = _plane_sample(src, Hm, H, W, np.float64)
                    with np.errstate(all="ignore"):
                        near_x = ((np.abs(sx) < R.BORDER_EPS) | (np.abs(sx - (W - 1)) < R.BORDER_EPS)) & (sy > -R.BORDER_EPS) & (sy < H - 1 + R.BORDER_EPS)
                        near_y = ((np.abs(sy) < R.BORDER_EPS) | (np.abs(sy - (H - 1)) < R.BORDER_EPS)) & (sx > -R.BORDER_EPS) & (sx < W - 1 + R.BORDER_EPS)
                        flag |= (np.abs(q2) < R.Q2_EPS) | near_x | near_y | ~np.isfinite(q2)
                    invalid = box((~valid).astype(np.float64), np.float64) > 0          # a window with one tap outside the source
                else:
                    T, inv = np.asarray(c.rel_pose[f, s], np.float32), np.float32(c.inv_dist[f, k])
                    b, nrm = _sphere_sample(a, src, T, inv, d, dt)
                    if dt == np.float32:
                        _, nrm = _sphere_sample(a.astype(np.float64), src, T, inv, d64, np.float64)
                    flag |= ~(nrm >= S.CENTRE_EPS)
                    invalid = np.zeros((H, W), bool)
                cost, va, vb = correlation_cost(n, Sa, Saa, box(b), box(b * b), box(a * b), var_floor, dt)
                acc = acc + np.where(invalid, dt(oob), cost)
                VA[f] = va
                VB[f, k] = np.minimum(VB[f, k], np.where(invalid, np.inf, vb))
            C[f, k] = acc / slots
            amb[f, k] = box(flag.astype(np.float64), np.float64) > 0
    assert C.dtype == dt
    return (C, amb, VA, VB) if with_variances else (C, amb)


PLANE_CASES = tuple(kw for kw in R.GPU_CASES if kw["r"] >= 1)
SPHERE_CASES = tuple(kw for kw in S.GPU_CASES if kw["r"] >= 1)
PLANE_R0 = next(kw for kw in R.GPU_CASES if kw["r"] == 0)       # used only to check the refusal
SPHERE_R0 = next(kw for kw in S.GPU_CASES if kw["r"] == 0)


def case_id(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items() if k in ("F", "H", "W", "He", "We", "S", "D", "r")) + ("-out" if kw.get("push_out") else "") + \
        ("-yaw" if kw.get("yaw_step") else "")


_cache = {}


def cached(kind, **kw):
    """(the R / S cached case, its float64 ZNCC volume Z64 [F,D,H,W], ambiguous [F,D,H,W]) at the stage defaults; computed once per process
    and never modified by a test"""
    key = (kind,) + tuple(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in kw.items()))
    if key not in _cache:
        c = R.cached_case(**kw) if kind == "plane" else S.cached_case(**kw)
        Z, amb = zncc_volume(kind, c, VAR_FLOOR, OOB_COST, np.float64)
        Z.setflags(write=False)
        amb.setflags(write=False)
        _cache[key] = (c, Z, amb)
    return _cache[key]


def truth_and_tables(kind, c):
    """(true depth or distance [F,H,W], inverse table float32 [F,D], hypothesis step [F]) of a case"""
    if kind == "plane":
        return c.true_depth, c.inv_depth, np.diff(c.setup.inv_depth, axis=1)[:, 0]
    return c.true_dist, c.inv_dist, np.diff(c.setup.inv_dist, axis=1)[:, 0]


def recovery(kind, c, C):
    """R.kept_and_correct of the winner of the cost volume C [F,D,H,W] (R.sweep_ref per view) -> share"""
    truth, inv, step = truth_and_tables(kind, c)
    n_present = R.present(c.src_index, c.F).sum(1)
    outs = [R.sweep_ref(C[f], inv[f], n_present[f]) for f in range(c.F)]
    return R.kept_and_correct(np.stack([o[1] for o in outs]), np.stack([o[0] for o in outs]), truth, step)[0]


def recovery_shares(kind):
    """RECOVERY_CASE of the kind -> dict(zncc_clean, zncc_flicker, sad_clean, sad_flicker): the float64 oracles' shares; computed once"""
    key = ("recovery", kind)
    if key not in _cache:
        if kind == "plane":
            c = R.cached_case(**R.RECOVERY_CASE)
            fl = flicker(plane_unrounded(c))
            sad = lambda g: R.cost_volume(g, c.homographies, c.src_index, c.r, c.oob, np.float64)[0]
            sad_clean = c.C64
        else:
            c = S.cached_case(**S.RECOVERY_CASE)
            fl = flicker(sphere_unrounded(c))
            sad = lambda g: S.cost_volume(g, c.rel_pose, c.src_index, c.inv_dist, c.r, np.float64)[0]
            sad_clean = c.C64
        assert np.array_equal(flicker(plane_unrounded(c) if kind == "plane" else sphere_unrounded(c))[0], c.grey[0])     # view 0 does not flicker
        _cache[key] = dict(case=c, flickered=fl,
                           zncc_clean=recovery(kind, c, cached(kind, **(R.RECOVERY_CASE if kind == "plane" else S.RECOVERY_CASE))[1]),
                           zncc_flicker=recovery(kind, c, zncc_volume(kind, c, grey=fl)[0]),
                           sad_clean=recovery(kind, c, sad_clean), sad_flicker=recovery(kind, c, sad(fl)))
    return _cache[key]
