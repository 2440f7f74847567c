"""numpy oracle of the semi-global aggregation of the sweeps' cost volume (evoworld_amd/csrc/mvs_sgm.hip and the volume variants of the
two sweeps, evoworld_amd/mvs.py; include/evoworld_hip.h states the rules).  A helper module, not a test.

  quantise               float costs -> the uint16 entries of a cost volume, in float32 in the header's order
  sgm_aggregate_ref      the recurrence along 4 or 8 path directions, in int64
  sgm_select_ref         winner, parabola, confidence on (float32)agg: the rules of tests/mvs_ref.py evaluated in float32
  weak_scene / noisy     the box scene with its texture at 20 % amplitude, and +-3 grey levels of uniform noise
  plane_benefit_case / sphere_benefit_case    the inputs on which the benefit is asserted, with their float32 cost volumes
  share_within           the figure: the share of ALL pixels whose inverse depth is within 1.5 hypothesis steps of the truth
  AGG_SHAPES, PENALTIES  the case tables of tests/test_gpu_mvs_sgm.py
"""
import numpy as np

import mvs_ref as R
import mvs_sphere_ref as RS

COST_MAX = 4095
MAX_D = 256
# (dx, dy) in the header's order; the last four only with paths = 8
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))

# (N, H, W, D): D below, at and above a wave and not a multiple of it; a lone pixel, a lone row, a lone column; ragged lines
AGG_SHAPES = ((1, 1, 1, 1), (1, 1, 7, 2), (1, 7, 1, 3), (3, 37, 53, 32), (2, 9, 11, 64), (2, 9, 11, 65), (1, 8, 8, 100), (1, 5, 6, 256))
PENALTIES = ((0, 0), (32, 256), (300, 300), (4095, 4095))
BENEFIT_P1, BENEFIT_P2, BENEFIT_SCALE = 32, 256, 32.0        # 1 and 8 grey levels at 32 units per grey level
BENEFIT_MARGIN = 0.05
QUANTISATION_MARGIN = 0.01


def quantise(C, cost_scale):
    """q = min(4095, (int)floorf(C cost_scale + 0.5f)) with the product and the sum rounded to float32 one after the other; NaN -> 4095"""
    C = np.asarray(C, np.float32)
    with np.errstate(all="ignore"):
        v = np.floor(C * np.float32(cost_scale) + np.float32(0.5))
        q = np.where(v < np.float32(COST_MAX), np.maximum(v, np.float32(0)), np.float32(COST_MAX))
    assert v.dtype == np.float32
    return q.astype(np.uint16)


def _recur(C, Lq, has_pred, P1, P2):
    """one step of the recurrence: C, Lq int64 [..., D]; has_pred bool [...]"""
    far = np.int64(1) << 40
    m = Lq.min(-1, keepdims=True)
    pad = np.full(Lq.shape[:-1] + (1,), far, np.int64)
    lo = np.concatenate([pad, Lq[..., :-1]], -1) + P1
    hi = np.concatenate([Lq[..., 1:], pad], -1) + P1
    best = np.minimum(np.minimum(Lq, lo), np.minimum(hi, m + P2))
    return np.where(has_pred[..., None], C + best - m, C)


def path_costs_ref(cost, P1, P2, direction):
    """L_r of one direction r = (dx, dy): cost [N,H,W,D] -> int64 [N,H,W,D]"""
    C = np.asarray(cost).astype(np.int64)
    N, H, W, D = C.shape
    dx, dy = direction
    L = np.zeros_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for x in xs:
            q = x - dx
            ok = 0 <= q < W
            L[:, :, x] = _recur(C[:, :, x], L[:, :, q] if ok else C[:, :, x], np.full((N, H), ok), P1, P2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for y in ys:
        qy = y - dy
        qx = np.arange(W) - dx
        ok = (0 <= qy < H) & (qx >= 0) & (qx < W)
        Lq = L[:, qy if 0 <= qy < H else y][:, np.clip(qx, 0, W - 1)]
        L[:, y] = _recur(C[:, y], Lq, np.broadcast_to(ok, (N, W)), P1, P2)
    return L


def sgm_aggregate_ref(cost, P1, P2, paths):
    """cost uint16 [N,H,W,D] -> agg int64 [N,H,W,D] = the sum over the first `paths` directions of L_r"""
    assert paths in (4, 8) and 0 <= P1 <= P2 <= COST_MAX
    return sum(path_costs_ref(cost, P1, P2, d) for d in DIRECTIONS[:paths])


def sgm_select_ref(agg, inv, n_present):
    """agg [N,H,W,D] (any integer type), inv float32 [N,D] of those views, n_present int [N] -> (out = 1 / inverse, conf, winner,
    winner cost), float32 [N,H,W] (winner int64): every operation in float32, in the header's order"""
    f32 = np.float32
    agg = np.asarray(agg)
    N, H, W, D = agg.shape
    inv = np.asarray(inv, f32)
    out, conf, win, cost = (np.zeros((N, H, W), f32), np.zeros((N, H, W), f32), np.zeros((N, H, W), np.int64), np.zeros((N, H, W), f32))
    for n in range(N):
        S = np.ascontiguousarray(agg[n].astype(f32).transpose(2, 0, 1))
        k = R.winner_ref(S)
        off, _, _ = R.parabola_offset(S, k)
        iv = R.inverse_depth_at(inv[n], k, off.astype(f32))
        c, _ = R.confidence_ref(S, k, n_present[n])
        assert off.dtype == f32 and iv.dtype == f32 and c.dtype == f32
        with np.errstate(all="ignore"):
            out[n] = f32(1) / iv
        conf[n], win[n], cost[n] = c, k, np.take_along_axis(S, k[None], 0)[0]
    return out, conf, win, cost


class WeakScene(R.BoxScene):
    """BoxScene with the texture at 20 % of its amplitude around mid grey: walls with little to match on"""

    def texture(self, P):
        return 128.0 + 0.2 * (super().texture(P) - 128.0)


def weak_scene():
    return WeakScene()


def noisy(grey):
    """+-3 grey levels of uniform noise, the same for every caller"""
    noise = np.random.default_rng(7).integers(-3, 4, grey.shape)
    return np.clip(grey.astype(np.int64) + noise, 0, 255).astype(np.uint8)


def share_within(out, truth, step, limit=1.5):
    """the share of ALL pixels whose inverse depth (or distance) is within `limit` hypothesis steps of the truth; step [F]"""
    with np.errstate(all="ignore"):
        err = np.abs(1.0 / np.asarray(out, np.float64) - 1.0 / truth) / np.abs(np.asarray(step))[:, None, None]
    return float((err <= limit).mean())


_cache = {}


def plane_benefit_case():
    """F = 5, 48 x 64, S = 4, D = 32, r = 1 on weak_scene() + noisy, with the float32 cost volume C32 [F,D,H,W]; computed once"""
    if "plane" not in _cache:
        c = R.sweep_case(F=5, H=48, W=64, S=4, D=32, r=1, scene=weak_scene())
        c.grey = noisy(c.grey)
        c.C32, _ = R.cost_volume(c.grey, c.homographies, c.src_index, c.r, c.oob, np.float32)
        c.C32.setflags(write=False)
        c.truth, c.inv, c.step = c.true_depth, c.inv_depth, np.diff(c.setup.inv_depth, axis=1)[:, 0]
        _cache["plane"] = c
    return _cache["plane"]


def sphere_benefit_case():
    """F = 5, 48 x 96, S = 4, D = 32, r = 1 on weak_scene() + noisy, with the float32 cost volume C32 [F,D,He,We]; computed once"""
    if "sphere" not in _cache:
        c = RS.sphere_case(F=5, He=48, We=96, S=4, D=32, r=1, scene=weak_scene())
        c.grey = noisy(c.grey)
        c.C32, _ = RS.cost_volume(c.grey, c.rel_pose, c.src_index, c.inv_dist, c.r, np.float32)
        c.C32.setflags(write=False)
        c.truth, c.inv, c.step = c.true_dist, c.inv_dist, np.diff(c.setup.inv_dist, axis=1)[:, 0]
        _cache["sphere"] = c
    return _cache["sphere"]


def benefit_shares(c, paths=4):
    """-> (winner-take-all share on the float32 costs, the same on the quantised costs, share after SGM) of a benefit case"""
    n_present = R.present(c.src_index, c.F).sum(1)
    wta = np.stack([R.sweep_ref(c.C32[f], c.inv[f], n_present[f])[0] for f in range(c.F)])
    q = quantise(c.C32, BENEFIT_SCALE).transpose(0, 2, 3, 1)
    wta_q = sgm_select_ref(q, c.inv, n_present)[0]
    sgm = sgm_select_ref(sgm_aggregate_ref(q, BENEFIT_P1, BENEFIT_P2, paths), c.inv, n_present)[0]
    return share_within(wta, c.truth, c.step), share_within(wta_q, c.truth, c.step), share_within(sgm, c.truth, c.step)
