"""-m gpu: the ZNCC matching cost of the two sweeps on the device (csrc/mvs_zncc.hip, evoworld_amd/mvs.py) against the
numpy oracle of tests/mvs_zncc_ref.py.  Cost tolerance: Z.COST_TOL[kind] = twice the float32-order margin that tests/test_cpu_mvs_zncc.py
measures on these very inputs, in percent of cost; (pixel, hypothesis) pairs whose window holds a tap that may fall on either side of a
source's border or centre are left out (at most 0.5 %).  Every case is at most 5 views of 48 x 96."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvs_ref as R  # noqa: E402
import mvs_sgm_ref as G  # noqa: E402
import mvs_sphere_ref as S  # noqa: E402
import mvs_zncc_ref as Z  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = {torch.float32: -777.25, torch.int32: -777, torch.uint16: 0x5A5A}
PAD = 4096
SCALE = Z.COST_SCALE
KINDS = [("plane", kw) for kw in Z.PLANE_CASES] + [("sphere", kw) for kw in Z.SPHERE_CASES]
KIND_IDS = [f"{kind}-{Z.case_id(kw)}" for kind, kw in KINDS]


class Guarded:
    """`view` of the given shape in the middle of a buffer filled with a pattern; check() asserts the bands either side still hold it.
    A uint16 buffer is allocated, filled and compared as int16 (the same bits)."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        raw = torch.int16 if dtype == torch.uint16 else dtype
        self.buf = torch.full((PAD + n + PAD,), FILL[dtype], dtype=raw, device=DEV)
        self.view = self.buf[PAD:PAD + n].view(dtype).view(shape)
        self.n, self.fill = n, FILL[dtype]

    def check(self):
        assert bool((self.buf[:PAD] == self.fill).all()), "guard band in front of the output was written"
        assert bool((self.buf[PAD + self.n:] == self.fill).all()), "guard band behind the output was written"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tables(kind, c):
    """the device inputs of a case in the entries' order: (grey, homographies | rel_pose, src_index, inv)"""
    if kind == "plane":
        return _dev(c.grey), _dev(c.homographies), _dev(c.src_index), _dev(c.inv_depth)
    return _dev(c.grey), _dev(c.rel_pose), _dev(c.src_index), _dev(c.inv_dist)


def _fused(kind, c, tables=None, out=None, var_floor=Z.VAR_FLOOR, oob=Z.OOB_COST):
    from evoworld_amd import ops
    t = tables or _tables(kind, c)
    if kind == "plane":
        return ops.mvs_plane_sweep_zncc(*t, c.r, oob, var_floor, out=out)
    return ops.mvs_sphere_sweep_zncc(*t, c.r, var_floor, out=out)


def _volume(kind, c, tables, b=0, m=None, out=None, scale=SCALE):
    from evoworld_amd import ops
    if kind == "plane":
        return ops.mvs_plane_sweep_zncc_volume(*tables, c.r, Z.OOB_COST, Z.VAR_FLOOR, scale, b, m, out=out)
    return ops.mvs_sphere_sweep_zncc_volume(*tables, c.r, Z.VAR_FLOOR, scale, b, m, out=out)


def _sweep(kind, c, guarded=False):
    shape = (c.F, c.H, c.W)
    g = [Guarded(shape, dt) for dt in (torch.float32, torch.float32, torch.int32, torch.float32)] if guarded else None
    out = _fused(kind, c, out=[x.view for x in g] if g else None)
    torch.cuda.synchronize()
    for x in g or ():
        x.check()
    return [o.cpu().numpy() for o in out]


# ------------------------------------------------------------------ the fused entries against the oracle
@pytest.mark.parametrize("kind,kw", KINDS, ids=KIND_IDS)
def test_fused_sweep_matches_the_float64_oracle(kind, kw):
    c, C64, ambiguous = Z.cached(kind, **kw)
    tol = Z.COST_TOL[kind]
    depth, conf, win, cost = _sweep(kind, c, guarded=True)
    again = _sweep(kind, c)
    for a, b in zip((depth, conf, win, cost), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ"
    assert float(ambiguous.mean()) <= Z.MAX_AMBIGUOUS_SHARE
    assert win.min() >= 0 and win.max() < c.D and np.isfinite(depth).all() and np.isfinite(cost).all()
    n_present = R.present(c.src_index, c.F).sum(1)
    inv32 = Z.truth_and_tables(kind, c)[1]
    worst_cost = worst_regret = 0.0
    for f in range(c.F):
        C, amb, k = C64[f], ambiguous[f], win[f].astype(np.int64)
        if n_present[f] == 0:                             # no source: every cost 0, hypothesis 0, no confidence
            assert (k == 0).all() and (cost[f] == 0).all() and (conf[f] == 0).all()
            assert np.array_equal(depth[f], np.full_like(depth[f], np.float32(1) / inv32[f, 0]))
            continue
        at = lambda A, kk: np.take_along_axis(A, kk[None], 0)[0]
        clear = ~at(amb, k)
        d_cost = np.abs(cost[f].astype(np.float64) - at(C, k))[clear]
        regret = (at(C, k) - np.where(amb, np.inf, C).min(0))[clear]
        worst_cost, worst_regret = max(worst_cost, float(d_cost.max())), max(worst_regret, float(regret.max()))
        assert d_cost.max() <= tol, f"view {f}: winner cost off by {d_cost.max():.3e} (tolerance {tol:.1e})"
        assert regret.max() <= tol, f"view {f}: the device's winner costs {regret.max():.3e} more than the best hypothesis (tolerance {tol:.1e})"
        # depth: the parabola rule on the float64 costs around the device's winner, the tolerance carried through the rule
        inner = (k > 0) & (k < c.D - 1)
        clear3 = clear & ~at(amb, np.maximum(k - 1, 0)) & ~at(amb, np.minimum(k + 1, c.D - 1))
        off, _, curv = R.parabola_offset(C, k)
        num = np.abs(at(C, np.maximum(k - 1, 0)) - at(C, np.minimum(k + 1, c.D - 1)))
        inv_dev = 1.0 / depth[f].astype(np.float64)
        base = inv32[f].astype(np.float64)[k]
        step = float(np.abs(np.diff(inv32[f].astype(np.float64))).max()) if c.D > 1 else 0.0
        exact = ~inner | (curv < -4 * tol)                # the rule gives no refinement, whatever the last bits of the costs
        assert np.array_equal(depth[f][exact & clear3], (np.float32(1) / inv32[f][k])[exact & clear3])
        sure = inner & (curv > 4 * tol) & clear3          # refined on both sides: |d off| <= (tol curv + 2 tol |cl - cr|) / (curv (curv - 4 tol))
        with np.errstate(all="ignore"):
            d_off = np.where(sure, (tol * curv + 2 * tol * num) / (curv * (curv - 4 * tol)), 0.0) + 1e-5
        want = base + off * np.sign(np.diff(inv32[f].astype(np.float64)).mean() if c.D > 1 else 1.0) * step
        assert (np.abs(inv_dev - want)[sure] <= (d_off * step + 4e-6 * base)[sure]).all(), f"view {f}: refined depth"
        unsure = inner & ~sure & ~exact & clear3          # convexity hangs on the last bits: anywhere within half a step
        assert (np.abs(inv_dev - base)[unsure] <= 0.5 * step * (1 + 1e-5) + 4e-6 * base[unsure]).all()
        # confidence: 0 exactly where the rules say 0; elsewhere the rule's value
        far = np.abs(np.arange(c.D)[:, None, None] - k[None]) > 1
        none = ~far.any(0)
        assert (conf[f][none] == 0).all()
        c64, has = R.confidence_ref(C, k, n_present[f])
        c2 = np.where(far, C, np.inf).min(0)
        ok = has & ~amb.any(0) & (c2 > 1.0)
        assert (np.abs(conf[f] - c64)[ok] <= (3 * tol / c2 + 1e-5)[ok]).all(), f"view {f}: confidence"
        assert (conf[f] >= 0).all() and (conf[f] <= 1).all()
    print(f"{kind} {c.id}: winner cost within {worst_cost:.3e}, regret {worst_regret:.3e} (tolerance {tol:.1e}); "
          f"ambiguous pairs left out {float(ambiguous.mean()):.5f}")


@pytest.mark.parametrize("kind", ["plane", "sphere"])
@pytest.mark.parametrize("view", [0, 2, 4])
def test_a_view_does_not_depend_on_the_rest_of_the_batch(kind, view):
    """View i of the F = 5 call against a call that holds only it and its sources: bit-identical."""
    c = R.cached_case(**R.RECOVERY_CASE) if kind == "plane" else S.cached_case(**S.RECOVERY_CASE)
    full = _sweep(kind, c)
    sub = [view] + [int(s) for s in c.src_index[view] if s >= 0]
    one = SimpleNamespace(F=len(sub), H=c.H, W=c.W, r=c.r, grey=c.grey[sub], src_index=np.full((len(sub), c.S), -1, np.int32))
    if kind == "plane":
        one.homographies, one.inv_depth = c.homographies[sub].copy(), c.inv_depth[sub].copy()
    else:
        one.rel_pose, one.inv_dist = c.rel_pose[sub].copy(), c.inv_dist[sub].copy()
    remap = {v: i for i, v in enumerate(sub)}
    one.src_index[0] = [remap.get(int(s), -1) for s in c.src_index[view]]
    alone = _sweep(kind, one)
    for a, b, name in zip(full, alone, ("depth", "conf", "winner", "cost")):
        assert np.array_equal(a[view].view(np.int32), b[0].view(np.int32)), name


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_a_flat_image_costs_100_everywhere(kind):
    """Grey level 128 everywhere: a = 0 exactly, so cov = 0 exactly whatever the last bit of a blend, and every cost is exactly 100 --
    winner 0, confidence 0, nothing non-finite.  (Plane: a window that leaves a source costs oob_cost = 100 as well.)"""
    c = R.cached_case(**R.RECOVERY_CASE) if kind == "plane" else S.cached_case(**S.RECOVERY_CASE)
    flat = SimpleNamespace(**{**vars(c), "grey": np.full_like(c.grey, 128)})
    depth, conf, win, cost = _sweep(kind, flat)
    assert (cost == 100).all() and (win == 0).all() and (conf == 0).all() and np.isfinite(depth).all()
    out = _fused(kind, flat, var_floor=0.0)                 # without a floor the correlation is 0 / 0: defined as 0, never a NaN
    assert all(bool(torch.isfinite(o.float()).all()) for o in out) and bool((out[3] == 100).all())


# ------------------------------------------------------------------ the volume entries
@pytest.mark.parametrize("kind,kw", KINDS, ids=KIND_IDS)
def test_volume_is_the_fused_sweeps_cost_quantised(kind, kw):
    """The way tests/test_gpu_mvs_sgm.py checks the SAD volumes: within the tolerance (x scale, + 0.5 for the rounding) of the float64
    oracle, 0 for a view without a source, bit-equal to the fused entry's quantised winner cost at its winner, and a middle range of views
    written alone equal to the full call's."""
    c, C64, ambiguous = Z.cached(kind, **kw)
    tables = _tables(kind, c)
    g = Guarded((c.F, c.H, c.W, c.D), torch.uint16)
    q = _volume(kind, c, tables, 0, c.F, g.view)
    torch.cuda.synchronize()
    g.check()
    q = q.cpu().numpy()
    assert q.max() <= 200 * SCALE + 1 <= G.COST_MAX
    qd = q.transpose(0, 3, 1, 2).astype(np.float64)         # [F,D,H,W] like the oracle's
    bound = Z.COST_TOL[kind] * SCALE + 0.5
    err = np.abs(qd - C64 * SCALE)
    assert (err[~ambiguous] <= bound).all(), f"{c.id}: quantised cost off by {err[~ambiguous].max():.4f} (bound {bound:.4f})"
    n_present = R.present(c.src_index, c.F).sum(1)
    for f in np.flatnonzero(n_present == 0):
        assert (q[f] == 0).all(), "a view without a present source stores 0 everywhere"
    _, _, win, wcost = [o.cpu().numpy() for o in _fused(kind, c, tables)]
    at = np.take_along_axis(q, win[..., None].astype(np.int64), axis=3)[..., 0]
    assert np.array_equal(at, G.quantise(wcost, SCALE)), f"{c.id}: the volume at the fused winner is not its quantised cost"
    if kw.get("push_out"):                                   # windows that leave every present source cost oob_cost exactly
        _, _, _, vb = Z.zncc_volume(kind, c, with_variances=True)
        lost = np.isinf(vb) & (n_present > 0)[:, None, None, None] & ~ambiguous
        assert lost.mean() > 0.1 and (qd[lost] == Z.OOB_COST * SCALE).all()
    b, m = (1, c.F - 2) if c.F >= 3 else (1, 1)
    gm = Guarded((m, c.H, c.W, c.D), torch.uint16)
    part = _volume(kind, c, tables, b, m, gm.view)
    torch.cuda.synchronize()
    gm.check()
    assert np.array_equal(part.cpu().numpy(), q[b:b + m]), f"{c.id}: views {b} .. {b + m - 1} alone differ from the full call"
    print(f"{kind} {c.id}: quantised costs within {float(err[~ambiguous].max()):.4f} of C64 x {SCALE:g} (bound {bound:.4f})")


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_volume_with_more_hypotheses_than_one_flush_of_the_staging_holds(kind):
    """D = 65: two full flushes of 32 and a last one of a single hypothesis; against single-hypothesis volumes either side of every flush
    and against the fused sweep's winner."""
    c = R.sweep_case(F=3, H=37, W=53, S=2, D=65, r=1) if kind == "plane" else S.sphere_case(F=3, He=20, We=40, S=2, D=65, r=1)
    tables = _tables(kind, c)
    g = Guarded((c.F, c.H, c.W, c.D), torch.uint16)
    q = _volume(kind, c, tables, out=g.view)
    torch.cuda.synchronize()
    g.check()
    q = q.cpu().numpy()
    grey, warp, src, inv = tables
    for k in (0, 31, 32, 63, 64):                            # the cost of a hypothesis does not depend on the others
        one = (grey, warp[:, :, k:k + 1].contiguous() if kind == "plane" else warp, src, inv[:, k:k + 1].contiguous())
        assert np.array_equal(_volume(kind, c, one).cpu().numpy()[..., 0], q[..., k]), k
    _, _, win, wcost = [o.cpu().numpy() for o in _fused(kind, c, tables)]
    assert np.array_equal(np.take_along_axis(q, win[..., None].astype(np.int64), axis=3)[..., 0], G.quantise(wcost, SCALE))


# ------------------------------------------------------------------ argument checks
def test_argument_checks_of_the_wrappers_and_of_the_entries():
    from evoworld_amd import _lib, ops
    P = ops._ptr
    cp = R.cached_case(**Z.PLANE_R0)                         # r = 0: used only for the refusal
    cs = S.cached_case(**Z.SPHERE_R0)
    for kind, c0 in (("plane", cp), ("sphere", cs)):
        t = _tables(kind, c0)
        with pytest.raises(ValueError, match="patch_radius"):
            _fused(kind, c0, t)
        with pytest.raises(ValueError, match="patch_radius"):
            _volume(kind, c0, t)
    c = R.cached_case(**Z.PLANE_CASES[5])                    # 8 x 8, F = 2, D = 32, r = 2
    g, hm, si, iv = t = _tables("plane", c)
    outs = [torch.empty(c.F, c.H, c.W, dtype=dt, device=DEV) for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]
    vol = torch.empty((c.F, c.H, c.W, c.D), dtype=torch.uint16, device=DEV)
    for bad in (dict(var_floor=-1.0), dict(var_floor=float("nan")), dict(var_floor=float("inf")), dict(patch_radius=4)):
        with pytest.raises(ValueError):
            ops.mvs_plane_sweep_zncc(g, hm, si, iv, **{"patch_radius": c.r, **bad})
        with pytest.raises(ValueError):
            ops.mvs_plane_sweep_zncc_volume(g, hm, si, iv, **{"patch_radius": c.r, **bad})
    for bad in (dict(cost_scale=0.0), dict(cost_scale=float("nan")), dict(view_begin=2), dict(view_begin=1, n_views=2), dict(n_views=0)):
        with pytest.raises(ValueError):
            ops.mvs_plane_sweep_zncc_volume(g, hm, si, iv, **{"patch_radius": c.r, **bad})
    with pytest.raises(TypeError):
        ops.mvs_plane_sweep_zncc(g.float(), hm, si, iv, c.r)
    with pytest.raises(TypeError):
        ops.mvs_plane_sweep_zncc(g, hm.double(), si, iv, c.r)
    with pytest.raises(TypeError):
        ops.mvs_plane_sweep_zncc(g, hm, si.long(), iv, c.r)
    with pytest.raises(ValueError):
        ops.mvs_plane_sweep_zncc(g, hm[:, :, :5].contiguous(), si, iv, c.r)
    with pytest.raises(ValueError):
        ops.mvs_plane_sweep_zncc(g, hm, si, iv, c.r, out=[torch.empty(1, device=DEV)] * 4)
    with pytest.raises(ValueError):
        ops.mvs_plane_sweep_zncc_volume(g, hm, si, iv, c.r, out=vol[..., :4])
    with pytest.raises(TypeError):
        ops.mvs_plane_sweep_zncc_volume(g, hm, si, iv, c.r, out=vol.view(torch.int16))
    with pytest.raises(_lib.EvoWorldHipError, match="must live on the GPU"):
        ops.mvs_plane_sweep_zncc(g.cpu(), hm, si, iv, c.r)
    # the entries' own checks, behind the wrappers'
    for r, vf in ((0, 1.0), (4, 1.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(_lib.EvoWorldHipError):
            ops._call("ew_mvs_plane_sweep_zncc", P(g), P(hm), P(si), P(iv), *[P(o) for o in outs], c.F, c.H, c.W, c.S, c.D, r, 100.0, vf)
        with pytest.raises(_lib.EvoWorldHipError):
            ops._call("ew_mvs_plane_sweep_zncc_volume", P(g), P(hm), P(si), P(iv), P(vol), c.F, c.H, c.W, c.S, c.D, r, 100.0, vf, 16.0, 0, c.F)
    for scale, b, m in ((0.0, 0, 2), (float("inf"), 0, 2), (16.0, 1, 2), (16.0, -1, 1), (16.0, 0, 0)):
        with pytest.raises(_lib.EvoWorldHipError):
            ops._call("ew_mvs_plane_sweep_zncc_volume", P(g), P(hm), P(si), P(iv), P(vol), c.F, c.H, c.W, c.S, c.D, c.r, 100.0, 1.0, scale, b, m)
    c = S.cached_case(**Z.SPHERE_CASES[3])                   # 8 x 16, F = 2, D = 3, r = 3
    g, pose, si, iv = _tables("sphere", c)
    vol = torch.empty((c.F, c.H, c.W, c.D), dtype=torch.uint16, device=DEV)
    with pytest.raises(ValueError):
        ops.mvs_sphere_sweep_zncc(g[:, :, :5].contiguous(), pose, si, iv, 3)             # We = 5 < 2 x 3 + 1
    with pytest.raises(ValueError):
        ops.mvs_sphere_sweep_zncc(g, pose[:, :, :2].contiguous(), si, iv, 1)
    with pytest.raises(TypeError):
        ops.mvs_sphere_sweep_zncc(g, pose, si, iv.double(), 1)
    for bad in (dict(var_floor=-1.0), dict(patch_radius=4), dict(cost_scale=float("nan")), dict(view_begin=-1), dict(view_begin=1, n_views=2)):
        with pytest.raises(ValueError):
            ops.mvs_sphere_sweep_zncc_volume(g, pose, si, iv, **{"patch_radius": c.r, **bad})
    outs = [torch.empty(c.F, c.H, c.W, dtype=dt, device=DEV) for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]
    for r, vf, We in ((0, 1.0, c.W), (2, -1.0, c.W), (3, 1.0, 5)):
        with pytest.raises(_lib.EvoWorldHipError):
            ops._call("ew_mvs_sphere_sweep_zncc", P(g), P(pose), P(si), P(iv), *[P(o) for o in outs], c.F, c.H, We, c.S, c.D, r, vf)
        with pytest.raises(_lib.EvoWorldHipError):
            ops._call("ew_mvs_sphere_sweep_zncc_volume", P(g), P(pose), P(si), P(iv), P(vol), c.F, c.H, We, c.S, c.D, r, vf, 16.0, 0, c.F)
    with pytest.raises(_lib.EvoWorldHipError):
        ops._call("ew_mvs_sphere_sweep_zncc_volume", P(g), P(pose), P(si), P(iv), P(vol), c.F, c.H, c.W, c.S, c.D, c.r, 1.0, 16.0, 0, 3)


# ------------------------------------------------------------------ the stages
def _stage(kind, c, **kw):
    from evoworld_amd import mvs
    if kind == "plane":
        return mvs.PlaneSweepDepth(n_src=c.S, planes=c.D, patch_radius=c.r, oob_cost=c.oob, **kw), "view_w2c"
    return mvs.SphereSweepDepth(n_src=c.S, planes=c.D, patch_radius=c.r, **kw), "pano_w2c"


@pytest.mark.parametrize("kind", ["plane", "sphere"])
def test_stage_recovers_the_flickering_scene_and_the_default_is_untouched(kind):
    """RECOVERY_CASE under Z.flicker through the whole stage (the cross-view check off, as in the oracle's figure): the device's ZNCC share
    is at least the float64 oracle's - 0.01 (G.QUANTISATION_MARGIN) and at least the device's SAD share + 0.2; with aggregate='sgm' the
    result does not depend on the chunks of views; cost='sad' gives the bits of a call without the argument."""
    s = Z.recovery_shares(kind)
    c, truth = s["case"], Z.truth_and_tables(kind, s["case"])
    rgb = _dev(np.repeat(s["flickered"][..., None], 3, -1))

    def run(**kw):
        stage, pose = _stage(kind, c, **kw)
        return stage(rgb, **{pose: c.w2c})

    def share(p):
        return R.kept_and_correct(p["depth_conf"].cpu().numpy(), p["depth"][..., 0].cpu().numpy().astype(np.float64), truth[0], truth[2])[0]

    sad, zncc = share(run(min_consistent=0)), share(run(min_consistent=0, cost="zncc"))
    print(f"{kind} under flicker on the device: SAD {sad:.4f}, ZNCC {zncc:.4f} (float64 oracle: SAD {s['sad_flicker']:.4f}, ZNCC {s['zncc_flicker']:.4f})")
    assert zncc >= s["zncc_flicker"] - G.QUANTISATION_MARGIN
    assert zncc >= sad + 0.2
    plain, named = run(), run(cost="sad")
    full = run(cost="zncc")                                  # with the cross-view check, as the loop runs it
    assert set(plain) == set(named) == set(full)
    for k in plain:
        assert torch.equal(plain[k], named[k]), k
        assert full[k].dtype == plain[k].dtype and full[k].shape == plain[k].shape and full[k].is_cuda
    assert not torch.equal(full["depth"], plain["depth"])
    conf = full["depth_conf"].cpu().numpy()
    assert (conf >= 0).all() and (conf <= 1).all() and (conf > 0).any()
    sgm, sgm_one, sgm_sad = run(cost="zncc", aggregate="sgm"), run(cost="zncc", aggregate="sgm", workspace_bytes=1), run(aggregate="sgm")
    for k in sgm:
        assert torch.equal(sgm[k], sgm_one[k]), k
    assert not torch.equal(sgm["depth"], sgm_sad["depth"]) and not torch.equal(sgm["depth"], full["depth"])
    print(f"{kind} under flicker on the device, cost='zncc' + aggregate='sgm' (reported, not asserted): {share(run(min_consistent=0, cost='zncc', aggregate='sgm')):.4f}")


# ------------------------------------------------------------------ the episode and the command line
@pytest.fixture(scope="module")
def tiny():
    from evoworld_amd.pipeline import StableVideoDiffusionPipeline
    from evoworld_amd.unet import DEFAULT_CONFIG, UNetSpatioTemporalConditionModel, random_state_dict
    from oracle.unet_ref import tiny_config
    cfg = tiny_config()
    cfg["num_frames"] = 25
    sd = random_state_dict({**DEFAULT_CONFIG, **cfg}, 0)
    unet = UNetSpatioTemporalConditionModel(**cfg).load_state_dict(sd, device="cuda")
    return cfg, StableVideoDiffusionPipeline(unet=unet)


def test_episode_with_the_zncc_cost_and_the_default_untouched(tiny, tmp_path):
    """The tiny 2-segment synthetic episode of tests/test_gpu_mvs.py: the default loader, both sweep stages with the SAD cost and with
    mvs_cost='zncc', then the default loader again.  The ZNCC runs go through and render memory panoramas that differ from the SAD runs';
    the two default runs are bit-identical, frames and panoramas."""
    from PIL import Image
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.mvs import PlaneSweepDepth, SphereSweepDepth
    from evoworld_amd.stages import load_stages
    cfg, pipe = tiny
    H, W, T = 128, 256, 25
    i = np.arange(60, dtype=np.float64)
    cam = np.stack([0.04 * i * np.sin(i / 9), 0 * i, 0.04 * i * np.cos(i / 9), 0 * i, 95 + 3.6 * i, 0 * i], 1)
    start = (torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    saved = (pipe.vae, pipe.image_encoder, pipe.vae_scale_factor)

    def run(name, depth_stage, cost=None):
        args = SimpleNamespace(svd_path=None, mvs_planes=16, mvs_sources=2, mvs_cost=cost)
        st = load_stages(None, args, depth_stage=depth_stage, cross_attention_dim=cfg["cross_attention_dim"], camera_params=cam, depth_hw=(48, 64))
        assert isinstance(st.depth_model, PlaneSweepDepth) == (depth_stage == "mvs") and isinstance(st.depth_model, SphereSweepDepth) == (depth_stage == "mvs_pano")
        if depth_stage:
            assert st.depth_model.cost == (cost or "sad")
        pipe.set_components(vae=st.vae, image_encoder=st.image_encoder)
        loop = UnifiedLoopConsistencyPipeline(pipe, st.depth_model, height=H, width=W, num_frames=T, num_segments=2, num_inference_steps=1,
                                              pano_size=(64, 128), face_res=32)
        frames = loop.process_episode(start, cam, save_dir=str(tmp_path / name))
        d = tmp_path / name / "rendered_panorama_vggt_open3d_0"
        return frames, np.stack([np.asarray(Image.open(d / f"{k:02}.png")) for k in range(24)])

    try:
        f0, p0 = run("default_before", None)
        _, p_sad = run("mvs_sad", "mvs")
        f_z, p_z = run("mvs_zncc", "mvs", "zncc")
        _, q_sad = run("pano_sad", "mvs_pano")
        g_z, q_z = run("pano_zncc", "mvs_pano", "zncc")
        f1, p1 = run("default_after", None)
    finally:
        pipe.vae, pipe.image_encoder, pipe.vae_scale_factor = saved
    for f, p, sad in ((f_z, p_z, p_sad), (g_z, q_z, q_sad)):
        assert f.shape == (49, 3, H, W) and torch.isfinite(f).all()
        assert (p != 0).any(), "the ZNCC memory rendered nothing"
        assert not np.array_equal(p, sad), "the memory panoramas of the ZNCC run equal the SAD run's"
        assert not np.array_equal(p, p0)
    assert torch.equal(f0, f1) and np.array_equal(p0, p1)


def test_cloud_cli_with_zncc_writes_a_cloud_and_names_the_setting(tmp_path, capsys):
    import json
    from PIL import Image
    from evoworld_amd import mvs
    from evoworld_amd.geometry import UNITY_TO_OPENCV, xyz_euler_to_four_by_four_matrix_batch
    from evoworld_amd.memory import read_ply
    scene, cam, n = R.pose_scene(), R.POSE_CAM, 5
    c2w = xyz_euler_to_four_by_four_matrix_batch(torch.tensor(cam[:n]), relative=False).numpy()
    (tmp_path / "frames").mkdir()
    for i, p in enumerate(scene.render_panos(c2w, 128, 256)):
        Image.fromarray(p).save(tmp_path / "frames" / f"{i + 1:03}.png")
    with open(tmp_path / "camera_poses.txt", "w") as f:
        f.write("Frame,PosX,PosY,PosZ,RotX,RotY,RotZ\n")
        for i, row in enumerate(cam * np.asarray(UNITY_TO_OPENCV, np.float64)):
            f.write(",".join([str(i + 1)] + [repr(float(v)) for v in row]) + "\n")
    base = ["cloud", "--frames", str(tmp_path / "frames"), "--poses", str(tmp_path / "camera_poses.txt"), "--segment", "0", "--planes", "32",
            "--view_height", "48", "--view_width", "64"]
    out = tmp_path / "zncc.ply"
    mvs.main(base + ["--output", str(out), "--cost", "zncc"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (rec["cost"], rec["aggregate"], rec["stage"]) == ("zncc", "box", "plane")
    pts, _ = read_ply(str(out))
    assert rec["views"] == 5 and rec["points_out"] == len(pts) and 5 * 48 * 64 // 2 <= len(pts) <= 5 * 48 * 64
    first = np.linalg.inv(np.concatenate([mvs.view_poses(cam, n, 0, relative=False)[0], [[0, 0, 0, 1.0]]]))
    P = pts.astype(np.float64) @ first[:3, :3].T + first[:3, 3]
    z_far = mvs.sweep_setup(mvs.view_poses(cam, n, 0), mvs.pinhole(48, 64), 4, 32).z_far
    depth = np.linalg.norm(P - first[:3, 3], axis=1)
    share = float((scene.wall_distance(P) <= 1.5 / z_far.min() * depth ** 2).mean())
    print(f"cloud CLI --cost zncc: {len(pts)} points, {share:.4f} within 1.5 plane steps of a wall (reported, not asserted)")
    sad = tmp_path / "sad.ply"
    mvs.main(base + ["--output", str(sad)])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["cost"] == "sad" and not np.array_equal(read_ply(str(sad))[0], pts)
    sph = tmp_path / "sphere.ply"
    mvs.main(base[:9] + ["--stage", "sphere", "--sweep_size", "64", "128", "--cost", "zncc", "--aggregate", "sgm", "--output", str(sph)])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (rec["cost"], rec["aggregate"], rec["stage"]) == ("zncc", "sgm", "sphere")
    assert 5 * 64 * 128 // 2 <= rec["points_out"] == len(read_ply(str(sph))[0]) <= 5 * 64 * 128
