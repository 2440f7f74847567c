"""-m gpu: the semi-global aggregation of the sweeps' cost volume on the device (csrc/mvs_sgm.hip, the volume variants in csrc/mvs.hip
and csrc/mvs_sphere.hip, evoworld_amd/mvs.py) against the numpy oracle of tests/mvs_sgm_ref.py.  The aggregation is
integer arithmetic: agg, winner and winner cost must be EQUAL.  Depth and confidence are float32 operations in a fixed order, each
correctly rounded: equality is expected and 4 ulps are allowed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvs_ref as R  # noqa: E402
import mvs_sgm_ref as G  # noqa: E402
import mvs_sphere_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = {torch.float32: -777.25, torch.int32: -777, torch.uint16: 0x5A5A}
PAD = 4096
ULPS = 4
SCALE = 32.0


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


def _ulps(a, b):
    """the largest distance in float32 ulps between two arrays of finite values of equal sign"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (np.signbit(a) == np.signbit(b)).all()
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def _tables(N, D, seed):
    """inv fp32 [F,D] and src_index int32 [F,1] for a volume of the views 1 .. N of F = N + 1: every view has its one source present
    except, when there are two or more, the last"""
    rng = np.random.default_rng(seed)
    inv = np.sort(rng.uniform(0.02, 1.5, size=(N + 1, D)).astype(np.float32), axis=1)
    src = np.zeros((N + 1, 1), np.int32)
    src[0, 0] = 1
    if N >= 2:
        src[N, 0] = -1
    return inv, src


def _aggregate_and_select(cost, P1, P2, paths, inv, src):
    """device: guarded agg and the four guarded outputs of the select for the views 1 .. N"""
    from evoworld_amd import ops
    N, H, W, D = cost.shape
    ga = Guarded(cost.shape, torch.uint16)
    agg = ops.mvs_sgm_aggregate(_dev(cost), P1, P2, paths, out=ga.view)
    g = [Guarded((N, H, W), dt) for dt in (torch.float32, torch.float32, torch.int32, torch.float32)]
    out = ops.mvs_sgm_select(agg, _dev(inv), _dev(src), view_begin=1, out=[x.view for x in g])
    torch.cuda.synchronize()
    for x in [ga] + g:
        x.check()
    return agg.cpu().numpy(), [o.cpu().numpy() for o in out]


def _check_against_oracle(cost, P1, P2, paths, inv, src):
    agg, (depth, conf, win, wcost) = _aggregate_and_select(cost, P1, P2, paths, inv, src)
    want = G.sgm_aggregate_ref(cost, P1, P2, paths)
    assert want.max() <= 65520
    assert np.array_equal(agg.astype(np.int64), want), f"agg differs at P = ({P1}, {P2}), {paths} paths"
    n_present = R.present(src, len(src)).sum(1)[1:]
    d_ref, c_ref, k_ref, w_ref = G.sgm_select_ref(want, inv[1:], n_present)
    assert np.array_equal(win.astype(np.int64), k_ref), "winner"
    assert np.array_equal(wcost, w_ref), "winner cost"
    ud, uc = _ulps(depth, d_ref), _ulps(conf, c_ref)
    assert ud <= ULPS and uc <= ULPS, (ud, uc)
    assert (conf[n_present == 0] == 0).all()
    return ud, uc


# ------------------------------------------------------------------ ew_mvs_sgm_aggregate, ew_mvs_sgm_select against the oracle
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("shape", G.AGG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_aggregate_and_select_equal_the_oracle_on_random_volumes(shape, paths):
    N, H, W, D = shape
    rng = np.random.default_rng(sum(shape) + paths)
    cost = rng.integers(0, G.COST_MAX + 1, size=shape).astype(np.uint16)
    if D >= 3:
        cost[..., 1] = np.minimum(cost[..., 1], cost[..., 0])      # ties between neighbouring hypotheses occur
        cost[0, 0, 0, :] = 17                                     # and a pixel that is one tie throughout
    inv, src = _tables(N, D, 5)
    worst = (0, 0)
    for P1, P2 in G.PENALTIES:
        worst = tuple(max(a, b) for a, b in zip(worst, _check_against_oracle(cost, P1, P2, paths, inv, src)))
    print(f"{shape} {paths} paths: depth within {worst[0]} ulps, confidence within {worst[1]} ulps of the float32 restatement")


@pytest.mark.parametrize("level", [0, G.COST_MAX])
def test_aggregate_and_select_on_constant_volumes(level):
    """All 4095: with P2 = 4095 the largest value the recurrence can see; all 0: every hypothesis ties."""
    shape = (2, 9, 11, 65)
    cost = np.full(shape, level, np.uint16)
    inv, src = _tables(shape[0], shape[3], 6)
    for paths in (4, 8):
        for P1, P2 in G.PENALTIES:
            _check_against_oracle(cost, P1, P2, paths, inv, src)
    agg, (_, conf, win, wcost) = _aggregate_and_select(cost, G.COST_MAX, G.COST_MAX, 8, inv, src)
    assert (agg == 8 * level).all() and (win == 0).all() and (conf == 0).all() and (wcost == 8 * level).all()


def test_two_calls_agree_and_a_view_alone_equals_the_view_in_the_batch():
    shape = (3, 37, 53, 32)
    cost = np.random.default_rng(11).integers(0, G.COST_MAX + 1, size=shape).astype(np.uint16)
    inv, src = _tables(3, 32, 7)
    agg, outs = _aggregate_and_select(cost, 32, 256, 8, inv, src)
    agg2, outs2 = _aggregate_and_select(cost, 32, 256, 8, inv, src)
    assert np.array_equal(agg, agg2) and all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(outs, outs2))
    for v in range(3):
        inv1, src1 = np.stack([inv[0], inv[v + 1]]), np.stack([src[0], src[v + 1]])
        a1, o1 = _aggregate_and_select(cost[v:v + 1], 32, 256, 8, inv1, src1)
        assert np.array_equal(a1[0], agg[v]), f"view {v}: agg"
        for a, b, name in zip(o1, outs, ("depth", "conf", "winner", "cost")):
            assert np.array_equal(a[0].view(np.int32), b[v].view(np.int32)), f"view {v}: {name}"


def test_argument_checks_of_the_wrappers_and_of_the_entries():
    from evoworld_amd import _lib, ops
    vol = torch.zeros((2, 3, 4, 8), dtype=torch.uint16, device=DEV)
    inv, src = torch.ones(3, 8, device=DEV), torch.zeros(3, 1, dtype=torch.int32, device=DEV)
    for bad in ((5, 4, 4), (-1, 4, 4), (0, 4096, 4), (1, 2, 6)):
        with pytest.raises(ValueError):
            ops.mvs_sgm_aggregate(vol, *bad)
    with pytest.raises(TypeError):
        ops.mvs_sgm_aggregate(vol.view(torch.int16), 1, 2)
    with pytest.raises(ValueError):
        ops.mvs_sgm_aggregate(vol[..., ::2], 1, 2)                                      # not contiguous
    with pytest.raises(ValueError):
        ops.mvs_sgm_aggregate(vol, 1, 2, out=vol)                                       # in place
    with pytest.raises(ValueError):
        ops.mvs_sgm_aggregate(vol, 1, 2, out=torch.zeros((2, 3, 4, 9), dtype=torch.uint16, device=DEV))
    with pytest.raises(ValueError):
        ops.mvs_sgm_aggregate(torch.zeros((1, 1, 1, 257), dtype=torch.uint16, device=DEV), 1, 2)
    with pytest.raises(ValueError):
        ops.mvs_sgm_select(vol, inv[:, :7].contiguous(), src)                           # D of inv
    with pytest.raises(ValueError):
        ops.mvs_sgm_select(vol, inv, src, view_begin=2)                                 # views 2 .. 3 of F = 3
    with pytest.raises(TypeError):
        ops.mvs_sgm_select(vol, inv.double(), src)
    with pytest.raises(ValueError):
        ops.mvs_sgm_select(vol, inv, src, out=[torch.empty(1, device=DEV)] * 4)
    with pytest.raises(_lib.EvoWorldHipError):             # the entries' own checks, behind the wrappers'
        ops._call("ew_mvs_sgm_aggregate", ops._ptr(vol), ops._ptr(torch.empty_like(vol)), 2, 3, 4, 8, 5, 4, 4)
    with pytest.raises(_lib.EvoWorldHipError):
        ops._call("ew_mvs_sgm_aggregate", ops._ptr(vol), ops._ptr(torch.empty_like(vol)), 2, 3, 4, 257, 1, 2, 4)
    with pytest.raises(_lib.EvoWorldHipError):
        ops._call("ew_mvs_sgm_aggregate", ops._ptr(vol), ops._ptr(vol), 2, 3, 4, 8, 1, 2, 4)
    c = R.cached_case(**R.GPU_CASES[5])                    # 8 x 8, F = 2
    g, hm, si, iv = _dev(c.grey), _dev(c.homographies), _dev(c.src_index), _dev(c.inv_depth)
    for bad in (dict(cost_scale=0.0), dict(view_begin=2), dict(view_begin=1, n_views=2), dict(n_views=0), dict(patch_radius=4)):
        with pytest.raises(ValueError):
            ops.mvs_plane_sweep_volume(g, hm, si, iv, **{"patch_radius": c.r, **bad})
    with pytest.raises(ValueError):
        ops.mvs_plane_sweep_volume(g, hm, si, iv, c.r, out=torch.zeros((2, 8, 8, 4), dtype=torch.uint16, device=DEV))
    with pytest.raises(_lib.EvoWorldHipError):
        ops._call("ew_mvs_plane_sweep_volume", ops._ptr(g), ops._ptr(hm), ops._ptr(si), ops._ptr(iv), ops._ptr(vol), c.F, c.H, c.W, c.S, c.D, c.r,
                  48.0, 32.0, 1, 2)
    cs = S.cached_case(**S.GPU_CASES[4])                   # 8 x 16, F = 2
    g, pose, si, iv = _dev(cs.grey), _dev(cs.rel_pose), _dev(cs.src_index), _dev(cs.inv_dist)
    for bad in (dict(cost_scale=float("nan")), dict(view_begin=-1), dict(view_begin=1, n_views=2), dict(patch_radius=4)):
        with pytest.raises(ValueError):
            ops.mvs_sphere_sweep_volume(g, pose, si, iv, **{"patch_radius": cs.r, **bad})
    with pytest.raises(_lib.EvoWorldHipError):
        ops._call("ew_mvs_sphere_sweep_volume", ops._ptr(g), ops._ptr(pose), ops._ptr(si), ops._ptr(iv), ops._ptr(vol), cs.F, cs.H, cs.W, cs.S, cs.D,
                  cs.r, 32.0, 0, 3)


# ------------------------------------------------------------------ the volume kernels on the sweeps' own inputs
def _check_volume(c, tol, volume, fused):
    """volume(view_begin, n_views, out) -> device uint16 [n,H,W,D]; fused() -> the fused sweep's four outputs"""
    g = Guarded((c.F, c.H, c.W, c.D), torch.uint16)
    q = volume(0, c.F, g.view)
    torch.cuda.synchronize()
    g.check()
    q = q.cpu().numpy()
    assert q.max() <= G.COST_MAX
    assert float(c.ambiguous.mean()) <= 0.005
    qd = q.transpose(0, 3, 1, 2).astype(np.float64)         # [F,D,H,W] like the oracle's
    t = c.C64 * SCALE
    bound = tol * SCALE + 0.5
    clear = ~c.ambiguous
    below = qd < G.COST_MAX
    err = np.abs(qd - t)
    assert (err[clear & below] <= bound).all(), f"{c.id}: quantised cost off by {err[clear & below].max():.4f} (bound {bound:.4f})"
    assert (t[clear & ~below] >= G.COST_MAX - bound).all(), f"{c.id}: an entry is clipped at 4095 below 4095"
    n_present = R.present(c.src_index, c.F).sum(1)
    for f in np.flatnonzero(n_present == 0):
        assert (q[f] == 0).all(), "a view without a present source stores 0 everywhere"
    # one cost routine: the entry at the fused kernel's winner is the fused kernel's winner cost, quantised
    _, _, win, wcost = [o.cpu().numpy() for o in fused()]
    at = np.take_along_axis(q, win[..., None].astype(np.int64), axis=3)[..., 0]
    assert np.array_equal(at, G.quantise(wcost, SCALE)), f"{c.id}: the volume at the fused winner is not its quantised cost"
    # a middle range written alone
    b, m = (1, c.F - 2) if c.F >= 3 else (1, 1)
    gm = Guarded((m, c.H, c.W, c.D), torch.uint16)
    part = volume(b, m, gm.view)
    torch.cuda.synchronize()
    gm.check()
    assert np.array_equal(part.cpu().numpy(), q[b:b + m]), f"{c.id}: views {b} .. {b + m - 1} alone differ from the full call"
    worst = float(err[clear & below].max()) if (clear & below).any() else 0.0
    print(f"{c.id}: quantised costs within {worst:.4f} of C64 x {SCALE:g} (bound {bound:.4f}); clipped entries {int((~below).sum())}")


@pytest.mark.parametrize("kw", R.GPU_CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items() if k in "FHWSDr") + ("-out" if kw.get("push_out") else ""))
def test_plane_volume_is_the_fused_sweeps_cost_quantised(kw):
    from evoworld_amd import ops
    c = R.cached_case(**kw)
    grey, hm, src, inv = _dev(c.grey), _dev(c.homographies), _dev(c.src_index), _dev(c.inv_depth)
    _check_volume(c, R.COST_TOL, lambda b, m, out: ops.mvs_plane_sweep_volume(grey, hm, src, inv, c.r, c.oob, SCALE, b, m, out=out),
                  lambda: ops.mvs_plane_sweep(grey, hm, src, inv, c.r, c.oob))


@pytest.mark.parametrize("kw", S.GPU_CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items() if k in ("F", "He", "We", "S", "D", "r")) + ("-yaw" if kw.get("yaw_step") else ""))
def test_sphere_volume_is_the_fused_sweeps_cost_quantised(kw):
    from evoworld_amd import ops
    c = S.cached_case(**kw)
    grey, pose, src, inv = _dev(c.grey), _dev(c.rel_pose), _dev(c.src_index), _dev(c.inv_dist)
    _check_volume(c, S.COST_TOL, lambda b, m, out: ops.mvs_sphere_sweep_volume(grey, pose, src, inv, c.r, SCALE, b, m, out=out),
                  lambda: ops.mvs_sphere_sweep(grey, pose, src, inv, c.r))


def test_volume_with_more_planes_than_one_flush_of_the_staging_holds():
    """D = 100: the staged planes are written out several times and a last, partial time; against single-plane volumes either side of
    every power-of-two boundary a flush can fall on, and against the fused sweep's winner."""
    from evoworld_amd import mvs, ops
    c = R.sweep_case(F=3, H=37, W=53, S=2, D=100, r=1)
    grey, hm, src, inv = _dev(c.grey), _dev(c.homographies), _dev(c.src_index), _dev(c.inv_depth)
    g = Guarded((c.F, c.H, c.W, c.D), torch.uint16)
    q = ops.mvs_plane_sweep_volume(grey, hm, src, inv, c.r, c.oob, SCALE, out=g.view)
    torch.cuda.synchronize()
    g.check()
    q = q.cpu().numpy()
    # plane k of the volume = the single-plane volume of plane k (the cost of a plane does not depend on the others)
    for k in (0, 15, 16, 31, 32, 63, 64, 95, 96, 99):
        one = ops.mvs_plane_sweep_volume(grey, hm[:, :, k:k + 1].contiguous(), src, inv[:, k:k + 1].contiguous(), c.r, c.oob, SCALE).cpu().numpy()
        assert np.array_equal(one[..., 0], q[..., k]), k
    _, _, win, wcost = [o.cpu().numpy() for o in ops.mvs_plane_sweep(grey, hm, src, inv, c.r, c.oob)]
    assert np.array_equal(np.take_along_axis(q, win[..., None].astype(np.int64), axis=3)[..., 0], G.quantise(wcost, SCALE))
    assert mvs.PlaneSweepDepth(planes=100, aggregate="sgm").planes == 100


# ------------------------------------------------------------------ the classes
def _stage_runs(case):
    from evoworld_amd import mvs
    if case == "plane":
        c = G.plane_benefit_case()
        make = lambda **kw: mvs.PlaneSweepDepth(n_src=c.S, planes=c.D, patch_radius=c.r, oob_cost=c.oob, **kw)
        call = lambda stage, rgb: stage(rgb, view_w2c=c.w2c)
    else:
        c = G.sphere_benefit_case()
        make = lambda **kw: mvs.SphereSweepDepth(n_src=c.S, planes=c.D, patch_radius=c.r, **kw)
        call = lambda stage, rgb: stage(rgb, pano_w2c=c.w2c)
    rgb = _dev(np.repeat(c.grey[..., None], 3, -1))
    return c, make, lambda **kw: call(make(**kw), rgb)


@pytest.mark.parametrize("case", ["plane", "sphere"])
def test_stage_with_sgm_recovers_more_and_does_not_depend_on_the_chunks(case):
    """On weak_scene() + noisy the device's SGM share of all pixels within 1.5 hypothesis steps is at least the device's winner-take-all
    share + 0.05; one view per chunk gives the bits of one chunk; aggregate='box' gives the bits of a call without the argument."""
    c, make, run = _stage_runs(case)
    plain, box, sgm, sgm_one = run(), run(aggregate="box"), run(aggregate="sgm"), run(aggregate="sgm", workspace_bytes=1)
    assert set(plain) == set(box) == set(sgm)
    for k in plain:
        assert torch.equal(plain[k], box[k]), k
        assert torch.equal(sgm[k], sgm_one[k]), k
        assert sgm[k].dtype == plain[k].dtype and sgm[k].shape == plain[k].shape and sgm[k].is_cuda
    share = lambda p: G.share_within(p["depth"][..., 0].cpu().numpy(), c.truth, c.step)
    wta, got = share(plain), share(sgm)
    print(f"{case} on the device: winner-take-all {wta:.4f}, SGM {got:.4f}, gain {got - wta:+.4f}")
    assert got >= wta + G.BENEFIT_MARGIN
    conf = sgm["depth_conf"].cpu().numpy()
    assert (conf >= 0).all() and (conf <= 1).all() and (conf > 0).any()


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


def test_episode_with_sgm_and_the_default_untouched(tiny, tmp_path):
    """The tiny 2-segment synthetic episode of tests/test_gpu_mvs.py: the default loader, depth_stage='mvs' with the box winner, the same
    with aggregate='sgm', then the default again.  The SGM run goes through, writes its memory panoramas and they differ from the box
    run's; the two default runs are bit-identical, frames and panoramas."""
    from types import SimpleNamespace
    from PIL import Image
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.mvs import PlaneSweepDepth
    from evoworld_amd.stages import load_stages
    cfg, pipe = tiny
    H, W, T = 128, 256, 25
    i = np.arange(60, dtype=np.float64)
    cam = np.stack([0.04 * i * np.sin(i / 9), 0 * i, 0.04 * i * np.cos(i / 9), 0 * i, 95 + 3.6 * i, 0 * i], 1)
    start = (torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    saved = (pipe.vae, pipe.image_encoder, pipe.vae_scale_factor)

    def run(name, depth_stage, aggregate=None):
        args = SimpleNamespace(svd_path=None, mvs_planes=16, mvs_sources=2, mvs_aggregate=aggregate)
        st = load_stages(None, args, depth_stage=depth_stage, cross_attention_dim=cfg["cross_attention_dim"], camera_params=cam, depth_hw=(48, 64))
        assert isinstance(st.depth_model, PlaneSweepDepth) == (depth_stage == "mvs")
        if depth_stage == "mvs":
            assert st.depth_model.aggregate == (aggregate or "box")
        pipe.set_components(vae=st.vae, image_encoder=st.image_encoder)
        loop = UnifiedLoopConsistencyPipeline(pipe, st.depth_model, height=H, width=W, num_frames=T, num_segments=2, num_inference_steps=1,
                                              pano_size=(64, 128), face_res=32)
        frames = loop.process_episode(start, cam, save_dir=str(tmp_path / name))
        d = tmp_path / name / "rendered_panorama_vggt_open3d_0"
        return frames, np.stack([np.asarray(Image.open(d / f"{k:02}.png")) for k in range(24)])

    try:
        f0, p0 = run("default_before", None)
        f1, p1 = run("mvs_box", "mvs")
        f2, p2 = run("mvs_sgm", "mvs", "sgm")
        f3, p3 = run("default_after", None)
    finally:
        pipe.vae, pipe.image_encoder, pipe.vae_scale_factor = saved
    assert f2.shape == (49, 3, H, W) and torch.isfinite(f2).all()
    assert (p2 != 0).any(), "the SGM memory rendered nothing"
    assert not np.array_equal(p2, p1), "the memory panoramas of the SGM run equal the box run's"
    assert not np.array_equal(p2, p0)
    assert torch.equal(f0, f3) and np.array_equal(p0, p3)


def test_cloud_cli_with_sgm_writes_a_cloud_and_names_the_setting(tmp_path, capsys):
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
    out = tmp_path / "sgm.ply"
    mvs.main(base + ["--output", str(out), "--aggregate", "sgm", "--sgm_p1", "0.5", "--sgm_p2", "6", "--sgm_paths", "8"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (rec["aggregate"], rec["sgm_p1"], rec["sgm_p2"], rec["sgm_paths"], rec["stage"]) == ("sgm", 0.5, 6.0, 8, "plane")
    pts, _ = read_ply(str(out))
    assert rec["views"] == 5 and rec["points_out"] == len(pts) and 5 * 48 * 64 // 2 <= len(pts) <= 5 * 48 * 64
    first = np.linalg.inv(np.concatenate([mvs.view_poses(cam, n, 0, relative=False)[0], [[0, 0, 0, 1.0]]]))
    P = pts.astype(np.float64) @ first[:3, :3].T + first[:3, 3]
    z_far = mvs.sweep_setup(mvs.view_poses(cam, n, 0), mvs.pinhole(48, 64), 4, 32).z_far
    depth = np.linalg.norm(P - first[:3, 3], axis=1)
    share = float((scene.wall_distance(P) <= 1.5 / z_far.min() * depth ** 2).mean())
    print(f"cloud CLI --aggregate sgm: {len(pts)} points, {share:.4f} within 1.5 plane steps of a wall (reported, not asserted)")
    box = tmp_path / "box.ply"
    mvs.main(base + ["--output", str(box)])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["aggregate"] == "box" and not np.array_equal(read_ply(str(box))[0], pts)
    sph = tmp_path / "sphere.ply"
    mvs.main(base[:9] + ["--stage", "sphere", "--sweep_size", "64", "128", "--aggregate", "sgm", "--output", str(sph)])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (rec["aggregate"], rec["stage"]) == ("sgm", "sphere") and 5 * 64 * 128 // 2 <= rec["points_out"] == len(read_ply(str(sph))[0]) <= 5 * 64 * 128
