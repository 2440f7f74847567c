"""-m gpu: the point-cloud kernels of the reprojection stage at the sizes and edges the product runs, bit for bit against
references that need no GPU (numpy boolean masks, np.sort, oracle/reproject_ref.py).

What each test pins (kernel path in brackets):
- test_filter_compact_scale: ew_filter_compact beyond one scan chunk [compact_scan_kernel's chunk loop and `carry`: nblk =
  ceil(n / 2048) is 1024 (one full chunk), 1025 (first block of the second), 2049 (third chunk, ragged last block) and 1860
  (product, 25 x 294 x 518 points)], with keep-all, keep-none (*total == 0, nothing written), "late" / "early" clouds whose kept
  rows are placed by the carry alone, ties at the threshold, both image layouts, rows past *total untouched, top RGBX byte 0.
- test_select_kth_*: ew_select_kth_f32 at the product n, on all-equal and two-valued arrays (degenerate histogram passes) and
  with +-inf / +-FLT_MAX; the percentile threshold against np.percentile at the product n.
- test_splat_*: ew_splat_cubemap + ew_splat_resolve against splat_ref, zbuf and faces guarded [splat_kernel's grid-stride loop
  (n > 1 048 576) and its cnt < 4 tail, zfill_kernel's odd cell, resolve_kernel's npix % 4 tail, all four <CI, CO>
  instantiations, same-depth ties (lowest index wins), non-finite and pixel-border coordinates].
- test_cube2equi_product_channels: ew_cube2equi_gather with 4-channel faces at 2000 x 1000 x 512 [cube2equi_kernel<4>, dword path].
Outputs live in Guarded buffers, workspaces are prefilled too, and every call runs with both prefill patterns."""
import ctypes

import numpy as np
import pytest
import torch

from kernel_checks import Guarded, assert_same_bits, fill_pattern
from oracle import reproject_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_PRODUCT = 25 * 294 * 518                            # 3 807 300 points: 25 frames of a 294 x 518 VGGT map
N_LATE = 2_100_000                                    # > 1024 blocks x 2048 points: past the first scan chunk


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ ew_filter_compact
def _conf(n, kind, rng):
    """(conf float32 [n], thr): the pattern decides what is kept"""
    f32 = np.float32
    conf, thr = rng.random(n, dtype=f32), 0.5
    if kind == "late":                                # nothing kept in the first scan chunk: every kept row's position is the carry
        conf[:N_LATE] *= f32(0.49)
        conf[N_LATE:] = conf[N_LATE:] * f32(0.49) + f32(0.51)
    elif kind == "early":
        conf[:N_LATE] = conf[:N_LATE] * f32(0.49) + f32(0.51)
        conf[N_LATE:] *= f32(0.49)
    elif kind == "keep_all":
        thr = -np.inf
    elif kind == "keep_none":
        thr = float(np.nextafter(conf.max(), f32(np.inf)))
    elif kind == "ties":                              # a ninth of the points sit exactly on the threshold: >= keeps them
        conf = (rng.integers(0, 9, size=n) / 8.0).astype(f32)
    else:
        assert kind == "uniform"
    return conf, thr


_FC = [(2048 * 1024, "uniform", 0), (2048 * 1024, "keep_all", 0), (2048 * 1024 + 1, "uniform", 0), (2048 * 1024 + 1, "keep_none", 0),
       (2048 * 2048 + 7, "uniform", 0), (2048 * 2048 + 7, "late", 0), (2048 * 2048 + 7, "early", 0), (2048 * 2048 + 7, "ties", 0)]
_FC += [(N_PRODUCT, kind, 1) for kind in ("uniform", "late", "early", "keep_all", "keep_none", "ties")]
_FC += [(N_PRODUCT, "uniform", 0), (N_PRODUCT, "late", 0)]


@pytest.mark.parametrize("n,kind,nchw", _FC, ids=[f"{n}-{k}-{'nchw' if c else 'nhwc'}" for n, k, c in _FC])
def test_filter_compact_scale(n, kind, nchw):
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    nblk = (n + 2047) // 2048
    assert nblk > 1024 or n == 2048 * 1024
    rng = np.random.default_rng(n % 1000 + len(kind))
    conf, thr = _conf(n, kind, rng)
    xyz = rng.standard_normal((n, 3), dtype=np.float32)
    hw = 294 * 518 if nchw else 0
    img = rng.random((n, 3), dtype=np.float32)                                 # NHWC order: the reference's
    img[::1001] = np.float32(1.0)
    img[5::1003] = np.float32(0.0)
    keep = conf >= np.float32(thr)
    m = int(keep.sum())
    assert {"keep_all": m == n, "keep_none": m == 0}.get(kind, 0 < m < n)
    if kind in ("late", "early"):
        assert keep[:N_LATE].all() == (kind == "early") and keep[N_LATE:].all() == (kind == "late") and keep[:N_LATE].any() == (kind == "early")
    want_xyz, want_rgb = xyz[keep], (img * 255).astype(np.uint8)[keep]
    img_dev = img.reshape(-1, hw, 3).transpose(0, 2, 1) if nchw else img       # [S,3,hw] planes
    d_conf, d_xyz, d_img = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (conf, xyz, img_dev))
    ws_bytes = lib.ew_filter_compact_workspace_bytes(n)
    assert ws_bytes >= (nblk + 1) * 4
    outs = []
    for k in (0, 1):
        g_xyz = Guarded(m, 3, torch.float32, ld=3, pad_rows=4096, prefill=k, device=DEV)      # rows = the expected kept count
        g_rgbx = Guarded(m, 4, torch.uint8, ld=4, pad_rows=4096, prefill=k, device=DEV)
        ws = fill_pattern(torch.empty(ws_bytes + 64, dtype=torch.uint8, device=DEV), k)
        total = fill_pattern(torch.empty(4, dtype=torch.uint8, device=DEV), k)
        _lib.check(lib.ew_filter_compact(_p(d_conf), n, ctypes.c_float(thr), _p(d_xyz), _p(d_img), 1 if nchw else 0, hw, _p(g_xyz.buf),
                                         _p(g_rgbx.buf), _p(ws), _p(total), ops._stream()), "ew_filter_compact")
        torch.cuda.synchronize()
        got_total = int(total.view(torch.int32).item())
        assert got_total == m, f"*total {got_total}, expected {m} ({nblk} blocks)"
        g_xyz.check()                                                          # nothing past row m (m == 0: nothing at all)
        g_rgbx.check()
        assert bool((ws[ws_bytes:] == ws[-1]).all()), "workspace overrun"
        got_xyz, got_rgbx = g_xyz.view.cpu().numpy(), g_rgbx.view.cpu().numpy()
        bad = (got_xyz.view(np.uint32) != want_xyz.view(np.uint32)).any(1) | (got_rgbx[:, :3] != want_rgb).any(1)
        if bad.any():
            r = int(np.argmax(bad))
            src = int(np.flatnonzero(keep)[r])
            raise AssertionError(f"kept row {r} (source point {src}, block {src // 2048}, scan chunk {src // 2048 // 1024}): xyz {got_xyz[r]} vs "
                                 f"{want_xyz[r]}, rgb {got_rgbx[r]} vs {want_rgb[r]}; {int(bad.sum())} rows differ")
        assert not got_rgbx[:, 3].any(), "RGBX top byte must be 0 (R | G << 8 | B << 16)"
        outs.append((g_xyz, g_rgbx))
    assert_same_bits(outs[0][0].view, outs[1][0].view, "out_xyz")
    assert_same_bits(outs[0][1].view, outs[1][1].view, "out_rgbx")


# ------------------------------------------------------------------------------------------------ ew_select_kth_f32
def _check_select(a, ks):
    from evoworld_amd import ops
    n = a.size
    srt = np.sort(a)
    x = torch.from_numpy(a).to(DEV)
    for k in sorted({int(k) for k in ks if 0 <= k < n}):
        got = ops.select_kth(x, k).cpu().numpy()
        assert got[0] == srt[k], (n, k, got[0], srt[k])                        # by value: +-0 ordering is not an issue
        assert got[1] == srt[min(k + 1, n - 1)], (n, k, got[1], srt[min(k + 1, n - 1)])
    return x


def _ranks(n):
    from evoworld_amd import reprojection as RP
    ks = {0, n // 2, n - 2, n - 1}
    for q in (50.0, 30.0, 99.5):
        lo, hi, _ = RP.percentile_rank(n, q)
        ks |= {lo, hi}
    return ks


def test_select_kth_product_scale_with_ties_across_the_median():
    from evoworld_amd import reprojection as RP
    rng = np.random.default_rng(11)
    n = N_PRODUCT
    a = rng.random(n, dtype=np.float32)
    a[a == 0] = np.float32(0.5)                                                # uniform in (0, 1)
    a[rng.choice(n, 100_000, replace=False)] = np.float32(0.5)                 # a block of exact ties across the median
    srt = np.sort(a)
    assert srt[n // 2] == np.float32(0.5) and srt[n // 2 - 1000] == np.float32(0.5) and srt[n // 2 + 1000] == np.float32(0.5)
    x = _check_select(a, _ranks(n))
    for q in (50.0, 30.0, 99.5):
        assert RP.percentile_threshold(x, q) == np.percentile(a, q), q


def test_select_kth_all_equal():
    n = N_PRODUCT
    _check_select(np.full(n, 0.37, dtype=np.float32), _ranks(n))


@pytest.mark.parametrize("lo,hi", [(0.25, 0.75), (1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0)))), (-0.0, 0.0)])
@pytest.mark.parametrize("dc", [-1, 0, 1])
def test_select_kth_two_valued(lo, hi, dc):
    """c copies of `lo`, the rest `hi`, shuffled; the boundary sits at k - 1, k and k + 1 for k = n // 2"""
    n = 1_000_003
    k = n // 2
    c = k + dc
    a = np.full(n, hi, dtype=np.float32)
    a[:c] = np.float32(lo)
    np.random.default_rng(3).shuffle(a)
    _check_select(a, {0, k - 2, k - 1, k, k + 1, n - 2, n - 1})


def test_select_kth_infinities_and_negatives():
    rng = np.random.default_rng(4)
    n = 100_003
    fmax = np.finfo(np.float32).max
    a = -np.abs(rng.standard_normal(n).astype(np.float32)) - np.float32(1e-3)  # negative values only, plus the extremes
    a[:40] = -np.inf
    a[40:50] = np.inf
    a[50:60] = fmax
    a[60:70] = -fmax
    rng.shuffle(a)
    _check_select(a, {0, 39, 40, 49, 50, n // 2, n - 21, n - 20, n - 11, n - 10, n - 2, n - 1})


# ------------------------------------------------------------------------------------------------ ew_splat_cubemap + ew_splat_resolve
def _views(V, seed):
    rng = np.random.default_rng(seed)
    c2w = np.repeat(np.eye(4)[None], V, 0)
    for v in range(1, V):                             # view 0 stays the identity: the border cases rely on it
        a = rng.uniform(-np.pi, np.pi)
        c2w[v, :3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) * 1.3
        c2w[v, :3, 3] = rng.normal(size=3)
    return c2w


def _cloud(n, seed, spread=4.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * spread).astype(np.float32), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def _splat(xyz, rgb, w2c, res, fx, fy, cx, cy, z_near, rgb_stride=3, face_channels=3):
    """ABI call with zbuf and faces guarded, both prefills, the two runs bit-identical -> (faces [V,6,res,res,ch], zbuf u64)"""
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    V, n = w2c.shape[0], xyz.shape[0]
    ncell = V * 6 * res * res
    d_xyz, d_w2c = torch.from_numpy(np.ascontiguousarray(xyz)).to(DEV), torch.from_numpy(np.ascontiguousarray(w2c)).to(DEV)
    cols = rgb if rgb_stride == 3 else np.concatenate([rgb, np.full((n, 1), 0xEE, np.uint8)], 1)   # X byte set: it must be masked off
    d_rgb = torch.from_numpy(np.ascontiguousarray(cols)).to(DEV)
    assert d_xyz.data_ptr() % 16 == 0
    runs = []
    for k in (0, 1):
        g_z = Guarded(ncell, 8, torch.uint8, ld=8, pad_rows=4096, prefill=k, device=DEV)     # documented as uninitialised on entry
        g_f = Guarded(ncell, face_channels, torch.uint8, ld=face_channels, pad_rows=4096, prefill=k, device=DEV)
        _lib.check(lib.ew_splat_cubemap(_p(d_xyz), n, _p(d_w2c), _p(g_z.buf), V, res, fx, fy, cx, cy, z_near, ops._stream()), "ew_splat_cubemap")
        _lib.check(lib.ew_splat_resolve(_p(g_z.buf), _p(d_rgb), rgb_stride, _p(g_f.buf), face_channels, V, res, ops._stream()),
                   "ew_splat_resolve")
        torch.cuda.synchronize()
        g_z.check()
        g_f.check()
        runs.append((g_z, g_f))
    assert_same_bits(runs[0][0].view, runs[1][0].view, "zbuf")
    assert_same_bits(runs[0][1].view, runs[1][1].view, "faces")                # 4-channel faces: the fourth byte is written, and the same way
    zbuf = runs[0][0].view.cpu().numpy().reshape(-1).view(np.uint64).reshape(V, 6, res, res)
    faces = runs[0][1].view.cpu().numpy().reshape(V, 6, res, res, face_channels)
    return faces, zbuf


def _assert_splat(xyz, rgb, w2c, res, fx, fy, cx, cy, z_near, **kw):
    faces, zbuf = _splat(xyz, rgb, w2c, res, fx, fy, cx, cy, z_near, **kw)
    with np.errstate(all="ignore"):                   # non-finite coordinates: inf * 0 and inf - inf are part of the case
        want_faces, want_z = R.splat_ref(xyz, rgb, w2c, res, fx, fy, cx, cy, z_near)
    bad = zbuf != want_z
    if bad.any():
        v, f, y, x = (int(i) for i in np.argwhere(bad)[0])
        g, w = int(zbuf[v, f, y, x]), int(want_z[v, f, y, x])
        raise AssertionError(f"zbuf[{v},{f},{y},{x}]: depth bits / index {g >> 32:#x} / {g & 0xffffffff} vs oracle {w >> 32:#x} / {w & 0xffffffff} "
                             f"(index % 4 = {(g & 0xffffffff) % 4}, n = {xyz.shape[0]}); {int(bad.sum())} cells differ")
    assert np.array_equal(faces[..., :3], want_faces)
    return want_z


@pytest.mark.parametrize("n,V,res", [(2_300_003, 2, 512), (4097, 2, 64), (4098, 2, 64), (4099, 2, 64)])
def test_splat_grid_stride_and_tail(n, V, res):
    """n = 2 300 003 > 2 x 1 048 576: three trips of the grid-stride loop, n % 4 == 3; 4097..4099: cnt = 1, 2, 3 in the last thread"""
    xyz, rgb = _cloud(n, 1)
    f = res / 2.0
    want_z = _assert_splat(xyz, rgb, R.face_w2c_ref(_views(V, 2)), res, f, f, f, f, 0.1)
    hit = want_z != np.uint64(0xFFFFFFFFFFFFFFFF)
    idx = (want_z[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    if n > 2 * 1024 * 1024:
        assert (idx >= 2 * 1024 * 1024).sum() > 1000                           # third-trip points are visible


@pytest.mark.parametrize("V,res,n", [(1, 511, 300_000), (3, 511, 300_000), (3, 1, 5000), (1, 1, 7)])
def test_splat_odd_geometry(V, res, n):
    """odd res x odd V: V*6*res*res % 4 == 2 -> resolve's scalar tail; res = 1, V = 1: 6 cells"""
    assert (V * 6 * res * res) % 4 == 2
    xyz, rgb = _cloud(n, 5)
    f = res / 2.0
    for ch in (3, 4):
        _assert_splat(xyz, rgb, R.face_w2c_ref(_views(V, 6)), res, f, f, f, f, 0.1, rgb_stride=ch, face_channels=ch)


@pytest.mark.parametrize("rgb_stride", [3, 4])
@pytest.mark.parametrize("face_channels", [3, 4])
def test_splat_resolve_all_instantiations(rgb_stride, face_channels):
    xyz, rgb = _cloud(300_001, 7)
    _assert_splat(xyz, rgb, R.face_w2c_ref(_views(3, 8)), 128, 64.0, 64.0, 64.0, 64.0, 0.1, rgb_stride=rgb_stride, face_channels=face_channels)


def test_splat_ties_triplicated_cloud():
    """every point three times at shuffled positions with different colours: the lowest index must win every pixel"""
    xyz0, _ = _cloud(60_000, 9)
    rng = np.random.default_rng(10)
    perm = rng.permutation(180_000)
    xyz = np.tile(xyz0, (3, 1))[perm]
    rgb = rng.integers(0, 256, size=(180_000, 3), dtype=np.uint8)
    want_z = _assert_splat(xyz, rgb, R.face_w2c_ref(_views(3, 11)), 64, 32.0, 32.0, 32.0, 32.0, 0.1)
    hit = want_z != np.uint64(0xFFFFFFFFFFFFFFFF)
    win = (want_z[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    first = np.full(60_000, 180_000)
    np.minimum.at(first, perm % 60_000, np.arange(180_000))
    assert np.array_equal(win, first[perm[win] % 60_000])                       # the oracle itself picked the first copy


def test_splat_ties_plane_of_equal_depth():
    """a plane z = const in front of the identity view's front face, sampled 3 x denser than the pixel grid: nine fragments of
    identical depth bits per pixel"""
    res = 64
    t = (np.arange(3 * res, dtype=np.float64) + 0.5) / 3.0                     # pixel coordinate of each sample
    u, v = np.meshgrid(t, t)
    z = 2.0
    xyz = np.stack([(u - 32.0) * z / 32.0, (v - 32.0) * z / 32.0, np.full_like(u, z)], -1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(12)
    xyz = xyz[rng.permutation(len(xyz))]
    rgb = rng.integers(0, 256, size=(len(xyz), 3), dtype=np.uint8)
    want_z = _assert_splat(xyz, rgb, R.face_w2c_ref(np.eye(4)[None]), res, 32.0, 32.0, 32.0, 32.0, 0.1)
    front = want_z[0, 4]
    assert (front >> np.uint64(32) == np.uint64(np.float32(z).view(np.uint32))).all()       # every front pixel: the same depth bits


def test_splat_non_finite_and_border_coordinates():
    res, z = 64, 2.0
    base, _ = _cloud(50_001, 13)
    sp = []
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for axis in range(3):
            p = np.array([0.3, -0.2, 1.5])
            p[axis] = bad
            sp.append(p)
        sp.append(np.full(3, bad))
    for x in (0.0, 0.01, -0.01):                      # zc == z_near exactly on the identity view's front face: rejected (the test is >)
        sp.append([x, 0.0, np.float32(0.1)])
    sp.append([0.0, 0.0, np.nextafter(np.float32(0.1), np.float32(1.0))])
    # identity view, front face, z = 2, fx = cx = 32: pu = 32 x / 2 + 32 is exact for these x -> pixel borders, pu in (-1, 0), pu == res
    ts = [0.0, -0.0625, -0.5, -0.9375, -1.0, 1.0, 0.9375, 31.0, 32.0, res - 1.0, res - 0.0625, float(res), res + 0.5]
    for tu in ts:
        for tv in ts:
            sp.append([(tu - 32.0) * z / 32.0, (tv - 32.0) * z / 32.0, z])
    sp = np.array(sp, dtype=np.float32)
    rng = np.random.default_rng(14)
    xyz = np.concatenate([base, sp])
    xyz = xyz[rng.permutation(len(xyz))]
    rgb = rng.integers(0, 256, size=(len(xyz), 3), dtype=np.uint8)
    _assert_splat(xyz, rgb, R.face_w2c_ref(_views(2, 15)), res, 32.0, 32.0, 32.0, 32.0, float(np.float32(0.1)))
    # the specials alone: their fate is not hidden behind nearer points of the cloud
    want_z = _assert_splat(sp, rgb[:len(sp)], R.face_w2c_ref(_views(2, 15)), res, 32.0, 32.0, 32.0, 32.0, float(np.float32(0.1)))
    front = want_z[0, 4] != np.uint64(0xFFFFFFFFFFFFFFFF)
    assert front[0, 0] and front[res - 1, res - 1] and front[31, 32]           # pu == 0 and pu == res - 0.0625 land inside; -0.0625 and res do not
    assert int(front.sum()) == 5 * 5                                           # ts lands on pixels 0 (0, 0.9375), 1, 31, 32, 63 (63, 63.9375) only


# ------------------------------------------------------------------------------------------------ ew_cube2equi_gather
def test_cube2equi_product_channels():
    """4-channel faces at 2000 x 1000 x 512, V = 2: what render_cubemaps_to_panoramas runs"""
    from evoworld_amd import _lib, ops
    from evoworld_amd.reprojection import build_cube2equi_lut
    lib = _lib.load()
    V, H, W, res = 2, 1000, 2000, 512
    lut = build_cube2equi_lut(W, H, res)
    g = torch.Generator().manual_seed(0)
    faces = torch.randint(0, 256, (V, 6, res, res, 4), generator=g, dtype=torch.uint8)
    want = R.cube2equi_gather_ref(faces.numpy()[..., :3], lut.numpy())
    d_faces, d_lut = faces.to(DEV), lut.to(DEV)
    runs = []
    for k in (0, 1):
        g_p = Guarded(V * H * W, 3, torch.uint8, ld=3, pad_rows=4096, prefill=k, device=DEV)
        _lib.check(lib.ew_cube2equi_gather(_p(d_faces), 4, _p(d_lut), _p(g_p.buf), V, H, W, res, ops._stream()), "ew_cube2equi_gather")
        torch.cuda.synchronize()
        g_p.check()
        runs.append(g_p)
    assert_same_bits(runs[0].view, runs[1].view, "pano")
    assert np.array_equal(runs[0].view.cpu().numpy().reshape(V, H, W, 3), want)
