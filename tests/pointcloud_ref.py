"""numpy restatement of the voxel-grid downsample (ew_points_bounds / ew_voxel_keys / ew_voxel_reduce, include/evoworld_hip.h; a
helper module, not a test file).  Written from the specification of the operation, in the arithmetic it prescribes:
    bounds over the points whose three coordinates are finite; origin = min - 0.5 * voxel in float32;
    index = floor((p - origin) / voxel) in float32, per axis; key = ix << 42 | iy << 21 | iz;
    np.unique on the keys (ascending); per voxel: fp64 mean of the positions rounded to float32, per-channel integer sum / count
    rounded half to even in integer arithmetic, alpha 255, and the count."""
import numpy as np

GRID_BITS = 21


def finite_mask(xyz):
    return np.isfinite(xyz).all(axis=1)


def points_bounds_ref(xyz):
    """-> (min float32 [3], max float32 [3], n_finite); +inf / -inf and 0 without a finite point"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    p = xyz[finite_mask(xyz)]
    if len(p) == 0:
        return np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32), 0
    return p.min(axis=0), p.max(axis=0), len(p)


def voxel_indices_ref(xyz, voxel):
    """float32 index arithmetic of the finite points -> (int64 [m,3] indices, mask of the finite points)"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    m = finite_mask(xyz)
    p = xyz[m]
    v = np.float32(voxel)
    origin = (p.min(axis=0) - np.float32(0.5) * v).astype(np.float32)
    q = ((p - origin).astype(np.float32) / v).astype(np.float32)
    return np.floor(q).astype(np.int64), m


def voxel_keys_ref(xyz, voxel):
    """int64 [n]: the key of every point, 2^63 - 1 for a non-finite one (no range check)"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    keys = np.full(len(xyz), np.iinfo(np.int64).max, np.int64)
    if finite_mask(xyz).any():
        idx, m = voxel_indices_ref(xyz, voxel)
        keys[m] = (idx[:, 0] << (2 * GRID_BITS)) | (idx[:, 1] << GRID_BITS) | idx[:, 2]
    return keys


def main_case(n=4097):
    """the main downsample case: seed 1, integer coordinates in [-512, 512) / 64 (fp64 sums are exact), random uint8 colours"""
    rng = np.random.default_rng(1)
    xyz = (rng.integers(-512, 512, (n, 3)) / 64).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    return xyz, rgb


def half_even_div(s, c):
    """round-half-to-even of s / c for non-negative integer arrays, in integer arithmetic"""
    q, r = s // c, s % c
    up = (2 * r > c) | ((2 * r == c) & (q % 2 == 1))
    return q + up


def voxel_downsample_ref(xyz, rgb, voxel):
    """xyz float32 [n,3], rgb uint8 [n,3|4] (a fourth byte is ignored) -> dict(xyz float32 [m,3], rgba uint8 [m,4], count int32 [m],
    keys int64 [m] ascending, ties: how many channel means sat exactly half-way, run_max).  ValueError beyond 2^21 cells per axis."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, dtype=np.uint8)
    rgb = rgb.reshape(len(xyz), rgb.shape[-1] if rgb.ndim == 2 else 3)[:, :3]
    if len(xyz) == 0 or not finite_mask(xyz).any():
        return dict(xyz=np.zeros((0, 3), np.float32), rgba=np.zeros((0, 4), np.uint8), count=np.zeros(0, np.int32),
                    keys=np.zeros(0, np.int64), ties=0, run_max=0)
    idx, m = voxel_indices_ref(xyz, voxel)
    if idx.min() < 0 or idx.max() >= 1 << GRID_BITS:
        raise ValueError("voxel index outside [0, 2^21)")
    keys = (idx[:, 0] << (2 * GRID_BITS)) | (idx[:, 1] << GRID_BITS) | idx[:, 2]
    uk, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(uk), 3), np.float64)
    np.add.at(sums, inv, xyz[m].astype(np.float64))
    csum = np.zeros((len(uk), 3), np.int64)
    np.add.at(csum, inv, rgb[m].astype(np.int64))
    c = cnt.astype(np.int64)[:, None]
    rgba = np.full((len(uk), 4), 255, np.uint8)
    rgba[:, :3] = half_even_div(csum, c).astype(np.uint8)
    return dict(xyz=(sums / cnt[:, None].astype(np.float64)).astype(np.float32), rgba=rgba, count=cnt.astype(np.int32), keys=uk,
                ties=int((2 * (csum % c) == c).sum()), run_max=int(cnt.max()))
