"""Inputs shared by tests/test_gpu_frame_io.py (-m gpu) and tests/test_cpu_reproject_helpers.py (-m "not gpu"), so that the
conditions the GPU tests rest on (excluded share of the equi2pers comparison, number of exact rounding ties in the
quantiser's input) are checked on the CPU before a GPU sees them.  A plain module, imported like kernel_checks."""
import itertools
import math

import numpy as np

# ------------------------------------------------------------------------------------------------ ew_equi2pers
# A pixel whose float64 reference value lies within E2P_DELTA of an integer is held to |got - floor(ref)| <= 1 only; every other
# pixel must equal floor(ref).  E2P_DELTA is the value error float32 coordinate arithmetic can cause, MEASURED ON THE CPU BETWEEN
# THE TWO REFERENCES (oracle.reproject_ref.equi2pers_ref, float64, and equi2pers_ref32, the kernel's expression tree in numpy
# float32), never against the kernel: max |ref64 - ref32| over all cases below = 3.42e-3 (the 384x512 view of the 1000x2000
# panorama, next to a pole; 3.26e-3 over the 48x64 views of that panorama, 2.4e-4 on the two small panoramas), times 4 for the ulp
# differences between the device's atan2f / asinf and numpy's = 1.37e-2, rounded up.
# test_cpu_reproject_helpers.py re-measures the distance and fails if the references are ever further apart than E2P_DELTA / 4.
E2P_DELTA = 1.4e-2
# Share of pixels assertion (b) may leave out, per case.  Measured with E2P_DELTA on the float64 reference on the CPU: 3.1 % ... 4.3 %
# per case (2 * E2P_DELTA = 2.8 % for uniformly distributed fractional parts, plus the pixels a pole view takes from the clamped last
# row, whose values are exact integers wherever two neighbouring columns are equal).  If a case ever exceeds the cap, lower the
# gradient of smooth_pano, not the cap.
E2P_MAX_EXCLUDED = 0.05

E2P_PANOS = [(72, 144), (97, 211), (1000, 2000)]
E2P_YAWS = [0.0, 0.7, math.pi, -math.pi / 2]          # yaw = pi: the longitude seam runs through the view centre
E2P_PITCHES = [0.0, 1.4, -1.4]                        # +-1.4 rad: the view contains a pole (uj clamp, y1 = He - 1)
E2P_ROLLS = [0.0, 0.5]
E2P_FOVS = [90.0, 60.0]


def e2p_rots():
    return [{"yaw": y, "pitch": p, "roll": r} for y, p, r in itertools.product(E2P_YAWS, E2P_PITCHES, E2P_ROLLS)]


def e2p_cases():
    """(He, We, Hp, Wp, fov, rots): every rotation x fov x panorama size at 48 x 64, and the product's 384 x 512 once."""
    cases = [(He, We, 48, 64, fov, e2p_rots()) for (He, We), fov in itertools.product(E2P_PANOS, E2P_FOVS)]
    big = [{"yaw": math.pi, "pitch": 1.4, "roll": 0.5}, {"yaw": 0.0, "pitch": -1.4, "roll": 0.0},
           {"yaw": 0.7, "pitch": 0.0, "roll": 0.5}, {"yaw": -math.pi / 2, "pitch": 0.0, "roll": 0.0}]
    cases.append((1000, 2000, 384, 512, 90.0, big))
    return cases


def e2p_case_id(c):
    return f"{c[0]}x{c[1]}-{c[2]}x{c[3]}-fov{int(c[4])}"


def e2p_decidable(ref64):
    """mask of the pixels assertion (b) covers: float64 value at least E2P_DELTA away from an integer"""
    frac = ref64 - np.floor(ref64)
    return (frac >= E2P_DELTA) & (frac <= 1.0 - E2P_DELTA)


# ------------------------------------------------------------------------------------------------ ew_f32_chw_to_u8_hwc
QUANT_MIN_TIES = 100


def quant_inputs():
    """float32 [n] for the f32 -> u8 quantiser, no NaN: the 255 rounding midpoints x_k = 2 (k + 0.5) / 255 - 1 with their
    float32 neighbours on both sides, a dense sweep across and beyond [-1, 1], and the edges (+-0, +-1, just outside, +-inf,
    +-1e30)."""
    f32 = np.float32
    k = np.arange(255, dtype=np.float64)
    mid = (2.0 * (k + 0.5) / 255.0 - 1.0).astype(f32)
    up, dn = np.nextafter(mid, f32(np.inf)), np.nextafter(mid, f32(-np.inf))
    one = f32(1.0)
    edges = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(one, f32(2)), np.nextafter(-one, f32(-2)), np.nextafter(one, f32(0)),
                      np.nextafter(-one, f32(0)), 1.0001, -1.0001, np.inf, -np.inf, 1e30, -1e30, 1e-45, -1e-45], dtype=f32)
    dense = np.linspace(-1.2, 1.2, 2_000_001).astype(f32)
    return np.concatenate([mid, up, dn, edges, dense])


def count_exact_ties(scaled):
    """number of float32 scaled values that are exactly k + 0.5: the inputs on which half-even and half-up differ or agree
    by the rule alone"""
    s = scaled.astype(np.float64)
    return int(((s - np.floor(s)) == 0.5).sum())
