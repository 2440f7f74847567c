"""fp64 numpy restatement of the reference's per-frame PSNR / SSIM (evoworld/metrics/other_metrics/calculate_psnr.py:6-15,
calculate_ssim.py:6-40) used by the metric tests as the oracle for shapes the golden fixture does not hold.  The 11x11 window is
applied as two 11-tap passes over the 'valid' region; its values agree with the golden (a run of the reference's own code) to
~1e-15 (tests/test_cpu_metrics.py)."""
import math

import numpy as np


def gaussian11(sigma=1.5):
    """cv2.getGaussianKernel(11, sigma) in double: exp(-0.5/sigma^2 * x^2), x = i - 5, times 1 / sum"""
    x = np.arange(11, dtype=np.float64) - 5.0
    t = np.exp((-0.5 / (sigma * sigma)) * x * x)
    return t * (1.0 / t.sum())


def u8_values(u8):
    """uint8 -> float32 k / 255 (torch's uint8 / 255.0: a correctly rounded float32 division)"""
    return (np.asarray(u8).astype(np.float32) / np.float32(255.0)).astype(np.float32)


def sse_ref(a, b):
    """float32 [C,H,W] pair -> sum of float32 (a - b)^2, in fp64"""
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float32)
    return float(np.sum((d * d).astype(np.float32), dtype=np.float64))


def psnr_ref(a, b):
    mse = sse_ref(a, b) / np.asarray(a).size
    if mse < 1e-10:
        return 100
    return 20 * math.log10(1 / math.sqrt(mse))


def _valid_filter(x, g):
    H, W = x.shape
    h = sum(g[j] * x[:, j:j + W - 10] for j in range(11))
    return sum(g[i] * h[i:i + H - 10, :] for i in range(11))


def ssim_plane_ref(a, b):
    x, y = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g = gaussian11()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m1, m2 = _valid_filter(x, g), _valid_filter(y, g)
    m1s, m2s, m12 = m1 ** 2, m2 ** 2, m1 * m2
    s1 = _valid_filter(x * x, g) - m1s
    s2 = _valid_filter(y * y, g) - m2s
    s12 = _valid_filter(x * y, g) - m12
    return ((2 * m12 + C1) * (2 * s12 + C2) / ((m1s + m2s + C1) * (s1 + s2 + C2))).mean()


def ssim_ref(a, b):
    """float32 [C,H,W] pair, C = 1 or 3 -> the reference's per-frame SSIM"""
    return float(np.array([ssim_plane_ref(a[c], b[c]) for c in range(a.shape[0])]).mean())
