"""fp64 numpy restatement of the row-weighted per-frame metrics (ew_video_metrics_ws, include/evoworld_hip.h; a helper module, not
collected): the oracle of tests/test_gpu_ws_metrics.py and tests/test_gpu_metrics_viewports.py.  Nothing of this is in the
reference: the definitions in the header are the specification.  The squared error, the SSIM map and its window are those of
tests/metrics_ref.py; only the averaging differs."""
import math

import numpy as np

from metrics_ref import _valid_filter, gaussian11, u8_values


def latitude_weights(H):
    y = np.arange(H, dtype=np.float64)
    return np.cos((y + 0.5 - H / 2) * np.pi / H)


def wsse_ref(a, b, w):
    """float32 [C,H,W] pair, w fp64 [H] -> sum_{c,y,x} w[y] * float32((a - b)^2), in fp64"""
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float32)
    d2 = (d * d).astype(np.float32).astype(np.float64)
    return float(np.sum(d2 * np.asarray(w, np.float64)[None, :, None]))


def ws_psnr_ref(a, b, w):
    C, H, W = np.asarray(a).shape
    wmse = wsse_ref(a, b, w) / (C * W * float(np.sum(w)))
    if wmse < 1e-10:
        return 100
    return 20 * math.log10(1 / math.sqrt(wmse))


def ssim_map_ref(a, b):
    """one plane pair -> the [H-10, W-10] SSIM map of metrics_ref.ssim_plane_ref"""
    x, y = np.asarray(a, np.float64), np.asarray(b, np.float64)
    g = gaussian11()
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m1, m2 = _valid_filter(x, g), _valid_filter(y, g)
    m1s, m2s, m12 = m1 ** 2, m2 ** 2, m1 * m2
    s1 = _valid_filter(x * x, g) - m1s
    s2 = _valid_filter(y * y, g) - m2s
    s12 = _valid_filter(x * y, g) - m12
    return (2 * m12 + C1) * (2 * s12 + C2) / ((m1s + m2s + C1) * (s1 + s2 + C2))


def wssim_ref(a, b, w):
    """float32 [C,H,W] pair -> mean over the channels of the SSIM map averaged under the weights of the windows' centre rows"""
    C, H, W = np.asarray(a).shape
    wc = np.asarray(w, np.float64)[5:H - 5]                      # output row i is centred on image row i + 5
    vals = [float(np.sum(ssim_map_ref(a[c], b[c]) * wc[:, None]) / ((W - 10) * np.sum(wc))) for c in range(C)]
    return float(np.mean(vals))


def frames_u8(u8):
    """uint8 [H,W,C] -> float32 [C,H,W] = k / 255"""
    return u8_values(u8).transpose(2, 0, 1)
