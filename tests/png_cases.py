"""The inputs of the PNG encoder tests (tests/test_gpu_png.py), built on the CPU and shared with tests/test_cpu_png.py.  Every case is
(frames uint8 [V,H,W,3], rows_per_segment or None for the default).

Shapes: 1x1; 1x7 (H = 1: no row above); 5x1 (W = 1: nothing to the left); 40x72 (3 W = 216, a multiple of 4: the word loads, one
segment); 33x130 with 8 rows per segment (3 W = 390: the byte loads, five segments, the last one ragged); 3x1100 (3 W = 3300 > 256
threads x 12 bytes: a second pass of the filter's row loop).  Contents: gradient, sinusoid texture, noise of sigma 4 around a
gradient, uniform random bytes, a constant frame, a frame with large black areas.  `mixed_*` hold three different contents in one
call, so that tables and offsets are per frame."""
import numpy as np

import png_ref as R


def gradient(H, W, seed=0):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    r = 255 * x / max(W - 1, 1)
    g = 255 * y / max(H - 1, 1)
    b = 255 * (x + y + seed) / (W + H + seed)
    return np.rint(np.stack([r, g, b], axis=-1)).astype(np.uint8)


def texture(H, W, seed=0):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = [127.5 + 100 * np.sin(0.31 * x + 0.17 * y + seed + c) * np.cos(0.05 * x * (c + 1) - 0.23 * y) for c in range(3)]
    return np.rint(np.stack(ch, axis=-1)).astype(np.uint8)


def noise4(H, W, seed=0):
    g = gradient(H, W, seed).astype(np.float64) * 0.8 + 25
    return np.clip(np.rint(g + np.random.default_rng(seed).normal(0, 4, g.shape)), 0, 255).astype(np.uint8)


def random_bytes(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def constant(H, W, seed=0):
    return np.full((H, W, 3), 37 + seed, np.uint8)


def black_areas(H, W, seed=0):
    f = texture(H, W, seed)
    f[: H // 2, : (2 * W) // 3] = 0
    f[(3 * H) // 4:] = 0
    return f


CONTENTS = {"gradient": gradient, "texture": texture, "noise4": noise4, "random": random_bytes, "constant": constant, "black": black_areas}
SHAPES = {"1x1": (1, 1, None), "1x7": (1, 7, None), "5x1": (5, 1, None), "40x72": (40, 72, None), "33x130": (33, 130, 8),
          "3x1100": (3, 1100, None)}


def build():
    cases = {}
    for sname, (H, W, rps) in SHAPES.items():
        for cname, fn in CONTENTS.items():
            if sname == "3x1100" and cname not in ("noise4", "black"):
                continue
            cases[f"{cname}_{sname}"] = (fn(H, W)[None], rps)
    cases["mixed_40x72"] = (np.stack([texture(40, 72, 1), constant(40, 72, 2), random_bytes(40, 72, 3)]), None)
    cases["mixed_33x130"] = (np.stack([black_areas(33, 130, 1), noise4(33, 130, 2), gradient(33, 130, 3)]), 8)
    return cases


CASES = build()
_filtered = {}


def rows_per_segment(name):
    frames, rps = CASES[name]
    H, W = frames.shape[1:3]
    return min(H, rps if rps is not None else max(1, 32768 // (1 + 3 * W)))


def segments(name):
    """[(first row, rows)] of a frame of the case"""
    H = CASES[name][0].shape[1]
    rps = rows_per_segment(name)
    return [(r, min(rps, H - r)) for r in range(0, H, rps)]


def filtered(name, mode=R.ADAPTIVE):
    """the oracle's filtered rows uint8 [V,H,1+3W] of a case, computed once and read-only"""
    key = (name, mode)
    if key not in _filtered:
        f = np.stack([R.filter_frame(fr, mode) for fr in CASES[name][0]])
        f.setflags(write=False)
        _filtered[key] = f
    return _filtered[key]
