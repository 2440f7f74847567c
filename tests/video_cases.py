"""The inputs of the MJPEG kernel tests (tests/test_gpu_video.py), built on the CPU and shared with tests/test_cpu_video.py, which checks
the oracle-only preconditions without a GPU.  Every case is (frames uint8 [V,H,W,3], quality); each runs under both samplings.

Shapes: one MCU of each sampling (8x8, 16x16), replication on both axes (9x17), several MCU rows / columns with W no multiple of 16
(40x72, V = 3), more than 8 MCU rows so that the RST index wraps (152x40), a width just past the DCT kernel's 128-pixel x-tile
(24x136) and one past the entropy kernel's 256-block round (16x700: 264 blocks per segment under either sampling).
Contents: uniform noise, smooth ramps (long zero runs), flat 0 / 128 / 255, left half 0 and right half 255 at quality 100 (DC
differences of category 11), and images synthesised by inverse DCT (below).

The seeds of the noise cases were chosen on the oracle alone: the first seed from 0 for which at most 0.2 % of the case's float64
quotients lie within 1e-3 of a half-integer under both samplings (test_near_tie_precondition asserts exactly that).  A quotient
spread over many integers lands in that window with probability 2e-3, so full-range noise sits at the limit by construction and a
tiny image needs a seed with no such quotient at all."""
import numpy as np

import jpeg_ref as J

NOISE = {  # name: (V, H, W, quality, seed)
    "noise_8x8": (1, 8, 8, 90, 5),
    "noise_16x16": (1, 16, 16, 90, 1),
    "noise_9x17": (2, 9, 17, 75, 0),
    "noise_40x72": (3, 40, 72, 90, 2),
    "noise_152x40": (1, 152, 40, 50, 0),
    "noise_24x136": (2, 24, 136, 90, 3),
    "noise_16x700": (1, 16, 700, 90, 0),
}


def _noise(V, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (V, H, W, 3), dtype=np.uint8)


def _ramp(V, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for v in range(V):
        r = 255 * x / max(W - 1, 1)
        g = 255 * y / max(H - 1, 1)
        b = 255 * (x + y + 7 * v) / (W + H + 7 * v)
        out.append(np.stack([r, g, b][v % 3:] + [r, g, b][:v % 3], axis=-1))
    return np.rint(np.stack(out)).astype(np.uint8)


def _flat(H, W):
    return np.stack([np.full((H, W, 3), v, np.uint8) for v in (0, 128, 255)])


def _halves(H, W):
    f = np.zeros((1, H, W, 3), np.uint8)
    f[:, :, W // 2:] = 255
    return f


def _idct_blocks(coef_blocks):
    """[rows, cols, 8, 8] DCT coefficients (natural order) -> the grey uint8 image [rows * 8, cols * 8, 3] of their inverse DCT + 128"""
    d = J.dct_matrix()
    px = d.T @ coef_blocks @ d + 128.0
    rows, cols = px.shape[:2]
    img = np.rint(np.clip(px, 0, 255)).astype(np.uint8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)
    return np.repeat(img[..., None], 3, axis=2)


def synth_zrl():
    """24x136 at quality 50: every block holds one or two luminance coefficients of one quantisation step, at zigzag positions chosen so
    that a run of at least 16 zeros precedes a non-zero one (ZRL); the pixel rounding (|error| <= 0.5 per pixel, so < 0.5 per
    orthonormal coefficient ... against steps of >= 10) leaves the other positions zero."""
    rng = np.random.default_rng(5)
    ql, _ = J.quant_tables_ref(50)
    blocks = np.zeros((3, 17, 64))
    for b in blocks.reshape(-1, 64):
        k1 = int(rng.integers(17, 40))
        k2 = int(rng.integers(k1 + 17, 64)) if k1 + 17 < 64 and rng.random() < 0.5 else None
        for k in (k1, k2):
            if k is not None:
                nat = J.ZIGZAG[k]
                b[nat] = float(rng.choice([-1, 1])) * 1.0 * ql[nat]
        b[0] = float(rng.integers(-20, 20)) * ql[0]
    return _idct_blocks(blocks.reshape(3, 17, 8, 8))[None], 50


def synth_max():
    """16x32 at quality 100 (every divisor 1): blocks whose pixels are 0 / 255 in the sign pattern of one DCT basis function with
    |cos| constant (frequencies 0 and 4), the inverse DCT of the largest coefficient that basis can carry.  With Y in [-128, 127]
    that is 32 * 0.125 * (128 + 127) = 1020: the orthonormal DCT of 8-bit pixels cannot pass 8 * 128 = 1024 in DC and 1020 in AC, so
    the +-1023 clamp of the AC coefficients is out of the reach of any image (test_entropy_clamps_injected_coefficients covers the
    clamp itself); 1020 is in the same category (10) as 1023.  The (4,4) block has 40 zeros in front of its coefficient: two ZRL."""
    d = J.dct_matrix()
    sign = np.sign(d[4])
    one = np.ones(8)
    pats = [np.outer(sign, sign), np.outer(one, sign), np.outer(sign, one), -np.outer(sign, sign)]
    rows = [np.concatenate([np.where(p > 0, 255, 0) for p in pats], axis=1)] * 2
    img = np.concatenate(rows, axis=0).astype(np.uint8)
    return np.repeat(img[..., None], 3, axis=2)[None], 100


def build():
    cases = {name: (_noise(V, H, W, seed), q) for name, (V, H, W, q, seed) in NOISE.items()}
    cases["ramp_40x72"] = (_ramp(3, 40, 72), 90)
    cases["ramp_152x40"] = (_ramp(1, 152, 40), 75)
    cases["flat_9x17"] = (_flat(9, 17), 90)
    cases["flat_16x16"] = (_flat(16, 16), 100)
    cases["halves_16x32"] = (_halves(16, 32), 100)
    cases["halves_40x72"] = (_halves(40, 72), 100)
    cases["synth_zrl_24x136"] = synth_zrl()
    cases["synth_max_16x32"] = synth_max()
    return cases


CASES = build()
SUBSAMPLINGS = ("4:2:0", "4:4:4")
_oracle = {}


def oracle(name, subsampling):
    """(quotients float64, coefficients int16) [V, mcu_rows, mcu_cols, blocks_per_mcu, 64] of a case, computed once"""
    key = (name, subsampling)
    if key not in _oracle:
        frames, quality = CASES[name]
        q = np.stack([J.quotients_ref(f, quality, subsampling) for f in frames])
        q.setflags(write=False)
        c = J.quantise_ref(q.copy())
        c.setflags(write=False)
        _oracle[key] = (q, c)
    return _oracle[key]
