#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- golden vectors of the reference's panorama/cubemap pair (runs ONLY where the reference tree is).

Imports the reference with the stubs of oracle/make_goldens_pipeline.py (read-only, nothing copied) and runs its own
`Navigator.convert_panorama_to_cubemap`, `precompute_rotation_matrix` and `cubemap_to_equirectangular`
(evoworld/inference/navigator_evoworld.py:514-705, 707-743, 745-864; numpy + PIL only).  8-bit inputs and outputs only.

  (a) bilinear and nearest crosses + faces of a noise-like, a smooth and a plateau image (saturated 0 / 255 blocks, every seam
      column distinct); per bilinear case a sensitivity mask over the scaled cross, recomputed here in this file's own words:
      a pixel is masked where uf or vf lies within 1e-9 of an integer, or where the float64 blend of any channel lies within 1e-6
      of an integer before truncation
  (b) nearest mode on a pixel-index-encoded panorama (R = ui & 255, G = vi & 255, B = ui >> 8 | (vi >> 8) << 4; not stored)
  (c) cubemap_to_equirectangular on index-encoded faces (R = position in the key order + 1, G / B = low / high byte of
      v*res + u; not stored) of two
      resolutions handed over in shuffled dict orders, one dict with a face missing, and one LANCZOS-downscaled case
  (e) precompute_rotation_matrix(90, -90, 180)
The three LANCZOS resizes alone (d) need no stored vector: the tests compare against PIL itself.

Usage:  python tools/make_goldens_cubemap.py   (from the repo root)  ->  tests/golden/cubemap.npz
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "cubemap.npz")

FACE_NAMES = ["right", "left", "top", "bottom", "front", "back"]
# (tag, image, W0, scale_factor): scaled widths 256 (edge 64) and 512 (edge 128); the incompressible images stay small (file size)
A_CASES = [("noise_128_s2", "noise", 128, 2), ("smooth_128_s2", "smooth", 128, 2), ("plateau_256_s2", "plateau", 256, 2),
           ("plateau_512_s1", "plateau", 512, 1)]
SHARE_SIZES = (512, 2048, 4096)


def noise_image(w):
    rng = np.random.default_rng(w)
    return rng.integers(0, 256, size=(w // 2, w, 3), dtype=np.uint8)


def smooth_image(w):
    y, x = np.mgrid[0:w // 2, 0:w].astype(np.float64)
    ch = [127.5 + 127.5 * np.sin(2 * np.pi * (fx * x / w + fy * y / (w // 2)) + p) for fx, fy, p in ((1, 0.5, 0.3), (2, 1, 1.1), (0.5, 1.5, 2.0))]
    return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)


def plateau_image(w):
    """blocks of saturated 0 / 255 and a mid plateau (200, 37, 128); the first and last four columns count up and down so
    that every column next to the seam is distinct"""
    h = w // 2
    y, x = np.mgrid[0:h, 0:w]
    bx, by = x // (w // 8), y // (h // 4)
    img = np.zeros((h, w, 3), np.uint8)
    img[(bx + by) % 3 == 0] = 255
    img[(bx + by) % 3 == 1] = (200, 37, 128)
    for k in range(4):
        img[:, k] = (10 + 40 * k, 250 - 30 * k, 5 + k)
        img[:, w - 1 - k] = (245 - 50 * k, 20 + 35 * k, 100 + k)
    return img


IMAGES = {"noise": noise_image, "smooth": smooth_image, "plateau": plateau_image}


def index_pano(w):
    y, x = np.mgrid[0:w // 2, 0:w]
    return np.stack([x & 255, y & 255, (x >> 8) | ((y >> 8) << 4)], -1).astype(np.uint8)


def index_faces(res):
    v, u = np.mgrid[0:res, 0:res]
    k = v * res + u
    return {n: np.stack([np.full_like(k, i + 1), k & 255, k >> 8], -1).astype(np.uint8) for i, n in enumerate(FACE_NAMES)}


def source_coords(W):
    """(uf, vf, used) over the 3E x 4E cross of a W-wide panorama: the reference's formula, written out again."""
    E = W // 4
    i, j = np.meshgrid(np.arange(W), np.arange(3 * E), indexing="xy")
    cell, row = i // E, j // E
    a, b = 2.0 * i / E, 2.0 * j / E
    one = np.ones_like(a)
    mid = [(-one, 1.0 - a), (a - 3.0, -one), (one, a - 5.0), (7.0 - a, one)]
    x = np.select([row == 0, row == 2] + [cell == c for c in range(4)], [b - 1.0, 5.0 - b] + [m[0] for m in mid])
    y = np.select([row == 0, row == 2] + [cell == c for c in range(4)], [a - 5.0, a - 5.0] + [m[1] for m in mid])
    z = np.select([row == 0, row == 2], [one, -one], 3.0 - b)
    theta = np.arctan2(y, x)
    phi = np.arctan2(z, np.hypot(x, y))
    uf = 2.0 * E * (theta + np.pi) / np.pi
    vf = 2.0 * E * (np.pi / 2 - phi) / np.pi
    return uf, vf, (row == 1) | (cell == 2)


def near_integer(t, eps):
    return np.abs(t - np.rint(t)) <= eps


def sensitivity_mask(pixels, W):
    """(mask [3E,4E] bool over the cross, share of used pixels under the coordinate criterion, share under either)"""
    uf, vf, used = source_coords(W)
    H = W // 2
    m1 = near_integer(uf, 1e-9) | near_integer(vf, 1e-9)
    u0, v0 = np.floor(uf).astype(int), np.floor(vf).astype(int)
    mu, nu = (uf - u0)[..., None], (vf - v0)[..., None]
    cu = lambda t: np.clip(t, 0, W - 1)
    cv = lambda t: np.clip(t, 0, H - 1)
    A, B = pixels[cv(v0), cu(u0)], pixels[cv(v0), cu(u0 + 1)]
    C, D = pixels[cv(v0 + 1), cu(u0)], pixels[cv(v0 + 1), cu(u0 + 1)]
    blend = A * (1 - mu) * (1 - nu) + B * mu * (1 - nu) + C * (1 - mu) * nu + D * mu * nu
    m2 = near_integer(blend, 1e-6).any(-1)
    n = used.sum()
    return (m1 | m2) & used, float((m1 & used).sum() / n), float(((m1 | m2) & used).sum() / n), blend


def main():
    from oracle.make_goldens_pipeline import _patch_reference
    _patch_reference()
    import evoworld.inference.navigator_evoworld as NV
    from PIL import Image
    nav = NV.Navigator.__new__(NV.Navigator)
    nav.logger = SimpleNamespace(info=lambda *a, **k: None)
    gold = {}

    # coordinate-criterion shares at the sizes of the issue (no image involved)
    for W in SHARE_SIZES:
        uf, vf, used = source_coords(W)
        m1 = (near_integer(uf, 1e-9) | near_integer(vf, 1e-9)) & used
        half = (near_integer(uf - 0.5, 1e-9) | near_integer(vf - 0.5, 1e-9)) & used
        print(f"W={W}: coordinate criterion {100 * m1.sum() / used.sum():.2f} % of used cross pixels; nearest within 1e-9 of a half-integer: {int(half.sum())}")
        assert half.sum() == 0

    def faces_array(faces):
        assert list(faces) == FACE_NAMES
        return np.stack([np.asarray(faces[n]) for n in FACE_NAMES])

    # (a)
    for tag, kind, W0, s in A_CASES:
        img = IMAGES[kind](W0)
        gold[f"a_{tag}_input"] = img
        for mode, interp in (("bilinear", True), ("nearest", False)):
            cubemap, faces = nav.convert_panorama_to_cubemap(Image.fromarray(img), interpolation=interp, scale_factor=s)
            gold[f"a_{tag}_{mode}_cubemap"] = np.asarray(cubemap)
            gold[f"a_{tag}_{mode}_faces"] = faces_array(faces)
        W = W0 * s
        scaled = np.asarray(Image.fromarray(img).resize((W, W // 2), Image.LANCZOS))
        mask, share1, share, blend = sensitivity_mask(scaled, W)
        E = W // 4
        # this file's blend, truncated, must be the reference's faces wherever it is not masked (the mask means what it says)
        mine = blend.astype(np.uint8)
        f = gold[f"a_{tag}_bilinear_faces"]
        cells = {"right": (3, 1), "left": (1, 1), "top": (2, 0), "bottom": (2, 2), "front": (2, 1), "back": (0, 1)}
        for k, n in enumerate(FACE_NAMES):
            c, r = cells[n]
            sl = (slice(r * E, (r + 1) * E), slice(c * E, (c + 1) * E))
            assert np.array_equal(mine[sl][~mask[sl]], f[k][~mask[sl]])
        if E >= 128:
            assert share1 <= 0.03, (tag, share1)
        gold[f"a_{tag}_mask"] = np.packbits(mask)
        print(f"{tag}: W={W} edge {E}: masked by coordinates {100 * share1:.2f} %, by either criterion {100 * share:.2f} % of used pixels")
    fp = gold["a_plateau_512_s1_bilinear_faces"]
    print("plateau 512 s1: pixels at 254 / 199 (A - 1):", int((fp == 254).sum()), int((fp[..., 0] == 199).sum()))

    # (b)
    for W0 in (256,):                                    # the input is index_pano(W0): the test rebuilds it from the formula above
        cubemap, faces = nav.convert_panorama_to_cubemap(Image.fromarray(index_pano(W0)), interpolation=False, scale_factor=1)
        gold[f"b_{W0}_faces"] = faces_array(faces)

    # (c)
    rng = np.random.default_rng(7)
    for tag, res, (w, h), s, drop in (("r64", 64, (256, 128), 1, None), ("r32", 32, (200, 100), 1, None),
                                      ("r64_notop", 64, (256, 128), 1, "top"), ("r64_s2", 64, (128, 64), 2, None)):
        faces = index_faces(res)
        order = [FACE_NAMES[k] for k in rng.permutation(6)]
        d = {n: Image.fromarray(faces[n]) for n in order if n != drop}
        pano = nav.cubemap_to_equirectangular(d, w, h, scale_factor=s)
        gold[f"c_{tag}_res"] = np.array(res, np.int64)       # the faces are index_faces(res)
        gold[f"c_{tag}_order"] = np.array([n for n in order if n != drop])
        gold[f"c_{tag}_size"] = np.array([w, h, s], np.int64)
        gold[f"c_{tag}_pano"] = np.asarray(pano)
        print(f"c_{tag}: dict order {list(d)}; black pixels {int((np.asarray(pano).sum(-1) == 0).sum())}")

    # (e)
    gold["e_rotation_90_m90_180"] = nav.precompute_rotation_matrix(90, -90, 180)

    np.savez_compressed(OUT, **gold)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
