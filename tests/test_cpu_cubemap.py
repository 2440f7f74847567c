"""-m 'not gpu': host side of the panorama <-> cubemap conversions (Navigator.convert_panorama_to_cubemap /
precompute_rotation_matrix / cubemap_to_equirectangular, evoworld/inference/navigator_evoworld.py:514-864): the LANCZOS tables
against PIL itself, the bilinear tables unchanged, the cubemap -> equirect LUT against a run of the reference
(tests/golden/cubemap.npz, tools/make_goldens_cubemap.py), the rotation matrix, the 2:1 assertion and the CLI's arguments."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN

FACE_NAMES = ["right", "left", "top", "bottom", "front", "back"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "cubemap.npz"))


def apply_tables(img, coeffs_h, coeffs_v):
    """Pillow's two 8bpc passes (horizontal, then vertical, 8-bit intermediate) in numpy: what ew_resize_aa_u8 computes"""
    def one(a, kk, bounds):                             # along axis 1
        kk, bounds = kk.numpy().astype(np.int64), bounds.numpy()
        out = np.empty((a.shape[0], len(kk), 3), np.uint8)
        for xo, (xmin, n) in enumerate(bounds):
            acc = (a[:, xmin:xmin + n].astype(np.int64) * kk[xo, :n, None]).sum(1) + (1 << 21)
            out[:, xo] = np.clip(acc >> 22, 0, 255)
        return out
    tmp = one(img, *coeffs_h)
    return one(tmp.transpose(1, 0, 2), *coeffs_v).transpose(1, 0, 2)


def test_lanczos_tables_equal_pil_bit_for_bit():
    """(d) the three resizes of the two methods: x2 up (:527-530), the 4:3 cross back down (:701-703), /2 down (:858-860)"""
    from evoworld_amd.reprojection import resample_coeffs
    rng = np.random.default_rng(0)
    for (wi, hi), (wo, ho) in (((128, 64), (256, 128)), ((256, 128), (128, 64)), ((512, 384), (256, 192)), ((200, 100), (100, 50)),
                               ((600, 450), (200, 150))):
        img = rng.integers(0, 256, size=(hi, wi, 3), dtype=np.uint8)
        img[: hi // 4, : wi // 4] = 255                  # saturated blocks: LANCZOS over- and undershoots them, clip8 must clamp
        img[hi // 2:, wi // 2:] = 0
        want = np.asarray(Image.fromarray(img).resize((wo, ho), Image.LANCZOS))
        got = apply_tables(img, resample_coeffs(wi, wo, "lanczos"), resample_coeffs(hi, ho, "lanczos"))
        assert np.array_equal(got, want), ((wi, hi), (wo, ho), int((got != want).sum()))
    kk, _ = resample_coeffs(256, 128, "lanczos")
    assert kk.shape[1] == 13 and int(kk.min()) < 0        # support 3.0 * 2, negative lobes kept


def _bilinear_tables_before(in_size, out_size):
    """resample_coeffs as it was before it took a filter argument (the bilinear default must still produce these tables)"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)], dtype=np.float64)
        ww = w.sum()
        if ww != 0.0:
            w = w / ww
        q = w * (1 << 22)
        kk[xx, :xmax] = np.where(q < 0, q - 0.5, q + 0.5).astype(np.int64)
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def test_bilinear_tables_unchanged():
    from evoworld_amd.reprojection import resample_coeffs
    for i, o in ((1000, 576), (2000, 1024)):
        kk0, b0 = _bilinear_tables_before(i, o)
        for tables in (resample_coeffs(i, o), resample_coeffs(i, o, "bilinear")):
            assert np.array_equal(tables[0].numpy(), kk0) and np.array_equal(tables[1].numpy(), b0)
    with pytest.raises(KeyError):
        resample_coeffs(10, 5, "bicubic")


def index_faces(res):
    v, u = np.mgrid[0:res, 0:res]
    k = v * res + u
    return {n: np.stack([np.full_like(k, i + 1), k & 255, k >> 8], -1).astype(np.uint8) for i, n in enumerate(FACE_NAMES)}


def test_cubemap2equi_lut_equals_reference_run(gold):
    """(c) the host LUT, applied in numpy to the index-encoded faces, is the reference's panorama -- every pixel, the black ones
    of the dict without 'top' included"""
    from evoworld_amd.reprojection import FACE_ORDER, build_cubemap2equi_lut
    for tag in ("r64", "r32", "r64_notop"):
        w, h, s = (int(v) for v in gold[f"c_{tag}_size"])
        assert s == 1
        res = int(gold[f"c_{tag}_res"])
        faces, have = index_faces(res), set(gold[f"c_{tag}_order"].tolist())
        stack = np.stack([faces[n] if n in have else np.zeros_like(faces[n]) for n in FACE_ORDER])
        lut = build_cubemap2equi_lut(w, h, res).numpy().astype(np.int64)
        assert lut.shape == (h, w, 3) and lut.dtype == np.int64
        got = stack[lut[..., 0], lut[..., 1], lut[..., 2]]
        want = gold[f"c_{tag}_pano"]
        assert np.array_equal(got, want), (tag, int((got != want).any(-1).sum()))
    assert (gold["c_r64_notop_pano"].sum(-1) == 0).sum() > 1000       # the missing face really is a large black area


def test_rotation_matrix(gold):
    from evoworld_amd.inference import Navigator
    R = Navigator.precompute_rotation_matrix(90, -90, 180)
    assert R.dtype == np.float64 and R.shape == (3, 3)
    assert np.abs(R - gold["e_rotation_90_m90_180"]).max() <= 1e-15
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15


def test_non_2_to_1_panorama_is_refused():
    """a 1024x576 model frame is not 2:1: the reference's assertion and message (:534-535), before any device work"""
    from evoworld_amd import reprojection as RP
    frames = torch.zeros(1, 576, 1024, 3, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="Panorama width must be twice the height."):
        RP.panorama_to_cubemap(frames)
    from evoworld_amd.inference import Navigator
    assert "resize" in Navigator.convert_panorama_to_cubemap.__doc__
    for name in ("convert_panorama_to_cubemap", "precompute_rotation_matrix", "cubemap_to_equirectangular"):
        assert callable(getattr(Navigator, name))


def test_cross_faces_are_the_reference_crops():
    from evoworld_amd.reprojection import CUBEMAP_FACE_NAMES, cross_faces
    E = 4
    cross = torch.arange(2 * 3 * E * 4 * E * 3, dtype=torch.int32).reshape(2, 3 * E, 4 * E, 3)
    faces = cross_faces(cross)
    assert list(faces) == list(CUBEMAP_FACE_NAMES) == FACE_NAMES
    boxes = {"right": (3 * E, E), "left": (E, E), "top": (2 * E, 0), "bottom": (2 * E, 2 * E), "front": (2 * E, E), "back": (0, E)}   # :674-687
    for n, (x1, y1) in boxes.items():
        assert torch.equal(faces[n], cross[:, y1:y1 + E, x1:x1 + E])


def test_cli_arguments():
    from evoworld_amd.cubemap import parse_args
    a = parse_args(["to-cubemap", "--input", "in", "--output", "out"])
    assert (a.command, a.input, a.output, a.scale_factor, a.nearest, a.size) == ("to-cubemap", "in", "out", 2, False, None)
    a = parse_args(["to-cubemap", "--input", "in", "--output", "out", "--scale_factor", "1", "--nearest", "--size", "1024", "512"])
    assert (a.scale_factor, a.nearest, a.size) == (1, True, [1024, 512])
    b = parse_args(["to-pano", "--input", "in", "--output", "out", "--size", "512", "256"])
    assert (b.command, b.size, b.scale_factor) == ("to-pano", [512, 256], 2)
    with pytest.raises(SystemExit):
        parse_args(["to-pano", "--input", "in", "--output", "out"])              # --size is required
    with pytest.raises(SystemExit):
        parse_args(["to-cubemap", "--input", "in", "--output", "out", "--scale_factor", "0"])


def test_cli_file_discovery(tmp_path):
    from evoworld_amd.cubemap import face_stems, panorama_stems
    for f in ("001.png", "002.png", "001_cubemap.png", "notes.txt"):
        (tmp_path / f).write_bytes(b"")
    for n in FACE_NAMES:
        (tmp_path / f"001_{n}.png").write_bytes(b"")
    (tmp_path / "002_right.png").write_bytes(b"")                                # incomplete set
    assert panorama_stems(str(tmp_path)) == ["001", "002"]
    assert face_stems(str(tmp_path)) == ["001"]
