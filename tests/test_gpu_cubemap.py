"""-m gpu: panorama <-> cubemap on the device (ew_equi2cube_u8, the LANCZOS tables through ew_resize_aa_u8, the cubemap LUT through
ew_cube2equi_gather, Navigator's three methods, the CLI) against a run of the reference's own convert_panorama_to_cubemap /
cubemap_to_equirectangular (tests/golden/cubemap.npz, tools/make_goldens_cubemap.py).

Bounds.  Nearest mode, the gather and the resizes are integer paths: bit-exact.  Bilinear: bit-exact on every pixel the generator
did not mask; a masked pixel (uf or vf within 1e-9 of an integer, or the float64 blend within 1e-6 of one before truncation) may
differ by one level, because the device evaluates atan2 / hypot itself and may differ from the host libm in the last place.
Masked shares the generator measured (coordinate criterion, share of used cross pixels): 2.59 % at W = 512, 0.65 % at 2048,
0.33 % at 4096, 5.14 % at W = 256; nearest mode has 0 pixels within 1e-9 of a half-integer at 512 / 2048 / 4096.  With the blend
criterion added: noise 5.35 %, smooth 18.25 % (W = 256), plateau 74.29 % (256 x2) and 96.92 % (512 x1) -- on a flat area the
blend IS an integer up to rounding, which is where truncation yields A - 1; those pixels are checked to one level, and both the
golden and the device output must contain A - 1 pixels (a rounding implementation yields none)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN
from kernel_checks import Guarded, assert_same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACE_NAMES = ["right", "left", "top", "bottom", "front", "back"]
CELLS = {"right": (3, 1), "left": (1, 1), "top": (2, 0), "bottom": (2, 2), "front": (2, 1), "back": (0, 1)}       # (column, row)
A_CASES = [("noise_128_s2", 2), ("smooth_128_s2", 2), ("plateau_256_s2", 2), ("plateau_512_s1", 1)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "cubemap.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def index_pano(w):
    y, x = np.mgrid[0:w // 2, 0:w]
    return np.stack([x & 255, y & 255, (x >> 8) | ((y >> 8) << 4)], -1).astype(np.uint8)


def index_faces(res):
    v, u = np.mgrid[0:res, 0:res]
    k = v * res + u
    return {n: np.stack([np.full_like(k, i + 1), k & 255, k >> 8], -1).astype(np.uint8) for i, n in enumerate(FACE_NAMES)}


def cross_of(faces6):
    """the scaled cross [3E,4E,3] the reference cut its faces from: the six faces in their cells, black elsewhere"""
    E = faces6.shape[1]
    cross = np.zeros((3 * E, 4 * E, 3), np.uint8)
    for k, n in enumerate(FACE_NAMES):
        c, r = CELLS[n]
        cross[r * E:(r + 1) * E, c * E:(c + 1) * E] = faces6[k]
    return cross


def used_cells(E):
    m = np.zeros((3 * E, 4 * E), bool)
    for c, r in CELLS.values():
        m[r * E:(r + 1) * E, c * E:(c + 1) * E] = True
    return m


def scaled_cross(img, interpolation, s):
    from evoworld_amd import ops
    from evoworld_amd import reprojection as RP
    x = dev(img)[None]
    return ops.equi2cube(RP.resize_u8(x, img.shape[0] * s, img.shape[1] * s, "lanczos"), interpolation)[0].cpu().numpy()


@pytest.mark.parametrize("tag,s", A_CASES)
def test_nearest_cross_faces_and_cubemap_bit_exact(gold, tag, s):
    from evoworld_amd.inference import Navigator
    img = gold[f"a_{tag}_input"]
    cubemap, faces = Navigator.convert_panorama_to_cubemap(dev(img), interpolation=False, scale_factor=s)
    assert list(faces) == FACE_NAMES
    want = gold[f"a_{tag}_nearest_faces"]
    for k, n in enumerate(FACE_NAMES):
        assert np.array_equal(faces[n].cpu().numpy(), want[k]), (tag, n)
    cross = scaled_cross(img, False, s)
    assert np.array_equal(cross, cross_of(want))                                   # black cells included
    assert np.array_equal(cubemap.cpu().numpy(), gold[f"a_{tag}_nearest_cubemap"])


def test_nearest_source_indices_bit_exact(gold):
    """(b) the panorama's pixels carry their own (ui, vi): the faces spell out which source pixel every cross pixel read"""
    from evoworld_amd import ops
    W0 = 256
    cross = ops.equi2cube(dev(index_pano(W0))[None], False)[0].cpu().numpy()
    want = cross_of(gold[f"b_{W0}_faces"])
    assert np.array_equal(cross, want)
    E = W0 // 4
    black = (want.sum(-1) == 0) & used_cells(E)
    assert black.sum() >= 1                                                        # the seam pixel(s) whose column rounds to W
    ui = cross[..., 0].astype(int) | ((cross[..., 2].astype(int) & 15) << 8)
    assert ui[used_cells(E) & ~black].max() == W0 - 1


@pytest.mark.parametrize("tag,s", A_CASES)
def test_bilinear_exact_off_mask_one_level_on_it(gold, tag, s):
    img = gold[f"a_{tag}_input"]
    want = cross_of(gold[f"a_{tag}_bilinear_faces"])
    E = want.shape[0] // 3
    mask = np.unpackbits(gold[f"a_{tag}_mask"])[: 3 * E * 4 * E].reshape(3 * E, 4 * E).astype(bool)
    got = scaled_cross(img, True, s)
    diff = np.abs(got.astype(int) - want.astype(int)).max(-1)
    print(f"CUBEMAP {tag}: masked {int(mask.sum())} of {int(used_cells(E).sum())} used pixels; differing pixels {int((diff > 0).sum())} "
          f"(off the mask {int((diff[~mask] > 0).sum())}), largest difference {int(diff.max())}")
    assert (diff[~mask] == 0).all(), (tag, int((diff[~mask] > 0).sum()))
    assert diff[mask].max(initial=0) <= 1, (tag, int(diff[mask].max()))
    assert (got[~used_cells(E)] == 0).all()
    # the downscale alone is an integer path: from the reference's own scaled cross it must give the reference's cubemap
    from evoworld_amd import reprojection as RP
    W0 = img.shape[1]
    small = RP.resize_u8(dev(want)[None], int(W0 * 3 / 4), W0, "lanczos")[0].cpu().numpy()
    assert np.array_equal(small, gold[f"a_{tag}_bilinear_cubemap"])


def test_plateau_truncation_is_reproduced(gold):
    """on the flat 255 and (200, 37, 128) areas of the plateau image the reference's truncation yields 254 / 199 / 36 / 127"""
    tag, s = "plateau_512_s1", 1
    want = cross_of(gold[f"a_{tag}_bilinear_faces"])
    got = scaled_cross(gold[f"a_{tag}_input"], True, s)
    E = want.shape[0] // 3
    mask = np.unpackbits(gold[f"a_{tag}_mask"])[: 3 * E * 4 * E].reshape(3 * E, 4 * E).astype(bool)
    for level in (254, 199):
        w, g = want[..., 0] == level, got[..., 0] == level
        print(f"CUBEMAP plateau: red == {level}: golden {int(w.sum())}, device {int(g.sum())}, both {int((w & g).sum())}, golden off the mask {int((w & ~mask).sum())}")
        assert w.sum() >= 1 and g.sum() >= 1
        assert np.array_equal(w[~mask], g[~mask])


def test_lanczos_resizes_equal_pil():
    """(d) x2 up, the 4:3 cross down, /2 down -- through ew_resize_aa_u8"""
    from evoworld_amd import reprojection as RP
    rng = np.random.default_rng(1)
    for (wi, hi), (wo, ho) in (((256, 128), (512, 256)), ((512, 384), (256, 192)), ((512, 256), (256, 128)), ((200, 100), (100, 50))):
        img = rng.integers(0, 256, size=(2, hi, wi, 3), dtype=np.uint8)
        img[:, : hi // 4, : wi // 4] = 255
        img[:, hi // 2:, wi // 2:] = 0
        got = RP.resize_u8(dev(img), ho, wo, "lanczos").cpu().numpy()
        for k in range(2):
            assert np.array_equal(got[k], np.asarray(Image.fromarray(img[k]).resize((wo, ho), Image.LANCZOS))), ((wi, hi), (wo, ho))


@pytest.mark.parametrize("tag", ["r64", "r32", "r64_notop", "r64_s2"])
def test_panorama_from_faces_bit_exact(gold, tag):
    """(c) shuffled dict order, two face resolutions, a missing face (black pixels), and the LANCZOS-downscaled form"""
    from evoworld_amd.inference import Navigator
    w, h, s = (int(v) for v in gold[f"c_{tag}_size"])
    faces = index_faces(int(gold[f"c_{tag}_res"]))
    d = {n: dev(faces[n]) for n in gold[f"c_{tag}_order"].tolist()}
    pano = Navigator.cubemap_to_equirectangular(d, w, h, scale_factor=s)
    assert pano.shape == (h, w, 3) and pano.is_cuda
    assert np.array_equal(pano.cpu().numpy(), gold[f"c_{tag}_pano"])
    rev = Navigator.cubemap_to_equirectangular(dict(reversed(list(d.items()))), w, h, scale_factor=s)
    assert torch.equal(rev, pano)


def test_clip_of_25_equals_single_calls(gold):
    from evoworld_amd.inference import Navigator
    rng = np.random.default_rng(2)
    clip = dev(rng.integers(0, 256, size=(25, 64, 128, 3), dtype=np.uint8))
    for interp in (True, False):
        cm, faces = Navigator.convert_panorama_to_cubemap(clip, interpolation=interp, scale_factor=2)
        assert cm.shape == (25, 96, 128, 3) and faces["front"].shape == (25, 64, 64, 3)
        for v in range(25):
            cm1, f1 = Navigator.convert_panorama_to_cubemap(clip[v], interpolation=interp, scale_factor=2)
            assert torch.equal(cm[v], cm1)
            for n in FACE_NAMES:
                assert torch.equal(faces[n][v], f1[n])
    pano = Navigator.cubemap_to_equirectangular({n: f.contiguous() for n, f in faces.items()}, 128, 64, scale_factor=2)
    assert pano.shape == (25, 64, 128, 3)
    for v in (0, 7, 24):
        assert torch.equal(pano[v], Navigator.cubemap_to_equirectangular({n: f[v].contiguous() for n, f in faces.items()}, 128, 64, 2))


def test_pil_in_pil_out_equals_tensor_path(gold):
    from evoworld_amd.inference import Navigator
    img = gold["a_smooth_128_s2_input"]
    nav = Navigator.__new__(Navigator)                       # the methods need no pipeline
    cm_p, f_p = nav.convert_panorama_to_cubemap(Image.fromarray(img), interpolation=True, scale_factor=2)
    cm_t, f_t = nav.convert_panorama_to_cubemap(dev(img), interpolation=True, scale_factor=2)
    assert isinstance(cm_p, Image.Image) and cm_p.size == (128, 96) and list(f_p) == FACE_NAMES
    assert np.array_equal(np.asarray(cm_p), cm_t.cpu().numpy())
    for n in FACE_NAMES:
        assert isinstance(f_p[n], Image.Image) and f_p[n].size == (64, 64)
        assert np.array_equal(np.asarray(f_p[n]), f_t[n].cpu().numpy())
    pano_p = nav.cubemap_to_equirectangular(f_p, 128, 64, scale_factor=2)
    pano_t = nav.cubemap_to_equirectangular({n: f.contiguous() for n, f in f_t.items()}, 128, 64, scale_factor=2)
    assert isinstance(pano_p, Image.Image) and pano_p.size == (128, 64)
    assert np.array_equal(np.asarray(pano_p), pano_t.cpu().numpy())
    with pytest.raises(AssertionError, match="Panorama width must be twice the height."):
        nav.convert_panorama_to_cubemap(Image.new("RGB", (1024, 576)))


def test_cli_round_trip(gold, tmp_path):
    from evoworld_amd import cubemap as CLI
    from evoworld_amd.inference import Navigator
    src, mid, out = tmp_path / "panos", tmp_path / "cube", tmp_path / "back"
    src.mkdir()
    imgs = {"001": gold["a_smooth_128_s2_input"], "002": gold["a_noise_128_s2_input"]}
    for k, a in imgs.items():
        Image.fromarray(a).save(src / f"{k}.png")
    assert CLI.main(["to-cubemap", "--input", str(src), "--output", str(mid)]) == 2
    assert CLI.main(["to-pano", "--input", str(mid), "--output", str(out), "--size", "128", "64"]) == 2
    for k, a in imgs.items():
        cm, faces = Navigator.convert_panorama_to_cubemap(dev(a))
        assert np.array_equal(np.asarray(Image.open(mid / f"{k}_cubemap.png")), cm.cpu().numpy())
        for n in FACE_NAMES:
            assert np.array_equal(np.asarray(Image.open(mid / f"{k}_{n}.png")), faces[n].cpu().numpy())
        pano = Navigator.cubemap_to_equirectangular({n: f.contiguous() for n, f in faces.items()}, 128, 64)
        assert np.array_equal(np.asarray(Image.open(out / f"{k}.png")), pano.cpu().numpy())
    # the smooth panorama survives the trip closely (two resamplings each way)
    back = np.asarray(Image.open(out / "001.png")).astype(int)
    assert np.abs(back - imgs["001"].astype(int)).mean() < 8
    # a 4:3-ish frame goes through --size first
    odd = tmp_path / "odd"
    odd.mkdir()
    Image.fromarray(np.asarray(Image.fromarray(imgs["001"]).resize((128, 72)))).save(odd / "001.png")
    assert CLI.main(["to-cubemap", "--input", str(odd), "--output", str(tmp_path / "odd_out"), "--size", "128", "64", "--nearest",
                     "--scale_factor", "1"]) == 1
    assert Image.open(tmp_path / "odd_out" / "001_front.png").size == (32, 32)


@pytest.mark.parametrize("interp", [True, False])
def test_no_write_outside_the_cross(interp):
    from evoworld_amd import ops
    rng = np.random.default_rng(3)
    V, H, W = 3, 64, 128
    x = dev(rng.integers(0, 256, size=(V, H, W, 3), dtype=np.uint8))
    outs = []
    for prefill in (0, 1):
        g = Guarded(V * 3 * (W // 4), W * 3, torch.uint8, ld=W * 3, pad_rows=64, prefill=prefill, device=DEV)
        ops.equi2cube(x, interp, out=g.view.view(V, 3 * (W // 4), W, 3))
        torch.cuda.synchronize()
        g.check()
        outs.append(g.view)
    assert_same_bits(outs[0], outs[1], "cross")                    # every byte written, none read back
    assert torch.equal(outs[0].view(V, 3 * (W // 4), W, 3), ops.equi2cube(x, interp))


def test_product_size_structure_and_determinism():
    """2048x1024, scale_factor 2 -> an edge-1024 cross (device only: the reference takes seconds per frame on the host)"""
    from evoworld_amd.inference import Navigator
    y, x = np.mgrid[0:1024, 0:2048]
    img = dev(np.stack([(x * 7 + y * 3) % 256, (x + y * 5) % 251, (x ^ y) % 256], -1).astype(np.uint8))
    cm, faces = Navigator.convert_panorama_to_cubemap(img, interpolation=True, scale_factor=2)
    cm2, faces2 = Navigator.convert_panorama_to_cubemap(img, interpolation=True, scale_factor=2)
    E = 1024
    assert cm.shape == (1536, 2048, 3) and all(f.shape == (E, E, 3) for f in faces.values())
    assert torch.equal(cm, cm2) and all(torch.equal(faces[n], faces2[n]) for n in FACE_NAMES)
    cross = faces["front"]._base if faces["front"]._base is not None else None
    assert cross is not None and cross.shape[-3:] == (3 * E, 4 * E, 3)       # the faces are views of one cross
    cross = cross.reshape(3 * E, 4 * E, 3)
    for n, (c, r) in CELLS.items():
        assert torch.equal(faces[n], cross[r * E:(r + 1) * E, c * E:(c + 1) * E])
    for r in (0, 2):
        for c in (0, 1, 3):
            assert int(cross[r * E:(r + 1) * E, c * E:(c + 1) * E].max()) == 0
    assert all(int(f.max()) > 0 for f in faces.values())
