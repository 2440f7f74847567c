"""-m gpu: the image kernels of the reprojection / frame-I/O path against references that need no GPU, bit for bit.

What each test pins (kernel path in brackets):
- test_equi2pers_every_pixel: ew_equi2pers with pitch, roll, the pole clamp (uj clamp, y1 = He - 1) and the longitude seam (x1
  wrap) on a panorama that is periodic in longitude, against the float64 oracle: every pixel within 1 of floor(ref), and equal
  to it wherever the float64 value is E2P_DELTA away from an integer (reproject_cases.py: measured between two references).
- test_f32_to_u8_*: ew_f32_chw_to_u8_hwc's round-half-even, clamp, +-inf and NaN on the vector path (H*W % 4 == 0) and the
  scalar path (H*W % 4 == 2), at four alignments of the data against the 4-pixel packing, and at the product shape.
- test_u8_to_f32_all_levels / test_u8_f32_u8_identity: ew_u8_hwc_to_f32_chw on all 256 levels at each of the 12 byte positions of
  the 4-pixel packing, both paths, and the u8 -> f32 -> u8 identity the episode loop relies on.
- test_resize_routing_seams: ew_resize_aa_u8 against Pillow at the seams of its routing (LDS row pass at exactly 60 KB and just
  above, generic horizontal + dword vertical, unaligned base pointers, upscale, unchanged axis), tmp and dst guarded.
Outputs live in Guarded buffers and every call runs with two prefill patterns (kernel_checks)."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import reproject_cases as C
from kernel_checks import Guarded, assert_same_bits, pattern, two_prefills
from oracle import reproject_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ ew_equi2pers
@pytest.mark.parametrize("case", C.e2p_cases(), ids=C.e2p_case_id)
def test_equi2pers_every_pixel(case):
    from evoworld_amd.reprojection import Equi2Pers
    He, We, Hp, Wp, fov, rots = case
    img = R.smooth_pano(He, We)
    equi = np.ascontiguousarray(np.broadcast_to(img[None], (len(rots),) + img.shape))
    e2p = Equi2Pers(Hp, Wp, fov)
    got = e2p.batch(torch.from_numpy(equi).to(DEV), rots).cpu().numpy().astype(np.int64)
    ref = R.equi2pers_ref(equi, np.stack([e2p.rotation(r) for r in rots]), Hp, Wp, fov)
    want = np.floor(ref).astype(np.int64)
    dec = C.e2p_decidable(ref)
    off = np.abs(got - want)
    wrong = (got != want) & dec
    print(f"E2P {C.e2p_case_id(case)}: max |got - floor(ref)| {int(off.max())}, differing {int((off > 0).sum())} of {off.size} "
          f"({int(wrong.sum())} of them decidable), excluded share {1 - dec.mean():.4f}")
    assert 1.0 - dec.mean() <= C.E2P_MAX_EXCLUDED
    if off.max() > 1:                                                   # (a) every pixel, seam and poles included
        i = tuple(int(v) for v in np.argwhere(off > 1)[0])
        raise AssertionError(f"view {rots[i[0]]} pixel {i[1:]}: got {got[i]}, float64 reference {ref[i]:.4f}; {int((off > 1).sum())} such")
    if wrong.any():                                                     # (b) exact wherever float32 coordinates cannot decide it
        i = tuple(int(v) for v in np.argwhere(wrong)[0])
        raise AssertionError(f"view {rots[i[0]]} pixel {i[1:]}: got {got[i]}, float64 reference {ref[i]:.4f} (delta {C.E2P_DELTA}); "
                             f"{int(wrong.sum())} such")


# ------------------------------------------------------------------------------------------------ ew_f32_chw_to_u8_hwc
_NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)


def _quant_case(x_chw):
    """x_chw float32 [V,3,H,W] (numpy) through the ABI into a guarded [V,H,W,3], two prefills; compared with f32_to_u8_ref
    everywhere except at NaN inputs, which must only be written in bounds and identically."""
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    V, _, H, W = x_chw.shape
    src = torch.from_numpy(x_chw).to(DEV)

    def run(o, k):
        _lib.check(lib.ew_f32_chw_to_u8_hwc(_p(src), _p(o), V, H, W, ops._stream()), "ew_f32_chw_to_u8_hwc")
    g = two_prefills(run, (V * H * W, 3, torch.uint8, dict(ld=3, pad_rows=1024)))[0]
    got = g.view.cpu().numpy().reshape(V, H, W, 3)
    nan = np.isnan(x_chw)
    want, scaled = R.f32_to_u8_ref(np.where(nan, np.float32(0), x_chw))
    want, nan = want.transpose(0, 2, 3, 1), nan.transpose(0, 2, 3, 1)
    bad = (got != want) & ~nan
    if bad.any():
        v, y, x, c = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"[{v},{c},{y},{x}] x = {x_chw[v, c, y, x]!r} (scaled {scaled[v, c, y, x]!r}): got {got[v, y, x, c]}, "
                             f"want {want[v, y, x, c]}; {int(bad.sum())} such")
    return scaled[~np.isnan(x_chw)]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("H,W", [(218, 1024), (218, 1025)], ids=["vec4", "scalar"])
def test_f32_to_u8_half_even_clamp_and_edges(H, W, shift):
    """[3,3,218,1024]: H*W % 4 == 0, the 4-pixel path; [3,3,218,1025]: H*W % 4 == 2, the scalar path.  `shift` moves the same
    values to the next position of the 4-pixel packing."""
    assert (H * W) % 4 == (0 if W == 1024 else 2)
    x = np.concatenate([np.zeros(shift, np.float32), C.quant_inputs(), _NANS])
    n = 3 * 3 * H * W
    assert n >= x.size
    scaled = _quant_case(np.resize(x, n).reshape(3, 3, H, W))
    ties = C.count_exact_ties(scaled)
    print(f"QUANT {H}x{W} shift {shift}: {ties} exact ties")
    assert ties >= C.QUANT_MIN_TIES                                     # the half-even rule is really exercised


def test_f32_to_u8_small_scalar_shape():
    """57 x 102 (H*W % 4 == 2) with the midpoints, their neighbours and the edges only"""
    x = np.concatenate([C.quant_inputs()[:255 * 3 + 16], _NANS])
    scaled = _quant_case(np.resize(x, 3 * 3 * 57 * 102).reshape(3, 3, 57, 102))
    assert C.count_exact_ties(scaled) >= C.QUANT_MIN_TIES


def test_f32_to_u8_product_shape():
    """25 x 576 x 1024, the decoded segment handed to the next one"""
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(25, 3, 576, 1024, generator=g) * 2.2 - 1.1).numpy()
    q = C.quant_inputs()
    x.reshape(-1)[:q.size] = q
    x.reshape(-1)[-q.size:] = q
    _quant_case(x)


# ------------------------------------------------------------------------------------------------ ew_u8_hwc_to_f32_chw
def _levels(V, H, W):
    """uint8 [V,H,W,3] in which each of the 12 byte positions of a 4-pixel group sees all 256 levels"""
    i = np.arange(V * H * W * 3, dtype=np.int64)
    return ((i // 12 + (i % 12) * 21) % 256).astype(np.uint8).reshape(V, H, W, 3)


@pytest.mark.parametrize("H,W", [(32, 44), (57, 102)], ids=["vec4", "scalar"])
def test_u8_to_f32_all_levels(H, W):
    from evoworld_amd import _lib, ops
    lib = _lib.load()
    V = 3
    x = _levels(V, H, W)
    seen = np.zeros((12, 256), bool)
    seen[np.arange(x.size) % 12, x.reshape(-1)] = True
    assert seen.all()
    src = torch.from_numpy(x).to(DEV)

    def run(o, k):
        _lib.check(lib.ew_u8_hwc_to_f32_chw(_p(src), _p(o), V, H, W, ops._stream()), "ew_u8_hwc_to_f32_chw")
    g = two_prefills(run, (V * 3, H * W, torch.float32, dict(ld=H * W, pad_rows=2)))[0]
    want = (torch.from_numpy(x).permute(0, 3, 1, 2).float() / 255) * 2 - 1
    assert torch.equal(g.view.cpu().reshape(V, 3, H, W), want)


@pytest.mark.parametrize("H,W", [(32, 44), (57, 102)], ids=["vec4", "scalar"])
def test_u8_f32_u8_identity(H, W):
    from evoworld_amd import ops
    x = torch.from_numpy(_levels(3, H, W)).to(DEV)
    assert torch.equal(ops.f32_chw_to_u8_hwc(ops.u8_hwc_to_f32_chw(x)), x)


# ------------------------------------------------------------------------------------------------ ew_resize_aa_u8
class _ByteBuf:
    """n bytes at `offset` bytes past a 256-byte aligned base, with guard bytes before and after"""

    def __init__(self, n, offset, prefill):
        self.n, self.offset = n, offset
        self.g = Guarded(1, offset + n, torch.uint8, ld=offset + n, pad_rows=1, prefill=prefill, device=DEV)
        self.pat = pattern(torch.uint8, prefill)
        self.ptr = ctypes.c_void_p(self.g.buf.data_ptr() + offset)

    def data(self):
        return self.g.buf[self.offset: self.offset + self.n]

    def check(self):
        self.g.check()
        assert bool((self.g.buf[: self.offset] == self.pat).all()), "guard: bytes before the buffer written"


# (Hi, Wi, Ho, Wo, byte offset of src / tmp / dst, horizontal pass, vertical pass): the passes follow from the conditions in
# ew_resize_aa_u8 -- LDS row pass iff aligned, Wi*3 % 4 == 0, Wo % 4 == 0 and Wi*3 <= 60 KB; dword vertical iff aligned, Wo*3 % 4 == 0
_RESIZE = [
    (33, 77, 33, 20, 0, "generic", "dword"),          # Wi*3 % 4 == 3, Wo % 4 == 0
    (8, 20480, 8, 1024, 0, "lds", "dword"),           # Wi*3 == 61440 == 60 KB exactly
    (8, 20484, 8, 1024, 0, "generic", "dword"),       # Wi*3 == 61452: just over
    (50, 100, 73, 131, 0, "generic", "generic"),      # upscale on both axes, odd output sizes
    (100, 200, 100, 104, 0, "lds", "dword"),          # one axis unchanged
    (40, 200, 30, 104, 1, "generic", "generic"),      # the LDS + dword shape, every base pointer 1 byte past a 4-byte boundary
]


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,off,hpass,vpass", _RESIZE, ids=[f"{c[0]}x{c[1]}-{c[2]}x{c[3]}+{c[4]}" for c in _RESIZE])
def test_resize_routing_seams(Hi, Wi, Ho, Wo, off, hpass, vpass):
    from evoworld_amd import _lib, ops
    from evoworld_amd import reprojection as RP
    lib = _lib.load()
    al = off % 4 == 0
    assert hpass == ("lds" if al and (Wi * 3) % 4 == 0 and Wo % 4 == 0 and Wi * 3 <= 60 * 1024 else "generic")
    assert vpass == ("dword" if al and (Wo * 3) % 4 == 0 else "generic")
    V = 3
    rng = np.random.default_rng(Hi * 7 + Wi)
    imgs = rng.integers(0, 256, size=(V, Hi, Wi, 3), dtype=np.uint8)
    want = np.stack([np.array(Image.fromarray(imgs[v]).resize((Wo, Ho), Image.BILINEAR)) for v in range(V)])
    (kh, bh), (kv, bv) = [tuple(t.to(DEV) for t in RP.resample_coeffs(a, b)) for a, b in ((Wi, Wo), (Hi, Ho))]
    outs = []
    for k in (0, 1):
        src, tmp, dst = _ByteBuf(imgs.size, off, k), _ByteBuf(V * Hi * Wo * 3, off, k), _ByteBuf(V * Ho * Wo * 3, off, k)
        src.data().copy_(torch.from_numpy(imgs).reshape(-1))
        assert (src.ptr.value % 4 == 0) == al
        st = lib.ew_resize_aa_u8(src.ptr, tmp.ptr, dst.ptr, _p(kh), _p(bh), kh.shape[1], _p(kv), _p(bv), kv.shape[1], V, Hi, Wi, Ho, Wo,
                                 ops._stream())
        if st != 0 and hpass == "lds" and Wi * 3 == 60 * 1024:
            # a runtime that refuses the 60 KB dynamic-LDS launch must say so: a clean error, never wrong pixels
            msg = lib.ew_last_error()
            print(f"RESIZE {Wi}: launch refused: {msg!r}")
            assert msg and b"ew_resize_aa_u8" in msg
            torch.cuda.synchronize()
            return
        _lib.check(st, "ew_resize_aa_u8")
        torch.cuda.synchronize()
        for b in (src, tmp, dst):
            b.check()
        assert np.array_equal(src.data().cpu().numpy(), imgs.reshape(-1))
        got = dst.data().cpu().numpy().reshape(V, Ho, Wo, 3)
        bad = got != want
        if bad.any():
            i = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError(f"{hpass} horizontal / {vpass} vertical: first difference at {i}: got {got[i]}, Pillow {want[i]}; "
                                 f"{int(bad.sum())} such")
        outs.append((tmp.data().clone(), dst.data().clone()))
    assert_same_bits(outs[0][0], outs[1][0], "tmp")
    assert_same_bits(outs[0][1], outs[1][1], "dst")
