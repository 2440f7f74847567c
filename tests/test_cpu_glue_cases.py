"""-m "not gpu": what tests/test_gpu_glue_kernels.py rests on, checked without a GPU (tests/glue_cases.py holds the tables).

1. every *_2pass case exceeds its launch's block cap and its second grid-stride trip covers the image / frame / plane / channel /
   view boundary the table claims;
2. the references agree with independent statements (bicubic restatement against torch's fp32 F.interpolate, blur against a double
   loop, patchify against explicit indexing);
3. an fp32 numpy emulation of each kernel's arithmetic passes the very check functions the GPU test uses (the bounds are
   conditions on the reference side alone, so they must hold for any correct fp32 evaluation);
4. deliberately wrong restatements fail them on the same inputs, so the inputs discriminate."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as G
from kernel_checks import pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# block caps of the grid-stride launches (blocks of 256 threads)
CAP = {
    "ew": 4096,       # elementwise.hip grid_for(): layout forward / split / backward, ew_euler_cfg_step(_split)
    "tconv": 16384,   # elementwise.hip ew_time_conv3_f32(): `if (blocks > 16384) blocks = 16384`, one four-pixel group per thread
    "geom": 8192,     # geometry.hip grid_for(): ew_plucker_embed, ew_depth_unproject
    "clip": 8192,     # clip.hip ew_blur_axis_f32(), ew_bicubic_resize_f32(), ew_vit_patchify_f16(): `if (b > 8192) b = 8192`
}
PAT = [pattern(torch.float16, k) for k in (0, 1)]


def _small(cases):
    return [c for c in cases if not c["name"].endswith("_2pass")]


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ 1. caps and second trips
def test_caps_match_the_sources():
    def src(name):
        with open(os.path.join(ROOT, "evoworld_amd", "csrc", name)) as f:
            return f.read()
    ew, geom, clip = src("elementwise.hip"), src("geometry.hip"), src("clip.hip")
    assert re.search(r"inline int grid_for\(long long n\).*b < 4096 .* : 4096\)", ew)
    assert "if (blocks > 16384) blocks = 16384;" in ew
    assert re.search(r"inline int grid_for\(long long n\).*b < 8192 .* : 8192\)", geom)
    assert clip.count("if (b > 8192) b = 8192;") == 3


def test_every_2pass_case_has_a_claim():
    names = {c["name"] for c in G.all_cases() if c["name"].endswith("_2pass")}
    assert names == {c[0] for c in G.second_pass_claims()} and len(names) == 12
    assert len({c["name"] for c in G.all_cases()}) == len(G.all_cases())


@pytest.mark.parametrize("name,kind,total,unit,first,last", G.second_pass_claims(), ids=[c[0] for c in G.second_pass_claims()])
def test_second_trip_covers_the_claimed_boundary(name, kind, total, unit, first, last):
    start = CAP[kind] * G.THREADS                      # first work item of the second trip
    assert total > start
    assert total <= 2 * start                          # (two trips, not three: the claim is about the second)
    assert start // unit == first and (total - 1) // unit == last, (start // unit, (total - 1) // unit)


def test_second_trip_details():
    by = {c["name"]: c for c in G.all_cases()}
    c = by["tconv_2pass"]
    start = CAP["tconv"] * G.THREADS
    hq = c["HW"] // 4
    assert start // hq == 19 and 19 % c["T"] == c["T"] - 2 and 20 % c["T"] == c["T"] - 1 and 20 // c["T"] == c["B"] - 1    # frame 20: t = T - 1
    assert 0 < start % hq < hq                         # the trip starts inside frame 19 (whose kt = 2 tap is frame 20) and then covers frame 20
    for a in (0, 1):
        c = by[f"blur-axis{a}_2pass"]
        row = (CAP["clip"] * G.THREADS - 4 * c["H"] * c["W"]) // c["W"]
        assert 0 < row < c["H"] - c["ksize"] // 2      # the second trip holds the last plane's last rows: the reflect at H - 1 / the full width
    c = by["bwd_2pass"]
    assert c["N"] * c["H"] * c["W"] * c["C"] >= 63488


def test_layout_inputs_hold_what_they_claim():
    pats = set(G.finite_f16_patterns().tolist())
    assert len(pats) == 63488
    x = G.layout_bwd_input(next(c for c in G.LAYOUT_BWD if c["name"] == "bwd_2pass"))
    seen = set(np.unique(x[:, :3].contiguous().view(torch.int16).numpy().view(np.uint16)).tolist())
    assert seen == pats                                # every finite fp16 bit pattern, and no inf / NaN
    assert bool(torch.isfinite(x.float()).all())
    case = next(c for c in G.LAYOUT_FWD if c["name"] == "split-c14")
    ref = G.layout_fwd_ref(case, G.layout_fwd_input(case))
    hi = ref["hi"].float()
    assert bool(torch.isinf(hi).any()) and bool((hi == 65504).any())                      # 65520 -> inf, 65519 -> 65504
    assert bool(((hi != 0) & (hi.abs() < 2.0 ** -14)).any())                               # fp16 subnormals
    hb = G.bits(ref["hi"])
    assert bool((hb == -32768).any()) and bool((hb == 0).any())                            # -0 and +0


# ------------------------------------------------------------------------------------------------ 2. references cross-checked
@pytest.mark.parametrize("H,W,Ho,Wo", G.BICUBIC_SHAPES + [(64, 64, 840, 840)])
def test_bicubic_restatement_matches_torch_fp32(H, W, Ho, Wo):
    case = dict(name=f"x-{H}x{W}-{Ho}x{Wo}", N=1, C=2, H=H, W=W, Ho=Ho, Wo=Wo, affine=False)
    x, _, _ = G.bicubic_input(case)
    want = F.interpolate(x, size=(Ho, Wo), mode="bicubic", align_corners=True)
    got, _ = G.bicubic_apply(case, x, None, None)
    d = float((got - want.double()).abs().max())
    print(f"bicubic restatement vs torch fp32 {H}x{W}->{Ho}x{Wo}: {d:.2e}")
    assert d < 3e-5                                    # the existing resize test's number


def test_blur_reference_matches_a_double_loop():
    for case in G.BLUR_CASES:
        if case["ksize"] in (4, 7) and case["H"] * case["W"] <= 25:
            x, kern = G.blur_input(case)
            ref, _ = G.blur_apply(x, kern, case["axis"])
            assert float((ref - G.blur_double_loop(x, kern, case["axis"])).abs().max()) < 1e-13, case["name"]


def test_blur_cases_are_the_shapes_the_kernel_accepts():
    for case in _small(G.BLUR_CASES):
        n = case["H"] if case["axis"] == 0 else case["W"]
        assert case["ksize"] // 2 < n


def test_patchify_reference_matches_explicit_indexing():
    for case in G.PATCHIFY_CASES[:4]:
        x = G.patchify_input(case)
        assert torch.equal(G.patchify_ref(case, x), G.patchify_explicit(case, x)), case["name"]


# ------------------------------------------------------------------------------------------------ 3. fp32 emulations pass the checks
@pytest.mark.parametrize("case", _small(G.EULER_CASES), ids=lambda c: c["name"])
def test_euler_emulation_is_inside_the_bounds(case):
    eps, lat, guid = G.euler_input(case)
    for p in PAT:
        lat_new, rows = G.euler_emulate(case, eps, lat, guid, p)
        G.check_euler(case, lat_new, rows, eps, lat, guid, p)


def test_time_conv3_emulation_is_inside_the_bound():
    for case in _small(G.TCONV_CASES):
        x, w, b = G.tconv_input(case)
        G.check_tconv(case, G.tconv_emulate(x, w, b), x, w, b)


def test_blur_emulation_is_inside_the_bound():
    for case in _small(G.BLUR_CASES):
        x, kern = G.blur_input(case)
        G.check_blur(case, G.blur_apply(x, kern, case["axis"], dtype=torch.float32)[0], x, kern)


@pytest.mark.parametrize("case", G.BICUBIC_CASES, ids=lambda c: c["name"])
def test_bicubic_emulation_is_inside_the_bound(case):
    x, scale, shift = G.bicubic_input(case)
    out, _ = G.bicubic_apply(case, x, scale, shift, dtype=np.float32)
    assert out.dtype == torch.float32
    G.check_bicubic(case, out, x, scale, shift)


def test_layout_and_patchify_restatements_pass_their_checks():
    for case in _small(G.LAYOUT_FWD):
        x = G.layout_fwd_input(case)
        for p in PAT:
            G.check_layout_fwd(case, G.layout_fwd_emulate(case, x, p), x, p)
    for case in G.PATCHIFY_CASES[:4]:
        x = G.patchify_input(case)
        G.check_patchify(case, G.patchify_explicit(case, x), x)


# ------------------------------------------------------------------------------------------------ 4. wrong restatements fail
def _blur_wrong(kw):
    def one(case):
        x, kern = G.blur_input(case)
        try:
            out = G.blur_apply(x, kern, case["axis"], dtype=torch.float32, **kw(case))[0]
        except RuntimeError:                           # torch refuses a reflect padding as wide as the axis: this variant cannot state the case
            return
        G.check_blur(case, out, x, kern)
    return lambda: [_fails(lambda c=c: one(c)) for c in _small(G.BLUR_CASES)]


def _bicubic_wrong(**kw):
    def one(case):
        x, scale, shift = G.bicubic_input(case)
        G.check_bicubic(case, G.bicubic_apply(case, x, scale, shift, dtype=np.float32, **kw)[0], x, scale, shift)
    return lambda: [_fails(lambda c=c: one(c)) for c in _small(G.BICUBIC_CASES)]


def _patchify_wrong():
    def one(case):
        x = G.patchify_input(case)
        G.check_patchify(case, G.patchify_ref(case, x, k_order="ky,kx,c"), x)
    return [_fails(lambda c=c: one(c)) for c in G.PATCHIFY_CASES[:4]]


def _tconv_wrong():
    def one(case):
        x, w, b = G.tconv_input(case)
        G.check_tconv(case, G.tconv_emulate(x, w, b, pad_from_neighbour=True), x, w, b)
    return [_fails(lambda c=c: one(c)) for c in _small(G.TCONV_CASES)]


def _layout_wrong():
    def one(case):
        x = G.layout_fwd_input(case)
        G.check_layout_fwd(case, G.layout_fwd_emulate(case, x, PAT[0], lo_ignores_c_off=True), x, PAT[0])
    return [_fails(lambda c=c: one(c)) for c in _small(G.LAYOUT_FWD)]


def _euler_wrong():
    def one(case):
        eps, lat, guid = G.euler_input(case)
        lat_new, rows = G.euler_emulate(case, eps, lat, guid, PAT[0], guidance_by_pixel=True)
        G.check_euler(case, lat_new, rows, eps, lat, guid, PAT[0])
    return [_fails(lambda c=c: one(c)) for c in _small(G.EULER_CASES)]


WRONG = {
    "blur, kernel flipped": _blur_wrong(kw=lambda c: dict(flip=True)),
    "blur, pad_front = ksize // 2": _blur_wrong(kw=lambda c: dict(pad_front=c["ksize"] // 2)),
    "blur, edge repeat instead of reflect": _blur_wrong(kw=lambda c: dict(mode="replicate")),
    "bicubic, align_corners=False coordinates": _bicubic_wrong(align_corners=False),
    "bicubic, affine indexed by pl // C": _bicubic_wrong(affine_by_image=True),
    "patchify, K order (ky, kx, c)": _patchify_wrong,
    "time_conv3, padding read from the neighbouring batch": _tconv_wrong,
    "layout, c_off ignored in the lo block": _layout_wrong,
    "Euler, guidance indexed by pixel": _euler_wrong,
}


@pytest.mark.parametrize("what", list(WRONG), ids=list(WRONG))
def test_wrong_restatement_fails_at_least_one_case(what):
    failed = WRONG[what]()
    print(f"{what}: fails {sum(failed)} of {len(failed)} cases")
    assert any(failed)
