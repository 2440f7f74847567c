"""-m gpu: the device MJPEG decoder (csrc/video_decode.hip: ew_jpeg_huffman_decode, ew_jpeg_idct, ew_jpeg_planes_to_rgb, ew_resize_linear_u8
through ops.* and evoworld_amd.video.decode_jpeg / read_video / the extract and scores commands) against the oracle
tests/jpeg_decode_ref.py on the inputs of tests/video_cases.py, against the device encoder, and against libjpeg (Pillow).  DESIGN.md 4.6.

Coefficients are exact: the decoder returns what the encoder quantised, the encoder's entropy coder turns them back into the same
bytes, and on streams of another encoder (Pillow: default, fitted Huffman tables, restart intervals of a row and of 3 MCUs, none) they
equal the plain-Python decoder's.
Samples and pixels: a device value may differ from the float64 oracle's by exactly 1, only where the oracle's unrounded value lies
within 1e-3 of a half-integer, and such places are at most 1 % of a case (tests/test_cpu_video_decode.py asserts the share, and that the
float32 error bound of the inverse DCT stays below the window, on the oracle alone).  The RGB stage is compared with the oracle applied
to the device's own planes.  synth_zrl_24x136 is left out of both: its samples sit on half-integers by construction (1.5 % / 1.1 % in
the window).
libjpeg: PSNR(device decode, source) >= PSNR(Pillow's decode of the same bytes, source) - PSNR_SLACK, twice the largest shortfall
measured on an MI355X over the cases of this file with a floor of 0.05 dB (DESIGN.md 4.6 holds the table).
Every kernel output of the case table is written between guard bands that must stay intact, also for damaged streams."""
import io
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_decode_ref as D
import jpeg_ref as J
import video_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
PSNR_SLACK = 0.101          # dB: max(2 * the largest measured shortfall (0.0504, ramp_40x72 at 4:4:4, frame 1), the floor 0.05)
GUARD = 65536               # elements in front of and behind every output: more than one restart segment's worth in each of them
ALL = [(n, s) for n in C.CASES for s in C.SUBSAMPLINGS]
PIXELS = [(n, s) for n, s in ALL if n != "synth_zrl_24x136"]
_device = {}


def _guarded(shape, dtype):
    """(buffer, view): a tensor of `shape` between two guard bands holding a pattern"""
    pattern = 0x5A5A if dtype == torch.int16 else 0x5A
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), pattern, dtype=dtype, device=DEV)
    return buf, buf[GUARD: GUARD + n].view(shape)


def _intact(buf, what):
    pattern = 0x5A5A if buf.dtype == torch.int16 else 0x5A
    assert bool((buf[:GUARD] == pattern).all()) and bool((buf[-GUARD:] == pattern).all()), f"{what}: guard band written"


def _segments_of(jpegs):
    """host side of decode_jpeg for one group of frames: (stream, seg_start, seg_bytes, tables, qtables, info) on the device"""
    from evoworld_amd import video
    info = video.parse_jpeg(jpegs[0])
    scan, starts, lengths = video.scan_batch(jpegs, info)
    return _upload(scan.tobytes(), starts, lengths, info)


def _upload(scan, starts, lengths, info):
    from evoworld_amd import video
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return (dev(np.frombuffer(scan, np.uint8).copy()), dev(np.asarray(starts, np.int64)), dev(np.asarray(lengths, np.int32)),
            dev(video.huffman_device_tables(info["huffman"])), dev(np.stack(info["qtables"]).astype(np.uint8)), info)


def _decode_guarded(jpegs, H, W, sub, stop_at_coefficients=False):
    """the three kernels on one group of frames, every output between guard bands -> (coef, status, planes, rgb) on the host"""
    from evoworld_amd import ops
    stream, starts, lengths, tables, qt, info = _segments_of(jpegs)
    mcu, bpm = J.MCU[sub], J.BPM[sub]
    V, mr, mc = len(jpegs), -(-H // mcu), -(-W // mcu)
    assert GUARD >= mc * bpm * 64 and GUARD >= W * mcu * 3
    cbuf, cview = _guarded((V, mr, mc, bpm, 64), torch.int16)
    coef, status = ops.jpeg_huffman_decode(stream, starts, lengths, tables, V, mr, mc, bpm, info["restart_interval"], out=cview)
    torch.cuda.synchronize()
    _intact(cbuf, "coefficients")
    if stop_at_coefficients:
        return coef.cpu().numpy(), status.cpu().numpy(), None, None
    pb = [_guarded(s, torch.uint8) for s in ((V, mr * mcu, mc * mcu), (V, mr * 8, mc * 8), (V, mr * 8, mc * 8))]
    planes = ops.jpeg_idct(coef, qt, out=tuple(v for _, v in pb))
    rbuf, rview = _guarded((V, H, W, 3), torch.uint8)
    rgb = ops.jpeg_planes_to_rgb(planes, H, W, sub, out=rview)
    torch.cuda.synchronize()
    for b, _ in pb:
        _intact(b, "planes")
    _intact(rbuf, "rgb")
    assert torch.equal(ops.jpeg_planes_to_rgb(ops.jpeg_idct(coef, qt), H, W, sub), rgb)          # two calls, identical bytes
    return coef.cpu().numpy(), status.cpu().numpy(), tuple(p.cpu().numpy() for p in planes), rgb.cpu().numpy()


def device(name, sub):
    """a case through the device encoder and the guarded decoder, computed once"""
    from evoworld_amd import ops, video
    key = (name, sub)
    if key not in _device:
        frames, quality = C.CASES[name]
        d = torch.from_numpy(frames).to(DEV)
        jpegs = video.encode_jpeg(d, quality, sub)
        coef, status, planes, rgb = _decode_guarded(jpegs, frames.shape[1], frames.shape[2], sub)
        _device[key] = {"jpegs": jpegs, "encoder": ops.jpeg_dct_quant(d, quality, sub).cpu().numpy(), "coef": coef, "status": status,
                        "planes": planes, "rgb": rgb, "info": video.parse_jpeg(jpegs[0])}
    return _device[key]


# ------------------------------------------------------------------ 1. coefficients, exact
@pytest.mark.parametrize("name,sub", ALL)
def test_coefficients_are_the_encoders(name, sub):
    from evoworld_amd import ops, video
    r = device(name, sub)
    assert not r["status"].any()
    assert r["coef"].dtype == np.int16 and np.array_equal(r["coef"], r["encoder"])
    got = video.decode_jpeg(r["jpegs"], return_coefficients=True)
    assert np.array_equal(got.cpu().numpy(), r["encoder"])
    stream, frame_bytes = ops.jpeg_pack(*ops.jpeg_entropy(got), got.shape[1])                      # ew_jpeg_entropy accepts them unchanged
    at = r["info"]["scan_offset"]
    assert stream.cpu().numpy().tobytes() == b"".join(j[at:-2] for j in r["jpegs"])
    assert frame_bytes.tolist() == [len(j) - at - 2 for j in r["jpegs"]]
    assert np.array_equal(video.decode_jpeg(r["jpegs"]).cpu().numpy(), r["rgb"])                   # the public call = the guarded kernels


@pytest.mark.parametrize("name,variant,sub", D.FOREIGN)
def test_foreign_coefficients_equal_the_python_decoders(name, variant, sub):
    why = D.pillow_unsupported()
    if why:
        pytest.skip(why)
    from evoworld_amd import video
    jpeg = D.foreign_stream(name, variant, sub)
    info = video.parse_jpeg(jpeg)
    assert info["subsampling"] == sub
    if variant == "optimize":
        assert info["huffman"] != tuple(video.HUFFMAN[k] for k in ((0, 0), (0, 1), (1, 0), (1, 1)))  # tables of its own
    if variant == "restart_blocks":
        assert info["restart_interval"] == 3          # divides the MCU row of 40x72 at 4:4:4 (9) and 152x40 at 4:2:0 (3), not the other four
    if variant.startswith("plain") or variant in ("default", "optimize"):
        assert info["restart_interval"] == 0
    want, status = D.huffman_decode_ref(jpeg)
    assert not any(status)
    H, W = C.CASES[name][0].shape[1:3]
    coef, st, _, _ = _decode_guarded([jpeg], H, W, sub, stop_at_coefficients=True)
    assert not st.any() and len(st) == len(status)
    assert np.array_equal(coef[0], want)
    rgb = video.decode_jpeg([jpeg]).cpu().numpy()[0]
    pil = np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))
    print(f"{name} {variant} {sub}: max |device - Pillow| = {np.abs(rgb.astype(int) - pil.astype(int)).max()} levels (unpinned at 4:2:0)")
    assert rgb.shape == pil.shape


# ------------------------------------------------------------------ 2. / 3. samples and pixels against the float64 oracle
@pytest.mark.parametrize("name,sub", PIXELS)
def test_sample_planes_against_the_oracle(name, sub):
    r = device(name, sub)
    qt = np.stack(r["info"]["qtables"])
    counts = []
    for v in range(len(r["coef"])):
        want, bound = D.planes_ref(r["coef"][v], qt, sub)
        for which, got, x, b in zip(("y", "cb", "cr"), r["planes"], want, bound):
            assert b.max() <= D.TIE_WINDOW
            counts.append(D.check_ties(f"{name} {sub} frame {v} {which}", got[v], x, cap=None))
    D.check_cap(f"{name} {sub} planes", counts)


@pytest.mark.parametrize("name,sub", PIXELS)
def test_rgb_is_the_oracle_transform_of_the_device_planes(name, sub):
    r = device(name, sub)
    V, H, W, _ = C.CASES[name][0].shape
    if sub == "4:2:0" and name in ("noise_8x8", "noise_9x17", "flat_9x17"):
        assert r["planes"][1].shape[1] == 8 or r["planes"][1].shape[2] == 8        # a chroma plane of one block: every tap clamps
    D.check_cap(f"{name} {sub} rgb", [D.check_ties(f"{name} {sub} frame {v} rgb", r["rgb"][v], D.rgb_ref(tuple(p[v] for p in r["planes"]), H, W, sub),
                                                   cap=None) for v in range(V)])


@pytest.mark.parametrize("sub", C.SUBSAMPLINGS)
def test_chroma_taps_clamp_at_all_four_borders(sub):
    """planes no image gives: noise in every chroma sample, the Y plane flat, sizes whose last row / column is even and odd"""
    from evoworld_amd import ops
    rng = np.random.default_rng(7)
    for H, W in ((16, 16), (15, 31), (1, 1), (17, 33)):
        mcu = J.MCU[sub]
        ph, pw = -(-H // mcu) * mcu, -(-W // mcu) * mcu
        cs = (ph // 2, pw // 2) if sub == "4:2:0" else (ph, pw)
        planes = (np.full((2, ph, pw), 128, np.uint8), rng.integers(0, 256, (2, *cs), dtype=np.uint8), rng.integers(0, 256, (2, *cs), dtype=np.uint8))
        buf, view = _guarded((2, H, W, 3), torch.uint8)
        got = ops.jpeg_planes_to_rgb(tuple(torch.from_numpy(p).to(DEV) for p in planes), H, W, sub, out=view).cpu().numpy()
        _intact(buf, "rgb")
        for v in range(2):
            D.check_ties(f"borders {H}x{W} {sub}", got[v], D.rgb_ref(tuple(p[v] for p in planes), H, W, sub))


def test_flat_and_halves_come_back_exactly():
    """quality 100 (every divisor 1): flat 0 / 128 / 255 frames and the 0 | 255 halves decode to the source, as the oracle's do"""
    from evoworld_amd import video
    for name in ("flat_16x16", "halves_16x32", "halves_40x72"):
        frames, quality = C.CASES[name]
        assert quality == 100
        for sub in C.SUBSAMPLINGS:
            jpegs = video.encode_jpeg(torch.from_numpy(frames).to(DEV), quality, sub)
            assert np.array_equal(video.decode_jpeg(jpegs).cpu().numpy(), frames), (name, sub)


# ------------------------------------------------------------------ 4. against libjpeg
@pytest.mark.parametrize("name,sub", ALL)
def test_psnr_is_libjpegs(name, sub):
    r = device(name, sub)
    frames, _ = C.CASES[name]
    worst = -np.inf
    for v, (jpeg, frame) in enumerate(zip(r["jpegs"], frames)):
        pil = np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))
        ours, theirs = J.psnr(r["rgb"][v], frame), J.psnr(pil, frame)
        print(f"PSNR {name} {sub} frame {v}: device {ours:.3f} dB, Pillow's decoder {theirs:.3f} dB, shortfall {theirs - ours:+.3f}, "
              f"max |device - Pillow| {np.abs(r['rgb'][v].astype(int) - pil.astype(int)).max()} levels")
        worst = max(worst, theirs - ours)
    assert worst <= PSNR_SLACK, f"{name} {sub}: {worst:.3f} dB below Pillow's decoder"


# ------------------------------------------------------------------ 5. damaged streams
def _damaged():
    """{kind: (segments of frame 0 of noise_40x72 at 4:2:0 with segment 1 damaged, the status the oracle reports for it)}"""
    if "damaged" in _device:
        return _device["damaged"]
    jpeg = device("noise_40x72", "4:2:0")["jpegs"][0]
    h = D.parse(jpeg)
    segs = D.split_segments(h["scan"])
    assert len(segs) == 3
    books = [(D._code_book(*h["huff"][(0, d)]), D._code_book(*h["huff"][(1, a)])) for d, a in h["sel"]]
    seg = segs[1]
    oracle = lambda s: D.decode_segment(s, 5, 6, books)[1]
    assert oracle(seg) == D.OK
    out = {}
    for n in range(len(seg) - 2, 0, -1):                                       # cut short
        if oracle(seg[:n]) == D.EXHAUSTED:
            out["cut"] = (seg[:n], D.EXHAUSTED)
            break
    out["garbage"] = (seg + b"\x12\x34", D.LEFTOVER)
    assert oracle(out["garbage"][0]) == D.LEFTOVER
    out["marker"] = (seg[:7] + b"\xff\xc4" + seg[9:], D.MARKER)
    assert oracle(out["marker"][0]) == D.MARKER
    for at in range(4, len(seg) - 2):                                          # a byte replaced: 16 one-bits match no code
        if b"\xff" in seg[at - 1: at + 3]:
            continue
        for new in (b"\xff\x00\xff\x00", b"\xff\x00"):
            s = seg[:at] + new + seg[at + len(new) // 2:]
            if "bad_code" not in out and oracle(s) == D.BAD_CODE:
                out["bad_code"] = (s, D.BAD_CODE)
        for new in (0xF0, 0x0F, 0xAA, 0x55, 0xFE):
            s = seg[:at] + bytes([new]) + seg[at + 1:]
            if "index" not in out and oracle(s) == D.INDEX:
                out["index"] = (s, D.INDEX)
        if "bad_code" in out and "index" in out:
            break
    assert set(out) == {"cut", "garbage", "marker", "bad_code", "index"}, sorted(out)
    _device["damaged"] = (jpeg, segs, out)
    return _device["damaged"]


@pytest.mark.parametrize("kind", ["cut", "garbage", "marker", "bad_code", "index"])
def test_damaged_segment_is_refused_and_stays_inside(kind):
    from evoworld_amd import ops, video
    jpeg, segs, damaged = _damaged()
    seg, want = damaged[kind]
    parts = [segs[0], seg, segs[2]]
    ref_coef, ref_status = D.huffman_decode_ref(jpeg, segments=parts)
    assert ref_status == [0, want, 0]
    info = video.parse_jpeg(jpeg)
    lengths = [len(p) for p in parts]
    stream, starts, nbytes, tables, _, _ = _upload(b"".join(parts), np.cumsum([0] + lengths[:-1]), lengths, info)
    buf, view = _guarded((1, 3, 5, 6, 64), torch.int16)
    coef, status = ops.jpeg_huffman_decode(stream, starts, nbytes, tables, 1, 3, 5, 6, info["restart_interval"], out=view)
    torch.cuda.synchronize()
    _intact(buf, f"coefficients of the {kind} stream")
    assert status.tolist() == [0, want, 0]
    assert np.array_equal(coef.cpu().numpy()[0], ref_coef)                     # what was decoded before the stop, zeros behind it
    head = jpeg[:info["scan_offset"]]
    broken = head + parts[0] + b"\xff\xd0" + parts[1] + b"\xff\xd1" + parts[2] + b"\xff\xd9"
    if kind != "marker":                                                       # (that one no longer splits into three segments on the host)
        with pytest.raises(ValueError, match=f"frame 1, restart segment 1.*status {want}"):
            video.decode_jpeg([jpeg, broken])
    else:
        with pytest.raises(ValueError):
            video.decode_jpeg([jpeg, broken])
    assert video.decode_jpeg([jpeg, jpeg]).shape == (2, 40, 72, 3)


def test_wrapper_refusals():
    from evoworld_amd import _lib, ops, video
    jpeg = device("noise_8x8", "4:4:4")["jpegs"][0]
    stream, starts, nbytes, tables, qt, info = _segments_of([jpeg])
    with pytest.raises(_lib.EvoWorldHipError):
        ops.jpeg_huffman_decode(stream.cpu(), starts, nbytes, tables, 1, 1, 1, 3, 1)
    with pytest.raises(ValueError):
        ops.jpeg_huffman_decode(stream, starts, nbytes, tables, 1, 1, 1, 4, 1)
    with pytest.raises(ValueError):
        ops.jpeg_huffman_decode(stream, starts, nbytes, tables, 2, 1, 1, 3, 1)                     # two frames need two segments
    with pytest.raises(ValueError):
        ops.jpeg_huffman_decode(stream, starts, nbytes, tables[:-4].contiguous(), 1, 1, 1, 3, 1)
    coef, status = ops.jpeg_huffman_decode(stream, torch.tensor([5], device=DEV), nbytes, tables, 1, 1, 1, 3, 1)
    assert status.tolist() == [_lib.EW_JPEG_SEG_RANGE] and not coef.any()                          # a segment outside the bytes: not read
    coef, _ = ops.jpeg_huffman_decode(stream, starts, nbytes, tables, 1, 1, 1, 3, 1)
    with pytest.raises(ValueError):
        ops.jpeg_idct(coef, qt[:1].contiguous())
    with pytest.raises(TypeError):
        ops.jpeg_idct(coef.int(), qt)
    planes = ops.jpeg_idct(coef, qt)
    with pytest.raises(ValueError):
        ops.jpeg_planes_to_rgb(planes, 8, 8, "4:2:2")
    with pytest.raises(ValueError):
        ops.jpeg_planes_to_rgb(planes, 9, 8, "4:4:4")
    with pytest.raises(ValueError):
        ops.resize_linear_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=DEV), 0, 4)
    with pytest.raises(ValueError, match="mixed frame sizes"):
        video.decode_jpeg([jpeg, device("noise_16x16", "4:4:4")["jpegs"][0]])
    with pytest.raises(ValueError):
        video.decode_jpeg([])
    mixed = video.decode_jpeg([jpeg, video.encode_jpeg(torch.from_numpy(C.CASES["noise_8x8"][0]).to(DEV), 50, "4:2:0")[0], jpeg])
    assert mixed.shape == (3, 8, 8, 3) and torch.equal(mixed[0], mixed[2])                         # three frames, two header groups


# ------------------------------------------------------------------ 6. resize
_big = {}


@pytest.mark.parametrize("shape,size", [((2, 40, 72), (64, 64)), ((1, 576, 1024), (64, 64)), ((2, 40, 72), (40, 72)), ((1, 7, 5), (3, 11))])
def test_resize_linear_against_the_oracle(shape, size):
    from evoworld_amd import ops
    V, H, W = shape
    src = np.random.default_rng(H).integers(0, 256, (V, H, W, 3), dtype=np.uint8)
    buf, view = _guarded((V, *size, 3), torch.uint8)
    got = ops.resize_linear_u8(torch.from_numpy(src).to(DEV), *size, out=view).cpu().numpy()
    _intact(buf, "resize")
    if size == (H, W):
        assert np.array_equal(got, src)
    for v in range(V):
        D.check_ties(f"resize {H}x{W} -> {size}", got[v], D.resize_ref(src[v], *size), exact_halves=True)


# ------------------------------------------------------------------ 7. the public surface
def test_read_video_round_trip(tmp_path):
    from evoworld_amd import video
    frames, _ = C.CASES["ramp_40x72"]
    d = torch.from_numpy(frames).to(DEV)
    for sub in C.SUBSAMPLINGS:
        path = str(tmp_path / f"clip{sub[-1]}.avi")
        video.write_video(path, d, fps=7, quality=90, subsampling=sub)
        got, fps = video.read_video(path)
        assert fps == 7 and got.shape == (3, 40, 72, 3) and got.dtype == torch.uint8 and got.is_cuda
        assert torch.equal(got, video.decode_jpeg(video.encode_jpeg(d, 90, sub)))
        assert J.psnr(got.cpu().numpy(), frames) > 35


def test_extract_png_writes_the_decoded_frames(tmp_path, capsys):
    from evoworld_amd import video
    frames, _ = C.CASES["noise_40x72"]
    path = str(tmp_path / "clip.avi")
    video.write_video(path, torch.from_numpy(frames).to(DEV), fps=10)
    want = video.read_video(path)[0].cpu().numpy()
    video.main(["extract", "--input", path, "--output", str(tmp_path / "png"), "--format", "png"])
    assert sorted(os.listdir(tmp_path / "png")) == ["001.png", "002.png", "003.png"]
    for i in range(3):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "png" / f"{i + 1:03}.png")), want[i])
    video.main(["extract", "--input", path, "--output", str(tmp_path / "jpg")])                   # the default is unchanged
    assert sorted(os.listdir(tmp_path / "jpg")) == ["001.jpg", "002.jpg", "003.jpg"]
    assert "3 frames 72x40" in capsys.readouterr().out


def test_scores_command(tmp_path, capsys):
    from evoworld_amd import metrics, ops, video
    rng = np.random.default_rng(11)
    base = C._ramp(25, 40, 72)
    for ep in ("ep_a", "ep_b"):
        os.makedirs(tmp_path / ep)
        noisy = np.clip(base.astype(np.int16) + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8)
        video.write_video(str(tmp_path / ep / "navigated.avi"), torch.from_numpy(noisy).to(DEV))
        video.write_video(str(tmp_path / ep / "original.avi"), torch.from_numpy(base).to(DEV))
    os.makedirs(tmp_path / "ep_incomplete")
    video.write_video(str(tmp_path / "ep_incomplete" / "navigated.avi"), torch.from_numpy(base).to(DEV))
    (tmp_path / "notes.txt").write_text("not an episode")
    video.main(["scores", "--input_folder", str(tmp_path)])
    got = json.loads(capsys.readouterr().out)
    load = lambda name: torch.stack([ops.resize_linear_u8(video.read_video(str(tmp_path / ep / name))[0], 64, 64)
                                     for ep in ("ep_a", "ep_b")]).permute(0, 1, 4, 2, 3).float() / 255.0
    v1, v2 = load("navigated.avi"), load("original.avi")
    assert v1.shape == (2, 25, 3, 64, 64)
    for key, fn in (("psnr", metrics.calculate_psnr), ("ssim", metrics.calculate_ssim)):
        assert got[key] == json.loads(json.dumps(fn(v1, v2))), key
    assert 10 < got["psnr"]["value_mean"] < 40
    assert sorted(got["not_computed"]) == ["fvd", "lpips"] and "fvd" not in got and "lpips" not in got
    assert got["videos"] == ["ep_a", "ep_b"]
    empty = tmp_path / "ep_incomplete"
    video.main(["scores", "--input_folder", str(empty)])
    assert capsys.readouterr().out.strip() == "No valid videos found. Exiting."
    video.write_video(str(tmp_path / "ep_incomplete" / "original.avi"), torch.from_numpy(base[:24]).to(DEV))
    with pytest.raises(ValueError, match="differ in length"):
        video.video_scores(str(tmp_path))
