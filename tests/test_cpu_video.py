"""-m "not gpu": the host side of the MJPEG video output (evoworld_amd/video.py), the oracle tests/jpeg_ref.py itself, the preconditions
of tests/test_gpu_video.py that need the oracle alone, the BICUBIC resample tables, the CLI flags and the header prototypes."""
import inspect
import io
import os
import struct

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as J
import video_cases as C
from evoworld_amd import video


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 95, 100])
def test_quant_tables_are_libjpegs(quality):
    b = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(b, "JPEG", quality=quality)
    theirs = Image.open(io.BytesIO(b.getvalue())).quantization               # natural order
    luma, chroma = video.quant_tables(quality)
    assert luma.tolist() == list(theirs[0]) and chroma.tolist() == list(theirs[1])
    for ours, ref in zip((luma, chroma), J.quant_tables_ref(quality)):
        assert np.array_equal(ours, ref)
    for bad in (0, 101, 50.0, True):
        with pytest.raises(ValueError):
            video.quant_tables(bad)


def test_tables_are_annex_k():
    """the package's typed Huffman tables against the ones libjpeg writes (read back from a Pillow file), and the zigzag walk"""
    std = J.std_huffman()
    assert set(std) == set(video.HUFFMAN)
    for key, (bits, vals) in std.items():
        assert tuple(bits) == video.HUFFMAN[key][0] and tuple(vals) == video.HUFFMAN[key][1]
    assert tuple(J.ZIGZAG.tolist()) == video.ZIGZAG and sorted(video.ZIGZAG) == list(range(64))


def test_packer_flat_128_block_by_hand():
    """a flat-128 block: Y = Cb = Cr = 0, so every block is DC difference 0 (category 0) followed by EOB.  4:4:4, one MCU:
    Y: DC code 00, EOB 1010; Cb, Cr: DC code 00, EOB 00  ->  001010 0000 0000 + two 1-bits of padding = 0x28 0x03"""
    frame = np.full((8, 8, 3), 128, np.uint8)
    coef = J.quantise_ref(J.quotients_ref(frame, 90, "4:4:4"))
    assert coef.shape == (1, 1, 3, 64) and not coef.any()
    assert J.pack_scan(coef, "4:4:4") == bytes([0x28, 0x03])
    # 4:2:0, one MCU: four Y blocks 001010, then 0000 0000 = 32 bits, no padding
    coef = J.quantise_ref(J.quotients_ref(np.full((16, 16, 3), 128, np.uint8), 90, "4:2:0"))
    assert J.pack_scan(coef, "4:2:0") == int("001010" * 4 + "00000000", 2).to_bytes(4, "big")
    # two MCU rows: RST0 between them
    coef = J.quantise_ref(J.quotients_ref(np.full((16, 8, 3), 128, np.uint8), 90, "4:4:4"))
    assert J.pack_scan(coef, "4:4:4") == bytes([0x28, 0x03, 0xFF, 0xD0, 0x28, 0x03])


@pytest.mark.parametrize("subsampling", C.SUBSAMPLINGS)
@pytest.mark.parametrize("name", ["noise_9x17", "noise_40x72", "noise_152x40", "ramp_40x72", "halves_40x72"])
def test_oracle_stream_decodes_in_pillow(name, subsampling):
    frames, quality = C.CASES[name]
    _, coef = C.oracle(name, subsampling)
    h, w = frames.shape[1:3]
    if name == "noise_152x40":
        assert coef.shape[1] > 8                                               # the RST index wraps
    for v, frame in enumerate(frames):
        jpeg = J.frame_bytes(coef[v], w, h, quality, subsampling)
        assert jpeg[: len(video.jpeg_header(w, h, quality, subsampling))] == video.jpeg_header(w, h, quality, subsampling)
        img = Image.open(io.BytesIO(jpeg))
        assert img.size == (w, h)
        got = np.asarray(img.convert("RGB"))
        b = io.BytesIO()
        Image.fromarray(frame).save(b, "JPEG", quality=quality, subsampling={"4:2:0": 2, "4:4:4": 0}[subsampling])
        theirs = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
        assert J.psnr(got, frame) >= J.psnr(theirs, frame) - 0.05


@pytest.mark.parametrize("subsampling", C.SUBSAMPLINGS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_near_tie_precondition(name, subsampling):
    quot, _ = C.oracle(name, subsampling)
    assert J.near_ties(quot).mean() <= 0.002


def test_oracle_streams_cover_zrl_and_stuffing():
    st = {}
    for name in ("synth_zrl_24x136", "synth_max_16x32", "noise_40x72"):
        _, coef = C.oracle(name, "4:2:0")
        for c in coef:
            J.pack_scan(c, "4:2:0", st)
    assert st["zrl"] > 0 and st["stuffed"] > 0
    _, coef = C.oracle("synth_max_16x32", "4:4:4")
    assert np.abs(coef[..., 1:]).max() == 1020
    _, coef = C.oracle("halves_16x32", "4:4:4")
    assert (coef[0, 0, 1, 0, 0], coef[0, 0, 2, 0, 0]) == (-1024, 1016)


# ------------------------------------------------------------------ container
def _jpegs(n=5):
    rng = np.random.default_rng(3)
    return [J.encode_ref(rng.integers(0, 256, (9, 17, 3), dtype=np.uint8), 50 + 10 * i) for i in range(n)]


def test_avi_round_trip_and_layout(tmp_path):
    jpegs = _jpegs()
    assert any(len(j) & 1 for j in jpegs) and any(not len(j) & 1 for j in jpegs)      # odd and even payloads
    path = str(tmp_path / "a.avi")
    size = video.write_avi(path, jpegs, 17, 9, fps=10)
    data = open(path, "rb").read()
    assert size == len(data) and data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack_from("<I", data, 4)[0] == len(data) - 8
    fps, width, height, back = video.read_avi(path)
    assert (fps, width, height) == (10, 17, 9) and back == jpegs
    # hdrl
    assert data[12:16] == b"LIST" and data[20:24] == b"hdrl" and data[24:28] == b"avih"
    hdrl_size = struct.unpack_from("<I", data, 16)[0]
    avih = struct.unpack_from("<14I", data, 32)
    assert avih[0] == 100000 and avih[3] & 0x10 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (17, 9)     # dwMicroSecPerFrame ...
    strl = 32 + 56
    assert data[strl: strl + 4] == b"LIST" and data[strl + 8: strl + 16] == b"strlstrh"
    strh = strl + 20
    assert data[strh: strh + 8] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack_from("<4I", data, strh + 20)
    assert (scale, rate, length) == (1, 10, 5)
    strf = strh + 56
    assert data[strf: strf + 4] == b"strf"
    bi = struct.unpack_from("<IiiHH4sI", data, strf + 8)
    assert bi == (40, 17, 9, 1, 24, b"MJPG", 17 * 9 * 3)
    # movi
    movi = 12 + 8 + hdrl_size
    assert data[movi: movi + 4] == b"LIST" and data[movi + 8: movi + 12] == b"movi"
    movi_size = struct.unpack_from("<I", data, movi + 4)[0]
    assert movi_size % 2 == 0 and movi_size == 4 + sum(8 + len(j) + (len(j) & 1) for j in jpegs)
    # idx1: every offset (relative to the movi tag) lands on a 00dc chunk holding one whole JPEG
    idx = movi + 8 + movi_size
    assert data[idx: idx + 4] == b"idx1" and struct.unpack_from("<I", data, idx + 4)[0] == 16 * 5 and idx + 8 + 80 == len(data)
    for i, j in enumerate(jpegs):
        cc, flags, off, n = struct.unpack_from("<4sIII", data, idx + 8 + 16 * i)
        at = movi + 8 + off
        assert cc == b"00dc" and flags == 0x10 and n == len(j) and at % 2 == 0
        assert data[at: at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == n
        assert data[at + 8: at + 10] == b"\xff\xd8" and data[at + 8 + n - 2: at + 8 + n] == b"\xff\xd9"
    # a fractional rate
    video.write_avi(path, jpegs[:1], 17, 9, fps=29.97)
    assert abs(video.read_avi(path)[0] - 29.97) < 1e-3
    with pytest.raises(ValueError):
        video.write_avi(path, [], 17, 9)


def test_avi_refuses_two_gib_and_other_extensions(tmp_path):
    frame = b"\xff\xd8" + bytes(2 ** 20) + b"\xff\xd9"
    path = str(tmp_path / "big.avi")
    with pytest.raises(ValueError, match="2 GiB"):
        video.write_avi(path, [frame] * 2048, 64, 64)                         # one shared 1 MiB object: nothing is copied or written
    assert not os.path.exists(path)
    for name in ("clip.mp4", "clip.mkv", "clip"):
        with pytest.raises(ValueError, match="only Motion-JPEG AVI.*H.264"):
            video.write_video(str(tmp_path / name), None)
    with pytest.raises(ValueError):
        video.read_avi(__file__)


def test_cli_flags_signatures_and_prototypes():
    import unified_loop_consistency as cli
    from evoworld_amd import _lib
    from evoworld_amd.inference import Navigator, UnifiedLoopConsistencyPipeline
    a = cli.parse_arguments(["--unet_path", "x"])
    assert a.save_video is False and a.video_fps == 10 and a.video_quality == 90
    a = cli.parse_arguments(["--unet_path", "x", "--save_video", "--video_fps", "24", "--video_quality", "75"])
    assert a.save_video is True and a.video_fps == 24 and a.video_quality == 75
    for script in ("run_unified_pipeline.sh", "run_single_segment.sh"):
        text = open(os.path.join(os.path.dirname(cli.__file__), script)).read()
        assert '[ "$SAVE_VIDEO" = 1 ] && CMD="$CMD --save_video"' in text and "$VIDEO_FPS" in text and "$VIDEO_QUALITY" in text
    sig = inspect.signature(UnifiedLoopConsistencyPipeline.process_episode).parameters
    assert sig["save_video"].default is False and sig["video_fps"].default == 10 and sig["video_quality"].default == 90
    for method in (Navigator.save_video, Navigator.save_gif):                 # the reference's signatures (navigator_evoworld.py:233, :259)
        p = inspect.signature(method).parameters
        assert list(p) == ["self", "save_path", "fps"] and p["fps"].default == 10
    p = inspect.signature(video.encode_jpeg).parameters
    assert list(p) == ["frames", "quality", "subsampling"] and p["quality"].default == 90 and p["subsampling"].default == "4:2:0"
    p = inspect.signature(video.write_video).parameters
    assert list(p) == ["path", "frames", "fps", "quality", "subsampling"] and p["fps"].default == 10
    e = video.parse_arguments(["encode", "--input", "d", "--output", "x.avi"])
    assert (e.fps, e.quality, e.subsampling) == (10, 90, "4:2:0")
    x = video.parse_arguments(["extract", "--input", "x.avi", "--output", "d"])
    assert x.command == "extract"
    H = _lib.HEADER
    assert H.constants["EW_ABI_VERSION"] >= 19 and H.constants["EW_JPEG_420"] == 420 and H.constants["EW_JPEG_444"] == 444
    assert H.functions["ew_jpeg_segment_slot_bytes"] == ("size_t", ["int", "int"])
    assert H.functions["ew_jpeg_dct_quant"] == ("ew_status", ["const uint8_t*", "int16_t*", "int", "int", "int", "int", "int", "void*"])
    assert H.functions["ew_jpeg_entropy"] == ("ew_status", ["const int16_t*", "uint8_t*", "int*", "long long", "int", "int", "size_t", "void*"])
    assert H.functions["ew_jpeg_pack"] == ("ew_status", ["const uint8_t*", "const int*", "const long long*", "uint8_t*", "long long", "int",
                                                         "size_t", "long long", "void*"])


def test_extract_cli_writes_the_frames_back(tmp_path, capsys):
    jpegs = _jpegs(3)
    video.write_avi(str(tmp_path / "a.avi"), jpegs, 17, 9, fps=5)
    video.main(["extract", "--input", str(tmp_path / "a.avi"), "--output", str(tmp_path / "out")])
    assert sorted(os.listdir(tmp_path / "out")) == ["001.jpg", "002.jpg", "003.jpg"]
    assert open(tmp_path / "out" / "002.jpg", "rb").read() == jpegs[1]
    assert Image.open(tmp_path / "out" / "003.jpg").size == (17, 9)
    assert "3 frames 17x9 at 5 fps" in capsys.readouterr().out


# ------------------------------------------------------------------ BICUBIC tables
def _two_pass(img, coeffs_h, coeffs_v):
    """Pillow's two 8bpc passes (horizontal, then vertical, 8-bit intermediate) in numpy: what ew_resize_aa_u8 computes"""
    def one(a, kk, bounds):                                                    # along axis 1
        kk, bounds = kk.numpy().astype(np.int64), bounds.numpy()
        out = np.empty((a.shape[0], len(kk), 3), np.uint8)
        for xo, (xmin, n) in enumerate(bounds):
            acc = (a[:, xmin:xmin + n].astype(np.int64) * kk[xo, :n, None]).sum(1) + (1 << 21)
            out[:, xo] = np.clip(acc >> 22, 0, 255)
        return out
    return one(one(img, *coeffs_h).transpose(1, 0, 2), *coeffs_v).transpose(1, 0, 2)


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(100, 200, 57, 102), (20, 36, 40, 72), (33, 77, 90, 131)])
def test_bicubic_tables_equal_pil_bit_for_bit(Hi, Wi, Ho, Wo):
    """the filter is named "pillow_bicubic": the plain name "bicubic" stays an unknown filter (KeyError), as test_cpu_cubemap.py pins"""
    from evoworld_amd.reprojection import resample_coeffs
    img = np.random.default_rng(Hi).integers(0, 256, (Hi, Wi, 3), dtype=np.uint8)
    got = _two_pass(img, resample_coeffs(Wi, Wo, filter="pillow_bicubic"), resample_coeffs(Hi, Ho, filter="pillow_bicubic"))
    want = np.asarray(Image.fromarray(img).resize((Wo, Ho), Image.BICUBIC))
    assert np.array_equal(got, want)
