"""-m "not gpu": the host side of the MJPEG decoder (evoworld_amd/video.py: parse_jpeg, the segment table, the Huffman tables in the
kernel's form), the oracle tests/jpeg_decode_ref.py itself, and the preconditions of tests/test_gpu_video_decode.py that need the oracle
alone: the share of values near a rounding tie, and the float32 error bound of the inverse DCT against the tie window."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_decode_ref as D
import jpeg_ref as J
import video_cases as C
from evoworld_amd import video

ALL = [(n, s) for n in C.CASES for s in C.SUBSAMPLINGS]
PIXELS = [(n, s) for n, s in ALL if n != "synth_zrl_24x136"]          # the cases of the sample and pixel checks on the device


def _oracle_jpeg(name, sub, v=0):
    frames, quality = C.CASES[name]
    return J.frame_bytes(C.oracle(name, sub)[1][v], frames.shape[2], frames.shape[1], quality, sub)


def _pillow(frame, **kw):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", **kw)
    return b.getvalue()


@pytest.mark.parametrize("name,sub", ALL)
def test_oracle_decoder_inverts_the_oracle_packer(name, sub):
    frames, quality = C.CASES[name]
    _, coef = C.oracle(name, sub)
    for v in range(len(frames)):
        jpeg = _oracle_jpeg(name, sub, v)
        got, status = D.huffman_decode_ref(jpeg)
        assert status == [D.OK] * coef.shape[1] and np.array_equal(got, coef[v])
        info = video.parse_jpeg(jpeg)
        assert (info["width"], info["height"], info["subsampling"]) == (frames.shape[2], frames.shape[1], sub)
        assert info["restart_interval"] == coef.shape[2] and jpeg[info["scan_offset"]:][:info["scan_bytes"]] == D.parse(jpeg)["scan"]
        for ours, ref in zip(info["qtables"], J.quant_tables_ref(quality)):
            assert np.array_equal(ours, ref)
        starts, lengths, nbytes = video._segment_table(jpeg, info, v)
        segs = D.split_segments(D.parse(jpeg)["scan"])
        assert nbytes == info["scan_bytes"] and [jpeg[info["scan_offset"] + s:][:n] for s, n in zip(starts, lengths)] == segs


@pytest.mark.parametrize("name,sub", PIXELS)
def test_near_tie_precondition_of_the_pixel_stages(name, sub):
    """On the oracle alone: at most 1 % of a case's samples, and of its RGB values, lie within TIE_WINDOW of a half-integer, and the
    float32 error bound of the inverse DCT (19 u sum |m||m||x| + 512 u) stays inside that window for every sample."""
    frames, _ = C.CASES[name]
    _, coef = C.oracle(name, sub)
    H, W = frames.shape[1:3]
    near = {"planes": [0, 0], "rgb": [0, 0]}
    for v in range(len(frames)):
        h = D.parse(_oracle_jpeg(name, sub, v))
        vals, bounds = D.planes_ref(coef[v], h["qt"], sub)
        assert max(b.max() for b in bounds) <= D.TIE_WINDOW
        for x in vals:
            near["planes"][0] += int(D.near_half(x).sum())
            near["planes"][1] += x.size
        rgb = D.rgb_ref(tuple(D.to_u8(x) for x in vals), H, W, sub)
        near["rgb"][0] += int(D.near_half(rgb).sum())
        near["rgb"][1] += rgb.size
    for what, (n, total) in near.items():
        print(f"{name} {sub} {what}: {n} of {total} near a tie ({100 * n / total:.3f} %)")
        assert n <= 0.01 * total, what


def test_the_excluded_case_breaks_the_cap():
    """why synth_zrl_24x136 is left out of the sample and pixel checks: its samples sit on half-integers by construction"""
    for sub in C.SUBSAMPLINGS:
        h = D.parse(_oracle_jpeg("synth_zrl_24x136", sub))
        vals, _ = D.planes_ref(C.oracle("synth_zrl_24x136", sub)[1][0], h["qt"], sub)
        assert sum(int(D.near_half(x).sum()) for x in vals) > 0.01 * sum(x.size for x in vals)


def test_oracle_decodes_flat_and_halves_exactly():
    for name in ("flat_16x16", "halves_16x32", "halves_40x72"):
        frames, quality = C.CASES[name]
        assert quality == 100
        for sub in C.SUBSAMPLINGS:
            for v, f in enumerate(frames):
                assert np.array_equal(D.decode_ref(_oracle_jpeg(name, sub, v)), f)


def test_oracle_pixel_stages_by_hand():
    # one DC coefficient: a flat block of 128 + c * q / 8
    coef = np.zeros((1, 1, 3, 64), np.int16)
    coef[0, 0, 0, 0] = 5
    (y, cb, cr), _ = D.planes_ref(coef, np.stack([np.full(64, 16), np.full(64, 17)]), "4:4:4")
    assert np.allclose(y, 138.0) and np.allclose(cb, 128.0) and y.shape == (8, 8)
    # the triangle filter on a 1 x 2 plane: the outer taps clamp
    up = D._upsample(np.array([[0, 16]], np.uint8))
    assert up.tolist() == [[0, 4, 12, 16], [0, 4, 12, 16]]
    # grey stays grey, full red
    assert D.rgb_ref((np.full((8, 8), 77, np.uint8),) + (np.full((8, 8), 128, np.uint8),) * 2, 3, 5, "4:4:4").tolist() == [[[77.0] * 3] * 5] * 3
    r = D.rgb_ref((np.full((8, 8), 76, np.uint8), np.full((8, 8), 85, np.uint8), np.full((8, 8), 255, np.uint8)), 1, 1, "4:4:4")[0, 0]
    assert D.to_u8(r).tolist() == [254, 0, 0]
    # resize: identity, and 2 -> 4 along x (centres at -0.25, 0.25, 0.75, 1.25)
    img = np.array([[[0, 0, 0], [100, 100, 100]]], np.uint8)
    assert np.array_equal(D.resize_ref(img, 1, 2), img.astype(np.float64))
    assert D.resize_ref(img, 1, 4)[0, :, 0].tolist() == [0.0, 25.0, 75.0, 100.0]


def _walk_device_table(raw, bits16):
    """the kernel's lookup on one table in the device form: the 16 bits in front -> (length, symbol) or None"""
    look = raw[:1024].view("<u2")
    maxcode, valoff, vals = raw[1024:1096].view("<i4"), raw[1096:1168].view("<i4"), raw[1168:1424]
    e = int(look[bits16 >> 7])
    if e:
        return e >> 8, e & 255
    for length in range(10, 17):
        code = bits16 >> (16 - length)
        if code <= maxcode[length]:
            return length, int(vals[(code + valoff[length]) & 255])
    return None


def test_device_huffman_tables_decode_every_code():
    """Annex K's four tables and the tables libjpeg fits to an image, in the form the kernel reads: every code, followed by any bits,
    comes back as its symbol and length; bit strings no code starts are refused."""
    fitted = D.parse(_pillow(C.CASES["noise_40x72"][0][0], optimize=True, quality=30))["huff"]
    for tables in ([video.HUFFMAN[k] for k in ((0, 0), (0, 1), (1, 0), (1, 1))], [fitted[k] for k in ((0, 0), (0, 1), (1, 0), (1, 1))]):
        raw = video.huffman_device_tables(tables)
        assert raw.dtype == np.uint8 and raw.shape == (4 * video.HUFF_TABLE_BYTES,)
        rng = np.random.default_rng(0)
        for t, (bits, vals) in enumerate(tables):
            one = raw[t * video.HUFF_TABLE_BYTES: (t + 1) * video.HUFF_TABLE_BYTES]
            codes = J.huff_codes(bits, vals)
            assert len(codes) == len(vals)
            for sym, (code, length) in codes.items():
                for tail in (0, (1 << (16 - length)) - 1, int(rng.integers(0, 1 << (16 - length)))):
                    assert _walk_device_table(one, code << (16 - length) | tail) == (length, sym)
            taken = np.zeros(1 << 16, bool)
            for code, length in codes.values():
                taken[code << (16 - length): (code + 1) << (16 - length)] = True
            for free in np.flatnonzero(~taken)[:: max(1, int((~taken).sum()) // 64)]:
                assert _walk_device_table(one, int(free)) is None
    with pytest.raises(ValueError, match="prefix code"):
        video.huffman_device_tables([((3,) + (0,) * 15, (0, 1, 2))] * 4)          # three codes of one bit


def test_parse_jpeg_reads_libjpegs_files():
    why = D.pillow_unsupported()
    if why:
        pytest.skip(why)
    frame = C.CASES["noise_40x72"][0][0]
    for variant, sub in (("default", "4:2:0"), ("optimize", "4:4:4"), ("restart_rows", "4:2:0"), ("restart_blocks", "4:4:4"), ("plain_q30", "4:2:0")):
        jpeg = D.foreign_stream("noise_40x72", variant, sub)
        info, ref = video.parse_jpeg(jpeg), D.parse(jpeg)
        assert (info["width"], info["height"], info["subsampling"]) == (72, 40, sub) == (ref["width"], ref["height"], ref["subsampling"])
        theirs = Image.open(io.BytesIO(jpeg)).quantization
        assert info["qtables"][0].tolist() == list(theirs[0]) and info["qtables"][1].tolist() == list(theirs[1])
        assert [(list(b), list(v)) for b, v in info["huffman"]] == [tuple(map(list, ref["huff"][k])) for k in ((0, 0), (0, 1), (1, 0), (1, 1))]
        mc = -(-72 // J.MCU[sub])
        assert info["restart_interval"] == {"restart_rows": mc, "restart_blocks": 3}.get(variant, 0) == ref["dri"]
        assert jpeg[info["scan_offset"]:][:info["scan_bytes"]] == ref["scan"] and jpeg[info["scan_offset"] + info["scan_bytes"]:] == b"\xff\xd9"
        starts, lengths, _ = video._segment_table(jpeg, info, 0)
        assert [jpeg[info["scan_offset"] + s:][:n] for s, n in zip(starts, lengths)] == D.split_segments(ref["scan"])
        mcus = mc * -(-40 // J.MCU[sub])
        assert len(starts) == (-(-mcus // info["restart_interval"]) if info["restart_interval"] else 1)
        assert frame.shape == D.decode_ref(jpeg).shape


def test_parse_jpeg_refusals():
    frame = C.CASES["noise_40x72"][0][0]
    good = video.jpeg_header(72, 40) + J.pack_scan(C.oracle("noise_40x72", "4:2:0")[1][0], "4:2:0") + b"\xff\xd9"
    assert video.parse_jpeg(good)["restart_interval"] == 5
    cmyk = io.BytesIO()
    Image.new("CMYK", (8, 8)).save(cmyk, "JPEG")
    cases = {
        "progressive": (_pillow(frame, progressive=True), "progressive"),
        "greyscale": (_pillow(frame[..., 0]), "greyscale"),
        "4:2:2": (_pillow(frame, subsampling=1), "4:2:2"),
        "cmyk": (cmyk.getvalue(), "4 components"),
        "12 bit": (good.replace(b"\xff\xc0\x00\x11\x08", b"\xff\xc0\x00\x11\x0c"), "12 bit"),
        "arithmetic": (good.replace(b"\xff\xc0\x00\x11", b"\xff\xc9\x00\x11"), "arithmetic"),
        "truncated header": (good[:200], "truncated"),
        "truncated scan": (good[:-2], "truncated"),
        "two scans": (good[:-2] + b"\xff\xda\x00\x0c" + good[-12:], "several scans"),
        "no SOI": (good[2:], "SOI"),
        "missing table": (good.replace(b"\xff\xc4\x00\x1f\x00", b"\xff\xe5\x00\x1f\x00"), "missing table: DHT DC 0"),
        "scan before frame": (good.replace(b"\xff\xc0\x00\x11", b"\xff\xe5\x00\x11"), "in front of the frame header"),
    }
    for what, (data, message) in cases.items():
        with pytest.raises(ValueError, match=message):
            video.parse_jpeg(data)
    assert video.parse_jpeg(good[:20] + b"\xff\xfe\x00\x05abc" + b"\xff\xe7\x00\x04xy" + good[20:])["width"] == 72       # COM, APP7 skipped
    # restart markers: out of order, missing (decode_jpeg checks them on the host, before anything reaches the device)
    info = video.parse_jpeg(good)
    assert good.count(b"\xff\xd0") == 1 and good.count(b"\xff\xd1") == 1
    with pytest.raises(ValueError, match="frame 0: restart marker 0 is RST1.*out of order"):
        video.decode_jpeg([good.replace(b"\xff\xd0", b"\xff\xd7").replace(b"\xff\xd1", b"\xff\xd0").replace(b"\xff\xd7", b"\xff\xd1")])
    at = good.index(b"\xff\xd1")
    with pytest.raises(ValueError, match="1 restart markers.*3 segments"):
        video.decode_jpeg([good[:at] + good[at + 2:]])
    with pytest.raises(ValueError, match="frame 1.*progressive"):
        video.decode_jpeg([good, cases["progressive"][0]])
    with pytest.raises(ValueError, match="mixed frame sizes"):
        video.decode_jpeg([good, video.jpeg_header(8, 8) + b"\x00\xff\xd9"])
    assert info["scan_bytes"] == len(good) - info["scan_offset"] - 2


def test_cli_flags_and_prototypes():
    from evoworld_amd import _lib
    a = video.parse_arguments(["extract", "--input", "a.avi", "--output", "d"])
    assert a.format == "jpg"
    assert video.parse_arguments(["extract", "--input", "a.avi", "--output", "d", "--format", "png"]).format == "png"
    a = video.parse_arguments(["scores", "--input_folder", "x"])
    assert (a.target_size, a.lpips_weights, a.fvd_weights, a.channel_order, a.result_file) == (64, None, None, "rgb", None)
    a = video.parse_arguments(["scores", "--input_folder", "x", "--target_size", "32", "--lpips_weights", "a", "b", "--fvd_weights", "c"])
    assert (a.target_size, a.lpips_weights, a.fvd_weights) == (32, ["a", "b"], ["c"])
    H = _lib.HEADER
    assert H.constants["EW_JPEG_HUFF_TABLE_BYTES"] == video.HUFF_TABLE_BYTES == 512 * 2 + 18 * 4 + 18 * 4 + 256
    assert [H.constants[f"EW_JPEG_SEG_{n}"] for n in ("OK", "BAD_CODE", "INDEX", "SIZE", "EXHAUSTED", "LEFTOVER", "MARKER")] == \
        [D.OK, D.BAD_CODE, D.INDEX, D.SIZE, D.EXHAUSTED, D.LEFTOVER, D.MARKER]
    assert H.functions["ew_jpeg_huffman_decode"] == ("ew_status", ["const uint8_t*", "long long", "const long long*", "const int*", "const uint8_t*",
                                                                   "int16_t*", "int*", "long long", "int", "int", "int", "int", "int", "void*"])
    assert H.functions["ew_jpeg_idct"] == ("ew_status", ["const int16_t*", "const uint8_t*", "uint8_t*", "uint8_t*", "uint8_t*", "int", "int", "int",
                                                         "int", "void*"])
    assert H.functions["ew_jpeg_planes_to_rgb"] == ("ew_status", ["const uint8_t*", "const uint8_t*", "const uint8_t*", "uint8_t*", "int", "int",
                                                                  "int", "int", "void*"])
    assert H.functions["ew_resize_linear_u8"] == ("ew_status", ["const uint8_t*", "uint8_t*", "int", "int", "int", "int", "int", "void*"])
