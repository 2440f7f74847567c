"""-m "not gpu": the host side of the device PNG encoder (evoworld_amd/png.py) -- the length-limited Huffman builder, the dynamic-block
header, the Adler-32 combine, the container --, the oracle tests/png_ref.py itself against libpng / zlib, the header prototypes, the
flags and the refusals of evoworld_amd.ops that need no device."""
import inspect
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as C
import png_ref as R
from evoworld_amd import ops, png


def _oracle_file(frame, rps):
    """a whole file from the oracle's own parse, the package's tables and the oracle's emitter"""
    H, W, _ = frame.shape
    filt = R.filter_frame(frame)
    segs = [filt[r: r + rps].tobytes() for r in range(0, H, rps)]
    toks = [R.simple_tokens(s) for s in segs]
    t = png.FrameTables(sum(R.histogram(tk) for tk in toks))
    out = []
    for k, (s, tk) in enumerate(zip(segs, toks)):
        last = k == len(segs) - 1
        assert R.replay(tk) == s
        out.append(R.emit_stored(s, last) if k % 3 == 2 else R.emit_segment(tk, t.lit, t.dist, t.header, t.header_bits, last))
    return R.png_bytes(frame, out), filt


@pytest.mark.parametrize("name", ["gradient_1x1", "texture_1x7", "noise4_5x1", "constant_40x72", "black_40x72", "random_40x72",
                                  "gradient_33x130", "black_33x130", "mixed_33x130"])
def test_oracle_files_decode_in_pillow(name):
    """the oracle against libpng / zlib: filters, code assignment, header, emitter, stored blocks, Adler-32, chunk framing"""
    frames, _ = C.CASES[name]
    for frame in frames:
        data, filt = _oracle_file(frame, C.rows_per_segment(name))
        kinds = R.chunks(data)
        assert [k for k, _ in kinds] == [b"IHDR", b"IDAT", b"IEND"] and kinds[1][1][:2] == b"\x78\x01"
        assert zlib.decompress(kinds[1][1]) == filt.tobytes()
        img = Image.open(io.BytesIO(data))
        assert img.mode == "RGB" and np.array_equal(np.asarray(img), frame)


@pytest.mark.parametrize("mode", range(5))
def test_oracle_filters_are_libpngs(mode):
    """every forced filter type reverses in Pillow's decoder: a file of stored blocks around the oracle's filtered rows"""
    frame = C.noise4(9, 14, mode)
    filt = R.filter_frame(frame, mode)
    assert (filt[:, 0] == mode).all()
    raw = filt.tobytes()
    body = b"\x78\x01" + R.emit_stored(raw, True) + zlib.adler32(raw).to_bytes(4, "big")
    data = png.PNG_SIGNATURE + png.chunk(b"IHDR", (14).to_bytes(4, "big") + (9).to_bytes(4, "big") + bytes([8, 2, 0, 0, 0])) + \
        png.chunk(b"IDAT", body) + png.chunk(b"IEND", b"")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), frame)


def _fibonacci(n):
    """n ascending counts whose Huffman tree is a chain: 1, 1, 2, 3, 5 ... up to 60 terms (1.5e12), ones in front of them beyond that"""
    f = [1, 1]
    while len(f) < min(n, 60):
        f.append(f[-1] + f[-2])
    return [1] * (n - len(f)) + f


@pytest.mark.parametrize("n,limit", [(286, 15), (40, 15), (30, 15), (19, 7), (12, 7)])
def test_length_limited_builder_on_fibonacci_counts(n, limit):
    """Fibonacci counts make Huffman's tree a chain (depth n - 1): the limit must hold and the code must stay complete"""
    freqs = _fibonacci(n)
    lengths = png.limited_code_lengths(freqs, limit)
    assert all(1 <= l <= limit for l in lengths) and max(lengths) == limit
    num, den = R.kraft(lengths)
    assert num == den
    assert all(lengths[i] >= lengths[i + 1] for i in range(n - 1))             # rarer symbols never get shorter codes
    rng = np.random.default_rng(n)
    freqs = (rng.integers(0, 2, n) * rng.integers(1, 10 ** 6, n)).tolist()    # with holes
    freqs[0], freqs[1] = 1, 5
    lengths = png.limited_code_lengths(freqs, limit)
    assert all((l == 0) == (f == 0) for l, f in zip(lengths, freqs)) and max(lengths) <= limit
    assert R.kraft(lengths)[0] == R.kraft(lengths)[1]


def test_length_limited_builder_is_optimal_where_huffman_fits():
    freqs = [5, 9, 12, 13, 16, 45]
    lengths = png.limited_code_lengths(freqs, 15)
    assert sorted(lengths) == [1, 3, 3, 3, 4, 4]
    # the limit binds: package-merge's cost is the least of all complete codes of at most 3 bits over 6 symbols
    lengths = png.limited_code_lengths(freqs, 3)
    cost = sum(f * l for f, l in zip(freqs, lengths))
    assert max(lengths) == 3 and R.kraft(lengths)[0] == R.kraft(lengths)[1] and cost == 2 * (45 + 16) + 3 * (13 + 12 + 9 + 5)


def test_single_symbol_histograms_get_complete_codes():
    for n, limit in ((286, 15), (30, 15), (19, 7)):
        for s in (0, 1, n - 1):
            freqs = [0] * n
            freqs[s] = 7
            lengths = png.limited_code_lengths(freqs, limit)
            assert lengths[s] == 1 and sorted(lengths)[-2:] == [1, 1] and sum(lengths) == 2
        assert sum(png.limited_code_lengths([0] * n, limit)) == 2
    # a frame without a match: literals and the end-of-block symbol only
    hist = np.zeros(316, np.int64)
    hist[[3, 200, 256]] = 10, 4, 1
    t = png.FrameTables(hist)
    assert t.dist[:2] == [1, 1] and not any(t.dist[2:])
    assert t.lit[256] > 0 and R.kraft(t.lit)[0] == R.kraft(t.lit)[1]
    # symbol 256 gets a code also when the histogram forgot it
    hist[256] = 0
    assert png.FrameTables(hist).lit[256] > 0


@pytest.mark.parametrize("seed", range(6))
def test_header_round_trips_through_zlib(seed):
    """a block built from known tokens -- the package's header, the oracle's emitter -- inflates to the bytes the tokens stand for"""
    rng = np.random.default_rng(seed)
    if seed == 0:
        tokens = [65, 66, 67] + [0x80000000 | (258 - 3) | (2 << 8)] * 3 + [0x80000000 | 0 | (0 << 8), 7]
    elif seed == 1:
        tokens = list(rng.integers(0, 256, 4000))                                  # no match at all: two distance codes of length 1
    elif seed == 2:
        tokens = [9]                                                               # one literal
    else:
        tokens, have = [], 0
        for _ in range(3000):
            if have >= 1 and rng.random() < 0.5:
                dist = int(min(have, rng.choice([1, 2, 3, 4, 5, 24, 25, 100, 1000, 5000, 24577, 32768])))
                length = int(rng.choice([3, 4, 10, 11, 12, 18, 130, 131, 226, 227, 257, 258]))
                tokens.append(0x80000000 | (length - 3) | ((dist - 1) << 8))
                have += length
            else:
                tokens.append(int(rng.integers(0, 256 if seed == 3 else 3)))
                have += 1
    want = R.replay(tokens)
    t = png.FrameTables(R.histogram(tokens))
    assert max(t.lit) <= 15 and max(t.dist) <= 15 and max(t.clc) <= 7
    for lengths in (t.lit, t.dist, t.clc):
        assert R.kraft(lengths)[0] == R.kraft(lengths)[1]
    assert t.header[0] & 7 == 0b100 and len(t.header) == (t.header_bits + 7) // 8    # BFINAL 0, BTYPE 10
    block = R.emit_segment(tokens, t.lit, t.dist, t.header, t.header_bits, True)
    d = zlib.decompressobj(-15)
    assert d.decompress(block) == want and d.eof and d.unused_data == b""
    # not last: the empty stored block ends the segment on a byte, and a second segment continues the stream
    two = R.emit_segment(tokens, t.lit, t.dist, t.header, t.header_bits, False) + block
    assert two[len(two) - len(block) - 4: len(two) - len(block)] == b"\x00\x00\xff\xff"
    d = zlib.decompressobj(-15)
    assert d.decompress(two) == want + want and d.eof
    # the package's lut and cost agree with the oracle's canonical codes
    codes = R.canonical(t.lit)
    for s, (code, n) in codes.items():
        assert int(t.lut[s]) >> 16 == n and png.reverse_bits(int(t.lut[s]) & 0xFFFF, n) == code
    bits = t.header_bits + int((R.histogram(tokens) * t.cost).sum())
    assert (bits + 7) // 8 == len(block)


def test_adler_combine_matches_zlib():
    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, 200000, dtype=np.uint8).tobytes()
    for _ in range(20):
        cuts = sorted(rng.integers(0, len(data), int(rng.integers(1, 6))).tolist())
        a, b = 1, 0
        ra, rb = 1, 0
        for lo, hi in zip([0] + cuts, cuts + [len(data)]):
            part = data[lo:hi]
            a, b = png.adler_combine(a, b, *R.adler_halves(part), len(part))
            ra, rb = R.adler_combine(ra, rb, *R.adler_halves(part), len(part))
        assert (b << 16) | a == zlib.adler32(data) == (rb << 16) | ra
    assert png.adler_combine(1, 0, 1, 0, 0) == (1, 0)
    ff = b"\xff" * 70000                                                          # both halves wrap
    a, b = png.adler_combine(*R.adler_halves(ff), *R.adler_halves(ff), len(ff))
    assert (b << 16) | a == zlib.adler32(ff + ff)


def test_container_and_sizes():
    data = png.png_file(3, 2, R.emit_stored(bytes(2 * 10), True), zlib.adler32(bytes(20)))
    assert [k for k, _ in R.chunks(data)] == [b"IHDR", b"IDAT", b"IEND"]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), np.zeros((2, 3, 3), np.uint8))
    assert png.stored_size(1) == 6 and png.stored_size(65535) == 65540 and png.stored_size(65536) == 65546
    assert png.frames_per_batch(576, 1024) == 37 and png.frames_per_batch(65535, 65535) == 1
    assert 4 * 37 * 576 * 3073 <= png.TOKEN_WORKSPACE_BYTES < 4 * 38 * 576 * 3073
    assert ops.png_rows_per_segment(576, 1024) == 10 and ops.png_rows_per_segment(4, 1024) == 4
    assert ops.png_rows_per_segment(1000, 20000) == 1 and ops.png_rows_per_segment(33, 130, 8) == 8


def test_prototypes_flags_and_signatures():
    import unified_loop_consistency as cli
    from evoworld_amd import _lib, cubemap, video
    from evoworld_amd.frames import write_numbered
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.reprojection import CubemapRenderer, predictions_to_target_view
    H = _lib.HEADER
    assert H.constants["EW_ABI_VERSION"] == _lib.ABI_VERSION == 20
    assert (H.constants["EW_PNG_FILTER_ADAPTIVE"], H.constants["EW_PNG_SEG_CODED"], H.constants["EW_PNG_SEG_STORED"]) == (5, 0, 1)
    assert H.constants["EW_PNG_HIST_COLS"] == 286 + 30
    assert H.functions["ew_png_filter"] == ("ew_status", ["const uint8_t*", "uint8_t*", "int*", "int", "int", "int", "int", "int", "void*"])
    assert H.functions["ew_png_lz77"] == ("ew_status", ["const uint8_t*", "uint32_t*", "int*", "int*", "int", "int", "int", "int", "long long",
                                                        "void*"])
    assert H.functions["ew_png_emit"] == ("ew_status", ["const uint32_t*", "const int*", "const uint8_t*", "const int*", "const long long*",
                                                        "const long long*", "const uint32_t*", "const uint8_t*", "const int*", "int",
                                                        "uint8_t*", "long long", "int", "int", "int", "int", "long long", "void*"])
    a = cli.parse_arguments(["--unet_path", "x"])
    assert a.device_png is False
    assert cli.parse_arguments(["--unet_path", "x", "--device_png"]).device_png is True
    for script in ("run_unified_pipeline.sh", "run_single_segment.sh"):
        text = open(os.path.join(os.path.dirname(cli.__file__), script)).read()
        assert '[ "$DEVICE_PNG" = 1 ] && CMD="$CMD --device_png"' in text
    assert inspect.signature(UnifiedLoopConsistencyPipeline.process_episode).parameters["png_on_device"].default is False
    assert inspect.signature(write_numbered).parameters["on_device"].default is False
    assert inspect.signature(predictions_to_target_view).parameters["png_on_device"].default is False
    assert inspect.signature(CubemapRenderer.render_cubemaps_to_panoramas).parameters["png_on_device"].default is False
    x = video.parse_arguments(["extract", "--input", "x.avi", "--output", "d", "--format", "png"])
    assert x.device_png is False
    assert video.parse_arguments(["extract", "--input", "x.avi", "--output", "d", "--format", "png", "--device_png"]).device_png is True
    assert cubemap.parse_args(["to-cubemap", "--input", "a", "--output", "b"]).device_png is False
    assert cubemap.parse_args(["to-pano", "--input", "a", "--output", "b", "--size", "8", "4", "--device_png"]).device_png is True
    p = inspect.signature(png.encode_png).parameters
    assert list(p) == ["frames_u8", "filter", "rows_per_segment"] and p["filter"].default == "adaptive" and p["rows_per_segment"].default is None
    assert list(inspect.signature(png.write_png).parameters) == ["path", "frame"]
    p = inspect.signature(png.write_png_frames).parameters
    assert list(p) == ["dir", "frames", "start", "digits"] and p["start"].default == 0 and p["digits"].default == 3
    e = png.parse_arguments(["encode", "--input", "x.avi", "--output", "d"])
    assert e.command == "encode" and e.filter == "adaptive" and e.rows_per_segment is None


def test_ops_refusals_without_a_device():
    ok = torch.zeros(1, 2, 2, 3, dtype=torch.uint8)
    with pytest.raises(TypeError, match="expected torch.uint8"):
        ops.png_filter(ok.float())
    for bad in (torch.zeros(2, 2, 3, dtype=torch.uint8), torch.zeros(1, 2, 2, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"frames_u8 must be \[V,H,W,3\]"):
            ops.png_filter(bad)
    for bad in ("best", 5, -1, 2.0, None):
        with pytest.raises(ValueError, match="filter must be one of"):
            ops.png_filter(ok, bad)
    for bad in (0, -3, 2.5, "4"):
        with pytest.raises(ValueError, match="rows_per_segment must be an integer >= 1"):
            ops.png_filter(ok, "adaptive", bad)
    meta = lambda *s: torch.empty(*s, dtype=torch.uint8, device="meta")            # a shape without memory
    for shape in ((65536, 1, 1, 3), (1, 65536, 1, 3), (1, 1, 65536, 3), (0, 4, 4, 3), (1, 0, 4, 3), (1, 4, 0, 3)):
        with pytest.raises(ValueError, match="V, H and W must be 1..65535"):
            ops.png_filter(meta(*shape))
    with pytest.raises(ValueError, match=r"n_segments = \d+ must be below 2\^31"):
        ops.png_filter(meta(65535, 65535, 1, 3), "none", 1)
    for bad in (meta(2, 2), meta(1, 2, 6), meta(1, 2, 1), meta(0, 2, 7)):
        with pytest.raises(ValueError, match=r"filtered must be \[V,H,1\+3W\]"):
            ops.png_lz77(bad)
    with pytest.raises(ValueError, match=r"n_segments = \d+ must be below 2\^31"):
        ops.png_lz77(meta(65535, 65535, 4), 1)
    with pytest.raises(ValueError, match="rows_per_segment must be an integer >= 1"):
        ops.png_lz77(meta(1, 2, 7), 0)
    # the device check comes last and is the package's own error: there is no CPU path
    from evoworld_amd._lib import EvoWorldHipError
    with pytest.raises(EvoWorldHipError, match="must live on the GPU"):
        ops.png_filter(ok)
    with pytest.raises(EvoWorldHipError, match="must live on the GPU"):
        ops.png_lz77(torch.zeros(1, 2, 7, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"frames_u8 must be \[V,H,W,3\]"):
        png.encode_png(torch.zeros(1, 2, 2, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"frame must be \[H,W,3\]"):
        png.write_png("x.png", ok)
