"""-m gpu: the device PNG encoder (csrc/png.hip, evoworld_amd/png.py) against the oracle tests/png_ref.py -- filtered rows, tokens and
histograms, the emitted stream, whole files through Pillow and zlib, the derivable size bounds, the measured size ratios, and the
opt-in wiring.  PNG is lossless and the code is integer code: every comparison is exact."""
import functools
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as C
import png_ref as R
from evoworld_amd import ops, png
from test_gpu_inference import tiny  # noqa: F401  (the module-scoped tiny U-Net fixture)

pytestmark = pytest.mark.gpu
MODES = {0: "none", 1: "sub", 2: "up", 3: "average", 4: "paeth", R.ADAPTIVE: "adaptive"}
GUARD = 0xA5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def device_parse(name):
    """the device's filtered rows, Adler halves, tokens and histograms of a case (adaptive filter), computed once, as numpy"""
    frames, _ = C.CASES[name]
    rps = C.rows_per_segment(name)
    filtered, adler = ops.png_filter(dev(frames), "adaptive", rps)
    tokens, n_tokens, hist = ops.png_lz77(filtered, rps)
    out = filtered.cpu().numpy(), adler.cpu().numpy(), tokens.cpu().numpy().view(np.uint32), n_tokens.cpu().numpy(), hist.cpu().numpy()
    for a in out:
        a.setflags(write=False)
    return out


def segment_bytes(name, filt):
    """[(frame, segment index, the segment's filtered bytes)] in the order of the device's segment index"""
    return [(v, k, filt[v, r0: r0 + n].tobytes()) for v in range(filt.shape[0]) for k, (r0, n) in enumerate(C.segments(name))]


def check_tokens(tokens, data):
    """every match has length 3 .. 258 and distance <= min(32768, position); the replay gives `data`; -> the split tokens"""
    pos, out = 0, []
    for t in tokens:
        tok = R.split_token(t)
        if tok[0] == "match":
            assert int(t) & 0x7F800000 == 0, "bits 23 - 30 of a match are clear"
            assert 3 <= tok[1] <= 258 and 1 <= tok[2] <= min(32768, pos), (tok, pos)
            pos += tok[1]
        else:
            assert int(t) < 256
            pos += 1
        out.append(tok)
    assert R.replay(tokens) == data
    return out


# ------------------------------------------------------------------ filter
@pytest.mark.parametrize("name", list(C.CASES))
def test_filtered_rows_equal_oracle(name):
    frames, _ = C.CASES[name]
    d = dev(frames)
    for mode, label in MODES.items():
        got, _ = ops.png_filter(d, mode if mode in (0, 2, 4) else label, C.rows_per_segment(name))    # by number and by name
        assert np.array_equal(got.cpu().numpy(), C.filtered(name, mode)), (name, label)


def test_filter_ties_and_unaligned_frames():
    """A constant row 0 makes Sub and Paeth tie (both leave the first pixel and zeros; Average leaves c - c // 2 everywhere and None / Up
    the row itself): type 1 must win.  Under a constant row, Up wins alone with cost 0.  An all-zero frame ties all five: type 0.
    A frame that starts at an odd address (a slice of a batch with 3 W H odd) takes the byte loads and must not change."""
    row = np.full((1, 1, 9, 3), 200, np.uint8)
    cands = [R.filter_row(f, row.reshape(-1), np.zeros(27, np.uint8)).astype(np.int64) for f in range(5)]
    costs = [int(np.where(c < 128, c, 256 - c).sum()) for c in cands]
    assert costs[1] == costs[4] == min(costs) and costs[0] > costs[1] and costs[3] > costs[1]
    got, _ = ops.png_filter(dev(row))
    assert got[0, 0, 0].item() == 1 and np.array_equal(got.cpu().numpy()[0], R.filter_frame(row[0]))
    got, _ = ops.png_filter(dev(np.full((1, 4, 9, 3), 200, np.uint8)))
    assert got[0, :, 0].tolist() == [1, 2, 2, 2]
    got, _ = ops.png_filter(dev(np.zeros((2, 5, 8, 3), np.uint8)))
    assert not got.any()
    frames = np.stack([C.noise4(3, 7, s) for s in range(3)])                        # 63 bytes per frame: frame 1 starts at an odd address
    whole = dev(frames)
    got, _ = ops.png_filter(whole[1:2])
    assert np.array_equal(got.cpu().numpy()[0], R.filter_frame(frames[1]))
    frames = np.stack([C.texture(5, 8, s) for s in range(3)])                       # 3 W = 24, rows on words, but the base is not (+ 1)
    flat = torch.empty(frames.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = dev(frames).reshape(-1)
    got, _ = ops.png_filter(flat[1:].view(3, 5, 8, 3))
    assert np.array_equal(got.cpu().numpy(), np.stack([R.filter_frame(f) for f in frames]))


@pytest.mark.parametrize("name", ["mixed_33x130", "black_40x72", "noise4_3x1100"])
def test_adler_halves_equal_zlib(name):
    filt, adler, *_ = device_parse(name)
    for s, (v, k, data) in enumerate(segment_bytes(name, filt)):
        assert tuple(adler[s]) == R.adler_halves(data), (name, s)


# ------------------------------------------------------------------ tokens
@pytest.mark.parametrize("name", list(C.CASES))
def test_tokens_replay_to_the_filtered_bytes(name):
    filt, _, tokens, n_tokens, hist = device_parse(name)
    assert np.array_equal(filt, C.filtered(name))
    for s, (v, k, data) in enumerate(segment_bytes(name, filt)):
        assert 1 <= n_tokens[s] <= len(data)
        toks = tokens[s, : n_tokens[s]]
        check_tokens(toks, data)
        assert np.array_equal(hist[s], R.histogram(toks)), (name, s)


def _parse(frame, rps, filter="none"):
    filtered, _ = ops.png_filter(dev(frame[None]), filter, rps)
    tokens, n_tokens, hist = ops.png_lz77(filtered, rps)
    assert n_tokens.numel() == 1
    n = int(n_tokens[0])
    return filtered.cpu().numpy().reshape(-1).tobytes(), tokens[0, :n].cpu().numpy().view(np.uint32), hist[0].cpu().numpy()


def test_distance_cap_in_a_segment_longer_than_the_window():
    """4 x 4096, one segment of 49156 bytes, filter None, random bytes whose last 3000 repeat the first 3000 from 46155 bytes back:
    the only copy lies outside the 32 KiB window, so nothing there may become a match"""
    flat = np.random.default_rng(11).integers(0, 256, 4 * 4096 * 3, dtype=np.uint8)
    flat[-3000:] = flat[:3000]
    data, toks, hist = _parse(flat.reshape(4, 4096, 3), 4)
    assert len(data) == 4 * (1 + 3 * 4096) and data[-3000:] == data[1:3001]
    split = check_tokens(toks, data)
    assert np.array_equal(hist, R.histogram(toks))
    pos = 0
    for tok in split:                                                            # inside the repeated tail: literals or chance matches only
        n = tok[1] if tok[0] == "match" else 1
        assert not (pos >= len(data) - 2990 and tok[0] == "match" and tok[1] > 8), (pos, tok)
        pos += n


def test_matches_across_the_16_bit_position_wrap():
    """6 x 4096, one segment of 73734 bytes: positions pass 65535, where the hash table's 16-bit entries wrap.  Bytes 70000 .. 71000
    repeat 64000 .. 65000 (distance 6000, candidate below the wrap, position above it) and 72000 .. 72500 repeat 3000 .. 3500 (69000
    back: outside the window, although the entry's low bits look 3464 bytes old)."""
    flat = np.random.default_rng(12).integers(0, 256, 6 * 4096 * 3, dtype=np.uint8).reshape(6, -1)
    filt = np.concatenate([np.zeros((6, 1), np.uint8), flat], axis=1).reshape(-1)
    filt[70000:71000] = filt[64000:65000]
    filt[72000:72500] = filt[3000:3500]
    frame = filt.reshape(6, -1)[:, 1:].reshape(6, 4096, 3)
    data, toks, hist = _parse(np.ascontiguousarray(frame), 6)
    assert len(data) == 73734 and data[70000:71000] == data[64000:65000] and data[72000:72500] == data[3000:3500]
    split = check_tokens(toks, data)
    assert np.array_equal(hist, R.histogram(toks))
    pos, long_matches, far = 0, 0, 0
    for tok in split:
        n = tok[1] if tok[0] == "match" else 1
        if tok[0] == "match" and 70000 <= pos < 71000 and tok[2] == 6000:
            long_matches += tok[1]
        if tok[0] == "match" and 72000 <= pos < 72500 and tok[1] > 8:
            far += 1
        pos += n
    assert long_matches >= 900 and far == 0


def test_constant_frame_gives_full_length_matches_to_the_last_byte():
    filt, _, tokens, n_tokens, _ = device_parse("constant_40x72")
    split = check_tokens(tokens[0, : n_tokens[0]], filt[0].tobytes())
    assert sum(1 for t in split if t[0] == "match" and t[1] == 258) >= 10
    assert split[-1][0] == "match"                                               # it ends on the segment's last byte: the replay is exact
    assert n_tokens[0] < 100                                                     # 8680 bytes
    # every segment of the ragged case ends in a match too, the last one 391 bytes long
    filt, _, tokens, n_tokens, _ = device_parse("constant_33x130")
    for s, (v, k, data) in enumerate(segment_bytes("constant_33x130", filt)):
        assert check_tokens(tokens[s, : n_tokens[s]], data)[-1][0] == "match"


# ------------------------------------------------------------------ stream
def _emit(name, guard=64):
    """-> (bytes of the guarded buffer, total, per-frame tables, seg_mode, seg_bytes) of the case's stream emitted on the device"""
    frames, _ = C.CASES[name]
    V, H, W, _ = frames.shape
    rps = C.rows_per_segment(name)
    filtered, _ = ops.png_filter(dev(frames), "adaptive", rps)
    tokens, n_tokens, hist = ops.png_lz77(filtered, rps)
    spf = len(C.segments(name))
    tables = [png.FrameTables(h) for h in hist.view(V, spf, -1).sum(dim=1).cpu().numpy()]
    luts, headers, header_bits = png.upload_tables(tables, "cuda")
    mode, seg_bytes, offsets, frame_bytes = png.segment_sizes(hist, tables, V, H, W, rps)
    total = int(frame_bytes.sum())
    buf = torch.full((total + 2 * guard,), GUARD, dtype=torch.uint8, device="cuda")
    ops.png_emit(tokens, n_tokens, filtered, mode, offsets, seg_bytes, luts, headers, header_bits, buf[guard: guard + total], rps)
    return buf.cpu().numpy().tobytes(), total, tables, mode.cpu().numpy(), seg_bytes.cpu().numpy()


@pytest.mark.parametrize("name", list(C.CASES))
def test_stream_equals_the_oracles_emission_of_the_device_tokens(name):
    filt, _, tokens, n_tokens, _ = device_parse(name)
    buf, total, tables, mode, seg_bytes = _emit(name)
    want, n_last = [], len(C.segments(name)) - 1
    for s, (v, k, data) in enumerate(segment_bytes(name, filt)):
        t = tables[v]
        coded = R.emit_segment(tokens[s, : n_tokens[s]], t.lit, t.dist, t.header, t.header_bits, k == n_last)
        stored = R.emit_stored(data, k == n_last)
        assert mode[s] == (1 if len(coded) >= len(stored) else 0), (name, s, len(coded), len(stored))
        want.append(stored if mode[s] else coded)
        assert seg_bytes[s] == len(want[-1]), (name, s)
    want = b"".join(want)
    assert total == len(want)                                                    # the sizes computed before the emission are exact
    assert buf[:64] == bytes([GUARD]) * 64 and buf[64 + total:] == bytes([GUARD]) * 64
    assert buf[64: 64 + total] == want
    assert _emit(name)[0] == buf                                                 # two calls, identical bytes
    if name.startswith("random_40x72"):
        assert mode.all()                                                        # uniform bytes: stored
    if name.startswith("mixed_40x72"):
        assert mode.tolist() == [0, 0, 1]                                        # per frame: texture and constant coded, random stored


def test_emit_skips_a_segment_that_leaves_the_buffer():
    name = "mixed_33x130"
    frames, _ = C.CASES[name]
    V, H, W, _ = frames.shape
    rps = C.rows_per_segment(name)
    filtered, _ = ops.png_filter(dev(frames), "adaptive", rps)
    tokens, n_tokens, hist = ops.png_lz77(filtered, rps)
    tables = [png.FrameTables(h) for h in hist.view(V, 5, -1).sum(dim=1).cpu().numpy()]
    luts, headers, header_bits = png.upload_tables(tables, "cuda")
    mode, seg_bytes, offsets, frame_bytes = png.segment_sizes(hist, tables, V, H, W, rps)
    total = int(frame_bytes.sum())
    full = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    ops.png_emit(tokens, n_tokens, filtered, mode, offsets, seg_bytes, luts, headers, header_bits, full, rps)
    cut = int(offsets[-1]) + 1                                                   # the last segment no longer fits; negative offsets neither
    offsets2 = offsets.clone()
    offsets2[0] = -1
    buf = torch.full((total,), GUARD, dtype=torch.uint8, device="cuda")
    ops.png_emit(tokens, n_tokens, filtered, mode, offsets2, seg_bytes, luts, headers, header_bits, buf[:cut], rps)
    first = int(seg_bytes[0])
    assert (buf[:first] == GUARD).all() and (buf[int(offsets[-1]):] == GUARD).all()
    assert torch.equal(buf[first: int(offsets[-1])], full[first: int(offsets[-1])])


# ------------------------------------------------------------------ files
@pytest.mark.parametrize("name", list(C.CASES))
def test_files_decode_to_the_input(name):
    frames, rps = C.CASES[name]
    files = png.encode_png(dev(frames), rows_per_segment=rps)
    assert len(files) == len(frames)
    for v, (data, frame) in enumerate(zip(files, frames)):
        kinds = R.chunks(data)                                                   # lengths and CRCs
        assert [k for k, _ in kinds] == [b"IHDR", b"IDAT", b"IEND"]
        H, W, _ = frame.shape
        assert kinds[0][1] == W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 2, 0, 0, 0]) and kinds[1][1][:2] == b"\x78\x01"
        assert zlib.decompress(kinds[1][1]) == C.filtered(name)[v].tobytes()     # zlib checks the Adler-32
        img = Image.open(io.BytesIO(data))
        assert img.mode == "RGB" and np.array_equal(np.asarray(img), frame), (name, v)


def test_forced_filters_and_batches_decode_too(monkeypatch):
    frames = np.stack([C.black_areas(21, 50, s) for s in range(5)])
    for f in ("none", "sub", "up", "average", "paeth"):
        for data, frame in zip(png.encode_png(dev(frames[:2]), filter=f, rows_per_segment=4), frames):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), frame)
    whole = png.encode_png(dev(frames))
    monkeypatch.setattr(png, "TOKEN_WORKSPACE_BYTES", 2 * 4 * 21 * 151)         # two frames per batch: 2 + 2 + 1
    assert png.frames_per_batch(21, 50) == 2 and png.encode_png(dev(frames)) == whole
    assert png.encode_png(dev(frames[3])) == whole[3:4]                         # one frame [H,W,3]


# ------------------------------------------------------------------ sizes
def _pillow_size(frame):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "PNG")
    return len(b.getvalue())


def test_sizes_that_can_be_derived():
    """256 x 512, raw = 393216 bytes.  Constant: runs cost a few bits per 258 bytes, plus 13 segment headers -- at most 2 % of raw.
    Uniform random bytes: the stored fallback holds -- at most raw x 1.01 + 1 KiB."""
    raw = 256 * 512 * 3
    const, rand = png.encode_png(dev(np.stack([C.constant(256, 512), C.random_bytes(256, 512, 7)])))
    print(f"constant {len(const)} bytes = {len(const) / raw:.4f} of raw; random {len(rand)} bytes = {len(rand) / raw:.4f} of raw")
    assert len(const) <= 0.02 * raw
    assert len(rand) <= raw * 1.01 + 1024
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(rand))), C.random_bytes(256, 512, 7))


# file size / Pillow's size at its default settings on the 256 x 512 frames, as measured on an MI355X host (DESIGN.md 4.7,
# profiles/png_bench.json: 7262 / 2982, 271409 / 256167, 258030 / 225646 bytes).  Our bytes are a deterministic function of the frame, so
# the ratio moves only with Pillow / zlib: the 10 % margin below is for their versions, not for kernel changes.
MEASURED_RATIO = {"gradient": 2.435, "texture": 1.060, "noise4": 1.144}


@pytest.mark.parametrize("content", list(MEASURED_RATIO))
def test_size_ratio_to_pillow(content):
    frame = C.CONTENTS[content](256, 512)
    data = png.encode_png(dev(frame))[0]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), frame)
    ratio = len(data) / _pillow_size(frame)
    print(f"{content}: {len(data)} bytes, Pillow {_pillow_size(frame)}, ratio {ratio:.4f}")
    assert ratio <= MEASURED_RATIO[content] * 1.10


# ------------------------------------------------------------------ wiring
def _decoded(folder):
    return {n: np.asarray(Image.open(os.path.join(folder, n))) for n in sorted(os.listdir(folder)) if n.endswith(".png")}


def test_write_png_frames_names_like_save_u8_frames(tmp_path):
    from evoworld_amd.frames import write_numbered                              # the writer of every frame dump, episode and CLI
    frames = dev(np.stack([C.texture(12, 20, s) for s in range(3)]))
    write_numbered(str(tmp_path / "a"), frames, 24)
    paths = png.write_png_frames(str(tmp_path / "b"), frames, 24)
    write_numbered(str(tmp_path / "c"), frames, 24, on_device=True)
    assert [os.path.basename(p) for p in paths] == sorted(os.listdir(tmp_path / "a")) == ["025.png", "026.png", "027.png"]
    a, b, c = _decoded(tmp_path / "a"), _decoded(tmp_path / "b"), _decoded(tmp_path / "c")
    assert list(a) == list(b) == list(c) and all(np.array_equal(a[n], b[n]) and np.array_equal(a[n], c[n]) for n in a)
    assert open(tmp_path / "b" / "025.png", "rb").read() == open(tmp_path / "c" / "025.png", "rb").read()
    assert write_numbered(str(tmp_path / "e"), frames, 24, True) == [str(tmp_path / "e" / n) for n in a]     # as both CLI paths call it
    assert sorted(os.listdir(tmp_path / "e")) == list(a)
    assert open(tmp_path / "e" / "026.png", "rb").read() == open(tmp_path / "b" / "026.png", "rb").read()
    assert png.write_png(str(tmp_path / "one.png"), frames[1]) == os.path.getsize(tmp_path / "one.png")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "one.png")), frames[1].cpu().numpy())
    assert [os.path.basename(p) for p in png.write_png_frames(str(tmp_path / "d"), frames, 0, 2)] == ["01.png", "02.png", "03.png"]


def test_process_episode_writes_the_same_files_on_the_device(tiny, tmp_path):  # noqa: F811
    """the tiny two-segment episode of test_gpu_inference with png_on_device against the default: same names, same pixels, same frames --
    and the default run does not import evoworld_amd.png"""
    from evoworld_amd.inference import UnifiedLoopConsistencyPipeline
    from evoworld_amd.stages import SyntheticStages
    cfg, pipe = tiny
    H, W, T = 128, 256, 25
    i = np.arange(60, dtype=np.float64)
    cam = np.stack([0.04 * i * np.sin(i / 9), 0 * i, 0.04 * i * np.cos(i / 9), 0 * i, 95 + 3.6 * i, 0 * i], 1)
    st = SyntheticStages(cross_attention_dim=cfg["cross_attention_dim"], camera_params=cam, depth_hw=(48, 64))
    saved = (pipe.vae, pipe.image_encoder, pipe.vae_scale_factor)
    pipe.set_components(vae=st.vae, image_encoder=st.image_encoder)
    kept = {k: sys.modules.pop(k) for k in [k for k in sys.modules if k == "evoworld_amd.png"]}
    try:
        loop = UnifiedLoopConsistencyPipeline(pipe, st.depth_model, height=H, width=W, num_frames=T, num_segments=2,
                                              num_inference_steps=1, pano_size=(64, 128), face_res=32)
        start = (torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1).to("cuda")
        a = loop.process_episode(start, cam, save_dir=str(tmp_path / "host"), save_segment_frames=True)
        assert "evoworld_amd.png" not in sys.modules                             # the default path never reaches the new code
        sys.modules.update(kept)
        b = loop.process_episode(start, cam, save_dir=str(tmp_path / "device"), save_segment_frames=True, png_on_device=True)
    finally:
        sys.modules.update(kept)
        pipe.vae, pipe.image_encoder, pipe.vae_scale_factor = saved
    assert torch.equal(a, b)
    folders = sorted(os.listdir(tmp_path / "host"))
    assert folders == sorted(os.listdir(tmp_path / "device"))
    assert {"perspective_look_at_center_0", "predictions_0", "predictions_1", "rendered_panorama_vggt_open3d_0"} <= set(folders)
    n = 0
    for d in (f for f in folders if os.path.isdir(tmp_path / "host" / f)):
        host, device = _decoded(tmp_path / "host" / d), _decoded(tmp_path / "device" / d)
        assert list(host) == list(device) and len(host) >= 24
        for name in host:
            assert np.array_equal(host[name], device[name]), (d, name)
            with open(tmp_path / "device" / d / name, "rb") as f:
                assert [k for k, _ in R.chunks(f.read())] == [b"IHDR", b"IDAT", b"IEND"]      # ours: one IDAT, no ancillary chunk
            n += 1
    assert n == 25 + 24 + 25 + 24


def test_video_extract_device_png(tmp_path):
    from evoworld_amd import video
    frames = dev(np.stack([C.texture(24, 40, s) for s in range(3)]))
    video.write_video(str(tmp_path / "a.avi"), frames, fps=5)
    video.main(["extract", "--input", str(tmp_path / "a.avi"), "--output", str(tmp_path / "host"), "--format", "png"])
    video.main(["extract", "--input", str(tmp_path / "a.avi"), "--output", str(tmp_path / "device"), "--format", "png", "--device_png"])
    host, device = _decoded(tmp_path / "host"), _decoded(tmp_path / "device")
    assert list(host) == list(device) == ["001.png", "002.png", "003.png"]
    assert all(np.array_equal(host[n], device[n]) for n in host)
    png.main(["encode", "--input", str(tmp_path / "a.avi"), "--output", str(tmp_path / "cli")])
    cli = _decoded(tmp_path / "cli")
    assert list(cli) == list(host) and all(np.array_equal(host[n], cli[n]) for n in host)
    png.main(["encode", "--input", str(tmp_path / "host"), "--output", str(tmp_path / "cli2"), "--filter", "paeth", "--rows_per_segment", "5"])
    assert all(np.array_equal(host[n], a) for n, a in _decoded(tmp_path / "cli2").items())


def test_cubemap_cli_device_png(tmp_path):
    from evoworld_amd import cubemap
    os.makedirs(tmp_path / "in")
    for s in range(2):
        Image.fromarray(C.texture(32, 64, s)).save(tmp_path / "in" / f"{s + 1:03}.png")
    cubemap.main(["to-cubemap", "--input", str(tmp_path / "in"), "--output", str(tmp_path / "host")])
    cubemap.main(["to-cubemap", "--input", str(tmp_path / "in"), "--output", str(tmp_path / "device"), "--device_png"])
    host, device = _decoded(tmp_path / "host"), _decoded(tmp_path / "device")
    assert list(host) == list(device) and len(host) == 14 and all(np.array_equal(host[n], device[n]) for n in host)
    cubemap.main(["to-pano", "--input", str(tmp_path / "host"), "--output", str(tmp_path / "p0"), "--size", "64", "32"])
    cubemap.main(["to-pano", "--input", str(tmp_path / "host"), "--output", str(tmp_path / "p1"), "--size", "64", "32", "--device_png"])
    p0, p1 = _decoded(tmp_path / "p0"), _decoded(tmp_path / "p1")
    assert list(p0) == list(p1) == ["001.png", "002.png"] and all(np.array_equal(p0[n], p1[n]) for n in p0)


def test_memory_panoramas_on_the_device(tmp_path):
    """CubemapRenderer.render_cubemaps_to_panoramas, the writer the episode test reaches only through process_episode: with an outdir it
    leaves 00.png .. (two digits, from zero) holding the panoramas it returns, whichever encoder wrote them; without one, no file."""
    from evoworld_amd.reprojection import CubemapRenderer
    g = torch.Generator().manual_seed(5)
    xyz = (torch.rand(4000, 3, generator=g) * 4 - 2).cuda()                     # a cloud around the three cameras: every face sees points
    rgb = torch.randint(0, 256, (4000, 3), generator=g, dtype=torch.uint8).cuda()
    c2w = np.repeat(np.eye(4)[None], 3, 0)
    c2w[:, 0, 3] = [0.0, 0.2, 0.4]
    cr = CubemapRenderer(face_res=32)
    host = cr.render_cubemaps_to_panoramas(xyz, rgb, c2w, 3, str(tmp_path / "host"), width=128, height=64)
    device = cr.render_cubemaps_to_panoramas(xyz, rgb, c2w, 3, str(tmp_path / "new" / "device"), width=128, height=64, png_on_device=True)
    none = cr.render_cubemaps_to_panoramas(xyz, rgb, c2w, 3, None, width=128, height=64, png_on_device=True)
    assert host.shape == (3, 64, 128, 3) and torch.equal(host, device) and torch.equal(host, none)
    assert len({p.cpu().numpy().tobytes() for p in host}) == 3 and all(bool(p.any()) for p in host)      # three different views, none blank
    a, b = _decoded(tmp_path / "host"), _decoded(tmp_path / "new" / "device")
    assert list(a) == list(b) == ["00.png", "01.png", "02.png"] == sorted(os.listdir(tmp_path / "host"))
    assert sorted(os.listdir(tmp_path)) == ["host", "new"]
    for k, n in enumerate(a):
        assert np.array_equal(a[n], host[k].cpu().numpy()) and np.array_equal(b[n], a[n]), n
