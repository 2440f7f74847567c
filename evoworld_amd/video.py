"""Video files of generated clips: Motion-JPEG in AVI, the frames encoded on the device (csrc/video.hip).

The reference writes its clips through imageio / ffmpeg (Navigator.save_video, evoworld/inference/navigator_evoworld.py:233-257) and
its calculate_scores.py loads navigated.mp4 / original.mp4 per episode.  No H.264 encoder (ffmpeg, imageio, PyAV, cv2) exists here, so
the container is written by hand, as the GLB was: every frame is a stand-alone baseline JPEG whose scan data come from the GPU
(ops.jpeg_dct_quant -> ops.jpeg_entropy -> ops.jpeg_pack; only the compressed stream crosses to the host), wrapped in a RIFF `AVI `
file with one MJPG video stream and an idx1 index.  ffplay, VLC and cv2.VideoCapture read that layout; none of them is available to
test against (unpinned), so the tests check the container field by field and the frames through libjpeg (Pillow).

The way back runs on the device too (csrc/video_decode.hip): the host parses the headers and cuts the scan into restart
segments, the scan bytes are uploaded once, and Huffman decoding, inverse DCT, chroma upsampling and the colour transform are kernels
(ops.jpeg_huffman_decode -> ops.jpeg_idct -> ops.jpeg_planes_to_rgb).  It reads any baseline 4:2:0 / 4:4:4 JPEG with one interleaved
scan, not only this module's own; `scores` is calculate_scores.py on the two AVIs of every episode folder.

  quant_tables / jpeg_header / encode_jpeg     the frames
  parse_jpeg / decode_jpeg                     and back (scan_batch, huffman_device_tables: what the Huffman kernel is handed)
  write_avi / read_avi / write_video           the container
  read_video                                   X.avi -> (uint8 [V,H,W,3] on the device, fps)
  video_scores                                 a folder of episodes -> calculate_scores.py's result
  python -m evoworld_amd.video encode --input DIR --output X.avi [--fps 10 --quality 90 --subsampling 4:2:0]
  python -m evoworld_amd.video extract --input X.avi --output DIR [--format jpg|png]
  python -m evoworld_amd.video scores --input_folder DIR [--target_size 64 --lpips_weights ... --fvd_weights ... --result_file X.json]
"""
import argparse
import os
import struct
import sys
from fractions import Fraction

import numpy as np

SUBSAMPLINGS = ("4:2:0", "4:4:4")
MCU_SIZE = {"4:2:0": 16, "4:4:4": 8}
AVI_MAX_BYTES = 2 ** 31                   # RIFF sizes beyond 2 GiB need OpenDML, which is not written

# zigzag position -> natural index (T.81 figure A.6)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# T.81 tables K.1 / K.2 in natural order
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
           103, 99)
K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66) + (99,) * 38
# T.81 tables K.3 - K.6 as (codes per length 1..16, symbols in code order); the kernel holds the same four (csrc/video.hip)
HUFFMAN = {
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
             (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
              0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
              0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
              0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
              0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
              0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
              0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
              0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
             (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
              0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
              0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
              0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
              0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
              0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
              0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
              0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa)),
}


# ------------------------------------------------------------------ frames
def _check_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"quality must be an integer 1..100, got {quality!r}")
    return int(quality)


def _check_subsampling(subsampling):
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"subsampling must be one of {SUBSAMPLINGS}, got {subsampling!r}")
    return subsampling


def quant_tables(quality):
    """(luminance, chrominance) int arrays [64] in natural order: T.81 K.1 / K.2 under libjpeg's quality rule (jpeg_quality_scaling,
    jpeg_add_quant_table with force_baseline): scale = 5000 // q below 50, 200 - 2 q otherwise; (t * scale + 50) // 100 in 1..255."""
    q = _check_quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(t, dtype=np.int64) * scale + 50) // 100, 1, 255) for t in (K1_LUMA, K2_CHROMA))


def _segment(marker, payload):
    return bytes((0xFF, marker)) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_header(width, height, quality=90, subsampling="4:2:0"):
    """Everything in front of a frame's scan data: SOI, APP0 / JFIF, both DQT, SOF0, the four DHT, DRI (one MCU row), SOS."""
    _check_subsampling(subsampling)
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"a JPEG is 1..65535 pixels wide and high, got {width} x {height}")
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))
    for i, t in enumerate((ql, qc)):
        out += _segment(0xDB, bytes((i,)) + bytes(int(t[k]) for k in ZIGZAG))
    sampling = 0x22 if subsampling == "4:2:0" else 0x11
    out += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes((1, sampling, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for cls, idx in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = HUFFMAN[(cls, idx)]
        out += _segment(0xC4, bytes((cls << 4 | idx,)) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", -(-width // MCU_SIZE[subsampling])))
    return out + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def _frames_u8(frames):
    """uint8 [V,H,W,3], or float [V,3,H,W] in [-1,1] (the pipeline's 8-bit mapping), on the device"""
    import torch

    from . import ops
    if not isinstance(frames, torch.Tensor) or frames.ndim != 4:
        raise TypeError("frames must be a 4-D device tensor: uint8 [V,H,W,3] or float [V,3,H,W] in [-1,1]")
    if frames.dtype == torch.uint8:
        if frames.shape[3] != 3:
            raise ValueError(f"uint8 frames must be [V,H,W,3], got {tuple(frames.shape)}")
        return frames.contiguous()
    if not frames.is_floating_point() or frames.shape[1] != 3:
        raise ValueError(f"float frames must be [V,3,H,W], got {tuple(frames.shape)} {frames.dtype}")
    return ops.f32_chw_to_u8_hwc(frames.float().contiguous())


def encode_jpeg(frames, quality=90, subsampling="4:2:0"):
    """frames uint8 [V,H,W,3] or float [V,3,H,W] in [-1,1], on the device -> list of V stand-alone baseline JPEGs (bytes).
    Colour transform, DCT, quantisation and Huffman coding run on the device; the host adds the headers and EOI."""
    from . import ops
    quality, subsampling = _check_quality(quality), _check_subsampling(subsampling)
    u8 = _frames_u8(frames)
    V, H, W, _ = u8.shape
    if V == 0:
        return []
    coef = ops.jpeg_dct_quant(u8, quality, subsampling)
    stream, frame_bytes = ops.jpeg_pack(*ops.jpeg_entropy(coef), coef.shape[1])
    data = stream.cpu().numpy().tobytes()
    head, out, at = jpeg_header(W, H, quality, subsampling), [], 0
    for n in frame_bytes.tolist():
        out.append(head + data[at: at + n] + b"\xff\xd9")
        at += n
    return out


# ------------------------------------------------------------------ container
def _chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _rate_scale(fps):
    f = Fraction(fps).limit_denominator(1001)
    if f <= 0:
        raise ValueError(f"fps must be positive, got {fps!r}")
    return f.numerator, f.denominator


def write_avi(path, jpegs, width, height, fps=10):
    """A RIFF `AVI ` file with one MJPG video stream: LIST hdrl (avih, LIST strl (strh vids / MJPG with rate / scale from fps, strf =
    BITMAPINFOHEADER with biCompression MJPG)), LIST movi of `00dc` chunks padded to even length, and idx1 (offsets relative to the
    `movi` tag).  ValueError when the file would pass 2 GiB (OpenDML is not supported) or there is no frame."""
    jpegs = list(jpegs)
    if not jpegs:
        raise ValueError("write_avi: no frames")
    rate, scale = _rate_scale(fps)
    n = len(jpegs)
    movi_bytes = 4 + sum(8 + len(j) + (len(j) & 1) for j in jpegs)
    total = 12 + (8 + 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))) + (8 + movi_bytes) + (8 + 16 * n)
    if total >= AVI_MAX_BYTES:
        raise ValueError(f"write_avi: {n} frames make a file of {total} bytes; an AVI without OpenDML extensions ends at 2 GiB "
                         "(split the clip, or lower the quality)")
    biggest = max(len(j) for j in jpegs)
    usec = (1000000 * scale + rate // 2) // rate
    avih = struct.pack("<14I", usec, (biggest * rate + scale - 1) // scale, 0, 0x10, n, 0, 1, biggest, width, height, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIIIHHHH", 0, 0, 0, 0, scale, rate, 0, n, biggest, 0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    strl = b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
    hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", strl)
    index, at = [], 4
    for j in jpegs:
        index.append(struct.pack("<4sIII", b"00dc", 0x10, at, len(j)))
        at += 8 + len(j) + (len(j) & 1)
    assert at == movi_bytes
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI ")
        f.write(_chunk(b"LIST", hdrl))
        f.write(b"LIST" + struct.pack("<I", movi_bytes) + b"movi")
        for j in jpegs:
            f.write(_chunk(b"00dc", j))
        f.write(_chunk(b"idx1", b"".join(index)))
        assert f.tell() == total
    return total


def _walk(data, start, end):
    """(fourcc, payload start, payload size) of the chunks in data[start:end]"""
    at = start
    while at + 8 <= end:
        size = struct.unpack_from("<I", data, at + 4)[0]
        yield data[at: at + 4], at + 8, size
        at += 8 + size + (size & 1)


def read_avi(path):
    """-> (fps, width, height, [jpeg bytes]) of an MJPG AVI as write_avi lays it out (frames in movi order)"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    fps = width = height = None
    frames = []
    for cc, at, size in _walk(data, 12, min(len(data), 8 + struct.unpack_from("<I", data, 4)[0])):
        if cc != b"LIST":
            continue
        kind = data[at: at + 4]
        if kind == b"hdrl":
            for c2, a2, s2 in _walk(data, at + 4, at + size):
                if c2 == b"avih":
                    width, height = struct.unpack_from("<II", data, a2 + 32)
                elif c2 == b"LIST" and data[a2: a2 + 4] == b"strl":
                    for c3, a3, s3 in _walk(data, a2 + 4, a2 + s2):
                        if c3 == b"strh":
                            if data[a3: a3 + 8] != b"vidsMJPG":
                                raise ValueError(f"{path}: the stream is {data[a3: a3 + 8]!r}, not an MJPG video stream")
                            scale, rate = struct.unpack_from("<II", data, a3 + 20)
                            fps = rate / scale
        elif kind == b"movi":
            frames = [data[a2: a2 + s2] for c2, a2, s2 in _walk(data, at + 4, at + size) if c2 == b"00dc"]
    if fps is None or width is None:
        raise ValueError(f"{path}: no avih / strh header")
    return fps, width, height, frames


def write_video(path, frames, fps=10, quality=90, subsampling="4:2:0"):
    """frames (uint8 [V,H,W,3] or float [V,3,H,W] in [-1,1], on the device) -> an MJPEG AVI at `path`; returns the file's size."""
    if not str(path).lower().endswith(".avi"):
        raise ValueError(f"{path}: only Motion-JPEG AVI is produced (give a path ending in .avi): no H.264 encoder (ffmpeg, imageio, "
                         "PyAV, cv2) exists here, so .mp4 and the like cannot be written")
    u8 = _frames_u8(frames)
    return write_avi(path, encode_jpeg(u8, quality, subsampling), u8.shape[2], u8.shape[1], fps)


# ------------------------------------------------------------------ reading frames back
HUFF_TABLE_BYTES = 1424                   # EW_JPEG_HUFF_TABLE_BYTES: look uint16 [512], maxcode int32 [18], valoff int32 [18], vals uint8 [256]
_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xC5: "differential sequential (SOF5)",
              0xC6: "differential progressive (SOF6)", 0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic-coded sequential (SOF9)",
              0xCA: "arithmetic-coded progressive (SOF10)", 0xCB: "arithmetic-coded lossless (SOF11)", 0xCD: "arithmetic-coded differential (SOF13)",
              0xCE: "arithmetic-coded differential progressive (SOF14)", 0xCF: "arithmetic-coded differential lossless (SOF15)"}


def _scan_markers(data, start):
    """offsets, from byte `start` on, of every FF that is followed by neither 00 (a stuffed byte) nor FF (fill)"""
    a = np.frombuffer(data, np.uint8)[start:]
    return np.flatnonzero((a[:-1] == 0xFF) & (a[1:] != 0) & (a[1:] != 0xFF)) + start if len(a) > 1 else np.zeros(0, np.int64)


def _scan_end(data, start):
    """(offset of the first marker behind the scan data that is no RSTm, offsets of the RSTm markers in front of it)"""
    marks = _scan_markers(data, start)
    codes = np.frombuffer(data, np.uint8)[marks + 1]
    other = np.flatnonzero((codes < 0xD0) | (codes > 0xD7))
    if not len(other):
        raise ValueError("truncated JPEG: the scan data are not closed by a marker (EOI)")
    end = int(marks[other[0]])
    if codes[other[0]] != 0xD9:
        raise ValueError(f"the scan is followed by marker FF {codes[other[0]]:02X} at byte {end}: several scans (or tables between them) "
                         "are not decoded, only one interleaved scan")
    return end, marks[:other[0]]


def _check_huffman(bits, vals, name):
    code = 0
    for length, n in enumerate(bits, 1):
        code = (code + n) << 1
        if code > 2 << length:
            raise ValueError(f"{name}: the code lengths {list(bits)} describe no prefix code")
    if len(vals) != sum(bits) or len(vals) > 256:
        raise ValueError(f"{name}: {sum(bits)} codes but {len(vals)} symbols")


def parse_jpeg(data):
    """The headers of one JPEG stream, read on the host -> dict: width, height, subsampling ("4:2:0" | "4:4:4"), qtables (luminance,
    chrominance: int arrays [64] in natural order), huffman ((bits [16], symbols) of DC luminance, DC chrominance, AC luminance, AC
    chrominance, resolved through the scan's table selectors), restart_interval (MCUs, 0 = none), scan_offset and scan_bytes (the
    entropy-coded data, RSTm markers included, EOI excluded).
    Accepted: baseline sequential (SOF0), 8 bit, three components sampled 22 11 11 or 11 11 11 whose two chroma components share their
    tables, one interleaved scan, any DQT / DHT / DRI; APPn and COM segments are skipped.  ValueError names anything else."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG stream: it does not start with SOI (FF D8)")
    at, qt, huff, frame, dri = 2, {}, {}, None, 0
    while True:
        if at + 4 > len(data):
            raise ValueError(f"truncated JPEG: the headers end at byte {len(data)} without a scan (SOS)")
        if data[at] != 0xFF:
            raise ValueError(f"byte {at}: {data[at]:02X} where a marker should start")
        m = data[at + 1]
        if m == 0xFF:
            at += 1
            continue
        if m == 0xD9 or 0xD0 <= m <= 0xD8 or m == 0x01:
            raise ValueError(f"byte {at}: marker FF {m:02X} in front of the scan")
        n = int.from_bytes(data[at + 2: at + 4], "big")
        if n < 2 or at + 2 + n > len(data):
            raise ValueError(f"truncated JPEG: the segment FF {m:02X} at byte {at} claims {n} bytes, the stream ends at {len(data)}")
        p = data[at + 4: at + 2 + n]
        at += 2 + n
        if m in _SOF_NAMES:
            raise ValueError(f"{_SOF_NAMES[m]} JPEG: only baseline sequential (SOF0) streams are decoded")
        if m == 0xCC:
            raise ValueError("arithmetic coding (DAC segment): only Huffman-coded baseline streams are decoded")
        if m == 0xC0:
            if frame is not None:
                raise ValueError("a second SOF0 segment")
            if len(p) < 6 or len(p) != 6 + 3 * p[5]:
                raise ValueError("malformed SOF0 segment")
            precision, height, width, ncomp = p[0], int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big"), p[5]
            if precision != 8:
                raise ValueError(f"{precision} bit samples: only 8 bit streams are decoded")
            if ncomp != 3:
                raise ValueError(f"{ncomp} component{'s' if ncomp > 1 else ' (greyscale)'}: only three-component YCbCr streams are decoded")
            comps = [(p[6 + 3 * i], p[7 + 3 * i], p[8 + 3 * i]) for i in range(3)]
            sampling = tuple(c[1] for c in comps)
            if sampling not in ((0x22, 0x11, 0x11), (0x11, 0x11, 0x11)):
                raise ValueError(f"sampling factors {' '.join(f'{v:02X}' for v in sampling)}: only 22 11 11 (4:2:0) and 11 11 11 (4:4:4) are "
                                 "decoded (4:2:2 and the others are not)")
            if width < 1 or height < 1:
                raise ValueError(f"a frame of {width} x {height} pixels (DNL is not supported)")
            frame = (width, height, comps)
        elif m == 0xDB:
            while p:
                if p[0] >> 4:
                    raise ValueError("16-bit quantisation table: only 8 bit baseline streams are decoded (12 bit is not)")
                if len(p) < 65:
                    raise ValueError("malformed DQT segment")
                t = np.zeros(64, np.int64)
                t[list(ZIGZAG)] = list(p[1:65])
                qt[p[0] & 15], p = t, p[65:]
        elif m == 0xC4:
            while p:
                if len(p) < 17 or len(p) < 17 + sum(p[1:17]) or p[0] >> 4 > 1:
                    raise ValueError("malformed DHT segment")
                bits = tuple(p[1:17])
                vals = tuple(p[17: 17 + sum(bits)])
                _check_huffman(bits, vals, f"Huffman table {'AC' if p[0] >> 4 else 'DC'} {p[0] & 15}")
                huff[(p[0] >> 4, p[0] & 15)], p = (bits, vals), p[17 + sum(bits):]
        elif m == 0xDD:
            if len(p) != 2:
                raise ValueError("malformed DRI segment")
            dri = int.from_bytes(p, "big")
        elif m == 0xDA:
            if frame is None:
                raise ValueError("a scan (SOS) in front of the frame header (SOF0)")
            width, height, comps = frame
            if not p or p[0] != 3 or len(p) != 10:
                raise ValueError(f"a scan of {p[0] if p else 0} component(s): only one interleaved scan of all three is decoded (several "
                                 "scans are not)")
            if [p[1], p[3], p[5]] != [c[0] for c in comps]:
                raise ValueError("the scan lists the components in another order than the frame header")
            if tuple(p[7:10]) != (0, 63, 0):
                raise ValueError("a spectral selection or successive approximation (progressive scan parameters) in the scan header")
            sel = [(p[2 + 2 * i] >> 4, p[2 + 2 * i] & 15, comps[i][2]) for i in range(3)]          # (DC table, AC table, quantisation table)
            if sel[1] != sel[2]:
                raise ValueError("Cb and Cr use different tables: not decoded")
            for dc, ac, tq in sel[:2]:
                missing = [name for name, have in ((f"DHT DC {dc}", (0, dc) in huff), (f"DHT AC {ac}", (1, ac) in huff), (f"DQT {tq}", tq in qt))
                           if not have]
                if missing:
                    raise ValueError(f"missing table: {', '.join(missing)}")
            end, _ = _scan_end(data, at)
            return {"width": width, "height": height, "subsampling": "4:2:0" if comps[0][1] == 0x22 else "4:4:4",
                    "qtables": (qt[sel[0][2]], qt[sel[1][2]]),
                    "huffman": (huff[(0, sel[0][0])], huff[(0, sel[1][0])], huff[(1, sel[0][1])], huff[(1, sel[1][1])]),
                    "restart_interval": dri, "scan_offset": at, "scan_bytes": end - at}
        # APPn, COM and anything else with a length: skipped


def huffman_device_tables(tables):
    """((bits, symbols) x 4, as parse_jpeg returns them) -> uint8 [4 * HUFF_TABLE_BYTES], the form ew_jpeg_huffman_decode reads: per table
    a 9-bit prefix lookup (length << 8 | symbol), the canonical maxcode / valoff of the lengths 1..16 (T.81 F.2.2.3) and the symbols."""
    out = np.zeros((4, HUFF_TABLE_BYTES), np.uint8)
    for i, (bits, vals) in enumerate(tables):
        _check_huffman(bits, vals, f"Huffman table {i}")
        look, maxcode, valoff = np.zeros(512, "<u2"), np.full(18, -1, "<i4"), np.zeros(18, "<i4")
        sym = np.zeros(256, np.uint8)
        sym[:len(vals)] = vals
        code = k = 0
        for length in range(1, 17):
            n = bits[length - 1]
            if n:
                valoff[length] = k - code
                if length <= 9:
                    for j in range(n):
                        look[(code + j) << (9 - length): (code + j + 1) << (9 - length)] = (length << 8) | vals[k + j]
                code, k = code + n, k + n
                maxcode[length] = code - 1
            code <<= 1
        out[i] = np.concatenate([look.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), sym])
    return out.reshape(-1)


def _segment_table(data, info, frame):
    """(starts, lengths, scan bytes) of the restart segments of one frame's scan, relative to the scan's first byte; the RSTm markers are
    checked (count as the frame's size implies, indices 0..7 in a cycle) and left out."""
    mcu = MCU_SIZE[info["subsampling"]]
    mcus = -(-info["height"] // mcu) * -(-info["width"] // mcu)
    interval = info["restart_interval"]
    want = -(-mcus // interval) if 0 < interval < mcus else 1
    at = info["scan_offset"]
    end, rst = _scan_end(data, at)
    if len(rst) != want - 1:
        raise ValueError(f"frame {frame}: {len(rst)} restart markers, but {mcus} MCUs at restart interval {interval} make {want} segments")
    idx = np.frombuffer(data, np.uint8)[rst + 1] - 0xD0
    if not np.array_equal(idx, np.arange(len(rst)) % 8):
        bad = int(np.flatnonzero(idx != np.arange(len(rst)) % 8)[0])
        raise ValueError(f"frame {frame}: restart marker {bad} is RST{int(idx[bad])}, expected RST{bad % 8} (markers out of order)")
    starts = np.concatenate([[at], rst + 2]).astype(np.int64) - at
    ends = np.concatenate([rst, [end]]).astype(np.int64) - at
    return starts, ends - starts, end - at


def scan_batch(jpegs, info, names=None):
    """Frames with identical headers (info = parse_jpeg of any of them) -> what ops.jpeg_huffman_decode takes, on the host: (scan uint8
    [bytes]: the frames' entropy-coded data back to back, seg_start int64 [n], seg_bytes int32 [n]).  names: the frames' numbers for
    error messages."""
    starts, lengths, scans, base = [], [], [], 0
    for v, j in enumerate(jpegs):
        s, n, nbytes = _segment_table(j, info, v if names is None else names[v])
        starts.append(s + base)
        lengths.append(n)
        scans.append(j[info["scan_offset"]: info["scan_offset"] + nbytes])
        base += nbytes
    if base == 0:
        raise ValueError("empty scan")
    lengths = np.concatenate(lengths)
    if lengths.max() >= 2 ** 31:
        raise ValueError("a restart segment of 2 GiB or more")
    return np.frombuffer(b"".join(scans), np.uint8).copy(), np.concatenate(starts), lengths.astype(np.int32)


def decode_jpeg(jpegs, return_coefficients=False):
    """A list of JPEG streams of one frame size (bytes, as encode_jpeg and read_avi return them) -> uint8 [V,H,W,3] on the device.  The
    headers are parsed and the scans cut into restart segments on the host (parse_jpeg; vectorised numpy), the scan bytes go to the
    device once, and Huffman decoding, dequantisation, inverse DCT, chroma upsampling and the colour transform run there (ops.jpeg_huffman_decode
    -> ops.jpeg_idct -> ops.jpeg_planes_to_rgb), one batch of launches per group of frames with identical headers (a file
    of write_video is one group).  return_coefficients: stop behind the Huffman decoder and return the quantised coefficients int16
    [V, mcu_rows, mcu_cols, blocks_per_mcu, 64] (the layout of ops.jpeg_dct_quant) instead.  ValueError: a stream parse_jpeg refuses, mixed
    frame sizes (or samplings, for coefficients), a damaged segment (names the frame, the segment and the reason)."""
    import torch

    from . import ops
    jpegs = [bytes(j) for j in jpegs]
    if not jpegs:
        raise ValueError("decode_jpeg: no frames")
    infos, groups = [], {}
    for v, j in enumerate(jpegs):
        try:
            info = parse_jpeg(j)
        except ValueError as e:
            raise ValueError(f"frame {v}: {e}") from None
        infos.append(info)
        groups.setdefault(j[:info["scan_offset"]], []).append(v)
    first = infos[0]
    for v, info in enumerate(infos):
        if (info["width"], info["height"]) != (first["width"], first["height"]):
            raise ValueError(f"mixed frame sizes: frame 0 is {first['width']} x {first['height']}, frame {v} is {info['width']} x {info['height']}")
        if return_coefficients and info["subsampling"] != first["subsampling"]:
            raise ValueError(f"mixed samplings: frame 0 is {first['subsampling']}, frame {v} is {info['subsampling']}")
    W, H = first["width"], first["height"]
    out = None
    for members in groups.values():
        info = infos[members[0]]
        sub = info["subsampling"]
        mcu, bpm = MCU_SIZE[sub], ops.JPEG_SAMPLING[sub][2]
        mr, mc = -(-H // mcu), -(-W // mcu)
        scan, starts, lengths = scan_batch([jpegs[v] for v in members], info, members)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        coef, status = ops.jpeg_huffman_decode(dev(scan), dev(starts), dev(lengths), dev(huffman_device_tables(info["huffman"])),
                                               len(members), mr, mc, bpm, info["restart_interval"])
        status = status.cpu().numpy()
        if status.any():
            s = int(np.flatnonzero(status)[0])
            per = len(status) // len(members)
            raise ValueError(f"frame {members[s // per]}, restart segment {s % per}: {ops.JPEG_SEG_STATUS.get(int(status[s]), status[s])} "
                             f"(status {int(status[s])}; {int((status != 0).sum())} of {len(status)} segments are damaged)")
        if return_coefficients:
            got = coef
        else:
            qt = dev(np.stack(info["qtables"]).astype(np.uint8))
            got = ops.jpeg_planes_to_rgb(ops.jpeg_idct(coef, qt), H, W, sub)
        if len(groups) == 1:
            return got
        if out is None:
            out = torch.empty(len(jpegs), *got.shape[1:], dtype=got.dtype, device=got.device)
        out[torch.tensor(members, device=got.device)] = got
    return out


def read_video(path):
    """An MJPG AVI (write_video's, or any whose frames parse_jpeg accepts) -> (frames uint8 [V,H,W,3] on the device, fps)"""
    fps, width, height, jpegs = read_avi(path)
    if not jpegs:
        raise ValueError(f"{path}: no frames")
    frames = decode_jpeg(jpegs)
    if (frames.shape[2], frames.shape[1]) != (width, height):
        raise ValueError(f"{path}: the container says {width} x {height}, the frames are {frames.shape[2]} x {frames.shape[1]}")
    return frames, fps


def video_scores(input_folder, target_size=64, lpips_weights=None, fvd_weights=None, channel_order="rgb"):
    """calculate_scores.py's main on MJPEG AVIs: every sub-folder of input_folder that holds both navigated.avi and original.avi is one
    video; the frames are decoded on the device, resized to target_size x target_size (ops.resize_linear_u8, the restatement of
    cv2.resize's default), stacked to [N,T,3,h,w] in [0,1] and scored once as a batch, navigated first.  -> the result dict (fvd, ssim,
    psnr, lpips in the reference's order, the two networks only with their weights, else under not_computed), or None when no folder
    qualifies.  ValueError when the folders' frame counts differ (the reference's torch.stack fails there)."""
    import torch

    from . import metrics, ops
    names = sorted(d for d in os.listdir(input_folder) if os.path.isdir(os.path.join(input_folder, d)))
    navigated, original, used = [], [], []
    for d in names:
        paths = [os.path.join(input_folder, d, f) for f in ("navigated.avi", "original.avi")]
        if not all(os.path.exists(p) for p in paths):
            continue
        clips = [ops.resize_linear_u8(read_video(p)[0], target_size, target_size) for p in paths]
        navigated.append(clips[0])
        original.append(clips[1])
        used.append(d)
    if not used:
        return None
    counts = {d: (len(a), len(b)) for d, a, b in zip(used, navigated, original)}
    if len({n for pair in counts.values() for n in pair}) != 1:
        raise ValueError(f"the videos differ in length (frames of navigated.avi, original.avi per folder): {counts}")
    to_float = lambda clips: torch.stack(clips).permute(0, 1, 4, 2, 3).float() / 255.0
    videos1, videos2 = to_float(navigated), to_float(original)
    result = {}
    if fvd_weights:
        from . import fvd
        result["fvd"] = fvd.calculate_fvd(videos1, videos2, fvd.I3D.from_files(fvd_weights, "cuda"), channel_order)
    result["ssim"] = metrics.calculate_ssim(videos1, videos2)
    result["psnr"] = metrics.calculate_psnr(videos1, videos2)
    if lpips_weights:
        from .lpips import LPIPSAlex
        result["lpips"] = metrics.calculate_lpips(videos1, videos2, LPIPSAlex.from_files(lpips_weights, "cuda"), channel_order)
    result["not_computed"] = {k: metrics.NOT_COMPUTED[k] for k in ("fvd", "lpips") if k not in result}
    result["videos"] = used
    return result


# ------------------------------------------------------------------ command line
def _cli_encode(args):
    from .frames import list_images, read_frames
    names = list_images(args.input, (".png",))
    if not names:
        raise SystemExit(f"{args.input}: no .png frames")
    frames = read_frames([os.path.join(args.input, n) for n in names], "cuda")
    size = write_video(args.output, frames, args.fps, args.quality, args.subsampling)
    print(f"{args.output}: {len(names)} frames {frames.shape[2]}x{frames.shape[1]}, {size} bytes")


def _cli_extract(args):
    from .frames import numbered_paths, write_numbered
    fps, width, height, jpegs = read_avi(args.input)
    os.makedirs(args.output, exist_ok=True)
    if args.format == "png":
        if jpegs:
            write_numbered(args.output, decode_jpeg(jpegs), on_device=args.device_png)
    else:
        for path, j in zip(numbered_paths(args.output, len(jpegs), ext=".jpg"), jpegs):
            with open(path, "wb") as f:
                f.write(j)
    print(f"{args.output}: {len(jpegs)} frames {width}x{height} at {fps:g} fps")


def _cli_scores(args):
    import json
    result = video_scores(args.input_folder, args.target_size, args.lpips_weights, args.fvd_weights, args.channel_order)
    if result is None:
        print("No valid videos found. Exiting.")
        return
    print(json.dumps(result, indent=4))
    if args.result_file:
        with open(args.result_file, "w") as f:
            json.dump(result, f, indent=4)


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(prog="python -m evoworld_amd.video", description="MJPEG AVI of a folder of NNN.png frames, and back")
    sub = p.add_subparsers(dest="command", required=True)
    e = sub.add_parser("encode", help="a folder of NNN.png (e.g. predictions_{seg}) -> X.avi, encoded on the GPU")
    e.add_argument("--input", required=True)
    e.add_argument("--output", required=True)
    e.add_argument("--fps", type=float, default=10)
    e.add_argument("--quality", type=int, default=90)
    e.add_argument("--subsampling", choices=SUBSAMPLINGS, default="4:2:0")
    e.set_defaults(run=_cli_encode)
    x = sub.add_parser("extract", help="X.avi -> NNN.jpg, the frames as they are stored, or NNN.png, decoded on the GPU")
    x.add_argument("--input", required=True)
    x.add_argument("--output", required=True)
    x.add_argument("--format", choices=("jpg", "png"), default="jpg")
    x.add_argument("--device_png", action="store_true", help="with --format png: encode the files on the GPU (evoworld_amd.png)")
    x.set_defaults(run=_cli_extract)
    s = sub.add_parser("scores", help="PSNR / SSIM (LPIPS, FVD with their weights) of navigated.avi against original.avi over the "
                                      "sub-folders of a folder, as the reference's calculate_scores.py")
    s.add_argument("--input_folder", required=True, help="the folder whose sub-folders hold navigated.avi and original.avi")
    s.add_argument("--target_size", type=int, default=64, help="every frame is resized to this square (calculate_scores.py: 64)")
    s.add_argument("--lpips_weights", type=str, nargs="+", default=None, metavar="PATH", help="as python -m evoworld_amd.metrics")
    s.add_argument("--fvd_weights", type=str, nargs="+", default=None, metavar="PATH", help="as python -m evoworld_amd.metrics")
    s.add_argument("--channel_order", choices=("bgr", "rgb"), default="rgb",
                   help="rgb (default): calculate_scores.py swaps its cv2 frames to RGB before the networks see them")
    s.add_argument("--result_file", type=str, default=None, help="also write the JSON here")
    s.add_argument("--device", type=str, default="cuda", help="parsed and ignored: there is no CPU path")
    s.set_defaults(run=_cli_scores)
    return p.parse_args(argv)


def main(argv=None):
    args = parse_arguments(argv)
    args.run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
