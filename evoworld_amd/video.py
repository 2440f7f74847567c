"""Video files of generated clips: Motion-JPEG in AVI, the frames encoded on the device (csrc/video.hip).

The reference writes its clips through imageio / ffmpeg (Navigator.save_video, evoworld/inference/navigator_evoworld.py:233-257) and
its calculate_scores.py loads navigated.mp4 / original.mp4 per episode.  No H.264 encoder (ffmpeg, imageio, PyAV, cv2) exists here, so
the container is written by hand, as the GLB was: every frame is a stand-alone baseline JPEG whose scan data come from the GPU
(ops.jpeg_dct_quant -> ops.jpeg_entropy -> ops.jpeg_pack; only the compressed stream crosses to the host), wrapped in a RIFF `AVI `
file with one MJPG video stream and an idx1 index.  ffplay, VLC and cv2.VideoCapture read that layout; none of them is available to
test against (unpinned), so the tests check the container field by field and the frames through libjpeg (Pillow).

  quant_tables / jpeg_header / encode_jpeg     the frames
  write_avi / read_avi / write_video           the container
  python -m evoworld_amd.video encode --input DIR --output X.avi [--fps 10 --quality 90 --subsampling 4:2:0]
  python -m evoworld_amd.video extract --input X.avi --output DIR
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


# ------------------------------------------------------------------ command line
def _cli_encode(args):
    import torch
    from PIL import Image
    names = sorted(n for n in os.listdir(args.input) if n.lower().endswith(".png"))
    if not names:
        raise SystemExit(f"{args.input}: no .png frames")
    arr = np.stack([np.asarray(Image.open(os.path.join(args.input, n)).convert("RGB")) for n in names])
    size = write_video(args.output, torch.from_numpy(arr).cuda(), args.fps, args.quality, args.subsampling)
    print(f"{args.output}: {len(names)} frames {arr.shape[2]}x{arr.shape[1]}, {size} bytes")


def _cli_extract(args):
    fps, width, height, frames = read_avi(args.input)
    os.makedirs(args.output, exist_ok=True)
    for i, j in enumerate(frames):
        with open(os.path.join(args.output, f"{i + 1:03}.jpg"), "wb") as f:
            f.write(j)
    print(f"{args.output}: {len(frames)} frames {width}x{height} at {fps:g} fps")


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
    x = sub.add_parser("extract", help="X.avi -> NNN.jpg, the frames as they are stored")
    x.add_argument("--input", required=True)
    x.add_argument("--output", required=True)
    x.set_defaults(run=_cli_extract)
    return p.parse_args(argv)


def main(argv=None):
    args = parse_arguments(argv)
    args.run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
