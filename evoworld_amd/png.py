"""PNG frame dumps encoded on the device (csrc/png.hip): only a frame's compressed bytes cross to the host.

The reference's --save_frames runs end in `Image.fromarray(f).save(...)` per frame on one host thread
(unified_loop_consistency.py:104-108, :432-453; reproject_vggt_open3d_utils.py's cv2.imwrite); the files are what
calculate_metrics.sh reads afterwards, so they stay PNG.  Here the filter, the LZ77 parse and the bit packing are kernels; the host
builds the Huffman tables of every frame from a [V, 316] histogram, and afterwards frames the bytes that arrived: signature, IHDR,
one IDAT (zlib header 78 01, the deflate stream, the Adler-32 combined from the segments' halves), IEND.  The pixels a decoder
returns are the input's, bit for bit; the file bytes are not Pillow's, which is why every caller opts in.

  python -m evoworld_amd.png encode --input X.avi|DIR --output DIR [--filter adaptive] [--rows_per_segment N]
      the frames of an MJPEG AVI (decoded on the device) or of a folder of images -> DIR/NNN.png
"""
import argparse
import heapq
import os
import struct
import sys
import zlib

import numpy as np

from .frames import list_images, numbered_paths, read_frames

NLIT,NDIST, NCLC = 286, 30, 19
MAX_BITS, MAX_CLC_BITS = 15, 7
END_OF_BLOCK = 256
CLC_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)        # RFC 1951 3.2.7
# extra bits of the length symbols 257 .. 285 and of the distance codes 0 .. 29 (RFC 1951 3.2.5)
LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_EXTRA = (0, 0, 0, 0) + tuple(e for e in range(1, 14) for _ in (0, 1))
ADLER_MOD = 65521
STORED_MAX = 65535
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
ZLIB_HEADER = b"\x78\x01"
TOKEN_WORKSPACE_BYTES = 256 << 20        # encode_png's bound on the token buffer of one batch


# ------------------------------------------------------------------ Huffman tables (host, no GPU)
def _huffman_depths(freqs):
    """plain Huffman code lengths of the symbols with freqs > 0 (at least two of them); ties by symbol order"""
    heap = [(int(f), i, (i,)) for i, f in enumerate(freqs) if f > 0]
    depth = [0] * len(freqs)
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ia, sa = heapq.heappop(heap)
        fb, ib, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ia, ib), sa + sb))
    return depth


def _package_merge(freqs, limit):
    """optimal code lengths <= limit (Larmore & Hirschberg's package-merge) of the symbols with freqs > 0, at least two and at most
    2^limit of them"""
    syms = sorted((int(f), i) for i, f in enumerate(freqs) if f > 0)
    n = len(syms)
    leaves_w = np.array([w for w, _ in syms], dtype=np.int64)
    leaves_c = np.eye(n, dtype=np.int32)
    w, c = leaves_w, leaves_c
    for _ in range(limit - 1):
        m = len(w) // 2
        pw, pc = w[0:2 * m:2] + w[1:2 * m:2], c[0:2 * m:2] + c[1:2 * m:2]
        w, c = np.concatenate([leaves_w, pw]), np.concatenate([leaves_c, pc])
        order = np.argsort(w, kind="stable")                                     # leaves before packages of the same weight
        w, c = w[order], c[order]
    lengths = c[: 2 * n - 2].sum(axis=0)
    out = [0] * len(freqs)
    for (_, i), l in zip(syms, lengths):
        out[i] = int(l)
    return out


def limited_code_lengths(freqs, limit, always=()):
    """Code lengths (0 = no code) of a complete prefix code, none above `limit`: every symbol with a count, every symbol of `always`,
    and -- so that the code is complete (Kraft sum exactly 1) also for a histogram with fewer than two symbols -- the lowest unused
    symbols until there are two.  Huffman's lengths where they fit, package-merge's otherwise."""
    freqs = [int(f) for f in freqs]
    if 1 << limit < len(freqs):
        raise ValueError(f"{len(freqs)} symbols cannot all have codes of at most {limit} bits")
    if min(freqs, default=0) < 0 or sum(freqs) >= 1 << 62:
        raise ValueError("counts must be non-negative and sum to less than 2^62")
    work = list(freqs)
    for s in always:
        work[s] = max(work[s], 1)
    for s in range(len(work)):
        if sum(1 for f in work if f > 0) >= 2:
            break
        if work[s] == 0:
            work[s] = 1
    lengths = _huffman_depths(work)
    if max(lengths) > limit:
        lengths = _package_merge(work, limit)
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2: codes of the given lengths, consecutive within a length in symbol order"""
    count = [0] * (max(lengths, default=0) + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * len(count)
    for bits in range(1, len(count)):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def reverse_bits(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


class BitString:
    """LSB-first bits, as deflate packs them"""

    def __init__(self):
        self.value, self.bits = 0, 0

    def put(self, v, n):                       # a number: least significant bit first
        self.value |= (v & ((1 << n) - 1)) << self.bits
        self.bits += n

    def put_code(self, code, n):               # a Huffman code: most significant bit first
        self.put(reverse_bits(code, n), n)

    def tobytes(self):
        return self.value.to_bytes((self.bits + 7) // 8, "little")


def run_length_code(lengths):
    """the code lengths of a block header as (symbol 0 .. 18, extra bits, extra value): 16 repeats the previous length 3 - 6 times,
    17 / 18 stand for 3 - 10 / 11 - 138 zeros"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, run = lengths[i], 1
        while i + run < n and lengths[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, 7, r - 11))
                run -= r
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, 2, r - 3))
                run -= r
        out += [(v, 0, 0)] * run
    return out


class FrameTables:
    """One frame's deflate tables from its histogram int [316]: the code lengths (lit / dist), the dynamic-block header with BFINAL = 0
    as an LSB-first bit string (header, header_bits), lut uint32 [316] (bit-reversed code | length << 16, what ew_png_emit reads) and
    cost int64 [316] (code length + extra bits per symbol: hist . cost + header_bits is a segment's block size in bits).  Symbol 256
    always has a code; the distance code always holds at least two codes, also for a frame without a match."""

    def __init__(self, hist):
        hist = [int(h) for h in hist]
        if len(hist) != NLIT + NDIST:
            raise ValueError(f"a histogram holds {NLIT + NDIST} counts, got {len(hist)}")
        self.lit = limited_code_lengths(hist[:NLIT], MAX_BITS, always=(END_OF_BLOCK,))
        self.dist = limited_code_lengths(hist[NLIT:], MAX_BITS)
        lit_codes, dist_codes = canonical_codes(self.lit), canonical_codes(self.dist)
        nlit = max(257, max(i for i, l in enumerate(self.lit) if l) + 1)
        ndist = max(1, max(i for i, l in enumerate(self.dist) if l) + 1)
        rle = run_length_code(self.lit[:nlit] + self.dist[:ndist])
        clc_hist = [0] * NCLC
        for s, _, _ in rle:
            clc_hist[s] += 1
        self.clc = limited_code_lengths(clc_hist, MAX_CLC_BITS)
        clc_codes = canonical_codes(self.clc)
        nclen = max(4, max(i for i, s in enumerate(CLC_ORDER) if self.clc[s]) + 1)
        b = BitString()
        b.put(0, 1)                             # BFINAL: ew_png_emit sets it on a frame's last segment
        b.put(2, 2)                             # BTYPE = 10, dynamic Huffman
        b.put(nlit - 257, 5)
        b.put(ndist - 1, 5)
        b.put(nclen - 4, 4)
        for s in CLC_ORDER[:nclen]:
            b.put(self.clc[s], 3)
        for s, nbits, extra in rle:
            b.put_code(clc_codes[s], self.clc[s])
            if nbits:
                b.put(extra, nbits)
        self.header, self.header_bits = b.tobytes(), b.bits
        lengths = self.lit + self.dist
        codes = lit_codes + dist_codes
        self.lut = np.array([reverse_bits(c, l) | (l << 16) for c, l in zip(codes, lengths)], dtype=np.uint32)
        extra = (0,) * 257 + LENGTH_EXTRA + DIST_EXTRA
        self.cost = np.array([l + e for l, e in zip(lengths, extra)], dtype=np.int64)


# ------------------------------------------------------------------ container (host)
def adler_combine(a1, b1, a2, b2, len2):
    """Adler-32 halves of a concatenation from the halves of its two parts (each started at a = 1, b = 0)"""
    return (a1 + a2 - 1) % ADLER_MOD, (b1 + b2 + len2 % ADLER_MOD * (a1 - 1 + ADLER_MOD)) % ADLER_MOD


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_file(width, height, deflate, adler):
    """The file around one frame's deflate stream: 8-bit RGB (colour type 2), no interlace, IHDR, one IDAT, IEND"""
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)
    return PNG_SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", ZLIB_HEADER + bytes(deflate) + struct.pack(">I", adler)) + chunk(b"IEND", b"")


def stored_size(n):
    return n + 5 * -(-n // STORED_MAX)


# ------------------------------------------------------------------ the device path
def frames_per_batch(H, W):
    """encode_png's batch: as many frames as keep the token workspace -- 4 bytes per filtered byte, the worst case of one token per
    byte -- at or below TOKEN_WORKSPACE_BYTES (256 MiB), at least one (a 576 x 1024 frame takes 6.75 MiB: 37 frames)."""
    return max(1, TOKEN_WORKSPACE_BYTES // (4 * H * (1 + 3 * W)))


def segment_sizes(hist, tables, V, H, W, rps):
    """Exact sizes from the histograms (torch on the device, plumbing): -> (seg_mode int32 [n], seg_bytes int64 [n], seg_offsets int64
    [n], frame_bytes int64 [V]).  A segment is coded unless its stored form is not larger."""
    import torch
    dev = hist.device
    spf = -(-H // rps)
    row = 1 + 3 * W
    cost = torch.from_numpy(np.stack([t.cost for t in tables])).to(dev)                         # [V,316]
    hbits = torch.tensor([t.header_bits for t in tables], dtype=torch.int64, device=dev)
    bits = (hist.view(V, spf, -1).to(torch.int64) * cost[:, None, :]).sum(dim=2) + hbits[:, None]
    coded = (bits + 3 + 7) // 8 + 4                                                             # + the empty stored block
    coded[:, -1] = (bits[:, -1] + 7) // 8                                                       # a frame's last segment: BFINAL, padded
    rows = torch.full((spf,), rps, dtype=torch.int64, device=dev)
    rows[-1] = H - (spf - 1) * rps
    raw = rows * row
    stored = (raw + 5 * ((raw + STORED_MAX - 1) // STORED_MAX))[None, :].expand(V, spf)
    mode = coded >= stored
    seg_bytes = torch.where(mode, stored, coded).reshape(-1).contiguous()
    ends = torch.cumsum(seg_bytes, 0)
    return mode.reshape(-1).to(torch.int32).contiguous(), seg_bytes, (ends - seg_bytes).contiguous(), seg_bytes.view(V, spf).sum(dim=1)


def upload_tables(tables, device):
    """-> (luts int32 [V,316], headers uint8 [V,n], header_bits int32 [V]) on the device"""
    import torch
    n = max(len(t.header) for t in tables)
    headers = np.zeros((len(tables), n), np.uint8)
    for i, t in enumerate(tables):
        headers[i, : len(t.header)] = np.frombuffer(t.header, np.uint8)
    luts = np.stack([t.lut for t in tables]).view(np.int32)
    hb = np.array([t.header_bits for t in tables], np.int32)
    return torch.from_numpy(luts).to(device), torch.from_numpy(headers).to(device), torch.from_numpy(hb).to(device)


def _encode_batch(frames, filter, rows_per_segment):
    import torch

    from . import ops
    V, H, W, _ = frames.shape
    rps = ops.png_rows_per_segment(H, W, rows_per_segment)
    spf = -(-H // rps)
    filtered, adler = ops.png_filter(frames, filter, rps)
    tokens, n_tokens, hist = ops.png_lz77(filtered, rps)
    tables = [FrameTables(h) for h in hist.view(V, spf, -1).sum(dim=1).cpu().numpy()]           # the one small copy: [V,316]
    luts, headers, header_bits = upload_tables(tables, frames.device)
    mode, seg_bytes, offsets, frame_bytes = segment_sizes(hist, tables, V, H, W, rps)
    frame_bytes = frame_bytes.cpu().numpy()                                                    # the sync that gives the total
    out = torch.empty(int(frame_bytes.sum()), dtype=torch.uint8, device=frames.device)
    ops.png_emit(tokens, n_tokens, filtered, mode, offsets, seg_bytes, luts, headers, header_bits, out, rps)
    stream, adler = out.cpu().numpy(), adler.cpu().numpy().astype(np.int64).reshape(V, spf, 2)
    seg_len = [min(rps, H - k * rps) * (1 + 3 * W) for k in range(spf)]
    files, at = [], 0
    for v in range(V):
        a, b = 1, 0
        for k in range(spf):
            a, b = adler_combine(a, b, int(adler[v, k, 0]), int(adler[v, k, 1]), seg_len[k])
        n = int(frame_bytes[v])
        files.append(png_file(W, H, stream[at: at + n].tobytes(), (b << 16) | a))
        at += n
    return files


def encode_png(frames_u8, filter="adaptive", rows_per_segment=None):
    """uint8 [V,H,W,3] (or one frame [H,W,3]) on the device -> list of V complete PNG files (bytes).  filter: "adaptive" (libpng's
    per-row choice) | "none" | "sub" | "up" | "average" | "paeth"; rows_per_segment: the rows of one independently deflated segment
    (default: the most that stay within 32 KiB).  The frames are encoded in batches of frames_per_batch(H, W), which bounds the token
    workspace at TOKEN_WORKSPACE_BYTES = 256 MiB (or one frame's, if that is larger); beside it a batch holds its filtered rows (a
    quarter of that) and the compressed stream.  Two host synchronisations per batch: the histograms, then the sizes."""
    if frames_u8.ndim == 3:
        frames_u8 = frames_u8[None]
    if frames_u8.ndim != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"frames_u8 must be [V,H,W,3], got {tuple(frames_u8.shape)}")
    frames_u8 = frames_u8.contiguous()
    step = frames_per_batch(frames_u8.shape[1], frames_u8.shape[2])
    files = []
    for i in range(0, frames_u8.shape[0], step):
        files += _encode_batch(frames_u8[i: i + step], filter, rows_per_segment)
    return files


def write_png(path, frame):
    """one frame uint8 [H,W,3] on the device -> the file `path`; returns its size"""
    if frame.ndim != 3:
        raise ValueError(f"frame must be [H,W,3], got {tuple(frame.shape)}")
    data = encode_png(frame)[0]
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def write_png_files(paths, frames_u8, filter="adaptive", rows_per_segment=None):
    """frames uint8 [V,H,W,3] on the device -> one file per path; returns the bytes written"""
    paths = list(paths)
    if len(paths) != frames_u8.shape[0]:
        raise ValueError(f"{len(paths)} paths for {frames_u8.shape[0]} frames")
    total = 0
    for p, data in zip(paths, encode_png(frames_u8, filter, rows_per_segment) if paths else ()):
        with open(p, "wb") as f:
            f.write(data)
        total += len(data)
    return total


def write_png_frames(dir, frames, start=0, digits=3):
    """uint8 [F,H,W,3] on the device -> dir/NNN.png, 1-based and offset by `start` (frames.numbered_paths, the names of every frame dump);
    `digits` is the least width of the number.  Returns the paths."""
    os.makedirs(dir, exist_ok=True)
    paths = numbered_paths(dir, frames.shape[0], start, digits=digits)
    write_png_files(paths, frames)
    return paths


# ------------------------------------------------------------------ command line
def _cli_encode(args):
    if os.path.isdir(args.input):
        names = list_images(args.input, (".png", ".jpg", ".jpeg"))
        if not names:
            raise SystemExit(f"{args.input}: no image files")
        frames = read_frames([os.path.join(args.input, n) for n in names], "cuda")
    else:
        from .video import read_video
        frames = read_video(args.input)[0]
    os.makedirs(args.output, exist_ok=True)
    paths = numbered_paths(args.output, frames.shape[0])
    size = write_png_files(paths, frames, args.filter, args.rows_per_segment)
    print(f"{args.output}: {len(paths)} frames {frames.shape[2]}x{frames.shape[1]}, {size} bytes")


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(prog="python -m evoworld_amd.png", description="PNG files encoded on the GPU")
    sub = p.add_subparsers(dest="command", required=True)
    e = sub.add_parser("encode", help="the frames of X.avi (MJPEG) or of a folder of images -> DIR/NNN.png")
    e.add_argument("--input", required=True)
    e.add_argument("--output", required=True)
    e.add_argument("--filter", choices=("adaptive", "none", "sub", "up", "average", "paeth"), default="adaptive")
    e.add_argument("--rows_per_segment", type=int, default=None)
    e.set_defaults(run=_cli_encode)
    return p.parse_args(argv)


def main(argv=None):
    args = parse_arguments(argv)
    args.run(args)


if __name__ == "__main__":
    main(sys.argv[1:])
