"""The oracle of the device PNG encoder (evoworld_amd/png.py, csrc/png.hip): numpy / pure Python, written from RFC 1951 (deflate), RFC 1950
(zlib) and RFC 2083 (PNG) with their tables typed out, sharing no code with the package.  It holds the scanline filters with libpng's
selection rule, a token replayer, the canonical code assignment, a bit-exact emitter for given tokens and tables, and the Adler-32
combine.  The LZ77 parse itself has no oracle: any parse is valid, so the tests replay the device's tokens and emit *them* here."""
import struct
import zlib

import numpy as np

ADAPTIVE = 5
NLIT, NDIST = 286, 30
# RFC 1951 3.2.5: (symbol, extra bits, first length) and (code, extra bits, first distance)
LENGTH_TABLE = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10), (265, 1, 11),
                (266, 1, 13), (267, 1, 15), (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31), (273, 3, 35),
                (274, 3, 43), (275, 3, 51), (276, 3, 59), (277, 4, 67), (278, 4, 83), (279, 4, 99), (280, 4, 115), (281, 5, 131),
                (282, 5, 163), (283, 5, 195), (284, 5, 227), (285, 0, 258)]
DIST_TABLE = [(0, 0, 1), (1, 0, 2), (2, 0, 3), (3, 0, 4), (4, 1, 5), (5, 1, 7), (6, 2, 9), (7, 2, 13), (8, 3, 17), (9, 3, 25), (10, 4, 33),
              (11, 4, 49), (12, 5, 65), (13, 5, 97), (14, 6, 129), (15, 6, 193), (16, 7, 257), (17, 7, 385), (18, 8, 513), (19, 8, 769),
              (20, 9, 1025), (21, 9, 1537), (22, 10, 2049), (23, 10, 3073), (24, 11, 4097), (25, 11, 6145), (26, 12, 8193),
              (27, 12, 12289), (28, 13, 16385), (29, 13, 24577)]


def length_symbol(length):
    """3 .. 258 -> (symbol, extra bits, extra value); 258 is symbol 285, not 284 + 31"""
    if length == 258:
        return 285, 0, 0
    for sym, nbits, first in reversed(LENGTH_TABLE[:-1]):
        if length >= first:
            return sym, nbits, length - first
    raise ValueError(length)


def dist_symbol(dist):
    for sym, nbits, first in reversed(DIST_TABLE):
        if dist >= first:
            return sym, nbits, dist - first
    raise ValueError(dist)


# ------------------------------------------------------------------ filters (RFC 2083 section 6)
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_row(f, cur, up):
    """cur, up: int arrays [3 W] (up = zeros for row 0) -> the row filtered with type f, uint8"""
    cur, up = cur.astype(np.int64), up.astype(np.int64)
    a = np.concatenate([np.zeros(3, np.int64), cur[:-3]])
    c = np.concatenate([np.zeros(3, np.int64), up[:-3]])
    pred = [np.zeros_like(cur), a, up, (a + up) // 2, _paeth(a, up, c)][f]
    return ((cur - pred) % 256).astype(np.uint8)


def filter_frame(frame, mode=ADAPTIVE):
    """uint8 [H,W,3] -> filtered uint8 [H, 1 + 3 W].  mode 0 .. 4 forces a type; ADAPTIVE takes per row the type with the smallest sum
    of (v < 128 ? v : 256 - v), the lowest type on a tie"""
    H, W, _ = frame.shape
    rows = frame.reshape(H, 3 * W)
    out = np.empty((H, 1 + 3 * W), np.uint8)
    for y in range(H):
        up = rows[y - 1] if y else np.zeros(3 * W, np.uint8)
        cands = [filter_row(f, rows[y], up) for f in range(5)]
        if mode == ADAPTIVE:
            costs = [int(np.where(c < 128, c.astype(np.int64), 256 - c.astype(np.int64)).sum()) for c in cands]
            f = costs.index(min(costs))
        else:
            f = mode
        out[y, 0], out[y, 1:] = f, cands[f]
    return out


# ------------------------------------------------------------------ tokens
def split_token(t):
    """uint32 token -> ('lit', byte) or ('match', length, distance)"""
    t = int(t) & 0xFFFFFFFF
    if t >> 31:
        return "match", (t & 0xFF) + 3, ((t >> 8) & 0x7FFF) + 1
    return "lit", t & 0xFF


def replay(tokens):
    """the bytes a token list stands for; raises on a match that reaches before the segment's first byte"""
    out = bytearray()
    for t in tokens:
        tok = split_token(t)
        if tok[0] == "lit":
            out.append(tok[1])
        else:
            _, length, dist = tok
            if dist > len(out):
                raise ValueError(f"distance {dist} at position {len(out)}")
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def histogram(tokens):
    """int64 [316]: literal/length symbols (end of block once), then distance codes"""
    h = np.zeros(NLIT + NDIST, np.int64)
    for t in tokens:
        tok = split_token(t)
        if tok[0] == "lit":
            h[tok[1]] += 1
        else:
            h[length_symbol(tok[1])[0]] += 1
            h[NLIT + dist_symbol(tok[2])[0]] += 1
    h[256] += 1
    return h


# ------------------------------------------------------------------ codes and bits
def canonical(lengths):
    """RFC 1951 3.2.2 -> {symbol: (code, length)} for the symbols with a length"""
    lengths = [int(l) for l in lengths]
    code, out = 0, {}
    for bits in range(1, max(lengths) + 1):
        for s, l in enumerate(lengths):
            if l == bits:
                out[s] = (code, bits)
                code += 1
        code <<= 1
    return out


def kraft(lengths):
    """sum of 2^-l over the coded symbols as an exact fraction (numerator, denominator)"""
    top = max(lengths)
    return sum(1 << (top - l) for l in lengths if l), 1 << top


class Bits:
    def __init__(self):
        self.b = []

    def number(self, v, n):                    # LSB first
        self.b += [(v >> i) & 1 for i in range(n)]

    def code(self, code, n):                   # MSB first
        self.b += [(code >> (n - 1 - i)) & 1 for i in range(n)]

    def align(self):
        self.b += [0] * (-len(self.b) % 8)

    def tobytes(self):
        assert len(self.b) % 8 == 0
        a = np.array(self.b, np.uint8).reshape(-1, 8)
        return bytes((a << np.arange(8)).sum(axis=1).astype(np.uint8))


def emit_segment(tokens, lit_lengths, dist_lengths, header, header_bits, last):
    """One coded segment, bit for bit: the frame's dynamic-block header (bytes + bit count, BFINAL = 0 in it), set BFINAL if last, the
    tokens, end of block; then zero padding (last) or the empty stored block 000, pad, 00 00 FF FF"""
    lit, dist = canonical(lit_lengths), canonical(dist_lengths)
    w = Bits()
    hb = [(header[i >> 3] >> (i & 7)) & 1 for i in range(header_bits)]
    if last:
        hb[0] = 1
    w.b += hb
    for t in tokens:
        tok = split_token(t)
        if tok[0] == "lit":
            w.code(*lit[tok[1]])
        else:
            sym, nbits, extra = length_symbol(tok[1])
            w.code(*lit[sym])
            w.number(extra, nbits)
            sym, nbits, extra = dist_symbol(tok[2])
            w.code(*dist[sym])
            w.number(extra, nbits)
    w.code(*lit[256])
    if not last:
        w.number(0, 3)
    w.align()
    return w.tobytes() + (b"" if last else b"\x00\x00\xff\xff")


def emit_stored(data, last):
    out = b""
    for at in range(0, len(data), 65535):
        part = data[at: at + 65535]
        final = last and at + 65535 >= len(data)
        out += bytes([1 if final else 0]) + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
    return out


# ------------------------------------------------------------------ Adler-32 and the file
def adler_halves(data):
    v = zlib.adler32(data)
    return v & 0xFFFF, v >> 16


def adler_combine(a1, b1, a2, b2, len2):
    return (a1 + a2 - 1) % 65521, (b1 + b2 + len2 * (a1 - 1)) % 65521


def chunks(data):
    """walk a PNG file -> [(type, payload)], checking the signature, every length and every CRC"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at: at + 8])
        body = data[at + 8: at + 8 + n]
        assert len(body) == n, "chunk runs past the file"
        assert struct.unpack(">I", data[at + 8 + n: at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        out.append((kind, body))
        at += 12 + n
    assert at == len(data)
    return out


def png_bytes(frame, segments):
    """a whole file from the oracle alone: `segments` = the deflate bytes of the frame's segments, in order"""
    H, W, _ = frame.shape
    raw = filter_frame(frame).tobytes()

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    idat = b"\x78\x01" + b"".join(segments) + struct.pack(">I", zlib.adler32(raw))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def simple_tokens(data):
    """a plain host parse for the oracle's own files: runs of one byte become distance-1 matches, everything else literals"""
    out, i, n = [], 0, len(data)
    while i < n:
        run = 1
        while i + run < n and data[i + run] == data[i] and run < 259:
            run += 1
        out.append(data[i])
        i += 1
        if run - 1 >= 3:
            out.append(0x80000000 | (run - 1 - 3) | (0 << 8))
            i += run - 1
    return out
