"""The oracle of the MJPEG tests (tests/test_cpu_video.py, tests/test_gpu_video.py): the stream format of DESIGN.md 4.5 restated in numpy
float64, a plain-Python Huffman packer over given coefficients, and the header writer.  Not imported by the package.

The Huffman tables are not typed in here: they are read back from the DHT segments of a file libjpeg wrote through Pillow (its
standard Annex K tables), so that the package's own copy is checked against a second source.  The base quantisation tables are Annex
K.1 / K.2 as printed in T.81; tests/test_cpu_video.py checks the package's scaled tables against libjpeg's through Pillow."""
import io

import numpy as np

MCU = {"4:2:0": 16, "4:4:4": 8}
BPM = {"4:2:0": 6, "4:4:4": 3}
TIE_WINDOW = 1e-3          # a device coefficient may differ (by exactly 1) only where the quotient is this close to k + 1/2


def zigzag():
    """zigzag position -> natural index, walked along the anti-diagonals (T.81 figure A.6)"""
    out = []
    for s in range(15):
        diag = [(i, s - i) for i in range(8) if 0 <= s - i < 8]
        out += diag if s % 2 else diag[::-1]
    return np.array([r * 8 + c for r, c in out])


ZIGZAG = zigzag()

K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
               103, 99])
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66] + [99] * 38)


def quant_tables_ref(quality):
    """(luma, chroma) int arrays [64] in natural order: libjpeg's quality rule"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (K1, K2))


def _segments(jpeg):
    """(marker, payload) of every segment up to and including SOS"""
    i = 2
    while i < len(jpeg):
        assert jpeg[i] == 0xFF
        m, n = jpeg[i + 1], int.from_bytes(jpeg[i + 2: i + 4], "big")
        yield m, jpeg[i + 4: i + 2 + n]
        if m == 0xDA:
            return
        i += 2 + n


def dht_tables(jpeg):
    """{(class, id): (bits [16], values)} of a JPEG's DHT segments"""
    out = {}
    for m, p in _segments(jpeg):
        if m != 0xC4:
            continue
        while p:
            bits = list(p[1:17])
            n = sum(bits)
            out[(p[0] >> 4, p[0] & 15)] = (bits, list(p[17: 17 + n]))
            p = p[17 + n:]
    return out


_std = None


def std_huffman():
    """libjpeg's standard tables {(class, id): (bits, values)}: class 0 DC / 1 AC, id 0 luminance / 1 chrominance"""
    global _std
    if _std is None:
        from PIL import Image
        b = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(b, "JPEG", quality=75, optimize=False)
        _std = dht_tables(b.getvalue())
        assert sorted(_std) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    return _std


def huff_codes(bits, values):
    """{symbol: (code, length)} (T.81 annex C)"""
    out, code, at = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[values[at]] = (code, length)
            at += 1
            code += 1
        code <<= 1
    return out


# ------------------------------------------------------------------ coefficients (float64)
def dct_matrix():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    d = 0.5 * np.cos((2 * n + 1) * k * np.pi / 16)
    d[0] = np.sqrt(1 / 8)
    return d


def _blocks(plane):
    """[Hp, Wp] -> [Hp/8, Wp/8, 8, 8]"""
    hp, wp = plane.shape
    return plane.reshape(hp // 8, 8, wp // 8, 8).transpose(0, 2, 1, 3)


def quotients_ref(frame, quality, subsampling):
    """frame uint8 [H,W,3] -> float64 [mcu_rows, mcu_cols, blocks_per_mcu, 64]: c / t of every coefficient in scan and zigzag order"""
    mcu = MCU[subsampling]
    h, w, _ = frame.shape
    mr, mc = -(-h // mcu), -(-w // mcu)
    f = np.pad(frame, ((0, mr * mcu - h), (0, mc * mcu - w), (0, 0)), mode="edge").astype(np.float64)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b - 128.0
    cb = -0.168735892 * r - 0.331264108 * g + 0.5 * b
    cr = 0.5 * r - 0.418687589 * g - 0.081312411 * b
    if subsampling == "4:2:0":
        cb, cr = (p.reshape(mr * 8, 2, mc * 8, 2).mean(axis=(1, 3)) for p in (cb, cr))
    d = dct_matrix()
    ql, qc = (t.astype(np.float64).reshape(8, 8) for t in quant_tables_ref(quality))

    def coded(plane, table):
        blk = _blocks(plane)
        c = d @ (blk @ d.T)                     # rows, then columns
        return (c / table).reshape(*blk.shape[:2], 64)[..., ZIGZAG]

    yq, bq, rq = coded(y, ql), coded(cb, qc), coded(cr, qc)
    if subsampling == "4:2:0":
        yq = yq.reshape(mr, 2, mc, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mr, mc, 4, 64)
        return np.concatenate([yq, bq[:, :, None], rq[:, :, None]], axis=2)
    return np.stack([yq, bq, rq], axis=2)


def quantise_ref(q):
    """round half to even, AC clamped to +-1023, DC to [-1024, 1023]"""
    c = np.rint(q)
    c[..., 1:] = np.clip(c[..., 1:], -1023, 1023)
    c[..., 0] = np.clip(c[..., 0], -1024, 1023)
    return c.astype(np.int16)


def near_ties(q):
    """bool mask: the quotient lies within TIE_WINDOW of a half-integer"""
    return np.abs(np.abs(q - np.floor(q)) - 0.5) <= TIE_WINDOW


# ------------------------------------------------------------------ entropy coding (plain Python)
class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, val, length):
        self.acc = (self.acc << length) | val
        self.n += length

    def stuffed(self):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        return self.acc.to_bytes(self.n // 8, "big").replace(b"\xff", b"\xff\x00")


def _size_bits(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def pack_segment(blocks, subsampling, stats=None):
    """blocks int [mcu_cols, blocks_per_mcu, 64] of one MCU row -> its entropy-coded bytes (stuffed, padded with 1-bits)"""
    std = std_huffman()
    dc = [huff_codes(*std[(0, 0)]), huff_codes(*std[(0, 1)])]
    ac = [huff_codes(*std[(1, 0)]), huff_codes(*std[(1, 1)])]
    ncomp_y = BPM[subsampling] - 2
    pred = [0, 0, 0]
    out = _Bits()
    for mcu in blocks:
        for j, blk in enumerate(mcu):
            comp = 0 if j < ncomp_y else j - ncomp_y + 1
            tab = 0 if comp == 0 else 1
            diff = int(blk[0]) - pred[comp]
            pred[comp] = int(blk[0])
            size, extra = _size_bits(diff)
            out.put(*dc[tab][size])
            out.put(extra, size)
            run = 0
            for k in range(1, 64):
                v = int(blk[k])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    out.put(*ac[tab][0xF0])
                    run -= 16
                    if stats is not None:
                        stats["zrl"] = stats.get("zrl", 0) + 1
                size, extra = _size_bits(v)
                out.put(*ac[tab][(run << 4) | size])
                out.put(extra, size)
                run = 0
            if run:
                out.put(*ac[tab][0x00])
    return out.stuffed()


def pack_scan(coef, subsampling, stats=None):
    """coef int [mcu_rows, mcu_cols, blocks_per_mcu, 64] -> the scan's bytes: one restart segment per MCU row, RSTm between them"""
    parts = []
    for row, blocks in enumerate(coef):
        seg = pack_segment(blocks, subsampling, stats)
        if stats is not None and b"\xff\x00" in seg:
            stats["stuffed"] = stats.get("stuffed", 0) + seg.count(b"\xff\x00")
        parts.append(seg)
        if row != len(coef) - 1:
            parts.append(bytes([0xFF, 0xD0 + row % 8]))
    return b"".join(parts)


# ------------------------------------------------------------------ headers
def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def headers(width, height, quality, subsampling):
    """SOI APP0 DQT DQT SOF0 DHT x4 DRI SOS"""
    ql, qc = quant_tables_ref(quality)
    std = std_huffman()
    mc = -(-width // MCU[subsampling])
    samp = 0x22 if subsampling == "4:2:0" else 0x11
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _seg(0xDB, b"\x00" + bytes(int(v) for v in ql[ZIGZAG])) + _seg(0xDB, b"\x01" + bytes(int(v) for v in qc[ZIGZAG]))
    out += _seg(0xC0, b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03" + bytes([1, samp, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for key in [(0, 0), (1, 0), (0, 1), (1, 1)]:
        bits, vals = std[key]
        out += _seg(0xC4, bytes([key[0] << 4 | key[1]]) + bytes(bits) + bytes(vals))
    out += _seg(0xDD, mc.to_bytes(2, "big"))
    return out + _seg(0xDA, b"\x03" + bytes([1, 0x00, 2, 0x11, 3, 0x11]) + b"\x00\x3f\x00")


def frame_bytes(coef, width, height, quality, subsampling, stats=None):
    """the stand-alone .jpg of one frame's coefficients"""
    return headers(width, height, quality, subsampling) + pack_scan(coef, subsampling, stats) + b"\xff\xd9"


def encode_ref(frame, quality=90, subsampling="4:2:0"):
    h, w, _ = frame.shape
    return frame_bytes(quantise_ref(quotients_ref(frame, quality, subsampling)), w, h, quality, subsampling)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 100.0 if mse < 1e-10 else 10 * np.log10(255.0 ** 2 / mse)
