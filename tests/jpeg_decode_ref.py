"""The oracle of the MJPEG decoder tests (tests/test_cpu_video_decode.py, tests/test_gpu_video_decode.py): a table-driven Huffman decoder
for any baseline three-component file in plain Python, and the decoder's three pixel stages and the bilinear resize
restated in numpy float64.  Not imported by the package, and it imports nothing of it: the headers are walked here a second time.

Segment status values are those of include/evoworld_hip.h (EW_JPEG_SEG_*), typed in again.  Where a stream is damaged the first
thing met wins, under the same reading rule as the kernel's: the bits behind a segment's end read as zeros while a code is matched,
and a code or value that needs more bits than are left is EXHAUSTED."""
import numpy as np

import jpeg_ref as J

OK, BAD_CODE, INDEX, SIZE, EXHAUSTED, LEFTOVER, MARKER = range(7)
TIE_WINDOW = J.TIE_WINDOW
U = 2.0 ** -24             # float32 unit roundoff


# ------------------------------------------------------------------ headers
def parse(jpeg):
    """-> dict(width, height, subsampling, qt [2][64] natural order (luminance, chrominance), huff {(class, id)}, sel [(dc, ac)] per
    component, dri, scan (the entropy-coded bytes, RSTm included, EOI excluded))"""
    out = {"qt": {}, "dri": 0}
    i = 2
    while True:
        assert jpeg[i] == 0xFF
        m, n = jpeg[i + 1], int.from_bytes(jpeg[i + 2: i + 4], "big")
        p = jpeg[i + 4: i + 2 + n]
        i += 2 + n
        if m == 0xDB:
            while p:
                assert p[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[J.ZIGZAG] = list(p[1:65])
                out["qt"][p[0] & 15], p = t, p[65:]
        elif m == 0xC0:
            assert p[0] == 8 and p[5] == 3
            out["height"], out["width"] = int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big")
            comps = [(p[6 + 3 * c], p[7 + 3 * c], p[8 + 3 * c]) for c in range(3)]
            out["subsampling"] = {(0x22, 0x11, 0x11): "4:2:0", (0x11, 0x11, 0x11): "4:4:4"}[tuple(c[1] for c in comps)]
            tq = [c[2] for c in comps]
        elif m == 0xDD:
            out["dri"] = int.from_bytes(p, "big")
        elif m == 0xDA:
            assert p[0] == 3
            out["sel"] = [(p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15) for c in range(3)]
            break
    out["huff"] = J.dht_tables(jpeg)
    assert tq[1] == tq[2]
    out["qt"] = np.stack([out["qt"][tq[0]], out["qt"][tq[1]]])
    end = i
    while not (jpeg[end] == 0xFF and jpeg[end + 1] not in (0, 0xFF) and not 0xD0 <= jpeg[end + 1] <= 0xD7):
        end += 1
    out["scan"], out["scan_offset"] = jpeg[i:end], i
    return out


def split_segments(scan):
    """the scan's restart segments without their RSTm markers (one when there is none)"""
    segs, at, i = [], 0, 0
    while i + 1 < len(scan):
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            segs.append(scan[at:i])
            at = i = i + 2
        else:
            i += 1
    return segs + [scan[at:]]


# ------------------------------------------------------------------ Huffman decoding (plain Python)
def _code_book(bits, values):
    """{(length, code): symbol} (T.81 annex C)"""
    return {(length, code): sym for sym, (code, length) in J.huff_codes(bits, values).items()}


class _Reader:
    def __init__(self, seg):
        self.marker = False
        data = bytearray()
        i = 0
        while i < len(seg):
            data.append(seg[i])
            if seg[i] == 0xFF:
                if i + 1 < len(seg) and seg[i + 1] == 0:
                    i += 1                                 # the stuffed 00
                else:
                    data.pop()
                    self.marker = True
                    break
            i += 1
        self.bits = "".join(f"{b:08b}" for b in data)
        self.at = 0

    def left(self):
        return len(self.bits) - self.at

    def short(self):
        return MARKER if self.marker else EXHAUSTED

    def symbol(self, book):
        """-> (symbol, None) or (None, status)"""
        code = 0
        for length in range(1, 17):
            bit = int(self.bits[self.at + length - 1]) if self.at + length <= len(self.bits) else 0
            code = code << 1 | bit
            if (length, code) in book:
                if length > self.left():
                    return None, self.short()
                self.at += length
                return book[(length, code)], None
        return None, BAD_CODE

    def value(self, size):
        if size > self.left():
            return None, self.short()
        v = int(self.bits[self.at: self.at + size], 2)
        self.at += size
        return (v - (1 << size) + 1 if v < 1 << (size - 1) else v), None


def decode_segment(seg, n_mcu, bpm, books):
    """seg: one restart segment's bytes; books: [(dc book, ac book)] per component -> (int16 [n_mcu, bpm, 64], status)"""
    out = np.zeros((n_mcu, bpm, 64), np.int16)
    rd = _Reader(seg)
    pred = [0, 0, 0]
    n_y = bpm - 2
    for m in range(n_mcu):
        for j in range(bpm):
            comp = 0 if j < n_y else j - n_y + 1
            dc, ac = books[comp]
            size, err = rd.symbol(dc)
            if err:
                return out, err
            if size > 11:
                return out, SIZE
            diff = 0
            if size:
                diff, err = rd.value(size)
                if err:
                    return out, err
            pred[comp] += diff
            out[m, j, 0] = pred[comp]
            k = 1
            while k < 64:
                rs, err = rd.symbol(ac)
                if err:
                    return out, err
                run, size = rs >> 4, rs & 15
                if size == 0:
                    if run == 0:
                        break
                    if run != 15:
                        return out, BAD_CODE
                    k += 16
                    if k > 63:
                        return out, INDEX
                    continue
                if size > 10:
                    return out, SIZE
                k += run
                if k > 63:
                    return out, INDEX
                v, err = rd.value(size)
                if err:
                    return out, err
                out[m, j, k] = v
                k += 1
    if rd.marker:
        return out, MARKER
    return out, (LEFTOVER if rd.left() > 7 else OK)


def huffman_decode_ref(jpeg, segments=None):
    """One frame -> (coef int16 [mcu_rows, mcu_cols, blocks_per_mcu, 64], [status per restart segment]); `segments` replaces the
    scan's own split (damaged streams)."""
    h = parse(jpeg)
    mcu, bpm = J.MCU[h["subsampling"]], J.BPM[h["subsampling"]]
    mr, mc = -(-h["height"] // mcu), -(-h["width"] // mcu)
    mcus = mr * mc
    interval = h["dri"] if 0 < h["dri"] < mcus else mcus
    segs = split_segments(h["scan"]) if segments is None else segments
    assert len(segs) == -(-mcus // interval), (len(segs), mcus, interval)
    books = [(_code_book(*h["huff"][(0, d)]), _code_book(*h["huff"][(1, a)])) for d, a in h["sel"]]
    coef, status = np.zeros((mcus, bpm, 64), np.int16), []
    for s, seg in enumerate(segs):
        n = min(interval, mcus - s * interval)
        coef[s * interval: s * interval + n], st = decode_segment(seg, n, bpm, books)
        status.append(st)
    return coef.reshape(mr, mc, bpm, 64), status


# ------------------------------------------------------------------ pixel stages (float64)
def _unblock(b):
    """[rows, cols, 8, 8] -> [rows * 8, cols * 8]"""
    r, c = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(r * 8, c * 8)


def planes_ref(coef, qt, subsampling):
    """coef int [mcu_rows, mcu_cols, bpm, 64] (zigzag), qt [2][64] natural -> ((y, cb, cr) float64, unrounded: dequantised, inverse
    DCT, + 128; (by, bb, br): the float32 error bound of each value, idct_error_bound)"""
    mr, mc, bpm, _ = coef.shape
    d = J.dct_matrix()
    nat = np.zeros(coef.shape, np.float64)
    nat[..., J.ZIGZAG] = coef
    vals, bounds = [], []
    n_y = bpm - 2
    for j in range(bpm):
        x = (nat[:, :, j] * qt[1 if j >= n_y else 0]).reshape(mr, mc, 8, 8)
        vals.append(d.T @ x @ d + 128.0)
        bounds.append(19 * U * (np.abs(d).T @ np.abs(x) @ np.abs(d)) + 512 * U)
    out = []
    for src in (vals, bounds):
        if subsampling == "4:2:0":
            y = np.stack(src[:4], axis=2).reshape(mr, mc, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mr * 16, mc * 16)
        else:
            y = _unblock(src[0])
        out.append((y, _unblock(src[n_y]), _unblock(src[n_y + 1])))
    return out[0], out[1]


def to_u8(x):
    """round half to even, clamp: T.81's 8-bit sample"""
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def _upsample(p):
    """centred triangle filter by 2 on both axes, taps clamped to the plane: out[2i] = 3/4 p[i] + 1/4 p[i-1], out[2i+1] = 3/4 p[i] + 1/4 p[i+1]"""
    p = p.astype(np.float64)
    for axis in (0, 1):
        n = p.shape[axis]
        idx = np.arange(n)
        prev, nxt = np.take(p, np.maximum(idx - 1, 0), axis), np.take(p, np.minimum(idx + 1, n - 1), axis)
        even, odd = 0.75 * p + 0.25 * prev, 0.75 * p + 0.25 * nxt
        p = np.stack([even, odd], axis=axis + 1).reshape([2 * n if a == axis else s for a, s in enumerate(p.shape)])
    return p


def rgb_ref(planes_u8, H, W, subsampling):
    """(y, cb, cr) uint8 of the padded size -> float64 [H,W,3], unrounded"""
    y, cb, cr = planes_u8
    if subsampling == "4:2:0":
        cb, cr = _upsample(cb), _upsample(cr)
    y, cb, cr = (p[:H, :W].astype(np.float64) for p in (y, cb, cr))
    cb, cr = cb - 128.0, cr - 128.0
    return np.stack([y + 1.402 * cr, y - 0.344136286 * cb - 0.714136286 * cr, y + 1.772 * cb], axis=-1)


def resize_ref(img, h, w):
    """uint8 [H,W,3] -> float64 [h,w,3], unrounded: bilinear at half-pixel centres, neighbours clamped"""
    H, W, _ = img.shape
    f = img.astype(np.float64)

    def taps(n_dst, n_src):
        s = (np.arange(n_dst) + 0.5) * n_src / n_dst - 0.5
        i0 = np.floor(s)
        return np.clip(i0, 0, n_src - 1).astype(int), np.clip(i0 + 1, 0, n_src - 1).astype(int), s - i0

    y0, y1, fy = taps(h, H)
    x0, x1, fx = taps(w, W)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = (1 - fx) * f[y0][:, x0] + fx * f[y0][:, x1]
    bot = (1 - fx) * f[y1][:, x0] + fx * f[y1][:, x1]
    return (1 - fy) * top + fy * bot


def decode_ref(jpeg):
    """one frame -> uint8 [H,W,3] through the two-stage definition (8-bit sample planes, then RGB)"""
    h = parse(jpeg)
    coef, status = huffman_decode_ref(jpeg)
    assert not any(status), status
    (y, cb, cr), _ = planes_ref(coef, h["qt"], h["subsampling"])
    return to_u8(rgb_ref((to_u8(y), to_u8(cb), to_u8(cr)), h["height"], h["width"], h["subsampling"]))


# ------------------------------------------------------------------ streams of another encoder (libjpeg through Pillow)
FOREIGN_CASES = ("noise_40x72", "ramp_152x40", "noise_16x700")
FOREIGN_VARIANTS = {                      # Image.save options; "default" takes Pillow's own sampling (4:2:0)
    "default": {},
    "optimize": {"optimize": True},                       # Huffman tables fitted to the image
    "restart_rows": {"restart_marker_rows": 1},
    "restart_blocks": {"restart_marker_blocks": 3},       # an interval that does not divide the MCU row
    "plain_q30": {"quality": 30},
    "plain_q100": {"quality": 100},
}
FOREIGN = [(n, "default", "4:2:0") for n in FOREIGN_CASES] + [(n, v, s) for n in FOREIGN_CASES for v in FOREIGN_VARIANTS if v != "default"
                                                             for s in ("4:2:0", "4:4:4")]


def pillow_unsupported():
    """None, or why this Pillow cannot write the foreign streams (restart intervals through Image.save need Pillow >= 10.2)"""
    import io

    from PIL import Image, features
    if not features.check("jpg"):
        return "Pillow without JPEG support"
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 64, 3), np.uint8)).save(b, "JPEG", restart_marker_blocks=3)
    dri = [p for m, p in J._segments(b.getvalue()) if m == 0xDD]
    if not dri or int.from_bytes(dri[0], "big") != 3:
        return "Pillow's Image.save ignores restart_marker_blocks"
    return None


def foreign_stream(name, variant, subsampling):
    """frame 0 of a case of video_cases through Pillow's encoder"""
    import io

    import video_cases as C
    from PIL import Image
    kw = dict(FOREIGN_VARIANTS[variant])
    if variant != "default":
        kw["subsampling"] = {"4:2:0": 2, "4:4:4": 0}[subsampling]
    b = io.BytesIO()
    Image.fromarray(C.CASES[name][0][0]).save(b, "JPEG", **kw)
    return b.getvalue()


# ------------------------------------------------------------------ the tie rule
def near_half(x, window=TIE_WINDOW):
    """bool mask: x lies within `window` (scalar or array) of a half-integer"""
    return np.abs(np.abs(x - np.floor(x)) - 0.5) <= window


def check_ties(label, got, unrounded, window=TIE_WINDOW, cap=0.01, exact_halves=False):
    """got uint8 against the oracle's unrounded float64 values: a difference is exactly 1 and sits where the unrounded value is within
    `window` of a half-integer; such places are at most `cap` of `got` (None: the caller pools the returned (near ties, values) of a
    case's frames and planes and applies the cap to the case, check_cap).  exact_halves: the stage's arithmetic is exact in float32
    and float64 wherever the value is exactly k + 1/2 (dyadic weights on bytes), so those round half to even on both sides and are no
    ties.  Prints the figures, then asserts."""
    want = to_u8(unrounded)
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape, got.dtype)
    ties = near_half(unrounded, window)
    if exact_halves:
        ties &= unrounded * 2 != np.rint(unrounded * 2)
    diff = got.astype(np.int32) - want.astype(np.int32)
    wrong = diff != 0
    print(f"{label}: {int(wrong.sum())} of {wrong.size} values differ, {int(ties.sum())} near ties ({100 * ties.mean():.3f} %)")
    assert np.abs(diff).max() <= 1, f"{label}: a value is off by {np.abs(diff).max()}"
    assert not (wrong & ~ties).any(), f"{label}: {int((wrong & ~ties).sum())} values differ away from a tie"
    if cap is not None:
        assert ties.mean() <= cap, f"{label}: {100 * ties.mean():.2f} % of the values lie in the tie window"
    return int(ties.sum()), ties.size


def check_cap(label, counts, cap=0.01):
    """counts: (near ties, values) of every part of one case (check_ties with cap=None): together at most `cap` of the case"""
    n, total = (sum(c[i] for c in counts) for i in (0, 1))
    print(f"{label}: {n} of {total} values near a tie ({100 * n / total:.3f} %)")
    assert n <= cap * total, f"{label}: {100 * n / total:.2f} % of the case's values lie in the tie window"
