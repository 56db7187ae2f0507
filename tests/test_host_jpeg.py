"""The JPEG writer's statement on the host (rtc_jpeg_format and friends, include/rtc.h): the file's segments read by this
test's own marker parser, its entropy-coded data read back by this test's own baseline Huffman decoder, the quantisation
tables and quantiser restated independently, the DCT pinned to libjpeg's ISLOW through PIL where PIL is installed."""
import io
from pathlib import Path

import numpy as np
import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"

STD_Q = [
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66] + [99] * 38,
]
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


# ---- this test's own reader ------------------------------------------------------------------------------------------

def parse_jpeg(b: bytes) -> dict:
    """Segments in order with their fields; the entropy-coded data between SOS and EOI."""
    assert b[:2] == b"\xff\xd8", "SOI"
    i, segs, out = 2, [], {"dqt": {}, "dht": {}}
    while True:
        assert b[i] == 0xFF, f"marker expected at {i}"
        m = b[i + 1]
        n = int.from_bytes(b[i + 2:i + 4], "big")
        body = b[i + 4:i + 2 + n]
        segs.append(m)
        if m == 0xE0:
            out["app0"] = body
        elif m == 0xDB:
            assert len(body) == 65 and body[0] >> 4 == 0
            out["dqt"][body[0] & 15] = list(body[1:])
        elif m == 0xC0:
            out["sof"] = body
        elif m == 0xC4:
            bits = list(body[1:17])
            vals = list(body[17:17 + sum(bits)])
            assert len(body) == 17 + sum(bits)
            out["dht"][(body[0] >> 4, body[0] & 15)] = (bits, vals)
        elif m == 0xDA:
            out["sos"] = body
            j = i + 2 + n
            assert b[-2:] == b"\xff\xd9", "EOI"
            out["data"] = b[j:-2]
            break
        else:
            pytest.fail(f"unexpected marker {m:#x}")
        i += 2 + n
    out["segments"] = segs
    return out


def huff_lookup(bits, vals):
    code, k, table = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


class BitReader:
    def __init__(self, data: bytes):
        out, i = bytearray(), 0
        while i < len(data):
            out.append(data[i])
            if data[i] == 0xFF:
                assert i + 1 < len(data) and data[i + 1] == 0, f"unstuffed 0xFF at {i}"
                i += 1
            i += 1
        self.bytes, self.pos = bytes(out), 0

    def bit(self):
        v = (self.bytes[self.pos >> 3] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return v

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise AssertionError("no Huffman code matches")


def extend(v, n):
    return v - (1 << n) + 1 if n and v < (1 << (n - 1)) else v


def decode_coefficients(b: bytes) -> np.ndarray:
    """Baseline, 3 components at 1x1, no restarts: (MCUs, 3, 64) int16, natural order. Checks the padding too."""
    j = parse_jpeg(b)
    sof = j["sof"]
    h, w = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big")
    dc = [huff_lookup(*j["dht"][(0, t)]) for t in (0, 1)]
    ac = [huff_lookup(*j["dht"][(1, t)]) for t in (0, 1)]
    r = BitReader(j["data"])
    n = ((w + 7) // 8) * ((h + 7) // 8)
    out = np.zeros((n, 3, 64), dtype=np.int16)
    pred = [0, 0, 0]
    for m in range(n):
        for c in range(3):
            t = 1 if c else 0
            s = r.symbol(dc[t])
            pred[c] += extend(r.bits(s), s)
            out[m, c, 0] = pred[c]
            k = 1
            while k < 64:
                rs = r.symbol(ac[t])
                run, size = rs >> 4, rs & 15
                if size == 0:
                    if run == 15:
                        k += 16
                        continue
                    assert run == 0, "EOB expected"
                    break
                k += run
                out[m, c, ZIGZAG[k]] = extend(r.bits(size), size)
                k += 1
            assert k <= 64
    rest = len(r.bytes) * 8 - r.pos
    assert rest < 8 and r.bits(rest) == (1 << rest) - 1, "padding must be 1-bits within the last byte"
    return out


# ---- references restated here ----------------------------------------------------------------------------------------

def quant_tables(q):
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([[min(max((v * s + 50) // 100, 1), 255) for v in t] for t in STD_Q], dtype=np.uint16)


def round_half_away(x):
    return np.where(x < 0, -np.floor(-x + 0.5), np.floor(x + 0.5)).astype(np.int64)


def golden_canvases(rtc):
    out = []
    for p in sorted(GOLDEN.glob("*.npy")):
        a = np.load(p)
        if a.ndim == 3 and a.shape[2] == 3 and a.dtype == np.float64:
            out.append((p.stem, rtc.color_scale255(a.reshape(-1, 3)).reshape(a.shape)))
    return out[:4]


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))


# ---- tests -----------------------------------------------------------------------------------------------------------

def test_segments_and_header_fields(rtc):
    rng = np.random.default_rng(0)
    for (h, w), q in (((17, 33), 75), ((1, 65535), 10), ((300, 2), 100)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b = rtc.jpeg_encode(img, q)
        j = parse_jpeg(b)
        assert j["segments"] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
        assert j["app0"] == b"JFIF\x00\x01\x02\x00\x00\x01\x00\x01\x00\x00"
        assert j["sof"] == bytes([8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
        assert list(j["dht"]) == [(0, 0), (1, 0), (0, 1), (1, 1)]
        assert j["sos"] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
        qt = quant_tables(q)
        for t in (0, 1):
            assert j["dqt"][t] == [int(qt[t][ZIGZAG[k]]) for k in range(64)]
        assert b.find(b"\xff\xdd") < 0 and all(b.find(bytes([0xFF, 0xD0 + k]), 623) < 0 for k in range(8)), "no restarts"
        assert b.index(b"\xff\xda") + 14 == 623, "623 header bytes"


def test_annex_k_huffman_tables(rtc):
    j = parse_jpeg(rtc.jpeg_encode(np.zeros((8, 8, 3), dtype=np.uint8)))
    assert j["dht"][(0, 0)] == ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
    assert j["dht"][(0, 1)] == ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
    for t in (0, 1):
        bits, vals = j["dht"][(1, t)]
        assert sum(bits) == 162 and sorted(vals) == sorted([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)])


def test_quant_tables_restated(rtc):
    for q in range(1, 101):
        assert np.array_equal(rtc.jpeg_quant_tables(q), quant_tables(q)), q
    for q in (0, 101, -5):
        with pytest.raises(rtc.RtcError):
            rtc.jpeg_quant_tables(q)


def test_quant_and_huffman_tables_equal_pils(rtc):
    Image = pytest.importorskip("PIL.Image")
    img = Image.fromarray(np.random.default_rng(1).integers(0, 256, (16, 16, 3), dtype=np.uint8))
    for q in range(1, 101):
        buf = io.BytesIO()
        img.save(buf, "JPEG", quality=q, subsampling=0, optimize=False)
        theirs, ours = parse_jpeg(buf.getvalue()), parse_jpeg(rtc.jpeg_encode(np.asarray(img), q))
        assert theirs["dqt"] == ours["dqt"], q
        if q == 75:
            assert theirs["dht"] == ours["dht"]


def test_integer_quantiser_equals_f32_round_exhaustively(rtc):
    """sign(t) * ((2|t| + q) // (2q)) == ((t as f32) / (q as f32)).round() for every t the DCT can give and q in 1..255."""
    t = np.arange(-2048, 2049, dtype=np.int64)
    for q in range(1, 256):
        a = np.abs(t)
        ints = np.sign(t) * ((2 * a + q) // (2 * q))
        f = t.astype(np.float32) / np.float32(q)
        # f32::round: halves away from zero, exact (|f| + 0.5 is exact in f64, so no f32 rounding of the sum)
        rounded = np.sign(f) * np.floor(np.abs(f.astype(np.float64)) + 0.5)
        assert np.array_equal(ints, rounded.astype(np.int64)), q


def _pil_coefficients(ycc: np.ndarray, q: int) -> np.ndarray:
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(ycc, "YCbCr").save(buf, "JPEG", quality=q, subsampling=0, optimize=False)
    return decode_coefficients(buf.getvalue())


def _islow_quantised(rtc, ycc: np.ndarray, q: int) -> np.ndarray:
    h, w, _ = ycc.shape
    qt = quant_tables(q)
    mw, mh = (w + 7) // 8, (h + 7) // 8
    pad = np.pad(ycc, ((0, mh * 8 - h), (0, mw * 8 - w), (0, 0)), mode="edge")
    out = np.zeros((mw * mh, 3, 64), dtype=np.int64)
    for my in range(mh):
        for mx in range(mw):
            for c in range(3):
                d = rtc.jpeg_fdct(pad[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8, c]).reshape(64).astype(np.float64)
                out[my * mw + mx, c] = round_half_away(d / (8.0 * qt[1 if c else 0]))
    return out


def test_dct_is_libjpeg_islow_through_pil(rtc):
    """YCbCr-mode images go through PIL's libjpeg without colour conversion: its quantised coefficients equal
    round-half-away(rtc_jpeg_fdct / (8q)). q = 100 (divisor 8) holds whatever libjpeg's quantiser does internally."""
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (24, 40, 3), dtype=np.uint8), rng.integers(100, 140, (16, 16, 3), dtype=np.uint8)]
    for _, f in golden_canvases(rtc):
        images.append(f[:64, :64].copy())
    for img in images:
        for q in (100, 75, 50):
            theirs = _pil_coefficients(img, q)
            ours = _islow_quantised(rtc, img, q)
            assert np.array_equal(theirs, ours), (img.shape, q, int(np.abs(theirs - ours).max()))


def _roundtrip(rtc, img, q):
    b = rtc.jpeg_encode(img, q)
    got = decode_coefficients(b)
    assert np.array_equal(got, rtc.jpeg_coefficients(img, q)), (img.shape, q)
    return b


def test_decoder_recovers_coefficients(rtc):
    rng = np.random.default_rng(9)
    for name, f in golden_canvases(rtc):
        for q in (75, 100, 1):
            _roundtrip(rtc, f, q)
    for shape in ((1, 1), (9, 1), (7, 7), (8, 8), (8, 9), (33, 17), (1, 65535)):
        _roundtrip(rtc, rng.integers(0, 256, shape + (3,), dtype=np.uint8), 100)
        _roundtrip(rtc, rng.integers(0, 256, shape + (3,), dtype=np.uint8), 75)
    _roundtrip(rtc, np.full((20, 30, 3), (200, 10, 99), dtype=np.uint8), 75)


def stuffing_frames(rtc):
    """The q = 100 noise frame that stuffs many 0xFF bytes, and the first 8 x 8 noise frame whose last data byte is 0xFF
    made by the 1-bit padding (None if the search finds none)."""
    many = np.random.default_rng(11).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    for seed in range(400):
        img = np.random.default_rng(seed).integers(0, 256, (8, 8, 3), dtype=np.uint8)
        if parse_jpeg(rtc.jpeg_encode(img, 100))["data"].endswith(b"\xff\x00"):
            return many, img
    return many, None


def test_noise_stuffs_0xff_including_the_padded_byte(rtc):
    img, last = stuffing_frames(rtc)
    b = _roundtrip(rtc, img, 100)
    data = parse_jpeg(b)["data"]
    assert data.count(b"\xff\x00") > 10
    assert last is not None
    _roundtrip(rtc, last, 100)


def flat_blocks_frame():
    """4000 flat 8 x 8 blocks of random colours, one above the other: (colours, frame)."""
    rng = np.random.default_rng(3)
    cols = rng.integers(0, 256, (4000, 3))
    img = np.repeat(cols[:, None, :], 8, axis=1).reshape(4000, 8, 3)
    img = np.repeat(img[:, None], 8, axis=1).reshape(4000 * 8, 8, 3).astype(np.uint8)
    return cols, img


def test_flat_block_dc_matches_bt601(rtc):
    """The DC of a flat block at q = 100 (every divisor 1) is 8 * (sample - 128): the converted sample, checked against
    float64 BT.601 to +-1."""
    cols, img = flat_blocks_frame()
    co = rtc.jpeg_coefficients(img, 100)
    assert np.all(co[:, :, 1:] == 0)
    assert np.all(co[:, :, 0] % 8 == 0)
    got = co[:, :, 0].astype(np.float64) / 8 + 128
    r, g, b = (cols[:, k].astype(np.float64) for k in range(3))
    want = np.stack([0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128,
                     0.5 * r - 0.418688 * g - 0.081312 * b + 128], -1)
    assert np.abs(got - np.floor(want)).max() <= 1.0   # the byte is truncated: compare with the truncated value


# PSNR of PIL's decode measured on the CPU when this test was written (q = 75): golden canvases jamis_100x50 31.25 dB,
# synthetic100_96x54 28.87 dB, test7_80x60 33.65 dB (small renders with hard edges); the gradient 44.00 dB
PSNR_MIN = 25.0


def test_pil_decodes_with_psnr(rtc):
    Image = pytest.importorskip("PIL.Image")
    y, x = np.mgrid[0:120, 0:200]
    grad = np.stack([x * 255 // 199, y * 255 // 119, (x + y) * 255 // 318], -1).astype(np.uint8)
    for name, f in golden_canvases(rtc) + [("gradient", grad)]:
        dec = np.asarray(Image.open(io.BytesIO(rtc.jpeg_encode(f, 75))).convert("RGB"))
        assert dec.shape == f.shape
        assert psnr(dec, f) >= PSNR_MIN, (name, psnr(dec, f))


def test_three_and_four_channels_give_the_same_file(rtc, tmp_path):
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, (21, 35, 3), dtype=np.uint8)
    rgba = np.concatenate([rgb, rng.integers(0, 256, (21, 35, 1), dtype=np.uint8)], -1)
    assert rtc.jpeg_encode(rgb, 80) == rtc.jpeg_encode(rgba, 80)
    assert np.array_equal(rtc.jpeg_coefficients(rgb, 80), rtc.jpeg_coefficients(rgba, 80))
    rtc.write_jpeg(tmp_path / "x.jpg", rgba, 80)
    assert (tmp_path / "x.jpg").read_bytes() == rtc.jpeg_encode(rgb, 80)


def test_errors_and_cap(rtc):
    import ctypes as C
    lib = rtc.lib()
    P8 = C.POINTER(C.c_uint8)
    img = np.zeros((3, 5, 3), dtype=np.uint8)
    p = img.ctypes.data_as(P8)
    need = lib.rtc_jpeg_format(p, 5, 3, 3, 75, None, 0)
    assert need == len(rtc.jpeg_encode(img))
    for w, h, c, q in ((0, 3, 3, 75), (5, 0, 3, 75), (65536, 3, 3, 75), (5, 65536, 3, 75), (5, 3, 2, 75), (5, 3, 3, 0), (5, 3, 3, 101)):
        assert lib.rtc_jpeg_format(p, w, h, c, q, None, 0) == 0, (w, h, c, q)
    assert lib.rtc_jpeg_format(None, 5, 3, 3, 75, None, 0) == 0
    buf = np.full(need + 8, 0xAB, dtype=np.uint8)
    assert lib.rtc_jpeg_format(p, 5, 3, 3, 75, buf.ctypes.data_as(P8), 100) == need
    assert bytes(buf[:100]) == rtc.jpeg_encode(img)[:100] and np.all(buf[100:] == 0xAB)
    out16 = np.zeros(192, dtype=np.int16)
    assert lib.rtc_jpeg_coefficients(p, 5, 3, 3, 75, None) != 0
    assert lib.rtc_jpeg_coefficients(None, 5, 3, 3, 75, out16.ctypes.data_as(C.POINTER(C.c_int16))) != 0
    assert lib.rtc_jpeg_fdct(None, None) != 0
    assert lib.rtc_canvas_write_jpeg(None, p, 5, 3, 3, 75) != 0
    with pytest.raises(rtc.RtcError):
        rtc.jpeg_encode(img, 101)
    with pytest.raises(rtc.RtcError):
        rtc.jpeg_coefficients(img, 0)
