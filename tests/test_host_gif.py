"""The GIF writer of StartAnimation / AddFrame on the host (rtc_gif_quantize, rtc_gif_lzw, rtc_gif_format): container
layout, the exact and median-cut quantisers, nearest-entry mapping and the segmented LZW stream, decoded by a parser in
this file and, where PIL is importable, by PIL as well."""
import io
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
S = 4096


def lzw_decode(data: bytes, min_size: int = 8) -> list:
    """A plain GIF LZW decoder (variable width, clear / end codes, 4096-entry dictionary)."""
    clear, eoi = 1 << min_size, (1 << min_size) + 1
    out, pos, nbits = [], 0, len(data) * 8
    width, table, prev = min_size + 1, None, None

    def reset():
        return [bytes([i]) for i in range(clear)] + [b"", b""]

    table = reset()
    while pos + width <= nbits:
        code = (int.from_bytes(data[pos >> 3: (pos >> 3) + 3], "little") >> (pos & 7)) & ((1 << width) - 1)
        pos += width
        if code == clear:
            table, width, prev = reset(), min_size + 1, None
            continue
        if code == eoi:
            return out
        if prev is None:
            entry = table[code]
        else:
            entry = table[code] if code < len(table) else prev + prev[:1]
            if len(table) < 4096:
                table.append(prev + entry[:1])
        out.append(entry)
        prev = entry
        if len(table) == (1 << width) and width < 12:
            width += 1
    raise AssertionError("no end code")


def parse_gif(b: bytes) -> dict:
    """Blocks of a GIF89a file -> header fields and per-frame (gce, descriptor, table, decoded indices)."""
    assert b[:6] == b"GIF89a"
    w, h, packed = int.from_bytes(b[6:8], "little"), int.from_bytes(b[8:10], "little"), b[10]
    p, frames, gce = 13, [], None
    assert packed & 0x80 == 0, "no global colour table"
    while True:
        t = b[p]
        if t == 0x3B:
            assert p == len(b) - 1, "bytes after the trailer"
            break
        if t == 0x21:
            label, size = b[p + 1], b[p + 2]
            assert label == 0xF9 and size == 4, "only graphic control extensions"
            gce = {"packed": b[p + 3], "delay": int.from_bytes(b[p + 4:p + 6], "little"), "transparent": b[p + 6]}
            assert b[p + 7] == 0
            p += 8
            continue
        assert t == 0x2C, hex(t)
        left, top, fw, fh = (int.from_bytes(b[p + 1 + 2 * k: p + 3 + 2 * k], "little") for k in range(4))
        fp = b[p + 9]
        p += 10
        table = None
        if fp & 0x80:
            n = 2 << (fp & 7)
            table = np.frombuffer(b[p:p + 3 * n], dtype=np.uint8).reshape(n, 3)
            p += 3 * n
        min_size = b[p]
        p += 1
        data = bytearray()
        while b[p]:
            assert 1 <= b[p] <= 255
            data += b[p + 1:p + 1 + b[p]]
            p += 1 + b[p]
        p += 1
        idx = np.frombuffer(b"".join(lzw_decode(bytes(data), min_size)), dtype=np.uint8)
        frames.append({"gce": gce, "rect": (left, top, fw, fh), "packed": fp, "table": table, "min_size": min_size,
                       "indices": idx, "blocks_ok": True, "data": bytes(data)})
        gce = None
    return {"size": (w, h), "frames": frames}


def decoded_rgb(parsed: dict) -> list:
    w, h = parsed["size"]
    return [f["table"][f["indices"]].reshape(h, w, 3) for f in parsed["frames"]]


def pil_frames(b: bytes):
    try:
        from PIL import Image
    except ImportError:
        return None
    im = Image.open(io.BytesIO(b))
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append(np.array(im.convert("RGB")))
    return out


def check_roundtrip(rtc, frames):
    """Encode, parse, check the layout, and return the decoded frames (also checked against PIL where it exists)."""
    b = rtc.gif_encode(frames)
    g = parse_gif(b)
    h, w = frames[0].shape[:2]
    assert g["size"] == (w, h) and len(g["frames"]) == len(frames)
    for f in g["frames"]:
        assert f["gce"] == {"packed": 0, "delay": 7, "transparent": 0}
        assert f["rect"] == (0, 0, w, h) and f["packed"] == 0x87 and f["table"].shape == (256, 3) and f["min_size"] == 8
        assert f["indices"].size == w * h
    dec = decoded_rgb(g)
    p = pil_frames(b)
    if p is not None:
        assert len(p) == len(dec) and all(np.array_equal(x, y) for x, y in zip(p, dec))
    return b, g, dec


def brute_nearest(frame, pal):
    px = frame.reshape(-1, 3).astype(np.int64)
    d = ((px[:, None, :] - pal[None, :, :].astype(np.int64)) ** 2).sum(-1)
    return np.argmin(d, axis=1).astype(np.uint8)   # first minimum: the lowest index on ties


def gradient(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 127 // max(w + h - 2, 1))], -1).astype(np.uint8)


def uniform_676_mse(frame):
    levels = [np.round(np.linspace(0, 255, k)).astype(np.int64) for k in (6, 7, 6)]
    px = frame.reshape(-1, 3).astype(np.int64)
    err = 0
    for c in range(3):
        err += ((px[:, c:c + 1] - levels[c][None, :]) ** 2).min(axis=1).sum()
    return err / px.size


def test_container_layout_and_multi_frame(rtc):
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (23, 31, 3), dtype=np.uint8) for _ in range(3)]
    b, g, dec = check_roundtrip(rtc, frames)
    assert b[10:13] == b"\0\0\0" and b.count(b"NETSCAPE") == 0 and b[-1] == 0x3B
    for f, d in zip(frames, dec):
        pal, idx, used = rtc.gif_quantize(f)
        assert np.array_equal(d, pal[idx])


def test_exact_palette_is_lossless_and_sorted(rtc):
    rng = np.random.default_rng(5)
    colours = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    colours = np.unique(colours, axis=0)
    frame = colours[rng.integers(0, len(colours), (40, 50))]
    pal, idx, used = rtc.gif_quantize(frame)
    keys = colours.astype(np.int64) @ np.array([65536, 256, 1])
    srt = colours[np.argsort(keys)]
    assert used == len(colours) and np.array_equal(pal[:used], srt) and not pal[used:].any()
    _, _, dec = check_roundtrip(rtc, [frame])
    assert np.array_equal(dec[0], frame)


def test_exact_palette_256_with_black(rtc):
    frame = exact_256_with_black_frame()
    pal, idx, used = rtc.gif_quantize(frame)
    assert used == len(np.unique(frame.reshape(-1, 3), axis=0))
    _, _, dec = check_roundtrip(rtc, [frame])
    assert np.array_equal(dec[0], frame)


@pytest.mark.parametrize("shape", [(8, 8), (17, 33), (1, 600), (600, 1)])
def test_mapping_is_nearest_entry_with_lowest_index_ties(rtc, shape):
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    pal, idx, used = rtc.gif_quantize(frame)
    assert np.array_equal(idx.ravel(), brute_nearest(frame, pal))
    _, _, dec = check_roundtrip(rtc, [frame])
    assert np.array_equal(dec[0], pal[idx])


def small_median_cut_frame():
    """Two flat colours plus a sprinkle of 300 colours in one bin."""
    rng = np.random.default_rng(2)
    frame = np.zeros((30, 30, 3), dtype=np.uint8)
    frame[:, :15] = (200, 40, 40)
    frame[:, 15:] = (16, 16, 200)
    i = np.arange(300)
    pos = rng.permutation(900)[:300]
    frame.reshape(-1, 3)[pos] = np.stack([200 + (i & 7), 40 + ((i >> 3) & 7), 40 + ((i >> 6) & 7)], -1)   # one bin
    return frame


def exact_256_with_black_frame():
    v = np.arange(256, dtype=np.uint8)
    frame = np.stack([v, v[::-1], v], -1).reshape(16, 16, 3)
    frame[0, 0] = 0   # black replaces one colour: 256 -> 256 distinct still (0,255,0) gone, (0,0,0) in
    return frame


def test_median_cut_rules_on_a_small_frame(rtc):
    """Two flat colours plus a sprinkle: 300 distinct colours in few bins, so boxes run out before 256 and the unused
    entries are black; every box mean is the rounded mean of its pixels."""
    frame = small_median_cut_frame()
    assert len(np.unique(frame.reshape(-1, 3), axis=0)) > 256
    pal, idx, used = rtc.gif_quantize(frame)
    assert used == 2 and not pal[used:].any()
    px = frame.reshape(-1, 3).astype(np.int64)
    for k, sel in enumerate((px[:, 0] < 100, px[:, 0] >= 100)):   # the longest axis is r: box 0 = the blue half
        n = sel.sum()
        assert tuple(pal[k]) == tuple((2 * px[sel].sum(0) + n) // (2 * n)), (k, pal[:2])
    assert np.array_equal(idx.ravel(), brute_nearest(frame, pal))


@pytest.mark.parametrize("name", ["jamis_100x50", "synthetic100_96x54", "test7_80x60"])
def test_median_cut_beats_uniform_palette_on_golden_canvases(rtc, name):
    canvas = np.load(ROOT / "tests" / "golden" / f"{name}.npy")
    frame = np.ascontiguousarray(rtc.to_rgba8(canvas)[..., :3])
    pal, idx, used = rtc.gif_quantize(frame)
    mse = ((pal[idx].astype(np.int64) - frame.astype(np.int64)) ** 2).mean() * 3
    assert mse <= uniform_676_mse(frame), (mse, uniform_676_mse(frame))
    _, _, dec = check_roundtrip(rtc, [frame])
    assert np.array_equal(dec[0], pal[idx])


@pytest.mark.parametrize("shape", [(64, 64), (300, 200), (1080, 1920)])
def test_median_cut_beats_uniform_palette_on_gradients(rtc, shape):
    frame = gradient(*shape)
    pal, idx, used = rtc.gif_quantize(frame)
    mse = ((pal[idx].astype(np.int64) - frame.astype(np.int64)) ** 2).mean() * 3
    assert mse <= uniform_676_mse(frame)


@pytest.mark.parametrize("n", [1, 2, 3, S - 1, S, S + 1, 2 * S, 3 * S, 3 * S + 7])
def test_lzw_segment_edges(rtc, n):
    rng = np.random.default_rng(n)
    idx = (rng.integers(0, 4, n) * 60).astype(np.uint8)
    stream = rtc.gif_lzw(idx)
    assert np.array_equal(np.frombuffer(b"".join(lzw_decode(stream)), np.uint8), idx)
    clears = n_clears(stream)
    assert clears == (n + S - 1) // S   # one per segment, nothing else fills a dictionary here


def n_clears(stream: bytes, min_size: int = 8) -> int:
    """Count clear codes by re-running the decoder's width rule."""
    clear, eoi = 256, 257
    pos, width, size, prev, k = 0, 9, 258, False, 0
    while True:
        code = (int.from_bytes(stream[pos >> 3:(pos >> 3) + 3], "little") >> (pos & 7)) & ((1 << width) - 1)
        pos += width
        if code == clear:
            k += 1
            width, size, prev = 9, 258, False
            continue
        if code == eoi:
            return k
        if prev and size < 4096:
            size += 1
        prev = True
        if size == (1 << width) and width < 12:
            width += 1


def test_lzw_noise_fills_the_dictionary_inside_a_segment(rtc):
    rng = np.random.default_rng(9)
    n = 2 * S + 100
    idx = rng.integers(0, 256, n).astype(np.uint8)
    stream = rtc.gif_lzw(idx)
    assert np.array_equal(np.frombuffer(b"".join(lzw_decode(stream)), np.uint8), idx)
    assert n_clears(stream) > 3   # 3 segments + at least one dictionary restart
    frame = rng.integers(0, 256, (S // 64 * 3, 64, 3), dtype=np.uint8)
    pal, idx2, used = rtc.gif_quantize(frame)
    _, _, dec = check_roundtrip(rtc, [frame])
    assert np.array_equal(dec[0], pal[idx2])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (13, 11), (1, S), (1, S - 1), (1, S + 1), (4, S), (2 * S + 3, 1)])
def test_edge_sizes_roundtrip(rtc, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    frame = (rng.integers(0, 3, shape + (3,)) * 100).astype(np.uint8)
    _, _, dec = check_roundtrip(rtc, [frame])
    assert np.array_equal(dec[0], frame)    # <= 27 colours: exact


def test_single_colour_frame(rtc):
    frame = np.full((50, 70, 3), (12, 34, 56), dtype=np.uint8)
    pal, idx, used = rtc.gif_quantize(frame)
    assert used == 1 and tuple(pal[0]) == (12, 34, 56) and not idx.any()
    b, _, dec = check_roundtrip(rtc, [frame])
    assert np.array_equal(dec[0], frame) and len(b) < 1000


def test_errors(rtc):
    a = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(rtc.RtcError) as e:
        rtc.gif_encode([a, np.zeros((5, 4, 3), np.uint8)])
    assert "RTC_ERR_ARG" in str(e.value)
    with pytest.raises(rtc.RtcError) as e:
        rtc.gif_encode([np.zeros((1, 65536, 3), np.uint8)])
    assert "RTC_ERR_ARG" in str(e.value)
    with pytest.raises(rtc.RtcError):
        rtc.gif_file_header(70000, 3)
