"""The writers' boundary cases (encoder_cases.py) on the MI355X: for every case and every entry it names, the device file
equals the host statement byte for byte and the case's predicate holds on the device file; the host suites' own
constructed frames through the device; every entry with its frame at byte offsets 0, 1, 3, 8 and 13 inside a larger
buffer, and on a band of rows that starts at an odd offset inside a larger frame (for GIF one of more than 2^21 pixels,
so k_gif_scan_pixels' grid-stride loop runs on an unaligned source); one encoder of each kind over all its cases in
falling, then rising size."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import encoder_cases as E  # noqa: E402
import test_host_gif as HG  # noqa: E402
import test_host_image_formats as HI  # noqa: E402
import test_host_jpeg as HJ  # noqa: E402
import test_host_png as HP  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = E.all_cases()
OFFSETS = (0, 1, 3, 8, 13)
IMAGE_FORMATS = ("bmp", "tga", "tiff", "ico", "farbfeld", "pam", "png", "jpeg", "gif", "ppm")


def to_device(px, offset=0):
    """A device buffer holding `px`'s bytes at `offset`, with spare bytes after: (buffer, address of the frame)."""
    import torch
    flat = torch.from_numpy(np.ascontiguousarray(px).reshape(-1))
    buf = torch.zeros(offset + flat.numel() + 64, dtype=torch.uint8, device="cuda:0")
    buf[offset:offset + flat.numel()] = flat.to("cuda:0")
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


class Encoders:
    """One encoder of each kind on a context; GIF files come from a fresh writer per file (a writer is one animation)."""

    def __init__(self, rtc, ctx):
        self.rtc, self.ctx = rtc, ctx
        self.png, self.jpeg, self.image = rtc.PngEncoder(ctx), rtc.JpegEncoder(ctx), rtc.ImageEncoder(ctx)

    def file(self, entry, ptr, shape, quality=75):
        h, w, c = shape
        if entry == "PngEncoder":
            return self.png.encode_device(ptr, w, h, c)
        if entry == "JpegEncoder":
            return self.jpeg.encode_device(ptr, w, h, c, quality)
        if entry == "GifWriter":
            g = self.rtc.GifWriter(self.ctx)
            try:
                g.append_device(ptr, w, h)
                return g.bytes()
            finally:
                g.close()
        assert entry.startswith("image:"), entry
        return self.image.encode_device(entry[6:], ptr, w, h, c)

    def close(self):
        for e in (self.png, self.jpeg, self.image):
            e.close()


@pytest.fixture(scope="module")
def encs(rtc, gpu):
    e = Encoders(rtc, gpu)
    yield e
    e.close()


def device_entries(case):
    return [e for e in case.entries if e not in ("png_encode", "jpeg_encode", "gif_encode")]


def host_file(rtc, case, entry):
    return rtc.image_encode(entry[6:], case.pixels()) if entry.startswith("image:") else case.host()


def assert_same(got, want, what):
    if got != want:
        k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{what}: device file differs from the host's ({len(got)} vs {len(want)} bytes, first difference at {k})")


def check_predicate(case, entry, got):
    """The case's predicate on a device file, where the entry writes the case's own kind of file."""
    px = case.pixels()
    if case.kind == "packed":
        case.check(px, got, entry[6:])
    elif got == case.host():
        case.check(px, got)
    else:   # ImageEncoder's ico row, its jpeg row (quality 75) and its png row of an RGBA frame (alpha dropped) differ
        assert entry in ("image:ico", "image:jpeg") or (entry == "image:png" and px.shape[2] == 4), entry


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_device_equals_host(rtc, encs, case):
    px = case.pixels()
    buf, ptr = to_device(px)
    for entry in device_entries(case):
        got = encs.file(entry, ptr, px.shape, case.quality)
        assert_same(got, host_file(rtc, case, entry), f"{case.name} via {entry}")
        check_predicate(case, entry, got)
    del buf


ALIGN_CASES = [c for c in CASES if c.pixels().nbytes <= 1 << 24]   # the two largest JPEG frames go through the bands below


@pytest.mark.parametrize("case", ALIGN_CASES, ids=[c.name for c in ALIGN_CASES])
def test_case_at_unaligned_offsets(rtc, encs, case):
    px = case.pixels()
    want = {entry: host_file(rtc, case, entry) for entry in device_entries(case)}
    for off in OFFSETS:
        buf, ptr = to_device(px, off)
        for entry, w in want.items():
            assert_same(encs.file(entry, ptr, px.shape, case.quality), w, f"{case.name} via {entry} at offset {off}")
        del buf


def band_entries(c):
    return ["PngEncoder", "JpegEncoder"] + (["GifWriter"] if c == 3 else []) + \
        [f"image:{f}" for f in IMAGE_FORMATS if f != "gif" or c == 3]


def host_band(rtc, entry, band):
    if entry == "PngEncoder":
        return rtc.png_encode(band)
    if entry == "JpegEncoder":
        return rtc.jpeg_encode(band, 75)
    if entry == "GifWriter":
        return rtc.gif_encode([band])
    return rtc.image_encode(entry[6:], band)


@pytest.mark.parametrize("shape,y0,rows", [((97, 255, 3), 3, 40), ((61, 201, 4), 5, 17), ((300, 1001, 3), 7, 250)])
def test_band_of_rows_at_an_odd_offset(rtc, encs, shape, y0, rows):
    """A band of rows of a larger frame of odd width: its first byte sits y0 * w * c bytes in, an odd offset (4 bytes past
    an 8-byte boundary for RGBA)."""
    h, w, c = shape
    frame = E.smooth_tile_frame(h, w, h)
    if c == 4:
        frame = np.concatenate([frame, np.random.default_rng(w).integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
    frame[::3, ::5] = np.random.default_rng(h).integers(0, 256, frame[::3, ::5].shape, dtype=np.uint8)   # > 256 colours
    assert (y0 * w * c) % (2 if c == 3 else 8) != 0
    buf, base = to_device(frame)
    band = np.ascontiguousarray(frame[y0:y0 + rows])
    for entry in band_entries(c):
        if entry == "image:ico" and max(band.shape[:2]) > 256:
            continue
        got = encs.file(entry, base + y0 * w * c, band.shape)
        assert_same(got, host_band(rtc, entry, band), f"band {shape} rows {y0}..{y0 + rows} via {entry}")
    del buf


def test_gif_frame_above_2_21_pixels_unaligned(rtc, encs):
    """2048 x 1040 pixels (> 256 workgroups x 1024 threads x 8 pixels): the grid-stride loops of k_gif_scan_pixels and
    k_gif_box_sums run a second pass, here on sources at odd offsets (u64 loads only where a thread's 24 bytes are
    8-aligned)."""
    h, w = 1040, 2048
    assert h * w > 256 * 1024 * 8
    frame = E.smooth_tile_frame(h, w, 5)
    frame[::7, ::3] = np.random.default_rng(6).integers(0, 256, frame[::7, ::3].shape, dtype=np.uint8)
    want = rtc.gif_encode([frame])
    assert rtc.gif_quantize(frame)[2] == 256   # the median cut: k_gif_box_sums runs too
    for off in (1, 3, 13):
        buf, ptr = to_device(frame, off)
        assert_same(encs.file("GifWriter", ptr, (h, w, 3)), want, f"2048x1040 at offset {off}")
        assert_same(encs.file("image:gif", ptr, (h, w, 3)), want, f"2048x1040 image:gif at offset {off}")
        del buf


def test_one_encoder_each_falling_then_rising_sizes(rtc):
    """Scratch reuse: a fresh PngEncoder, JpegEncoder and ImageEncoder each run all of their cases, largest first, then
    smallest first (the GIF writer is one animation per file: its cases go through ImageEncoder's gif row)."""
    ctx = rtc.Context(0)
    try:
        enc = Encoders(rtc, ctx)
        for kind, entry in (("png", "PngEncoder"), ("jpeg", "JpegEncoder")):
            cs = sorted((c for c in CASES if c.kind == kind), key=lambda c: -c.pixels().nbytes)
            for c in cs + cs[::-1]:
                buf, ptr = to_device(c.pixels())
                assert_same(enc.file(entry, ptr, c.pixels().shape, c.quality), c.host(), f"{c.name} via {entry} (reuse)")
                del buf
        work = [(c, e) for c in CASES for e in device_entries(c) if e.startswith("image:")]
        work.sort(key=lambda ce: -ce[0].pixels().nbytes)
        for c, e in work + work[::-1]:
            buf, ptr = to_device(c.pixels())
            assert_same(enc.file(e, ptr, c.pixels().shape), host_file(rtc, c, e), f"{c.name} via {e} (reuse)")
            del buf
        enc.close()
    finally:
        ctx.close()


def host_suite_frames(rtc):
    """The frames the host suites build for their rules, by kind."""
    png = [HP.mixed(), HP.mixed(90, 130, 4), HP.gradient(100, 150, 3), HP.noise(9, 31, 4), np.zeros((3, 5, 3), np.uint8)]
    png += [HP.mixed(60, 70, c) for c in (3, 4)] + [HP.gradient(20, 11, c) for c in (3, 4)]
    png += [HP.sized_for(k * HP.SEG + d) for k in (1, 2) for d in (-1, 0, 1)] + [f for _, f in HP.golden_frames()]
    many, last = HJ.stuffing_frames(rtc)
    assert last is not None
    jpeg = [(HJ.flat_blocks_frame()[1], 100), (many, 100), (last, 100), (np.full((20, 30, 3), (200, 10, 99), np.uint8), 75)]
    jpeg += [(f, q) for _, f in HJ.golden_canvases(rtc) for q in (75, 100, 1)]
    rng = np.random.default_rng(5)
    colours = np.unique(rng.integers(0, 256, (256, 3), dtype=np.uint8), axis=0)
    gif = [HG.small_median_cut_frame(), HG.exact_256_with_black_frame(), colours[rng.integers(0, len(colours), (40, 50))],
           HG.gradient(64, 64), HG.gradient(7, 300)]
    return png, jpeg, gif, [f for f in HI.FRAMES.values()]


def test_host_suite_frames_on_device(rtc, encs):
    png, jpeg, gif, packed = host_suite_frames(rtc)
    for i, f in enumerate(png):
        buf, ptr = to_device(f)
        got = encs.file("PngEncoder", ptr, f.shape)
        assert_same(got, rtc.png_encode(f), f"host PNG frame {i} {f.shape}")
        if f.size <= 1 << 16:
            HP.check_stream(got, f)
        del buf
    for i, (f, q) in enumerate(jpeg):
        buf, ptr = to_device(f)
        got = encs.file("JpegEncoder", ptr, f.shape, q)
        assert_same(got, rtc.jpeg_encode(f, q), f"host JPEG frame {i} {f.shape} q{q}")
        if f.size <= 1 << 16:
            assert np.array_equal(HJ.decode_coefficients(got), rtc.jpeg_coefficients(f, q))
        del buf
    for i, f in enumerate(gif):
        buf, ptr = to_device(f)
        got = encs.file("GifWriter", ptr, f.shape)
        assert_same(got, rtc.gif_encode([f]), f"host GIF frame {i} {f.shape}")
        E.check_gif(f, got)
        del buf
    for i, f in enumerate(packed):
        buf, ptr = to_device(f)
        for fmt in IMAGE_FORMATS:
            if fmt != "ico" or max(f.shape[:2]) <= 256:
                assert_same(encs.file(f"image:{fmt}", ptr, f.shape), rtc.image_encode(fmt, f), f"host image frame {i} {f.shape} {fmt}")
        del buf
