"""The save-by-name writer of include/rtc.h on the host (rtc_image_format_for_name, rtc_image_format, rtc_canvas_save):
the extension table; BMP, TGA, TIFF, ICO, farbfeld and PAM checked field by field against the layouts written in rtc.h and
decoded back to to_imgbuf's pixels (PIL for BMP, TGA, TIFF and ICO; this file's own readers for farbfeld and PAM); the
3- and 4-channel forms of a frame giving one file; the size limits; PNG, JPEG, GIF and PPM equal to their own writers.
CPU only."""
import io
import struct

import numpy as np
import pytest

from _bootstrap import package

rtc = package()
Image = pytest.importorskip("PIL.Image")

NEW = ("bmp", "tga", "tiff", "ico", "farbfeld", "pam")
ALL = NEW + ("png", "jpeg", "gif", "ppm")
STRIP = 65536


def canvas_like(h, w, seed=0):
    """A rendered-like f64 canvas: smooth gradients, a disc, highlights above 1 and a black border row."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    c = np.empty((h, w, 3))
    c[..., 0] = x / max(w - 1, 1)
    c[..., 1] = y / max(h - 1, 1)
    c[..., 2] = 0.5 + 0.5 * np.sin((x + 2 * y + seed) / 7.0)
    disc = (x - w / 2) ** 2 + (y - h / 2) ** 2 < (min(w, h) / 3) ** 2
    c[disc] = [1.3, 0.9, 0.1]
    c[-1] = 0.0
    return c


def frames():
    rng = np.random.default_rng(7)
    out = {}
    for (h, w) in [(48, 64), (37, 61)]:
        c = canvas_like(h, w, h)
        out[f"render{w}x{h}"] = rtc.color_scale255(c).reshape(h, w, 3)
        out[f"render{w}x{h}_g2.2"] = rtc.to_rgba8(c, 2.2)
    for (h, w) in [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17), (2, 16384), (3, 16385), (9, 16383), (70, 4096)]:
        out[f"noise{w}x{h}"] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return out


FRAMES = frames()


def rgba_of(px):
    """to_imgbuf's RGBA: the R, G, B bytes with alpha 255."""
    return np.concatenate([px[..., :3], np.full(px.shape[:2] + (1,), 255, np.uint8)], axis=2)


def with_random_alpha(px, seed=1):
    a = np.random.default_rng(seed).integers(0, 256, px.shape[:2] + (1,), dtype=np.uint8)
    return np.concatenate([px[..., :3], a], axis=2)


def read_farbfeld(b):
    assert b[:8] == b"farbfeld"
    w, h = struct.unpack(">II", b[8:16])
    v = np.frombuffer(b[16:], dtype=">u2").reshape(h, w, 4)
    assert np.all(v % 257 == 0)
    return (v // 257).astype(np.uint8)


def read_pam(b):
    end = b.index(b"ENDHDR\n") + 7
    head = b[:end].decode()
    lines = head.split("\n")
    assert lines[0] == "P7"
    fields = dict(line.split(" ", 1) for line in lines[1:] if " " in line)
    w, h = int(fields["WIDTH"]), int(fields["HEIGHT"])
    assert fields["DEPTH"] == "4" and fields["MAXVAL"] == "255" and fields["TUPLTYPE"] == "RGB_ALPHA"
    assert head == f"P7\nWIDTH {w}\nHEIGHT {h}\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n"
    return np.frombuffer(b[end:], dtype=np.uint8).reshape(h, w, 4)


def decode(fmt, b):
    if fmt == "farbfeld":
        return read_farbfeld(b)
    if fmt == "pam":
        return read_pam(b)
    im = Image.open(io.BytesIO(b))
    im.load()
    return np.asarray(im.convert("RGBA"))


# ---- header fields, against the layouts of include/rtc.h ----------------------------------------------------------------

def check_bmp(b, w, h):
    assert b[:2] == b"BM"
    size, res, off = struct.unpack("<III", b[2:14])
    assert (size, res, off) == (len(b), 0, 122) and len(b) == 122 + 4 * w * h
    f = struct.unpack("<IiiHHIIiiII", b[14:54])
    assert f == (108, w, h, 1, 32, 3, 4 * w * h, 0, 0, 0, 0)
    assert struct.unpack("<IIIII", b[54:74]) == (0x00FF0000, 0x0000FF00, 0x000000FF, 0xFF000000, 0x73524742)
    assert b[74:122] == bytes(48)
    px = np.frombuffer(b[122:], np.uint8).reshape(h, w, 4)[::-1]   # bottom-up rows, B,G,R,A
    return px[..., [2, 1, 0, 3]]


def check_tga(b, w, h):
    assert b[:12] == bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    assert struct.unpack("<HHBB", b[12:18]) == (w, h, 32, 0x28)
    assert len(b) == 18 + 4 * w * h
    return np.frombuffer(b[18:], np.uint8).reshape(h, w, 4)[..., [2, 1, 0, 3]]


def check_tiff(b, w, h):
    assert b[:8] == b"II" + struct.pack("<HI", 42, 8)
    assert struct.unpack("<H", b[8:10])[0] == 14
    ents = [struct.unpack("<HHI4s", b[10 + 12 * i:22 + 12 * i]) for i in range(14)]
    assert struct.unpack("<I", b[178:182])[0] == 0
    rows = max(1, STRIP // (4 * w))
    rows = min(rows, h)
    strips = -(-h // rows)
    head = 206 + (8 * strips if strips > 1 else 0)
    assert len(b) == head + 4 * w * h
    short = lambda v: struct.pack("<HH", v, 0)  # noqa: E731
    long_ = lambda v: struct.pack("<I", v)  # noqa: E731
    offs = list(range(head, head + strips * rows * 4 * w, rows * 4 * w))
    cnts = [min(rows, h - s * rows) * 4 * w for s in range(strips)]
    want = [(256, 4, 1, long_(w)), (257, 4, 1, long_(h)), (258, 3, 4, long_(182)), (259, 3, 1, short(1)), (262, 3, 1, short(2)),
            (273, 4, strips, long_(offs[0] if strips == 1 else 206)), (277, 3, 1, short(4)), (278, 4, 1, long_(rows)),
            (279, 4, strips, long_(cnts[0] if strips == 1 else 206 + 4 * strips)), (282, 5, 1, long_(190)),
            (283, 5, 1, long_(198)), (284, 3, 1, short(1)), (296, 3, 1, short(1)), (338, 3, 1, short(2))]
    assert ents == want
    assert struct.unpack("<4H", b[182:190]) == (8, 8, 8, 8)
    assert struct.unpack("<4I", b[190:206]) == (1, 1, 1, 1)
    if strips > 1:
        assert list(struct.unpack(f"<{strips}I", b[206:206 + 4 * strips])) == offs
        assert list(struct.unpack(f"<{strips}I", b[206 + 4 * strips:head])) == cnts
    return np.frombuffer(b[head:], np.uint8).reshape(h, w, 4)


def check_ico(b, w, h, px):
    assert struct.unpack("<HHH", b[:6]) == (0, 1, 1)
    bw, bh, colours, res, planes, bpp, n, off = struct.unpack("<BBBBHHII", b[6:22])
    assert (bw, bh, colours, res, planes, bpp, off) == (w % 256, h % 256, 0, 0, 1, 32, 22)
    assert n == len(b) - 22
    assert b[22:] == rtc.png_encode(rgba_of(px))   # the PNG of the RGBA frame, colour type 6
    return np.asarray(Image.open(io.BytesIO(b[22:])).convert("RGBA"))


def check_farbfeld(b, w, h):
    assert b[:16] == b"farbfeld" + struct.pack(">II", w, h) and len(b) == 16 + 8 * w * h
    return read_farbfeld(b)


def check_pam(b, w, h):
    assert len(b) == len(f"P7\nWIDTH {w}\nHEIGHT {h}\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n") + 4 * w * h
    return read_pam(b)


CASES = [(f, n) for f in NEW for n in sorted(FRAMES) if f != "ico" or max(FRAMES[n].shape[:2]) <= 256]  # ICO: 256 at most


@pytest.mark.parametrize("fmt,name", CASES)
def test_new_formats_fields_and_pixels(fmt, name):
    px = FRAMES[name]
    h, w = px.shape[:2]
    b = rtc.image_encode(fmt, px)
    want = rgba_of(px)
    if fmt == "ico":
        got = check_ico(b, w, h, px)
    else:
        got = {"bmp": check_bmp, "tga": check_tga, "tiff": check_tiff, "farbfeld": check_farbfeld, "pam": check_pam}[fmt](b, w, h)
    assert np.array_equal(got, want), (fmt, name)
    assert np.array_equal(decode(fmt, b), want), (fmt, name)


@pytest.mark.parametrize("fmt", ALL)
def test_three_and_four_channels_give_one_file(fmt):
    for name, px in FRAMES.items():
        h, w = px.shape[:2]
        if fmt == "ico" and (w > 256 or h > 256):
            continue
        rgb = np.ascontiguousarray(px[..., :3])
        b = rtc.image_encode(fmt, rgb)
        assert rtc.image_encode(fmt, rgba_of(px)) == b, (fmt, name)
        assert rtc.image_encode(fmt, with_random_alpha(px)) == b, (fmt, name)   # alpha is never read


def test_delegated_formats_equal_their_writers():
    for name, px in FRAMES.items():
        rgb = np.ascontiguousarray(px[..., :3])
        h, w = rgb.shape[:2]
        assert rtc.image_encode("png", px) == rtc.png_encode(rgb), name
        assert rtc.image_encode("jpeg", px) == rtc.jpeg_encode(rgb, 75) == rtc.jpeg_encode(px, 75), name
        assert rtc.image_encode("gif", px) == rtc.gif_encode([rgb]), name
        n = rtc.lib().rtc_canvas_format_ppm_rgb8(rgb.ctypes.data_as(rtc.C.POINTER(rtc.C.c_uint8)), w, h, None, 0)
        buf = rtc.C.create_string_buffer(n + 1)
        rtc.lib().rtc_canvas_format_ppm_rgb8(rgb.ctypes.data_as(rtc.C.POINTER(rtc.C.c_uint8)), w, h, buf, n + 1)
        assert rtc.image_encode("ppm", px) == buf.raw[:n], name


def test_ico_tga_bmp_tiff_limits():
    px = np.full((256, 256, 3), 9, np.uint8)
    b = rtc.image_encode("ico", px)
    assert b[6:8] == b"\x00\x00" and np.array_equal(decode("ico", b), rgba_of(px))
    for shape in [(257, 256, 3), (256, 257, 3), (1, 257, 4)]:
        with pytest.raises(rtc.RtcError) as e:
            rtc.image_encode("ico", np.zeros(shape, np.uint8))
        assert e.value.status == 4
    assert len(rtc.image_encode("tga", np.zeros((1, 65535, 3), np.uint8))) == 18 + 4 * 65535
    for shape in [(1, 65536, 3), (65536, 1, 3)]:
        with pytest.raises(rtc.RtcError) as e:
            rtc.image_encode("tga", np.zeros(shape, np.uint8))
        assert e.value.status == 4
    # files beyond a u32: refused before any pixel is read (a 1-pixel buffer stands in for the frame)
    one = (rtc.C.c_uint8 * 4)()
    for f in (rtc.IMAGE_FORMATS["bmp"], rtc.IMAGE_FORMATS["tiff"]):
        assert rtc.lib().rtc_image_format(f, one, 40000, 40000, 3, None, 0) == 0
        assert rtc.lib().rtc_image_format(f, one, 0, 1, 3, None, 0) == 0
    assert rtc.lib().rtc_image_format(10, one, 1, 1, 3, None, 0) == 0         # not a format
    assert rtc.lib().rtc_image_format(100, one, 1, 1, 3, None, 0) == 0        # an internal packing is not one either
    assert rtc.lib().rtc_image_format(rtc.IMAGE_FORMATS["pam"], one, 1, 1, 2, None, 0) == 0


def test_extension_table():
    F = rtc.IMAGE_FORMATS
    cases = {"a.png": "png", "A.PNG": "png", "x.jpg": "jpeg", "x.JPEG": "jpeg", "x.Jpg": "jpeg", "y.gif": "gif", "z.ppm": "ppm",
             "b.bmp": "bmp", "b.BMP": "bmp", "t.tga": "tga", "t.TGA": "tga", "i.tif": "tiff", "i.tiff": "tiff", "i.TiF": "tiff",
             "c.ico": "ico", "f.ff": "farbfeld", "f.FF": "farbfeld", "p.pam": "pam", "dir.d/x.bmp": "bmp",
             "scene.png.bmp": "bmp", "x.bmp.png": "png", "/tmp/a.b/c.tga": "tga"}
    for name, fmt in cases.items():
        assert rtc.image_format_for_name(name) == F[fmt], name
    for name in ["noext", "", ".png", "dir/.bmp", "a.", "a.xyz", "a.png.bak", "dir.png/file", "a.pgm", "a.webp", "a.hdr",
                 "a.jpe", "a.tif ", "a.p ng"]:
        with pytest.raises(rtc.RtcError) as e:
            rtc.image_format_for_name(name)
        assert e.value.status == 8, name


def test_canvas_save_by_name(tmp_path):
    px = FRAMES["render61x37"]
    for name, fmt in {"a.bmp": "bmp", "b.TGA": "tga", "c.tif": "tiff", "d.tiff": "tiff", "e.ico": "ico", "f.ff": "farbfeld",
                      "g.pam": "pam", "h.png": "png", "i.jpeg": "jpeg", "j.JPG": "jpeg", "k.gif": "gif", "l.ppm": "ppm"}.items():
        rtc.save(tmp_path / name, px)
        assert (tmp_path / name).read_bytes() == rtc.image_encode(fmt, px), name
    for name in ["x.xyz", "noext", "x.png.tmp", ".bmp"]:
        with pytest.raises(rtc.RtcError) as e:
            rtc.save(tmp_path / name, px)
        assert e.value.status == 8
        assert not (tmp_path / name).exists(), name
    with pytest.raises(rtc.RtcError) as e:
        rtc.save(tmp_path / "big.ico", np.zeros((300, 10, 3), np.uint8))
    assert e.value.status == 4 and not (tmp_path / "big.ico").exists()
