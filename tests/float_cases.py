"""The case tables of the float file writers (Radiance HDR, PFM, OpenEXR), shared by the host test
(test_host_float_formats.py) and the GPU test (test_gpu_float_formats.py), and the small numpy decoders both use — written
from the public descriptions of the three formats, independent of the library.

Everything here is numpy only; nothing imports the package."""
import struct

import numpy as np

# ---- conversions -----------------------------------------------------------------------------------------------------


def _bits(u):
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


# ties, the double-rounding witness, the largest and smallest normals and subnormals of f32 and f16 and their neighbours,
# +-0, +-inf, NaNs of several payloads
CONVERSION_VALUES = np.array(
    [0.0, -0.0, 1.0, -1.0, 0.1, -0.1, 1.0 / 3.0, 2.5, 1e10, -1e10,
     1 + 2.0 ** -11 + 2.0 ** -30,                               # f16 0x3C01 directly, 0x3C00 through f32
     1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 - 2.0 ** -40,      # f16 ties (to even: down, up) and just below one
     1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -52, 1 + 2.0 ** -24 - 2.0 ** -53,   # the same for f32
     65504.0, 65519.999, 65520.0, 65536.0, -65520.0,            # f16: largest normal, the last value below the tie, overflow
     2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -14 * (1 - 2.0 ** -12),   # f16: smallest normal and below it
     2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -40), 3 * 2.0 ** -25, 2.0 ** -26, 1023 * 2.0 ** -24,   # f16 subnormals
     3.4028234663852886e38, 3.4028235677973366e38, 3.4028235677973362e38, 1e39, -1e39, 1.7976931348623157e308,   # f32 top
     2.0 ** -126, 2.0 ** -126 * (1 - 2.0 ** -24), 2.0 ** -126 * (1 - 2.0 ** -25),    # f32: smallest normal and below it
     2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * (1 + 2.0 ** -50), 3 * 2.0 ** -150, 2.0 ** -151, 1e-45, 7e-46,    # f32 subnormals
     2.2250738585072014e-308, 5e-324, -5e-324,                 # f64's own smallest normal and subnormal
     np.inf, -np.inf, np.nan, -np.nan,
     _bits(0x7FF0000000000001), _bits(0xFFF0000000000001), _bits(0x7FF8000000000000), _bits(0x7FFFFFFFFFFFFFFF),
     _bits(0xFFF4000020000000), _bits(0x7FF0000020000000)],
    dtype=np.float64)


def f32_bits(x):
    """numpy's f64 -> f32 (IEEE round-to-nearest-even), NaNs made 0x7FC00000."""
    with np.errstate(all="ignore"):
        b = np.asarray(x, dtype=np.float64).astype(np.float32).view(np.uint32).copy()
    b[np.isnan(x)] = 0x7FC00000
    return b


def f16_bits(x):
    """numpy's f64 -> f16 (rounded directly from the double), NaNs made 0x7E00."""
    with np.errstate(all="ignore"):
        b = np.asarray(x, dtype=np.float64).astype(np.float16).view(np.uint16).copy()
    b[np.isnan(x)] = 0x7E00
    return b


RGBE_TOP = float.fromhex("0x1.FEp+126")


def rgbe_map(rgb):
    """The rule's first step: NaN or < 0 -> 0, above 0x1.FEp+126 -> that."""
    c = np.asarray(rgb, dtype=np.float64).copy()
    c[np.isnan(c) | (c < 0)] = 0.0
    return np.minimum(c, RGBE_TOP)


def rgbe_bytes(rgb):
    """The RGBE rule of include/rtc.h restated with np.frexp / np.ldexp: (..., 3) float64 -> (..., 4) uint8."""
    c = rgbe_map(rgb)
    v = c.max(axis=-1)
    _, e = np.frexp(v)
    out = np.zeros(c.shape[:-1] + (4,), dtype=np.uint8)
    lit = v >= 1e-32
    b = np.floor(np.ldexp(c, (8 - e)[..., None]))
    assert b[lit].max(initial=0) <= 255
    out[..., :3] = np.where(lit[..., None], b, 0).astype(np.uint8)
    out[..., 3] = np.where(lit, e + 128, 0).astype(np.uint8)
    return out


def rgbe_decode(bytes4):
    """byte * 2^(E - 136); E = 0 is black."""
    b = np.asarray(bytes4)
    return np.where(b[..., 3:4] == 0, 0.0, np.ldexp(b[..., :3].astype(np.float64), b[..., 3:4].astype(np.int64) - 136))


# ---- the Radiance run-length rule ------------------------------------------------------------------------------------


def rle_reference(plane):
    """The maximal-run rule of include/rtc.h, restated: runs of >= 4 become (128 + n, byte) tokens of at most 127, the
    stretches between them (n, bytes) tokens of at most 128."""
    b = bytes(bytearray(np.asarray(plane, dtype=np.uint8)))
    out, lit, i = bytearray(), bytearray(), 0

    def flush():
        for s in range(0, len(lit), 128):
            out.append(len(lit[s:s + 128]))
            out.extend(lit[s:s + 128])
        lit.clear()

    while i < len(b):
        j = i
        while j < len(b) and b[j] == b[i]:
            j += 1
        if j - i >= 4:
            flush()
            for s in range(0, j - i, 127):
                out.extend((128 + min(127, j - i - s), b[i]))
        else:
            lit.extend(b[i:j])
        i = j
    flush()
    return bytes(out)


def rle_decode(data, width, at=0):
    """The standard decoder of one plane: a count above 128 repeats the next byte count - 128 times, any other copies
    `count` bytes. Returns the plane and where it ended."""
    out = bytearray()
    while len(out) < width:
        c = data[at]
        at += 1
        if c > 128:
            out.extend(data[at:at + 1] * (c - 128))
            at += 1
        else:
            assert c > 0, "a zero count"
            out.extend(data[at:at + c])
            at += c
    assert len(out) == width, "a token crosses the plane's end"
    return np.frombuffer(bytes(out), dtype=np.uint8), at


def _runs(*pairs):
    """A plane from (length, value) pairs."""
    return np.concatenate([np.full(n, v, dtype=np.uint8) for n, v in pairs])


def _literal(n, first=0):
    """n bytes with no two neighbours equal."""
    return ((np.arange(n) % 7) * 2 + 1 + first).astype(np.uint8)


def boundary_planes():
    """{name: uint8 plane}: planes that sit on every decision of the run-length rule."""
    p = {}
    for n in (3, 4, 5, 126, 127, 128, 129, 254, 255):     # a run of n between two literals
        p[f"run{n}"] = np.concatenate([_literal(5), _runs((n, 200)), _literal(6, 20)])
    for n in (1, 127, 128, 129, 257):                      # a literal stretch of n between two runs
        p[f"lit{n}"] = np.concatenate([_runs((9, 100)), _literal(n), _runs((4, 101))])
    p["run_at_both_ends"] = np.concatenate([_runs((4, 7)), _literal(11), _runs((130, 9))])
    p["short_runs_are_literal"] = _runs((3, 1), (3, 2), (2, 3), (1, 4), (3, 5), (4, 6), (3, 7), (3, 6), (4, 6))
    p["adjacent_runs"] = _runs((4, 1), (4, 2), (127, 3), (127, 4), (128, 5), (5, 4))
    p["alternating"] = (np.arange(300) % 2).astype(np.uint8)     # the worst case: w + ceil(w / 128)
    p["alternating128"] = (np.arange(128) % 2).astype(np.uint8)
    p["constant"] = np.full(300, 42, dtype=np.uint8)
    p["constant8"] = np.full(8, 0, dtype=np.uint8)
    p["wave_edges"] = np.concatenate([_literal(61), _runs((6, 9)), _literal(59, 30), _runs((4, 8)), _literal(62), _runs((3, 5), (70, 6))])
    return p


def plane_max(w):
    return w + (w + 127) // 128


def canvas_from_bytes(r, g, b, e):
    """The (H, W, 3) canvas whose RGBE bytes are these planes (each (H, W) uint8): byte * 2^(E - 136) is exact in f64. Holds
    when every pixel's largest byte is >= 128 (its mantissa is normalised) or the pixel is all zero."""
    rgb = np.stack([r, g, b], axis=-1)
    assert np.all((rgb.max(axis=-1) >= 128) | ((rgb.max(axis=-1) == 0) & (np.asarray(e) == 0)))
    return np.ldexp(rgb.astype(np.float64), np.asarray(e, dtype=np.int64)[..., None] - 136)


def plane_canvases():
    """{name: (canvas, (H, W, 4) bytes)}: every boundary plane arriving as the R, the G and the B plane of a row (three
    rows), the other planes constant so that the mantissas stay normalised."""
    out = {}
    for name, p in boundary_planes().items():
        w = p.size
        full, e = np.full(w, 255, dtype=np.uint8), np.full(w, 130, dtype=np.uint8)
        rows = [(p, full, full, e), (full, p, full, e + 1), (full, full, p, e + 2)]
        planes = [np.stack([row[k] for row in rows]) for k in range(4)]
        out[name] = (canvas_from_bytes(*planes), np.stack(planes, axis=-1))
    return out


# ---- canvases and planes ---------------------------------------------------------------------------------------------

SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 1e-33, 1e39, 65504.0, 65520.0, 1e-8, 6e-8, -3.0, 1e38 * 3.3, 2.0 ** -130])


def noise_canvas(h, w, seed):
    """Values around [0, 4) with negatives, runs of equal pixels (so the RLE planes have runs of every short length) and the
    special values sprinkled in."""
    rng = np.random.default_rng(seed)
    c = rng.random((h, w, 3)) * 4.5 - 0.5
    flat = c.reshape(-1, 3)
    n = flat.shape[0]
    i = 0
    while i < n:                                      # runs: copy a pixel over the next k - 1
        k = int(rng.choice([1, 1, 1, 2, 3, 4, 5, 8, 30, 130, 260]))
        flat[i:i + k] = flat[i]
        i += k
    pick = rng.integers(0, flat.size, max(1, flat.size // 37))
    c.reshape(-1)[pick] = rng.choice(SPECIALS, pick.size)
    return c


def noise_planes(h, w, seed):
    """AOV planes of the dtypes rtc_aov_buffers names, with misses (+inf depth, index -1)."""
    rng = np.random.default_rng(seed + 1000)
    depth = rng.random((h, w)) * 50
    index = rng.integers(-1, 40, (h, w), dtype=np.int32)
    depth[index < 0] = np.inf
    return {"index": index, "depth": depth, "point": rng.standard_normal((h, w, 3)) * 10, "normal": rng.standard_normal((h, w, 3)),
            "flags": rng.integers(0, 4, (h, w), dtype=np.uint8), "shadow": rng.integers(0, 300, (h, w)).astype(np.uint16)}


EXR_CHANNELS = ("B", "G", "N.X", "N.Y", "N.Z", "P.X", "P.Y", "P.Z", "R", "Z", "id", "shadow")
SIZES = [(1, 1), (1, 7), (1, 8), (1, 9), (37, 7), (37, 8), (37, 64), (1, 65), (37, 129), (1, 32767), (1, 32768), (3, 1920)]   # (h, w)


def cases():
    """[(id, fmt, canvas or None, planes or None, rgb_type)]: every format at every size, EXR with each single channel
    group, with all twelve channels, as HALF and as FLOAT; the boundary planes through HDR."""
    out = []
    for k, (h, w) in enumerate(SIZES):
        c = noise_canvas(h, w, 100 + k)
        out.append((f"hdr-{w}x{h}", "hdr", c, None, "half"))
        out.append((f"pfm-{w}x{h}", "pfm", c, None, "half"))
        out.append((f"exr-half-{w}x{h}", "exr", c, None, "half"))
        if w * h <= 37 * 129 or h == 3:
            out.append((f"exr-all-float-{w}x{h}", "exr", c, noise_planes(h, w, k), "float"))
    h, w = 5, 9
    c, p = noise_canvas(h, w, 7), noise_planes(h, w, 7)
    out.append(("exr-rgb-float", "exr", c, None, "float"))
    for name in ("depth", "normal", "point", "index", "shadow"):
        out.append((f"exr-only-{name}", "exr", None, {name: p[name]}, "half"))
    out.append(("exr-all-half", "exr", c, p, "half"))
    out.append(("exr-planes-no-canvas", "exr", None, p, "half"))
    for name, (canvas, _) in plane_canvases().items():
        out.append((f"hdr-plane-{name}", "hdr", canvas, None, "half"))
    return out


# ---- decoders --------------------------------------------------------------------------------------------------------


def decode_pfm(data):
    """-> (H, W, 3) uint32: the f32 bits, top row first."""
    assert data[:3] == b"PF\n"
    end = 3
    for _ in range(2):
        end = data.index(b"\n", end) + 1
    dims, scale = data[3:end].split(b"\n")[:2]
    w, h = (int(v) for v in dims.split())
    assert scale == b"-1.0"
    body = np.frombuffer(data, dtype="<u4", offset=end)
    assert body.size == w * h * 3, "file length"
    return body.reshape(h, w, 3)[::-1]


def decode_hdr(data):
    """-> (H, W, 4) uint8 R,G,B,E; checks the scanline markers and that the file ends with the last token."""
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y "
    assert data.startswith(head)
    end = data.index(b"\n", len(head)) + 1
    hs, xs, ws = data[len(head):end].split()
    assert xs == b"+X"
    h, w = int(hs), int(ws)
    if not 8 <= w <= 32767:
        assert len(data) == end + 4 * w * h, "file length"
        return np.frombuffer(data, dtype=np.uint8, offset=end).reshape(h, w, 4)
    out = np.empty((h, w, 4), dtype=np.uint8)
    at = end
    for y in range(h):
        assert data[at:at + 4] == bytes((2, 2, w >> 8, w & 255)), f"scanline {y}'s marker"
        at += 4
        for c in range(4):
            start = at
            out[y, :, c], at = rle_decode(data, w, at)
            assert at - start <= plane_max(w)
    assert at == len(data), "file length"
    return out


def exr_header_bytes(names_types, w, h):
    """The header the layout of include/rtc.h gives for these (name, type) channels, built independently."""
    def attr(name, typ, value):
        return name + b"\0" + typ + b"\0" + struct.pack("<i", len(value)) + value
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t in names_types) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (bytes((0x76, 0x2F, 0x31, 0x01)) + struct.pack("<i", 2) + attr(b"channels", b"chlist", chlist)
            + attr(b"compression", b"compression", b"\0") + attr(b"dataWindow", b"box2i", box) + attr(b"displayWindow", b"box2i", box)
            + attr(b"lineOrder", b"lineOrder", b"\0") + attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
            + attr(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0, 0)) + attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")


def decode_exr(data):
    """-> ({channel: (H, W) array of its bits: uint16 for HALF, uint32 for FLOAT and UINT}, [(name, type)]). Parses the
    attributes generically, follows every scanline offset and checks the file's length against the formula."""
    assert data[:8] == bytes((0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0))
    at, attrs = 8, {}
    while data[at] != 0:
        z = data.index(b"\0", at)
        name, at = data[at:z], z + 1
        z = data.index(b"\0", at)
        typ, at = data[at:z], z + 1
        size, = struct.unpack_from("<i", data, at)
        attrs[name] = (typ, data[at + 4:at + 4 + size])
        at += 4 + size
    at += 1
    assert list(attrs) == [b"channels", b"compression", b"dataWindow", b"displayWindow", b"lineOrder", b"pixelAspectRatio",
                           b"screenWindowCenter", b"screenWindowWidth"]
    assert attrs[b"compression"] == (b"compression", b"\0") and attrs[b"lineOrder"] == (b"lineOrder", b"\0")
    x0, y0, x1, y1 = struct.unpack("<4i", attrs[b"dataWindow"][1])
    assert (x0, y0) == (0, 0) and attrs[b"displayWindow"] == attrs[b"dataWindow"]
    w, h = x1 + 1, y1 + 1
    chans, c, cl = [], 0, attrs[b"channels"][1]
    while cl[c] != 0:
        z = cl.index(b"\0", c)
        t, lin, xs, ys = struct.unpack_from("<iB3xii", cl, z + 1)
        assert (lin, xs, ys) == (0, 1, 1)
        chans.append((cl[c:z].decode(), t))
        c = z + 17
    assert c + 1 == len(cl)
    assert [n for n, _ in chans] == sorted(n for n, _ in chans), "channels are stored in byte-wise alphabetical order"
    assert data[:at] == exr_header_bytes(chans, w, h)
    pixel = sum(2 if t == 1 else 4 for _, t in chans)
    line = 8 + pixel * w
    assert len(data) == at + 8 * h + line * h, "file length"
    offsets = np.frombuffer(data, dtype="<u8", count=h, offset=at)
    out = {n: np.empty((h, w), dtype=np.uint16 if t == 1 else np.uint32) for n, t in chans}
    for y in range(h):
        o = int(offsets[y])
        assert o == at + 8 * h + line * y, "a scanline offset"
        assert struct.unpack_from("<ii", data, o) == (y, pixel * w)
        o += 8
        for n, t in chans:
            out[n][y] = np.frombuffer(data, dtype="<u2" if t == 1 else "<u4", count=w, offset=o)
            o += w * (2 if t == 1 else 4)
    return out, chans


def expected_exr(canvas, planes, rgb_type):
    """{channel: bits} the rules of include/rtc.h give for these inputs."""
    out = {}
    if canvas is not None:
        conv = f16_bits if rgb_type == "half" else f32_bits
        for k, n in enumerate("RGB"):
            out[n] = conv(canvas[..., k])
    p = planes or {}
    if "depth" in p:
        out["Z"] = f32_bits(p["depth"])
    for key, pre in (("normal", "N"), ("point", "P")):
        if key in p:
            for k, ax in enumerate("XYZ"):
                out[f"{pre}.{ax}"] = f32_bits(p[key][..., k])
    if "index" in p:
        out["id"] = (p["index"].astype(np.int64) + 1).astype(np.uint32)
    if "shadow" in p:
        out["shadow"] = p["shadow"].astype(np.uint32)
    return out


def check_file(fmt, data, canvas, planes, rgb_type):
    """Decode `data` and compare exactly with the converted inputs."""
    if fmt == "pfm":
        assert np.array_equal(decode_pfm(data), f32_bits(canvas))
    elif fmt == "hdr":
        assert np.array_equal(decode_hdr(data), rgbe_bytes(canvas))
    else:
        got, chans = decode_exr(data)
        want = expected_exr(canvas, planes, rgb_type)
        assert set(got) == set(want) and set(got) <= set(EXR_CHANNELS)
        for n, t in chans:
            assert t == (0 if n in ("id", "shadow") else (1 if rgb_type == "half" else 2) if n in "RGB" else 2), n
            assert got[n].dtype == want[n].dtype and np.array_equal(got[n], want[n]), n
