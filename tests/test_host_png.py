"""The compressed PNG writer of include/rtc.h on the host (rtc_png_format, rtc_png_filter, rtc_canvas_write_png).

The files are checked with zlib and this file's own pieces: an unfilterer, a numpy restatement of the filter choice, a
pure-Python inflater that reports each block (type, code lengths, tokens, bit count), and Python restatements of the match,
lazy-parse, package-merge and block-cost rules. CPU only."""
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest

from _bootstrap import package

rtc = package()
SEG = 32768
CHAIN = 8
GOLDEN = Path(__file__).resolve().parent / "golden"


# ---- file structure ----------------------------------------------------------------------------------------------------
def chunks(png: bytes):
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(png):
        n = struct.unpack(">I", png[at:at + 4])[0]
        typ, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        crc = struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0]
        assert crc == zlib.crc32(typ + data), typ
        out.append((typ, data))
        at += 12 + n
    assert at == len(png)
    return out


def unfilter(raw: bytes, w: int, h: int, c: int) -> np.ndarray:
    row = w * c
    out = np.zeros((h, row), dtype=np.int32)
    a = np.frombuffer(raw, dtype=np.uint8).reshape(h, row + 1)
    for y in range(h):
        t, f = a[y, 0], a[y, 1:].astype(np.int32)
        up = out[y - 1] if y else np.zeros(row, np.int32)
        cur = out[y]
        for x in range(row):
            left = cur[x - c] if x >= c else 0
            ul = up[x - c] if x >= c else 0
            if t == 0:
                p = 0
            elif t == 1:
                p = left
            elif t == 2:
                p = up[x]
            elif t == 3:
                p = (left + up[x]) >> 1
            else:
                pp = left + up[x] - ul
                pa, pb, pc = abs(pp - left), abs(pp - up[x]), abs(pp - ul)
                p = left if pa <= pb and pa <= pc else (up[x] if pb <= pc else ul)
            cur[x] = (f[x] + p) & 255
    return out.astype(np.uint8).reshape(h, w, c)


def decode(png: bytes):
    cs = chunks(png)
    assert cs[0][0] == b"IHDR" and cs[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", cs[0][1])
    assert (depth, comp, filt, inter) == (8, 0, 0, 0) and ctype in (2, 6)
    c = 3 if ctype == 2 else 4
    idat = [d for t, d in cs if t == b"IDAT"]
    assert len(cs) == len(idat) + 2
    raw = zlib.decompress(b"".join(idat))
    assert len(raw) == h * (1 + w * c)
    return unfilter(raw, w, h, c), raw, idat


# ---- a pure-Python inflater that reports the blocks ------------------------------------------------------------------------
class Bits:
    def __init__(self, data: bytes):
        self.v = int.from_bytes(data, "little")
        self.n = 8 * len(data)
        self.pos = 0

    def get(self, k):
        assert self.pos + k <= self.n
        r = (self.v >> self.pos) & ((1 << k) - 1)
        self.pos += k
        return r


def canonical(lens):
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(nxt[l], l)] = s
            nxt[l] += 1
    return table


def read_sym(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.get(1)
        if (code, l) in table:
            return table[(code, l)]
    raise AssertionError("bad code")


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def inflate_blocks(zdata: bytes):
    """Blocks of a zlib stream: dicts of type, final, start/end bit, tokens (int literal or (length, distance)) and, for a
    dynamic block, its code lengths and code-length symbols."""
    assert zdata[:2] == b"\x78\x9c"
    bits = Bits(zdata[2:])
    out = bytearray()
    blocks = []
    while True:
        start = bits.pos
        final, btype = bits.get(1), bits.get(2)
        b = {"final": final, "type": btype, "start": start, "tokens": [], "out0": len(out)}
        if btype == 0:
            bits.pos = (bits.pos + 7) // 8 * 8
            ln, nln = bits.get(16), bits.get(16)
            assert ln ^ nln == 0xffff
            for _ in range(ln):
                out.append(bits.get(8))
        else:
            assert btype in (1, 2)
            if btype == 1:
                lit, dist = FIXED_LIT, [5] * 32
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = bits.get(3)
                clt = canonical(cl)
                seq, rle = [], []
                while len(seq) < hlit + hdist:
                    s = read_sym(bits, clt)
                    if s < 16:
                        seq.append(s)
                        rle.append((s, 0))
                    elif s == 16:
                        r = bits.get(2) + 3
                        seq += [seq[-1]] * r
                        rle.append((16, r))
                    elif s == 17:
                        r = bits.get(3) + 3
                        seq += [0] * r
                        rle.append((17, r))
                    else:
                        r = bits.get(7) + 11
                        seq += [0] * r
                        rle.append((18, r))
                assert len(seq) == hlit + hdist
                lit, dist = seq[:hlit], seq[hlit:]
                b.update(hlit=hlit, hdist=hdist, hclen=hclen, cl=cl, lit=lit, dist=dist, rle=rle)
            lt, dt = canonical(lit), canonical(dist)
            while True:
                s = read_sym(bits, lt)
                if s < 256:
                    out.append(s)
                    b["tokens"].append(s)
                elif s == 256:
                    break
                else:
                    k = s - 257
                    ln = LBASE[k] + bits.get(LEXT[k])
                    dc = read_sym(bits, dt)
                    d = DBASE[dc] + bits.get(DEXT[dc])
                    assert d <= len(out)
                    for _ in range(ln):
                        out.append(out[-d])
                    b["tokens"].append((ln, d))
        b["end"] = bits.pos
        b["out1"] = len(out)
        blocks.append(b)
        if final:
            break
    tail = (bits.pos + 7) // 8
    assert bits.v >> bits.pos & ((1 << (8 * tail - bits.pos)) - 1) == 0  # zero padding
    rest = zdata[2 + tail:]
    assert rest == struct.pack(">I", zlib.adler32(bytes(out)))
    return blocks, bytes(out)


# ---- restatements ------------------------------------------------------------------------------------------------------
def filter_sums(px: np.ndarray):
    """Per row, the five filters' sums of min(v, 256 - v) over the filtered bytes (the choice heuristic of include/rtc.h)."""
    h, w, c = px.shape
    a = px.reshape(h, w * c).astype(np.int32)
    out = []
    for y in range(h):
        cur = a[y]
        up = a[y - 1] if y else np.zeros_like(cur)
        left = np.concatenate([np.zeros(c, np.int32), cur[:-c]])
        ul = np.concatenate([np.zeros(c, np.int32), up[:-c]])
        p = left + up - ul
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        cands = [cur, cur - left, cur - up, cur - ((left + up) >> 1), cur - paeth]
        out.append([int(np.minimum(v & 255, 256 - (v & 255)).sum()) for v in cands])
    return out


def filters_numpy(px: np.ndarray):
    # argmin takes the first of equal sums
    return np.array([int(np.argmin(sums)) for sums in filter_sums(px)], dtype=np.uint8)


def hash3(s, p):
    return ((s[p] << 10) ^ (s[p + 1] << 5) ^ s[p + 2]) & 0x7fff


def lengths_all(s: bytes):
    """L(p) and its distance for every position, by the candidate rules of include/rtc.h."""
    n = len(s)
    chains = {}
    L, D = [0] * (n + 1), [0] * (n + 1)
    for p in range(n):
        if p + 3 > n:
            break
        h = hash3(s, p)
        lst = chains.setdefault(h, [])
        end = min(n, (p // SEG + 1) * SEG)
        cap = min(258, end - p)
        best, bd, seen = 0, 0, 0
        for q in reversed(lst):
            if p - q > 32768 or seen == CHAIN:
                break
            seen += 1
            l = 0
            while l < cap and s[q + l] == s[p + l]:
                l += 1
            if l >= 3 and l > best:
                best, bd = l, p - q
        L[p], D[p] = best, bd
        lst.append(p)
    return L, D


def parse(s, L, D, s0, end):
    toks, p = [], s0
    while p < end:
        if L[p] >= 3 and not (L[p + 1] > L[p]):
            toks.append((L[p], D[p]))
            p += L[p]
        else:
            toks.append(s[p])
            p += 1
    return toks


def len_code(l):
    return max(k for k in range(29) if LBASE[k] <= l)


def dist_code(d):
    return max(k for k in range(30) if DBASE[k] <= d)


def histo(toks):
    lit, dist, extra = [0] * 286, [0] * 30, 0
    for t in toks:
        if isinstance(t, int):
            lit[t] += 1
        else:
            lc, dc = len_code(t[0]), dist_code(t[1])
            lit[257 + lc] += 1
            dist[dc] += 1
            extra += LEXT[lc] + DEXT[dc]
    lit[256] = 1
    return lit, dist, extra


def package_merge(freq, maxbits):
    """The lengths of include/rtc.h's package-merge (same sort and tie rules)."""
    syms = [i for i, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(syms) < 2:
        for i in syms:
            lens[i] = 1
        for i in range(len(freq)):
            if sum(1 for x in lens if x) >= 2:
                break
            if not lens[i]:
                lens[i] = 1
        return lens
    order = sorted(syms, key=lambda i: (freq[i], i))
    m, keep = len(order), 2 * len(order) - 2
    leaves = [freq[i] for i in order]
    cur = leaves[:keep]
    levels = [[True] * len(cur)]
    for _ in range(maxbits - 1):
        pk = [cur[2 * i] + cur[2 * i + 1] for i in range(len(cur) // 2)]
        a = b = 0
        nxt, flags = [], []
        while len(nxt) < keep and (a < m or b < len(pk)):
            if a < m and (b >= len(pk) or leaves[a] <= pk[b]):
                nxt.append(leaves[a]); flags.append(True); a += 1
            else:
                nxt.append(pk[b]); flags.append(False); b += 1
        levels.append(flags)
        cur = nxt
    levels.reverse()   # top first
    take = keep
    for flags in levels:
        nl = sum(flags[:take])
        for i in range(nl):
            lens[order[i]] += 1
        take = 2 * (take - nl)
    return lens


def optimal_cost(freq, maxbits):
    """Textbook package-merge: the least sum of freq * length of a prefix code limited to maxbits (ties do not matter)."""
    w = sorted(f for f in freq if f)
    if len(w) < 2:
        return sum(w)
    lst = list(w)
    for _ in range(maxbits - 1):
        lst = sorted(w + [lst[i] + lst[i + 1] for i in range(0, len(lst) - 1, 2)])
    return sum(lst[:2 * len(w) - 2])


def rle(seq):
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                t = min(r, 138); out.append((18, t)); r -= t
            if r >= 3:
                out.append((17, r)); r = 0
            out += [(0, 0)] * r
        else:
            out.append((v, 0)); r -= 1
            while r >= 3:
                t = min(r, 6); out.append((16, t)); r -= t
            out += [(v, 0)] * r
    return out


def plan(toks, nbytes):
    """(bits as stored, fixed, dynamic; the dynamic code lengths and rle) by include/rtc.h's rules."""
    lit, dist, extra = histo(toks)
    stored = 40 + 8 * nbytes
    fixed = 3 + extra + sum(f * FIXED_LIT[i] for i, f in enumerate(lit)) + 5 * sum(dist)
    ll, dl = package_merge(lit, 15), package_merge(dist, 15)
    hlit = max(257, max(i for i, l in enumerate(ll) if l) + 1)
    hdist = max(1, max(i for i, l in enumerate(dl) if l) + 1)
    r = rle(ll[:hlit] + dl[:hdist])
    clf = [0] * 19
    for s, _ in r:
        clf[s] += 1
    cl = package_merge(clf, 7)
    hclen = max([4] + [i + 1 for i in range(19) if cl[CL_ORDER[i]]])
    xb = {16: 2, 17: 3, 18: 7}
    dyn = 3 + 14 + 3 * hclen + extra + sum(cl[s] + xb.get(s, 0) for s, _ in r)
    dyn += sum(f * ll[i] for i, f in enumerate(lit)) + sum(f * dl[i] for i, f in enumerate(dist))
    return (stored, fixed, dyn), dict(lit=ll[:hlit], dist=dl[:hdist], cl=cl, hclen=hclen, rle=r, litf=lit, distf=dist, clf=clf)


# ---- inputs -------------------------------------------------------------------------------------------------------------
def noise(h, w, c, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def gradient(h, w, c):
    y, x = np.mgrid[0:h, 0:w]
    px = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 7) & 255] + ([np.full_like(x, 200)] if c == 4 else []), -1)
    return px.astype(np.uint8)


def mixed(h=120, w=200, c=3):
    """Flat, gradient and noisy bands: a few segments with every block type and long and short matches."""
    px = gradient(h, w, c)
    px[h // 3:h // 2] = noise(h // 2 - h // 3, w, c, 7)
    px[h // 2:2 * h // 3] = 40
    px[2 * h // 3:, ::7] = noise(h - 2 * h // 3, (w + 6) // 7, c, 9)
    return px


def golden_frames():
    out = []
    for name in ("jamis_100x50", "synthetic100_96x54", "test7_80x60"):
        a = np.load(GOLDEN / f"{name}.npy")
        if a.ndim == 3 and a.shape[2] == 3 and a.dtype != np.uint8:
            a = rtc.color_scale255(a)
        out.append((name, np.ascontiguousarray(a, dtype=np.uint8)))
    return out


def sized_for(nbytes):
    """A frame whose filtered stream is exactly nbytes long: h rows of 1 + w * c bytes (3 channels where they fit, else 4)."""
    for c in (3, 4):
        for h in range(1, 64):
            if nbytes % h == 0 and (nbytes // h - 1) % c == 0 and (nbytes // h - 1) // c <= 65535:
                w = (nbytes // h - 1) // c
                return mixed(h, w, c) if h >= 6 else gradient(h, w, c) ^ noise(h, w, c, nbytes) // 64
    raise AssertionError(f"no frame of {nbytes} filtered bytes")


def roundtrip(px):
    png = rtc.png_encode(px)
    got, raw, _ = decode(png)
    np.testing.assert_array_equal(got, px)
    try:
        from PIL import Image
        import io
        im = np.asarray(Image.open(io.BytesIO(png)))
        np.testing.assert_array_equal(im, px)
    except ImportError:
        pass
    return png, raw


# ---- tests --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 2), (1, 3), (1, 17), (1, 1921), (5, 1), (7, 3), (33, 17)])
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("kind", ["noise", "flat", "gradient"])
def test_roundtrip_sizes(h, w, c, kind):
    px = noise(h, w, c) if kind == "noise" else np.full((h, w, c), 77, np.uint8) if kind == "flat" else gradient(h, w, c)
    roundtrip(px)


@pytest.mark.parametrize("name", ["jamis_100x50", "synthetic100_96x54", "test7_80x60"])
def test_roundtrip_golden(name):
    px = dict(golden_frames())[name]
    png, _ = roundtrip(px)
    assert len(png) < len(rtc.format_png(px))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_roundtrip_segment_boundaries(k, delta):
    px = sized_for(k * SEG + delta)
    png, raw = roundtrip(px)
    assert len(raw) == k * SEG + delta
    idat = [d for t, d in chunks(png) if t == b"IDAT"]
    assert len(idat) == -(-len(raw) // SEG)


def test_roundtrip_rgba_and_rgb_same_pixels():
    px = mixed(40, 50, 4)
    roundtrip(px)
    roundtrip(np.ascontiguousarray(px[..., :3]))


@pytest.mark.parametrize("c", [3, 4])
def test_filter_choice(c):
    for px in (mixed(60, 70, c), noise(9, 31, c), gradient(20, 11, c), np.zeros((3, 5, c), np.uint8)):
        types, filtered = rtc.png_filter(px)
        np.testing.assert_array_equal(types, filters_numpy(px))
        h, w, _ = px.shape
        assert filtered.size == h * (1 + w * c)
        np.testing.assert_array_equal(filtered.reshape(h, -1)[:, 0], types)
        np.testing.assert_array_equal(unfilter(filtered.tobytes(), w, h, c), px)


def check_stream(png: bytes, px: np.ndarray) -> list:
    """The per-segment structure of a compressed PNG of `px`, checked against this file's restatements: one block per
    segment and an empty stored block after each but the last, IDAT chunks on the segment boundaries, each block's type
    the cheapest by plan(), its tokens those of lengths_all / parse, its bit count exact, a dynamic block's code lengths,
    run-length codes and costs those of package-merge within 15 and 7 bits. Returns one dict per segment: the block, its
    tokens and bounds, and the plan's bits and parts."""
    _, raw, idat = decode(png)
    n = len(raw)
    nseg = -(-n // SEG)
    assert len(idat) == nseg
    assert idat[0][:2] == b"\x78\x9c"
    blocks, out = inflate_blocks(b"".join(idat))
    assert out == raw
    _, filtered = rtc.png_filter(px)
    assert filtered.tobytes() == raw
    # one block per segment, each followed by an empty stored block; BFINAL only on the last
    assert len(blocks) == 2 * nseg - 1
    for g in range(nseg):
        b = blocks[2 * g]
        assert (b["out0"], b["out1"]) == (g * SEG, min(n, (g + 1) * SEG))
        assert b["final"] == (g == nseg - 1)
        if g + 1 < nseg:
            f = blocks[2 * g + 1]
            assert (f["type"], f["final"], f["out0"], f["out1"]) == (0, 0, b["out1"], b["out1"])
    # each IDAT chunk is its segment's bytes: the chunk boundaries fall on the segment boundaries
    at = 0
    for g, d in enumerate(idat):
        at += len(d)
        if g + 1 < nseg:
            assert blocks[2 * g + 1]["end"] == 8 * (at - 2)
    L, D = lengths_all(raw)
    segs = []
    for g in range(nseg):
        b = blocks[2 * g]
        s0, end = g * SEG, min(n, (g + 1) * SEG)
        toks = parse(raw, L, D, s0, end)
        bits, pl = plan(toks, end - s0)
        segs.append({"block": b, "s0": s0, "end": end, "toks": toks, "bits": bits, "plan": pl, "L": L, "D": D, "raw": raw})
        best = min(range(3), key=lambda t: (bits[t], t))
        assert b["type"] == best, (g, bits)
        if b["type"] == 0:
            assert b["end"] - b["start"] - ((-(b["start"] + 3)) % 8) == bits[0] - ((-(b["start"] + 3)) % 8)
            continue
        assert b["tokens"] == toks
        pos = s0
        for t in b["tokens"]:
            if not isinstance(t, int):
                assert 1 <= t[1] <= 32768 and pos + t[0] <= end   # no match crosses its segment
                pos += t[0]
            else:
                pos += 1
        assert b["end"] - b["start"] == bits[b["type"]]
        if b["type"] == 2:
            assert b["lit"] == pl["lit"] and b["dist"] == pl["dist"] and b["cl"] == pl["cl"] and b["hclen"] == pl["hclen"]
            assert b["rle"] == [(s, r if s >= 16 else 0) for s, r in pl["rle"]]
            assert max(b["lit"] + b["dist"]) <= 15 and max(b["cl"]) <= 7
            lit, dist = pl["litf"], pl["distf"]
            assert sum(f * l for f, l in zip(lit, b["lit"] + [0] * 286)) == optimal_cost(lit, 15)
            if sum(1 for f in dist if f) >= 2:
                assert sum(f * l for f, l in zip(dist, b["dist"] + [0] * 30)) == optimal_cost(dist, 15)
            if sum(1 for f in pl["clf"] if f) >= 2:
                assert sum(f * l for f, l in zip(pl["clf"], b["cl"])) == optimal_cost(pl["clf"], 7)
    return segs


@pytest.mark.parametrize("px", [mixed(), mixed(90, 130, 4), gradient(100, 150, 3)], ids=["mixed", "mixed4", "gradient"])
def test_stream_structure(px):
    segs = check_stream(rtc.png_encode(px), px)
    assert any(s["block"]["type"] != 0 for s in segs), "no compressed block to check"


def test_package_merge_limits():
    """A Fibonacci-like histogram whose Huffman code would need more than 15 bits: the limit holds, the cost is optimal."""
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    lens = package_merge(fib + [0] * 256, 15)
    assert max(lens) == 15
    assert sum(f * l for f, l in zip(fib, lens)) == optimal_cost(fib, 15)


@pytest.mark.parametrize("shape", [(64, 64, 3), (200, 300, 3), (100, 250, 4), (1, 1921, 3)])
def test_noise_bound(shape):
    px = noise(*shape, seed=sum(shape))
    png = rtc.png_encode(px)
    n = shape[0] * (1 + shape[1] * shape[2])
    nseg = -(-n // SEG)
    assert len(png) <= n + 22 * nseg + 51
    blocks, _ = inflate_blocks(b"".join(d for t, d in chunks(png) if t == b"IDAT"))
    assert all(b["type"] == 0 for b in blocks)


def test_flat_frame_compresses():
    px = np.zeros((300, 400, 3), np.uint8)
    png, _ = roundtrip(px)
    assert len(png) < 2000


def test_write_png_deflate(tmp_path):
    px = mixed(30, 40, 3)
    p = tmp_path / "x.png"
    rtc.write_png_deflate(p, px)
    assert p.read_bytes() == rtc.png_encode(px)


def test_errors(tmp_path):
    with pytest.raises(rtc.RtcError):
        rtc.write_png_deflate(tmp_path / "no" / "such" / "dir.png", np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(ValueError):
        rtc.png_encode(np.zeros((2, 2, 2), np.uint8))
    with pytest.raises(rtc.RtcError):
        rtc.png_encode(np.zeros((1, 65536, 3), np.uint8))
    with pytest.raises(rtc.RtcError):
        rtc.png_filter(np.zeros((0, 5, 3), np.uint8))
    import ctypes as C
    P8 = C.POINTER(C.c_uint8)
    a = np.zeros((4, 4, 3), np.uint8)
    assert rtc.lib().rtc_png_format(a.ctypes.data_as(P8), 4, 4, 2, None, 0) == 0
    assert rtc.lib().rtc_png_format(a.ctypes.data_as(P8), 0, 4, 3, None, 0) == 0
    assert rtc.lib().rtc_png_format(None, 4, 4, 3, None, 0) == 0
    assert rtc.lib().rtc_canvas_write_png(None, a.ctypes.data_as(P8), 4, 4, 3) != 0


def test_stored_writer_unchanged():
    """format_png stays the stored writer: filter 0 on every row, stored blocks."""
    px = mixed(20, 30, 3)
    _, raw, idat = decode(rtc.format_png(px))
    assert all(raw[y * (1 + 90)] == 0 for y in range(20))
    assert idat[0][:2] == b"\x78\x01"
