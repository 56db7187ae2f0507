"""Boundary cases of the four GPU file writers (helper module, not collected): deterministic, seeded frames placed on the
decisions of the PNG, JPEG, GIF and packed-format writers that rendered frames, noise and flat frames never reach. Each case
has a name, the branch it targets, the entries it goes through and a predicate that proves, from a file's bytes, that the
branch is taken. The predicates use the host suites' restatements (test_host_png, test_host_jpeg, test_host_gif,
test_host_image_formats) and the numpy median cut below; test_host_encoder_cases asserts them on the host statement and
test_gpu_encoder_cases on the device's file.

PNG (rtc.png_encode, PngEncoder, ImageEncoder "png"; "ico" where the frame fits 256 x 256)
  png_lit_limit          the literal/length code needs more than 15 bits unlimited: a dynamic block whose longest code is 15
  png_dist_limit         the same for the distance code
  png_cl_limit           the code-length code needs more than 7 bits unlimited: its longest code is 7
  png_match_258          a copy longer than 258 bytes: a match of exactly 258
  png_match_cut          a copy running over the end of segment 0: the match is cut at the segment's end
  png_dist_32768         candidates at distance 32768 (taken) and 32769 (out of the window)
  png_chain_9th          the longest candidate is 9th in the hash chain (RTC_PNG_CHAIN = 8): not used
  png_hash_alias         triples that share a hash but not their bytes (bytes >= 32 alias) fill the chain
  png_lazy_run           L[p+1] > L[p] several positions in a row: a run of lazy deferrals
  png_fixed_wins         a short segment whose fixed block is the cheapest
  png_dynamic_no_match   a dynamic block without a match: the distance code of the "fewer than two symbols" rule
  png_last_one_byte      a last segment of one byte
  png_filter_ties        Sub, Up, Average and Paeth tie on the sum heuristic (the lowest type wins) and Paeth's pa == pb
JPEG (rtc.jpeg_encode, JpegEncoder, ImageEncoder "jpeg")
  jpeg_groups_1026       4104 x 4096: 1026 groups of 256 MCUs, a second iteration of k_jpeg_group_scan (its carry)
  jpeg_groups_4100       8200 x 8192: 4100 groups, five iterations, the last one partial
  jpeg_dc_cat11          quality 100, flat black and white blocks alternating: DC differences of category 11, both signs
  jpeg_ac_cat10          quality 100, a one-pixel checkerboard: AC coefficients of category 10
  jpeg_zz63_only         quality 100, a block whose only non-zero AC is at zigzag 63: three ZRLs and no EOB
  jpeg_zrl16             quality 100, a run of exactly 16 zeros before a coefficient (ZRL, then run 0)
  jpeg_ff_chunk_end      a 0xFF data byte that is the last byte of a 4096-byte CHUNK: its stuffed 0x00 opens the next
  jpeg_ff_last           the last data byte before the padding is 0xFF
GIF (rtc.gif_encode, GifWriter.append_device, ImageEncoder "gif")
  gif_256_colours        exactly 256 distinct colours: the exact palette
  gif_257_colours        257 distinct colours: the smallest median-cut frame
  gif_one_bin            257+ colours in one bin: one box, every other entry black
  gif_early_stop         300+ colours in 12 bins: the cut stops at 12 boxes
  gif_box_tie            two splittable boxes of equal pixel counts (the lower number splits), 2 * cum == n exactly
  gif_axis_tie           r and g of equal extent (r is cut), and b of equal extent to g (g is cut)
  gif_cut_fallback       the last plane holds most pixels: the cut falls back to hi - 1
  gif_equidistant        pixels equidistant from two palette entries: the lower index
  gif_dict_fill_last     the dictionary fills exactly on a segment's last index
  gif_subblock_*         packed LZW data of 255k - 1, 255k and 255k + 1 bytes
Packed (ImageEncoder "bmp", "tga", "tiff", "farbfeld", "pam", "ppm")
  packed_w8 .. packed_w11  widths with w * 3 % 4 = 0, 1, 2, 3
  packed_len_*           file lengths of 16k - 1, 16k and 16k + 1 (k_image_pack writes 16-byte stores), in the formats whose
                         layout reaches them (farbfeld, PAM, PPM; BMP, TGA and TIFF files never end on these lengths)
"""
import heapq
import io
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_host_png as HP  # noqa: E402
import test_host_jpeg as HJ  # noqa: E402
import test_host_gif as HG  # noqa: E402
from _bootstrap import package  # noqa: E402

rtc = package()
SEG = HP.SEG
CHUNK = 4096              # rtc_jpeg.hip: bytes of packed data per workgroup of k_jpeg_ffcount / k_jpeg_scatter
MCU_PER_GROUP = 256       # rtc_jpeg.hip: k_jpeg_mcu_scan
PACKED = ("bmp", "tga", "tiff", "farbfeld", "pam", "ppm")


@dataclass
class Case:
    name: str
    kind: str                      # "png", "jpeg", "gif" or "packed"
    branch: str
    make: Callable[[], np.ndarray]
    check: Callable[[np.ndarray, bytes], None]   # the predicate, on the pixels and a file of the case's kind
    entries: tuple = ()
    quality: int = 75
    formats: tuple = ()            # packed: the formats the case runs through
    _px: np.ndarray = field(default=None, repr=False)

    def pixels(self) -> np.ndarray:
        if self._px is None:
            self._px = np.ascontiguousarray(self.make(), dtype=np.uint8)
        return self._px

    def host(self, entry: str = None) -> bytes:
        px = self.pixels()
        if self.kind == "png":
            return rtc.png_encode(px)
        if self.kind == "jpeg":
            return rtc.jpeg_encode(px, self.quality)
        if self.kind == "gif":
            return rtc.gif_encode([px])
        return rtc.image_encode(entry, px)


# ---- shared pieces ------------------------------------------------------------------------------------------------------
def huffman_depth(freq) -> int:
    """The longest code of an unlimited Huffman code of the used symbols (plain heap build)."""
    h = [(f, i, 0) for i, f in enumerate(freq) if f]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    k = len(freq)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        k += 1
        heapq.heappush(h, (a[0] + b[0], k, max(a[2], b[2]) + 1))
    return h[0][2]


def fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


# ---- PNG ------------------------------------------------------------------------------------------------------------------
# Every PNG case but the filter ties and the one-byte segment is one row of 3-channel pixels whose None filter wins (checked
# by the predicate), so the filtered stream is the type byte 0 and then the row: the cases set that stream directly. Its
# material is bytes of small filter cost (-32..31, or -64..63) in an order where no 3-byte string occurs twice (no_repeat,
# Stream), so the only matches are the copies placed in it.
CHEAP = [v & 255 for v in range(-32, 32)]
WIDE = [v & 255 for v in range(-64, 64)]   # fewer chance repeats where a stream holds many copies


def no_repeat(n, rng, alphabet=CHEAP, counts=None):
    """n bytes (or the multiset `counts`) in an order where no 3-byte string occurs twice, where the shuffle allows it."""
    if counts is None:
        s = [int(x) for x in rng.choice(np.array(alphabet), n)]
    else:
        s = [b for b, c in sorted(counts.items()) for _ in range(c)]
        s = [int(x) for x in rng.permutation(np.array(s, dtype=np.int64))]
    seen = set()
    for i in range(2, len(s)):
        for _ in range(64):
            if (s[i - 2], s[i - 1], s[i]) not in seen:
                break
            if counts is None:
                s[i] = int(rng.choice(alphabet))
            else:
                j = int(rng.integers(i, len(s)))
                s[i], s[j] = s[j], s[i]
        seen.add((s[i - 2], s[i - 1], s[i]))
    return s


def row_frame(stream) -> np.ndarray:
    """The one-row RGB frame whose None-filtered stream is `stream` (its first byte, the type byte, is 0; the rest is cut
    to a multiple of 3)."""
    assert stream[0] == 0
    n = (len(stream) - 1) // 3 * 3
    return np.array(stream[1:1 + n], dtype=np.uint8).reshape(1, n // 3, 3)


def none_filtered(px):
    types, _ = rtc.png_filter(px)
    assert not types.any(), f"the stream was built for the None filter, got {types}"


def token_positions(seg):
    pos, out = seg["s0"], {}
    for t in seg["toks"]:
        out[pos] = t
        pos += 1 if isinstance(t, int) else t[0]
    return out


def make_lit_limit():
    rng = np.random.default_rng(101)
    counts = {b: 300 for b in CHEAP}
    for b, c in zip(range(96, 108), fib(13)[1:]):   # 1, 2, 3, 5, ... with the end-of-block's 1: a Fibonacci tail
        counts[b] = c
    counts[0] -= 1   # the filter type byte
    return row_frame([0] + no_repeat(0, rng, counts=counts))


def check_lit_limit(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    assert len(segs) == 1
    s = segs[0]
    assert s["block"]["type"] == 2
    assert huffman_depth(s["plan"]["litf"]) > 15
    assert max(s["block"]["lit"]) == 15
    assert sum(f * l for f, l in zip(s["plan"]["litf"], s["block"]["lit"])) == HP.optimal_cost(s["plan"]["litf"], 15)


class Stream:
    """A filtered stream built left to right in which every 3-byte string holding a fresh byte is new, so that the only
    matches are the copies placed on purpose."""

    def __init__(self, rng, alphabet=WIDE):
        self.s, self.seen, self.rng, self.alphabet = [0], set(), rng, alphabet

    def _add(self, b):
        self.s.append(b)
        if len(self.s) >= 3:
            self.seen.add(tuple(self.s[-3:]))

    def fresh(self, ahead=(), avoid=()):
        """One byte that makes no 3-byte string seen before, with the `ahead` bytes that will follow it."""
        for b in self.rng.permutation(self.alphabet):
            b = int(b)
            t = self.s[-2:] + [b] + list(ahead[:2])
            grams = [tuple(t[i:i + 3]) for i in range(len(t) - 2)]
            if b not in avoid and not any(g in self.seen for g in grams) and len(set(grams)) == len(grams):
                self._add(b)
                return
        raise AssertionError("no fresh byte")

    def copy(self, d, n):
        for _ in range(n):
            self._add(self.s[-d])


def make_dist_limit():
    """Distance codes 0..16 with Fibonacci counts. A code of distance d >= 5 gets zones of d bytes: the first fresh, each
    next one a gap byte and then, every 4 bytes, 3 bytes equal to the zone before's (a match of exactly 3 at distance d)
    and a fresh gap byte."""
    counts = fib(17)
    st = Stream(np.random.default_rng(102))
    for _ in range(8):
        st.fresh()
    for c in range(4):   # d = 1..4: d fresh bytes, a copy of 3, a fresh byte unlike the one d back
        d = HP.DBASE[c]
        for _ in range(counts[c]):
            for _ in range(d):
                st.fresh()
            st.copy(d, 3)
            st.fresh(avoid=(st.s[-d],))
            for _ in range(4):
                st.fresh()
    for c in range(4, 17):
        d, left = HP.DBASE[c], counts[c]
        per = (d - 1) // 4
        z0 = len(st.s)
        for _ in range(d):
            st.fresh()
        while left:
            zs = len(st.s)
            k = min(per, left)
            for o in range(d):
                src = zs + o - d
                if 1 <= o <= 4 * k and o % 4 != 0:
                    st._add(st.s[src])
                else:
                    nxt = st.s[src + 1:src + 3] if o + 1 <= 4 * k and (o + 1) % 4 == 1 else []
                    st.fresh(ahead=nxt, avoid=(st.s[src],))
            left -= k
        assert z0 < len(st.s)
    assert len(st.s) < SEG
    return row_frame(st.s)


def check_dist_limit(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    assert len(segs) == 1
    s = segs[0]
    assert s["block"]["type"] == 2
    assert huffman_depth(s["plan"]["distf"]) > 15
    assert max(s["block"]["dist"]) == 15
    assert sum(f * l for f, l in zip(s["plan"]["distf"], s["block"]["dist"])) == HP.optimal_cost(s["plan"]["distf"], 15)


def make_cl_limit():
    """Literal counts in nine levels of T * 2^-l (a staircase found by a seeded search): the lengths' run-length symbols
    come out in a spread that needs an 8-bit code-length code."""
    rng = np.random.default_rng(93)
    cheap = sorted(CHEAP, key=lambda b: min(b, 256 - b))
    others = list(range(32, 224))
    rng.shuffle(others)
    sizes = sorted((int(x) for x in rng.integers(1, 40, 9)), reverse=True)
    counts, pool, i = {}, cheap + others, 0
    for g, n in enumerate(sizes):
        for _ in range(n):
            counts[pool[i]] = max(1, int(24000 * 2.0 ** -(6 + g)))
            i += 1
    counts[0] -= 1
    return row_frame([0] + no_repeat(0, np.random.default_rng(7), counts=counts))


def check_cl_limit(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    assert len(segs) == 1
    s = segs[0]
    assert s["block"]["type"] == 2
    assert huffman_depth(s["plan"]["clf"]) > 7
    assert max(s["block"]["cl"]) == 7
    assert sum(f * l for f, l in zip(s["plan"]["clf"], s["block"]["cl"])) == HP.optimal_cost(s["plan"]["clf"], 7)


def make_match_258():
    s = [0] + no_repeat(3000, np.random.default_rng(103))
    s[2000:2600] = s[1000:1600]
    return row_frame(s)


def check_match_258(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    at = token_positions(segs[0])
    assert at[2000] == (258, 1000) and at[2258] == (258, 1000) and at[2516] == (84, 1000)


def make_match_cut():
    s = [0] + no_repeat(SEG + 600, np.random.default_rng(104))
    s[SEG - 100:SEG + 200] = s[SEG - 5100:SEG - 4800]
    return row_frame(s)


def check_match_cut(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    assert len(segs) == 2
    at = token_positions(segs[0])
    assert at[SEG - 100] == (100, 5000)          # would run on for 200 more bytes
    assert segs[0]["raw"][SEG] == segs[0]["raw"][SEG - 5000]
    assert token_positions(segs[1])[SEG] == (200, 5000)


def make_dist_32768():
    s = [0] + no_repeat(SEG + 1200, np.random.default_rng(105))
    s[100 + SEG:110 + SEG] = s[100:110]       # distance 32768: inside the window
    s[300 + SEG + 1:310 + SEG + 1] = s[300:310]   # distance 32769: outside
    return row_frame(s)


def check_dist_32768(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    assert len(segs) == 2
    at = token_positions(segs[1])
    assert at[100 + SEG] == (10, 32768)
    p = 300 + SEG + 1
    L, D, raw = segs[1]["L"], segs[1]["D"], segs[1]["raw"]
    assert raw[p:p + 10] == raw[300:310]
    assert L[p] < 10 and D[p] != 32769      # the 10 bytes 32769 back are not a candidate


def make_chain_9th():
    rng = np.random.default_rng(106)
    s = [0] + no_repeat(6000, rng)
    p = 5000
    # the string at p: 3 bytes shared with eight nearer sources, 24 with the farthest
    s[1000:1024] = s[p:p + 24]
    for k in range(8):
        q = 2000 + 300 * k
        s[q:q + 3] = s[p:p + 3]
        s[q + 3] = s[p + 3] ^ 1   # a different 4th byte: length exactly 3
    for q in [1000] + [2000 + 300 * k for k in range(8)]:
        s[q - 1] = s[p - 1] ^ 2    # and a different byte before: no match at p - 1
    return row_frame(s)


def check_chain_9th(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    L, D, raw = segs[0]["L"], segs[0]["D"], segs[0]["raw"]
    p = 5000
    assert (L[p], D[p]) == (3, p - 4100)             # the nearest of the eight
    assert raw[p:p + 24] == raw[1000:1024]            # ... while the 9th gives 24 bytes
    at = token_positions(segs[0])
    assert isinstance(at[p], int) and at[p + 1] == (23, p - 1000)   # lazy: the next position's match is longer


def make_hash_alias():
    rng = np.random.default_rng(107)
    s = [0] + no_repeat(4000, rng)
    # (x, y, z) and (x + 32 k, y, z) share a hash. A: one alias between the source and p; B: eight aliases fill the chain.
    pa, pb = 3000, 3500
    x, y, z = 5, s[pa + 1], s[pa + 2]
    s[pa] = x
    s[1000:1003] = [x, y, z]
    s[2000:2003] = [x + 32, y, z]
    xb, yb, zb = 9, s[pb + 1], s[pb + 2]
    s[pb] = xb
    s[1200:1203] = [xb, yb, zb]
    for k in range(8):
        s[2200 + 100 * k:2203 + 100 * k] = [(xb + 32 * (1 + k % 7)) & 255, yb, zb]
    return row_frame(s)


def check_hash_alias(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    L, D, raw = segs[0]["L"], segs[0]["D"], segs[0]["raw"]
    assert HP.hash3(raw, 2000) == HP.hash3(raw, 3000) and raw[2000] != raw[3000]
    assert L[3000] >= 3 and D[3000] == 2000
    assert raw[3500:3503] == raw[1200:1203]
    assert all(HP.hash3(raw, 2200 + 100 * k) == HP.hash3(raw, 3500) and raw[2200 + 100 * k] != raw[3500] for k in range(8))
    assert L[3500] == 0                              # the real source is 9th behind eight aliases


def make_lazy_run():
    rng = np.random.default_rng(108)
    s = [0] + no_repeat(4000, rng)
    p = 3000
    for j in range(5):   # source j: 3 + j bytes of the string at p + j
        q = 500 + 200 * j
        s[q:q + 3 + j] = s[p + j:p + 3 + 2 * j]
    return row_frame(s)


def check_lazy_run(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    L = segs[0]["L"]
    p = 3000
    assert [L[p + j] for j in range(5)] == [3, 4, 5, 6, 7]
    at = token_positions(segs[0])
    assert all(isinstance(at[p + j], int) for j in range(4)) and at[p + 4] == (7, p + 4 - 1300)


def make_fixed_wins():
    s = [0] + no_repeat(90, np.random.default_rng(109))
    s[60:80] = s[10:30]
    return row_frame(s)


def check_fixed_wins(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    s = segs[0]
    assert s["block"]["type"] == 1 and s["bits"][1] < min(s["bits"][0], s["bits"][2])
    assert any(not isinstance(t, int) for t in s["toks"])


def make_dynamic_no_match():
    st = Stream(np.random.default_rng(110), sorted(CHEAP, key=lambda b: min(b, 256 - b))[:24])
    for _ in range(2000):
        st.fresh()
    return row_frame(st.s)


def check_dynamic_no_match(px, png):
    none_filtered(px)
    segs = HP.check_stream(png, px)
    s = segs[0]
    assert s["block"]["type"] == 2 and all(isinstance(t, int) for t in s["toks"])
    assert s["block"]["dist"] == [1, 1]   # no distance used: symbols 0 and 1 get length 1


def make_last_one_byte():
    return HP.sized_for(SEG + 1)


def check_last_one_byte(px, png):
    segs = HP.check_stream(png, px)
    assert len(segs) == 2 and segs[1]["end"] - segs[1]["s0"] == 1


def make_filter_ties():
    y, x = np.mgrid[0:2, 0:20]
    v = 3 * (x + y)          # row 1 = row 0 + 3: Sub, Up, Average and Paeth all leave 3 per byte
    px = np.repeat(v[..., None], 3, axis=2)
    return np.concatenate([px, np.full((2, 20, 3), 50)], axis=0)   # and rows that None and Up tie on (up = the row itself)


def check_filter_ties(px, png):
    sums = HP.filter_sums(px)
    types, _ = rtc.png_filter(px)
    assert list(types) == list(HP.filters_numpy(px))
    assert sums[1][1] == sums[1][2] == sums[1][3] == sums[1][4] < sums[1][0] and types[1] == 1
    assert sums[3][2] == sums[3][4] == 0 and types[3] == 2       # Up and Paeth: 0 (Paeth's pa = pb there: up)
    got, _, _ = HP.decode(png)
    assert np.array_equal(got, px)
    HP.check_stream(png, px)


def png_cases():
    spec = [
        ("png_lit_limit", "rtc_png_huff_lengths limits the literal/length code to 15 bits", make_lit_limit, check_lit_limit),
        ("png_dist_limit", "rtc_png_huff_lengths limits the distance code to 15 bits", make_dist_limit, check_dist_limit),
        ("png_cl_limit", "rtc_png_huff_lengths limits the code-length code to 7 bits", make_cl_limit, check_cl_limit),
        ("png_match_258", "rtc_png_match caps a match at 258", make_match_258, check_match_258),
        ("png_match_cut", "rtc_png_match caps a match at its segment's end", make_match_cut, check_match_cut),
        ("png_dist_32768", "the window: 32768 is in, 32769 is out", make_dist_32768, check_dist_32768),
        ("png_chain_9th", "RTC_PNG_CHAIN: the 9th candidate is not looked at", make_chain_9th, check_chain_9th),
        ("png_hash_alias", "aliased hashes: candidates of length 0 fill the chain", make_hash_alias, check_hash_alias),
        ("png_lazy_run", "rtc_png_takes_match defers four times in a row", make_lazy_run, check_lazy_run),
        ("png_fixed_wins", "rtc_png_plan: fixed is the cheapest", make_fixed_wins, check_fixed_wins),
        ("png_dynamic_no_match", "rtc_png_plan: dynamic without a match, distance lengths of the < 2 symbols rule",
         make_dynamic_no_match, check_dynamic_no_match),
        ("png_last_one_byte", "a last segment of one byte", make_last_one_byte, check_last_one_byte),
        ("png_filter_ties", "k_png_filter / rtc_png_filter: equal sums go to the lowest type", make_filter_ties, check_filter_ties),
    ]
    out = []
    for name, branch, make, check in spec:
        c = Case(name, "png", branch, make, check)
        h, w = c.pixels().shape[:2]
        c.entries = ("png_encode", "PngEncoder", "image:png") + (("image:ico",) if max(h, w) <= 256 else ())
        out.append(c)
    return out


# ---- JPEG -----------------------------------------------------------------------------------------------------------------
def jpeg_groups(w, h):
    return -(-(((w + 7) // 8) * ((h + 7) // 8)) // MCU_PER_GROUP)


def jpeg_data(b: bytes) -> bytes:
    """The entropy-coded data of a JPEG with its stuffing removed (test_host_jpeg's reader)."""
    return HJ.BitReader(HJ.parse_jpeg(b)["data"]).bytes


def sof_size(b: bytes):
    sof = HJ.parse_jpeg(b)["sof"]
    return int.from_bytes(sof[3:5], "big"), int.from_bytes(sof[1:3], "big")


def smooth_tile_frame(h, w, seed):
    """A large frame cheaply: a smooth 72 x 88 tile with mild noise, repeated (blocks differ: the tile is not 8-aligned)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:72, 0:88]
    t = np.stack([x * 2 + y, 200 - y * 2, (x * y) // 40], -1) + rng.integers(0, 12, (72, 88, 3))
    t = np.clip(t, 0, 255).astype(np.uint8)
    return np.tile(t, (-(-h // 72), -(-w // 88), 1))[:h, :w]


def check_jpeg_decodes(px, b, psnr_min):
    """The file's size, and PIL's decode within `psnr_min` dB of the pixels."""
    w, h = sof_size(b)
    assert (h, w) == px.shape[:2]
    from PIL import Image
    im = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    assert HJ.psnr(im, px[..., :3]) >= psnr_min


def jpeg_groups_case(name, w, h, groups, seed):
    def check(px, b):
        assert jpeg_groups(*sof_size(b)) == groups
        check_jpeg_decodes(px, b, 30.0)
    return Case(name, "jpeg", f"k_jpeg_group_scan: {groups} groups, {-(-groups // 1024)} iterations of 1024",
                lambda: smooth_tile_frame(h, w, seed), check)


def check_coefficients(px, b, quality):
    """The own coefficient decoder reads the file back to rtc.jpeg_coefficients; returns them."""
    co = HJ.decode_coefficients(b)
    assert np.array_equal(co, rtc.jpeg_coefficients(px, quality))
    return co


def make_dc_cat11():
    blocks = (np.arange(8) % 2 * 255).astype(np.uint8)   # black, white, black, ... blocks in raster order
    px = np.repeat(np.repeat(blocks.reshape(1, 8), 8, 0), 8, 1)
    return np.repeat(np.concatenate([px, px[:, ::-1]], 0)[..., None], 3, axis=2)


def check_dc_cat11(px, b):
    co = check_coefficients(px, b, 100)
    dc = co[:, 0, 0].astype(np.int64)
    diff = np.diff(np.concatenate([[0], dc]))
    cats = [int(abs(v)).bit_length() for v in diff]
    assert 11 in [c for c, v in zip(cats, diff) if v > 0] and 11 in [c for c, v in zip(cats, diff) if v < 0]


def make_ac_cat10():
    y, x = np.mgrid[0:16, 0:16]
    return np.repeat((((x + y) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)


def check_ac_cat10(px, b):
    co = check_coefficients(px, b, 100)
    assert max(int(abs(int(v))).bit_length() for v in co[:, :, 1:].ravel()) == 10


def make_zz63_only():
    x = np.arange(8)
    c7 = np.cos((2 * x + 1) * 7 * np.pi / 16)
    blk = np.clip(np.round(128 + 1.25 * np.outer(c7, c7)), 0, 255).astype(np.uint8)   # found by a search over the amplitude
    return np.repeat(np.concatenate([blk, np.full((8, 8), 90, np.uint8)], 1)[..., None], 3, axis=2)


def check_zz63_only(px, b):
    co = check_coefficients(px, b, 100)
    zz = co[0, 0][HJ.ZIGZAG]
    assert [k for k in range(1, 64) if zz[k]] == [63] and not co[0, 1:, 1:].any()


def make_zrl16():
    rng = np.random.default_rng(18)
    x = np.arange(8)
    out = []
    for _ in range(16):
        a, us = rng.normal(0, 30, 4), rng.integers(0, 8, (4, 2))
        blk = 128 + sum(a[i] * np.outer(np.cos((2 * x + 1) * us[i, 0] * np.pi / 16), np.cos((2 * x + 1) * us[i, 1] * np.pi / 16))
                        for i in range(4))
        out.append(np.clip(np.round(blk), 0, 255).astype(np.uint8))
    return np.repeat(np.concatenate(out, 1)[..., None], 3, axis=2)


def zero_runs(zz):
    """The lengths of the runs of zeros that end in a non-zero AC coefficient."""
    out, run = [], 0
    for k in range(1, 64):
        if zz[k] == 0:
            run += 1
        else:
            out.append(run)
            run = 0
    return out


def check_zrl16(px, b):
    co = check_coefficients(px, b, 100)
    assert any(16 in zero_runs(blk[HJ.ZIGZAG]) for blk in co[:, 0])


def search_frame(shape, quality, want, seeds=range(2000)):
    for seed in seeds:
        px = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
        if want(jpeg_data(rtc.jpeg_encode(px, quality))):
            return seed
    raise AssertionError("no frame found")


def ff_at_chunk_end(d):
    return any(d[k - 1] == 0xFF for k in range(CHUNK, len(d) + 1, CHUNK))


FF_CHUNK_SEED = 17  # search_frame((48, 64, 3), 100, ff_at_chunk_end): the first seed
FF_LAST_SEED = 9    # search_frame((16, 16, 3), 100, lambda d: d[-1] == 0xFF)


def check_ff_chunk_end(px, b):
    check_coefficients(px, b, 100)
    assert ff_at_chunk_end(jpeg_data(b))


def check_ff_last(px, b):
    check_coefficients(px, b, 100)
    assert jpeg_data(b)[-1] == 0xFF and HJ.parse_jpeg(b)["data"][-2:] == b"\xff\x00"


def jpeg_cases(large=True):
    out = []
    if large:
        out += [jpeg_groups_case("jpeg_groups_1026", 4104, 4096, 1026, 1), jpeg_groups_case("jpeg_groups_4100", 8200, 8192, 4100, 2)]
    spec = [
        ("jpeg_dc_cat11", "a DC difference of category 11, both signs", make_dc_cat11, check_dc_cat11),
        ("jpeg_ac_cat10", "AC coefficients of category 10", make_ac_cat10, check_ac_cat10),
        ("jpeg_zz63_only", "the only AC at zigzag 63: three ZRLs, no EOB", make_zz63_only, check_zz63_only),
        ("jpeg_zrl16", "a run of exactly 16 zeros: a ZRL, then run 0", make_zrl16, check_zrl16),
        ("jpeg_ff_chunk_end", "0xFF as the last byte of a 4096-byte chunk of packed data",
         lambda: np.random.default_rng(FF_CHUNK_SEED).integers(0, 256, (48, 64, 3), dtype=np.uint8), check_ff_chunk_end),
        ("jpeg_ff_last", "0xFF as the last data byte, padding included",
         lambda: np.random.default_rng(FF_LAST_SEED).integers(0, 256, (16, 16, 3), dtype=np.uint8), check_ff_last),
    ]
    out += [Case(n, "jpeg", br, mk, ck, quality=100) for n, br, mk, ck in spec]
    for c in out:
        c.entries = ("jpeg_encode", "JpegEncoder", "image:jpeg") if c.quality == 75 else ("jpeg_encode", "JpegEncoder")
    return out


# ---- GIF ------------------------------------------------------------------------------------------------------------------
def median_cut_np(frame):
    """include/rtc.h's quantiser palette in numpy: the exact palette, or the median cut over the 32768 bins (box choice,
    axis, cut plane and rounded means); (palette (256, 3), entries used, events). The events name the tie and edge rules
    the cut met: box_tie, axis_tie, half (2 * cum == n), fallback (hi - 1), stop (fewer than 256 boxes)."""
    px = frame.reshape(-1, 3).astype(np.int64)
    pal = np.zeros((256, 3), np.int64)
    events = {}
    colours = np.unique(px[:, 0] << 16 | px[:, 1] << 8 | px[:, 2])
    if len(colours) <= 256:
        pal[:len(colours)] = np.stack([colours >> 16, (colours >> 8) & 255, colours & 255], -1)
        return pal.astype(np.uint8), len(colours), events
    bins = (px[:, 0] >> 3) << 10 | (px[:, 1] >> 3) << 5 | (px[:, 2] >> 3)
    cnt = np.bincount(bins, minlength=32768)
    sums = np.stack([np.bincount(bins, weights=px[:, c], minlength=32768) for c in range(3)], -1).astype(np.int64)
    occ = np.nonzero(cnt)[0]
    coord = np.stack([(occ >> 10) & 31, (occ >> 5) & 31, occ & 31], -1)
    owner = np.zeros(len(occ), np.int64)
    nb = 1
    while nb < 256:
        boxes = []
        for i in range(nb):
            sel = owner == i
            boxes.append((coord[sel].min(0), coord[sel].max(0), int(cnt[occ[sel]].sum())))
        split = [i for i, (lo, hi, n) in enumerate(boxes) if (hi > lo).any()]
        if not split:
            events["stop"] = nb
            break
        nmax = max(boxes[i][2] for i in split)
        tied = [i for i in split if boxes[i][2] == nmax]
        best = tied[0]
        if len(tied) > 1:
            events.setdefault("box_tie", []).append(tuple(tied))
        lo, hi, n = boxes[best]
        ext = hi - lo
        axis = int(np.argmax(ext))   # the first of equal extents
        if (ext == ext[axis]).sum() > 1:
            events.setdefault("axis_tie", []).append(tuple(int(a) for a in np.nonzero(ext == ext[axis])[0]))
        sel = owner == best
        planes = np.bincount(coord[sel, axis] - lo[axis], weights=cnt[occ[sel]], minlength=32).astype(np.int64)
        cut, cum = int(hi[axis]) - 1, 0
        for q in range(int(lo[axis]), int(hi[axis])):
            cum += int(planes[q - lo[axis]])
            if 2 * cum >= n:
                cut = q
                if 2 * cum == n:
                    events["half"] = events.get("half", 0) + 1
                break
        else:
            events["fallback"] = events.get("fallback", 0) + 1
        owner[sel & (coord[:, axis] > cut)] = nb
        nb += 1
    for i in range(nb):
        sel = owner == i
        n = int(cnt[occ[sel]].sum())
        s = sums[occ[sel]].sum(0)
        pal[i] = (2 * s + n) // (2 * n)
    return pal.astype(np.uint8), nb, events


def lzw_trace(idx):
    """include/rtc.h's LZW of one segment, restated: the dictionary's next code after each index, and the indices at which
    a full dictionary restarts. Returns (next_after, restarts, next_final) where next_final counts the last code."""
    d, nxt, width = {}, 258, 9
    prefix = int(idx[0])
    after, restarts = [nxt], []
    for i in range(1, len(idx)):
        k = int(idx[i])
        if (prefix, k) in d:
            prefix = d[(prefix, k)]
        else:
            if nxt < 4096:
                d[(prefix, k)] = nxt
                nxt += 1
            else:
                restarts.append(i)
                d, nxt = {}, 258
            prefix = k
        after.append(nxt)
    return after, restarts, nxt + 1 if nxt < 4096 else nxt


def gif_frame(b):
    g = HG.parse_gif(b)
    assert len(g["frames"]) == 1
    return g, g["frames"][0]


def check_gif(px, b, events=None):
    """The file against the numpy cut and nearest-entry rule: its table, its decoded indices; returns the cut's events."""
    g, f = gif_frame(b)
    pal, used, ev = median_cut_np(px)
    assert np.array_equal(f["table"], pal), "palette differs from the numpy median cut"
    assert np.array_equal(f["indices"], HG.brute_nearest(px, pal))
    assert np.array_equal(HG.decoded_rgb(g)[0], pal[f["indices"]].reshape(px.shape))
    if used <= 256 and len(np.unique(px.reshape(-1, 3), axis=0)) <= 256:
        assert np.array_equal(HG.decoded_rgb(g)[0], px)
    return pal, used, ev


def colours_in_bins(bins, per_bin, reps, rng):
    """Pixels: `per_bin` distinct colours in each bin (r>>3, g>>3, b>>3) of `bins`, each repeated reps[i] times."""
    out = []
    for (br, bg, bb), r in zip(bins, reps):
        offs = rng.permutation(512)[:per_bin]
        c = np.stack([br * 8 + (offs >> 6), bg * 8 + ((offs >> 3) & 7), bb * 8 + (offs & 7)], -1)
        out.append(np.repeat(c, r, axis=0))
    px = np.concatenate(out)
    return px


def to_frame(px, w, rng):
    n = -(-len(px) // w) * w
    if n > len(px):
        px = np.concatenate([px, np.repeat(px[-1:], n - len(px), axis=0)])   # the padding repeats a colour already counted
    return px[rng.permutation(n)].reshape(n // w, w, 3).astype(np.uint8)


def make_256_colours():
    rng = np.random.default_rng(201)
    c = rng.choice(1 << 24, 256, replace=False)
    px = np.stack([c >> 16, (c >> 8) & 255, c & 255], -1)
    return np.concatenate([px, px[rng.integers(0, 256, 40 * 33 - 256)]])[rng.permutation(40 * 33)].reshape(40, 33, 3)


def check_256(px, b):
    pal, used, ev = check_gif(px, b)
    assert used == 256 and len(np.unique(px.reshape(-1, 3), axis=0)) == 256


def make_257_colours():
    rng = np.random.default_rng(202)
    c = rng.choice(1 << 24, 257, replace=False)
    px = np.stack([c >> 16, (c >> 8) & 255, c & 255], -1)
    return np.concatenate([px, px[rng.integers(0, 257, 30 * 37 - 257)]])[rng.permutation(30 * 37)].reshape(30, 37, 3)


def check_257(px, b):
    pal, used, ev = check_gif(px, b)
    assert len(np.unique(px.reshape(-1, 3), axis=0)) == 257 and used == 256 and "stop" not in ev


def check_one_bin(px, b):
    pal, used, ev = check_gif(px, b)
    assert used == 1 and ev == {"stop": 1} and not pal[1:].any()


def check_early_stop(px, b):
    pal, used, ev = check_gif(px, b)
    assert used == 12 and ev.get("stop") == 12


def check_box_tie(px, b):
    pal, used, ev = check_gif(px, b)
    assert (0, 1) in ev.get("box_tie", []) and ev.get("half", 0) >= 1 and used == 4


def check_axis_tie(px, b):
    pal, used, ev = check_gif(px, b)
    assert ev.get("axis_tie") == [(0, 1), (1, 2)] and used == 3


def check_fallback(px, b):
    pal, used, ev = check_gif(px, b)
    assert ev.get("fallback", 0) >= 1


def equidistant_pixels(px, pal):
    """Pixels whose least distance is reached by two entries of different colours."""
    q = px.reshape(-1, 3).astype(np.int64)
    d = ((q[:, None, :] - pal[None, :, :].astype(np.int64)) ** 2).sum(-1)
    m = d.min(1, keepdims=True)
    out = []
    for i in np.nonzero((d == m).sum(1) > 1)[0]:
        tied = np.nonzero(d[i] == m[i])[0]
        if len({tuple(pal[t]) for t in tied}) > 1:
            out.append((int(i), [int(t) for t in tied]))
    return out


def check_equidistant(px, b):
    pal, used, ev = check_gif(px, b)
    eq = equidistant_pixels(px, pal)
    assert eq
    _, f = gif_frame(b)
    assert all(f["indices"][i] == t[0] for i, t in eq)


def make_equidistant():
    """Two clusters in neighbouring bins whose means lie 2 apart on b, and pixels half-way (found by a seeded search)."""
    rng = np.random.default_rng(EQ_SEED)
    px = colours_in_bins([(8, 8, 8), (8, 8, 9), (20, 4, 4)], 150, [3, 3, 2], rng)
    return to_frame(px, 30, rng)


EQ_SEED = 0


def make_dict_fill_last():
    """One segment of an exact-palette frame (the index is the colour's rank) that ends on the index at which the
    dictionary, full, restarts."""
    rng = np.random.default_rng(203)
    idx = rng.integers(0, 256, 4096)
    idx[:256] = rng.permutation(256)
    _, restarts, _ = lzw_trace(idx)
    n = restarts[0] + 1
    v = np.arange(256)
    colours = np.stack([v, 255 - v, (v * 7) & 255], -1)
    colours = colours[np.argsort(colours[:, 0] << 16 | colours[:, 1] << 8 | colours[:, 2])]
    return colours[idx[:n]].reshape(1, n, 3)


def check_dict_fill_last(px, b):
    check_gif(px, b)
    _, f = gif_frame(b)
    idx = f["indices"]
    assert len(idx) <= HG.S
    _, restarts, _ = lzw_trace(idx)
    assert restarts == [len(idx) - 1]
    assert HG.n_clears(f["data"]) == 2   # the opening clear and the restart on the last index


SUBBLOCK_SIZES = {509: 19787, 510: 19788, 511: 19871}   # LZW bytes 255k - 1, 255k, 255k + 1 of a one-colour (1, N) frame


def subblock_lengths(b: bytes) -> list:
    """The sub-block length bytes of a one-frame file: after the 13-byte header, the 8-byte graphic control extension, the
    10-byte descriptor, the 768-byte table and the minimum code size."""
    p, out = 13 + 8 + 10 + 768 + 1, []
    while b[p]:
        out.append(b[p])
        p += 1 + b[p]
    assert b[p:] == b"\x00\x3b"
    return out


def subblock_case(nbytes, n):
    def check(px, b):
        check_gif(px, b)
        _, f = gif_frame(b)
        assert len(f["data"]) == nbytes
        assert subblock_lengths(b) == [255] * (nbytes // 255) + ([nbytes % 255] if nbytes % 255 else [])
    return Case(f"gif_subblock_{nbytes}", "gif", f"{nbytes} bytes of LZW data: sub-blocks of 255 and {nbytes % 255}",
                lambda: np.full((1, n, 3), (10, 20, 30), np.uint8), check)


def gif_cases():
    rng = np.random.default_rng
    spec = [
        ("gif_256_colours", "k_gif_exact: 256 distinct colours", make_256_colours, check_256),
        ("gif_257_colours", "k_gif_median_cut: 257 distinct colours", make_257_colours, check_257),
        ("gif_one_bin", "k_gif_median_cut: 300 colours in one bin, one box",
         lambda: to_frame(colours_in_bins([(9, 17, 25)], 300, [2], rng(204)), 25, rng(204)), check_one_bin),
        ("gif_early_stop", "k_gif_median_cut: key == 0 after 12 boxes",
         lambda: to_frame(colours_in_bins([(i * 2, 31 - i, (i * 5) % 32) for i in range(12)], 30, [1 + i % 3 for i in range(12)],
                                          rng(205)), 41, rng(205)), check_early_stop),
        ("gif_box_tie", "k_gif_median_cut: equal counts, the lower box splits; 2 * cum == n",
         lambda: to_frame(colours_in_bins([(0, 3, 3), (2, 3, 3), (20, 3, 3), (22, 3, 3)], 100, [1, 1, 1, 1], rng(206)), 40, rng(206)),
         check_box_tie),
        ("gif_axis_tie", "k_gif_median_cut: r and g of equal extent (r), then g and b (g)",
         lambda: to_frame(colours_in_bins([(0, 0, 0), (0, 4, 4), (8, 8, 4)], 100, [1, 1, 1], rng(207)), 40, rng(207)),
         check_axis_tie),
        ("gif_cut_fallback", "k_gif_median_cut: the last plane holds most pixels, cut at hi - 1",
         lambda: to_frame(colours_in_bins([(0, 9, 9), (5, 9, 9)], 150, [1, 20], rng(208)), 50, rng(208)), check_fallback),
        ("gif_equidistant", "k_gif_map: equidistant entries, the lower index", make_equidistant, check_equidistant),
        ("gif_dict_fill_last", "k_gif_lzw: the dictionary fills on the segment's last index", make_dict_fill_last, check_dict_fill_last),
    ]
    out = [Case(n, "gif", br, mk, ck) for n, br, mk, ck in spec] + [subblock_case(k, n) for k, n in SUBBLOCK_SIZES.items()]
    for c in out:
        c.entries = ("gif_encode", "GifWriter", "image:gif")
    return out


# ---- packed formats -------------------------------------------------------------------------------------------------------
def packed_decoded(fmt, b):
    import test_host_image_formats as HI
    if fmt == "ppm":
        from PIL import Image
        return np.asarray(Image.open(io.BytesIO(b)).convert("RGBA"))
    return HI.decode(fmt, b)


def check_packed_pixels(px, b, fmt):
    want = np.concatenate([px[..., :3], np.full(px.shape[:2] + (1,), 255, np.uint8)], axis=2)
    assert np.array_equal(packed_decoded(fmt, b), want)


def packed_width_case(w):
    def check(px, b, fmt):
        assert px.shape[1] == w
        check_packed_pixels(px, b, fmt)
    return Case(f"packed_w{w}", "packed", f"width {w}: w * 3 % 4 = {w * 3 % 4}",
                lambda: np.random.default_rng(300 + w).integers(0, 256, (5, w, 3), dtype=np.uint8), check, formats=PACKED)


def packed_frame(h, w):
    return np.random.default_rng(400 + 7 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def packed_length_sizes(fmt, rem):
    """(h, w) of the first packed_frame of 1..12 rows whose `fmt` file is 16k + rem bytes long (rem -1, 0, 1) and at least
    1 KiB; None where the layout cannot give that length (BMP, TGA and TIFF store 4-byte pixels after a fixed header)."""
    for h in range(1, 13):
        for w in range(16, 200):
            n = len(rtc.image_encode(fmt, packed_frame(h, w)))
            if n >= 1024 and n % 16 == rem % 16:
                return h, w
    return None


# packed_length_sizes of every format that can reach the remainder, kept here because the search takes seconds
PACKED_LENGTHS = {("farbfeld", 0): (1, 126), ("pam", -1): (3, 101), ("pam", 0): (11, 101), ("ppm", -1): (1, 101),
                  ("ppm", 0): (1, 165), ("ppm", 1): (1, 121)}


def packed_length_case(fmt, rem, hw):
    h, w = hw

    def check(px, b, f):
        assert len(b) % 16 == rem % 16
        check_packed_pixels(px, b, f)
    return Case(f"packed_len_{fmt}_{rem:+d}", "packed", f"a {fmt} file of 16k{rem:+d} bytes: k_image_pack's last 16-byte store",
                lambda: packed_frame(h, w), check, formats=(fmt,))


def packed_cases():
    out = [packed_width_case(w) for w in (8, 9, 10, 11)]
    out += [packed_length_case(f, r, hw) for (f, r), hw in PACKED_LENGTHS.items()]
    for c in out:
        c.entries = tuple(f"image:{f}" for f in c.formats)
    return out


def all_cases(large=True):
    return png_cases() + jpeg_cases(large) + gif_cases() + packed_cases()
