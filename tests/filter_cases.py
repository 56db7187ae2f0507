"""The edge-aware filter's synthetic cases (include/rtc.h, "edge-aware filter") and an independent restatement of the host
statement, shared by tests/test_host_filter.py (host == restatement) and tests/test_gpu_filter.py (device == host).

The restatement walks the pixels and taps in plain Python over Python floats: IEEE binary64 like numpy's float64 scalars, one
rounding per operation, no fused multiply-add, and every product and sum written in the header's order.

The sizes are those at which the kernel can go wrong: smaller than the two-tap halo, one pixel wide or high, no multiple of
the 32 x 8 tile, several tiles, and at `passes = 5` (step 16) an image in which no tap but the centre is in range (16 x 16) and
one in which exactly one neighbour on each side is (17 x 17); every residue class of a step > 1 has another number of pixels in
37 x 29. Guides and values come from seeded generators; a case's arrays and its expected plane are computed once."""
import functools
import math

import numpy as np

SAME = 1
H5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
QNAN = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), dtype=np.float64)[0]
NAN = float(QNAN)   # the same bits as a Python float


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _pass(src, index, point, normal, width, height, ch, s, inv, squarings, same):
    """One pass over flat Python lists: src[ch*p + c], index[p], point[3*p + c], normal[3*p + c] -> the next plane."""
    dst = list(src)   # a miss, or no surviving tap: the pixel is copied
    for y in range(height):
        for x in range(width):
            p = y * width + x
            ip = index[p]
            if ip < 0:
                continue
            npx, npy, npz = normal[3 * p], normal[3 * p + 1], normal[3 * p + 2]
            ppx, ppy, ppz = point[3 * p], point[3 * p + 1], point[3 * p + 2]
            acc = [0.0] * ch
            wsum = 0.0
            for j in range(5):
                qy = y + (j - 2) * s
                if qy < 0 or qy >= height:
                    continue
                for i in range(5):
                    qx = x + (i - 2) * s
                    if qx < 0 or qx >= width:
                        continue
                    q = qy * width + qx
                    iq = index[q]
                    if iq < 0 or (same and iq != ip):
                        continue
                    ex, ey, ez = point[3 * q] - ppx, point[3 * q + 1] - ppy, point[3 * q + 2] - ppz
                    d = abs(((npx * ex) + (npy * ey)) + (npz * ez))
                    wz = 1.0 - d * inv
                    if not (wz > 0.0):
                        continue
                    m = ((npx * normal[3 * q]) + (npy * normal[3 * q + 1])) + (npz * normal[3 * q + 2])
                    if not (m > 0.0):
                        continue
                    for _ in range(squarings):
                        m = m * m
                    w = ((H5[j] * H5[i]) * wz) * m
                    if not (w > 0.0):
                        continue
                    for c in range(ch):
                        acc[c] = acc[c] + w * src[ch * q + c]
                    wsum = wsum + w
            if wsum > 0.0:
                for c in range(ch):
                    v = acc[c] / wsum
                    dst[ch * p + c] = v if v == v else NAN   # a NaN quotient is stored as the one quiet NaN
    return dst


def restate(values, planes, flt):
    """rtc_plane_filter restated. values: (H, W) or (H, W, 3) float64; planes: index / point / normal; flt = (plane_sigma, passes,
    normal_squarings, flags). -> an array of values' shape."""
    sigma, passes, squarings, flags = flt
    height, width = values.shape[:2]
    ch = 1 if values.ndim == 2 else 3
    index = planes["index"].reshape(-1).tolist()
    point = planes["point"].reshape(-1).tolist()
    normal = planes["normal"].reshape(-1).tolist()
    inv = 1.0 / sigma   # 0.0 for +infinity
    cur = values.reshape(-1).tolist()
    for k in range(passes):
        nxt = _pass(cur, index, point, normal, width, height, ch, 1 << k, inv, squarings, bool(flags & SAME))
        cur = nxt
    return np.array(cur, dtype=np.float64).reshape(values.shape)


# ---- guides ---------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _plane_points(rng, n, xs, ys, origin, pitch=0.03, noise=1e-4):
    """Points of a grid on the plane through `origin` with normal n, `pitch` apart, each lifted off the plane by its own noise."""
    a = _unit(np.cross(n, (0.0, 0.0, 1.0) if abs(n[2]) < 0.9 else (1.0, 0.0, 0.0)))
    b = np.cross(n, a)
    off = rng.uniform(-noise, noise, size=xs.shape)
    return np.asarray(origin) + xs[..., None] * pitch * a + ys[..., None] * pitch * b + off[..., None] * n


def _guides(kind, width, height, rng):
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    index = np.zeros((height, width), dtype=np.int32)
    point = np.zeros((height, width, 3))
    normal = np.zeros((height, width, 3))
    if kind in ("planes", "axis"):   # two planes meeting at the edge x = width / 2; "axis": with normals that are exact axis vectors
        n_left, n_right = ((0.0, 1.0, 0.0), (0.0, 0.0, -1.0)) if kind == "axis" else (_unit((0.3, 1.0, 0.2)), _unit((-0.8, 0.5, 0.1)))
        left = xs < width / 2.0
        edge = (width / 2.0) * 0.03
        pl = _plane_points(rng, np.asarray(n_left), xs, ys, (0.0, 0.0, 0.0))
        pr = _plane_points(rng, np.asarray(n_right), xs, ys, (edge, 0.0, 0.0))
        point[:] = np.where(left[..., None], pl, pr)
        normal[:] = np.where(left[..., None], n_left, n_right)
        index[:] = np.where(left, 0, 1)
    elif kind == "patches":   # random index patches, about 20 % misses, a normal per patch and a wobble per pixel
        cell = rng.integers(0, 6, size=((height + 4) // 5 + 1, (width + 6) // 7 + 1))
        index[:] = cell[(ys // 5).astype(int), (xs // 7).astype(int)]
        patch_n = _unit(rng.normal(size=(6, 3)))
        normal[:] = _unit(patch_n[index] + rng.normal(scale=0.05, size=(height, width, 3)))
        point[:] = np.stack([xs * 0.03, ys * 0.03, 0.02 * np.sin(xs * 0.4) * np.cos(ys * 0.3)], axis=-1) + rng.normal(scale=1e-3, size=(height, width, 3))
        miss = rng.uniform(size=(height, width)) < 0.2
        index[miss] = -1
        point[miss] = 0.0
        normal[miss] = 0.0
    elif kind == "allmiss":
        index[:] = -1
    else:
        raise KeyError(kind)
    return {"index": index, "point": point, "normal": normal}


# ---- the cases: name -> (width, height, channels, guides, (plane_sigma, passes, normal_squarings, flags), extras) -----------
INF = math.inf
TINY = 1e-300   # 1/TINY is finite; any neighbour lies farther than that off the pixel's tangent plane
CASES = {
    "1x1":              (1, 1, 1, "planes", (0.05, 3, 1, SAME), ()),
    "5x3-c3":           (5, 3, 3, "planes", (0.05, 5, 1, SAME), ()),
    "64x1":             (64, 1, 1, "patches", (INF, 4, 0, 0), ()),
    "1x64-c3":          (1, 64, 3, "patches", (0.05, 4, 8, SAME), ()),
    "37x29-planes":     (37, 29, 1, "planes", (0.05, 2, 8, SAME), ("nan-guides",)),
    "37x29-planes-c3":  (37, 29, 3, "planes", (0.05, 3, 1, 0), ()),
    "37x29-patches-c3": (37, 29, 3, "patches", (INF, 3, 0, 0), ("nan-guides",)),
    "37x29-poison":     (37, 29, 1, "patches", (INF, 3, 1, SAME), ("poison",)),
    "37x29-poison-c3":  (37, 29, 3, "planes", (0.05, 3, 0, SAME), ("poison",)),
    "37x29-tiny":       (37, 29, 1, "axis", (TINY, 3, 1, 0), ("dyadic",)),
    "37x29-tiny-c3":    (37, 29, 3, "axis", (TINY, 2, 8, SAME), ("dyadic",)),
    "16x16-p5":         (16, 16, 1, "patches", (INF, 5, 1, 0), ()),
    "16x16-p5-c3":      (16, 16, 3, "planes", (0.05, 5, 1, SAME), ()),
    "17x17-p5":         (17, 17, 1, "planes", (INF, 5, 0, 0), ()),
    "17x17-p5-c3":      (17, 17, 3, "patches", (INF, 5, 1, SAME), ()),
    "70x40-p1":         (70, 40, 1, "planes", (0.05, 1, 0, 0), ()),
    "70x40-p2-c3":      (70, 40, 3, "patches", (INF, 2, 1, SAME), ()),
    "70x40-p3":         (70, 40, 1, "patches", (0.05, 3, 8, 0), ()),
    "70x40-p4-c3":      (70, 40, 3, "planes", (0.05, 4, 1, SAME), ()),
    "70x40-p5":         (70, 40, 1, "planes", (INF, 5, 0, SAME), ()),
    "33x9-allmiss-c3":  (33, 9, 3, "allmiss", (0.05, 2, 1, SAME), ()),
}
NAMES = list(CASES)
POISON_AT = ((11, 9), (30, 20))   # (x, y): pixels of an index of their own that hold inf and NaN under RTC_FILTER_SAME_OBJECT
NAN_NORMAL_AT, NAN_POINT_AT = (5, 4), (20, 17)


@functools.lru_cache(maxsize=None)
def arrays(name):
    """-> (values, planes) of a case; read-only, shared by every test."""
    width, height, ch, kind, flt, extras = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + width * 31 + height)
    planes = _guides(kind, width, height, rng)
    shape = (height, width) if ch == 1 else (height, width, 3)
    values = rng.uniform(0.0, 1.0, size=shape)
    if "dyadic" in extras:   # values of few significant bits: an occlusion fraction count / 256
        values = rng.integers(0, 257, size=shape).astype(np.float64) / 256.0
    if "nan-guides" in extras:
        (x, y), (u, v) = NAN_NORMAL_AT, NAN_POINT_AT
        planes["index"][y, x] = planes["index"][v, u] = 0   # both hit
        planes["normal"][y, x] = QNAN
        planes["point"][v, u, 1] = QNAN
    if "poison" in extras:
        assert flt[3] & SAME
        for k, (x, y) in enumerate(POISON_AT):
            planes["index"][y, x] = 100 + k
            values[y, x] = (INF, QNAN)[k]
    for a in (values, *planes.values()):
        a.setflags(write=False)
    return values, planes


@functools.lru_cache(maxsize=None)
def expected(name):
    values, planes = arrays(name)
    out = restate(values, planes, CASES[name][4])
    out.setflags(write=False)
    return out


def spec(rtc, name):
    sigma, passes, squarings, flags = CASES[name][4]
    return rtc.filter_spec(sigma, passes=passes, normal_squarings=squarings, same_object=bool(flags & SAME))
