"""Named small canvases for the post-processing tests (tests/test_host_post.py, tests/test_gpu_post.py): values in [0, 8) from a
seeded generator, with the pixels planted at which the statistics, the curves and the bright pass decide: a NaN, a +inf, a negative
component, and a pixel whose luminance is exactly the bloom threshold of the case. No -0.0 is planted: -0.0 + 0.0 is +0.0, so a
pass that "changes nothing" would still change those bytes."""
import math

import numpy as np

# name -> (width, height); the sizes at which the kernels take another path: one pixel, one row, one column, a row segment or a
# tile and one more or less, an image narrower than the widest halo, more than one 256-pixel segment, more than one 64-row tile
SIZES = {"1x1": (1, 1), "1x40": (1, 40), "40x1": (40, 1), "31x9": (31, 9), "33x9": (33, 9), "5x3": (5, 3), "257x3": (257, 3), "70x70": (70, 70),
         "black-16x4": (16, 4)}
NAMES = list(SIZES)
RADII = (1, 2, 32)
THRESHOLD_PIXEL = (1.5, 0.75, 2.0)   # planted at pixel 5; its luminance is the case's bloom threshold
STAT_PIXELS = (255, 256, 257, 65536, 65537)   # the block edge, the second level exactly full, the first use of the third level


def luminance(c):
    """Y(c) in the header's order, on arrays (numpy never fuses)."""
    c = np.asarray(c, dtype=np.float64)
    return ((0.2126 * c[..., 0]) + (0.7152 * c[..., 1])) + (0.0722 * c[..., 2])


def threshold():
    return float(luminance(np.array(THRESHOLD_PIXEL)))


def canvas(name):
    """The (H, W, 3) float64 canvas of the case."""
    width, height = SIZES[name]
    if name.startswith("black"):
        return np.zeros((height, width, 3))
    rng = np.random.default_rng(1000 * width + height)
    c = rng.uniform(0.0, 8.0, size=(height, width, 3))
    flat = c.reshape(-1, 3)
    if len(flat) >= 8:
        flat[1, 1] = math.nan
        flat[2, 0] = math.inf
        flat[3] = (-0.5, 2.0, 1.0)
        flat[5] = THRESHOLD_PIXEL
        flat[len(flat) - 1] = (0.0, 0.0, 0.0)
    return c


def strip(n):
    """An n x 1 canvas for the statistics: [0, 8) with a NaN, a +inf, a negative and a black pixel where there is room."""
    rng = np.random.default_rng(n)
    c = rng.uniform(0.0, 8.0, size=(1, n, 3))
    c[0, n // 2, 2] = math.nan
    c[0, n // 3, 0] = math.inf
    c[0, n - 1] = (-4.0, 0.25, 0.0)
    c[0, 0] = (0.0, 0.0, 0.0)
    return c


# ---- the restatement: numpy and explicit loops, nothing of the library ------------------------------------------------------------
def canon(v):
    return np.where(np.isnan(v), np.nan, v)   # np.nan is 0x7FF8000000000000


def _tree(v):
    v = v.copy()
    s = 128
    while s >= 1:
        v[:s] = v[:s] + v[s:2 * s]
        s //= 2
    return v[0]


def expected_luminance(c):
    """(max, sum, count) by the header's statement."""
    y = luminance(c).reshape(-1)
    ok = (y > 0.0) & (y < math.inf)
    level = np.where(ok, y, 0.0)
    if len(level) == 0:
        level = np.zeros(1)
    while True:
        blocks = (len(level) + 255) // 256
        padded = np.zeros(blocks * 256)
        padded[:len(level)] = level
        level = np.array([_tree(padded[256 * b:256 * b + 256]) for b in range(blocks)])
        if blocks == 1:
            break
    return (float(y[ok].max()) if ok.any() else 0.0), float(level[0]), int(ok.sum())


def expected_resolve(exposure, white, flags, stats):
    """(m, inv_w2); stats = (max, sum, count) or None."""
    m = exposure
    with np.errstate(all="ignore"):
        if flags & 1:
            mx, total, count = stats
            mean = np.float64(total) / np.float64(count)
            m = float(np.float64(exposure) / mean) if count > 0 and mean > 0.0 else 1.0
        lw = white
        if flags & 2:
            lw = float(np.float64(stats[0]) * np.float64(m))
        inv = float(np.float64(1.0) / (np.float64(lw) * np.float64(lw))) if (lw > 0.0 and lw < math.inf) else 0.0
    return m, inv


def _aces(x):
    a = (2.51 * x) + 0.03
    b = (2.43 * x) + 0.59
    o = (x * a) / ((x * b) + 0.14)
    o = np.where(o > 1.0, 1.0, o)
    return np.where(x > 0.0, o, 0.0)


def expected_tonemap(c, curve, m, inv_w2):
    with np.errstate(all="ignore"):
        cp = np.asarray(c, dtype=np.float64) * m
        if curve == 1:
            lum = luminance(cp)
            s = (1.0 + (lum * inv_w2)) / (1.0 + lum)
            cp = np.where((lum > 0.0)[..., None], cp * s[..., None], cp)
        elif curve == 2:
            cp = _aces(cp)
        return canon(cp)


def expected_weights(sigma, radius):
    g = [math.exp(-float(k * k) / ((2.0 * sigma) * sigma)) for k in range(-radius, radius + 1)]
    total = 0.0
    for v in g:
        total = total + v
    return np.array([v / total for v in g])


def expected_bloom(c, thr, strength, sigma, radius):
    """The header's bloom with every out-of-image tap ADDED as +0.0 (the host statement skips them: the same bytes)."""
    c = np.asarray(c, dtype=np.float64)
    height, width = c.shape[:2]
    w = expected_weights(sigma, radius)
    with np.errstate(all="ignore"):
        lum = luminance(c)
        k = (lum - thr) / lum
        bright = np.where(((lum > thr) & (lum < math.inf))[..., None], c * k[..., None], 0.0)
        pad = np.zeros((height, width + 2 * radius, 3))
        pad[:, radius:radius + width] = bright
        hor = np.zeros((height, width, 3))
        for t in range(2 * radius + 1):
            hor = hor + (w[t] * pad[:, t:t + width])
        pad = np.zeros((height + 2 * radius, width, 3))
        pad[radius:radius + height] = hor
        ver = np.zeros((height, width, 3))
        for t in range(2 * radius + 1):
            ver = ver + (w[t] * pad[t:t + height])
        return canon(c + (strength * ver))
