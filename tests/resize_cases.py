"""Shared cases of the resize tests (tests/test_host_resize.py, tests/test_gpu_resize.py) and an independent restatement of the
rules of include/rtc.h ("resizing f64 canvases"), written from the header: Python floats (IEEE f64, one rounding per operation,
never fused), loops in tap order, math.floor and math.sin."""
import math

import numpy as np

FILTERS = ["box", "triangle", "catmull-rom", "mitchell", "lanczos3"]
RADIUS = {"box": 0.5, "triangle": 1.0, "catmull-rom": 2.0, "mitchell": 2.0, "lanczos3": 3.0}
POLYNOMIAL = FILTERS[:4]
AXIS_SIZES = [1, 2, 3, 5, 7, 13, 17, 31, 32, 33, 97]
# (w_in, h_in, w_out, h_out); the last one is LANCZOS3 only (1000 taps)
FRAME_SHAPES = [(1, 1, 1, 1), (1, 1, 3, 2), (7, 5, 1, 1), (17, 13, 7, 5), (7, 5, 17, 13), (31, 9, 8, 9), (9, 31, 9, 8), (33, 4, 32, 4)]
LONG_SHAPE = (1000, 1, 1, 1)
CANON_NAN = 0x7FF8000000000000


def kernel(name, x):
    a = abs(x)
    if name == "box":
        return 1.0 if (x > -0.5 and x <= 0.5) else 0.0
    if name == "triangle":
        return 1.0 - a if a < 1.0 else 0.0
    if name == "catmull-rom":
        if a < 1.0:
            return ((((1.5 * a) - 2.5) * a) * a) + 1.0
        if a < 2.0:
            return (((((-0.5 * a) + 2.5) * a) - 4.0) * a) + 2.0
        return 0.0
    if name == "mitchell":
        if a < 1.0:
            return (((((7.0 * a) - 12.0) * a) * a) + (16.0 / 3.0)) / 6.0
        if a < 2.0:
            return (((((((-7.0 / 3.0) * a) + 12.0) * a) - 20.0) * a) + (32.0 / 3.0)) / 6.0
        return 0.0
    assert name == "lanczos3"
    if x == 0.0:
        return 1.0
    if a < 3.0:
        p = 3.141592653589793 * x
        q = p / 3.0
        return (math.sin(p) / p) * (math.sin(q) / q)
    return 0.0


def support(n_in, n_out, name):
    scale = n_in / n_out
    return RADIUS[name] * (scale if scale > 1.0 else 1.0)


def axis(n_in, n_out, name):
    """-> (first, count, rows): per output its first tap, its tap count and the list of its weights."""
    if n_in == n_out:
        return list(range(n_out)), [1] * n_out, [[1.0] for _ in range(n_out)]
    scale = n_in / n_out
    fs = scale if scale > 1.0 else 1.0
    sup = RADIUS[name] * fs
    first, count, rows = [], [], []
    for o in range(n_out):
        c = (o + 0.5) * scale
        f = max(0, math.floor((c - sup) + 0.5))
        e = min(n_in, math.floor((c + sup) + 0.5))
        raw = [kernel(name, (((f + j) + 0.5) - c) / fs) for j in range(e - f)]
        s = 0.0
        for r in raw:
            s = s + r
        first.append(f)
        count.append(e - f)
        rows.append([r / s for r in raw])
    return first, count, rows


def table(n_in, n_out, name):
    """axis() in the library's layout: (first u32[n_out], count u32[n_out], w f64[n_out, taps])."""
    first, count, rows = axis(n_in, n_out, name)
    w = np.zeros((n_out, max(count)), dtype=np.float64)
    for o, r in enumerate(rows):
        w[o, :len(r)] = r
    return np.array(first, dtype=np.uint32), np.array(count, dtype=np.uint32), w


def _canon(v):
    return float("nan") if v != v else v


def _pass(lines, first, count, w):
    """One filtered pass over a list of lines, each a list of values: out[o] = sum of w[o][j] * line[first[o] + j] in tap order."""
    out = []
    for line in lines:
        row = []
        for o in range(len(first)):
            acc = 0.0
            for j in range(int(count[o])):
                acc = acc + (float(w[o][j]) * line[int(first[o]) + j])
            row.append(_canon(acc))
        out.append(row)
    return out


def resize(canvas, w_out, h_out, tab_h, tab_v):
    """The frame rule on an (H, W, 3) f64 array with the tables given (None: the axis is unchanged and copied): the horizontal
    pass first. NaNs produced by a filtered pass are Python's float('nan'), which numpy stores as 0x7FF8000000000000."""
    h_in, w_in = canvas.shape[:2]
    cur = np.array(canvas, dtype=np.float64, copy=True)
    if tab_h is not None:
        nxt = np.empty((h_in, w_out, 3), dtype=np.float64)
        for c in range(3):
            nxt[:, :, c] = np.array(_pass(cur[:, :, c].tolist(), *tab_h), dtype=np.float64).reshape(h_in, w_out)
        cur = nxt
    if tab_v is not None:
        nxt = np.empty((h_out, w_out, 3), dtype=np.float64)
        for c in range(3):
            nxt[:, :, c] = np.array(_pass(cur[:, :, c].T.tolist(), *tab_v), dtype=np.float64).reshape(w_out, h_out).T
        cur = nxt
    assert cur.shape == (h_out, w_out, 3)
    return cur


def canvas(w, h, seed=7):
    """A linear f64 frame with values on both sides of 0 and of 1, some of them exact."""
    rng = np.random.default_rng(seed * 100003 + w * 1009 + h)
    c = rng.uniform(-0.25, 2.5, size=(h, w, 3))
    c[rng.uniform(size=(h, w)) < 0.1] = 0.0
    c[rng.uniform(size=(h, w)) < 0.05] = 1.0
    return c


def special_canvas():
    """17 x 13 with a NaN (non-canonical payload), a +inf and a -inf at chosen pixels: (canvas, [(x, y, channel, kind)])."""
    c = canvas(17, 13, seed=11)
    c[c == 0.0] = 0.125   # no exact zeros elsewhere: what the specials touch is decided by coverage alone
    marks = [(3, 2, 0, "nan"), (12, 9, 1, "+inf"), (8, 6, 2, "-inf")]
    bits = c.view(np.uint64)
    bits[2, 3, 0] = 0x7FF0000000000123
    c[9, 12, 1] = math.inf
    c[6, 8, 2] = -math.inf
    return c, marks
