"""f64 square roots in the flat k_trace kernels without the expansion's range scaffolding, chosen per wave (rtc_kernels.hip
sqrt_wave: the expansion's ten-instruction core when every active lane's operand is a normal number of at least 2^-767,
plain sqrt for the whole wave otherwise), and the same root inside vnormalize_wave under one guard on the sum of squares.

Arithmetic: rtc_device_arith op 9 — the function the kernels call, thread t taking value t, so a wave holds 64 consecutive
values — against op 0 (plain sqrt on the device) and NumPy's sqrt, bit for bit, NaN for NaN: random mantissas at every
exponent, exact squares of 26-bit integers times powers of four with their neighbours one ulp below and above (the hard
roundings), the guard's edges, and denormals, zeros, negative numbers, infinities and NaN; in waves of one kind and in waves
of all kinds mixed.

Normalize: op 8 against op 6 over tests/test_gpu_shared_normalize_flat.py's triples and over triples whose sum of squares
sits on either side of 2^-767 and of 2^799, the edges of vnormalize_wave's guard on it.

Frames: a sphere, a cube, a plane and a ring-patterned plane, specular == 0, at 32x16 and 40x24 pixels through the flat
one-level kernel and, padded past 256 objects, the flat two-level one; as they are, scaled by 2^-450 (every sum of squares
is below 2^-767: the normalisations' roots fall back; the discriminants, of order 2^900, stay bare) and scaled by 2^450
(sums of squares of order 2^900 and discriminants of order 2^-900: every one of those roots falls back together with the
reciprocal; the ring pattern's root, taken in pattern space, is ordinary in all three). Canvas and rtc_color_at hit records
equal the oracle's bit for bit. The oracle's frames are computed first, once, and must hold hits, shadowed hits and misses."""
import math

import numpy as np
import pytest

from test_gpu_shared_normalize_flat import PADS, SRC_CULL, SRC_CULL2, _bits, _record, _same_bits, _scale_world, normalize_triples
from test_gpu_shared_normalize_flat import build as base_scene

pytestmark = pytest.mark.gpu

SIZES = ((32, 16), (40, 24))
SETTINGS = ("ordinary", "scaled 2^-450", "scaled 2^450")
WAVES = 4096
BELOW = float(np.nextafter(2.0 ** -767, 0.0))
DBL_MAX = float(np.finfo(np.float64).max)
EDGES = (2.0 ** -768, BELOW, 2.0 ** -767, 2.0 ** -766, 2.0 ** 1023, DBL_MAX)
OUTSIDE = (5e-324, 3e-320, 1e-310, 2.0 ** -1023, 0.0, -0.0, -1.0, -2.0 ** -800, -DBL_MAX, math.inf, -math.inf, math.nan)


# ---- arithmetic -------------------------------------------------------------------------------------------------------
def sqrt_guard(x):
    """sqrt_bare_ok per value, on the upper word as the device reads it."""
    hi = (np.ascontiguousarray(x).view(np.uint64) >> np.uint64(32)).astype(np.uint32)
    return (hi - np.uint32(256 << 20)) < np.uint32((2047 - 256) << 20)   # (uint32: wraps as the device's subtraction does)


def _values_of_kind(rng, kind, sub, n):
    """n values of one kind; `sub` picks the kind's variant: the whole range (0), wholly inside the guard (1), outside (2)."""
    if kind == 0:    # random mantissas at even and odd exponents
        lo, hi = ((-1022, 1024), (-767, 1024), (-1022, -767))[sub % 3]
        return np.ldexp(1.0 + rng.random(n), rng.integers(lo, hi, n))
    if kind == 1:    # m * m * 4^k, m a 26-bit integer (the square is exact: 52 bits), and its neighbours one ulp away
        m = rng.integers(2 ** 25, 2 ** 26, n).astype(np.float64)
        k = rng.integers(-530 if sub % 2 == 0 else -400, 481, n)
        sq = np.ldexp(m * m, 2 * k)
        step = rng.integers(-1, 2, n)
        return np.where(step < 0, np.nextafter(sq, 0.0), np.where(step > 0, np.nextafter(sq, np.inf), sq))
    if kind == 2:    # the guard's edges
        return np.array(EDGES)[rng.integers(0, len(EDGES), n)]
    return np.array(OUTSIDE)[rng.integers(0, len(OUTSIDE), n)]   # denormals, zeros, negative numbers, infinities, NaN


def sqrt_values():
    """64 * WAVES values: the first half in waves of one kind (64 consecutive values), the second half with every value's
    kind drawn on its own."""
    rng = np.random.default_rng(9)
    out = np.empty(WAVES * 64)
    for w in range(WAVES // 2):
        out[w * 64:(w + 1) * 64] = _values_of_kind(rng, w % 4, w // 4, 64)
    n_mixed = (WAVES - WAVES // 2) * 64
    kinds, subs = rng.integers(0, 4, n_mixed), rng.integers(0, 6, n_mixed)
    mixed = out[WAVES // 2 * 64:]
    for k in range(4):
        for s in range(6):
            sel = np.flatnonzero((kinds == k) & (subs == s))
            mixed[sel] = _values_of_kind(rng, k, s, len(sel))
    return out


def test_wave_sqrt_equals_plain_sqrt_and_the_host(gpu):
    x = sqrt_values()
    with np.errstate(all="ignore"):
        assert sqrt_guard(np.array([2.0 ** -767, 2.0 ** -766, DBL_MAX, 1.0])).all()
        assert not sqrt_guard(np.array([BELOW, 2.0 ** -768, math.inf, math.nan, 0.0, -0.0, -1.0, 2.0 ** -1023])).any()
    ok = sqrt_guard(x).reshape(-1, 64)
    whole_pass, whole_fail = int(ok.all(axis=1).sum()), int((~ok).all(axis=1).sum())
    mixed = len(ok) - whole_pass - whole_fail
    print(f"{len(x)} values in {len(ok)} waves: {whole_pass} wholly inside the guard, {whole_fail} wholly outside, {mixed} mixed")
    assert len(x) == 64 * 4096 and whole_pass > 100 and whole_fail > 100 and mixed > 100
    for e in EDGES:
        assert (x == e).any(), e
    tiny = np.abs(x) < 2.0 ** -1022
    assert ((x != 0.0) & tiny).any() and (x == 0.0).any() and np.signbit(x[x == 0.0]).any() and (x < 0.0).any()
    assert (x == math.inf).any() and (x == -math.inf).any() and np.isnan(x).any()
    wave = gpu.device_arith(9, x)
    plain = gpu.device_arith(0, x)
    with np.errstate(all="ignore"):
        host = np.sqrt(x)
    bad = np.flatnonzero(~_same_bits(wave, plain))
    assert len(bad) == 0, (len(bad), x[bad[:4]].tolist(), wave[bad[:4]].tolist(), plain[bad[:4]].tolist())
    bad = np.flatnonzero(~_same_bits(wave, host))
    assert len(bad) == 0, (len(bad), x[bad[:4]].tolist(), wave[bad[:4]].tolist(), host[bad[:4]].tolist())


# ---- normalize --------------------------------------------------------------------------------------------------------
S_EDGES = (-767, 799)   # vnormalize_wave's guard on the sum of squares s: 2^-767 <= s < 2^799


def _sum_of_squares(v):
    return v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]   # (the device's statement, unfused)


def edge_triples():
    """(64 * 512, 3): directions of length 2^(e/2) * (1 + d) for each edge 2^e of the guard on s — components near 2^-384 and
    near 2^399.5 — with d of either sign from 2^-52 to 2^-12; the first half in waves of one edge and one side, the second
    half with edge and side drawn per triple."""
    rng = np.random.default_rng(31)
    n = 64 * 512
    u = rng.normal(size=(n, 3))
    axis = rng.random(n) < 0.25   # a quarter along one axis: s is the square of one component
    u[axis] = 0.0
    u[axis, rng.integers(0, 3, int(axis.sum()))] = 1.0
    u /= np.sqrt(_sum_of_squares(u))[:, None]
    wave = np.arange(n) // 64
    first = wave < 256
    edge = np.where(first, wave % 2, rng.integers(0, 2, n))
    side = np.where(first, (wave // 2) % 2, rng.integers(0, 2, n)) * 2.0 - 1.0
    d = side * np.ldexp(1.0, -rng.integers(12, np.where(first, 41, 53), n))   # (whole waves: far enough for the side to be certain)
    length = np.where(edge == 0, math.sqrt(2.0) * 2.0 ** -384, math.sqrt(2.0) * 2.0 ** 399) * (1.0 + d)
    return u * length[:, None]


def test_wave_normalize_equals_three_divisions_at_the_new_guard(gpu):
    edges = edge_triples()
    s = _sum_of_squares(edges)
    for e in S_EDGES:   # triples within a factor 1 +- 2^-10 of the edge, on both sides of it
        near = (s > 2.0 ** e * (1.0 - 2.0 ** -10)) & (s < 2.0 ** e * (1.0 + 2.0 ** -10))
        assert (near & (s < 2.0 ** e)).sum() > 1000 and (near & (s >= 2.0 ** e)).sum() > 1000, e
    inside = ((s >= 2.0 ** -767) & (s < 2.0 ** 799)).reshape(-1, 64)
    assert inside.all(axis=1).sum() > 50 and (~inside).all(axis=1).sum() > 50 and (inside.any(axis=1) & ~inside.all(axis=1)).sum() > 50
    v = np.concatenate([normalize_triples(), edges])
    flat = np.ascontiguousarray(v.reshape(-1))
    wave = gpu.device_arith(8, flat).reshape(-1, 3)
    plain = gpu.device_arith(6, flat).reshape(-1, 3)
    bad = np.flatnonzero(~_same_bits(wave, plain).all(axis=1))
    assert len(bad) == 0, (len(bad), v[bad[:4]].tolist(), wave[bad[:4]].tolist(), plain[bad[:4]].tolist())


# ---- frames -----------------------------------------------------------------------------------------------------------
def build(rtc, setting, size, padded):
    """test_gpu_shared_normalize_flat's sphere, cube and floor, and a wall at x = -3 with a ring pattern whose transform
    turns the wall's own plane into the pattern's x-y plane (Pattern::ring reads x and y); then scaled."""
    M = rtc.Matrix
    w, cam = base_scene(rtc, "ordinary", size, padded)
    rings = ("ring", (0.9, 0.8, 0.2), (0.1, 0.3, 0.7), M.identity().scaling(0.4, 0.4, 0.4).rotation_x(1.0))
    w.add_shape(rtc.plane(M.identity().rotation_z(math.pi / 2).translation(-3.0, 0.0, 0.0), rtc.material(ambient=0.2, diffuse=0.7, specular=0.0, pattern=rings)))
    if setting.startswith("scaled"):
        w, cam = _scale_world(rtc, w, cam, 2.0 ** (-450 if "-450" in setting else 450))
    return w, cam


@pytest.fixture(scope="module")
def references(rtc, O):
    """{(setting, size, padded): (oracle canvas, oracle hit records of every pixel's ray, the rays)}: computed once, on the
    CPU, and checked to be finite and to hold hits, shadowed hits and misses."""
    out = {}
    for setting in SETTINGS:
        for size in SIZES:
            for padded in (False, True):
                w, cam = build(rtc, setting, size, padded)
                arr = w.array()
                canvas = O.render(arr, len(w), w.light, cam, mode=1)
                rays = np.array([rtc.ray_for_pixel(cam, x, y) for y in range(size[1]) for x in range(size[0])])
                recs = [_record(O.color_at(arr, len(w), w.light, tuple(r), 5, want_hit=True)[1]) for r in rays]
                hits = [r for r in recs if r[0] >= 0]
                shadowed = sum(1 for r in hits if r[1])
                assert np.isfinite(canvas).all() and np.isfinite(rays).all(), (setting, size)
                assert np.isfinite(np.array([[r[2], *r[3], *r[4], *r[5]] for r in hits])).all(), (setting, size)
                assert 0 < shadowed < len(hits) < len(recs), (setting, size, shadowed, len(hits), len(recs))
                wall = len(w) - 1
                if setting != "scaled 2^450":   # (a direction of 2^-450 in object space is parallel to a plane for the reference)
                    assert wall in {r[0] for r in hits}, (setting, size)
                if setting == "ordinary":   # every shape is seen, and the wall shows both of its rings' colours
                    assert {r[0] for r in hits} >= {0, 1, 2, wall}, (setting, size)
                    seen = canvas.reshape(-1, 3)[[i for i, r in enumerate(recs) if r[0] == wall]]
                    assert len({tuple(np.round(c / max(c.max(), 1e-300), 3)) for c in seen}) >= 2, (setting, size)
                assert (canvas != 0).any() and (canvas == 0).any()
                out[setting, size, padded] = (canvas, recs, rays)
    return out


@pytest.mark.parametrize("padded", (False, True), ids=("one-level", "two-level"))
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("setting", SETTINGS)
def test_flat_frames_equal_the_oracle_bit_for_bit(rtc, gpu, references, setting, size, padded):
    want, want_recs, rays = references[setting, size, padded]
    w, cam = build(rtc, setting, size, padded)
    dw = gpu.upload(w)
    try:
        got = dw.render(cam, rtc.MODE_RENDER_ASYNC)
        info = gpu.last_launch_info()
        _, hits = dw.color_at(rays, 5, want_hits=True)
    finally:
        dw.close()
    assert info["source"] == (SRC_CULL2 if padded else SRC_CULL) and not info["reflective"], info
    diff = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(diff) == 0, (setting, size, len(diff), diff[:4].tolist())
    for i, wr in enumerate(want_recs):
        assert _bits(_record(hits[i])) == _bits(wr), (setting, size, i, _record(hits[i]), wr)


# ---- resources --------------------------------------------------------------------------------------------------------
def _table(path):
    """{kernel tag: (scratch bytes per lane, occupancy)} of a tools/kernel_resources.py table."""
    import re
    out = {}
    for line in open(path):
        m = re.match(r"(\S.*?)\s+VGPR\s+\d+\s+SGPR\s+\d+\s+scratch\s+(\d+)\s+occupancy\s+(\d+)", line)
        if m:
            out[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return out


def test_recorded_resources_no_kernel_worse_than_the_parent():
    from pathlib import Path
    prof = Path(__file__).resolve().parent.parent / "profiles"
    head, parent = _table(prof / "bare_sqrt_kernel_resources.txt"), _table(prof / "bare_sqrt_kernel_resources_parent.txt")
    assert len(parent) > 40 and set(head) == set(parent), sorted(set(head) ^ set(parent))
    worse = {k: (parent[k], head[k]) for k in parent if head[k][0] > parent[k][0] or head[k][1] < parent[k][1]}
    assert not worse, worse
