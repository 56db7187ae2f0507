"""Vector::normalize in the flat k_trace kernels: one reciprocal per normalisation, chosen per wave (rtc_kernels.hip
vnormalize_wave: the shared-divisor form when every active lane of the wave passes its guard, the three IEEE divisions for
the whole wave otherwise).

Arithmetic: rtc_device_arith op 8 — the function the kernels call, thread t normalising triple t, so a wave holds 64
consecutive triples — against op 6 (three divisions on the device) and the host (NumPy f64: sqrt, then three divisions),
bit for bit, NaN for NaN. The triples sit on every side of the guard (components of +-0, 2^-499 .. 5e-324 beside
components of order 1; magnitudes of 2^+-399 .. 2^+-511; inf and NaN), in waves of one kind and in waves of all kinds mixed.

Frames: a sphere, a cube and a plane with specular == 0 materials (the family that is bit-identical to the oracle,
DESIGN.md §3) at 32x16 and 40x24 pixels, through the flat one-level kernel and — padded to more than 256 objects, as
tests/test_gpu_adversarial_flavours.py forces it — the flat two-level one. Canvas and rtc_color_at hit records (t, point,
over_point, normal, shadow bit) equal the oracle's bit for bit in three settings:
  a. an ordinary scene: every wave takes the shared form;
  b. the same scene and camera scaled by 2^-450 and by 2^450: every magnitude is out of the guard's range, every wave falls
     back. (A matrix that scales by 2^+-450 has no determinant in f64, so the scaled inverses are written directly: every
     factor is a power of two, the products are exact.)
  c. one element of the view's rotation block is 1e-170 and the camera stands 3.4e-155 above y = 0: the y component of a
     pixel's direction is an exact zero where 1e-170 * world_x is absorbed by the origin's y and about 1e-171 where it is
     not — lanes of one wave on both sides of the guard.
The oracle's frames are computed first, once, and must be finite and hold hits, shadowed hits and misses in every setting."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = ((32, 16), (40, 24))
SETTINGS = ("ordinary", "scaled 2^-450", "scaled 2^450", "tiny element")
SRC_CULL, SRC_CULL2 = 3, 4
PADS = 300   # more than 256 objects: the default launch is the two-level cull


# ---- arithmetic -------------------------------------------------------------------------------------------------------
TINY = (2.0 ** -499, 2.0 ** -500, 2.0 ** -501, 2.0 ** -969, 2.0 ** -1022, 1e-310, 3e-320, 5e-324)
MAG_EXP = (399, 400, 401, 511, -399, -400, -401, -511)
SPECIAL = (math.inf, -math.inf, math.nan)


def _triples_of_kind(rng, kind, sub, n):
    """n triples of one kind; `sub` picks the kind's variant (one tiny value, one magnitude, one special value)."""
    v = rng.normal(size=(n, 3))
    rows = np.arange(n)
    if kind == 1:    # exact zeros and -0 components, at least one per triple, possibly all three
        z = rng.random((n, 3)) < 0.5
        z[rows, rng.integers(0, 3, n)] = True
        v = np.where(z, np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0), v)
    elif kind == 2:  # one tiny component (either sign) beside components of order 1
        v[rows, rng.integers(0, 3, n)] = TINY[sub % len(TINY)] * np.where(rng.random(n) < 0.5, 1.0, -1.0)
    elif kind == 3:  # the magnitude at a power of two: exactly (one component), and a little above it (a scaled direction)
        e = MAG_EXP[sub % len(MAG_EXP)]
        axis = np.zeros((n, 3))
        axis[rows, rng.integers(0, 3, n)] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        unit = v / np.sqrt((v * v).sum(axis=1))[:, None]
        v = np.where((rng.random(n) < 0.5)[:, None], axis, unit * (1.0 + rng.random((n, 1)) * 2.0 ** -40)) * 2.0 ** e
    elif kind == 4:  # inf and NaN components
        v[rows, rng.integers(0, 3, n)] = SPECIAL[sub % len(SPECIAL)]
    return v


def normalize_triples():
    """(n, 3) with n = 64 * 4096: the first half in waves of one kind (64 consecutive triples), the second half with every
    triple's kind drawn on its own."""
    rng = np.random.default_rng(20)
    waves = 4096
    out = np.empty((waves * 64, 3))
    for w in range(waves // 2):
        out[w * 64:(w + 1) * 64] = _triples_of_kind(rng, w % 5, w // 5, 64)
    n_mixed = (waves - waves // 2) * 64
    kinds = rng.integers(0, 5, n_mixed)
    subs = rng.integers(0, 24, n_mixed)
    mixed = out[waves // 2 * 64:]
    for k in range(5):
        for s in range(24):
            sel = np.flatnonzero((kinds == k) & (subs == s))
            mixed[sel] = _triples_of_kind(rng, k, s, len(sel))
    return out


def guard_passes(v):
    """vnormalize_shared's documented condition per triple (host arithmetic)."""
    with np.errstate(all="ignore"):
        mag = np.sqrt((v * v).sum(axis=1))
    comp = ((v == 0.0) | (np.abs(v) >= 2.0 ** -500)).all(axis=1)
    return comp & (mag >= 2.0 ** -400) & (mag <= 2.0 ** 400)


def _same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def test_wave_normalize_equals_three_divisions_and_the_host(gpu):
    v = normalize_triples()
    ok = guard_passes(v).reshape(-1, 64)
    whole_pass, whole_fail = int(ok.all(axis=1).sum()), int((~ok).all(axis=1).sum())
    mixed = len(ok) - whole_pass - whole_fail
    print(f"{len(v)} triples in {len(ok)} waves: {whole_pass} wholly inside the guard, {whole_fail} wholly outside, {mixed} mixed")
    assert whole_pass > 100 and whole_fail > 100 and mixed > 100
    for x in TINY + tuple(2.0 ** e for e in MAG_EXP):
        assert (np.abs(v) == x).any(), x
    assert (v == math.inf).any() and (v == -math.inf).any() and np.isnan(v).any()
    assert (v == 0.0).any() and np.signbit(v[v == 0.0]).any()
    flat = np.ascontiguousarray(v.reshape(-1))
    wave = gpu.device_arith(8, flat).reshape(-1, 3)
    plain = gpu.device_arith(6, flat).reshape(-1, 3)
    with np.errstate(all="ignore"):
        mag = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        host = v / mag[:, None]
    bad = np.flatnonzero(~_same_bits(wave, plain).all(axis=1))
    assert len(bad) == 0, (len(bad), v[bad[:4]].tolist(), wave[bad[:4]].tolist(), plain[bad[:4]].tolist())
    bad = np.flatnonzero(~_same_bits(wave, host).all(axis=1))
    assert len(bad) == 0, (len(bad), v[bad[:4]].tolist(), wave[bad[:4]].tolist(), host[bad[:4]].tolist())


# ---- frames -----------------------------------------------------------------------------------------------------------
def _scale_world(rtc, w, cam, s):
    """The World and camera scaled uniformly by s, a power of two: object-to-world S(s) M has the inverse M^-1 S(1/s), the
    camera's view_inv becomes S(s) view_inv, the light moves to s * position. Every product is exact."""
    out = rtc.World(rtc.light(position=tuple(s * p for p in w.light.position), intensity=tuple(w.light.intensity)))
    for sh in w.shapes:
        inv = np.array(list(sh.inv)).reshape(4, 4)
        inv[:3, :3] *= 1.0 / s
        for i in range(4):
            for j in range(4):
                sh.inv[4 * i + j] = inv[i, j]
                sh.inv_t[4 * i + j] = inv[j, i]
        out.add_shape(sh)
    vi = np.array(list(cam.view_inv)).reshape(4, 4)
    vi[:3, :] *= s
    for i in range(16):
        cam.view_inv[i] = vi.reshape(16)[i]
    return out, cam


def build(rtc, setting, size, padded):
    """(World, camera) of one setting: a sphere, a cube and a plane, matte; `padded`: PADS small spheres behind the camera."""
    M = rtc.Matrix
    W, H = size
    matte = lambda c: rtc.material(color=c, ambient=0.15, diffuse=0.8, specular=0.0)
    tiny = setting == "tiny element"
    down = -1.0 if tiny else 0.0   # (the tiny-element camera stands at y = 0: everything else moves down by 1)
    # the light just under the floating cube: shadowed and lit hits in the ordinary and in both scaled worlds (in the 2^-450
    # world over_point is normal * 1e-5, far outside the scene, and only a few of the oracle's shadow rays meet anything)
    w = rtc.World(rtc.light(position=(-6.0, 6.0, -5.0) if tiny else (0.9, 0.1, -0.4)))
    w.add_shape(rtc.sphere(M.identity().scaling(0.9, 0.9, 0.9).translation(-0.8, 0.9 + down, 0.6), matte((0.9, 0.3, 0.2))))
    w.add_shape(rtc.cube(M.identity().scaling(0.5, 0.5, 0.5).rotation_y(0.5).translation(0.9, 0.7 + down, -0.4), matte((0.2, 0.5, 0.9))))
    w.add_shape(rtc.plane(M.identity().translation(0.0, down, 0.0), matte((0.6, 0.6, 0.5))))
    if padded:
        for k in range(PADS):
            w.add_shape(rtc.sphere(M.identity().scaling(0.05, 0.05, 0.05).translation(-7.0 + 0.05 * k, 3.0 + 0.3 * (k % 7) + down, -14.0 - 0.2 * (k % 11)), matte((0.5, 0.5, 0.5))))
    if tiny:
        cam = rtc.camera(W, H, 1.2, M.make_view_transform((0.0, 0.0, -5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
        # row y of view_inv: direction.y = ((1e-170 * world_x + 0 * world_y) + 0 * -1 + oy) - oy, which is 0 where oy absorbs the product
        cam.view_inv[4], cam.view_inv[5], cam.view_inv[6], cam.view_inv[7] = 1e-170, 0.0, 0.0, 0.75 * 1e-170 * 2.0 ** 52
    else:
        cam = rtc.camera(W, H, 1.0, M.make_view_transform((0.3, 2.2, -5.5), (0.0, 1.5, 0.0), (0.0, 1.0, 0.0)))
    if setting.startswith("scaled"):
        w, cam = _scale_world(rtc, w, cam, 2.0 ** (-450 if "-450" in setting else 450))
    return w, cam


def _record(h):
    return (h.hit_index, h.shadowed, h.t, tuple(h.point), tuple(h.over_point), tuple(h.normal)) if h.hit_index >= 0 else (-1,)


def _bits(rec):
    return tuple(np.float64(x).view(np.uint64) if isinstance(x, float) else _bits(x) if isinstance(x, tuple) else x for x in rec)


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
                if setting == "ordinary":   # the sphere, the cube and the plane are all seen (a direction of 2^-450 or 1e-170 in
                    assert {r[0] for r in hits} >= {0, 1, 2}, (setting, size)   # object space is parallel to a plane for the reference)
                assert (canvas != 0).any() and (canvas == 0).any()
                if setting == "tiny element":   # lanes of one 8x8 tile, a wave's pixels, on both sides of the guard
                    dy = rays[:, 4].reshape(size[1], size[0])
                    tiles = [dy[:8, x:x + 8] for x in range(0, size[0], 8)]
                    assert any((t == 0.0).any() and ((t != 0.0) & (np.abs(t) < 2.0 ** -500)).any() for t in tiles), dy[0]
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
