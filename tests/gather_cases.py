"""Shared by tests/test_host_gather.py and tests/test_gpu_gather.py: the worlds and passes of the one-bounce gather tests and
what the CPU oracle says each pixel's planes hold. Every expected plane is computed once per (world, pass), cached and never
written to.

A case is (world name, (radius, usteps, vsteps)). The expectation comes from the oracle alone: per sample and per light
color_at(ray, 0, want_hit=True), summed in light order; the radius applied to the record's t; `base` from the oracle's
orc_pattern_at_shape at the primary over_point, or material.color; everything packed by rtc_gather_from_hits."""
import ctypes as C
import functools
import math

import numpy as np

import ao_cases as AO

INF = math.inf

# (world, (radius, usteps, vsteps)): frames of 33x19 (five tiles by three, the right and bottom ones masked) and 9x7
CASES = (
    ("bleed", (1.5, 2, 2)),          # three shapes, the one-level cull; about the scene's size
    ("bleed", (INF, 4, 4)),          # unbounded
    ("bleed", (1.5, 1, 1)),          # one sample per pixel: the normal itself
    ("bleed+2", (INF, 2, 2)),        # two lights: the kernel-argument block
    ("bleed+9", (1.5, 2, 2)),        # nine lights at a 3x3 area light's cells: the World's light table
    ("closeup", (0.25, 2, 2)),       # the small radius, seen from near the floor
    ("closeup:9x7", (1.5, 16, 16)),  # 256 samples: the cap
    ("grid290", (0.5, 2, 2)),        # 290 shapes: the two-level walk (at radius 1.0 the radius cuts 1 % of the samples: too few)
    ("grid290", (INF, 4, 4)),
    ("inside", (3.0, 4, 4)),         # the camera inside a sphere: every sample hits, `inside` set on the shell's hits
    ("inside", (INF, 2, 2)),
)
SERIAL_CASES = (("bleed", (1.5, 2, 2)), ("grid290", (0.5, 2, 2)))  # also rendered under RTC_MODE_RENDER
IDS = [f"{n}-{a[0]}-{a[1]}x{a[2]}" for n, a in CASES]

RED, GREEN, BLUE, WHITE = (0.9, 0.15, 0.1), (0.1, 0.8, 0.2), (0.15, 0.2, 0.9), (1.0, 1.0, 1.0)


def _size(name, default):
    if ":" not in name:
        return name, default
    base, size = name.split(":")
    return base, tuple(int(v) for v in size.split("x"))


def bleed_shapes(rtc):
    """ao_cases' contact geometry in colour: a white checker floor without highlights, a red sphere and a cube striped green
    and blue resting on it."""
    M = rtc.Matrix
    floor = rtc.material(specular=0.0, pattern=("checker", WHITE, (0.75, 0.75, 0.75), None))
    ball = rtc.material(color=RED, diffuse=0.8, specular=0.3)
    box = rtc.material(diffuse=0.8, specular=0.2, pattern=("stripe", GREEN, BLUE, M.identity().scaling(0.25, 0.25, 0.25)))
    return [rtc.plane(M.identity(), floor), rtc.sphere(M.identity().translation(-1.1, 1.0, 0.0), ball),
            rtc.cube(M.identity().scaling(0.8, 0.8, 0.8).rotation_y(0.4).translation(1.1, 0.8, 0.3), box)]


BLEED_LIGHTS = {
    "bleed": lambda rtc: [rtc.light((-10.0, 10.0, -10.0))],
    "bleed+2": lambda rtc: [rtc.light((-10.0, 10.0, -10.0)), rtc.light((8.0, 6.0, -4.0), (0.5, 0.5, 0.5))],
    "bleed+9": lambda rtc: [rtc.area_light((-2.0, 6.0, -6.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), 3, 3)],
}


@functools.lru_cache(maxsize=None)
def world(rtc, name):
    """(World, camera). "bleed" (and "bleed+2", "bleed+9": the same shapes under other lights), "closeup" (the same shapes from
    near the floor), "grid290" (ao_cases' grid with red, green and blue shapes in turn), "inside" (a ring-patterned shell with
    coloured contents), each optionally with ":WxH"."""
    M = rtc.Matrix
    base, (width, height) = _size(name, (33, 19))
    if base in BLEED_LIGHTS or base == "closeup":
        w = rtc.World(BLEED_LIGHTS[base](rtc) if base in BLEED_LIGHTS else rtc.light((-10.0, 10.0, -10.0)))
        for s in bleed_shapes(rtc):
            w.add_shape(s)
        _, cam = AO.world(rtc, ("contact" if base in BLEED_LIGHTS else "closeup") + f":{width}x{height}")
        return w, cam
    if base == "grid290":
        src, cam = AO.world(rtc, f"grid290:{width}x{height}")
        w = rtc.World(rtc.light((-10.0, 10.0, -10.0)))
        w.add_shape(rtc.plane(M.identity(), rtc.material(specular=0.0)))
        for i in range(17):
            for j in range(17):
                x, z = i - 8.0, j - 8.0
                mat = rtc.material(color=(RED, GREEN, BLUE)[(i * 17 + j) % 3], specular=0.4)
                if (i + j) % 2:
                    w.add_shape(rtc.sphere(M.identity().scaling(0.45, 0.45, 0.45).translation(x, 0.45, z), mat))
                else:
                    w.add_shape(rtc.cube(M.identity().scaling(0.4, 0.35, 0.4).translation(x, 0.35, z), mat))
        assert len(w) == len(src)
        return w, cam
    if base == "inside":
        _, cam = AO.world(rtc, f"inside:{width}x{height}")
        w = rtc.World(rtc.light((0.0, 2.0, 0.0)))
        shell = rtc.material(specular=0.1, pattern=("ring", (0.9, 0.8, 0.3), (0.3, 0.5, 0.9), M.identity().scaling(0.2, 0.2, 0.2)))
        w.add_shape(rtc.sphere(M.identity().scaling(4, 4, 4), shell))
        w.add_shape(rtc.sphere(M.identity().translation(0.0, -1.0, 2.8284271247461903), rtc.material(color=RED)))
        w.add_shape(rtc.cube(M.identity().scaling(0.5, 0.5, 0.5).rotation_y(0.6).translation(-1.2, 0.3, 1.5), rtc.material(color=GREEN)))
        return w, cam
    raise KeyError(name)


_cache = {}


def oracle_hits(rtc, O, name):
    """The oracle's hit records for the centre rays of world `name` through its camera (an RtcHit array, row-major)."""
    k = (name, "hits")
    if k not in _cache:
        w, cam = world(rtc, name)
        arr, n, lgt = w.array(), len(w), w.samples()[0]
        npx = cam.hsize * cam.vsize
        hits = (rtc.RtcHit * npx)()
        for y in range(cam.vsize):
            for x in range(cam.hsize):
                _, h = O.color_at(arr, n, lgt, tuple(rtc.ray_for_pixel(cam, x, y)), 0, want_hit=True)
                C.memmove(C.byref(hits, (y * cam.hsize + x) * C.sizeof(rtc.RtcHit)), C.byref(h), C.sizeof(rtc.RtcHit))
        _cache[k] = hits
    return _cache[k]


def hit_mask(rtc, O, name):
    w, cam = world(rtc, name)
    hits = oracle_hits(rtc, O, name)
    return np.array([hits[i].hit_index >= 0 for i in range(cam.hsize * cam.vsize)]).reshape(cam.vsize, cam.hsize)


def albedo(rtc, O, name):
    """(npx, 3), read-only: base * diffuse of every pixel's primary hit from the oracle — orc_pattern_at_shape at the record's
    over_point (the point shade_hit passes to lighting) or material.color; zeros for a miss."""
    k = (name, "albedo")
    if k not in _cache:
        w, cam = world(rtc, name)
        hits = oracle_hits(rtc, O, name)
        arr = w.array()
        out = np.zeros((cam.hsize * cam.vsize, 3))
        L = O.lib()
        for i in range(cam.hsize * cam.vsize):
            h = hits[i]
            if h.hit_index < 0:
                continue
            shape = arr[h.hit_index]
            m = shape.material
            if m.pattern_kind != 0:
                col = type(h.over_point)()
                L.orc_pattern_at_shape(C.byref(m), C.byref(shape), h.over_point, col)
                base = np.array(list(col))
            else:
                base = np.array(list(m.color))
            out[i] = base * np.float64(m.diffuse)
        out.setflags(write=False)
        _cache[k] = out
    return _cache[k]


def oracle_samples(rtc, O, name, ao):
    """(sample RtcHit array [npx * n], colours (npx * n, 3), shadowed-by-the-first-light flags) of the oracle, read-only: for
    every pixel that hits and every sample k, rtc_ao_ray of the ORACLE's normal and over_point, then color_at(ray, 0) once per
    light sample of the World, the colours summed in light order. The record is the first light's (it does not depend on
    the light but for `shadowed`)."""
    radius, usteps, vsteps = ao
    k = (name, (usteps, vsteps), "samples")
    if k not in _cache:
        w, cam = world(rtc, name)
        hits = oracle_hits(rtc, O, name)
        arr, n, lights = w.array(), len(w), w.samples()
        dirs = rtc.ao_expand(rtc.ao(1.0, usteps, vsteps))
        ns, npx = usteps * vsteps, cam.hsize * cam.vsize
        recs = (rtc.RtcHit * (npx * ns))()
        rgb = np.zeros((npx * ns, 3))
        size = C.sizeof(rtc.RtcHit)
        for i in range(npx):
            h = hits[i]
            if h.hit_index < 0:
                for s in range(ns):
                    recs[i * ns + s].hit_index = -1
                continue
            normal, over = tuple(h.normal), tuple(h.over_point)
            for s, local in enumerate(dirs):
                ray = tuple(rtc.ao_ray(normal, over, local))
                total = None
                for li, lgt in enumerate(lights):
                    col, rec = O.color_at(arr, n, lgt, ray, 0, want_hit=True)
                    if li == 0:
                        C.memmove(C.byref(recs, (i * ns + s) * size), C.byref(rec), size)
                        total = col
                    else:
                        total = total + col   # f64, in light order
                rgb[i * ns + s] = total
        rgb.setflags(write=False)
        _cache[k] = (recs, rgb)
    return _cache[k]


def expected(rtc, O, name, ao, mode):
    """{"radiance", "bounce"}: (vsize, hsize, 3) read-only planes, rtc_gather_from_hits of the oracle's records and colours."""
    radius, usteps, vsteps = ao
    k = (name, ao, mode)
    if k not in _cache:
        w, cam = world(rtc, name)
        recs, rgb = oracle_samples(rtc, O, name, ao)
        planes = rtc.gather_from_hits(oracle_hits(rtc, O, name), recs, rgb, albedo(rtc, O, name), usteps * vsteps, radius,
                                      cam.hsize, cam.vsize, mode)
        for a in planes.values():
            a.setflags(write=False)
        _cache[k] = planes
    return _cache[k]


def shares(rtc, O, name, ao):
    """What the oracle says a case exercises, as shares: of the pixels that hit — nonzero radiance, channels that differ by
    more than 0.01; of the samples of those pixels — counted (a hit inside the radius), cut (a hit at or beyond it); of the
    counted samples — shadowed from the first light."""
    radius, usteps, vsteps = ao
    ns = usteps * vsteps
    w, cam = world(rtc, name)
    mask = hit_mask(rtc, O, name).reshape(-1)
    rad = expected(rtc, O, name, ao, 1)["radiance"].reshape(-1, 3)[mask]
    recs, _ = oracle_samples(rtc, O, name, ao)
    rec = np.frombuffer(recs, dtype=AO.A.HIT_DTYPE).reshape(-1, ns)[mask]
    has = rec["hit_index"] >= 0
    counted = has & (rec["t"] < radius)
    cut = has & ~counted
    return {"pixels": int(mask.sum()), "nonzero": float((rad != 0.0).any(axis=1).mean()),
            "spread": float(((rad.max(axis=1) - rad.min(axis=1)) > 0.01).mean()),
            "counted": float(counted.mean()), "cut": float(cut.mean()),
            "shadowed": float((rec["shadowed"][counted] != 0).mean()) if counted.any() else 0.0,
            "n_lights": len(w.samples())}


def conditions(rtc, O, name, ao):
    """The conditions a case misses (empty: a good case), from the oracle alone."""
    s = shares(rtc, O, name, ao)
    missed = []
    if s["pixels"] == 0:
        return ["no pixel hits"]
    if s["nonzero"] < 0.1: missed.append("nonzero radiance on 10 %% of the hit pixels (%.2f)" % s["nonzero"])
    if s["spread"] < 0.1: missed.append("a channel spread on 10 %% of the hit pixels (%.2f)" % s["spread"])
    if s["counted"] < 0.1: missed.append("10 %% of the samples counted (%.2f)" % s["counted"])
    if s["counted"] > 0.9 and not name.startswith("inside"): missed.append("at most 90 %% of the samples counted (%.2f)" % s["counted"])
    if s["n_lights"] == 1:
        if s["shadowed"] < 0.1: missed.append("10 %% of the counted hits shadowed (%.2f)" % s["shadowed"])
        if s["shadowed"] > 0.9: missed.append("10 %% of the counted hits lit (%.2f)" % (1.0 - s["shadowed"]))
    if ao[0] != INF and s["cut"] < 0.05: missed.append("5 %% of the samples cut by the radius (%.2f)" % s["cut"])
    return missed
