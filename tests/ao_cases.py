"""Shared by tests/test_host_ao.py and tests/test_gpu_ao.py: the worlds and passes of the ambient-occlusion tests and what the
CPU oracle says each pixel's plane entry is. Every expected plane is computed once per (world, pass), cached and never
written to. The worlds of tests/aov_cases.py are available under their names there.

A case is (world name, (radius, usteps, vsteps)). CASES are the ones the GPU tests render; test_host_ao.py checks, with the
oracle alone, that each of them exercises the count: see `conditions`."""
import ctypes as C
import functools
import math

import numpy as np

import aov_cases as A

INF = math.inf

# (world, (radius, usteps, vsteps)): frames of 33x19 (five tiles by three, the right and bottom ones masked) and 9x7
CASES = (
    ("closeup", (0.25, 2, 2)),      # three shapes, the one-level cull; the small radius, seen from near the floor
    ("contact", (1.5, 1, 1)),       # one sample per pixel
    ("contact", (1.5, 2, 2)),       # about the scene's size
    ("contact", (INF, 4, 4)),       # unbounded
    ("closeup:9x7", (0.25, 16, 16)),  # 256 samples: the cap
    ("grid290", (0.25, 2, 2)),      # 290 shapes: the two-level walk
    ("grid290", (1.0, 4, 4)),
    ("grid290", (INF, 2, 2)),
    ("grid290:9x7", (1.0, 16, 16)),
    ("inside", (3.0, 4, 4)),        # the camera inside a sphere: `inside` set, the normal flipped
    ("inside", (4.0, 2, 2)),
)
SERIAL_CASES = (("inside", (3.0, 4, 4)), ("grid290", (1.0, 4, 4)))  # also rendered under RTC_MODE_RENDER


def _size(name, default):
    if ":" not in name:
        return name, default
    base, size = name.split(":")
    return base, tuple(int(v) for v in size.split("x"))


def contact_shapes(rtc):
    """A floor, a unit sphere resting on it and a cube resting on it, a little apart."""
    M = rtc.Matrix
    return [rtc.plane(M.identity()), rtc.sphere(M.identity().translation(-1.1, 1.0, 0.0)),
            rtc.cube(M.identity().scaling(0.8, 0.8, 0.8).rotation_y(0.4).translation(1.1, 0.8, 0.3))]


@functools.lru_cache(maxsize=None)
def world(rtc, name):
    """(World, camera). Own names: "contact" (and "contact+2", "contact+area256": the same shapes under other lights),
    "closeup", "grid290", "inside", each optionally with ":WxH"; any other name is aov_cases'."""
    M = rtc.Matrix
    base, (width, height) = _size(name, (33, 19))
    if base.startswith("contact"):
        lights = {"contact": [rtc.light((-10.0, 10.0, -10.0))],
                  "contact+2": [rtc.light((-10.0, 10.0, -10.0)), rtc.light((8.0, 6.0, -4.0), (0.5, 0.5, 0.5))],
                  "contact+area256": [rtc.area_light((-2.0, 6.0, -6.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), 16, 16)]}[base]
        w = rtc.World(lights)
        for s in contact_shapes(rtc):
            w.add_shape(s)
        return w, rtc.camera(width, height, 0.9, M.make_view_transform((0.0, 2.2, -5.5), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)))
    if base == "closeup":  # the same shapes from near the floor, looking under the sphere at where it rests
        w = rtc.World(rtc.light((-10.0, 10.0, -10.0)))
        for s in contact_shapes(rtc):
            w.add_shape(s)
        return w, rtc.camera(width, height, 0.5, M.make_view_transform((-0.9, 0.3, -2.4), (-1.0, 0.1, -0.2), (0.0, 1.0, 0.0)))
    if base == "grid290":  # 17 x 17 cubes and spheres in turn, a unit apart, resting on a floor: 290 shapes, seen from above
        w = rtc.World(rtc.light((-10.0, 10.0, -10.0)))
        w.add_shape(rtc.plane(M.identity()))
        for i in range(17):
            for j in range(17):
                x, z = i - 8.0, j - 8.0
                if (i + j) % 2:
                    w.add_shape(rtc.sphere(M.identity().scaling(0.45, 0.45, 0.45).translation(x, 0.45, z)))
                else:
                    w.add_shape(rtc.cube(M.identity().scaling(0.4, 0.35, 0.4).translation(x, 0.35, z)))
        return w, rtc.camera(width, height, 0.5, M.make_view_transform((1.3, 9.0, -5.0), (0.2, 0.0, 0.3), (0.0, 1.0, 0.0)))
    if base == "inside":  # the camera inside a scale-4 sphere; a sphere resting against its wall and a cube in the middle
        w = rtc.World(rtc.light((0.0, 2.0, 0.0)))
        w.add_shape(rtc.sphere(M.identity().scaling(4, 4, 4)))
        w.add_shape(rtc.sphere(M.identity().translation(0.0, -1.0, 2.8284271247461903)))   # |centre| = 3: touches the shell
        w.add_shape(rtc.cube(M.identity().scaling(0.5, 0.5, 0.5).rotation_y(0.6).translation(-1.2, 0.3, 1.5)))
        return w, rtc.camera(width, height, 1.3, M.make_view_transform((0.3, 0.2, -2.5), (0.0, -0.3, 2.0), (0.0, 1.0, 0.0)))
    return A.world(rtc, name)


_cache = {}


def oracle_hits(rtc, O, name):
    """The oracle's hit records for the centre rays of world `name` through its camera, as aov_cases.oracle_hits takes them:
    one color_at(..., want_hit=True) per pixel."""
    k = (name, "hits")
    if k not in _cache:
        w, cam = world(rtc, name)
        arr, n, lgt = w.array(), len(w), w.samples()[0]
        npx = cam.hsize * cam.vsize
        hits = (rtc.RtcHit * npx)()
        for y in range(cam.vsize):
            for x in range(cam.hsize):
                _, h = O.color_at(arr, n, lgt, tuple(rtc.ray_for_pixel(cam, x, y)), 0, want_hit=True)
                i = y * cam.hsize + x
                C.memmove(C.byref(hits, i * C.sizeof(rtc.RtcHit)), C.byref(h), C.sizeof(rtc.RtcHit))
        _cache[k] = hits
    return _cache[k]


def expected_ao(rtc, O, name, ao, mode):
    """The expected plane (read-only): rtc_ao_from_hits of the oracle's centre-ray records and, per pixel that hits, the number
    of samples whose rtc_ao_ray (of the ORACLE's normal and over_point) the oracle answers with a hit at t < radius."""
    radius, usteps, vsteps = ao
    k = (name, ao, mode)
    if k not in _cache:
        w, cam = world(rtc, name)
        kc = (name, ao, "counts")
        if kc not in _cache:
            hits = oracle_hits(rtc, O, name)
            arr, n, lgt = w.array(), len(w), w.samples()[0]
            dirs = rtc.ao_expand(rtc.ao(radius, usteps, vsteps))
            counts = np.zeros(cam.hsize * cam.vsize, dtype=np.uint16)
            for i in range(cam.hsize * cam.vsize):
                h = hits[i]
                if h.hit_index < 0:
                    continue
                normal, over = tuple(h.normal), tuple(h.over_point)
                for local in dirs:
                    _, s = O.color_at(arr, n, lgt, tuple(rtc.ao_ray(normal, over, local)), 0, want_hit=True)
                    if s.hit_index >= 0 and s.t < radius:
                        counts[i] += 1
            counts.setflags(write=False)
            _cache[kc] = counts
        plane = rtc.ao_from_hits(oracle_hits(rtc, O, name), _cache[kc], cam.hsize, cam.vsize, mode)
        plane.setflags(write=False)
        _cache[k] = plane
    return _cache[k]


def hit_mask(rtc, O, name):
    w, cam = world(rtc, name)
    hits = oracle_hits(rtc, O, name)
    return np.array([hits[i].hit_index >= 0 for i in range(cam.hsize * cam.vsize)]).reshape(cam.vsize, cam.hsize)


def conditions(rtc, O, name, ao):
    """What a case must show, from the oracle alone; returns the list of conditions it misses (empty: a good case).
    With n >= 4 samples: the plane holds 0, holds n or at least one count >= 3n/4, holds counts strictly between, and at least
    10 % of the pixels that hit have 0 < count < n. No integer lies strictly between 0 and 1, so a one-sample pass has to hold
    both 0 and 1, each on at least 10 % of the pixels that hit."""
    radius, usteps, vsteps = ao
    n = usteps * vsteps
    plane = expected_ao(rtc, O, name, ao, 1)
    c = plane[hit_mask(rtc, O, name)]
    missed = []
    if c.size == 0:
        return ["no pixel hits"]
    if n == 1:
        if (c == 0).mean() < 0.1: missed.append("10 % open")
        if (c == 1).mean() < 0.1: missed.append("10 % occluded")
        return missed
    if not (c == 0).any(): missed.append("a 0")
    if not (4 * c >= 3 * n).any(): missed.append("a count >= 3n/4")
    between = (c > 0) & (c < n)
    if not between.any(): missed.append("a count strictly between")
    if between.mean() < 0.1: missed.append("10 %% between (%.1f %%)" % (100 * between.mean()))
    return missed
