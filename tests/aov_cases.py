"""Shared by tests/test_host_aov.py and tests/test_gpu_aov.py: the worlds of the AOV tests and what the CPU oracle says
each pixel's centre ray saw. Every expected record is computed once per (world, frame), cached and never written to."""
import ctypes as C
import functools
import importlib
import math

import numpy as np

PLANES = ("index", "depth", "point", "normal", "flags", "shadow")

# rtc_hit as a numpy record (include/rtc.h), for the numpy restatement of the packing rule
HIT_DTYPE = np.dtype([("hit_index", "<i4"), ("inside", "<u4"), ("shadowed", "<u4"), ("_pad", "<u4"), ("t", "<f8"), ("point", "<f8", 3),
                      ("over_point", "<f8", 3), ("under_point", "<f8", 3), ("eyev", "<f8", 3), ("normal", "<f8", 3), ("reflectv", "<f8", 3),
                      ("n1", "<f8"), ("n2", "<f8")])
assert HIT_DTYPE.itemsize == 184


def scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


def _with_lights(rtc, w, lights):
    m = rtc.World(lights)
    m.shapes = w.shapes
    return m


@functools.lru_cache(maxsize=None)
def world(rtc, name):
    """(World, camera) of one row of the issue's table."""
    S, M = scenes(rtc), rtc.Matrix
    if name == "mixed": return S.mixed(36, 20)
    if name == "s21": return S.synthetic(20, 33, 19)
    if name.startswith("s21:"):  # the same 21 objects at another frame size, "s21:WxH"
        width, height = (int(v) for v in name[4:].split("x"))
        return S.synthetic(20, width, height)
    if name == "default": return S.default_scene(20, 12)
    if name == "shell":  # the camera inside a scale-10 sphere, a cube and a sphere in front of it, the light inside too
        w = rtc.World(rtc.light((0.0, 3.0, 0.0)))
        w.add_shape(rtc.sphere(M.identity().scaling(10, 10, 10)))
        w.add_shape(rtc.cube(M.identity().translation(0, -1, 3)))
        w.add_shape(rtc.sphere(M.identity().translation(0, 1.5, 3).scaling(1, 1, 1)))
        return w, rtc.camera(17, 9, math.pi / 2, M.make_view_transform((0., 0., -5.), (0., 0., 0.), (0., 1., 0.)))
    if name == "s301": return S.synthetic(300, 40, 24)
    if name == "twice":  # 150 spheres inserted twice (indices j and j + 150), then the floor: ties under the Morton-ordered walk
        w0, cam = S.synthetic(150, 40, 24)
        spheres = [s for s in w0.shapes if s.kind != rtc.PLANE]
        w = rtc.World(w0.light)
        for s in spheres + spheres + [s for s in w0.shapes if s.kind == rtc.PLANE]:
            w.add_shape(s)
        return w, cam
    if name == "s40x2":  # a second light at (8, 6, -4)
        w, cam = S.synthetic(39, 33, 19)
        return _with_lights(rtc, w, [w.light, rtc.light((8.0, 6.0, -4.0), (0.5, 0.5, 0.5))]), cam
    if name == "s40area9":  # a 3x3 area light: 9 samples, the device-table path
        w, cam = S.synthetic(39, 33, 19)
        return _with_lights(rtc, w, [rtc.area_light((-11.0, 10.0, -11.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), 3, 3)]), cam
    if name == "s40area256":  # 16x16: the cap
        w, cam = S.synthetic(39, 16, 8)
        return _with_lights(rtc, w, [rtc.area_light((-2.0, 6.0, -6.0), (6.0, 0.0, 0.0), (0.0, 0.0, 6.0), 16, 16)]), cam
    raise KeyError(name)


_cache = {}


def oracle_hits(rtc, O, name):
    """(RtcHit array, uint16 shadow counts) of the oracle for the centre rays of world `name` through its camera:
    color_at(..., want_hit=True) per pixel, once per light sample for the counts."""
    w, cam = world(rtc, name)
    k = (name, "hits")
    if k not in _cache:
        arr, n = w.array(), len(w)
        lights = w.samples()
        npx = cam.hsize * cam.vsize
        hits = (rtc.RtcHit * npx)()
        counts = np.zeros(npx, dtype=np.uint16)
        for y in range(cam.vsize):
            for x in range(cam.hsize):
                ray = tuple(rtc.ray_for_pixel(cam, x, y))
                i = y * cam.hsize + x
                for li, lgt in enumerate(lights):
                    _, h = O.color_at(arr, n, lgt, ray, 5, want_hit=True)
                    if li == 0:
                        C.memmove(C.byref(hits, i * C.sizeof(rtc.RtcHit)), C.byref(h), C.sizeof(rtc.RtcHit))
                    if h.hit_index >= 0:
                        counts[i] += int(h.shadowed)
        counts.setflags(write=False)
        _cache[k] = (hits, counts)
    return _cache[k]


def expected(rtc, O, name, mode):
    """The expected planes: rtc_aov_from_hits of the oracle's records (read-only arrays)."""
    w, cam = world(rtc, name)
    k = (name, mode, "planes")
    if k not in _cache:
        hits, counts = oracle_hits(rtc, O, name)
        planes = rtc.aov_from_hits(hits, cam.hsize, cam.vsize, mode, shadow_counts=counts)
        for a in planes.values():
            a.setflags(write=False)
        _cache[k] = planes
    return _cache[k]


def same_planes(got, want, planes=PLANES):
    """Exact comparison (np.array_equal; +inf == +inf), plane by plane: the names of the planes that differ."""
    return [p for p in planes if not (got[p].dtype == want[p].dtype and got[p].shape == want[p].shape and np.array_equal(got[p], want[p]))]
