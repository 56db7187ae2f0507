"""Shared by tests/test_gpu_projection_passes.py: what the CPU oracle says the AOV, ambient-occlusion and gather passes hold
under an orthographic or panorama camera. The cases are tests/projection_cases.py's (CASES, build); a pixel's ray is
rtc_projection_ray's, its records the oracle's color_at(ray, want_hit=True), packed by the library's normative host
functions (rtc_aov_from_hits, rtc_ao_from_hits, rtc_gather_from_hits) exactly as tests/aov_cases.py, tests/ao_cases.py and
tests/gather_cases.py pack the pinhole's. Everything is computed once per key, cached and read-only. No GPU."""
import ctypes as C

import numpy as np

import projection_cases as PC

AMONG = ((1.5, 1.25, 4.0), (0.2, 0.45, 0.7))                                                # a second light among the shapes
A33 = ((-11.5, 10.0, -11.5), (3.0, 0.0, 0.0), (0.0, 0.5, 3.0), 3, 3, (1.0, 0.95, 0.9))      # a 3x3 area light: the light table
LIGHTS = ("one", "two", "nine")

_cache = {}


def build(rtc, name, lights="one"):
    """(World, camera, projection) of projection_cases' case `name` under its own light ("one"), with a second light in the
    kernel arguments ("two"), or under a 3x3 area light, nine samples from the World's device table ("nine")."""
    k = (name, lights, "world")
    if k not in _cache:
        w, cam, proj = PC.build(rtc, name)
        if lights != "one":
            own = rtc.light(position=tuple(w.light.position), intensity=tuple(w.light.intensity))
            m = rtc.World([own, rtc.light(position=AMONG[0], intensity=AMONG[1])] if lights == "two" else [rtc.area_light(*A33)])
            m.shapes = w.shapes
            w = m
        _cache[k] = (w, cam, proj)
    return _cache[k]


def rays(rtc, name):
    """(npx, 6), row-major: rtc_projection_ray of every pixel"""
    k = (name, "rays")
    if k not in _cache:
        _, cam, proj = PC.build(rtc, name)
        out = np.empty((cam.vsize * cam.hsize, 6))
        ray, fn, camr, projr = (C.c_double * 6)(), rtc.lib().rtc_projection_ray, C.byref(cam), C.byref(proj)
        for y in range(cam.vsize):
            for x in range(cam.hsize):
                assert fn(camr, projr, x, y, ray) == 0
                out[y * cam.hsize + x] = ray[:]
        out.setflags(write=False)
        _cache[k] = out
    return _cache[k]


def oracle_hits(rtc, O, name, lights="one"):
    """(RtcHit array, uint16 shadow counts): the oracle's record of every pixel's ray and how many of the World's light
    samples are hidden from its over_point (one color_at per sample, as tests/aov_cases.py counts them)."""
    k = (name, lights, "hits")
    if k not in _cache:
        w, cam, _ = build(rtc, name, lights)
        arr, n, samples, size = w.array(), len(w), w.samples(), C.sizeof(rtc.RtcHit)
        r = rays(rtc, name)
        hits = (rtc.RtcHit * len(r))()
        counts = np.zeros(len(r), dtype=np.uint16)
        for i in range(len(r)):
            ray = tuple(r[i])
            for li, lgt in enumerate(samples):
                _, h = O.color_at(arr, n, lgt, ray, 0, want_hit=True)
                if li == 0:
                    C.memmove(C.byref(hits, i * size), C.byref(h), size)
                if h.hit_index < 0:
                    break
                counts[i] += int(h.shadowed)
        counts.setflags(write=False)
        _cache[k] = (hits, counts)
    return _cache[k]


def expected_aov(rtc, O, name, mode, lights="one"):
    """The six planes: rtc_aov_from_hits of the oracle's records"""
    k = (name, lights, mode, "aov")
    if k not in _cache:
        _, cam, _ = build(rtc, name, lights)
        hits, counts = oracle_hits(rtc, O, name, lights)
        planes = rtc.aov_from_hits(hits, cam.hsize, cam.vsize, mode, shadow_counts=counts)
        for a in planes.values():
            a.setflags(write=False)
        _cache[k] = planes
    return _cache[k]


def expected_ao(rtc, O, name, ao, mode):
    """The count plane of the pass `ao` = (radius, usteps, vsteps): per pixel that hits, the samples whose rtc_ao_ray (of the
    ORACLE's normal and over_point) the oracle answers with a hit at t < radius; packed by rtc_ao_from_hits."""
    radius, usteps, vsteps = ao
    k = (name, ao, mode, "ao")
    if k not in _cache:
        w, cam, _ = build(rtc, name)
        hits, _ = oracle_hits(rtc, O, name)
        kc = (name, ao, "ao counts")
        if kc not in _cache:
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
        plane = rtc.ao_from_hits(hits, _cache[kc], cam.hsize, cam.vsize, mode)
        plane.setflags(write=False)
        _cache[k] = plane
    return _cache[k]


def _albedo(O, w, hits, npx):
    """base * diffuse of every pixel's hit (tests/gather_cases.py's rule): the pattern at over_point, or the material's colour"""
    arr, L = w.array(), O.lib()
    out = np.zeros((npx, 3))
    for i in range(npx):
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
    return out


def expected_gather(rtc, O, name, ao, mode, lights="one"):
    """{"radiance", "bounce"}: rtc_gather_from_hits of the oracle's records — per pixel that hits and per sample, color_at(
    rtc_ao_ray, 0) once per light sample, summed in light order."""
    radius, usteps, vsteps = ao
    k = (name, lights, ao, mode, "gather")
    if k not in _cache:
        w, cam, _ = build(rtc, name, lights)
        hits, _ = oracle_hits(rtc, O, name, lights)
        arr, n, samples, size = w.array(), len(w), w.samples(), C.sizeof(rtc.RtcHit)
        dirs = rtc.ao_expand(rtc.ao(1.0, usteps, vsteps))
        ns, npx = usteps * vsteps, cam.hsize * cam.vsize
        recs = (rtc.RtcHit * (npx * ns))()
        rgb = np.zeros((npx * ns, 3))
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
                for li, lgt in enumerate(samples):
                    col, rec = O.color_at(arr, n, lgt, ray, 0, want_hit=True)
                    if li == 0:
                        C.memmove(C.byref(recs, (i * ns + s) * size), C.byref(rec), size)
                        total = col
                        if rec.hit_index < 0:
                            break   # (a sample that meets nothing: black under every light)
                    else:
                        total = total + col   # f64, in light order
                rgb[i * ns + s] = total
        planes = rtc.gather_from_hits(hits, recs, rgb, _albedo(O, w, hits, npx), ns, radius, cam.hsize, cam.vsize, mode)
        for a in planes.values():
            a.setflags(write=False)
        _cache[k] = planes
    return _cache[k]
