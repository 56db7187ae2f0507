"""The cases of the projection tests (tests/test_host_projection.py, tests/test_gpu_projection.py): Worlds, cameras and
projections, the reference frames — the oracle's color_at of one normative ray per pixel, computed once, shared, never
written to — a Python restatement of include/rtc.h's projection arithmetic with the mistakes a kernel could make, and the
angles of each 8x8 tile's rays as make_bundle sees them. No GPU.

Cameras stand among the shapes, so a panorama sees geometry in every direction. rtc.camera's field of view is not read by a
projection; 1.0 everywhere."""
import ctypes as C
import functools
import importlib
import math
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

from adversarial_worlds import shape_frame, straddled_sphere

MODE_RENDER, MODE_RENDER_ASYNC = 0, 1
ORTHO, PANO = 1, 2
W, H = 70, 45
TIGHT_TOL = 1e-12  # per light (tests/test_gpu_lights.py, tests/test_gpu_parity.py)
TWO_PI, PI = 2.0 * math.pi, math.pi


@dataclass(frozen=True)
class Case:
    world: str            # _world's name
    size: tuple           # (hsize, vsize)
    kind: int
    spec: tuple           # orthographic: (width,); panorama: (h_span, v_span)
    view: tuple | None    # (from, to, up); None: the camera is built by the case's own rule (straddle)
    source: int = 3       # rtc_launch_info::source of the culled launch


# views: a panorama's `from` is inside the cloud of shapes; an orthographic view looks at the whole scene
FLAT_AMONG = ((0.3, 1.2, 8.0), (0.0, 1.0, 20.0), (0.0, 1.0, 0.0))       # synthetic(39): x -10..10, on the floor, z -5..25
FLAT_ABOVE = ((0.0, 6.0, -8.0), (0.0, 0.5, 10.0), (0.0, 1.0, 0.0))
MIXED_AMONG = ((0.2, 1.4, 2.0), (1.0, 1.2, 6.0), (0.0, 1.0, 0.0))       # mixed: x -4..4, y 0.2..2.7, z -2..6
MIXED_FRONT = ((0.5, 2.5, -7.0), (0.0, 1.0, 1.0), (0.0, 1.0, 0.0))
CRIT_AMONG = ((0.3, 1.0, -1.5), (-0.5, 1.0, 0.5), (0.0, 1.0, 0.0))      # criterion: three spheres round the origin, floor at y = -3
CRIT_ABOVE = ((0.0, 7.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0))
S300_AMONG = ((0.3, 3.0, 9.0), (0.0, 3.0, 20.0), (0.0, 1.0, 0.0))       # synthetic(299): y 0.15..8
S300_ABOVE = ((0.0, 9.0, -8.0), (0.0, 3.0, 10.0), (0.0, 1.0, 0.0))

CASES = {
    "flat-ortho": Case("flat", (W, H), ORTHO, (24.0,), FLAT_ABOVE),
    "flat-ortho-straddle": Case("flat", (W, H), ORTHO, (6.0,), None),    # the origin plane cuts through a sphere
    "flat-pano": Case("flat", (W, H), PANO, (TWO_PI, PI), FLAT_AMONG),
    "flat-pano-16x9": Case("flat", (16, 9), PANO, (TWO_PI, PI), FLAT_AMONG),    # a tile spans 180 degrees of longitude: B.off
    "flat-pano-32x16": Case("flat", (32, 16), PANO, (TWO_PI, PI), FLAT_AMONG),  # tiles in make_bundle's wide-but-bounded branch
    "flat-pano-window": Case("flat", (W, H), PANO, (PI / 2.0, PI / 3.0), FLAT_AMONG),   # all narrow
    "mixed-ortho": Case("mixed", (W, H), ORTHO, (10.0,), MIXED_FRONT),
    "mixed-pano": Case("mixed", (W, H), PANO, (TWO_PI, PI), MIXED_AMONG),
    "criterion-ortho": Case("criterion", (W, H), ORTHO, (8.0,), CRIT_ABOVE),
    "criterion-pano": Case("criterion", (W, H), PANO, (TWO_PI, PI), CRIT_AMONG),
    "s300-ortho": Case("s300", (40, 24), ORTHO, (26.0,), S300_ABOVE, source=4),
    "s300-pano": Case("s300", (40, 24), PANO, (TWO_PI, PI), S300_AMONG, source=4),
}
FLAT_CASES = [k for k, c in CASES.items() if c.world == "flat"]
STACK_CASES = [k for k, c in CASES.items() if c.world in ("mixed", "criterion")]
S300_CASES = [k for k, c in CASES.items() if c.world == "s300"]


def _scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


@functools.lru_cache(maxsize=None)
def _world(rtc, name):
    """(World, the scene's own pinhole camera at 70x45)"""
    S = _scenes(rtc)
    if name == "flat": return S.synthetic(39, W, H)
    if name == "mixed": return S.mixed(W, H)
    if name == "criterion": return S.criterion(W, H)
    if name == "s300": return S.synthetic(299, 40, 24)
    raise KeyError(name)


def make_projection(rtc, kind, spec):
    return rtc.projection(kind, width=spec[0]) if kind == ORTHO else rtc.projection(kind, h_span=spec[0], v_span=spec[1])


@functools.lru_cache(maxsize=None)
def build(rtc, name):
    """(World, camera, projection) of case `name`"""
    c = CASES[name]
    w, pin = _world(rtc, c.world)
    view = c.view
    if view is None:   # the z = 0 plane of the camera passes through the centre of a sphere in front of the scene's pinhole camera
        i = straddled_sphere(rtc, w, pin)
        assert i is not None
        _, centre, _ = shape_frame(rtc, w.shapes[i])
        frm = tuple(float(v) for v in centre)
        view = (frm, (frm[0] + 0.1, frm[1] - 0.2, frm[2] + 1.0), (0.0, 1.0, 0.0))
    cam = rtc.camera(c.size[0], c.size[1], 1.0, rtc.Matrix.make_view_transform(*view))
    return w, cam, make_projection(rtc, c.kind, c.spec)


# ---- include/rtc.h's arithmetic in Python floats (IEEE f64, one rounding per operation, nothing fused) -----------------
def _transform_point(O, cam, p):
    """Matrix::transform_point (transform.rs:122-128), the oracle's"""
    out = (C.c_double * 3)()
    O.lib().orc_transform_point((C.c_double * 16)(*cam.view_inv), (C.c_double * 3)(*p), out)
    return tuple(out)


def _normalized(d):
    mag = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])   # Vector::normalize vec.rs:65-76: sqrt of the sum, three divisions
    return (d[0] / mag, d[1] / mag, d[2] / mag)


def ortho_terms(hsize, vsize, width, wrong_branch=False):
    """half_w, half_h, pixel. wrong_branch: half_h taken from the OTHER aspect branch (the mistake of the non-vacuity test)."""
    aspect = float(hsize) / float(vsize)
    if aspect >= 1.0:
        half_w = width / 2.0
        half_h = half_w / aspect
        if wrong_branch: half_h = width / 2.0
    else:
        half_w = (width / 2.0) * aspect
        half_h = width / 2.0
        if wrong_branch: half_h = half_w / aspect
    return half_w, half_h, (half_w * 2.0) / float(hsize)


def pano_entry(span, i, n, flip=False):
    a = span * (0.5 - (float(i) + 0.5) / float(n))
    if flip: a = -a
    return (math.sin(a), math.cos(a))


def restated_ray(O, cam, proj, x, y, mistake=None):
    """The ray of pixel (x, y) as include/rtc.h states it; `mistake` names what a wrong kernel would do instead:
    "phi-sign" (longitude mirrored), "row-swapped" (sin and cos of the latitude exchanged), "transposed" (col indexed by y
    and row by x, clamped), "aspect" (orthographic: half_h from the wrong aspect branch)."""
    if proj.kind == ORTHO:
        half_w, half_h, pixel = ortho_terms(cam.hsize, cam.vsize, proj.width, wrong_branch=(mistake == "aspect"))
        world_x = half_w - (float(x) + 0.5) * pixel
        world_y = half_h - (float(y) + 0.5) * pixel
        origin = _transform_point(O, cam, (world_x, world_y, 0.0))
        target = _transform_point(O, cam, (world_x, world_y, -1.0))
    else:
        cx, ry = (min(y, cam.hsize - 1), min(x, cam.vsize - 1)) if mistake == "transposed" else (x, y)
        col = pano_entry(proj.h_span, cx, cam.hsize, flip=(mistake == "phi-sign"))
        row = pano_entry(proj.v_span, ry, cam.vsize)
        if mistake == "row-swapped": row = (row[1], row[0])
        origin = _transform_point(O, cam, (0.0, 0.0, 0.0))
        target = _transform_point(O, cam, (row[1] * col[0], row[0], -(row[1] * col[1])))
    return origin + _normalized(tuple(t - o for t, o in zip(target, origin)))


# ---- reference frames ------------------------------------------------------------------------------------------------
def frame_of_rays(O, w, light, cam, fill_ray, mode=MODE_RENDER_ASYNC, nthreads=8):
    """color_at(ray(x, y), MAX_REFLECTIONS) per pixel; fill_ray(x, y, ray) writes a (c_double * 6). RTC_MODE_RENDER leaves the
    last row and column black (camera.rs:120-121). Rows are shared out over threads (ctypes releases the GIL)."""
    shapes, n, color_at, lightr = w.array(), len(w), O.lib().orc_color_at, C.byref(light)
    out = np.zeros((cam.vsize, cam.hsize, 3), dtype=np.float64)

    def rows(y0, y1):
        ray, rgb = (C.c_double * 6)(), (C.c_double * 3)()
        for y in range(y0, y1):
            for x in range(cam.hsize):
                if mode == MODE_RENDER and (x + 1 >= cam.hsize or y + 1 >= cam.vsize):
                    continue
                fill_ray(x, y, ray)
                color_at(shapes, n, lightr, ray, 5, rgb, None)
                out[y, x] = (rgb[0], rgb[1], rgb[2])

    step = max(1, -(-cam.vsize // (4 * nthreads)))
    with ThreadPoolExecutor(nthreads) as pool:
        for f in [pool.submit(rows, y, min(cam.vsize, y + step)) for y in range(0, cam.vsize, step)]:
            f.result()
    out.setflags(write=False)
    return out


def reference_of(rtc, O, w, light, cam, proj, mode=MODE_RENDER_ASYNC):
    """The reference frame: the oracle's color_at of rtc_projection_ray(x, y)"""
    ray_fn, camr, projr = rtc.lib().rtc_projection_ray, C.byref(cam), C.byref(proj)

    def fill(x, y, ray):
        assert ray_fn(camr, projr, x, y, ray) == 0
    return frame_of_rays(O, w, light, cam, fill, mode)


@functools.lru_cache(maxsize=None)
def reference(rtc, O, name, light_spec=None, mode=MODE_RENDER_ASYNC):
    """... of case `name`; light_spec: (position, intensity) instead of the World's own light. Computed once, shared."""
    w, cam, proj = build(rtc, name)
    light = w.light if light_spec is None else rtc.light(position=light_spec[0], intensity=light_spec[1])
    return reference_of(rtc, O, w, light, cam, proj, mode)


@functools.lru_cache(maxsize=None)
def mistaken(rtc, O, name, mistake):
    """The frame a kernel with `mistake` (restated_ray) would give for case `name`; mistake None: the restatement itself."""
    w, cam, proj = build(rtc, name)

    def fill(x, y, ray):
        ray[:] = restated_ray(O, cam, proj, x, y, mistake)
    return frame_of_rays(O, w, w.light, cam, fill)


# ---- what make_bundle sees of a frame --------------------------------------------------------------------------------
def directions(rtc, cam, proj):
    out = np.empty((cam.vsize, cam.hsize, 3))
    ray, fn, camr, projr = (C.c_double * 6)(), rtc.lib().rtc_projection_ray, C.byref(cam), C.byref(proj)
    for y in range(cam.vsize):
        for x in range(cam.hsize):
            assert fn(camr, projr, x, y, ray) == 0
            out[y, x] = ray[3:6]
    return out


def tile_min_cosines(rtc, cam, proj):
    """Per 8x8 tile the smallest cosine between the tile's axis ray and any ray of the tile. The axis is make_bundle's: lane
    27, pixel (3, 3) of the tile, when that pixel is on the canvas, else the first lane above it that is, else the highest."""
    d = directions(rtc, cam, proj)
    out = []
    for ty in range(0, cam.vsize, 8):
        for tx in range(0, cam.hsize, 8):
            lanes = [l for l in range(64) if tx + (l & 7) < cam.hsize and ty + (l >> 3) < cam.vsize]
            above = [l for l in lanes if l >= 27]
            axis = above[0] if above else lanes[-1]
            a = d[ty + (axis >> 3), tx + (axis & 7)]
            out.append(min(float(np.dot(a, d[ty + (l >> 3), tx + (l & 7)])) for l in lanes))
    return out
