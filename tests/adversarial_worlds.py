"""Hostile worlds for every render flavour (helper module, not collected; used by test_gpu_parity.py, stress_parity.py,
test_gpu_lens.py, test_host_adversarial_worlds.py and test_gpu_adversarial_flavours.py).

Part 1: the seeded generators of the one-light pinhole tests (adversarial_scene) and of the stress campaign (big_world,
far_world, mirror_world, list_family), moved here with their bodies unchanged: a seed builds the same bytes as before
(test_host_adversarial_worlds.py pins the digests).
Part 2: what turns such a world into a hostile case of the multi-light, lens and AOV kernels: material twins, another frame
size, lights and area lights placed where a shadow bundle degenerates, lenses whose sample origins straddle a surface.
Part 3: the oracle's references (summed single-light frames, lens frames, hit records), each computed once and read-only.
Part 4: the case table both test files read.

Everything is derived from the world by the product's host arithmetic (rtc.Matrix, rtc_lens_ray) and the CPU oracle: no GPU."""
from __future__ import annotations

import ctypes as C
import functools
import itertools
import math
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

import candidate_list_cases as K

SPHERE, PLANE, CUBE = 0, 1, 2
MODE_RENDER, MODE_RENDER_ASYNC = 0, 1
NO_CULL = 1
SRC_SMEM, SRC_CULL, SRC_CULL2 = 0, 3, 4
TIGHT_TOL = 1e-12   # per light sample (tests/test_gpu_parity.py, test_gpu_lights.py, test_gpu_area_lights.py)
FRAME = (52, 37)    # partial 8x8 tiles on both edges (the generators' 56x40 / 64x40 / 96x64 frames are whole tiles)
CAP_FRAME = (9, 7)  # the 256-sample lens
PLANES = ("index", "depth", "point", "normal", "flags", "shadow")
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "pixels")


# ====================================================================================== 1. the seeded generators (moved)
def adversarial_scene(rtc, seed):
    """Scenes built to stress the cull's conservativeness: tiny far spheres, huge near ones, thin
    sheared ellipsoids, cubes, objects around and behind the camera and the light, the camera and
    the light inside objects, mirrors and glass (wide secondary bundles)."""
    rng = np.random.default_rng(seed)
    u = lambda a, b: float(rng.uniform(a, b))
    w = rtc.World(rtc.light((u(-6, 6), u(1, 9), u(-9, 2))))
    n = int(rng.integers(3, 40))
    for i in range(n):
        k = int(rng.integers(0, 6))
        if k == 0:   # tiny and far
            t = rtc.Matrix.identity().scaling(*(3 * [u(0.01, 0.05)])).translation(u(-30, 30), u(0, 20), u(10, 90))
        elif k == 1:  # huge, may contain camera or light
            t = rtc.Matrix.identity().scaling(*(3 * [u(5, 30)])).translation(u(-10, 10), u(-10, 10), u(-10, 30))
        elif k == 2:  # thin needle / pancake, rotated
            t = (rtc.Matrix.identity().scaling(u(0.02, 0.1), u(1, 4), u(0.02, 2)).rotation_x(u(0, 3)).rotation_z(u(0, 3))
                 .translation(u(-4, 4), u(0, 4), u(-2, 8)))
        elif k == 3:  # sheared
            t = (rtc.Matrix.identity().shearing(u(-1, 1), u(-1, 1), u(-1, 1), u(-1, 1), u(-1, 1), u(-1, 1)).scaling(u(0.3, 1.5), u(0.3, 1.5), u(0.3, 1.5))
                 .translation(u(-4, 4), u(0, 3), u(-3, 8)))
        elif k == 4:  # behind / beside the camera
            t = rtc.Matrix.identity().scaling(*(3 * [u(0.3, 2)])).translation(u(-6, 6), u(-1, 4), u(-14, -4))
        else:
            t = rtc.Matrix.identity().scaling(*(3 * [u(0.2, 1.2)])).translation(u(-5, 5), u(0, 4), u(-3, 9))
        glass = rng.random() < 0.25
        mat = rtc.material(color=(u(0, 1), u(0, 1), u(0, 1)), ambient=u(0, 0.3), diffuse=u(0.2, 0.9), specular=u(0, 0.9),
                           shininess=u(1, 300), reflective=(u(0.1, 0.9) if rng.random() < 0.4 else 0.0),
                           transparency=(u(0.3, 1.0) if glass else 0.0), refractive_index=(u(1.05, 2.2) if glass else 1.0))
        try:
            w.add_shape((rtc.cube if rng.random() < 0.25 else rtc.sphere)(t, mat))
        except rtc.RtcError:
            pass  # singular by the reference's 1e-8 determinant rule: the reference would panic too
    if rng.random() < 0.7:
        w.add_shape(rtc.plane(rtc.Matrix.identity().rotation_z(u(-0.2, 0.2)).translation(0, u(-1, 0), 0),
                              rtc.material(reflective=u(0, 0.5), specular=0.1, pattern=("checker", (0.3,) * 3, (0.7,) * 3, None))))
    cam = rtc.camera(56, 40, u(0.4, 2.0), rtc.Matrix.make_view_transform((u(-3, 3), u(0.2, 4), u(-9, -3)), (u(-1, 1), u(0, 2), u(0, 4)), (0, 1, 0)))
    return w, cam


def big_world(rtc, seed):
    """Up to ~2000 small objects (forces the two-level cull) with a few big / odd ones mixed in."""
    rng = np.random.default_rng(seed)
    u = lambda a, b: float(rng.uniform(a, b))
    w = rtc.World(rtc.light((u(-8, 8), u(2, 12), u(-10, 0))))
    n = int(rng.integers(257, 2000))
    for i in range(n):
        r = u(0.02, 0.4) if rng.random() < 0.97 else u(1.0, 6.0)
        t = rtc.Matrix.identity().scaling(r, r * u(0.5, 1.5), r).rotation_y(u(0, 3)).translation(u(-12, 12), u(-1, 8), u(-6, 30))
        glass = rng.random() < 0.03
        m = rtc.material(color=(u(0, 1), u(0, 1), u(0, 1)), ambient=u(0, 0.3), diffuse=u(0.3, 0.9), specular=u(0, 0.5), shininess=u(5, 100),
                         reflective=(u(0.1, 0.6) if rng.random() < 0.05 else 0.0), transparency=(u(0.3, 0.9) if glass else 0.0),
                         refractive_index=(u(1.1, 1.9) if glass else 1.0))
        w.add_shape((rtc.cube if rng.random() < 0.1 else rtc.sphere)(t, m))
    if rng.random() < 0.6:
        w.add_shape(rtc.plane(rtc.Matrix.identity(), rtc.material(specular=0.0, pattern=("checker", (0.3,) * 3, (0.7,) * 3, None))))
    cam = rtc.camera(64, 40, u(0.5, 1.4), rtc.Matrix.make_view_transform((u(-3, 3), u(0.5, 5), u(-10, -4)), (u(-1, 1), u(0, 2), u(2, 8)), (0, 1, 0)))
    return w, cam


def far_world(rtc, seed):
    """The f32 wave-level cull's worst cases: the whole scene (objects, camera, light) translated far from the origin
    (centres and apex lose up to 2^-24 of 1e3..1e7 when rounded to f32 — more than many of the radii), the scene scaled
    by 1e-3..1e3, tiny spheres far away, a few hundred objects now and then (two-level walk)."""
    rng = np.random.default_rng(seed)
    u = lambda a, b: float(rng.uniform(a, b))
    off = [0.0, 0.0, 0.0]
    if rng.random() < 0.8:
        mag = 10.0 ** u(2, 7)
        off = [mag * u(-1, 1), mag * u(-1, 1) * 0.3, mag * u(-1, 1)]
    sc = 10.0 ** u(-3, 3) if rng.random() < 0.5 else 1.0
    P = lambda x, y, z: (off[0] + sc * x, off[1] + sc * y, off[2] + sc * z)
    w = rtc.World(rtc.light(P(u(-8, 8), u(2, 12), u(-10, 0))))
    n = int(rng.integers(300, 700)) if rng.random() < 0.25 else int(rng.integers(5, 60))
    for i in range(n):
        r = sc * (u(0.001, 0.02) if rng.random() < 0.3 else u(0.05, 1.5))
        t = rtc.Matrix.identity().scaling(r, r * u(0.3, 1.7), r).rotation_z(u(0, 3)).translation(*P(u(-10, 10), u(-1, 6), u(-6, 40)))
        m = rtc.material(color=(u(0, 1), u(0, 1), u(0, 1)), ambient=u(0, 0.3), diffuse=u(0.3, 0.9), specular=u(0, 0.5), shininess=u(5, 100),
                         reflective=(u(0.1, 0.6) if rng.random() < 0.15 else 0.0))
        try:
            w.add_shape((rtc.cube if rng.random() < 0.15 else rtc.sphere)(t, m))
        except rtc.RtcError:
            pass  # singular by the reference's 1e-8 determinant rule
    if rng.random() < 0.5:
        w.add_shape(rtc.plane(rtc.Matrix.identity().translation(*P(0, u(-1, 0), 0)), rtc.material(specular=0.0, reflective=u(0, 0.4))))
    cam = rtc.camera(56, 40, u(0.4, 1.6), rtc.Matrix.make_view_transform(P(u(-3, 3), u(0.5, 5), u(-10, -4)), P(u(-1, 1), u(0, 2), u(2, 8)), (0, 1, 0)))
    return w, cam


def mirror_world(rtc, seed):
    """One-level worlds (<= 256 objects) of small MIRRORS: reflection rays off a sphere of a few pixels fan out over a
    hemisphere, no cone holds them, and the pass takes the per-lane walk over groups of 8 (walk_per_lane, round 3) with its
    distance limit; now and then glass (refraction rays likewise), cubes, flattened ellipsoids, a mirror floor, far offsets."""
    rng = np.random.default_rng(seed)
    u = lambda a, b: float(rng.uniform(a, b))
    off = [0.0, 0.0, 0.0]
    if rng.random() < 0.2:
        mag = 10.0 ** u(1, 5)
        off = [mag * u(-1, 1), mag * u(-1, 1) * 0.2, mag * u(-1, 1)]
    P = lambda x, y, z: (off[0] + x, off[1] + y, off[2] + z)
    w = rtc.World(rtc.light(P(u(-8, 8), u(3, 12), u(-10, 0))))
    n = int(rng.integers(3, 250))
    for i in range(n):
        r = u(0.03, 0.25) if rng.random() < 0.8 else u(0.4, 2.0)
        flat = u(0.05, 1.0) if rng.random() < 0.2 else 1.0
        t = rtc.Matrix.identity().scaling(r, r * flat, r).rotation_x(u(0, 3)).translation(*P(u(-6, 6), u(0, 4), u(-3, 14)))
        glass = rng.random() < 0.15
        m = rtc.material(color=(u(0, 1), u(0, 1), u(0, 1)), ambient=u(0, 0.3), diffuse=u(0.2, 0.9), specular=u(0, 0.9), shininess=u(5, 300),
                         reflective=(u(0.05, 1.0) if rng.random() < 0.8 else 0.0), transparency=(u(0.2, 1.0) if glass else 0.0),
                         refractive_index=(u(1.0, 2.0) if glass else 1.0))
        try:
            w.add_shape((rtc.cube if rng.random() < 0.15 else rtc.sphere)(t, m))
        except rtc.RtcError:
            pass
    if rng.random() < 0.7:
        w.add_shape(rtc.plane(rtc.Matrix.identity().translation(*P(0, u(-0.5, 0), 0)),
                              rtc.material(specular=0.0, reflective=u(0, 0.6), pattern=("checker", (0.3,) * 3, (0.7,) * 3, None))))
    cam = rtc.camera(64, 40, u(0.5, 1.4), rtc.Matrix.make_view_transform(P(u(-3, 3), u(0.5, 5), u(-10, -4)), P(u(-1, 1), u(0, 2), u(2, 8)), (0, 1, 0)))
    return w, cam


def list_family(rtc, seed):
    """candidate_list_cases.list_world: 32..1500 objects, planes in arbitrary poses, the light and the camera in odd places."""
    shapes, lgt, cam = K.list_world(seed, "small" if seed % 2 else "large")
    return K.as_world(rtc, shapes, lgt), cam


FAMILIES = {"adversarial_scene": adversarial_scene, "big_world": big_world, "far_world": far_world, "mirror_world": mirror_world,
            "list_family": list_family}


def world_digest(w, cam):
    """SHA-256 of the bytes a seed stands for: the shape records, the first light and the camera."""
    import hashlib
    h = hashlib.sha256()
    h.update(bytes(w.array()))
    h.update(bytes(w.light))
    h.update(bytes(cam))
    return h.hexdigest()


# ====================================================================================== 2. hostile twins, lights and lenses
def _copy(obj):
    out = type(obj)()
    C.memmove(C.byref(out), C.byref(obj), C.sizeof(obj))
    return out


def with_lights(rtc, w, lights):
    """The same shapes under other lights."""
    m = rtc.World(list(lights))
    m.shapes = list(w.shapes)
    return m


def with_materials(rtc, w, refl, refr):
    """A copy of `w` with every transparency 0 unless `refr` and every reflective 0 unless `refl`: (False, False) is the
    flat twin of a geometry, (True, False) its reflection-only twin, (True, True) the world as it is."""
    m = rtc.World([_copy(l) for l in w.lights])
    for s in w.shapes:
        c = _copy(s)
        if not refr:
            c.material.transparency = 0.0
        if not refl:
            c.material.reflective = 0.0
        m.shapes.append(c)
    return m


def recamera(rtc, cam, W, H):
    """The same view (view_inv bit for bit) and field of view at another frame size."""
    out = rtc.camera(W, H, cam.fov, None, samples=cam.samples)
    C.memmove(out.view_inv, cam.view_inv, C.sizeof(cam.view_inv))
    return out


def _np(v):
    return np.array(list(v), dtype=np.float64)


def cam_frame(cam):
    """(origin, right, up, forward) of a camera in world space, read off view_inv (row-major, translation in column 3)."""
    m = _np(cam.view_inv).reshape(4, 4)
    return m[:3, 3].copy(), m[:3, 0].copy(), m[:3, 1].copy(), -m[:3, 2]


def moved_camera(cam, origin):
    """`cam` with its origin at `origin`, same orientation."""
    out = _copy(cam)
    for r in range(3):
        out.view_inv[4 * r + 3] = float(origin[r])
    return out


def shape_frame(rtc, s):
    """(transform as a 4x4 array, centre, semi-axis lengths) of a shape: the inverse of its stored inverse (numpy's: the
    inverse of a large shape fails the reference's determinant rule, which is a rule for transforms)."""
    t = np.linalg.inv(_np(s.inv).reshape(4, 4))
    return t, t[:3, 3].copy(), np.sqrt((t[:3, :3] ** 2).sum(axis=0))


def bounded(w):
    return [i for i, s in enumerate(w.shapes) if s.kind != PLANE]


def largest_bounded(rtc, w):
    """Index of the bounded shape with the longest semi-axis (the first of equals); None in a world without one."""
    best, size = None, -1.0
    for i in bounded(w):
        a = float(shape_frame(rtc, w.shapes[i])[2].max())
        if a > size:
            best, size = i, a
    return best


def big_frame(rtc, w):
    """shape_frame of the largest bounded shape; the unit sphere at the scene's centre where the world has none."""
    i = largest_bounded(rtc, w)
    if i is None:
        t = np.eye(4)
        t[:3, 3] = scene_centre(rtc, w)
        return t, t[:3, 3].copy(), np.ones(3)
    return shape_frame(rtc, w.shapes[i])


def first_plane(rtc, w):
    """(point on the plane under the scene's centre, unit normal, a unit tangent) of the first plane; without a plane, the
    horizontal plane through the lowest bounded shape's centre (through the scene's centre in a world without shapes)."""
    c = scene_centre(rtc, w)
    for s in w.shapes:
        if s.kind == PLANE:
            t = shape_frame(rtc, s)[0]
            n = t[:3, 1] / np.linalg.norm(t[:3, 1])
            tan = t[:3, 0] / np.linalg.norm(t[:3, 0])
            p0 = t[:3, 3]
            return c - n * float(np.dot(c - p0, n)), n, tan
    low = min((shape_frame(rtc, w.shapes[i])[1] for i in bounded(w)), key=lambda p: p[1], default=c)
    return np.array([c[0], low[1], c[2]]), np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])


def scene_centre(rtc, w):
    """Centroid of the bounded shapes' centres; of a world without one, a point 5 below its light."""
    pts = [shape_frame(rtc, w.shapes[i])[1] for i in bounded(w)]
    return np.mean(pts, axis=0) if pts else _np(w.light.position) - np.array([0.0, 5.0, 0.0])


def centre_hit(rtc, O, w, cam, seed=0):
    """The oracle's hit record of the centre pixel's ray; where that ray misses, of the first pixel that hits in raster
    order from a start the seed picks. -> (x, y, RtcHit)"""
    W, H = cam.hsize, cam.vsize
    order = [(W // 2, H // 2)] + [((k + 7919 * seed) % (W * H) % W, (k + 7919 * seed) % (W * H) // W) for k in range(W * H)]
    arr, n = w.array(), len(w)
    for x, y in order:
        _, h = O.color_at(arr, n, w.light, tuple(rtc.ray_for_pixel(cam, x, y)), 5, want_hit=True)
        if h.hit_index >= 0:
            return x, y, h
    raise ValueError("no pixel of this frame hits anything")


HOSTILE_LIGHTS = ("in_big", "low", "at_eye", "behind", "near_surface", "far", "twice")
SECOND_INTENSITY = (0.6, 0.5, 0.4)


def hostile_lights(rtc, O, w, cam, seed=0):
    """{name: RtcLight}: positions derived from the world at which a shadow bundle degenerates."""
    origin, right, up, fwd = cam_frame(cam)
    centre = scene_centre(rtc, w)
    own = _np(w.light.position)
    p0, n, _ = first_plane(rtc, w)
    try:
        _, _, h = centre_hit(rtc, O, w, cam, seed)
        near = _np(h.over_point) + 0.01 * _np(h.normal)
    except ValueError:   # a frame that sees nothing (the stress campaign meets such worlds): the scene's centre instead
        near = centre
    d = own - centre
    pos = {
        "in_big": big_frame(rtc, w)[1],                                     # inside an object
        "low": p0 + 0.05 * n,                                               # grazing the floor
        "at_eye": origin,                                                   # shadow segments along the primary rays
        "behind": origin - 3.0 * fwd,
        "near_surface": near,                                               # the tile's hit points surround it: > a hemisphere
        "far": centre + 1e6 * (d / np.linalg.norm(d)),                      # the quadratic cancels
    }
    out = {k: rtc.light(position=tuple(float(c) for c in v), intensity=SECOND_INTENSITY) for k, v in pos.items()}
    out["twice"] = _copy(w.light)
    assert tuple(out) == HOSTILE_LIGHTS
    return out


HOSTILE_AREA_LIGHTS = ("cross_floor", "through_big", "coincident")


def hostile_area_light(rtc, w):
    """{name: RtcAreaLight}, each a 3x3 grid (9 samples: the smallest device table):
    cross_floor — u runs along the first plane's normal from 2 above it to 1 below: samples at +1.5, +0.5 and -0.5;
    through_big — u runs through the largest bounded shape's centre towards the world's own light, 4 semi-axes long:
                  samples outside, inside (the centre) and outside;
    coincident — uvec = vvec = 0 at the world's own light: nine coincident samples."""
    p0, n, tan = first_plane(rtc, w)
    own = _np(w.light.position)
    q = p0 + tan * float(np.dot(own - p0, tan)) * 0.25
    t, c, axes = big_frame(rtc, w)
    a = float(axes.max())
    ex = (own - c) / np.linalg.norm(own - c)
    ey = np.cross(ex, np.eye(3)[int(np.argmin(np.abs(ex)))])   # (the coordinate axis least along ex: never parallel)
    ey = ey / np.linalg.norm(ey)
    f = lambda v: tuple(float(x) for x in v)
    inten = tuple(w.light.intensity)
    return {
        "cross_floor": rtc.area_light(f(q + 2.0 * n - 1.0 * tan), f(-3.0 * n), f(2.0 * tan), 3, 3, inten),
        "through_big": rtc.area_light(f(c - 2.0 * a * ex - 0.15 * a * ey), f(4.0 * a * ex), f(0.3 * a * ey), 3, 3, inten),
        "coincident": rtc.area_light(f(own), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 3, 3, inten),
    }


HOSTILE_LENSES = ("straddle_shape", "straddle_plane", "short_focus", "long_focus", "in_cloud", "row", "column", "cap")


def straddled_sphere(rtc, w, cam):
    """Index of the sphere straddle_shape sits on: in front of the camera, shortest semi-axis 0.2 .. 3, the largest such."""
    origin, _, _, fwd = cam_frame(cam)
    best, size = None, -1.0
    for i, s in enumerate(w.shapes):
        if s.kind != SPHERE:
            continue
        _, c, axes = shape_frame(rtc, s)
        a = float(axes.min())
        if 0.2 <= a <= 3.0 and float(np.dot(c - origin, fwd)) > 0.0 and a > size:
            best, size = i, a
    return best


def small_centroid(rtc, w):
    """Centroid of the small shapes (longest semi-axis below 0.5): the middle of the cloud."""
    pts = [c for _, c, axes in (shape_frame(rtc, w.shapes[i]) for i in bounded(w)) if float(axes.max()) < 0.5]
    return np.mean(pts, axis=0) if pts else scene_centre(rtc, w)


def hostile_lenses(rtc, w, cam):
    """{name: ((aperture, focal_distance, usteps, vsteps), camera)}; a lens that needs what the world lacks (a plane, a
    sphere of moderate size, more than 256 objects) is left out."""
    origin, right, up, fwd = cam_frame(cam)
    out = {}
    i = straddled_sphere(rtc, w, cam)
    if i is not None:
        # the eye on the sphere's surface, on the side of the camera's own x axis: the lens plane holds the surface normal,
        # so the columns of the grid step through the surface
        s = w.shapes[i]
        t, c, axes = shape_frame(rtc, s)
        inv = _np(s.inv).reshape(4, 4)
        local = inv[:3, :3] @ right
        local /= np.linalg.norm(local)
        eye = t[:3, :3] @ local + c
        out["straddle_shape"] = ((0.5 * float(axes.min()), 4.0, 3, 2), moved_camera(cam, eye))
    if any(s.kind == PLANE for s in w.shapes):
        p0, n, _ = first_plane(rtc, w)
        a = 0.4
        eye = origin - n * float(np.dot(origin - p0, n)) + 0.25 * a * n   # a quarter of the aperture above the floor
        out["straddle_plane"] = ((a, 4.0, 2, 3), moved_camera(cam, eye))
    out["short_focus"] = ((2e-3, 1e-3, 2, 2), _copy(cam))
    out["long_focus"] = ((0.5, 1e6, 2, 2), _copy(cam))
    if len(w) > 256:
        out["in_cloud"] = ((0.3, 3.0, 2, 2), moved_camera(cam, small_centroid(rtc, w)))
    out["row"] = ((0.6, 6.0, 5, 1), _copy(cam))
    out["column"] = ((0.6, 6.0, 1, 5), _copy(cam))
    out["cap"] = ((0.4, 6.0, 16, 16), recamera(rtc, cam, *CAP_FRAME))
    return out


def lens_origins(rtc, cam, lens_spec):
    """The sample origins of a lens (rtc_lens_ray of pixel (0, 0): the origin does not depend on the pixel)."""
    lens = rtc.lens(*lens_spec)
    return np.array([rtc.lens_ray(cam, lens, 0, 0, k)[:3] for k in range(lens.usteps * lens.vsteps)])


def all_finite(w, cam, lights=()):
    vals = [np.frombuffer(bytes(w.array()), dtype=np.uint8)]   # (placeholder so that an empty world is handled)
    ok = True
    for s in w.shapes:
        m = s.material
        ok &= bool(np.isfinite(_np(s.inv)).all() and np.isfinite(_np(s.inv_t)).all() and np.isfinite(_np(m.color)).all())
        ok &= all(math.isfinite(v) for v in (m.ambient, m.diffuse, m.specular, m.shininess, m.reflective, m.transparency, m.refractive_index))
    ok &= bool(np.isfinite(_np(cam.view_inv)).all()) and all(math.isfinite(v) for v in (cam.fov, cam.half_width, cam.half_height, cam.pixel_size))
    for l in list(w.lights) + list(lights):
        for f in ("position", "corner", "uvec", "vvec", "intensity"):
            if hasattr(l, f):
                ok &= bool(np.isfinite(_np(getattr(l, f))).all())
    del vals
    return ok


def passes_determinant_rule(rtc, O, w):
    """Every shape's transform is invertible by the oracle's determinant rule (transform.rs:177): O.inverse raises otherwise."""
    for s in w.shapes:
        O.inverse(O.mat(shape_frame(rtc, s)[0]))
    return True


# ====================================================================================== 3. the oracle's references
def sample_key(l):
    return (tuple(l.position), tuple(l.intensity))


def oracle_lens_frame(rtc, O, shapes, n, light, cam, lens_spec, u_outer=False, mode=MODE_RENDER_ASYNC, nthreads=8):
    """Color::average_over of the oracle's color_at(rtc_lens_ray(x, y, k)), k in sample order (u_outer: in the WRONG,
    u-outer order): sums from 0.0 in sample order, one division by n. Rows are shared out over threads (ctypes releases the
    GIL); each pixel is computed by one thread in the stated order."""
    lens = rtc.lens(*lens_spec)
    lens_ray, color_at = rtc.lib().rtc_lens_ray, O.lib().orc_color_at
    camr, lensr, lightr = C.byref(cam), C.byref(lens), C.byref(light)
    us, vs = lens.usteps, lens.vsteps
    ns = us * vs
    order = [v * us + u for u in range(us) for v in range(vs)] if u_outer else list(range(ns))
    out = np.zeros((cam.vsize, cam.hsize, 3), dtype=np.float64)

    def rows(y0, y1):
        ray, rgb = (C.c_double * 6)(), (C.c_double * 3)()
        for y in range(y0, y1):
            for x in range(cam.hsize):
                if mode == MODE_RENDER and (x + 1 >= cam.hsize or y + 1 >= cam.vsize):
                    continue   # Camera::render leaves the last row and column black (camera.rs:120-121)
                r = g = b = 0.0
                for k in order:
                    assert lens_ray(camr, lensr, x, y, k, ray) == 0
                    color_at(shapes, n, lightr, ray, 5, rgb, None)
                    r += rgb[0]; g += rgb[1]; b += rgb[2]
                out[y, x] = (r / float(ns), g / float(ns), b / float(ns))

    if nthreads <= 1 or cam.vsize < 2:
        rows(0, cam.vsize)
    else:
        step = max(1, -(-cam.vsize // (4 * nthreads)))
        with ThreadPoolExecutor(nthreads) as pool:
            for f in [pool.submit(rows, y, min(cam.vsize, y + step)) for y in range(0, cam.vsize, step)]:
                f.result()
    out.setflags(write=False)
    return out


_frames: dict = {}
_hits: dict = {}


def oracle_frame(rtc, O, key, w, cam, sample, lens_spec=None, mode=MODE_RENDER_ASYNC):
    """The oracle's single-light frame of (world `key`, light sample, lens): computed once, shared, never written to."""
    k = (key, sample, lens_spec, cam.hsize, cam.vsize, bytes(cam.view_inv), mode)
    if k not in _frames:
        lgt = rtc.light(position=sample[0], intensity=sample[1])
        if lens_spec is None:
            out = O.render(w.array(), len(w), lgt, cam, mode=mode, nthreads=8)
            out.setflags(write=False)
        else:
            out = oracle_lens_frame(rtc, O, w.array(), len(w), lgt, cam, lens_spec, mode=mode)
        _frames[k] = out
    return _frames[k]


def oracle_sum(rtc, O, key, w, cam, samples, lens_spec=None, mode=MODE_RENDER_ASYNC):
    """The sum of the single-light frames in sample order: the reference of an n-sample world, bound n x TIGHT_TOL."""
    ref = oracle_frame(rtc, O, key, w, cam, samples[0], lens_spec, mode)
    for s in samples[1:]:
        ref = ref + oracle_frame(rtc, O, key, w, cam, s, lens_spec, mode)
    return ref


def oracle_stats(rtc, O, key, w, cam, sample):
    k = (key, sample, cam.hsize, cam.vsize, bytes(cam.view_inv), "stats")
    if k not in _frames:
        _frames[k] = O.render(w.array(), len(w), rtc.light(position=sample[0], intensity=sample[1]), cam, mode=1, nthreads=8, want_stats=True)[1]
    return _frames[k]


def oracle_hits(rtc, O, key, w, cam, samples):
    """(RtcHit array of the centre rays under the first sample, uint16 count of the samples that hide each hit point), as
    aov_cases.oracle_hits builds them: color_at(..., want_hit=True) per pixel and sample."""
    k = (key, tuple(samples), cam.hsize, cam.vsize, bytes(cam.view_inv))
    if k not in _hits:
        arr, n = w.array(), len(w)
        lights = [rtc.light(position=s[0], intensity=s[1]) for s in samples]
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
        _hits[k] = (hits, counts)
    return _hits[k]


def expected_planes(rtc, O, key, w, cam, samples, mode):
    """rtc_aov_from_hits of the oracle's records (read-only arrays), as aov_cases.expected."""
    k = (key, tuple(samples), cam.hsize, cam.vsize, bytes(cam.view_inv), mode, "planes")
    if k not in _hits:
        hits, counts = oracle_hits(rtc, O, key, w, cam, samples)
        planes = rtc.aov_from_hits(hits, cam.hsize, cam.vsize, mode, shadow_counts=counts)
        for a in planes.values():
            a.setflags(write=False)
        _hits[k] = planes
    return _hits[k]


def classes(rtc, O, key, w, cam, samples):
    """What the oracle's centre rays saw: counts of pixels some sample lights / some sample leaves in shadow / that miss /
    that are seen from inside, and the set of shadow counts over the samples."""
    p = expected_planes(rtc, O, key, w, cam, samples, MODE_RENDER_ASYNC)
    hit = p["index"] >= 0
    return {"lit": int((hit & (p["shadow"] < len(samples))).sum()), "shadowed": int((hit & (p["shadow"] > 0)).sum()), "miss": int((~hit).sum()),
            "inside": int(((p["flags"] & 2) != 0).sum()), "counts": sorted(set(p["shadow"][hit].tolist()))}


def lens_classes(rtc, O, key, w, cam, sample, lens_spec):
    """classes() for the rays of a lens: what the oracle's color_at saw along every rtc_lens_ray of the frame."""
    k = (key, sample, lens_spec, cam.hsize, cam.vsize, bytes(cam.view_inv), "lens classes")
    if k not in _hits:
        arr, n = w.array(), len(w)
        lgt = rtc.light(position=sample[0], intensity=sample[1])
        lens = rtc.lens(*lens_spec)
        c = {"lit": 0, "shadowed": 0, "miss": 0, "inside": 0}
        for y in range(cam.vsize):
            for x in range(cam.hsize):
                for j in range(lens.usteps * lens.vsteps):
                    _, h = O.color_at(arr, n, lgt, tuple(rtc.lens_ray(cam, lens, x, y, j)), 5, want_hit=True)
                    if h.hit_index < 0:
                        c["miss"] += 1
                    else:
                        c["shadowed" if h.shadowed else "lit"] += 1
                        c["inside"] += int(h.inside)
        _hits[k] = c
    return _hits[k]


def widest_angle_from(light_pos, points):
    """The largest angle (degrees) between two of the directions from `light_pos` to `points`."""
    d = np.asarray(points) - np.asarray(light_pos)
    d = d / np.linalg.norm(d, axis=1)[:, None]
    return float(np.degrees(np.arccos(np.clip((d @ d.T).min(), -1.0, 1.0))))


def tile_hit_points(rtc, O, key, w, cam, samples, x, y):
    """The oracle's over_points of the hits of the 8x8 tile that holds pixel (x, y)."""
    hits, _ = oracle_hits(rtc, O, key, w, cam, samples)
    tx, ty = x // 8 * 8, y // 8 * 8
    pts = []
    for py in range(ty, min(ty + 8, cam.vsize)):
        for px in range(tx, min(tx + 8, cam.hsize)):
            h = hits[py * cam.hsize + px]
            if h.hit_index >= 0:
                pts.append(list(h.over_point))
    return np.array(pts)


# ====================================================================================== 4. the case table
# The two geometries of the matrix and the two further ones of the AOV cases: (family, seed). Chosen so that the oracle's
# 52x37 frame under the world's own light shows lit, shadowed and missing pixels, the world has reflective and transparent
# shapes, a plane, and a sphere for straddle_shape to sit on (test_host_adversarial_worlds.py asserts all of it).
GEOMETRIES = {
    "one": ("adversarial_scene", 1012),
    "two": ("big_world", 5040),
    "inside": ("adversarial_scene", 1024),
    "far": ("far_world", 5013),
}
SHADINGS = {"flat": (False, False), "refl": (True, False), "refr": (True, True)}
SOURCES = {"cull": ("one", SRC_CULL), "cull2": ("two", SRC_CULL2)}
LIGHT_FORMS = ("one", "args", "table")
CAMERAS = ("pinhole", "lens")
AOV_SOURCES = ("smem", "cull", "cull2")


@functools.lru_cache(maxsize=None)
def geometry(rtc, name):
    """(World as generated, its camera at 52x37)"""
    fam, seed = GEOMETRIES[name]
    w, cam = FAMILIES[fam](rtc, seed)
    return w, recamera(rtc, cam, *FRAME)


@functools.lru_cache(maxsize=None)
def shaded(rtc, name, shading):
    """(one-light World of geometry `name` in its flat / refl / refr form, camera)"""
    w, cam = geometry(rtc, name)
    return with_materials(rtc, w, *SHADINGS[shading]), cam


@dataclass(frozen=True)
class Case:
    name: str
    part: str           # "matrix" | "aov_matrix" | "lights" | "lens" | "aov" | "update"
    geometry: str       # key of GEOMETRIES
    shading: str        # key of SHADINGS
    lights: tuple       # ("own",) | ("own", <hostile light>) | ("own", *HOSTILE_LIGHTS) | ("area", <hostile rectangle>)
    lens: str = ""      # "" = pinhole, else a name of HOSTILE_LENSES
    source: int = SRC_CULL
    mode: int = MODE_RENDER_ASYNC
    cell: tuple = ()    # matrix cells: (source, shading, light form, camera) / ("aov", source, light form)

    @property
    def light_form(self):
        n = self.n_samples
        return "one" if n == 1 else ("args" if n <= 8 else "table")

    @property
    def n_samples(self):
        return 9 if self.lights[0] == "area" else len(self.lights)


def _light_set(form):
    return {"one": ("own",), "args": ("own", "near_surface"), "table": ("area", "cross_floor")}[form]


def matrix_cells():
    """The full product of 2a, computed from the axes: every (source, shading, lights, camera) but one-light pinhole, and
    the nine k_aov shadow instantiations."""
    cells = [(s, sh, lf, c) for s, sh, lf, c in itertools.product(SOURCES, SHADINGS, LIGHT_FORMS, CAMERAS) if not (lf == "one" and c == "pinhole")]
    return cells + [("aov", s, lf) for s, lf in itertools.product(AOV_SOURCES, LIGHT_FORMS)]


def build_cases():
    cs = []
    # a. the instantiation matrix
    for src, (geo, src_id) in SOURCES.items():
        for sh in SHADINGS:
            for lf in LIGHT_FORMS:
                for c in CAMERAS:
                    if lf == "one" and c == "pinhole":
                        continue
                    cs.append(Case(f"matrix[{src}-{sh}-{lf}-{c}]", "matrix", geo, sh, _light_set(lf), "straddle_shape" if c == "lens" else "",
                                   src_id, cell=(src, sh, lf, c)))
    for src in AOV_SOURCES:   # smem: the NO_CULL launch (of the one-level geometry) is the cell; the others: the culled launch
        geo, src_id = {"smem": ("one", SRC_SMEM), "cull": ("one", SRC_CULL), "cull2": ("two", SRC_CULL2)}[src]
        for lf in LIGHT_FORMS:
            cs.append(Case(f"matrix[aov-{src}-{lf}]", "aov_matrix", geo, "refr", _light_set(lf), "", src_id, cell=("aov", src, lf)))
    # b. hostile lights, pinhole, REFR
    for src, (geo, src_id) in SOURCES.items():
        for l in HOSTILE_LIGHTS:
            cs.append(Case(f"lights[{src}-second:{l}]", "lights", geo, "refr", ("own", l), "", src_id))
        cs.append(Case(f"lights[{src}-all8]", "lights", geo, "refr", ("own",) + HOSTILE_LIGHTS, "", src_id))
        for a in HOSTILE_AREA_LIGHTS:
            cs.append(Case(f"lights[{src}-area:{a}]", "lights", geo, "refr", ("area", a), "", src_id))
    # c. hostile lenses
    for l in HOSTILE_LENSES:
        if l != "in_cloud":
            cs.append(Case(f"lens[cull-refr-{l}]", "lens", "one", "refr", ("own",), l, SRC_CULL))
    for sh in ("flat", "refl"):
        for l in ("in_cloud", "straddle_shape", "short_focus"):
            cs.append(Case(f"lens[cull2-{sh}-{l}]", "lens", "two", sh, ("own",), l, SRC_CULL2))
    # d. AOV planes on hostile worlds
    for geo, src_id in (("one", SRC_CULL), ("two", SRC_CULL2), ("inside", SRC_CULL), ("far", SRC_CULL2)):
        for lf in LIGHT_FORMS:
            cs.append(Case(f"aov[{geo}-{lf}]", "aov", geo, "refl" if geo == "far" else "refr", _light_set(lf), "", src_id))   # (far worlds have no glass)
    cs.append(Case("aov[two-args-serial]", "aov", "two", "refr", _light_set("args"), "", SRC_CULL2, MODE_RENDER))
    # e. the cell's world reached by DeviceWorld.update from a different world
    for src in SOURCES:
        geo, src_id = SOURCES[src]
        cs.append(Case(f"update[{src}-refr-table-lens]", "update", geo, "refr", _light_set("table"), "straddle_shape", src_id,
                       cell=(src, "refr", "table", "lens")))
    assert len({c.name for c in cs}) == len(cs)
    return cs


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}


def names(part):
    return [c.name for c in CASES if c.part == part]


_built: dict = {}


def build(rtc, O, case):
    """(World with the case's lights, camera, lens spec or None, light samples as (position, intensity) pairs, key of the
    shaded geometry for the reference caches). Built once per case."""
    if case.name not in _built:
        base, cam = shaded(rtc, case.geometry, case.shading)
        lens_spec = None
        if case.lens:
            lens_spec, cam = hostile_lenses(rtc, base, cam)[case.lens]
        # the hostile lights are derived from the geometry as generated and its own camera, whatever the case's lens
        g, gcam = geometry(rtc, case.geometry)
        if case.lights[0] == "area":
            lights = [hostile_area_light(rtc, g)[case.lights[1]]]
        else:
            hl = hostile_lights(rtc, O, g, gcam) if len(case.lights) > 1 else {}
            lights = [_copy(base.light) if l == "own" else hl[l] for l in case.lights]
        w = with_lights(rtc, base, lights)
        samples = tuple(sample_key(s) for s in w.samples())
        _built[case.name] = (w, cam, lens_spec, samples, (case.geometry, case.shading))
    return _built[case.name]


def reference(rtc, O, case):
    """The oracle reference of a colour case: the sum of its single-light (lens) frames in sample order."""
    w, cam, lens_spec, samples, key = build(rtc, O, case)
    return oracle_sum(rtc, O, key, w, cam, samples, lens_spec, case.mode)


def check_class(rtc, O, case):
    """Assert, from host data and the oracle alone, that `case` is what its name says and that its reference can tell a
    wrong kernel from a right one; -> the facts found (printed by the tests). Both test files call this, so a GPU case
    cannot pass vacuously and that is checked without a GPU."""
    w, cam, lens_spec, samples, key = build(rtc, O, case)
    facts = {"objects": len(w), "samples": len(samples)}
    # materials, object count, lights, frame
    any_refl = any(s.material.reflective > 0.0 for s in w.shapes)
    any_refr = any(s.material.transparency > 0.0 for s in w.shapes)
    assert (any_refl, any_refr) == {"flat": (False, False), "refl": (True, False), "refr": (True, True)}[case.shading], case.name
    if case.source == SRC_CULL:
        assert 0 < len(w) <= 256, case.name
    elif case.source == SRC_CULL2:
        assert len(w) > 256, case.name
    assert len(samples) == case.n_samples and (len(samples) > 8) == (case.light_form == "table"), case.name
    assert (cam.hsize, cam.vsize) == (CAP_FRAME if case.lens == "cap" else FRAME), case.name
    assert all_finite(w, cam) and all(np.isfinite(s[0]).all() and np.isfinite(s[1]).all() for s in samples), case.name
    if lens_spec is not None:
        assert lens_spec[2] * lens_spec[3] <= 6 or case.lens == "cap", case.name
        origins = lens_origins(rtc, cam, lens_spec)
        assert np.isfinite(origins).all()
        g, gcam = shaded(rtc, case.geometry, case.shading)
        if case.lens == "straddle_shape":   # |inv . origin| against 1 for the sphere
            s = w.shapes[straddled_sphere(rtc, g, gcam)]
            inv = _np(s.inv).reshape(4, 4)
            r = np.array([np.linalg.norm((inv @ np.append(o, 1.0))[:3]) for o in origins])
            facts["origins_inside"], facts["origins_outside"] = int((r < 1.0).sum()), int((r > 1.0).sum())
            assert facts["origins_inside"] > 0 and facts["origins_outside"] > 0, (case.name, r)
        if case.lens == "straddle_plane":
            p0, n, _ = first_plane(rtc, g)
            side = (origins - p0) @ n
            facts["origins_above"], facts["origins_below"] = int((side > 0).sum()), int((side < 0).sum())
            assert facts["origins_above"] > 0 and facts["origins_below"] > 0, (case.name, side)
        if case.lens == "in_cloud":   # the apex inside at least one shape's bounding sphere
            apex = cam_frame(cam)[0]
            holds = sum(1 for i in bounded(w) for _, c, axes in [shape_frame(rtc, w.shapes[i])] if np.linalg.norm(apex - c) < np.linalg.norm(axes))
            facts["bounding_spheres_around_apex"] = holds
            assert holds > 0, case.name
        if case.part != "aov":   # the lens is no no-op
            d = float(np.max(np.abs(oracle_frame(rtc, O, key, w, cam, samples[0], lens_spec) - oracle_frame(rtc, O, key, w, cam, samples[0]))))
            facts["lens_vs_pinhole"] = d
            assert d > TIGHT_TOL, (case.name, d)
    if lens_spec is not None:
        c = lens_classes(rtc, O, key, w, cam, samples[0], lens_spec)
    else:
        c = classes(rtc, O, key, w, cam, samples)
    facts.update(lit=c["lit"], shadowed=c["shadowed"], miss=c["miss"], inside=c["inside"])
    if case.part in ("aov", "aov_matrix"):
        counts = classes(rtc, O, key, w, cam, samples)["counts"]
        facts["shadow_counts"] = counts
        assert c["lit"] + c["shadowed"] > 0 and max(counts) > 0, (case.name, c)
        if len(samples) > 1:   # a penumbra: some samples hidden, not all
            assert any(0 < v < len(samples) for v in counts), (case.name, counts)
        if case.geometry == "inside":
            assert c["inside"] > 0, case.name
        if case.geometry == "far":
            facts["offset"] = float(np.abs(_np(geometry(rtc, "far")[0].light.position)).max())
            assert facts["offset"] > 1e5, case.name
    elif lens_spec is not None:   # a lens frame: lit, shadowed and black (missing) RAYS; a pixel is their mean
        facts["black"] = c["miss"]
        assert c["lit"] > 0 and c["shadowed"] > 0 and facts["black"] > 0, (case.name, facts)
    else:   # a colour frame: lit, shadowed and black pixels
        first = oracle_frame(rtc, O, key, w, cam, samples[0], lens_spec, case.mode)
        facts["black"] = int((first == 0).all(axis=2).sum())
        assert c["lit"] > 0 and c["shadowed"] > 0 and facts["black"] > 0, (case.name, facts)
    if "near_surface" in case.lights:   # the tile's hit points surround the light: wider than any cone
        g, gcam = geometry(rtc, case.geometry)
        x, y, _ = centre_hit(rtc, O, g, gcam)
        lp = samples[case.lights.index("near_surface")][0]
        own = (sample_key(g.light),)
        facts["near_surface_span_deg"] = widest_angle_from(lp, tile_hit_points(rtc, O, (case.geometry, "refr"), g, gcam, own, x, y))
        assert facts["near_surface_span_deg"] > 90.0, (case.name, facts)
    return facts
