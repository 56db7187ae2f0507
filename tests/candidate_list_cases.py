"""Worlds aimed at the candidate lists that are built ahead of the render: k_bin_tiles' per-tile lists and plane proof,
and the light-space direction-cell lists of rtc_world_create (helper module, not collected; used by
test_host_candidate_lists.py and test_gpu_candidate_lists.py). Built on the CPU oracle's bindings only.

Each case is a named world, light and camera with the decision it targets; `want` holds what the GPU read-backs must
show for the case to have reached its branch, `expect` a CPU-side check on the oracle's canvas / hit records. Everything is
finite and every transform passes the reference's |det| > 1e-8 rule (O.shape raises otherwise)."""
from __future__ import annotations

import importlib.util
import math
import sys
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

import oracle as O


def sibling(name):
    """A module of this directory (which is no package), executed once per process whoever asks for it."""
    key = "_clc_" + name
    if key in sys.modules:
        return sys.modules[key]
    spec = importlib.util.spec_from_file_location(key, Path(__file__).with_name(name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[key] = m          # (dataclasses look their module up)
    spec.loader.exec_module(m)
    return m


B = sibling("boundary_cases")
shp, mat, number, pixel_ray = B.shp, B.mat, B.number, B.pixel_ray
SPHERE, PLANE, CUBE = 0, 1, 2
LIGHT_R = 128                     # RTC_LIGHT_R
TILE_CAP = 64                     # RTC_TILE_LIST_CAP
CAP_SMALL, CAP_LARGE = 16, 128    # RTC_LIGHT_LIST_CAP_SMALL, RTC_LIGHT_LIST_CAP


@dataclass
class ListCase:
    name: str
    decision: str
    shapes: list
    light: object
    cam: object
    want: dict = field(default_factory=dict)   # read-backs (GPU): tile=(tx, ty, k), rows=(min, max), n_unb, cell=(index, k), ...
    expect: object = None                      # callable(case, canvas_by_mode) on the oracle's output (CPU)
    modes: tuple = (1,)                        # RTC_MODE_RENDER_ASYNC; (0, 1) where Camera::render's untraced edge matters

    def arr(self):
        a = (O.RtcShape * max(1, len(self.shapes)))()
        for i, s in enumerate(self.shapes):
            a[i] = s
        return a

    @property
    def n(self):
        return len(self.shapes)

    @property
    def lists(self):          # rtc_world_create builds light lists from 32 objects
        return self.n >= 32

    @property
    def cap(self):
        return 0 if not self.lists else (CAP_LARGE if self.n > 256 else CAP_SMALL)


# ------------------------------------------------------------------ helpers
def cam_of(W, H, fov, frm, to, up=(0., 1., 0.), pre=None):
    """Camera with view_transform(frm, to, up); `pre` = an op ("scaling", x, y, z) multiplied onto the view matrix."""
    v = O.view_transform(frm, to, up)
    if pre is not None:
        out = O.Mat16()
        getattr(O.lib(), "orc_matrix_" + pre[0])(v, *[O.C.c_double(x) for x in pre[1:]], out)
        v = out
    return O.camera(W, H, fov, v)


def xpoint(m, p):
    out = O.Vec3()
    O.lib().orc_transform_point(m, O.Vec3(*p), out)
    return tuple(out)


def xvector(m, p):
    out = O.Vec3()
    O.lib().orc_transform_vector(m, O.Vec3(*p), out)
    return tuple(out)


def ball(c, r, **m):
    return shp(SPHERE, ("scaling", r, r, r), ("translation", *c), m=mat(**m) if m else None)


def hits_of(case, step=1):
    """The oracle's hit record of every `step`-th pixel centre: [(x, y, RtcHit)]."""
    a = case.arr()
    out = []
    for y in range(0, case.cam.vsize, step):
        for x in range(0, case.cam.hsize, step):
            out.append((x, y, O.color_at(a, case.n, case.light, pixel_ray(case.cam, x, y), 5, want_hit=True)[1]))
    return out


def light_dist(case, h):
    p = tuple(case.light.position)
    return math.dist(p, tuple(h.over_point))


def light_cell(d):
    """The direction cell of a direction FROM the light (light_cell, rtc_kernels.hip), in plain f64."""
    ax = [abs(v) for v in d]
    a = 0 if ax[0] >= ax[1] and ax[0] >= ax[2] else (1 if ax[1] >= ax[2] else 2)
    m, u, v = d[a], d[(a + 1) % 3], d[(a + 2) % 3]
    iu = min(max(int((u / abs(m) + 1.) * 0.5 * LIGHT_R), 0), LIGHT_R - 1)
    iv = min(max(int((v / abs(m) + 1.) * 0.5 * LIGHT_R), 0), LIGHT_R - 1)
    return ((a * 2 + (1 if m < 0 else 0)) * LIGHT_R + iv) * LIGHT_R + iu


def bound_resid(s):
    """|| A F - I ||_max as bound_of (rtc_api.cpp) evaluates it for a shape's stored inverse; >= 1e-9: no bound."""
    m = list(s.inv)
    a = [[m[0], m[1], m[2]], [m[4], m[5], m[6]], [m[8], m[9], m[10]]]
    det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    f = [[(a[1][1] * a[2][2] - a[1][2] * a[2][1]) / det, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det, (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det],
         [(a[1][2] * a[2][0] - a[1][0] * a[2][2]) / det, (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det],
         [(a[1][0] * a[2][1] - a[1][1] * a[2][0]) / det, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det, (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det]]
    r = 0.
    for i in range(3):
        for j in range(3):
            v = -1. if i == j else 0.
            for k in range(3):
                v += a[i][k] * f[k][j]
            r = max(r, abs(v))
    return r


def ill_conditioned(kind, at, **m):
    """A sphere / cube whose stored inverse fails bound_of's residual test (1.2e-4 against 1e-9) while its determinant
    (-0.27) passes the reference's 1e-8 rule: scaling(1e6, 1e-6, 1) under a strong shear."""
    s = shp(kind, ("scaling", 1e6, 1e-6, 1.), ("shearing", 3., 2.1, 0.9, -3., 1.5, 3.), ("rotation_y", 0.7), ("translation", *at),
            m=mat(**m) if m else None)
    assert bound_resid(s) > 1e-7
    return s


# ------------------------------------------------------------------ CPU-side expectations
def expect_lit_and_shadowed_floor(floor_kind=PLANE):
    def f(case, canvases):
        hs = [h for _, _, h in hits_of(case, 2) if h.hit_index >= 0 and case.shapes[h.hit_index].kind == floor_kind]
        lit, dark = sum(1 for h in hs if not h.shadowed), sum(1 for h in hs if h.shadowed)
        assert lit > 0 and dark > 0, (case.name, lit, dark)
    return f


def expect_some_hits(case, canvases):
    img = canvases[case.modes[-1]]
    assert np.isfinite(img).all() and img.any(), case.name


def expect_untraced_edge_black(case, canvases):
    expect_some_hits(case, canvases)
    if 0 in canvases:       # Camera::render leaves the last row and column alone (camera.rs:120-121)
        assert not canvases[0][-1].any() and not canvases[0][:, -1].any(), case.name


def expect_every_member_decides(first, count):
    """Each of shapes[first : first + count] decides a pixel of its own: the oracle's canvas without it differs. A consumer
    that lost ANY one entry of the list these objects fill would therefore change the picture."""
    def f(case, canvases):
        base = canvases[1]
        assert base.any(), case.name
        for i in range(first, first + count):
            rest = case.shapes[:i] + case.shapes[i + 1:]
            a = (O.RtcShape * len(rest))(*rest)
            assert not np.array_equal(O.render(a, len(rest), case.light, case.cam, mode=1, nthreads=8), base), (case.name, i)
    return f


def expect_sky_band(top):
    """The 8 rows at the top (or bottom) of the oracle's canvas are black, the rest is not."""
    def f(case, canvases):
        img = canvases[1]
        band, rest = (img[:8], img[8:]) if top else (img[-8:], img[:-8])
        assert not band.any() and rest.any(), case.name
        expect_lit_and_shadowed_floor()(case, canvases)
    return f


def expect_many_cells_per_tile(case, canvases):
    """Some 8x8 tile's floor hit points see the light in more than four direction cells."""
    expect_lit_and_shadowed_floor()(case, canvases)
    lp = tuple(case.light.position)
    cells = {}
    for x, y, h in hits_of(case):
        if h.hit_index >= 0:
            cells.setdefault((x // 8, y // 8), set()).add(light_cell(tuple(h.over_point[i] - lp[i] for i in range(3))))
    most = max(len(v) for v in cells.values())
    assert most > 4, (case.name, most)


# ------------------------------------------------------------------ tile-list cases
def fan_of_spheres(cam, tx, ty, k):
    """k spheres inside tile (tx, ty), each 0.3 pixels in angular radius on the centre ray of a pixel of its own: sphere i
    on pixel i % 64 of the tile. Beyond 64 the pixels get a second, nearer sphere of clear glass (refractive index 1:
    the ray goes straight on to the opaque one behind it), so every sphere still decides its pixel."""
    out = []
    for i in range(k):
        j = i % 64
        r6 = pixel_ray(cam, tx * 8 + j % 8, ty * 8 + j // 8)
        o, d = r6[:3], r6[3:]
        t = (5. if i >= 64 else 8.) + 0.05 * j
        m = dict(color=(0.2 + 0.1 * (i % 7), 0.9 - 0.1 * (i % 5), 0.3 + 0.2 * (i % 3)), ambient=0.4)
        if i >= 64:
            m.update(color=(0.3, 0.1, 0.1), transparency=0.9, refractive_index=1.0)
        out.append(ball((o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]), 0.3 * cam.pixel_size * t, **m))
    return out


def string_of_spheres(cam, tx, ty, k, t0, t1):
    """k spheres on the ray through the centre pixel of tile (tx, ty) — the tile cone's axis pixel — each 0.6 pixels in
    angular radius: inside the tile, and more than a tile cone's half-angle (4.5 * sqrt 2 pixels) away from every
    neighbouring tile's axis (8 pixels)."""
    r6 = pixel_ray(cam, tx * 8 + 3, ty * 8 + 3)
    o, d = r6[:3], r6[3:]
    out = []
    for i in range(k):
        t = t0 + (t1 - t0) * i / max(1, k - 1)
        out.append(ball((o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]), 0.6 * cam.pixel_size * t,
                        color=(0.2 + 0.6 * (i % 3 == 0), 0.2 + 0.6 * (i % 3 == 1), 0.2 + 0.6 * (i % 3 == 2)), ambient=0.4))
    return out


def tile_cases():
    cs = []
    W, H = 64, 48
    front = cam_of(W, H, 1.0, (0., 0., 0.), (0., 0., 1.))
    L = O.light((-4., 6., -3.))
    # the 64-entry cap: RTC_TILE_LIST_CAP against cap + 1 (k_bin_tiles counts on, k_trace walks from 65). Every listed sphere
    # decides a pixel of its own, so a list that lost any entry shows. (No row words: the spheres on the tile's edge
    # pixels are inside the neighbouring tiles' circumscribed cones too.)
    for k in (63, 64, 65, 66):
        cs.append(ListCase(f"tile_cap[{k}]", "tile_cap", number(fan_of_spheres(front, 3, 2, k)), L, front,
                           want={"tile": (3, 2, k), "n_unb": 0}, expect=expect_every_member_decides(0, k)))
    # n_unb <= 4u: a floor and more floors hidden under it (the sky stays provable up to four planes)
    for planes in (0, 1, 4, 5):
        shapes = string_of_spheres(front, 3, 2, 10, 5., 8.)
        shapes += [shp(PLANE, ("translation", 0., -2. - i, 0.), m=mat(color=(0.5 + 0.1 * i, 0.6, 0.4), specular=0.)) for i in range(planes)]
        rows = (2, 2) if planes == 0 else ((2, 5) if planes <= 4 else (0, 5))
        cs.append(ListCase(f"plane_count[{planes}]", "n_unb_limit", number(shapes), L, front,
                           want={"tile": (3, 2, 10), "rows": rows, "n_unb": planes}, expect=expect_some_hits))
    # plane poses, each seen from its +y and from its -y side (s = +1 / -1 in cone_misses_plane)
    poses = {"ceiling": (("translation", 0., 4., 0.),), "wall_x": (("rotation_x", math.pi / 2), ("translation", 0., 0., 9.)),
             "wall_z": (("rotation_z", math.pi / 2), ("translation", -5., 0., 0.)), "tilted": (("rotation_z", 0.2),)}
    for nm, ops in poses.items():
        M = O.chain(*ops)
        for side, s in (("above", 1.), ("below", -1.)):
            shapes = [shp(PLANE, *ops, m=mat(pattern=("checker", (0.2, 0.3, 0.4), (0.9, 0.8, 0.7), None), specular=0.2))]
            rng = np.random.default_rng(len(cs))
            for i in range(20):
                c = xpoint(M, (float(rng.uniform(-3, 3)), s * float(rng.uniform(0.3, 2.)), float(rng.uniform(-2, 6))))
                shapes.append(ball(c, float(rng.uniform(0.1, 0.4)), color=tuple(rng.uniform(0.1, 1., 3))))
            cam = cam_of(W, H, 1.1, xpoint(M, (0., s * 2., -6.)), xpoint(M, (0., s * 0.5, 4.)), xvector(M, (0., 1., 0.)))
            # The view is pitched 8.5 degrees towards the plane and spans +-24.7 vertically: the tile row farthest from the
            # plane (the top one from above, the bottom one from below, `up` being the plane's +y) looks at least 8 degrees
            # away from it — provable, and empty (expect_sky_band) — while the next one ends 0.2 degrees from the horizon, so
            # its tiles' circumscribed cones (5.7 degrees) dip below it: not provable.
            cs.append(ListCase(f"plane_pose[{nm},{side}]", "plane_pose", number(shapes), O.light(xpoint(M, (-4., s * 6., -3.))), cam,
                               want={"n_unb": 1, "rows": (1, 5) if s > 0 else (0, 4)}, expect=expect_sky_band(top=s > 0)))
    # the camera origin ON the plane: o'.y == 0, no proof (every tile row stays)
    shapes = [shp(PLANE, m=mat(color=(0.4, 0.6, 0.8)))] + [ball((0.5 * i - 2., 0.6, 3. + 0.3 * i), 0.3, color=(0.9, 0.4, 0.2)) for i in range(8)]
    level = cam_of(W, H, 1.0, (0., 0., -6.), (0., 0., 4.))      # (a level view: its inverse puts the origin at y == 0.0 exactly)
    assert pixel_ray(level, 0, 0)[1] == 0.0
    cs.append(ListCase("plane_pose[through_camera]", "plane_oy_guard", number(shapes), L, level,
                       want={"n_unb": 1, "rows": (0, 5)}, expect=expect_some_hits))
    # extreme scales (determinant 1): the stored inverse row (0, 1/sy, 0) has a squared norm of 2^920 / 2^-920, beyond the rr
    # guards on either side — both are reachable under the 1e-8 rule
    for nm, sc in (("row_norm_above_2^900", (2.0 ** 230, 2.0 ** -460, 2.0 ** 230)), ("row_norm_below_2^-900", (2.0 ** -230, 2.0 ** 460, 2.0 ** -230))):
        shapes = [shp(PLANE, ("scaling", *sc), m=mat(color=(0.4, 0.6, 0.8), specular=0., shininess=0.))]
        shapes += [ball((0.5 * i - 2., 0.6, 3. + 0.3 * i), 0.3, color=(0.9, 0.4, 0.2)) for i in range(8)]
        cs.append(ListCase(f"plane_scale[{nm}]", "plane_rr_guard", number(shapes), L, cam_of(W, H, 1.0, (0., 2., -6.), (0., 1., 4.)),
                           want={"n_unb": 1, "rows": (0, 5)}, expect=expect_some_hits))
    # unbounded objects that are no planes (bound_of gives r = +inf): kind_s[k] != RTC_PLANE, no proof at all
    for kind, nm in ((SPHERE, "sphere"), (CUBE, "cube")):
        shapes = [ill_conditioned(kind, (0.5, 1., 6.), color=(0.9, 0.9, 0.2))]
        shapes += [ball((0.5 * i - 2., -0.5, 3. + 0.3 * i), 0.3, color=(0.2, 0.4, 0.9)) for i in range(8)]
        cs.append(ListCase(f"unbounded[{nm}]", "unbounded_non_plane", number(shapes), L, cam_of(W, H, 1.0, (0., 1., -6.), (0., 0., 4.)),
                           want={"n_unb": 1, "rows": (0, 5)}, expect=expect_some_hits))
    shapes = [ill_conditioned(SPHERE, (0.5, 1., 6.)), ill_conditioned(CUBE, (-1., 0.5, 7.)), shp(PLANE, ("translation", 0., -1., 0.))]
    shapes += [ball((0.5 * i - 2., -0.5, 3. + 0.3 * i), 0.3, color=(0.2, 0.4, 0.9)) for i in range(40)]
    cs.append(ListCase("unbounded[both_and_floor,lists]", "unbounded_non_plane", number(shapes), L, cam_of(W, H, 1.0, (0., 1., -6.), (0., 0., 4.)),
                       want={"n_unb": 3, "rows": (0, 5)}, expect=expect_some_hits))
    # wide cones: the centre tiles' corner rays are more than acos(0.7) from their axis (!narrow -> off): every bounded object
    # is their candidate — 40 of them fit a list, 300 overflow it
    for fov in (3.0, 3.1):
        for n in (40, 300):
            for (w, h) in ((64, 48), (16, 16)):
                shapes = field_world(n, seed=int(fov * 10) + n)
                cam = cam_of(w, h, fov, (0., 2., -8.), (0., 1., 5.))
                cs.append(ListCase(f"wide_cone[fov{fov},n{n},{w}x{h}]", "cone_off", shapes, L, cam,
                                   want={"tile": (w // 16, h // 16, n - 1), "n_unb": 1}, expect=expect_some_hits))
    # a very narrow view: the whole string inside one tile of a frame that sees 1e-3 rad
    far = cam_of(W, H, 1e-3, (0., 0., -1000.), (0., 0., 0.))
    cs.append(ListCase("narrow_cone[fov1e-3]", "cone_narrow", number(string_of_spheres(far, 4, 3, 30, 900., 1100.)), O.light((-400., 600., -1300.)), far,
                       want={"tile": (4, 3, 30)}, expect=expect_some_hits))   # (no row words: 1000 away the f32 cones' margins reach other tiles)
    # camera poses over one world of 60 objects and a floor
    base = field_world(61, seed=7)
    poses = {
        "roll": (dict(frm=(0., 2., -8.), to=(0., 1., 5.), up=(1., 1., 0.)), []),
        "straight_down": (dict(frm=(0., 5., 0.), to=(0., 0., 0.), up=(0., 0., 1.)), []),
        "inside_sphere": (dict(frm=(0., 2., -8.), to=(0., 1., 5.)), [ball((0., 2., -8.), 2.5, color=(0.6, 0.7, 0.9))]),
        "inside_cube": (dict(frm=(0., 2., -8.), to=(0., 1., 5.)), [shp(CUBE, ("scaling", 3., 3., 3.), ("rotation_y", 0.4), ("translation", 0., 2., -8.),
                                                                         m=mat(color=(0.6, 0.9, 0.7)))]),
        "inside_glass_sphere": (dict(frm=(0., 2., -8.), to=(0., 1., 5.)), [ball((0., 2., -8.), 2.5, color=(0.1, 0.1, 0.1), transparency=0.9,
                                                                                 refractive_index=1.5, reflective=0.2)]),
        "view_scaled": (dict(frm=(0., 2., -8.), to=(0., 1., 5.), pre=("scaling", 2., 1., 1.)), []),
        "view_mirrored": (dict(frm=(0., 2., -8.), to=(0., 1., 5.), pre=("scaling", -1., 1., 1.)), []),
    }
    for nm, (kw, extra) in poses.items():
        cs.append(ListCase(f"camera_pose[{nm}]", "camera_pose", number(list(base) + extra), L, cam_of(W, H, 0.9, **kw), want={"n_unb": 1},
                           expect=expect_some_hits))
    off = (1e6, 1e6, 1e6)     # the world, the light and the camera 1e6 away on every axis: the f32 apex rounds by 0.06
    cs.append(ListCase("camera_pose[far_1e6]", "camera_pose", field_world(61, seed=7, off=off), O.light((-4. + 1e6, 6. + 1e6, -3. + 1e6)),
                       cam_of(W, H, 0.9, (1e6, 2. + 1e6, -8. + 1e6), (1e6, 1. + 1e6, 5. + 1e6)), want={"n_unb": 1}, expect=expect_some_hits))
    # frame sizes that end inside a tile, in both modes; H = 65 in Camera::render: the last tile row is the untraced row only
    for (w, h) in ((63, 65), (65, 63), (129, 7), (7, 129), (1, 9)):
        cs.append(ListCase(f"frame[{w}x{h}]", "frame_edges", base, L, cam_of(w, h, 0.9, (0., 2., -8.), (0., 1., 5.)), want={"n_unb": 1},
                           expect=expect_untraced_edge_black if min(w, h) > 1 else None, modes=(0, 1)))
    return cs


def field_world(n, seed, off=(0., 0., 0.), variant="flat", floor=True):
    """n objects: a floor (last) and n - 1 small spheres, cubes and sheared ellipsoids hovering over it."""
    rng = np.random.default_rng(seed)
    u = lambda a, b: float(rng.uniform(a, b))
    shapes = []
    for i in range(n - (1 if floor else 0)):
        r = u(0.08, 0.35)
        c = (u(-5, 5) + off[0], u(0.4, 3.) + off[1], u(-3, 10) + off[2])
        m = dict(color=(u(0.1, 1), u(0.1, 1), u(0.1, 1)), specular=0.3, shininess=40.)
        if variant == "reflective" and i % 3 == 0:
            m["reflective"] = 0.5
        if variant == "glass" and i % 3 == 0:
            m.update(transparency=0.8, refractive_index=1.5, reflective=0.2)
        if variant == "shapes" and i % 2 == 0:
            ops = (("scaling", r, r * u(0.3, 2.), r), ("shearing", u(-1, 1), 0., u(-1, 1), 0., 0., u(-1, 1)), ("rotation_y", u(0, 3)), ("translation", *c))
            shapes.append(shp(CUBE if i % 4 == 0 else SPHERE, *ops, m=mat(**m)))
        else:
            shapes.append(ball(c, r, **m))
    if floor:
        fm = dict(pattern=("checker", (0.3,) * 3, (0.7,) * 3, None), specular=0.)
        if variant == "reflective":
            fm["reflective"] = 0.3
        shapes.append(shp(PLANE, ("translation", *off), m=mat(**fm)))
    return number(shapes)


# ------------------------------------------------------------------ light-list cases
def light_cases():
    cs = []
    W, H = 64, 48
    cam = cam_of(W, H, 0.9, (0., 4., -9.), (0., 0.5, 3.))
    L = O.light((-3., 8., -2.))
    shadows = expect_lit_and_shadowed_floor()
    # object counts: lists from 32 objects; 256 / 257 small-world against two-level path; a last group partly filled
    for n in (31, 32, 33, 256, 257, 320, 321):
        cs.append(ListCase(f"light_count[{n}]", "light_n", field_world(n, seed=n), L, cam, want={"n_unb": 1}, expect=shadows))
    # the per-cell cap: k spheres inside ONE direction cell (0.0004 rad each, the cell is 0.0156 wide) at 30..70 from the
    # light, the others far from that direction. Cell (70, 70) of the -y face; the shadows fall around (10.16, 0, 10.16).
    lp = (0., 100., 0.)
    g = (70 + 0.5) * 2. / LIGHT_R - 1.
    d = (g, -1., g)
    cell = light_cell(d)
    assert cell == ((1 * 2 + 1) * LIGHT_R + 70) * LIGHT_R + 70
    dl = math.sqrt(2 * g * g + 1.)
    for k, fill in ((16, 20), (17, 20), (128, 140), (129, 140)):
        shapes = [shp(PLANE, m=mat(color=(0.8, 0.8, 0.7), specular=0.))]
        side = math.ceil(math.sqrt(k))
        for i in range(k):      # fanned over the cell (+-0.0055 of its +-0.0078), 0.0004 rad each: every one shadows a floor spot of its own
            du, dv = (-0.0055 + 0.011 * (i % side) / (side - 1), -0.0055 + 0.011 * (i // side) / (side - 1))
            di = (g + dv, -1., g + du)
            t = 30. + 40. * ((i * 37) % k) / k
            shapes.append(ball((lp[0] + t * di[0], lp[1] + t * di[1], lp[2] + t * di[2]), 0.0004 * t * dl, color=(0.9, 0.2, 0.2)))
            assert light_cell(di) == cell
        shapes += [ball((-60. + 0.2 * i, 5. + 0.1 * i, 30. + 10. * (i % 7)), 2., color=(0.2, 0.9, 0.2)) for i in range(fill)]
        P = (100. * g, 0., 100. * g)    # straight down from under the spheres: 0.028 per pixel, a shadow spot is 0.08 wide, 0.1 apart
        c = ListCase(f"light_cell_cap[{k}]", "light_cap", number(shapes), O.light(lp), cam_of(64, 64, 0.09, (P[0], 20., P[2]), P, (0., 0., 1.)),
                     want={"n_unb": 1, "cell": (cell, k)}, expect=expect_every_member_decides(1, k))
        assert c.cap == (CAP_SMALL if k < 100 else CAP_LARGE)
        cs.append(c)
    # reach: a compact cluster right under the light over a floor seen to the horizon: hit points on both sides of 2 * far
    for n in (41, 300):
        rng = np.random.default_rng(n)
        shapes = [ball((float(rng.uniform(-.8, .8)), 3. + float(rng.uniform(-.8, .8)), float(rng.uniform(-.8, .8))), 0.12, color=(0.9, 0.5, 0.1))
                  for _ in range(n - 1)]
        shapes.append(shp(PLANE, m=mat(pattern=("checker", (0.3,) * 3, (0.7,) * 3, None), specular=0.)))
        far = max(math.dist((0., 5., 0.), xpoint(O.inverse(s.inv), (0., 0., 0.))) + 0.12 for s in shapes[:-1])

        def both_sides(case, canvases, far=far):
            ds = [light_dist(case, h) for _, _, h in hits_of(case, 2) if h.hit_index == case.n - 1]
            assert min(ds) < 1.9 * far and max(ds) > 2.1 * far, (case.name, min(ds), max(ds), far)
            expect_lit_and_shadowed_floor()(case, canvases)
        cs.append(ListCase(f"light_reach[{n}]", "light_reach", number(shapes), O.light((0., 5., 0.)), cam_of(W, H, 1.2, (0., 2., -9.), (0., 1.5, 0.)),
                           want={"n_unb": 1, "reach": (2. * far * 0.999, 2. * far * 1.001)}, expect=both_sides))
    # the light 0.05 above the floor inside the view: neighbouring floor points see it in directions cells apart
    for n in (60, 300):
        grounded = [ball((-3. + 0.7 * i, 0.25, 1. + (i % 3)), 0.25, color=(0.9, 0.7, 0.1)) for i in range(10)]   # low enough to shadow the floor
        cs.append(ListCase(f"light_low[{n}]", "light_many_cells", number(grounded + list(field_world(n - 10, seed=n + 1))), O.light((0.3, 0.05, 2.)), cam,
                           want={"n_unb": 1}, expect=expect_many_cells_per_tile))
    # light positions
    w60 = field_world(60, seed=3)
    big = ball((1., 1.5, 3.), 1.2, color=(0.8, 0.3, 0.3))
    box = shp(CUBE, ("scaling", 1.5, 1.5, 1.5), ("rotation_y", 0.3), ("translation", 1., 1.5, 3.), m=mat(color=(0.3, 0.8, 0.3)))
    for nm, shapes, pos, exp in (("sphere_centre", [big] + list(w60), (1., 1.5, 3.), expect_some_hits),
                                 ("inside_cube", [box] + list(w60), (1.2, 1.6, 3.1), expect_some_hits),
                                 ("on_floor", w60, (1., 0., 2.), expect_some_hits), ("below_floor", w60, (1., -2., 2.), expect_some_hits),
                                 ("at_camera", w60, (0., 4., -9.), expect_some_hits)):
        cs.append(ListCase(f"light_at[{nm}]", "light_position", number(list(shapes)), O.light(pos), cam, want={"n_unb": 1}, expect=exp))
    off = (1e6, 1e6, 1e6)
    cs.append(ListCase("light_at[far_1e6]", "light_position", field_world(60, seed=3, off=off), O.light((-3. + 1e6, 8. + 1e6, -2. + 1e6)),
                       cam_of(W, H, 0.9, (1e6, 4. + 1e6, -9. + 1e6), (1e6, 0.5 + 1e6, 3. + 1e6)), want={"n_unb": 1}, expect=shadows))
    # directions on a face border and on an axis: seen straight down from (4, 6, 0) on odd frame sizes, the centre column
    # of floor points has x = 4 — (x, -4, z) from the light at (0, 4, 0): |dx| == |dy| — and the centre row z = 0
    down = cam_of(65, 49, 0.8, (4., 6., 0.), (4., 0., 0.), (0., 0., 1.))

    def on_border(case, canvases):
        hs = [(x, y, h) for x, y, h in hits_of(case) if x == 32 or y == 24]
        bx = [abs(abs(h.over_point[0] - 0.) - abs(h.over_point[1] - 4.)) for x, y, h in hs if x == 32 and h.hit_index == case.n - 1]
        bz = [abs(h.over_point[2]) for x, y, h in hs if y == 24 and h.hit_index == case.n - 1]
        assert len(bx) > 10 and max(bx) < 1e-7 and len(bz) > 10 and max(bz) < 1e-9, (len(bx), max(bx), len(bz), max(bz))
    for n in (60, 300):
        rng = np.random.default_rng(n)
        shapes = [ball((float(rng.uniform(0.5, 5.)), float(rng.uniform(1., 3.)), float(rng.uniform(-2.5, 2.5))), 0.15, color=(0.9, 0.6, 0.2)) for _ in range(n - 1)]
        shapes.append(shp(PLANE, m=mat(color=(0.7, 0.7, 0.8), specular=0.)))
        cs.append(ListCase(f"light_face_border[{n}]", "light_face_border", number(shapes), O.light((0., 4., 0.)), down, want={"n_unb": 1}, expect=on_border))
    # !pre_ok: shadow origins beyond pre_limit = 64 x (the bounded objects' extent around the world origin). A translation
    # cannot get there (the extent grows with it); a low light far behind a compact cluster can: the cluster's shadows fall
    # ~200 away (|over|_1 > 64 * 2.2), and the light's distance keeps them within reach (2 * 201).
    for n in (40, 300):
        rng = np.random.default_rng(n + 9)
        shapes = [ball((float(rng.uniform(-.5, .5)), 1. + float(rng.uniform(-.3, .3)), float(rng.uniform(-.5, .5))), 0.1, color=(0.9, 0.6, 0.2)) for _ in range(n - 1)]
        shapes.append(shp(PLANE, m=mat(color=(0.7, 0.7, 0.8), specular=0.)))

        def beyond_limit(case, canvases):
            hs = [h for _, _, h in hits_of(case, 2) if h.hit_index == case.n - 1]
            far_shadowed = [h for h in hs if h.shadowed and sum(abs(v) for v in h.over_point) > 64. * 2.2 and light_dist(case, h) < 402.]
            assert len(far_shadowed) > 0 and any(not h.shadowed for h in hs), (case.name, len(far_shadowed))
        cs.append(ListCase(f"light_pre_limit[{n}]", "light_pre_ok", number(shapes), O.light((-200., 2., 0.)),
                           cam_of(W, H, 0.5, (200., 12., -25.), (200., 0., 0.)), want={"n_unb": 1}, expect=beyond_limit))
    # occluder shapes
    for n in (60, 300):
        cs.append(ListCase(f"occluder[cubes_and_sheared,{n}]", "light_occluder", field_world(n, seed=n + 2, variant="shapes"), L, cam, want={"n_unb": 1}, expect=shadows))
        needle = shp(SPHERE, ("scaling", 0.03, 6., 0.03), ("rotation_z", 1.2), ("rotation_y", 0.5), ("translation", 0., 2., 3.), m=mat(color=(0.9, 0.1, 0.1)))
        cs.append(ListCase(f"occluder[needle,{n}]", "light_occluder", number([needle] + list(field_world(n - 1, seed=n + 3))), L, cam, want={"n_unb": 1}, expect=shadows))
        huge = ball((0., 0., 0.), 40., color=(0.5, 0.6, 0.9))      # around the light, the camera and everything: in every cell
        cs.append(ListCase(f"occluder[in_every_cell,{n}]", "light_occluder", number([huge] + list(field_world(n - 1, seed=n + 4))), L, cam,
                           want={"n_unb": 1, "cell_min": 1}, expect=shadows))
        wall = shp(PLANE, ("rotation_z", math.pi / 2), ("translation", -1.5, 0., 0.), m=mat(color=(0.6, 0.5, 0.4)))   # between the light and the floor
        cs.append(ListCase(f"occluder[wall_plane,{n}]", "light_occluder", number([wall] + list(field_world(n - 1, seed=n + 5))), L, cam,
                           want={"n_unb": 2}, expect=expect_some_hits))
        for variant in ("reflective", "glass"):
            cs.append(ListCase(f"secondary[{variant},{n}]", "light_secondary", field_world(n, seed=n + 6, variant=variant), L, cam, want={"n_unb": 1}, expect=shadows))
    return cs


# ------------------------------------------------------------------ the seeded family
def list_world(seed, size_class):
    """adversarial_scene's ingredients (test_gpu_parity.py) at the sizes that reach the lists: 32..256 ("small") or
    257..1500 ("large") objects, 0..6 planes in arbitrary poses, the light and the camera now and then inside an object,
    on a plane, at each other's place or 1e6 away. A 96x64 frame."""
    rng = np.random.default_rng([seed, 0 if size_class == "small" else 1])
    u = lambda a, b: float(rng.uniform(a, b))
    off = (1e6, 1e6, 1e6) if rng.random() < 0.1 else (0., 0., 0.)
    P = lambda x, y, z: (x + off[0], y + off[1], z + off[2])
    n = int(rng.integers(32, 257)) if size_class == "small" else int(rng.integers(257, 1501))
    nplanes = int(rng.integers(0, 7))
    shapes = []
    for i in range(n - nplanes):
        k = int(rng.integers(0, 7))
        c = P(u(-6, 6), u(0, 5), u(-4, 14))
        if k == 0:      # tiny and far
            ops = (("scaling", *(3 * [u(0.01, 0.05)])), ("translation", *P(u(-30, 30), u(0, 20), u(10, 90))))
        elif k == 1 and rng.random() < 0.15:   # huge, may hold the camera or the light
            ops = (("scaling", *(3 * [u(5, 30)])), ("translation", *P(u(-10, 10), u(-10, 10), u(-10, 30))))
        elif k == 2:    # needle / pancake
            ops = (("scaling", u(0.02, 0.1), u(1, 4), u(0.02, 2)), ("rotation_x", u(0, 3)), ("rotation_z", u(0, 3)), ("translation", *c))
        elif k == 3:    # sheared
            ops = (("shearing", *[u(-1, 1) for _ in range(6)]), ("scaling", u(0.1, 0.6), u(0.1, 0.6), u(0.1, 0.6)), ("translation", *c))
        elif k == 4:    # behind / beside the camera
            ops = (("scaling", *(3 * [u(0.3, 2)])), ("translation", *P(u(-6, 6), u(-1, 4), u(-14, -4))))
        else:
            ops = (("scaling", *(3 * [u(0.08, 0.5)])), ("translation", *c))
        glass = rng.random() < 0.1
        m = mat(color=(u(0, 1), u(0, 1), u(0, 1)), ambient=u(0, 0.3), diffuse=u(0.2, 0.9), specular=u(0, 0.9), shininess=u(1, 300),
                reflective=(u(0.1, 0.9) if rng.random() < 0.15 else 0.0), transparency=(u(0.3, 1.0) if glass else 0.0),
                refractive_index=(u(1.05, 2.2) if glass else 1.0))
        try:
            shapes.append(shp(CUBE if rng.random() < 0.25 else SPHERE, *ops, m=m))
        except ValueError:
            pass        # singular by the reference's 1e-8 determinant rule
    for i in range(nplanes):
        ops = (("rotation_x", u(-3.2, 3.2)), ("rotation_z", u(-3.2, 3.2)), ("translation", *P(u(-8, 8), u(-3, 0) if i == 0 else u(-12, 12), u(-5, 20))))
        if i == 0 and rng.random() < 0.6:
            ops = (("rotation_z", u(-0.2, 0.2)), ("translation", *P(0, u(-1, 0), 0)))
        shapes.append(shp(PLANE, *ops, m=mat(reflective=(u(0, 0.5) if rng.random() < 0.3 else 0.), specular=0.1,
                                             pattern=("checker", (0.3,) * 3, (0.7,) * 3, None))))
    frm = P(u(-3, 3), u(0.2, 4), u(-9, -3))
    lpos = P(u(-6, 6), u(1, 9), u(-9, 2))
    r = rng.random()
    if r < 0.1:
        lpos = frm                                           # the light at the camera
    elif r < 0.2:
        lpos = xpoint(O.inverse(shapes[0].inv), (0., 0., 0.))  # at an object's centre
    elif r < 0.3 and nplanes:
        lpos = xpoint(O.inverse(shapes[-1].inv), (u(-2, 2), 0., u(-2, 2)))   # on a plane
    elif r < 0.4:
        lpos = P(u(-3, 3), 0.05, u(0, 5))                    # low over the usual floor height
    if rng.random() < 0.1:
        frm = xpoint(O.inverse(shapes[1].inv), (0.1, 0.1, 0.1))             # the camera inside an object
    up = (1., 1., 0.) if rng.random() < 0.1 else (0., 1., 0.)
    cam = cam_of(96, 64, u(0.4, 2.0) if rng.random() < 0.9 else 3.0, frm, P(u(-1, 1), u(0, 2), u(0, 4)), up)
    return number(shapes), O.light(lpos), cam


def as_world(rtc, shapes, light):
    """The product binding's World of a case (world ids as the case set them)."""
    w = rtc.World(light)
    w.shapes = list(shapes)
    return w


def all_cases():
    return tile_cases() + light_cases()
