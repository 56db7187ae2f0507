"""Boundary cases for the parity suite: rays and worlds placed exactly on the comparisons where the
intersect, shadow, shading, refraction, pattern and binning code decides something (helper module,
not collected; used by test_host_boundaries.py and test_gpu_boundaries.py).

Two kinds of case, both deterministic and built on the CPU oracle only:

* exact constructions: inputs whose outcome follows from the reference source line they cite; each
  carries an `expect` check on the oracle's literal (sorted-list) form;
* bisected pairs: one scalar parameter (a ray offset, a light coordinate, a sphere position, a camera
  pitch, a refractive index) is bisected over its f64 bit patterns until two adjacent doubles
  disagree on the targeted decision; the case family holds both doubles and +-2 ulp around them.

Every value is finite, no direction is zero, world-space direction components stay within 2^100.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
from dataclasses import dataclass, field

import oracle as O

EPS = 1e-8                                   # Vector::EPSILON vec.rs:16
SPHERE, PLANE, CUBE = 0, 1, 2
PAD_SPHERES = 300                            # > 256 objects: the default path becomes the two-level Morton cull


@dataclass
class Case:
    name: str
    decision: str
    shapes: list
    light: object
    rays: list
    expect: object = None                    # callable(hits, rgbs) on the literal oracle form (exact constructions)
    kind: str = "exact"

    def arr(self):
        a = (O.RtcShape * max(1, len(self.shapes)))()
        for i, s in enumerate(self.shapes):
            a[i] = s
        return a


@dataclass
class Pair:
    """Two adjacent doubles of a bisected parameter: cases[lo] and cases[hi] (ray 0 of each) must differ in `pred`."""
    name: str
    decision: str
    lo: Case
    hi: Case
    pred: object = field(repr=False)


@dataclass
class RenderCase:
    name: str
    decision: str
    shapes: list
    light: object
    cam: object

    def arr(self):
        a = (O.RtcShape * max(1, len(self.shapes)))()
        for i, s in enumerate(self.shapes):
            a[i] = s
        return a


# ------------------------------------------------------------------ small helpers
def _key(x: float) -> int:
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)


def _unkey(k: int) -> float:
    if k >= 0:
        return struct.unpack("<d", struct.pack("<q", k))[0]
    return -struct.unpack("<d", struct.pack("<q", -k))[0]


def ulps(x: float, n: int) -> float:
    return _unkey(_key(x) + n)


def bisect(f, lo: float, hi: float):
    """Adjacent doubles (a, b) in [lo, hi] with f(a) == f(lo) != f(b); f(lo) != f(hi) is required."""
    fa = f(lo)
    if f(hi) == fa:
        raise ValueError("bisect: no change of the decision between the end points")
    a, b = _key(lo), _key(hi)
    while abs(b - a) > 1:
        m = (a + b) // 2
        if f(_unkey(m)) == fa:
            a = m
        else:
            b = m
    return _unkey(a), _unkey(b)


def mat(**kw):
    return O.material(**kw)


def shp(kind, *ops, m=None, wid=None):
    s = O.shape(kind, O.chain(*ops) if ops else O.mat(), m)
    if wid is not None:
        s.world_id = wid
    return s


def number(shapes, ids=None):
    """World::add_shape ids (shape.rs:661-667), or the ids given."""
    for i, s in enumerate(shapes):
        s.world_id = ids[i] if ids is not None else i + 1
    return shapes


def probe(shapes, lgt, ray, remaining=5, streaming=False):
    a = (O.RtcShape * max(1, len(shapes)))()
    for i, s in enumerate(shapes):
        a[i] = s
    rgb, h = O.color_at(a, len(shapes), lgt, tuple(ray), remaining, streaming=streaming, want_hit=True)
    return rgb, h


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _normalize(v):
    m = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return (v[0] / m, v[1] / m, v[2] / m)


def _reflect(v, n):
    k = 2. * _dot(v, n)
    return (v[0] - n[0] * k, v[1] - n[1] * k, v[2] - n[2] * k)


# ------------------------------------------------------------------ decisions, restated from the hit record
def d_hit(shapes, lgt, ray):
    return probe(shapes, lgt, ray)[1].hit_index


def d_shadowed(shapes, lgt, ray):
    h = probe(shapes, lgt, ray)[1]
    return (h.hit_index, h.shadowed)


def d_inside(shapes, lgt, ray):
    h = probe(shapes, lgt, ray)[1]
    return (h.hit_index, h.inside)


def tir(h):
    """refracted_color shape.rs:756-759 / schlick shape.rs:771-775: sin2_t > 1.0."""
    n = h.n1 / h.n2
    cos_i = _dot(h.eyev, h.normal)
    return (n * n) * (1.0 - cos_i * cos_i) > 1.0


def d_tir(shapes, lgt, ray):
    h = probe(shapes, lgt, ray)[1]
    return (h.hit_index, h.hit_index >= 0 and tir(h))


def _light_terms(h, lgt):
    """material.rs:335-352: light_dot_normal and reflect_dot_eye at the hit's over_point."""
    p = tuple(lgt.position)
    lightv = _normalize((p[0] - h.over_point[0], p[1] - h.over_point[1], p[2] - h.over_point[2]))
    ldn = _dot(lightv, h.normal)
    rde = _dot(_reflect((-lightv[0], -lightv[1], -lightv[2]), h.normal), h.eyev)
    return ldn, rde


def d_ldn(shapes, lgt, ray):
    h = probe(shapes, lgt, ray)[1]
    return (h.hit_index, h.shadowed, h.hit_index >= 0 and _light_terms(h, lgt)[0] < 0.)


def d_rde(shapes, lgt, ray):
    h = probe(shapes, lgt, ray)[1]
    return (h.hit_index, h.shadowed, h.hit_index >= 0 and _light_terms(h, lgt)[1] <= 0.)


def d_pattern(shapes, lgt, ray):
    """material.rs:41-45 at the over_point lighting() receives (shape.rs:689-690)."""
    h = probe(shapes, lgt, ray)[1]
    if h.hit_index < 0:
        return None
    s = shapes[h.hit_index]
    rgb = O.Vec3()
    O.lib().orc_pattern_at_shape(C.byref(s.material), C.byref(s), O.Vec3(*h.over_point), rgb)
    return tuple(rgb)


PREDS = {"hit": d_hit, "shadowed": d_shadowed, "inside": d_inside, "tir": d_tir, "ldn": d_ldn, "rde": d_rde,
         "pattern": d_pattern}


def family(name, decision, lo, hi, build, pred=None):
    """Bisect `build(x) -> (shapes, light, ray)` over x in [lo, hi] on `pred`; six cases: the flip pair and +-2 ulp."""
    pred = pred or PREDS[decision]
    a, b = bisect(lambda x: pred(*build(x)), lo, hi)
    cases = []
    for i, x in enumerate((ulps(a, -2), ulps(a, -1), a, b, ulps(b, 1), ulps(b, 2))):
        shapes, lgt, ray = build(x)
        cases.append(Case(f"{name}[{i - 2 if i < 3 else i - 3:+d}{'lo' if i < 3 else 'hi'}]", decision, shapes, lgt, [tuple(ray)],
                          kind="bisect"))
    return cases, Pair(name, decision, cases[2], cases[3], lambda c: pred(c.shapes, c.light, c.rays[0]))


# ------------------------------------------------------------------ exact constructions
def _eq3(a, b):
    return tuple(a) == tuple(b)


def exact_cases():
    L = O.light
    cs = []

    # Sphere, shape.rs:361-375: disc < 0. at exactly 0 is a tangent hit (one double root t1 == t2).
    def tangent(h, _):
        assert h[0].hit_index == 0 and h[0].t == 5.0 and _eq3(h[0].normal, (1., 0., 0.)), "shape.rs:366: disc == 0 is a hit"
    rays = [(1., 0., -5., 0., 0., 1.)] + [(ulps(1., k), 0., -5., 0., 0., 1.) for k in (-1, 1, 2, 40, 41)]
    cs.append(Case("sphere_tangent_disc0", "sphere_disc", number([shp(SPHERE)]), L(), rays, tangent))
    # a ray starting on the surface (t1 = +0) and one starting inside (t1 < 0 <= t2), shape.rs:220-232 get_hit
    def on_surface(h, _):
        assert h[0].hit_index == 0 and h[0].t == 0.0 and not h[0].inside, "t1 == 0.0 is the hit (shape.rs:224 t >= 0.0)"
        assert h[1].hit_index == 0 and h[1].t == 1.0 and h[1].inside, "inside: t1 < 0 <= t2 picks t2 (shape.rs:224)"
        assert h[2].hit_index == 0 and h[2].t == 0.0 and h[2].inside, "exit root t2 == 0.0 is the hit"
        assert h[3].hit_index == -1, "both roots negative: no hit"
    rays = [(0., 0., -1., 0., 0., 1.), (0., 0., 0., 0., 0., 1.), (0., 0., 1., 0., 0., 1.), (0., 0., ulps(1., 1), 0., 0., 1.),
            (0., -1., 0., 0., 1., 0.), (0., 0., -1., 0., 0., -1.)]
    cs.append(Case("sphere_ray_on_and_inside_surface", "sphere_roots", number([shp(SPHERE, m=mat(color=(0.3, 0.6, 0.9)))]),
                   L((0., 10., -10.)), rays, on_surface))

    # Plane, shape.rs:463: fabs(d.y) < EPSILON misses; |d.y| == 1e-8 is NOT below it and hits.
    def plane_eps(h, _):
        assert h[0].hit_index == 0 and h[0].t == 1.0, "shape.rs:463: |d.y| == EPSILON is not < EPSILON: a hit"
        assert h[1].hit_index == -1, "|d.y| one ulp below EPSILON: no intersection"
        assert h[2].hit_index == 0
        assert h[3].hit_index == 0 and h[3].t == 1.0 and h[3].inside and h[4].hit_index == -1
    e_lo, e_hi = ulps(EPS, -1), ulps(EPS, 1)
    rays = [(0., EPS, 0., 1., -EPS, 0.), (0., EPS, 0., 1., -e_lo, 0.), (0., EPS, 0., 1., -e_hi, 0.),
            (0., -EPS, 0., 1., EPS, 0.), (0., -EPS, 0., 1., e_lo, 0.), (0., -EPS, 0., 1., e_hi, 0.)]
    cs.append(Case("plane_dy_epsilon", "plane_eps", number([shp(PLANE)]), L(), rays, plane_eps))
    # ray origin on the plane: t = -0/d.y is +0 or -0, both accepted by t >= 0.0 (shape.rs:224)
    def plane_origin(h, _):
        for i in range(4):
            assert h[i].hit_index == 0 and h[i].t == 0.0, f"ray {i}: t = +-0 on the plane is a hit"
    rays = [(0.5, 0., 0.5, 0., -1., 1.), (0.5, 0., 0.5, 0., 1., 1.), (0.5, -0., 0.5, 0., -1., 1.), (0.5, -0., 0.5, 0.25, 0.5, -1.)]
    cs.append(Case("plane_origin_on_plane", "plane_zero_t", number([shp(PLANE)]), L((1., 5., -2.)), rays, plane_origin))
    # plane_t_certainly_negative's guards (rtc_kernels.hip): scaling(2^260, 2^-520, 2^260) has determinant 1 and multiplies
    # the local o.y and d.y by 2^520. o.y = 2^-1020 -> 2^-500 (at the lo guard), d.y = 2^60 -> 2^580 (beyond hi): the quotient
    # -2^-1080 underflows to -0.0, which t >= 0.0 accepts. d.y = 2^-20 -> 2^500 exactly: t = -2^-1000, a miss.
    def plane_underflow(h, _):
        assert h[0].hit_index == 0 and h[0].t == 0.0 and math.copysign(1., h[0].t) == -1.0, "-0.0 >= 0.0: a hit"
        assert h[1].hit_index == 0 and h[1].t == 0.0, "mirror: both negative"
        assert h[2].hit_index == -1 and h[3].hit_index == -1, "t = -2^-1000: no hit"
    sc = ("scaling", 2.0 ** 260, 2.0 ** -520, 2.0 ** 260)
    rays = [(0.25, 2.0 ** -1020, 0.5, 0.5, 2.0 ** 60, 1.0), (0.25, -2.0 ** -1020, 0.5, 0.5, -2.0 ** 60, 1.0),
            (0.25, 2.0 ** -1020, 0.5, 0.5, 2.0 ** -20, 1.0), (0.25, -2.0 ** -1020, 0.5, 0.5, -2.0 ** -20, 1.0),
            (0.25, 2.0 ** -1000, 0.5, 0.5, 2.0 ** 80, 1.0), (0.25, 5e-324, 0.5, 0.5, 2.0 ** 100, 1.0)]
    # (shininess 0: eyev is as long as the direction, and pow(reflect_dot_eye, 0) == 1 keeps the colour finite)
    cs.append(Case("plane_underflow_to_negative_zero", "plane_guard", number([shp(PLANE, sc, m=mat(shininess=0.))]), L((0., 3., 0.)), rays, plane_underflow))

    # Cube check_axis shape.rs:540-564: d.x of 0, -0, +-EPSILON and one ulp either side; o.x of +-1 (a +-0 numerator), 0.5.
    dxs = [0., -0., EPS, -EPS, ulps(EPS, -1), -ulps(EPS, -1), ulps(EPS, 1), -ulps(EPS, 1)]
    rays = [(ox, 0.25, -5., dx, 0., 1.) for ox in (1., -1., 0.5) for dx in dxs]
    def cube_axis(h, _):
        at = lambda ox, dx: h[[1., -1., 0.5].index(ox) * len(dxs) + dxs.index(dx)]
        assert at(1., EPS).hit_index == -1, "|d.x| >= EPSILON divides: tmax = 0/1e-8 = 0 < tmin = 4, a miss"
        assert at(1., ulps(EPS, -1)).hit_index == 0 and at(1., ulps(EPS, -1)).t == 4.0, "|d.x| < EPSILON: tmax = +inf (0 >= 0.0)"
        assert at(1., 0.).hit_index == 0 and at(-1., 0.).hit_index == -1, "o.x = -1: tmin numerator +0 -> +inf, a miss"
        assert at(1., -EPS).hit_index == 0 and at(0.5, EPS).hit_index == 0
    cs.append(Case("cube_check_axis_epsilon", "cube_axis", number([shp(CUBE, m=mat(color=(0.9, 0.2, 0.1)))]), L(), rays, cube_axis))
    # normal_at_local shape.rs:601-610 ties x, then y, then z; a grazing ray along an edge has tmin == tmax (no hit, :587)
    def cube_ties(h, _):
        assert h[0].hit_index == 0 and _eq3(h[0].normal, (1., 0., 0.)), "corner (1,1,-1): the x test comes first"
        assert _eq3(h[1].normal, (0., 1., 0.)), "edge (0,1,-1): y before z"
        assert _eq3(h[2].normal, (-1., 0., 0.)), "edge (-1,0.5,-1) hit from -x: x before z"
        assert h[3].hit_index == -1, "tmin == tmax: grazing an edge is no hit (shape.rs:587 tmin < tmax)"
        assert h[4].hit_index == -1, "o.x == -1, d.x == 0: the tmin numerator +0 gives +inf (shape.rs:553)"
    rays = [(1., 1., -5., 0., 0., 1.), (0., 1., -5., 0., 0., 1.), (-5., 0.5, -5., 1., 0., 1.), (0., 0.25, -2., 1., 0., 1.),
            (-1., -1., -3., 0., 1., 1.), (0.5, 3., 0.5, 0., -2., 0.)]
    cs.append(Case("cube_edge_and_corner_normals", "cube_normal", number([shp(CUBE)]), L((-4., 6., -8.)), rays, cube_ties))

    # Hit ordering: equal t from different objects, the first inserted wins (shape.rs:195-207 _insert_sorted; closer()).
    def first_wins(h, _):
        assert all(x.hit_index == 0 for x in h), "equal t: the lower index wins"
    rays = [(0., 0., -5., 0., 0., 1.), (0.3, 0.2, -4., 0., 0., 1.), (0., 0., 0., 0., 1., 0.), (1., 0., -5., 0., 0., 1.)]
    cs.append(Case("tie_identical_spheres", "tie", number([shp(SPHERE, m=mat(color=(1., 0., 0.))), shp(SPHERE, m=mat(color=(0., 0., 1.))),
                                                         shp(SPHERE, m=mat(color=(0., 1., 0.)))]), L(), rays, first_wins))
    # a cube's top face coplanar with a plane, both orders
    rays = [(0.5, 5., 0.25, 0., -1., 0.), (0.25, 3., -0.5, 0.25, -1., 0.125), (-0.5, 2., 0.75, 0., -0.5, 0.)]
    for nm, order in (("tie_cube_face_then_plane", (CUBE, PLANE)), ("tie_plane_then_cube_face", (PLANE, CUBE))):
        shapes = number([shp(k, ("translation", 0., 1., 0.) if k == PLANE else ("scaling", 1., 1., 1.),
                             m=mat(color=(0.2, 0.8, 0.2) if k == CUBE else (0.8, 0.2, 0.8), reflective=0.25)) for k in order])
        cs.append(Case(nm, "tie", shapes, L(), rays, first_wins))
    # glass cubes face to face at z = 0 and z = 2: A's exit and B's entry have the same t (compute_refractive's containers,
    # shape.rs:115-141), distinct and shared world ids, both insertion orders
    def glass_tie(h, _):
        assert h[1].hit_index == 0 and h[1].t == 1.0, "the first inserted of the two t = 1 entries"
    for nm, zs, ids in (("glass_cubes_face_to_face", (0., 2.), None), ("glass_cubes_face_to_face_shared_id", (0., 2.), [7, 7]),
                        ("glass_cubes_face_to_face_b_first", (2., 0.), None), ("glass_cubes_face_to_face_b_first_shared_id", (2., 0.), [3, 3])):
        shapes = number([shp(CUBE, ("translation", 0., 0., z), m=mat(color=(0.1, 0.2, 0.3), transparency=0.9, reflective=0.3,
                                                                      refractive_index=1.5 if z == 0. else 2.0)) for z in zs], ids)
        rays = [(0.25, 0.5, -5., 0., 0., 1.), (0.25, 0.5, 0., 0., 0., 1.), (0.25, 0.5, 2., 0., 0., -1.), (0.5, 0.25, -5., 0.125, 0.0625, 1.)]
        cs.append(Case(nm, "containers", shapes, O.light((2., 3., -6.)), rays, glass_tie if zs[0] == 0. else None))

    # Shadow shape.rs:716-727: hit.t < distance is strict. A ceiling plane through the light: over_point (0, 1e-8, -4),
    # v = (0, 3 - 1e-8, 0), distance == |v.y| == the ceiling's t exactly -> not shadowed.
    def shadow_equal(h, _):
        assert h[0].hit_index == 0 and h[0].t == 1.0 and not h[0].shadowed, "t == distance is not < distance"
    shapes = number([shp(PLANE), shp(PLANE, ("translation", 0., 3., 0.), m=mat(color=(0.5, 0.5, 0.5)))])
    cs.append(Case("shadow_occluder_t_equals_distance", "shadow", shapes, O.light((0., 3., -4.)), [(0., 1., -5., 0., -1., 1.)], shadow_equal))

    # Shading material.rs:339-352 and the kernel's pow skip (lighting, rtc_kernels.hip): specular +-0, rde exactly 1, shininess
    # 0 / 200 / 1e300; from straight above with the light straight above, reflectv == eyev == normal: rde == 1.
    for sp in (0.0, -0.0, 0.9):
        for sh in (0.0, 200.0, 1e300):
            def rde_one(h, _, sp=sp):
                assert h[0].hit_index == 0 and not h[0].shadowed
                assert _light_terms(h[0], O.light((0., 10., 0.)))[1] == 1.0, "reflect_dot_eye == 1"
            cs.append(Case(f"shading_rde1_spec{sp!r}_shin{sh:g}", "specular", number([shp(PLANE, m=mat(specular=sp, shininess=sh))]),
                           O.light((0., 10., 0.)), [(0., 5., 0., 0., -1., 0.), (0.5, 5., 0.25, 0., -1., 0.), (0., 5., -5., 0., -1., 1.)], rde_one))

    # Refraction: sin2_t == 1.0 exactly (not > 1.0: no total internal reflection, shape.rs:758, :773). Inside a glass cube
    # leaving through z = 1 (normal flipped to (0,0,-1), cos_i == d.z == 0.5): n1 = 1.1547005383792515 (n2 = 1.0) makes
    # (n1 * n1) * (1 - 0.25) round to exactly 1.0.
    ior = _exact_index(0.5)
    def tir_edge(h, rgbs, shapes=shapes, rays=rays):
        assert h[0].hit_index == 0 and h[0].inside and h[0].n1 == ior and h[0].n2 == 1.0
        n = h[0].n1 / h[0].n2
        ci = _dot(h[0].eyev, h[0].normal)
        assert ci == 0.5 and (n * n) * (1.0 - ci * ci) == 1.0 and not tir(h[0]), "sin2_t == 1.0 is not > 1.0"
        assert not tir(h[2]), "a larger cos_i: sin2_t < 1.0"
        assert (rgbs[0] - probe(shapes, O.light((1., 8., -9.)), rays[0], remaining=0)[0]).max() > 0.1, "the refracted ray carries colour"
    rays = [(0., 0., 0., 0.25, 0., 0.5), (0., 0., 0., 0.25, 0., ulps(0.5, -1)), (0., 0., 0., 0.25, 0., ulps(0.5, 1)),
            (0., 0., 0., 0.25, 0.125, 0.5)]
    # (not reflective: Schlick's reflectance is exactly 1 at sin2_t == 1 and would zero the refracted term; the grazing
    # refracted ray runs along +x just outside the face and meets the sphere at x = 3, so it carries colour)
    shapes = number([shp(CUBE, m=mat(color=(0.2, 0.3, 0.4), transparency=0.5, refractive_index=ior)),
                     shp(PLANE, ("translation", 0., -3., 0.), m=mat(pattern=("checker", (0.2,) * 3, (0.9,) * 3, None))),
                     shp(SPHERE, ("translation", 4., 0., 1.), m=mat(color=(0.9, 0.8, 0.1), ambient=0.5))])
    cs.append(Case("refraction_sin2t_exactly_one", "tir", shapes, O.light((1., 8., -9.)), rays, tir_edge))

    # Patterns material.rs:97-241 at integer coordinates. A cube face z = -1 of scaling(8, 8, 1), pattern scaling(1/8, 1/8, 1):
    # pattern x, y == world x, y. Ring: sqrt(3*3 + 4*4) == 5 exactly -> floor 5, odd -> colour b.
    def ring(h, _):
        c = d_pattern(shapes_ring, L(), rays_ring[0])
        assert c == (0.0, 0.0, 1.0), "radius 5: floor 5 % 2 != 0 -> b (material.rs:163-170)"
    pat = lambda k: mat(pattern=(k, (1., 0., 0.), (0., 0., 1.), O.chain(("scaling", 0.125, 0.125, 1.))))
    shapes_ring = number([shp(CUBE, ("scaling", 8., 8., 1.), m=pat("ring"))])
    rays_ring = [(3., 4., -5., 0., 0., 1.), (ulps(3., -1), 4., -5., 0., 0., 1.), (-3., -4., -5., 0., 0., 1.), (0., 5., -5., 0., 0., 1.)]
    cs.append(Case("pattern_ring_radius_5", "pattern", shapes_ring, L(), rays_ring, ring))
    for k in ("stripe", "checker", "grid", "gradient"):
        rays = [(x, y, -5., 0., 0., 1.) for x in (2., ulps(2., -1), -1., ulps(-1., -1), ulps(-1., 1), 0., ulps(0.01, 0), 1.01)
                for y in (0.5, 3.)]
        cs.append(Case(f"pattern_{k}_integer_coordinates", "pattern", number([shp(CUBE, ("scaling", 8., 8., 1.), m=pat(k))]), L(), rays))

    # Stale transpose (rtc.h rtc_shape; shape.rs:319-322, 446-449): spheres and planes use inv_t as given, a cube ignores it
    # (shape.rs:627 transposes its inverse on the fly).
    stale = O.chain(("shearing", 0.5, 0., 0.25, 0., 0., 0.75), ("scaling", 1., 2., 1.))
    shapes = number([shp(SPHERE, ("scaling", 1., 0.5, 1.), ("translation", -2.5, 1., 0.)), shp(PLANE, ("rotation_z", 0.3)),
                     shp(CUBE, ("translation", 2.5, 1., 0.))])
    for s in shapes:
        for i in range(16):
            s.inv_t[i] = stale[i] if s.kind != CUBE else (i * 7.5 - 40.)   # a cube's inv_t: garbage
    def stale_t(h, rgbs, shapes=shapes):
        for x, kind in ((h[0], SPHERE), (h[1], PLANE), (h[2], CUBE)):
            s = shapes[x.hit_index]
            assert s.kind == kind
            lp, wn = O.Vec3(), O.Vec3()
            O.lib().orc_transform_point(s.inv, O.Vec3(*x.point), lp)
            ln = {SPHERE: tuple(lp), PLANE: (0., 1., 0.)}.get(kind)
            if ln is None:
                assert abs(abs(x.normal[0]) - 1.) < 1e-12 or abs(abs(x.normal[1]) - 1.) < 1e-12 or abs(abs(x.normal[2]) - 1.) < 1e-12, \
                    "cube normal ignores inv_t"
                continue
            O.lib().orc_transform_vector(s.inv_t, O.Vec3(*ln), wn)
            want = _normalize(tuple(wn))
            if x.inside:
                want = tuple(-v for v in want)
            assert tuple(x.normal) == want, "normal = inv_t * local normal (shape.rs:38)"
    rays = [(-2.5, 1.25, -5., 0., 0., 1.), (0., 4., -3., 0.25, -1., 0.5), (2.5, 1.25, -5., 0., 0., 1.), (-2.2, 1.1, -4., 0.1, 0., 1.)]
    cs.append(Case("stale_transpose", "stale_inv_t", shapes, L((-3., 6., -7.)), rays, stale_t))
    return cs


def _exact_index(c):
    """The double n nearest sqrt(1 / (1 - c*c)) with (n * n) * (1.0 - c * c) == 1.0 exactly."""
    s = 1.0 - c * c
    n0 = math.sqrt(1.0 / s)
    for k in range(4096):
        for n in (ulps(n0, k), ulps(n0, -k)):
            if (n * n) * s == 1.0:
                return n
    raise ValueError("no exact index")


# ------------------------------------------------------------------ bisected families
def bisected_cases():
    L = O.light
    fams = []
    # sphere disc at 0: the ray's offset from the silhouette (shape.rs:366)
    sph = number([shp(SPHERE, ("scaling", 1.5, 1.5, 1.5), ("translation", 0.25, 0.5, 3.), m=mat(color=(0.9, 0.5, 0.1)))])
    fams.append(family("sphere_silhouette_offset", "hit", 0.25, 2.5, lambda x: (sph, L(), (x, 0.5, -5., 0., 0., 1.))))
    fams.append(family("sphere_silhouette_angle", "hit", 0.0, 0.5, lambda x: (sph, L(), (0., 0., -5., x, 0.0625, 1.))))
    # plane |d.y| < EPSILON at an arbitrary transform
    pl = number([shp(PLANE, ("rotation_x", 0.25), ("translation", 0., -1., 0.))])
    fams.append(family("plane_epsilon_tilted", "hit", -0.2477, -0.3, lambda x: (pl, L(), (0., 0., 0., 0., x, 1.))))
    # cube: the strict tmin < tmax at an edge, bisecting the ray's x
    cb = number([shp(CUBE, ("rotation_y", 0.5), ("translation", 0., 0., 2.), m=mat(color=(0.3, 0.9, 0.3)))])
    fams.append(family("cube_edge_offset", "hit", 0.5, 2.0, lambda x: (cb, L(), (x, 0.25, -5., 0., 0., 1.))))
    # hit order between two objects: a sphere slid along z through a plane's hit point (equal t at the flip)
    def two(x):
        return (number([shp(PLANE, ("translation", 0., -1., 0.)), shp(SPHERE, ("translation", 0., 0., x), m=mat(color=(1., 0., 0.)))]),
                L(), (0., 5., 0.5, 0., -1., 0.))
    fams.append(family("sphere_through_plane_hit", "hit", 0.0, 2.0, lambda x: two(x)))
    # shadow: the strict t < distance (ceiling plane through the light), light y bisected
    ceil = number([shp(PLANE), shp(PLANE, ("translation", 0., 3., 0.), m=mat(color=(0.5, 0.5, 0.5)))])
    fams.append(family("shadow_light_height_at_ceiling", "shadowed", 2.5, 3.5,
                       lambda x: (ceil, L((0.25, x, -4.)), (0.25, 1., -5., 0., -1., 1.))))
    # shadow: a sphere occluder's silhouette, light slid sideways until the shadow ray's disc flips
    occ = number([shp(PLANE, m=mat(pattern=("checker", (0.3,) * 3, (0.7,) * 3, None))),
                  shp(SPHERE, ("scaling", 0.5, 0.5, 0.5), ("translation", 0., 2., -4.), m=mat(color=(0.8, 0.1, 0.1)))])
    fams.append(family("shadow_sphere_silhouette", "shadowed", 0.0, 3.0, lambda x: (occ, L((x, 5., -4.)), (0., 1., -5., 0., -1., 1.))))
    # shadow: a cube occluder's edge
    occ_c = number([shp(PLANE), shp(CUBE, ("scaling", 0.5, 0.25, 0.5), ("rotation_y", 0.3), ("translation", 0.5, 2., -3.5))])
    fams.append(family("shadow_cube_edge", "shadowed", 1.0, 1.5, lambda x: (occ_c, L((x, 6., -4.)), (0., 1., -5., 0., -1., 1.))))
    # shading: light_dot_normal < 0 (material.rs:339). A floor point's over_point is at y = 1e-8; with the light at that
    # height far to the side, lightv.y changes sign and the shadow ray is too flat to meet the floor (|d.y| < EPSILON)
    flo = number([shp(PLANE, m=mat(color=(0.2, 0.7, 0.9), specular=0.6, shininess=40.))])
    fams.append(family("ldn_sign_floor", "ldn", 1.0, -1.0, lambda x: (flo, L((12., x, 9.)), (0.25, 1., -5., 0., -1., 1.))))
    # shading: reflect_dot_eye <= 0 (material.rs:347): eyev (0,1,-1) against the light's mirror direction, light z bisected
    fams.append(family("rde_sign_floor", "rde", -20., 0., lambda x: (flo, L((0.25, 5., x)), (0.25, 1., -5., 0., -1., 1.))))
    # refraction: total internal reflection, refractive index bisected (ray inside a glass sphere)
    def glass(ior):
        return (number([shp(SPHERE, m=mat(color=(0.1, 0.1, 0.1), transparency=0.8, reflective=0.4, refractive_index=ior)),
                        shp(PLANE, ("translation", 0., -2., 0.), m=mat(pattern=("stripe", (0.9, 0.9, 0.9), (0.1, 0.4, 0.1), None)))]),
                L((2., 4., -6.)), (0., 0.7, 0., 1.0, 0.0625, 0.125))
    fams.append(family("tir_refractive_index", "tir", 1.0, 3.0, glass))
    # refraction: TIR by ray angle inside a glass cube
    gc = number([shp(CUBE, m=mat(color=(0.1, 0.2, 0.1), transparency=0.9, reflective=0.1, refractive_index=1.5)),
                 shp(PLANE, ("translation", 0., -2., 0.), m=mat(color=(0.9, 0.9, 0.6)))])
    fams.append(family("tir_ray_angle_cube", "tir", 0.1, 0.95, lambda x: (gc, L((1., 5., -5.)), (0., 0., 0.) + _normalize((x, 0.25, 1.)))))
    # inside: dot(normal, eyev) < 0 near 0 (shape.rs:79), a grazing ray at a sphere's rim
    fams.append(_inside_family())
    # patterns: stripe / checker / ring / grid thresholds by the ray's x, on the z = -1 face of a scaled cube (pattern space
    # rotated and scaled); the bisection starts from the first change found on a coarse scan
    pat = lambda k: mat(pattern=(k, (1., 0., 0.), (0., 0., 1.), O.chain(("rotation_z", 0.2), ("scaling", 0.3, 0.3, 0.3))))
    for k in ("stripe", "checker", "ring", "grid"):
        w = number([shp(CUBE, ("scaling", 8., 8., 1.), m=pat(k))])
        build = lambda x, w=w: (w, L(), (x, 0.125, -5., 0., 0., 1.))
        xs = [0.05 + (0.005 if k == "grid" else 0.05) * i for i in range(1500 if k == "grid" else 150)]
        hi = next(x for x in xs if d_pattern(*build(x)) != d_pattern(*build(xs[0])))
        fams.append(family(f"pattern_{k}_threshold", "pattern", xs[0], hi, build))
    cases, pairs = [], []
    for c, p in fams:
        cases += c
        pairs.append(p)
    return cases, pairs


def _inside_family():
    """A ray starting on a glass sphere's surface at (0, 0, -1), direction (1, 0, x): for x > 0 the hit is the entry root
    t1 = 0 seen from outside, for x < 0 the exit root t2 = 0 seen from inside (normal . eyev == x); bisect x through 0."""
    w = number([shp(SPHERE, m=mat(color=(0.6, 0.6, 0.2), transparency=0.5, refractive_index=1.3))])
    return family("inside_on_surface", "inside", -0.5, 0.5, lambda x: (w, O.light(), (0., 0., -1., 1., 0., x)))


# ------------------------------------------------------------------ render-level cases (binning proofs)
def _cam(W, H, fov, frm, to):
    return O.camera(W, H, fov, O.view_transform(frm, to, (0., 1., 0.)))


def pixel_ray(cam, x, y, xo=0.5, yo=0.5):
    r = O.Ray6()
    O.lib().orc_camera_ray_for_pixel(C.byref(cam), x, xo, y, yo, r)
    return tuple(r)


def tile_row_bound(cam, ty, W):
    """A plain restatement (f64) of cone_misses_plane's lower bound for the floor y = 0 over tile row ty: the smallest
    d.y of any pixel-area corner of the row, less the cone's margin (cone_misses_plane and its use in k_bin_tiles, rtc_kernels.hip)."""
    worst = math.inf
    for tx in range((W + 7) // 8):
        ax = pixel_ray(cam, tx * 8 + 3, ty * 8 + 3)[3:]
        q2 = 0.
        for cx, cy, xo, yo in ((tx * 8, ty * 8, 0., 0.), (tx * 8 + 7, ty * 8, 1., 0.), (tx * 8, ty * 8 + 7, 0., 1.), (tx * 8 + 7, ty * 8 + 7, 1., 1.)):
            f = pixel_ray(cam, min(cx, W - 1), cy, xo, yo)[3:]
            u = (ax[1] * f[2] - ax[2] * f[1], ax[2] * f[0] - ax[0] * f[2], ax[0] * f[1] - ax[1] * f[0])
            q2 = max(q2, _dot(u, u))
        sin_t = math.sqrt(q2) * 1.001 + 4e-6
        cos_t = math.sqrt(max(0., 1. - sin_t * sin_t))
        perp = math.sqrt(max(0., 1. - ax[1] * ax[1]) * 1.00001 + 1e-10)
        worst = min(worst, ax[1] * cos_t * 0.99999 - perp * sin_t)
    return worst


def render_cases():
    W, H = 64, 48
    floor = lambda: number([shp(PLANE, m=mat(pattern=("checker", (0.2, 0.3, 0.4), (0.9, 0.8, 0.7), None), specular=0.3))])
    out = []
    cam_at = lambda s: _cam(W, H, math.pi / 3, (0., 1., 0.), (0., 1. + s, 1.))
    # the horizon (floor hit / miss of a row's centre ray, shape.rs:463) in the last row of tile row 3 and the first of tile row 4
    for nm, row in (("horizon_last_row_of_tile", 31), ("horizon_first_row_of_tile", 32)):
        f = lambda s, row=row: d_hit(floor(), O.light(), pixel_ray(cam_at(s), W // 2, row))
        a, b = bisect(f, -0.5, 0.5)
        for k, s in (("lo", a), ("hi", b), ("lo-1", ulps(a, -1)), ("hi+1", ulps(b, 1))):
            out.append(RenderCase(f"{nm}[{k}]", "binning_horizon", floor(), O.light((-5., 8., -6.)), cam_at(s)))
    # the horizon just above a tile edge: the tile row above has its lowest corner direction within cone_misses_plane's 1e-4
    # margin (a plain restatement of the bound, tile_row_bound), so the proof has to decline it
    def near(s):
        return tile_row_bound(cam_at(s), 3, W) > 5e-5
    a, b = bisect(near, 0.3, -0.3)
    for k, s in (("lo", a), ("hi", b)):
        out.append(RenderCase(f"horizon_within_cone_margin[{k}]", "binning_margin", floor(), O.light((-5., 8., -6.)), cam_at(s)))
    # a sphere's silhouette tangent to the corner pixel (15, 15) of tile (1, 1): sphere x bisected until that pixel's disc flips
    cam = _cam(W, H, math.pi / 3, (0., 0., -5.), (0., 0., 0.))
    ball = lambda x: number([shp(SPHERE, ("scaling", 0.5, 0.5, 0.5), ("translation", x, 0.5, 0.), m=mat(color=(0.9, 0.3, 0.2)))])
    ray = pixel_ray(cam, 15, 15)
    a, b = bisect(lambda x: d_hit(ball(x), O.light(), ray), -2.5, -1.2)
    for k, x in (("lo", a), ("hi", b), ("lo-2", ulps(a, -2)), ("hi+2", ulps(b, 2))):
        out.append(RenderCase(f"silhouette_at_tile_corner[{k}]", "binning_silhouette", ball(x), O.light(), cam))
    # the same with a floor: candidate lists and the plane proof together
    for k, x in (("lo", a), ("hi", b)):
        out.append(RenderCase(f"silhouette_at_tile_corner_with_floor[{k}]", "binning_silhouette",
                              ball(x) + number([shp(PLANE, ("translation", 0., -1.5, 0.))], [2]), O.light(), cam))
    return out


# ------------------------------------------------------------------ padding
def padded(shapes):
    """The world plus PAD_SPHERES small spheres far below and behind everything (never hit, never shadowing): the
    default path becomes the two-level Morton-ordered cull, where tie order is decided by the index comparison."""
    out = list(shapes)
    base = max([s.world_id for s in shapes] + [0])
    for i in range(PAD_SPHERES):
        s = shp(SPHERE, ("scaling", 0.01, 0.01, 0.01), ("translation", 400. + 0.5 * (i % 20), -300. - 0.5 * (i // 20), -600.))
        s.world_id = base + 1 + i
        out.append(s)
    return out


def all_probe_cases():
    cases = exact_cases()
    bc, pairs = bisected_cases()
    return cases + bc, pairs
