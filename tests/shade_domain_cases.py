"""Shade-stage cases at the edges of the material and light domain (helper module, not collected; used by
test_host_shade_domain.py and test_gpu_shade_domain.py).

One small scene -- a floor, a ball, a cube, one light, a 9x17 camera -- and cases that each change ONE number the shade
stage consumes to a value no other family sends: NaN, +-inf, signed zeros, subnormals, negatives, 1e+-300. Each case names
the reference line whose comparison it targets. Nothing validates these numbers on the way in (a Lua scene can write 0/0),
so they are in the domain, and the reference's own comparisons (`<= 0.`, `== 0.0`, `> 1.0`, `< 0.`) decide what a NaN does.

Every base material has specular == 0, so a case's colour depends on a rounded `pow` result only where the case itself
asks for it: everything else must match the oracle bit for bit, through the flat, the reflective and
the refractive kernels.
"""
from __future__ import annotations

import importlib.util
import math
import sys
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

import oracle as O


def _sibling(name):
    key = "_shade_dom_" + name
    if key in sys.modules:
        return sys.modules[key]
    spec = importlib.util.spec_from_file_location(key, Path(__file__).with_name(name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[key] = m
    spec.loader.exec_module(m)
    return m


B = _sibling("boundary_cases")
SPHERE, PLANE, CUBE = B.SPHERE, B.PLANE, B.CUBE

NAN, INF = math.nan, math.inf
TINY = 5e-324
W, H = 9, 17                                   # 153 pixels; the centre pixel (4, 8) looks at the ball
CENTRE = (4, 8)
RDE_PIXEL = (4, 7)                             # the pixel whose reflect_dot_eye the rde cases put on either side of 1.0
LIGHT_POS = (-5., 6., -6.)
WHITE = (1., 1., 1.)
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "pixels")

# pow's error in ulp of the result, against the correctly rounded value (tests/test_gpu_parity.py, the mpmath test):
POW_ULP = 4.0                                  # asserted for exponents in [2^-10, 2^12]: the project's stated bound
POW_ULP_WIDE = 2.0                             # asserted for every other finite exponent: twice the largest error measured (1.0)
AFTER_POW = 60.0                               # roundings after the pow: at most 6 per recursion level x 6 levels, + the average
SPECIAL_SHININESS = lambda sh: sh == 0. or math.isinf(sh) or math.isnan(sh)   # pow's result is fixed by C99 Annex F


def pow_ulp_for(sh: float) -> float:
    return POW_ULP if 2.0 ** -10 <= sh <= 2.0 ** 12 else POW_ULP_WIDE


def camera(w=W, h=H):
    return O.camera(w, h, 1.0, O.view_transform((0., 1.5, -5.), (0., 1., 0.), (0., 1., 0.)))


BASE = {"floor": dict(color=(0.8, 0.8, 0.7), specular=0.),
        "ball": dict(color=(0.9, 0.2, 0.1), specular=0.),
        "cube": dict(color=(0.1, 0.3, 0.9), specular=0.)}
_GEOMETRY = {"floor": (PLANE, ()),
             "ball": (SPHERE, (("translation", 0., 1., 0.),)),
             "cube": (CUBE, (("scaling", 0.5, 0.5, 0.5), ("translation", 2., 0.5, -1.)))}
_COEFFS = ("ambient", "diffuse", "specular")


@dataclass
class ShadeCase:
    name: str
    group: str
    line: str                                   # the reference line(s) the case targets
    mats: dict = field(default_factory=dict)    # {"floor" | "ball" | "cube": {material field: value}} over BASE
    lights: list = field(default_factory=lambda: [(LIGHT_POS, WHITE)])   # (position, intensity) in light order
    nonfinite: bool = False                     # the oracle's frame must hold a NaN or an inf
    position: str = ""                          # light-position cases: "nan" | "finite" = what the whole frame must be

    def materials(self):
        out = {}
        for k, base in BASE.items():
            kw = dict(base)
            kw.update(self.mats.get(k, {}))
            out[k] = kw
        return out

    def shapes(self, padded=False):
        ms = self.materials()
        shapes = B.number([B.shp(_GEOMETRY[k][0], *_GEOMETRY[k][1], m=O.material(**ms[k])) for k in ("floor", "ball", "cube")])
        return B.padded(shapes) if padded else shapes

    def light_list(self):
        return [O.light(p, i) for p, i in self.lights]

    # ---- what the reference's comparisons imply for the launch
    def reflects(self):
        return any(not (m.get("reflective", 0.) <= 0.) for m in self.materials().values())   # shape.rs:730

    def refracts(self):
        return any(m.get("transparency", 0.) != 0.0 for m in self.materials().values())      # shape.rs:752

    # ---- the comparison class
    def exact(self):
        return all(m.get("specular", 0.9) == 0. or SPECIAL_SHININESS(m.get("shininess", 200.)) for m in self.materials().values())

    def pow_ulp(self):
        return max(pow_ulp_for(m.get("shininess", 200.)) for m in self.materials().values()
                   if not (m.get("specular", 0.9) == 0. or SPECIAL_SHININESS(m.get("shininess", 200.))))

    def negative_terms(self):
        ms = self.materials().values()
        return any(m.get(k, 0.) < 0. for m in ms for k in _COEFFS) or any(c < 0. for _, i in self.lights for c in i)

    def absolute(self):
        """The same case with |intensity| and |coefficients|: its frame is the sum of the |terms| of this one."""
        mats = {k: {f: (abs(v) if f in _COEFFS else v) for f, v in m.items()} for k, m in self.mats.items()}
        return ShadeCase(self.name + "|abs|", self.group, self.line, mats, [(p, tuple(abs(c) for c in i)) for p, i in self.lights])


def _f(x):
    return repr(float(x)).replace("-", "m") if not isinstance(x, tuple) else "_".join(_f(v) for v in x)


# ------------------------------------------------------------------ oracle renders
def arr(shapes):
    return (O.RtcShape * len(shapes))(*shapes)


def oracle_frame(case, cam=None, padded=False, streaming=False):
    """The oracle's frame and counters: for several lights the SUM of the single-light frames in light order (color_at is
    linear in the light, and in a flat world that sum is the kernel's order of additions), every light's shadow rays."""
    cam = cam or camera()
    shapes = case.shapes(padded)
    a = arr(shapes)
    frame, stats = None, None
    for lgt in case.light_list():
        f, st = O.render(a, len(shapes), lgt, cam, mode=1, nthreads=4, streaming=streaming, want_stats=True)
        if frame is None:
            frame, stats = f, dict(st)
        else:
            frame = frame + f
            stats["rays_shadow"] += st["rays_shadow"]
    return frame, stats


def pixel_rays(cam):
    return [B.pixel_ray(cam, x, y) for y in range(cam.vsize) for x in range(cam.hsize)]


def oracle_probes(case, cam=None, padded=False):
    """color_at of every pixel-centre ray: (rgb (n, 3) summed over the lights in order, the first light's hit records)."""
    cam = cam or camera()
    shapes = case.shapes(padded)
    a = arr(shapes)
    rgb, hits = None, None
    for lgt in case.light_list():
        out = [O.color_at(a, len(shapes), lgt, r, 5, want_hit=True) for r in pixel_rays(cam)]
        c = np.array([o[0] for o in out])
        if rgb is None:
            rgb, hits = c, [o[1] for o in out]
        else:
            rgb = rgb + c
    return rgb, hits


# ------------------------------------------------------------------ comparison
def canon(a):
    """The bit patterns of an f64 array with every NaN made the same NaN: equal iff the values are identical, signed zeros
    and infinities included, NaN payloads and signs aside (0 * inf is -NaN on x86 and +NaN on the GPU)."""
    c = np.array(a, dtype=np.float64, copy=True)
    c[np.isnan(c)] = np.nan
    return c.view(np.uint64)


def _bits(x):
    return "nan" if x != x else float(x).hex()


def hit_key(h):
    """Every field of an rtc_hit, floats by bit pattern (NaN: one value)."""
    vec = lambda v: tuple(_bits(x) for x in v)
    return (h.hit_index, h.inside, h.shadowed, _bits(h.t), vec(h.point), vec(h.over_point), vec(h.under_point), vec(h.eyev),
            vec(h.normal), vec(h.reflectv), _bits(h.n1), _bits(h.n2))


def compare(case, got, want, abs_want=None):
    """The comparison rule, per channel -> (list of complaints, largest |got - want| / |want| over the finite channels).
    Non-finite: NaN where the oracle has NaN, +-inf with the oracle's sign. Finite: bit-identical for an exact-class case;
    otherwise within (K + 60) * 2^-52 of the oracle's value -- of the |terms| frame `abs_want` when terms can cancel."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = []
    if got.shape != want.shape:
        return [f"shape {got.shape} != {want.shape}"], math.nan
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        bad.append(f"NaN in {int(np.isnan(got).sum())} channels, the oracle has {int(np.isnan(want).sum())}")
    inf = np.isinf(want) | np.isinf(got)
    if not np.array_equal(got[inf], want[inf], equal_nan=True):
        bad.append(f"infinities differ in {int((got[inf] != want[inf]).sum())} channels")
    fin = np.isfinite(want) & np.isfinite(got)
    g, w = got[fin], want[fin]
    nz = w != 0.
    rel = float(np.max(np.abs(g[nz] - w[nz]) / np.abs(w[nz]))) if nz.any() else 0.
    if case.exact():
        n = int((canon(g) != canon(w)).sum())
        if n:
            bad.append(f"exact class: {n} finite channels differ in their bits, largest relative difference {rel:.3e}")
    else:
        scale = np.abs(w)
        if case.negative_terms():
            assert abs_want is not None, "a case with negative terms is compared against its |terms| frame"
            scale = np.abs(np.asarray(abs_want, dtype=np.float64)[fin])
        bound = (case.pow_ulp() + AFTER_POW) * 2.0 ** -52 * scale
        over = np.abs(g - w) > bound
        if over.any():
            k = int(np.argmax(np.abs(g - w) - bound))
            bad.append(f"pow class: {int(over.sum())} channels beyond (K={case.pow_ulp():g} + 60) ulp, worst {g[k]!r} vs {w[k]!r}")
    return bad, rel


# ------------------------------------------------------------------ the cases
def _ball(**kw):
    return {"ball": kw}


def material_cases():
    cs = []
    add = lambda *a, **k: cs.append(ShadeCase(*a, **k))
    # reflected_color's `reflectiveness <= 0.` (shape.rs:730): false for NaN, so the reference casts the ray; Schlick's
    # `reflective > 0.0 && transparency > 0.0` (shape.rs:692) is false for NaN
    for v, nf in ((NAN, True), (TINY, False), (-0.0, False), (-0.5, False), (2.0, False), (INF, True)):
        add(f"reflective[ball={_f(v)}]", "reflective", "shape.rs:730", _ball(reflective=v), nonfinite=nf)
    add("reflective[floor=nan]", "reflective", "shape.rs:730", {"floor": dict(reflective=NAN)}, nonfinite=True)
    add("reflective[ball=nan,transparency=0.5]", "reflective", "shape.rs:730, 692", _ball(reflective=NAN, transparency=0.5), nonfinite=True)
    # refracted_color's `transparency == 0.0` (shape.rs:752)
    add("transparency[ball=nan]", "transparency", "shape.rs:752", _ball(transparency=NAN), nonfinite=True)
    add("transparency[ball=m0.5,reflective=0.5]", "transparency", "shape.rs:752, 692", _ball(transparency=-0.5, reflective=0.5))
    add(f"transparency[ball={_f(TINY)}]", "transparency", "shape.rs:752", _ball(transparency=TINY))
    add("transparency[ball=m0.0]", "transparency", "shape.rs:752", _ball(transparency=-0.0))
    add("transparency[ball=inf]", "transparency", "shape.rs:752", _ball(transparency=INF), nonfinite=True)
    # n_ratio and `sin2_t > 1.0` (shape.rs:756-759)
    # (a NaN index makes a NaN ray, which meets nothing: the refracted colour is BLACK * 0.5 and the frame stays finite)
    for v in (0.0, NAN, 1e-300, 1e300, -1.5):
        add(f"refractive_index[ball={_f(v)}]", "refractive_index", "shape.rs:756-759", _ball(transparency=0.5, refractive_index=v))
    # factor = reflect_dot_eye.powf(shininess); specular = intensity * specular * factor (material.rs:355-356)
    for sh in (0.0, -0.0, TINY, 0.5, 1.0, 1e3, 1e6, 1e300, INF, -3.0, -INF, NAN):
        for sp in (0.0, -0.0, 0.9, -0.5, INF, NAN):
            # 0 * pow is NaN where pow is inf or NaN; inf * pow where pow is 0; NaN * anything
            nf = (math.isnan(sp) or math.isinf(sp) or math.isnan(sh) or sh == -INF)
            add(f"shine[sh={_f(sh)},sp={_f(sp)}]", "shininess_specular", "material.rs:355-356", _ball(shininess=sh, specular=sp), nonfinite=nf)
    # ambient (material.rs:333) and diffuse (material.rs:344)
    for k, line in (("ambient", "material.rs:333"), ("diffuse", "material.rs:344")):
        for v in (-0.0, -1.0, INF, NAN):
            add(f"{k}[ball={_f(v)}]", "ambient_diffuse", line, _ball(**{k: v}), nonfinite=not math.isfinite(v))
    # effective_color = color * intensity (material.rs:330); stripe and checker colours on the floor (material.rs:97-135)
    for what, v in (("negative", -0.25), ("two", 2.0), ("negzero", -0.0), ("inf", INF), ("nan", NAN)):
        nf = not math.isfinite(v)
        add(f"color[ball.g={what}]", "colors", "material.rs:330", _ball(color=(0.9, v, 0.1)), nonfinite=nf)
        add(f"color[floor.stripe.a.r={what}]", "colors", "material.rs:97-110", {"floor": dict(pattern=("stripe", (v, 0.8, 0.7), (0.3, 0.3, 0.4), None))}, nonfinite=nf)
        add(f"color[floor.checker.b.b={what}]", "colors", "material.rs:120-135", {"floor": dict(pattern=("checker", (0.8, 0.8, 0.7), (0.3, 0.3, v), None))}, nonfinite=nf)
    return cs


INTENSITIES = (("negative", (-1., 0.5, 2.)), ("inf", (INF, 1., 0.)), ("nan", (NAN, 1., 1.)), ("huge_tiny", (1e300, 1e300, 1e-300)),
               ("negzero", (-0.0, 0., 0.)))
SECOND_POS = (4., 5., -3.)                     # the second light's place, over the cube's side of the scene
AREA_CORNER, AREA_STEP = (-5.5, 6., -6.5), 0.5  # 3x3 samples around LIGHT_POS, one ninth of white each


def area_samples(special):
    out = []
    for v in range(3):
        for u in range(3):
            out.append(((AREA_CORNER[0] + AREA_STEP * u, AREA_CORNER[1], AREA_CORNER[2] + AREA_STEP * v), (1. / 9.,) * 3))
    out[4] = (out[4][0], special)              # sample 5 of the nine
    return out


def light_cases():
    cs = []
    for what, inten in INTENSITIES:
        nf = not all(math.isfinite(c) for c in inten)
        cs.append(ShadeCase(f"intensity[{what}]", "intensity", "material.rs:330, 356", lights=[(LIGHT_POS, inten)], nonfinite=nf))
        cs.append(ShadeCase(f"intensity[second={what}]", "intensity_second", "material.rs:330, 356", lights=[(LIGHT_POS, WHITE), (SECOND_POS, inten)], nonfinite=nf))
        cs.append(ShadeCase(f"intensity[sample5={what}]", "intensity_table", "material.rs:330, 356", lights=area_samples(inten), nonfinite=nf))
    # lightv = (position - point).normalize() (material.rs:335), v / distance of is_shadowed (shape.rs:717-719)
    cs.append(ShadeCase("position[x=inf]", "position", "material.rs:335, shape.rs:717-719", lights=[((INF, 6., -6.), WHITE)], nonfinite=True, position="nan"))
    cs.append(ShadeCase("position[x=nan]", "position", "material.rs:335, shape.rs:717-719", lights=[((NAN, 6., -6.), WHITE)], nonfinite=True, position="nan"))
    # |v| overflows: distance = inf, direction = v / inf = 0: nothing is in shadow, light_dot_normal = 0, ambient only
    cs.append(ShadeCase("position[1e200]", "position", "material.rs:335, shape.rs:717-719", lights=[((1e200, 1e200, -1e200), WHITE)]))
    # the light exactly on the centre pixel's over_point: v = 0, distance = 0, direction = 0 / 0
    h = centre_hit(ShadeCase("plain", "plain", ""))
    cs.append(ShadeCase("position[over_point]", "position", "material.rs:335, shape.rs:717-719", lights=[(tuple(h.over_point), WHITE)], nonfinite=True))
    return cs


def centre_hit(case, light=None, pixel=CENTRE):
    shapes = case.shapes()
    lgt = light if light is not None else case.light_list()[0]
    return B.probe(shapes, lgt, B.pixel_ray(camera(), *pixel))[1]


def rde_of(x):
    """reflect_dot_eye (material.rs:346) of pixel RDE_PIXEL's hit with the light at (x, y, z of the mirror direction)."""
    lgt = O.light((x, _RDE["y"], _RDE["z"]))
    h = centre_hit(ShadeCase("plain", "plain", ""), lgt, RDE_PIXEL)
    return B._light_terms(h, lgt)[1]


_RDE = {}


def rde_cases():
    """The other leg of lighting()'s shortcut: reflect_dot_eye just above 1. The light is put on the mirror direction of
    a pixel's eye vector, where the rounded dot product of two unit vectors lands on either side of 1.0; its x is
    bisected over the f64 bit patterns between a place well off the mirror direction and one found with rde > 1.
    The pixel is (4, 7), the one above the centre: the centre pixel's own eye vector and normal are both rounded a little
    short of unit length (|eyev| * |normal| = 1 - 3 * 2^-53), and no light position lifts its rde above 1 - 2^-52."""
    if "cases" in _RDE:
        return _RDE["cases"], _RDE["pair"]
    plain = ShadeCase("plain", "plain", "")
    h = centre_hit(plain, pixel=RDE_PIXEL)
    r = B._reflect(tuple(-v for v in h.eyev), tuple(h.normal))     # where the eye's mirror image looks
    above = None
    for dist in (7.0, 5.5, 3.0):
        at = tuple(h.over_point[i] + dist * r[i] for i in range(3))
        _RDE["y"], _RDE["z"] = at[1], at[2]
        above = next((x for x in (B.ulps(at[0], k) for k in range(-40, 40)) if rde_of(x) > 1.0), None)
        if above is not None:
            break
    if above is None:
        raise ValueError("no light x near the mirror direction gives reflect_dot_eye > 1")
    a, b = B.bisect(lambda x: rde_of(x) > 1.0, at[0] - 0.5, above)
    cs = []
    for tag, x in (("lo-2", B.ulps(a, -2)), ("lo", a), ("hi", b), ("hi+2", B.ulps(b, 2))):
        for sp, sh in ((0.0, 200.0), (0.9, 200.0), (0.0, 1e300)):
            # specular 0 with shininess 1e300: pow(1 + ulp, 1e300) = inf and 0 * inf = NaN -- where rde <= 1 it is 0 * 0
            cs.append(ShadeCase(f"rde[{tag},sp={_f(sp)},sh={_f(sh)}]", "rde", "material.rs:347, 355", _ball(specular=sp, shininess=sh),
                                lights=[((x, at[1], at[2]), WHITE)], nonfinite=(rde_of(x) > 1.0 and sh == 1e300)))
    _RDE["cases"], _RDE["pair"] = cs, (a, b)
    return cs, (a, b)


_ALL = []


def all_cases():
    if not _ALL:
        _ALL.extend(material_cases() + light_cases() + rde_cases()[0])
        names = [c.name for c in _ALL]
        assert len(set(names)) == len(names)
    return _ALL


PLAIN = ShadeCase("plain", "plain", "")
GROUPS = ("reflective", "transparency", "refractive_index", "shininess_specular", "ambient_diffuse", "colors", "intensity",
          "intensity_second", "intensity_table", "position", "rde")
# two cases per group for the lens and the update routes
REPRESENTATIVES = ("reflective[ball=nan]", "reflective[ball=nan,transparency=0.5]", "transparency[ball=nan]", "transparency[ball=m0.5,reflective=0.5]",
                   "refractive_index[ball=nan]", "refractive_index[ball=0.0]", "shine[sh=nan,sp=0.0]", "shine[sh=1000000.0,sp=0.9]",
                   "ambient[ball=nan]", "diffuse[ball=m1.0]", "color[ball.g=nan]", "color[floor.checker.b.b=negative]",
                   "intensity[nan]", "intensity[negative]", "intensity[second=inf]", "intensity[second=negzero]",
                   "intensity[sample5=nan]", "intensity[sample5=huge_tiny]", "position[x=nan]", "position[over_point]",
                   "rde[hi,sp=0.0,sh=1e+300]", "rde[hi,sp=0.9,sh=200.0]")
WIDE_FRAME = ("reflective[ball=nan]", "reflective[ball=nan,transparency=0.5]", "shine[sh=minf,sp=0.0]")   # also at 20x12


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
