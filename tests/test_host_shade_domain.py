"""Shade-domain cases on the CPU (tests/shade_domain_cases.py), oracle only: every case is of the class it stands for, so
that the GPU file cannot pass vacuously -- enough finite colour to compare, a NaN or an inf where one is promised, the
secondary rays the reference's own comparisons cast, an rde pair that straddles 1.0 -- and the oracle's streaming form
(the kernel's algorithm) equals its literal sorted-list form on every case, NaN for NaN."""
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest


def _sibling(name):
    spec = importlib.util.spec_from_file_location("_shd_" + name, Path(__file__).with_name(name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m          # (dataclasses look their module up)
    spec.loader.exec_module(m)
    return m


S = _sibling("shade_domain_cases")
CASES = S.all_cases()
BY_GROUP = {g: [c for c in CASES if c.group == g] for g in S.GROUPS}


@pytest.fixture(scope="module")
def frames(O):
    """The oracle's (frame, counters) of every case and of the plain scene: computed once, never written to."""
    out = {}
    for c in CASES + [S.PLAIN]:
        f, st = S.oracle_frame(c)
        f.setflags(write=False)
        out[c.name] = (f, st)
    return out


def test_the_families_are_complete():
    assert set(BY_GROUP) == {c.group for c in CASES} and all(BY_GROUP.values())
    assert len(BY_GROUP["shininess_specular"]) == 12 * 6 and len(BY_GROUP["reflective"]) == 8 and len(BY_GROUP["transparency"]) == 5
    assert len(BY_GROUP["refractive_index"]) == 5 and len(BY_GROUP["ambient_diffuse"]) == 8 and len(BY_GROUP["colors"]) == 15
    assert len(BY_GROUP["intensity"]) == len(BY_GROUP["intensity_second"]) == len(BY_GROUP["intensity_table"]) == 5
    assert len(BY_GROUP["position"]) == 4 and len(BY_GROUP["rde"]) == 12
    assert all(c.line for c in CASES)
    assert all(len(c.lights) == {"intensity_second": 2, "intensity_table": 9}.get(c.group, 1) for c in CASES)
    reps = [S.by_name(n) for n in S.REPRESENTATIVES]
    assert all(sum(r.group == g for r in reps) == 2 for g in S.GROUPS)
    assert all(S.by_name(n) for n in S.WIDE_FRAME)


def test_the_plain_scene_is_the_one_the_cases_were_counted_on(frames):
    f, st = frames["plain"]
    assert int(f.reshape(-1, 3).any(axis=1).sum()) == 96
    assert st == {"rays_primary": 153, "rays_shadow": 96, "rays_reflect": 0, "rays_refract": 0, "pixels": 153}
    assert np.isfinite(f).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_is_of_its_class(frames, case):
    f, st = frames[case.name]
    finite_nonzero = int((np.isfinite(f) & (f != 0.)).sum())
    nonfinite = int((~np.isfinite(f)).sum())
    hit = frames["plain"][0].reshape(-1, 3).any(axis=1)          # the 96 pixels that see something
    px = f.reshape(-1, 3)
    if case.position:
        # a light at +-inf or NaN: v, distance and direction are all inf / NaN, and so is every hit pixel's colour
        assert case.position == "nan" and np.isnan(px[hit]).all() and finite_nonzero == 0, (case.name, nonfinite, finite_nonzero)
        assert not px[~hit].any()
    elif case.name == "intensity[negzero]":
        # the one case whose frame has no colour at all: with intensity (-0, 0, 0) lighting() returns red -0.0, and shade_hit's
        # `surface + reflected + refracted` (shape.rs:699) adds BLACK twice: -0 + 0 = +0. What the GPU has to reproduce is
        # that sign, in the flat kernel too, where nothing is reflected or refracted.
        assert finite_nonzero == 0 and nonfinite == 0 and not np.signbit(f).any()
        rgb, hits = S.oracle_probes(case)
        assert sum(h.hit_index >= 0 and not h.shadowed for h in hits) >= 60 and not np.signbit(rgb).any()
    else:
        assert finite_nonzero >= 60, (case.name, finite_nonzero)
    assert (nonfinite > 0) == case.nonfinite, (case.name, nonfinite)
    assert st["rays_primary"] == 153 and st["pixels"] == 153
    assert st["rays_shadow"] >= 96 * len(case.lights)


def test_secondary_rays_follow_the_references_comparisons(frames):
    """rays_reflect / rays_refract differ from the plain scene's (0, 0) exactly where `reflectiveness <= 0.` (shape.rs:730)
    and `transparency == 0.0` (shape.rs:752) are false, by the counts a 29-pixel ball gives."""
    for c in CASES:
        _, st = frames[c.name]
        if c.group in ("reflective", "transparency"):
            assert (st["rays_reflect"] != 0) == c.reflects(), c.name
            assert (st["rays_refract"] != 0) == c.refracts(), c.name
        elif c.group != "refractive_index":
            assert st["rays_reflect"] == 0 == st["rays_refract"] and not c.reflects() and not c.refracts(), c.name
    count = lambda name: (frames[name][1]["rays_reflect"], frames[name][1]["rays_refract"])
    assert count("reflective[ball=nan]") == (29, 0) == count("reflective[ball=5em324]") == count("reflective[ball=inf]") == count("reflective[ball=2.0]")
    assert count("reflective[ball=m0.0]") == (0, 0) == count("reflective[ball=m0.5]")
    assert frames["reflective[ball=nan]"][1]["rays_shadow"] == 109
    assert int(np.isnan(frames["reflective[ball=nan]"][0]).sum()) == 87
    assert count("reflective[floor=nan]")[0] > 29
    assert count("transparency[ball=nan]") == (0, 58) == count("transparency[ball=5em324]") == count("transparency[ball=inf]")
    assert count("transparency[ball=m0.0]") == (0, 0)
    # both rays are cast where Schlick's `> 0.0 && > 0.0` is false: NaN reflective, negative transparency
    for name in ("reflective[ball=nan,transparency=0.5]", "transparency[ball=m0.5,reflective=0.5]"):
        r, t = count(name)
        assert r >= 29 and t >= 58, name
    # n_ratio = 1 / 0 = inf: sin2_t = inf > 1.0, total internal reflection; n_ratio NaN: `sin2_t > 1.0` is false, a NaN ray
    assert count("refractive_index[ball=0.0]") == (0, 0)
    assert count("refractive_index[ball=nan]") == (0, 29)
    assert all(c.refracts() and not c.reflects() for c in BY_GROUP["refractive_index"])


def test_flavours_the_cases_stand_for():
    """Which kernel the reference's comparisons ask for: a NaN-reflective world is a reflective one."""
    want = {"reflective[ball=nan]": (True, False), "reflective[floor=nan]": (True, False), "reflective[ball=5em324]": (True, False),
            "reflective[ball=m0.0]": (False, False), "reflective[ball=m0.5]": (False, False), "reflective[ball=nan,transparency=0.5]": (True, True),
            "transparency[ball=nan]": (False, True), "transparency[ball=m0.0]": (False, False), "transparency[ball=m0.5,reflective=0.5]": (True, True),
            "shine[sh=nan,sp=nan]": (False, False)}
    for name, (refl, refr) in want.items():
        c = S.by_name(name)
        assert (c.reflects(), c.refracts()) == (refl, refr), name


def test_comparison_classes():
    exact = lambda n: S.by_name(n).exact()
    assert all(c.exact() for c in CASES if c.group not in ("shininess_specular", "rde"))
    assert exact("shine[sh=nan,sp=0.9]") and exact("shine[sh=minf,sp=m0.5]") and exact("shine[sh=m0.0,sp=inf]") and exact("shine[sh=1000.0,sp=m0.0]")
    assert not exact("shine[sh=1000.0,sp=0.9]") and S.by_name("shine[sh=1000.0,sp=0.9]").pow_ulp() == S.POW_ULP
    for n in ("shine[sh=1000000.0,sp=0.9]", "shine[sh=m3.0,sp=0.9]", "shine[sh=5em324,sp=0.9]", "shine[sh=1e+300,sp=m0.5]"):
        assert not exact(n) and S.by_name(n).pow_ulp() == S.POW_ULP_WIDE, n
    neg = [c.name for c in CASES if not c.exact() and c.negative_terms()]
    assert sorted(neg) == sorted(f"shine[sh={sh},sp=m0.5]" for sh in ("5em324", "0.5", "1.0", "1000.0", "1000000.0", "1e+300", "m3.0"))
    a = S.by_name("shine[sh=0.5,sp=m0.5]").absolute()
    assert a.materials()["ball"]["specular"] == 0.5 and not a.negative_terms()
    # the pow-class cases that are not marked negative have no negative term: every intensity, colour and coefficient >= 0
    for c in CASES:
        if not c.exact() and not c.negative_terms():
            ms = c.materials().values()
            assert all(not (m.get(k, 0.) < 0.) for m in ms for k in ("ambient", "diffuse", "specular")), c.name
            assert all(not (v < 0.) for m in ms for v in m["color"]) and all(not (v < 0.) for _, i in c.lights for v in i), c.name


def test_the_rde_pair_straddles_one():
    _, (lo, hi) = S.rde_cases()
    assert abs(S.B._key(hi) - S.B._key(lo)) == 1
    assert S.rde_of(lo) <= 1.0 < S.rde_of(hi), (S.rde_of(lo), S.rde_of(hi))
    h = S.centre_hit(S.PLAIN, S.O.light((hi, S._RDE["y"], S._RDE["z"])), S.RDE_PIXEL)
    assert h.hit_index == 1 and not h.shadowed, "the pixel sees the ball, lit"
    # what the pair is for: with specular 0 and shininess 1e300 the reference's colour is 0 * pow(rde, 1e300): 0 * 0 below
    # 1.0 and 0 * inf = NaN above it -- in that pixel only
    x, y = S.RDE_PIXEL
    for tag, want_nan in (("lo", False), ("hi", True)):
        f, _ = S.oracle_frame(S.by_name(f"rde[{tag},sp=0.0,sh=1e+300]"))
        assert np.isnan(f[y, x]).all() == want_nan and int(np.isnan(f).sum()) == (3 if want_nan else 0), tag


def test_the_over_point_light_sits_on_the_centre_pixels_over_point():
    c = S.by_name("position[over_point]")
    h = S.centre_hit(S.PLAIN)
    assert tuple(c.lights[0][0]) == tuple(h.over_point) and h.hit_index == 1
    f, _ = S.oracle_frame(c)
    x, y = S.CENTRE
    assert np.isnan(f[y, x]).all() and int(np.isnan(f).sum()) == 3, "v = 0: distance 0, direction 0 / 0, in that pixel only"


@pytest.mark.parametrize("group", S.GROUPS)
def test_literal_equals_streaming_and_padding_changes_nothing(O, frames, group):
    """orc_render's streaming form == its literal form, frames (NaN in the same places) and counters; the padded world's
    frame and counters are the small world's; color_at of the pixel-centre rays is the frame."""
    for c in BY_GROUP[group]:
        f, st = frames[c.name]
        g, sg = S.oracle_frame(c, streaming=True)
        assert np.array_equal(S.canon(f), S.canon(g)) and st == sg, c.name
        p, sp = S.oracle_frame(c, padded=True)
        assert np.array_equal(S.canon(f), S.canon(p)) and st == sp, c.name
    for name in S.REPRESENTATIVES:
        c = S.by_name(name)
        if c.group == group:
            rgb, hits = S.oracle_probes(c)
            assert np.array_equal(S.canon(rgb.reshape(f.shape)), S.canon(frames[c.name][0])), name
            assert sum(h.hit_index >= 0 for h in hits) == 96


def test_compare_rule():
    """The comparison rule itself: NaN for NaN, inf by sign, bits for the exact class, (K + 60) ulp for the pow class."""
    ex, pw, ng = S.by_name("reflective[ball=nan]"), S.by_name("shine[sh=1000.0,sp=0.9]"), S.by_name("shine[sh=1000.0,sp=m0.5]")
    w = np.array([1.0, 0.0, -0.0, math.nan, math.inf, -math.inf, 3e-5])
    assert S.compare(ex, w.copy(), w) == ([], 0.0)
    assert S.compare(ex, np.array([1.0, 0.0, -0.0, -math.nan, math.inf, -math.inf, 3e-5]), w)[0] == []
    for i, v in ((0, 1.0 + 2.0 ** -52), (1, -0.0), (2, 0.0), (3, 1.0), (4, -math.inf), (4, 1e308), (5, math.nan), (6, math.nan)):
        g = w.copy()
        g[i] = v
        assert S.compare(ex, g, w)[0], (i, v)
    g = w.copy()
    g[0] = 1.0 + 64 * 2.0 ** -52
    assert S.compare(pw, g, w)[0] == [] and S.compare(pw, g, w)[1] == 64 * 2.0 ** -52
    g[0] = 1.0 + 65 * 2.0 ** -52
    assert S.compare(pw, g, w)[0]
    g[1] = 5e-324
    assert S.compare(pw, g, w)[0], "an oracle zero allows nothing"
    g = w.copy()
    g[1] = 1e-17
    assert S.compare(ng, g, w, abs_want=np.abs(w) + 1.0)[0] == [] and S.compare(ng, g, w, abs_want=np.abs(w))[0]
