"""Boundary cases on the CPU (tests/boundary_cases.py): the exact constructions meet the outcome the reference source
gives them, the oracle's streaming form (the kernel's algorithm) equals its literal sorted-list form on every case, and
every bisected pair really straddles its decision."""
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest


def _sibling(name):
    spec = importlib.util.spec_from_file_location("_bnd_" + name, Path(__file__).with_name(name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m          # (dataclasses look their module up)
    spec.loader.exec_module(m)
    return m


B = _sibling("boundary_cases")
CASES, PAIRS = B.all_probe_cases()
RENDER = B.render_cases()


def hit_fields(h):
    return (h.hit_index, h.inside, h.shadowed, h.t, tuple(h.point), tuple(h.over_point), tuple(h.under_point),
            tuple(h.eyev), tuple(h.normal), tuple(h.reflectv), h.n1, h.n2)


def _run(O, shapes, lgt, rays, remaining, streaming=False):
    a = (O.RtcShape * max(1, len(shapes)))()
    for i, s in enumerate(shapes):
        a[i] = s
    out = [O.color_at(a, len(shapes), lgt, tuple(r), remaining, streaming=streaming, want_hit=True) for r in rays]
    return [o[0] for o in out], [o[1] for o in out]


def test_every_decision_is_covered():
    decisions = {c.decision for c in CASES} | {p.decision for p in PAIRS} | {r.decision for r in RENDER}
    for d in ("sphere_disc", "sphere_roots", "plane_eps", "plane_zero_t", "plane_guard", "cube_axis", "cube_normal", "tie",
              "containers", "shadow", "shadowed", "specular", "ldn", "rde", "tir", "inside", "pattern", "stale_inv_t", "hit",
              "binning_horizon", "binning_margin", "binning_silhouette"):
        assert d in decisions, d
    assert all(c.expect is not None for c in CASES if c.kind == "exact" and c.decision not in ("containers", "pattern"))


@pytest.mark.parametrize("case", [c for c in CASES if c.expect is not None], ids=lambda c: c.name)
def test_exact_construction_meets_the_reference(O, case):
    rgbs, hits = _run(O, case.shapes, case.light, case.rays, 5)
    case.expect(hits, rgbs)


@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_streaming_equals_literal_form(O, padded):
    """orc_color_at_streaming (min over entries, open-set n1/n2: the kernel's algorithm) == orc_color_at (the reference's
    sorted list), hit record and colour, at remaining 0 and 5 — on every case, and on the padded worlds."""
    for c in CASES:
        shapes = B.padded(c.shapes) if padded else c.shapes
        for rem in (0, 5):
            lr, lh = _run(O, shapes, c.light, c.rays, rem)
            sr, sh = _run(O, shapes, c.light, c.rays, rem, streaming=True)
            for i in range(len(c.rays)):
                assert hit_fields(lh[i]) == hit_fields(sh[i]), (c.name, i, rem)
                assert np.array_equal(lr[i], sr[i]), (c.name, i, rem)


def test_padding_never_hits_nor_shadows(O):
    """The padded variant adds far spheres only: every hit record and colour is the unpadded world's."""
    for c in CASES:
        r0, h0 = _run(O, c.shapes, c.light, c.rays, 5)
        r1, h1 = _run(O, B.padded(c.shapes), c.light, c.rays, 5)
        for i in range(len(c.rays)):
            assert hit_fields(h0[i]) == hit_fields(h1[i]) and np.array_equal(r0[i], r1[i]), (c.name, i)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: p.name)
def test_bisected_pair_straddles_its_decision(pair):
    lo, hi = pair.pred(pair.lo), pair.pred(pair.hi)
    assert lo != hi, (pair.name, lo, hi)
    # the two parameters are adjacent doubles
    xs = [v for v in _param(pair)]
    assert abs(B._key(xs[1]) - B._key(xs[0])) == 1, (pair.name, xs)


def _param(pair):
    """The one scalar that differs between the pair's two cases (ray, light or a shape's inverse)."""
    a, b = pair.lo, pair.hi
    diff = [(x, y) for x, y in zip(a.rays[0], b.rays[0]) if x != y]
    diff += [(x, y) for x, y in zip(a.light.position, b.light.position) if x != y]
    for sa, sb in zip(a.shapes, b.shapes):
        if sa.material.refractive_index != sb.material.refractive_index:
            diff.append((sa.material.refractive_index, sb.material.refractive_index))
        for i in range(16):
            if sa.inv[i] != sb.inv[i]:
                diff.append((-sa.inv[i], -sb.inv[i]))  # translation column of the inverse: -offset
    assert len(diff) >= 1, pair.name
    return diff[0]


def test_render_cases_sit_on_their_boundaries(O):
    """The horizon pairs flip the floor hit of their pixel row; the margin pair brackets 5e-5 of the restated cone bound
    (inside cone_misses_plane's 1e-4 margin, so the proof must decline that tile row); the silhouette pairs flip the disc of
    the tile-corner pixel (15, 15)."""
    byname = {r.name: r for r in RENDER}
    for nm, row in (("horizon_last_row_of_tile", 31), ("horizon_first_row_of_tile", 32)):
        lo, hi = byname[nm + "[lo]"], byname[nm + "[hi]"]
        f = lambda r: B.d_hit(r.shapes, r.light, B.pixel_ray(r.cam, r.cam.hsize // 2, row))
        assert f(lo) != f(hi), nm
    lo, hi = byname["horizon_within_cone_margin[lo]"], byname["horizon_within_cone_margin[hi]"]
    blo, bhi = B.tile_row_bound(lo.cam, 3, 64), B.tile_row_bound(hi.cam, 3, 64)
    assert 0. < min(blo, bhi) <= 5e-5 < max(blo, bhi) < 1e-4
    for nm in ("silhouette_at_tile_corner", "silhouette_at_tile_corner_with_floor"):
        lo, hi = byname[nm + "[lo]"], byname[nm + "[hi]"]
        f = lambda r: B.d_hit(r.shapes, r.light, B.pixel_ray(r.cam, 15, 15))
        assert f(lo) != f(hi), nm


def test_render_cases_literal_equals_streaming(O):
    for r in RENDER:
        a, sa = O.render(r.arr(), len(r.shapes), r.light, r.cam, mode=1, nthreads=4, want_stats=True)
        b, sb = O.render(r.arr(), len(r.shapes), r.light, r.cam, mode=1, nthreads=4, streaming=True, want_stats=True)
        assert np.array_equal(a, b) and sa == sb, r.name


def test_case_limits():
    """Finite inputs, no zero direction, world-space direction components within 2^100."""
    for c in CASES:
        for r in c.rays:
            assert all(math.isfinite(v) for v in r) and any(v != 0. for v in r[3:]) and max(abs(v) for v in r[3:]) <= 2.0 ** 100
        for s in c.shapes:
            assert all(math.isfinite(v) for v in list(s.inv) + list(s.inv_t))
