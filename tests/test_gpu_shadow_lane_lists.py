"""The one-level listed shadow pass (k_trace, SRC_CULL): every lane walks the light-space list of its OWN direction cell.
Worlds of at most 256 objects in which one 8x8 wave meets one cell, a few cells, many cells, a full and an overflowing
list, an occluder listed in many cells, unbounded occluders, origins beyond pre_limit, scaled and far worlds, no / one
object, secondary (reflective, glass) shadow rays and two lights — at two frame sizes that end inside a tile.

Per case the f64 canvas, the 8-bit frame and every ray counter are bit-identical with the lists on, with RTC_LIGHT_LISTS=0,
with the binning forced on and off, and under RTC_FLAG_NO_CULL; and equal to the oracle under the parity contract of
test_gpu_parity.py (TIGHT_TOL per light, exact counts). A launch without lists where lists were requested fails."""
import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).parent))
K = __import__("candidate_list_cases").sibling("candidate_list_cases")
_ctx_env = K.sibling("test_gpu_group")._ctx_env
TIGHT_TOL = K.sibling("test_gpu_parity").TIGHT_TOL
O = K.O
SIZES = ((37, 29), (64, 40))
LIGHT = (-3., 8., -2.)
VIEW = dict(fov=0.9, frm=(0., 4., -9.), to=(0., 0.5, 3.))


def floor(**m):
    return K.shp(K.PLANE, m=K.mat(**(m or dict(color=(0.8, 0.8, 0.7), specular=0.))))


def one_cell(k, fill, fov=0.09):
    """candidate_list_cases' light_cell_cap geometry: k tiny spheres inside ONE direction cell of a light 100 above the floor,
    seen straight down through a 0.09 rad view — a tile's hit points span a seventh of a cell (three sevenths at 0.27 rad:
    most tiles then lie across a border or a corner of the cells)."""
    lp = (0., 100., 0.)
    g = (70 + 0.5) * 2. / K.LIGHT_R - 1.
    cell = K.light_cell((g, -1., g))
    dl = math.sqrt(2 * g * g + 1.)
    shapes = [floor()]
    side = math.ceil(math.sqrt(k))
    for i in range(k):
        du, dv = (-0.0055 + 0.011 * (i % side) / (side - 1), -0.0055 + 0.011 * (i // side) / (side - 1))
        di = (g + dv, -1., g + du)
        t = 30. + 40. * ((i * 37) % k) / k
        shapes.append(K.ball((lp[0] + t * di[0], lp[1] + t * di[1], lp[2] + t * di[2]), 0.0004 * t * dl, color=(0.9, 0.2, 0.2)))
        assert K.light_cell(di) == cell
    shapes += [K.ball((-60. + 0.2 * i, 5. + 0.1 * i, 30. + 10. * (i % 7)), 2., color=(0.2, 0.9, 0.2)) for i in range(fill)]
    P = (100. * g, 0., 100. * g)
    return shapes, [lp], dict(fov=fov, frm=(P[0], 20., P[2]), to=P, up=(0., 0., 1.))


def scaled_field(n, seed, s):
    """field_world's layout with every length multiplied by s (objects, light and camera alike)."""
    rng = np.random.default_rng(seed)
    u = lambda a, b: float(rng.uniform(a, b))
    shapes = [K.ball((s * u(-5, 5), s * u(0.4, 3.), s * u(-3, 10)), s * u(0.08, 0.35), color=(u(0.1, 1), u(0.1, 1), u(0.1, 1))) for _ in range(n - 1)]
    shapes.append(floor(pattern=("checker", (0.3,) * 3, (0.7,) * 3, None), specular=0.))
    return shapes, [tuple(s * v for v in LIGHT)], dict(fov=0.9, frm=(0., 4. * s, -9. * s), to=(0., 0.5 * s, 3. * s))


def pre_limit_world(n):
    """A compact cluster and a low light far behind it: the shadows fall ~200 away, |over|_1 > pre_limit = 64 x the extent."""
    rng = np.random.default_rng(n + 9)
    shapes = [K.ball((float(rng.uniform(-.5, .5)), 1. + float(rng.uniform(-.3, .3)), float(rng.uniform(-.5, .5))), 0.1, color=(0.9, 0.6, 0.2)) for _ in range(n - 1)]
    shapes.append(floor(color=(0.7, 0.7, 0.8), specular=0.))
    return shapes, [(-200., 2., 0.)], dict(fov=0.5, frm=(200., 12., -25.), to=(200., 0., 0.))


def worlds():
    """name -> (shapes, light positions, view)."""
    off = (1e6, 1e6, 1e6)
    far = lambda p: tuple(a + b for a, b in zip(p, off))
    grounded = [K.ball((-3. + 0.7 * i, 0.25, 1. + (i % 3)), 0.25, color=(0.9, 0.7, 0.1)) for i in range(10)]
    big = K.ball((1., 1.5, 3.), 1.2, color=(0.8, 0.3, 0.3))                  # 1.2 wide, 8 from the light: in some 20 x 20 cells
    wall = K.shp(K.PLANE, ("rotation_z", math.pi / 2), ("translation", -1.5, 0., 0.), m=K.mat(color=(0.6, 0.5, 0.4)))
    return {
        "one_cell[16=cap]": one_cell(16, 20),
        "one_cell[17=overflow]": one_cell(17, 20),
        "few_cells": one_cell(16, 20, fov=0.27),
        "many_cells[field]": (list(K.field_world(60, seed=3)), [LIGHT], VIEW),       # (frames this small: a cell per pixel)
        "many_cells[field,256]": (list(K.field_world(256, seed=256)), [LIGHT], VIEW),
        "many_cells[light_low]": (grounded + list(K.field_world(50, seed=61)), [(0.3, 0.05, 2.)], VIEW),
        "occluder_in_many_cells": ([big] + list(K.field_world(59, seed=4)), [LIGHT], VIEW),
        "occluder_in_every_cell": ([K.ball((0., 0., 0.), 40., color=(0.5, 0.6, 0.9))] + list(K.field_world(59, seed=64)), [LIGHT], VIEW),
        "unbounded[wall_plane]": ([wall] + list(K.field_world(59, seed=65)), [LIGHT], VIEW),
        "unbounded[cube]": ([K.ill_conditioned(K.CUBE, (-1., 2.5, 3.), color=(0.3, 0.9, 0.4))] + list(K.field_world(59, seed=66)), [LIGHT], VIEW),
        "beyond_pre_limit": pre_limit_world(40),
        "scaled[x50]": scaled_field(60, 5, 50.),
        "scaled[x0.1]": scaled_field(60, 6, 0.1),
        "far_1e6": (list(K.field_world(60, seed=3, off=off)), [far(LIGHT)], dict(fov=0.9, frm=far(VIEW["frm"]), to=far(VIEW["to"]))),
        "objects[0]": ([], [LIGHT], VIEW),
        "objects[1]": ([floor()], [LIGHT], VIEW),
        "reflective": (list(K.field_world(60, seed=66, variant="reflective")), [LIGHT], VIEW),
        "glass": (list(K.field_world(60, seed=67, variant="glass")), [LIGHT], VIEW),
        "two_lights": (list(K.field_world(60, seed=8)), [LIGHT, (4., 5., -4.)], VIEW),
        "two_lights[reflective]": (list(K.field_world(40, seed=9, variant="reflective")), [LIGHT, (0.3, 0.05, 2.)], VIEW),
    }


WORLDS = worlds()
CONFIGS = {"lists": {}, "no_lists": dict(RTC_LIGHT_LISTS=0), "binned": dict(RTC_BIN_SMALL_PIXELS=0), "unbinned": dict(RTC_BINNING=0)}


@pytest.fixture(scope="module")
def ctxs(rtc):
    out = {name: _ctx_env(rtc, **env) for name, env in CONFIGS.items()}
    yield out
    for c in out.values():
        c.close()


@functools.lru_cache(maxsize=None)
def oracle_frame(name, size):
    """(sum of the oracle's single-light frames in light order, the first light's counters): computed once, never written to."""
    shapes, lights, view = WORLDS[name]
    shapes = K.number(list(shapes))
    cam = K.cam_of(*size, **view)
    a = (O.RtcShape * max(1, len(shapes)))(*shapes)
    ref, st = None, None
    for lp in lights:
        img, s = O.render(a, len(shapes), O.light(lp), cam, mode=1, nthreads=16, want_stats=True)
        ref, st = (img, s) if ref is None else (ref + img, st)
    ref.setflags(write=False)
    return ref, st


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(WORLDS))
def test_every_configuration_renders_the_same_frame(rtc, ctxs, name, size):
    shapes, lights, view = WORLDS[name]
    shapes = K.number(list(shapes))
    cam = K.cam_of(*size, **view)
    w = K.as_world(rtc, shapes, [O.light(lp) for lp in lights])
    want, ost = oracle_frame(name, size)
    ost = dict(ost, rays_shadow=len(lights) * ost["rays_shadow"])   # one shadow ray per hit and light, nothing else changes
    wants_lists = len(shapes) >= 32                                  # rtc_world_create builds light lists from 32 objects
    got, bad = {}, []
    for cfg, ctx in ctxs.items():
        dw = ctx.upload(w)
        try:
            img, st = dw.render(cam, with_stats=True)
            info = ctx.last_launch_info()
            u8 = dw.render_rgb8(cam)
            got[cfg] = (img, u8, st)
            if info["light_lists"] != (wants_lists and cfg != "no_lists"):
                bad.append((cfg, "light_lists", info["light_lists"]))
            if cfg in ("binned", "unbinned") and info["binned_primary_pass"] != (cfg == "binned" and len(shapes) > 0):   # (nothing to bin in an empty World)
                bad.append((cfg, "binned_primary_pass", info["binned_primary_pass"]))
            if cfg == "lists":
                brute, sb = dw.render(cam, flags=rtc.FLAG_NO_CULL, with_stats=True)
                got["no_cull"] = (brute, dw.render_rgb8(cam, flags=rtc.FLAG_NO_CULL), sb)
        finally:
            dw.close()
    img, u8, st = got["lists"]
    err = float(np.max(np.abs(img - want))) if img.size else 0.
    print(f"{name} {size}: n {len(shapes)} lights {len(lights)} max|d oracle| {err:.3e} (bound {len(lights) * TIGHT_TOL:.1e}) stats {st}")
    for cfg, (i2, u2, s2) in got.items():
        if i2.tobytes() != img.tobytes():
            bad.append((cfg, "canvas differs", int(np.count_nonzero((i2 != img).any(axis=2)))))
        if u2.tobytes() != u8.tobytes():
            bad.append((cfg, "8-bit frame differs"))
        if s2 != st:
            bad.append((cfg, "counters differ", s2, st))
    if not (err <= len(lights) * TIGHT_TOL and st == ost):
        bad.append(("oracle", err, st, ost))
    if len(shapes) and not img.any():
        bad.append(("black frame",))
    if wants_lists and not st["rays_shadow"]:
        bad.append(("no shadow rays",))
    assert not bad, bad


def test_the_cases_reach_what_they_are_built_for():
    """From the oracle's hit records alone, at 64x40: the number of direction cells one 8x8 tile's hit points see the light
    in, lit and shadowed floor points, origins beyond pre_limit's scale."""
    def tiles_of(name):
        shapes, lights, view = WORLDS[name]
        case = K.ListCase(name, "", K.number(list(shapes)), O.light(lights[0]), K.cam_of(64, 40, **view))
        cells, lit, dark = {}, 0, 0
        for x, y, h in K.hits_of(case):
            if h.hit_index >= 0:
                cells.setdefault((x // 8, y // 8), set()).add(K.light_cell(tuple(h.over_point[i] - lights[0][i] for i in range(3))))
                lit, dark = lit + (not h.shadowed), dark + bool(h.shadowed)
        return [len(v) for v in cells.values()], lit, dark
    per_tile, lit, dark = tiles_of("one_cell[16=cap]")
    assert min(per_tile) == 1 and max(per_tile) <= 2 and lit and dark, (per_tile, lit, dark)
    per_tile, lit, dark = tiles_of("few_cells")
    assert max(per_tile) <= 4 and sum(2 <= c <= 4 for c in per_tile) >= len(per_tile) // 2 and lit and dark, (per_tile, lit, dark)
    per_tile, lit, dark = tiles_of("many_cells[light_low]")
    assert max(per_tile) > 4 and lit and dark, (per_tile, lit, dark)
    for name in ("occluder_in_many_cells", "unbounded[cube]", "beyond_pre_limit", "scaled[x50]", "far_1e6"):
        _, lit, dark = tiles_of(name)
        assert lit and dark, (name, lit, dark)
    _, lit, dark = tiles_of("unbounded[wall_plane]")     # the wall stands between the light and everything the camera sees
    assert dark and not lit, (lit, dark)
