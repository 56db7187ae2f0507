"""The flat one-sample k_trace kernels' shorter load chains (trace_short_chains, csrc/rtc_kernels.hip): loads
are moved, merged and requested together, nothing else — so nothing may change. The generic anti-aliased kernel keeps the
code it had and is the in-tree reference: every case is rendered by a context that takes the flat whole-tile kernel, by one
under RTC_ONE_SAMPLE=0 (the generic kernel), by one under RTC_BINNING=0 (the same flat kernel without tile lists and row
words: its pointer tests) and by one under RTC_LIGHT_LISTS=0 (no light cells), and the f64 frames and every ray counter
are compared bit for bit; then against the CPU oracle — to the bit where every material has specular = 0, as
tests/test_gpu_whole_tile.py does, and within TIGHT_TOL (tests/test_gpu_sorted_tile_lists.py's bar) for the imported worlds
whose materials are specular: `pow` is the one operation that is not bit-exact between the device and the oracle. The same
cases run again as six launches over three rotating canvases on a pipeline of depth 3.

last_launch_info and rtc_debug_whole_tile_launch show that the first context really ran the flat whole-tile kernel with
tile lists, and the read-backs (rtc_debug_tile_counts, rtc_debug_tile_lists, rtc_debug_world_lists) that each case reached
the list length, the cell count, the row words or the n_unb it was built for, and that the short lists were sorted.

Frames are 64x64 or smaller. Worlds come from the builders of tests/candidate_list_cases.py and
tests/test_gpu_sorted_tile_lists.py; what they do not have (the three kinds in one wave, the nearer later candidate, cells of
0, 1, 4 and 5 entries, a frame of sky) is built here from the same pieces."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).parent))
K = __import__("candidate_list_cases").sibling("candidate_list_cases")
G = K.sibling("test_gpu_candidate_lists")
S = K.sibling("test_gpu_sorted_tile_lists")
HW = K.sibling("test_host_whole_tile")
ONE = K.sibling("test_gpu_one_sample")
_ctx_env, same_bits, FORCE_BINS = ONE._ctx_env, ONE.same_bits, ONE.FORCE_BINS
TIGHT_TOL = S.TIGHT_TOL
O = K.O
SPHERE, PLANE, CUBE = K.SPHERE, K.PLANE, K.CUBE
CAP, SORT_CAP, CAP_SMALL = K.TILE_CAP, S.SORT_CAP, K.CAP_SMALL
W = H = 64
DEV = "cuda:0"
MATTE = dict(specular=0.)


# ------------------------------------------------------------------ worlds
def floor(**m):
    return K.shp(PLANE, m=K.mat(pattern=("checker", (0.3,) * 3, (0.7,) * 3, None), **MATTE, **m))


def three_kinds():
    """One 8x8 frame — one wave — from inside a large sphere: its lanes hit the far side of that sphere (second root), a small
    sphere in front (first root), a cube and the floor."""
    cam = K.cam_of(8, 8, 0.9, (0., 1., -4.), (0., 0.6, 0.))
    shapes = [K.ball((0., 1., -4.), 9., color=(0.5, 0.6, 0.9), **MATTE), K.ball((-0.7, 0.9, -1.5), 0.45, color=(0.9, 0.3, 0.2), **MATTE),
              K.shp(CUBE, ("scaling", 0.4, 0.4, 0.4), ("rotation_y", 0.5), ("translation", 0.8, 0.8, -1.5), m=K.mat(color=(0.3, 0.8, 0.3), **MATTE)),
              floor()]
    return K.number(shapes), O.light((-2., 5., -6.)), cam


def nearer_later():
    """A large sphere whose list key (the distance to its bounding sphere) is the smallest of its tiles' lists, and a small cube
    whose key is larger but which stands in front of the sphere's surface where its pixels look: the cube is tested after
    the sphere and replaces it; the floor — unbounded, tested first of all — is replaced by both."""
    cam = K.cam_of(W, H, 1.2, (0., 2., -8.), (0., 2., 6.))
    # sphere: key 14 - 6 = 8, met after 11 where the cube's pixels look (0.42 rad off the axis, near its silhouette at 0.44);
    # cube: 9.6 away, key 9.6 - 0.3 sqrt 3 = 9.1
    shapes = [K.ball((0., 2., 6.), 6., color=(0.8, 0.8, 0.3), **MATTE),
              K.shp(CUBE, ("scaling", 0.3, 0.3, 0.3), ("rotation_y", 0.3), ("translation", 3.94, 2.0, 0.755), m=K.mat(color=(0.2, 0.4, 0.9), **MATTE)),
              floor()]
    return K.number(shapes), O.light((-4., 8., -6.)), cam


def unbounded(planes, spheres=10):
    """`spheres` small spheres in one tile over 0, 1 or 2 planes (a floor, a back wall)."""
    cam = K.cam_of(W, H, 1.0, (0., 0., 0.), (0., 0., 1.))
    shapes = K.string_of_spheres(cam, 3, 2, spheres, 5., 8.) if spheres else []
    poses = ((("translation", 0., -2., 0.),), (("rotation_x", math.pi / 2), ("translation", 0., 0., 12.)))
    shapes += [K.shp(PLANE, *poses[i], m=K.mat(color=(0.5 + 0.2 * i, 0.6, 0.4), **MATTE)) for i in range(planes)]
    return K.number(shapes), O.light((-4., 6., -3.)), cam


def one_sphere():
    return K.number([K.ball((0.3, 0.2, 5.), 1.2, color=(0.9, 0.5, 0.2), **MATTE)]), O.light((-4., 6., -3.)), K.cam_of(W, H, 1.0, (0., 0., 0.), (0., 0., 1.))


def all_sky():
    """Forty spheres behind the camera: every tile row is proven black."""
    shapes = [K.ball((0.4 * (i % 8) - 1.4, 0.4 * (i // 8), -6.), 0.15, color=(0.9, 0.5, 0.2), **MATTE) for i in range(40)]
    return K.number(shapes), O.light((-4., 6., -3.)), K.cam_of(W, H, 1.0, (0., 0., 0.), (0., 0., 1.))


LIGHT_AT = (0., 100., 0.)
CELL_G = (70 + 0.5) * 2. / K.LIGHT_R - 1.
CELL = K.light_cell((CELL_G, -1., CELL_G))


def cell_world(k):
    """k small spheres in ONE direction cell of the light (light_cases' light_cell_cap construction, candidate_list_cases.py),
    40 spheres far from that direction so that the World has light lists, a floor seen straight down under the cell."""
    g, lp = CELL_G, LIGHT_AT
    dl = math.sqrt(2 * g * g + 1.)
    shapes = [K.shp(PLANE, m=K.mat(color=(0.8, 0.8, 0.7), **MATTE))]
    side = max(2, math.ceil(math.sqrt(k)))
    for i in range(k):
        du, dv = (-0.0055 + 0.011 * (i % side) / (side - 1), -0.0055 + 0.011 * (i // side) / (side - 1))
        di = (g + dv, -1., g + du)
        t = 30. + 40. * ((i * 37) % k) / k
        shapes.append(K.ball((lp[0] + t * di[0], lp[1] + t * di[1], lp[2] + t * di[2]), 0.0004 * t * dl, color=(0.9, 0.2, 0.2), **MATTE))
        assert K.light_cell(di) == CELL
    shapes += [K.ball((-60. + 0.2 * i, 5. + 0.1 * i, 30. + 10. * (i % 7)), 2., color=(0.2, 0.9, 0.2), **MATTE) for i in range(40)]
    P = (100. * g, 0., 100. * g)
    return K.number(shapes), O.light(lp), K.cam_of(W, H, 0.09, (P[0], 20., P[2]), P, (0., 0., 1.))


def named(cases, name):
    c = next(c for c in cases if c.name == name)
    return c.shapes, c.light, c.cam


def build_cases():
    """name -> (shapes, light, camera, what the read-backs must show)"""
    tiles, lights = K.tile_cases(), K.light_cases()
    cs = {
        "three_kinds": (*three_kinds(), dict(n_unb=1)),
        "nearer_later": (*nearer_later(), dict(n_unb=1)),
        "tile_lengths": (*S.edge_world(), S.edge_cam(), dict(n_unb=1, tiles={S.T_EMPTY: 0, S.T_ONE: 1, S.T_COVER_MID: SORT_CAP, S.T_COVER_FIRST: SORT_CAP + 1,
                                                                              S.T_FULL: CAP, S.T_OVER: CAP + 6})),
        "unbounded[0]": (*unbounded(0), dict(n_unb=0, tiles={(3, 2): 10}, rows=(2, 2))),   # sky proven above and below the scene
        "unbounded[1]": (*unbounded(1), dict(n_unb=1, tiles={(3, 2): 10})),
        "unbounded[2]": (*unbounded(2), dict(n_unb=2, tiles={(3, 2): 10})),
        "plane_only": (*unbounded(1, spheres=0), dict(n_unb=1, n=1)),
        "sphere_only": (*one_sphere(), dict(n_unb=0, n=1)),
        "all_sky": (*all_sky(), dict(n_unb=0, rows=(0xffffffff, None))),
        "sky_below": (*named(tiles, "plane_pose[ceiling,below]"), dict(n_unb=1, rows=(0, 4))),
        "sky_above": (*named(tiles, "plane_pose[ceiling,above]"), dict(n_unb=1, rows=(1, 5))),
        "light_reach": (*named(lights, "light_reach[41]"), dict(n_unb=1, lists=True, beyond_reach=True)),
    }
    for k in (0, 1, 4, 5, CAP_SMALL, CAP_SMALL + 1):
        cs[f"light_cell[{k}]"] = (*cell_world(k), dict(n_unb=1, lists=True, cell=k))
    return cs


CASES = build_cases()


# ------------------------------------------------------------------ contexts and launches
@pytest.fixture(scope="module")
def ctxs(rtc):
    out = {"flat": _ctx_env(rtc, **FORCE_BINS), "generic": _ctx_env(rtc, RTC_ONE_SAMPLE=0, **FORCE_BINS), "walk": _ctx_env(rtc, RTC_BINNING=0),
           "no_light_lists": _ctx_env(rtc, RTC_LIGHT_LISTS=0, **FORCE_BINS), "pipelined": _ctx_env(rtc, **FORCE_BINS)}
    yield out
    for c in out.values():
        c.close()


class Frames:
    """Each case once per context: the frame, the counters, the launch info and the read-backs; the oracle's once."""

    def __init__(self, rtc, ctxs):
        self.rtc, self.ctxs, self.held, self.oracle = rtc, ctxs, {}, {}

    def want(self, name):
        if name not in self.oracle:
            shapes, lgt, cam, _ = CASES[name]
            a = (O.RtcShape * max(1, len(shapes)))(*shapes)
            img, st = O.render(a, len(shapes), lgt, cam, mode=1, nthreads=16, want_stats=True)
            img.setflags(write=False)
            self.oracle[name] = (img, st)
        return self.oracle[name]

    def on(self, name, ctx_name, launches=1, depth=1):
        key = (name, ctx_name, launches, depth)
        if key not in self.held:
            import torch
            shapes, lgt, cam, _ = CASES[name]
            ctx = self.ctxs[ctx_name]
            dw = ctx.upload(K.as_world(self.rtc, shapes, lgt))
            ring = [torch.full((cam.vsize, cam.hsize, 3), -1.0, dtype=torch.float64, device=DEV) for _ in range(depth)]
            torch.cuda.synchronize()
            ctx.set_pipeline(depth)
            try:
                ctx.reset_stats()
                for i in range(launches):
                    dw.render_rows(cam, 0, cam.vsize, ring[i % depth].data_ptr())
                ctx.synchronize()
                st = ctx.stats(extended=True)
            finally:
                ctx.set_pipeline(1)
            info = ctx.last_launch_info()
            tiles = G.tile_counts(self.rtc, ctx, dw)
            lists = S.tile_lists(self.rtc, ctx, dw) if tiles is not None else None
            world = G.world_lists(self.rtc, dw, cells=True)
            dw.close()
            self.held[key] = ([t.cpu().numpy() for t in ring], st, info, tiles, lists, world)
        return self.held[key]


@pytest.fixture(scope="module")
def frames(rtc, ctxs):
    return Frames(rtc, ctxs)


def matte(name):
    return all(s.material.specular == 0. for s in CASES[name][0])


def against_oracle(name, img, st, want, launches=1):
    wimg, wst = want
    if matte(name):
        assert same_bits(img, wimg), (name, "!= oracle", float(np.max(np.abs(img - wimg))))
    else:
        assert float(np.max(np.abs(img - wimg))) <= TIGHT_TOL, (name, float(np.max(np.abs(img - wimg))))
    assert {k: st[k] for k in wst} == {k: launches * v for k, v in wst.items()}, (name, st, wst)


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", list(CASES))
def test_flat_kernel_renders_what_the_generic_kernel_renders(rtc, frames, name):
    shapes, lgt, cam, show = CASES[name]
    (img,), st, info, tiles, lists, world = frames.on(name, "flat")
    # the launch: the flat (no frame stack) one-level kernel with tile lists, and a whole-tile launch by the host's own rule
    assert (info["source"], info["reflective"], info["refractive"], info["binned_primary_pass"]) == (3, False, False, True), info
    assert info["light_lists"] == (len(shapes) >= 32), info   # (rtc_world_create builds light lists from 32 objects)
    assert not show.get("lists") or info["light_lists"], info
    assert HW.whole(rtc, HW.frame(cam.hsize, cam.vsize)), "not a whole-tile launch"
    # ... and what the case was built to reach
    counts, rows = tiles
    assert world["n_unb"] == show["n_unb"] and world["n"] == show.get("n", len(shapes)), (name, world["n_unb"], world["n"])
    for (tx, ty), k in show.get("tiles", {}).items():
        assert counts[0, ty, tx] == k, (name, tx, ty, int(counts[0, ty, tx]), k)
    if "rows" in show:
        lo, hi = show["rows"]
        assert rows[0][0] == lo and (hi is None or rows[0][1] == hi), (name, rows)
        assert st["rays_primary_proven_miss"] == G.proven_rays(cam, 1, rows[0]) > 0, (name, st)
    if "cell" in show:
        assert world["cells"][CELL] == show["cell"] and world["cap"] == CAP_SMALL, (name, int(world["cells"][CELL]))
    if show.get("beyond_reach"):
        ds = [K.light_dist(K.ListCase(name, "", shapes, lgt, cam), h) for _, _, h in K.hits_of(K.ListCase(name, "", shapes, lgt, cam), 2)
              if h.hit_index == len(shapes) - 1]
        assert min(ds) < world["reach"] < max(ds), (name, min(ds), world["reach"], max(ds))
    # the lists the scalar walk reads are sorted
    for v, ty, tx in np.ndindex(*counts.shape):
        c = int(counts[v, ty, tx])
        if 1 < c <= SORT_CAP:
            assert (np.diff(lists[v, ty, tx, :c].astype(np.int64)) > 0).all(), (name, tx, ty, lists[v, ty, tx, :c].tolist())
    # bit for bit what the kernels that kept their code render, every ray counter included
    for other in ("generic", "walk", "no_light_lists"):
        (oimg,), ost, oinfo, *_ = frames.on(name, other)
        assert oinfo["source"] == 3 and oinfo["binned_primary_pass"] == (other != "walk"), (other, oinfo)
        assert same_bits(img, oimg), (name, other, int(np.count_nonzero((img != oimg).any(axis=2))))
        a, b = dict(st), dict(ost)
        if other == "walk":   # (the walk has no tile rows to prove black)
            a.pop("rays_primary_proven_miss"), b.pop("rays_primary_proven_miss")
        assert a == b, (name, other, st, ost)
    against_oracle(name, img, st, frames.want(name))


@pytest.mark.parametrize("name", list(CASES))
def test_six_pipelined_launches_over_rotating_canvases(frames, name):
    imgs, st, info, *_ = frames.on(name, "pipelined", launches=6, depth=3)
    assert info["binned_primary_pass"] and info["source"] == 3, info
    (ref,), rst, *_ = frames.on(name, "generic")
    for k, img in enumerate(imgs):
        assert same_bits(img, ref), (name, "canvas", k)
    assert st == {k: 6 * v for k, v in rst.items()}, (name, st, rst)
    against_oracle(name, imgs[0], st, frames.want(name), launches=6)


def test_three_kinds_and_both_roots_in_one_wave():
    """The case is what its name says: the one tile's 64 lanes hit a plane, a cube, a sphere from outside and one from inside."""
    shapes, lgt, cam, _ = CASES["three_kinds"]
    hs = [h for _, _, h in K.hits_of(K.ListCase("three_kinds", "", shapes, lgt, cam))]
    assert len(hs) == 64 and all(h.hit_index >= 0 for h in hs)
    seen = {(shapes[h.hit_index].kind, bool(h.inside)) for h in hs}
    assert {(SPHERE, True), (SPHERE, False), (CUBE, False), (PLANE, False)} <= seen, seen


def test_a_later_candidate_replaces_a_hit_of_another_kind(rtc, frames):
    """In some tile the cube decides pixels whose rays also meet the sphere and the floor behind it, and the tile's sorted
    list has the sphere in front of the cube."""
    shapes, lgt, cam, _ = CASES["nearer_later"]
    case = K.ListCase("nearer_later", "", shapes, lgt, cam)
    *_, tiles, lists, _ = frames.on("nearer_later", "flat")
    counts = tiles[0]
    a = (O.RtcShape * 1)(shapes[0])
    found = 0
    for x, y, h in K.hits_of(case):
        if h.hit_index == 1:      # the cube; does the sphere alone stop this ray?
            behind = O.color_at(a, 1, lgt, K.pixel_ray(cam, x, y), 5, want_hit=True)[1]
            order = (lists[0, y // 8, x // 8, :counts[0, y // 8, x // 8]] & 0xffff).tolist()
            if behind.hit_index == 0 and order[:2] == [0, 1]:
                found += 1
    assert found > 0
