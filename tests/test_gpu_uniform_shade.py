"""The flat one-sample k_trace kernels' uniform shading path (trace_uniform_shade, csrc/rtc_kernels.hip): a wave
whose hit lanes all name one object reads that object's records through scalar loads and shades from SGPRs; every other wave
shades per lane as before. Only where an operand comes from differs, so nothing may change: each world is rendered by the
default launch and compared bit for bit — the f64 canvas and every ray counter — with the same launch under
RTC_UNIFORM_SHADE=0 (the per-lane twin of the same kernel), with the generic kernel (RTC_ONE_SAMPLE=0) and with the brute-force
launch (RTC_FLAG_NO_CULL; it has no tile rows to prove black, so rays_primary_proven_miss is left out of that one comparison),
and, where no material is specular, with the CPU oracle (`pow` is the one operation that is not bit-exact between the device
and the oracle; the specular worlds are held to tests/test_gpu_sorted_tile_lists.py's bar). The same worlds run again as six
launches over three rotating canvases on a pipeline of depth 3.

A wave is one 8x8 tile, lane = 8 * (row in the tile) + (column in the tile). Each world is built for what one of its tiles
holds — one object under all 64 lanes, one object and sky, one lane's hit, 63 lanes on one object and one lane on another, two
objects with one material, nothing — and the oracle's hit records show, before anything is rendered, that the tile holds it.
Frames are 8x8 to 24x8 pixels. Some of the worlds run again with 300 more objects out of every ray's way: the two-level
kernel's flat one-sample form (RTC_UNIFORM_SHADE's bit 2)."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).parent))
K = __import__("candidate_list_cases").sibling("candidate_list_cases")
S = K.sibling("test_gpu_sorted_tile_lists")
HW = K.sibling("test_host_whole_tile")
ONE = K.sibling("test_gpu_one_sample")
_ctx_env, same_bits, FORCE_BINS, COUNTERS = ONE._ctx_env, ONE.same_bits, ONE.FORCE_BINS, ONE.COUNTERS
TIGHT_TOL = S.TIGHT_TOL
O = K.O
SPHERE, PLANE, CUBE = K.SPHERE, K.PLANE, K.CUBE
DEV = "cuda:0"
MATTE = dict(specular=0.)
PATTERN_KINDS = ("none", "test", "stripe", "gradient", "ring", "checker", "grid")


# ------------------------------------------------------------------ worlds
def front_cam(W=8, H=8, fov=0.3):
    return K.cam_of(W, H, fov, (0., 0., -5.), (0., 0., 0.))


def on_pixel_ray(cam, x, y, t):
    r = K.pixel_ray(cam, x, y)
    return tuple(r[i] + t * r[3 + i] for i in range(3))


def patterned(kind, xf=None):
    return None if kind == "none" else (kind, (0.9, 0.2, 0.1), (0.1, 0.3, 0.8), xf)


def plane_tile(pattern="checker", **m):
    """A floor seen from above at an angle: all 64 lanes hit the plane."""
    floor = K.shp(PLANE, m=K.mat(pattern=patterned(pattern, O.chain(("scaling", 0.11, 0.11, 0.11), ("rotation_y", 0.3))), color=(0.6, 0.7, 0.4), **MATTE, **m))
    return K.number([floor]), O.light((-3., 6., -4.)), K.cam_of(8, 8, 0.5, (0., 2., -3.), (0., 0., 0.))


def sphere_outside(light=(-4., 6., -6.), **m):
    """A sphere wider than the frame, seen from outside."""
    m = {**dict(color=(0.9, 0.5, 0.2)), **MATTE, **m}
    return K.number([K.ball((0., 0., 0.), 2., **m)]), O.light(light), front_cam()


def sphere_inside():
    """Camera and light inside one sphere: every lane hits it from inside (the second root, the flipped normal)."""
    return K.number([K.ball((0., 0., 0.), 5., color=(0.4, 0.6, 0.9), **MATTE)]), O.light((1., 2., -2.)), K.cam_of(8, 8, 1.0, (0., 0.5, -1.), (0., 0.5, 1.))


def cube_corner():
    """One cube seen along its diagonal, the corner in the middle of the frame: the three face branches of its normal in one wave."""
    cube = K.shp(CUBE, m=K.mat(color=(0.3, 0.8, 0.3), **MATTE))
    return K.number([cube]), O.light((6., 3., -8.)), K.cam_of(8, 8, 0.15, (4., 4., -4.), (1., 1., -1.))


def floor_and_sky():
    """The horizon between rows 3 and 4 of the one tile: sky above, floor below."""
    floor = K.shp(PLANE, m=K.mat(pattern=patterned("checker"), **MATTE))
    return K.number([floor]), O.light((-3., 6., -4.)), K.cam_of(8, 8, 0.8, (0., 1., -5.), (0., 1., 0.))


def sphere_silhouette():
    return K.number([K.ball((0.6, 0.4, 0.), 1.0, color=(0.9, 0.5, 0.2), **MATTE)]), O.light((-4., 6., -6.)), front_cam(fov=0.5)


def one_lane(px):
    """A sphere smaller than a pixel's spacing on the ray of pixel (px, px): that lane alone hits."""
    cam = front_cam(fov=0.5)
    return K.number([K.ball(on_pixel_ray(cam, px, px, 6.), 0.1, color=(0.9, 0.9, 0.2), **MATTE)]), O.light((-4., 6., -6.)), cam


def odd_one(px):
    """63 lanes on a sphere wider than the frame, the lane of pixel (px, px) on a small sphere in front of it."""
    cam = front_cam()
    shapes = [K.ball((0., 0., 0.), 2., color=(0.9, 0.5, 0.2), **MATTE), K.ball(on_pixel_ray(cam, px, px, 2.), 0.02, color=(0.1, 0.9, 0.9), ambient=0.4, **MATTE)]
    return K.number(shapes), O.light((-4., 6., -6.)), cam


def twins():
    """Two spheres with one material and different transforms meeting in the tile."""
    m = dict(color=(0.7, 0.3, 0.6), pattern=patterned("stripe", O.chain(("scaling", 0.2, 0.2, 0.2))), **MATTE)
    return K.number([K.ball((-0.9, 0., 0.), 1.2, **m), K.ball((0.9, 0., 0.3), 1.2, **m)]), O.light((-4., 6., -6.)), front_cam()


def all_miss_tile():
    """Three tiles in one tile row: a small sphere in the first, nothing in the other two."""
    cam = front_cam(24, 8, 0.9)
    return K.number([K.ball(on_pixel_ray(cam, 3, 3, 5.), 0.3, color=(0.9, 0.5, 0.2), **MATTE)]), O.light((-4., 6., -6.)), cam


def posed_pattern():
    """A scaled and rotated sphere wider than the frame under a pattern with a transform of its own."""
    xf = O.chain(("scaling", 0.3, 0.2, 0.25), ("rotation_z", 0.5), ("translation", 0.1, 0., 0.05))
    ball = K.shp(SPHERE, ("scaling", 2.5, 1.6, 2.0), ("rotation_z", 0.4), ("rotation_y", 0.7), m=K.mat(pattern=patterned("gradient", xf), **MATTE))
    return K.number([ball]), O.light((-4., 6., -6.)), front_cam()


def shadow_beside_light():
    """A floor under a slab that is out of view: the last tile lies in its shadow (lighting's ambient-only return), the first in the light."""
    floor = K.shp(PLANE, m=K.mat(pattern=patterned("grid", O.chain(("scaling", 0.07, 0.07, 0.07))), **MATTE))
    slab = K.shp(CUBE, ("scaling", 0.45, 0.05, 3.), ("translation", 0.55, 5., 0.), m=K.mat(color=(0.5, 0.5, 0.5), **MATTE))
    return K.number([floor, slab]), O.light((0., 10., 0.)), K.cam_of(24, 8, 0.3, (0., 1., -4.), (0., 0., 0.))


def crowded(shapes, lgt, cam):
    """The same world behind 300 small spheres that no ray of the frame and no shadow ray meets: more than 256 objects select
    the two-level kernel (source 4), whose flat one-sample form has the path too. The world's own objects keep indices 0..."""
    far = [K.ball((-30. + 0.2 * i, -40. - 0.1 * (i % 9), -60. - 0.3 * (i % 13)), 0.05, color=(0.2, 0.9, 0.2), **MATTE) for i in range(300)]
    return K.number(list(shapes) + far), lgt, cam


def build_cases():
    """name -> (shapes, light, camera, what the oracle's hit records must show of tile (tx, 0))"""
    cs = {
        "plane_tile": (*plane_tile(), dict(all_hit=0)),
        "sphere_outside": (*sphere_outside(), dict(all_hit=0, inside=False)),
        "sphere_inside": (*sphere_inside(), dict(all_hit=0, inside=True)),
        "cube_corner": (*cube_corner(), dict(all_hit=0, normals=3)),
        "floor_and_sky": (*floor_and_sky(), dict(hit_lanes=set(range(32, 64)))),
        "sphere_silhouette": (*sphere_silhouette(), dict(some_sky=True)),
        "one_lane[0]": (*one_lane(0), dict(hit_lanes={0})),
        "one_lane[63]": (*one_lane(7), dict(hit_lanes={63})),
        "odd_one[lowest]": (*odd_one(0), dict(odd=(0, 1, 0))),     # (lane, its object, everyone else's)
        "odd_one[highest]": (*odd_one(7), dict(odd=(63, 1, 0))),
        "twins": (*twins(), dict(objects={0, 1})),
        "all_miss_tile": (*all_miss_tile(), dict(empty_tiles=(1, 2))),
        "posed_pattern": (*posed_pattern(), dict(all_hit=0)),
        "shadow_beside_light": (*shadow_beside_light(), dict(shadowed_tile=2, lit_tile=0)),
    }
    for kind in PATTERN_KINDS:
        cs[f"pattern[{kind}]"] = (*plane_tile(kind), dict(all_hit=0))
    for ks in (0., 0.3):
        for sh in (0., 200.):
            cs[f"specular[{ks},{sh}]"] = (*sphere_outside(light=(-0.5, 0.5, -6.), specular=ks, shininess=sh), dict(all_hit=0))   # (the highlight inside the frame)
    for name in ("plane_tile", "sphere_inside", "cube_corner", "floor_and_sky", "odd_one[lowest]", "twins", "posed_pattern", "shadow_beside_light", "specular[0.3,200.0]"):
        cs[f"two_level[{name}]"] = (*crowded(*cs[name][:3]), cs[name][3])
    return cs


CASES = build_cases()


def source_of(name):
    return 4 if name.startswith("two_level") else 3


def tile_records(name):
    """The oracle's hit records of the case, per tile of its one tile row: {tx: [RtcHit of lane 0..63]}"""
    shapes, lgt, cam, _ = CASES[name]
    assert cam.vsize == 8 and cam.hsize % 8 == 0
    out = {tx: [None] * 64 for tx in range(cam.hsize // 8)}
    for x, y, h in K.hits_of(K.ListCase(name, "", shapes, lgt, cam)):
        out[x // 8][8 * y + x % 8] = h
    return out


def check_structure(name):
    show = CASES[name][3]
    tiles = tile_records(name)
    idx = {tx: [h.hit_index for h in hs] for tx, hs in tiles.items()}
    if "all_hit" in show:
        assert idx[0] == [show["all_hit"]] * 64, (name, idx[0])
    if "inside" in show:
        assert all(bool(h.inside) == show["inside"] for h in tiles[0]), name
    if "normals" in show:   # a cube's face normals: one axis each
        faces = {max(range(3), key=lambda a: abs(h.normal[a])) for h in tiles[0]}
        assert len(faces) == show["normals"], (name, faces)
    if "hit_lanes" in show:
        assert {l for l, j in enumerate(idx[0]) if j >= 0} == show["hit_lanes"], (name, idx[0])
    if show.get("some_sky"):
        assert 0 < sum(j >= 0 for j in idx[0]) < 64 and idx[0][0] < 0, (name, idx[0])   # (lane 0 misses: the lowest hit lane is not lane 0)
    if "odd" in show:
        lane, obj, rest = show["odd"]
        assert idx[0] == [obj if l == lane else rest for l in range(64)], (name, idx[0])
    if "objects" in show:
        assert set(idx[0]) == show["objects"], (name, idx[0])
    if "empty_tiles" in show:
        assert any(j >= 0 for j in idx[0]) and all(idx[tx] == [-1] * 64 for tx in show["empty_tiles"]), (name, idx)
    if "shadowed_tile" in show:
        assert idx[show["shadowed_tile"]] == [0] * 64 and all(h.shadowed for h in tiles[show["shadowed_tile"]]), name
        assert idx[show["lit_tile"]] == [0] * 64 and not any(h.shadowed for h in tiles[show["lit_tile"]]), name


# ------------------------------------------------------------------ contexts and launches
@pytest.fixture(scope="module")
def ctxs(rtc):
    out = {"default": _ctx_env(rtc, **FORCE_BINS), "per_lane": _ctx_env(rtc, RTC_UNIFORM_SHADE=0, **FORCE_BINS),
           "generic": _ctx_env(rtc, RTC_ONE_SAMPLE=0, **FORCE_BINS), "pipelined": _ctx_env(rtc, **FORCE_BINS)}
    yield out
    for c in out.values():
        c.close()


class Frames:
    """Each case once per kind of launch: the frames, the counters and the launch info; the oracle's frame once."""

    def __init__(self, rtc, ctxs):
        self.rtc, self.ctxs, self.held, self.oracle = rtc, ctxs, {}, {}

    def want(self, name):
        if name not in self.oracle:
            shapes, lgt, cam, _ = CASES[name]
            a = (O.RtcShape * max(1, len(shapes)))(*shapes)
            img, st = O.render(a, len(shapes), lgt, cam, mode=1, want_stats=True)
            img.setflags(write=False)
            self.oracle[name] = (img, st)
        return self.oracle[name]

    def on(self, name, ctx_name, launches=1, depth=1, flags=0):
        key = (name, ctx_name, launches, depth, flags)
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
                    dw.render_rows(cam, 0, cam.vsize, ring[i % depth].data_ptr(), self.rtc.MODE_RENDER_ASYNC, flags)
                ctx.synchronize()
                st = ctx.stats(extended=True)
            finally:
                ctx.set_pipeline(1)
            info = ctx.last_launch_info()
            dw.close()
            self.held[key] = ([t.cpu().numpy() for t in ring], st, info)
        return self.held[key]


@pytest.fixture(scope="module")
def frames(rtc, ctxs):
    return Frames(rtc, ctxs)


def matte(name):
    return all(s.material.specular == 0. for s in CASES[name][0])


def against_oracle(name, img, st, want, launches=1):
    wimg, wst = want
    err = float(np.max(np.abs(img - wimg)))
    if matte(name):
        assert same_bits(img, wimg), (name, "!= oracle", err)
    else:
        print(f"{name}: max|gpu - oracle| = {err:.3e} (bound {TIGHT_TOL:.1e})")
        assert err <= TIGHT_TOL, (name, err)
    assert {k: st[k] for k in wst} == {k: launches * v for k, v in wst.items()}, (name, st, wst)


# ------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", list(CASES))
def test_uniform_path_renders_what_the_per_lane_path_renders(rtc, frames, name):
    check_structure(name)
    shapes, lgt, cam, _ = CASES[name]
    (img,), st, info = frames.on(name, "default")
    # the launch: the flat (no frame stack) kernel of the world's size with tile lists, a whole-tile launch by the host's own rule
    assert (info["source"], info["reflective"], info["refractive"], info["binned_primary_pass"]) == (source_of(name), False, False, True), info
    assert HW.whole(rtc, HW.frame(cam.hsize, cam.vsize)), "not a whole-tile launch"
    for other in ("per_lane", "generic"):
        (oimg,), ost, oinfo = frames.on(name, other)
        assert oinfo["source"] == source_of(name) and oinfo["binned_primary_pass"], (other, oinfo)
        assert same_bits(img, oimg), (name, other, int(np.count_nonzero((img != oimg).any(axis=2))))
        assert st == ost, (name, other, st, ost)
    (bimg,), bst, binfo = frames.on(name, "default", flags=rtc.FLAG_NO_CULL)
    assert not binfo["binned_primary_pass"], binfo
    assert same_bits(img, bimg), (name, "brute force", int(np.count_nonzero((img != bimg).any(axis=2))))
    a, b = dict(st), dict(bst)
    a.pop("rays_primary_proven_miss"), b.pop("rays_primary_proven_miss")   # (the brute-force launch has no tile rows to prove black)
    assert a == b, (name, "brute force", st, bst)
    against_oracle(name, img, st, frames.want(name))


@pytest.mark.parametrize("name", list(CASES))
def test_the_one_sample_kernel_and_its_rgba_form(rtc, ctxs, frames, name):
    """The path's other two kernels: an 8-bit canvas beside the f64 one keeps a launch off the whole-tile kernel, a gamma table
    selects the RGBA form. Both against their per-lane twins, and the f64 rows against the whole-tile kernel's frame."""
    shapes, lgt, cam, _ = CASES[name]
    pair = [ctxs["default"], ctxs["per_lane"]]
    dws = [c.upload(K.as_world(rtc, shapes, lgt)) for c in pair]
    try:
        for output in ("f64+u8", "rgba"):
            got = [ONE.launch(rtc, c, d, [cam], rtc.MODE_RENDER_ASYNC, output) for c, d in zip(pair, dws)]
            for k in range(3):
                assert (got[0][k] is None) == (got[1][k] is None) and (got[0][k] is None or same_bits(got[0][k], got[1][k])), (name, output, k)
            assert got[0][3] == got[1][3], (name, output, got[0][3], got[1][3])
            if output == "f64+u8":
                assert same_bits(got[0][0], frames.on(name, "default")[0][0]), (name, "one-sample kernel != whole-tile kernel")
    finally:
        for d in dws:
            d.close()


@pytest.mark.parametrize("name", list(CASES))
def test_six_pipelined_launches_over_rotating_canvases(frames, name):
    imgs, st, info = frames.on(name, "pipelined", launches=6, depth=3)
    assert info["binned_primary_pass"] and info["source"] == source_of(name), info
    (ref,), rst, _ = frames.on(name, "per_lane")
    for k, img in enumerate(imgs):
        assert same_bits(img, ref), (name, "canvas", k)
    assert st == {k: 6 * v for k, v in rst.items()}, (name, st, rst)
    against_oracle(name, imgs[0], st, frames.want(name), launches=6)
