"""k_trace's one-sample flavour: a pinhole render launch of a camera with samples == 1 runs an instantiation from which the
anti-aliasing machinery (the sample loop, the sub-sample store, the resample test, the averaging) is compiled out. The generic
kernel takes the same path when samples == 1, so nothing may change: every frame here is rendered by the default context and
by one created under RTC_ONE_SAMPLE=0 (every launch on the generic kernel), and both are compared bit for bit with each other
and with the CPU oracle, ray counters included. An anti-aliased camera must never reach the new kernel: its frames, on a scene
where pixels trip the resample test, equal the oracle's in both contexts too.

Small on purpose (the shape of tests/test_gpu_tile_setup.py): frames of 1x1, 7x3, 8x8, 9x17 and 20x12 pixels, and 72x40 (45
tiles) under RTC_TILES_SLOTS=2, where the launch plan cuts the tiles into chunks of every level. The binned primary pass is
forced (RTC_BIN_SMALL_PIXELS=0, RTC_BIN_SMALL_PIXELS_PIPELINED=0). Every material has specular = 0, so that `pow` — the one
operation that is not bit-exact between the device and the oracle — plays no part.

Worlds: three matte spheres on a checker floor and the same without the floor (the flat one-level kernel), the floor scene
with reflective materials and with a glass sphere (the frame-stack kernels), and 300 small spheres — more than 256 objects
select the two-level kernel — matte, with mirrors, with mirrors and glass. One light; two lights as the kernel-argument block
and, under RTC_LIGHT_TABLE=1, as the device table. A two-light frame's reference is the sum, in light order, of the oracle's
one-light frames (tests/test_gpu_lights.py): exact for the matte worlds, where a pixel is one lighting() per light; the
recursive worlds round differently in the last place there and are held to that file's bar against the oracle, and to the
bits against the generic kernel."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORCE_BINS = dict(RTC_BIN_SMALL_PIXELS=0, RTC_BIN_SMALL_PIXELS_PIPELINED=0)
SMALL_FRAMES = ((1, 1), (7, 3), (8, 8), (9, 17), (20, 12))
CHUNK_FRAME = (72, 40)
WORLDS = ("floor", "noplane", "mirror", "glass", "many", "manymirror", "manyglass")
MATTE = ("floor", "noplane", "many")
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "pixels")
TIGHT_TOL = 1e-12  # tests/test_gpu_lights.py's bar per light for a sum of one-light oracle frames
SECOND_LIGHT = ((1.5, 6.0, -4.0), (0.2, 0.45, 0.7))


def _ctx_env(rtc, **env):
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        return rtc.Context(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.fixture(scope="module")
def ctxs(rtc):
    """(one-sample kernel, generic kernel) per configuration"""
    out = {name: (_ctx_env(rtc, **env, **FORCE_BINS), _ctx_env(rtc, RTC_ONE_SAMPLE=0, **env, **FORCE_BINS))
           for name, env in (("binned", {}), ("chunks", dict(RTC_TILES_SLOTS=2)), ("table", dict(RTC_LIGHT_TABLE=1)),
                             ("table chunks", dict(RTC_LIGHT_TABLE=1, RTC_TILES_SLOTS=2)))}
    yield out
    for pair in out.values():
        for c in pair:
            c.close()


def scene(rtc, kind, W, H, lights=None):
    M = rtc.Matrix
    w = rtc.World(lights if lights is not None else rtc.light())
    mirror = 0.35 if kind == "mirror" else 0.0
    balls = ((-1.5, 0.5, 0.0, 0.5, (0.9, 0.3, 0.2)), (0.2, 1.0, 1.0, 1.0, (0.2, 0.8, 0.3)), (1.7, 0.4, -1.0, 0.4, (0.3, 0.4, 0.9)))
    if kind.startswith("many"):   # 20 x 15 small spheres over the floor, the three balls in front of them
        for i in range(300):
            x, z = -4.75 + 0.5 * (i % 20), 2.5 + 0.8 * (i // 20)
            col = (0.2 + 0.6 * ((i * 7) % 11) / 10.0, 0.2 + 0.6 * ((i * 5) % 13) / 12.0, 0.2 + 0.6 * ((i * 3) % 17) / 16.0)
            mat = dict(color=col, ambient=0.15, diffuse=0.75, specular=0.0)
            if kind != "many" and i % 7 == 0:
                mat.update(reflective=0.3)
            if kind == "manyglass" and i % 11 == 3:
                mat.update(transparency=0.7, refractive_index=1.4)
            w.add_shape(rtc.sphere(M.identity().scaling(0.17, 0.17, 0.17).translation(x, 0.17 + 0.05 * (i % 3), z), rtc.material(**mat)))
    for k, (x, y, z, r, col) in enumerate(balls):
        mat = dict(color=col, ambient=0.2, diffuse=0.7, specular=0.0, reflective=mirror)
        if kind in ("glass", "manyglass") and k == 1:
            mat = dict(color=(0.1, 0.1, 0.1), ambient=0.1, diffuse=0.2, specular=0.0, transparency=0.9, reflective=0.2, refractive_index=1.5)
        w.add_shape(rtc.sphere(M.identity().scaling(r, r, r).translation(x, y, z), rtc.material(**mat)))
    if kind != "noplane":
        w.add_shape(rtc.plane(M.identity(), rtc.material(specular=0.0, reflective=mirror, pattern=("checker", (0.35, 0.35, 0.35), (0.65, 0.65, 0.65), None))))
    cam = rtc.camera(W, H, 0.9, M.make_view_transform((0.0, 2.0, -8.0), (0.0, 1.6, 5.0), (0.0, 1.0, 0.0)))   # the horizon inside the frame
    return w, cam


def other_camera(rtc, W, H):
    return rtc.camera(W, H, 0.8, rtc.Matrix.make_view_transform((1.0, 3.0, -9.0), (0.0, 1.5, 5.0), (0.0, 1.0, 0.0)))


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float64:
        return bool(np.array_equal(got, want))
    return bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


class Oracle:
    """The CPU oracle's frames and ray counts, each computed once and never written to."""

    def __init__(self, O):
        self.O, self.cache = O, {}

    def frame(self, key, w, cam, mode, y0=0, y1=None, light=None, flags=0):
        k = (key, cam.hsize, cam.vsize, cam.samples, mode, y0, y1, flags)
        if k not in self.cache:
            img, st = self.O.render(w.array(), len(w), light if light is not None else w.light, cam, mode=mode, y0=y0, y1=y1,
                                    want_stats=True, flags=flags)
            img.setflags(write=False)
            self.cache[k] = (img, st)
        return self.cache[k]


@pytest.fixture(scope="module")
def oracle(O):
    return Oracle(O)


def launch(rtc, ctx, dw, cams, mode, output, y0=0, flags=0):
    """One launch of `cams` (one camera: rtc_render_rows; several: rtc_render_views; RGBA: rtc_render_views_rgba8) ->
    (f64 rows, 8-bit rows, RGBA rows — None where not asked for —, the context's counters of the launch)."""
    import torch
    W, H = cams[0].hsize, cams[0].vsize
    HP = -(-H // 8) * 8
    rows = H - y0 if len(cams) == 1 and output != "rgba" else len(cams) * HP
    f = torch.full((rows, W, 3), -1.0, dtype=torch.float64, device=DEV) if output in ("f64", "f64+u8") else None
    q = torch.full((rows, W, 3), 9, dtype=torch.uint8, device=DEV) if output in ("f64+u8", "u8") else None
    a = torch.full((rows, W, 4), 9, dtype=torch.uint8, device=DEV) if output == "rgba" else None
    torch.cuda.synchronize()
    ctx.reset_stats()
    fp, qp = (f.data_ptr() if f is not None else None), (q.data_ptr() if q is not None else None)
    if output == "rgba":
        assert y0 == 0
        dw.render_views_rgba8(cams, 0, 1, a.data_ptr(), HP, 2.2, mode, flags)
    elif len(cams) == 1:
        dw.render_rows(cams[0], y0, H, fp, mode, flags, d_ptr8=qp)
    else:
        assert y0 == 0
        dw.render_views(cams, 0, 1, fp, HP, mode, flags, d_ptr8=qp)
    st = ctx.stats(extended=True)
    ctx.synchronize()
    return (None if f is None else f.cpu().numpy(), None if q is None else q.cpu().numpy(), None if a is None else a.cpu().numpy(), st)


def check_pair(rtc, one, generic, wants, what, exact=True, tol=0.0):
    """The two kernels' outputs and counters against each other (always to the bit) and against the oracle's frames `wants`
    (one (image, stats) per view; to the bit, or within `tol` where the reference itself is a rounded sum)."""
    for k in range(3):
        assert (one[k] is None) == (generic[k] is None), what
        if one[k] is not None:
            assert same_bits(one[k], generic[k]), (what, "one-sample kernel != generic kernel", ("f64", "u8", "rgba")[k])
    assert one[3] == generic[3], (what, one[3], generic[3])
    f, q, a, st = one
    H = wants[0][0].shape[0]
    stride = H if len(wants) == 1 and a is None else -(-H // 8) * 8
    for v, (img, _) in enumerate(wants):
        r0 = v * stride
        if f is not None:
            if exact:
                assert same_bits(f[r0:r0 + H], img), (what, v)
            else:
                err = float(np.max(np.abs(f[r0:r0 + H] - img)))
                print(f"{what} view {v}: max|gpu - oracle| = {err:.3e} (bound {tol:.1e})")
                assert err <= tol and np.array_equal(f[r0:r0 + H] != 0, img != 0), (what, v, err)
            assert bool((f[r0 + H:r0 + stride] == -1.0).all()), (what, v)   # rows past the frame stay untouched
        if q is not None and exact:
            assert np.array_equal(q[r0:r0 + H], rtc.color_scale255(img).reshape(img.shape)), (what, v)
        if a is not None and exact:
            assert np.array_equal(a[r0:r0 + H], rtc.to_rgba8(img, 2.2).reshape(H, -1, 4)) and bool((a[r0 + H:r0 + stride] == 9).all()), (what, v)
    want_st = {k: sum(s[k] for _, s in wants) for k in COUNTERS}
    assert {k: st[k] for k in COUNTERS} == want_st, (what, st, want_st)


@pytest.mark.parametrize("kind", WORLDS)
def test_frames_outputs_and_modes(rtc, ctxs, oracle, kind):
    """Every frame size, output form (the RGBA8 flavour included) and mode; rtc_render's own path too."""
    some_proven = False
    for W, H in SMALL_FRAMES + (CHUNK_FRAME,):
        w, cam = scene(rtc, kind, W, H)
        pair = ctxs["chunks" if (W, H) == CHUNK_FRAME else "binned"]
        dws = [c.upload(w) for c in pair]
        for mode in (rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER):   # (MODE_RENDER: the last row and column stay untouched)
            want = oracle.frame(kind, w, cam, mode)
            for output in ("f64", "f64+u8", "u8", "rgba"):
                what = (kind, W, H, mode, output)
                got = [launch(rtc, c, d, [cam], mode, output) for c, d in zip(pair, dws)]
                info = [c.last_launch_info() for c in pair]
                assert info[0] == info[1] and info[0]["binned_primary_pass"], (what, info)
                assert info[0]["source"] == (4 if kind.startswith("many") else 3), (what, info)
                assert (info[0]["reflective"], info[0]["refractive"]) == (kind not in MATTE, kind.endswith("glass")), (what, info)
                if (W, H) == CHUNK_FRAME:
                    assert info[0]["multi_tile_workgroups"] > 0, what
                check_pair(rtc, got[0], got[1], [want], what)
                some_proven = some_proven or got[0][3]["rays_primary_proven_miss"] > 0
            imgs = [d.render(cam, mode, with_stats=True) for d in dws]
            assert same_bits(imgs[0][0], want[0]) and same_bits(imgs[1][0], want[0]) and imgs[0][1] == imgs[1][1] == want[1], (kind, W, H, mode)
        for d in dws:
            d.close()
    assert some_proven, kind   # tiles proven black skipped the pass on their way to the one output stage


@pytest.mark.parametrize("kind", WORLDS)
def test_views_and_rows(rtc, ctxs, oracle, kind):
    """Two and three views in one launch, and row ranges from y0 = 8 and y0 = 5."""
    for (W, H), name in (((9, 17), "binned"), ((20, 12), "binned"), (CHUNK_FRAME, "chunks")):
        pair = ctxs[name]
        w, cam = scene(rtc, kind, W, H)
        cam_b = other_camera(rtc, W, H)
        dws = [c.upload(w) for c in pair]
        for order in ("ab", "bab"):
            cams = [cam if c == "a" else cam_b for c in order]
            for mode in (rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER):
                wants = [oracle.frame((kind, c), w, cm, mode) for c, cm in zip(order, cams)]
                for output in ("f64+u8", "rgba"):
                    got = [launch(rtc, c, d, cams, mode, output) for c, d in zip(pair, dws)]
                    check_pair(rtc, got[0], got[1], wants, (kind, W, H, order, mode, output))
        for y0 in (8, 5):
            if y0 >= H:
                continue
            for mode in (rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER):
                want = oracle.frame(kind, w, cam, mode, y0, H)
                got = [launch(rtc, c, d, [cam], mode, "f64+u8", y0) for c, d in zip(pair, dws)]
                check_pair(rtc, got[0], got[1], [want], (kind, W, H, "rows from", y0, mode))
        for d in dws:
            d.close()


@pytest.mark.parametrize("form", ("kernel arguments", "device table"))
@pytest.mark.parametrize("kind", WORLDS)
def test_two_lights(rtc, ctxs, oracle, kind, form):
    """Worlds with two lights through the one-sample kernel: the lights in the kernel-argument block and in the device table."""
    specs = (((-10.0, 10.0, -10.0), (1.0, 1.0, 1.0)), SECOND_LIGHT)
    lights = [rtc.light(position=p, intensity=i) for p, i in specs]
    for (W, H), name in (((9, 17), "binned"), ((20, 12), "binned"), (CHUNK_FRAME, "chunks")):
        pair = ctxs[("table " + name).replace(" binned", "") if form == "device table" else name]
        w, cam = scene(rtc, kind, W, H, lights)
        dws = [c.upload(w) for c in pair]
        for mode in (rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER):
            per_light = [oracle.frame((kind, "light", i), w, cam, mode, light=l) for i, l in enumerate(lights)]
            # the sum in light order; geometry does not depend on the light, so every light's frame casts the same rays
            want_st = dict(per_light[0][1])
            want_st["rays_shadow"] = sum(s["rays_shadow"] for _, s in per_light)
            want = (per_light[0][0] + per_light[1][0], want_st)
            for output in ("f64+u8", "rgba"):
                got = [launch(rtc, c, d, [cam], mode, output) for c, d in zip(pair, dws)]
                info = [c.last_launch_info() for c in pair]
                assert info[0] == info[1] and info[0]["light_table"] == (form == "device table"), (kind, form, info)
                check_pair(rtc, got[0], got[1], [want], (kind, form, W, H, mode, output), exact=kind in MATTE, tol=2 * TIGHT_TOL)
        for d in dws:
            d.close()


@pytest.mark.parametrize("kind", ("floor", "mirror", "many"))
def test_anti_aliased_cameras_keep_the_generic_kernel(rtc, ctxs, oracle, kind):
    """samples != 1 on frames where pixels trip the resample test (checked on the oracle first), with the resample taken and
    without: both contexts give the oracle's frame and counts. One ray per pixel — the new kernel — could not."""
    for (W, H), name in (((20, 12), "binned"), (CHUNK_FRAME, "chunks")):
        pair = ctxs[name]
        w, cam = scene(rtc, kind, W, H)
        dws = [c.upload(w) for c in pair]
        for samples, flags in ((4, 0), (3, rtc.FLAG_AA_RESAMPLE), (0, 0)):
            cam.samples = samples
            want_img, want_st = oracle.frame(kind, w, cam, rtc.MODE_RENDER_ASYNC, flags=flags)
            assert 0 < want_st["pixels_resample"] < W * H, (kind, W, H, samples)
            extra = samples if flags & rtc.FLAG_AA_RESAMPLE else 0
            assert want_st["rays_primary"] == 4 * W * H + extra * want_st["pixels_resample"]
            for d in dws:
                img, st = d.render(cam, rtc.MODE_RENDER_ASYNC, flags=flags, with_stats=True)
                assert same_bits(img, want_img) and st == want_st, (kind, W, H, samples, flags, st, want_st)
        for d in dws:
            d.close()
