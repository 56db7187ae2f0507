"""Worlds with several lights on the HIP path (rtc_world_create_lights, k_trace's multi-light instantiations).

shade_hit sums lighting() over the lights, each with its own shadow test. The reference stops at its first light (`FIXME --
multiple lights`, shape.rs:686), so the reference frame here is the SUM, in light order, of the oracle's single-light
frames of the same world: color_at is linear in the light (geometry, recursion depth and Schlick weights do not depend on
it). Frames are 70x45: partial 8x8 tiles on both edges."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 70, 45
TIGHT_TOL = 1e-12  # the bar of tests/test_gpu_parity.py: per light one pow, the only operation that is not bit-exact
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "pixels")
NO_CULL = 1

# (position, intensity): KEY is the scenes' own light; AMONG sits between the shapes; FAR lies far outside every world's bounds
KEY = ((-10.0, 10.0, -10.0), (1.0, 1.0, 1.0))
AMONG = ((1.5, 1.25, 4.0), (0.2, 0.45, 0.7))
FAR = ((300.0, 400.0, -250.0), (0.55, 0.4, 0.25))
LIGHT_SETS = {2: (FAR, AMONG), 3: (KEY, AMONG, FAR)}
WORLDS = ("s5", "s40", "s300", "refl40", "mixed")  # no lists / small lists / two-level with lists / REFL / REFL + REFR


def _scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


@functools.lru_cache(maxsize=None)
def _scene(rtc, name):
    """(World, camera) at 70x45; the World's own light is left alone (callers pass lights explicitly)."""
    S = _scenes(rtc)
    if name == "s5": return S.synthetic(4, W, H)
    if name == "s40": return S.synthetic(39, W, H)
    if name == "s300": return S.synthetic(299, W, H)
    if name == "refl40": return S.synthetic(39, W, H, reflective=True)
    if name == "mixed": return S.mixed(W, H)
    raise KeyError(name)


def _lights(rtc, spec):
    return [rtc.light(position=p, intensity=i) for p, i in spec]


def _with_lights(rtc, name, lights):
    w, cam = _scene(rtc, name)
    m = rtc.World(lights)
    m.shapes = w.shapes
    return m, cam


@functools.lru_cache(maxsize=None)
def _oracle_frame(rtc, O, name, spec, samples=1):
    """The oracle's single-light frame of world `name` under light `spec`: computed once, shared, never written to."""
    w, cam = _scene(rtc, name)
    c = rtc.RtcCamera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(rtc.RtcCamera))
    c.samples = samples
    out = O.render(w.array(), len(w), rtc.light(position=spec[0], intensity=spec[1]), c, mode=1, nthreads=8)
    out.setflags(write=False)
    return out


def _oracle_sum(rtc, O, name, specs, samples=1):
    ref = _oracle_frame(rtc, O, name, specs[0], samples)
    for s in specs[1:]:
        ref = ref + _oracle_frame(rtc, O, name, s, samples)   # in light order
    return ref


def _render(rtc, gpu, world, cam, flags=0):
    dw = gpu.upload(world)
    try:
        return dw.render(cam, rtc.MODE_RENDER_ASYNC, flags=flags, with_stats=True)
    finally:
        dw.close()


def _check_linear(got, ref, n_lights, what):
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max|gpu - sum(oracle_i)| = {err:.3e} (bound {n_lights * TIGHT_TOL:.1e})")
    assert err <= n_lights * TIGHT_TOL, (what, err)
    assert np.array_equal(got != 0, ref != 0), what


@pytest.mark.parametrize("name", ["s5", "s40", "s300"])
def test_one_light_through_create_lights_is_the_one_light_world(rtc, gpu, name):
    """rtc_world_create_lights(.., 1) and rtc_world_create: the same canvas bytes and the same rtc_stats, in the three
    regimes (no lists, small lists, two-level with lists)."""
    w, cam = _scene(rtc, name)
    via_lights = gpu.upload(w)   # DeviceWorld creates with rtc_world_create_lights
    h = C.c_void_p()
    assert rtc.lib().rtc_world_create(gpu._h, w.array(), len(w), C.byref(w.light), C.byref(h)) == 0
    try:
        assert rtc.lib().rtc_world_light_count(via_lights._h) == 1 == rtc.lib().rtc_world_light_count(h)
        a, sa = via_lights.render(cam, with_stats=True)
        keep, via_lights._h = via_lights._h, h   # the same binding, the other handle
        b, sb = via_lights.render(cam, with_stats=True)
        via_lights._h = keep
        assert a.tobytes() == b.tobytes() and sa == sb and a.any()
    finally:
        rtc.lib().rtc_world_destroy(h)
        via_lights.close()


@pytest.mark.parametrize("name", ["s40", "mixed"])
def test_black_second_light_changes_only_the_shadow_ray_count(rtc, gpu, name):
    w, cam = _scene(rtc, name)
    one, s1 = _render(rtc, gpu, w, cam)
    m, _ = _with_lights(rtc, name, [w.light, rtc.light(position=AMONG[0], intensity=(0.0, 0.0, 0.0))])
    two, s2 = _render(rtc, gpu, m, cam)
    assert np.array_equal(two, one)   # == on f64: -0 == 0
    assert s2["rays_shadow"] == 2 * s1["rays_shadow"] and s1["rays_shadow"] > 0
    assert all(s2[k] == s1[k] for k in COUNTERS if k != "rays_shadow")


@pytest.mark.parametrize("name", ["s300", "refl40", "mixed"])
def test_the_same_light_twice_doubles_the_frame_exactly(rtc, gpu, name):
    """s + s and every later scaling by 2 are exact: the frame is 2x the one-light frame bit for bit, through the
    reflection-only (refl40) and the reflection + refraction (mixed) frame-stack kernels too."""
    w, cam = _scene(rtc, name)
    one, s1 = _render(rtc, gpu, w, cam)
    m, _ = _with_lights(rtc, name, [w.light, w.light])
    two, s2 = _render(rtc, gpu, m, cam)
    assert two.tobytes() == (2.0 * one).tobytes() and one.any()
    assert s2["rays_shadow"] == 2 * s1["rays_shadow"] and s2["rays_reflect"] == s1["rays_reflect"] and s2["rays_refract"] == s1["rays_refract"]
    if name != "s300":
        assert s1["rays_reflect"] > 0
    if name == "mixed":
        assert s1["rays_refract"] > 0


@functools.lru_cache(maxsize=None)
def _separated(rtc, O, name, a, b):
    """From the oracle's hit records alone: (hit pixels shadowed from a only, from b only)."""
    w, cam = _scene(rtc, name)
    la, lb = rtc.light(position=a[0], intensity=a[1]), rtc.light(position=b[0], intensity=b[1])
    arr, n = w.array(), len(w)
    only_a = only_b = 0
    for y in range(0, H, 2):
        for x in range(0, W, 2):
            ray = rtc.ray_for_pixel(cam, x, y)
            _, ha = O.color_at(arr, n, la, ray, want_hit=True)
            if ha.hit_index < 0:
                continue
            _, hb = O.color_at(arr, n, lb, ray, want_hit=True)
            only_a += bool(ha.shadowed) and not hb.shadowed
            only_b += bool(hb.shadowed) and not ha.shadowed
    return only_a, only_b


@pytest.mark.parametrize("n_lights", [2, 3])
@pytest.mark.parametrize("name", WORLDS)
def test_frames_are_the_sum_of_the_oracles_single_light_frames(rtc, gpu, O, name, n_lights):
    specs = LIGHT_SETS[n_lights]
    only_a, only_b = _separated(rtc, O, name, specs[0], specs[1])
    assert only_a > 0 and only_b > 0, ("the scene does not separate the lights", only_a, only_b)
    ref = _oracle_sum(rtc, O, name, specs)
    m, cam = _with_lights(rtc, name, _lights(rtc, specs))
    got, st = _render(rtc, gpu, m, cam)
    _check_linear(got, ref, n_lights, f"{name} x{n_lights}")
    brute, sb = _render(rtc, gpu, m, cam, flags=NO_CULL)
    _check_linear(brute, ref, n_lights, f"{name} x{n_lights} NO_CULL")
    assert brute.tobytes() == got.tobytes()
    assert all(st[k] == sb[k] for k in COUNTERS)
    w, _ = _scene(rtc, name)
    _, o1 = O.render(w.array(), len(w), m.lights[0], cam, mode=1, want_stats=True, nthreads=8)
    assert st["rays_shadow"] == n_lights * o1["rays_shadow"] and all(st[k] == o1[k] for k in COUNTERS if k != "rays_shadow")


@pytest.mark.parametrize("name", ["s40", "mixed"])
def test_four_sample_frames_are_linear_too(rtc, gpu, O, name):
    """samples == 4 without RTC_FLAG_AA_RESAMPLE: the mean of the four sub-samples is linear in the lights."""
    specs = LIGHT_SETS[3]
    ref = _oracle_sum(rtc, O, name, specs, samples=4)
    m, cam = _with_lights(rtc, name, _lights(rtc, specs))
    c = rtc.RtcCamera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(rtc.RtcCamera))
    c.samples = 4
    got, _ = _render(rtc, gpu, m, c)
    _check_linear(got, ref, 3, f"{name} x3 samples=4")


@pytest.mark.parametrize("name", ["s40", "s300", "mixed"])
def test_color_at_sums_the_lights_and_reports_the_first_lights_shadow(rtc, gpu, O, name):
    specs = LIGHT_SETS[3]
    m, cam = _with_lights(rtc, name, _lights(rtc, specs))
    rays = np.array([rtc.ray_for_pixel(cam, x, y) for x, y in ((5, 40), (20, 30), (35, 22), (50, 35), (64, 44), (33, 28), (12, 25), (60, 20))])
    dw = gpu.upload(m)
    try:
        for flags in (0, NO_CULL):
            rgb, hits = dw.color_at(rays, remaining=5, want_hits=True, flags=flags)
            n_hit = 0
            for i, ray in enumerate(rays):
                want = np.zeros(3)
                first = None
                for k, l in enumerate(m.lights):
                    c, h = O.color_at(m.array(), len(m), l, ray, want_hit=True)
                    want = c if k == 0 else want + c
                    first = h if k == 0 else first
                assert np.max(np.abs(rgb[i] - want)) <= 3 * TIGHT_TOL and np.array_equal(rgb[i] != 0, want != 0), (name, i)
                assert hits[i].hit_index == first.hit_index and hits[i].shadowed == first.shadowed, (name, i)
                n_hit += first.hit_index >= 0
            assert n_hit >= 4
    finally:
        dw.close()


def test_update_lights_changes_the_light_count_of_a_resident_world(rtc, gpu):
    """1 -> 2 -> 1 lights on a resident World: at each step the bytes and counters of a freshly created World."""
    name = "s40"
    w, cam = _scene(rtc, name)
    two, _ = _with_lights(rtc, name, _lights(rtc, LIGHT_SETS[2]))
    fresh = {1: _render(rtc, gpu, w, cam), 2: _render(rtc, gpu, two, cam)}
    assert fresh[1][0].tobytes() != fresh[2][0].tobytes()
    dw = gpu.upload(w)
    try:
        for world, n in ((two, 2), (w, 1), (two, 2)):
            dw.update(world)
            assert rtc.lib().rtc_world_light_count(dw._h) == n
            got, st = dw.render(cam, with_stats=True)
            assert got.tobytes() == fresh[n][0].tobytes() and st == fresh[n][1], n
        # rejected calls leave the World as it was
        assert rtc.lib().rtc_world_update_lights(gpu._h, dw._h, w.array(), len(w), w.light_array(), 0) == 4
        assert rtc.lib().rtc_world_update_lights(gpu._h, dw._h, w.array(), len(w), w.light_array(), 9) == 4
        assert rtc.lib().rtc_world_light_count(dw._h) == 2
        assert dw.render(cam).tobytes() == fresh[2][0].tobytes()
    finally:
        dw.close()
    h = C.c_void_p()
    for n in (0, 9):
        assert rtc.lib().rtc_world_create_lights(gpu._h, w.array(), len(w), w.light_array(), n, C.byref(h)) == 4 and not h


def test_every_render_entry_takes_a_multi_light_world(rtc, gpu):
    """The 8-bit entries and rtc_render_views render the same pixels as rtc_render; RTC_FLAG_LDS_TABLE is refused."""
    import torch
    m, cam = _with_lights(rtc, "s40", _lights(rtc, LIGHT_SETS[3]))
    dw = gpu.upload(m)
    try:
        f64 = dw.render(cam)
        assert np.array_equal(dw.render_rgb8(cam), rtc.color_scale255(f64).reshape(H, W, 3))
        assert np.array_equal(dw.render_rgba8(cam, gamma=2.2), rtc.to_rgba8(f64, 2.2))
        rows = 48
        buf = torch.zeros((2 * rows, W, 3), dtype=torch.float64, device="cuda:0")
        dw.render_views([cam, cam], 0, 1, buf.data_ptr(), rows)
        gpu.synchronize()
        host = buf.cpu().numpy()
        assert host[:H].tobytes() == f64.tobytes() and host[rows:rows + H].tobytes() == f64.tobytes()
        with pytest.raises(rtc.RtcError) as e:
            dw.render(cam, flags=NO_CULL | 4)   # RTC_FLAG_LDS_TABLE: a measurement-only path without multi-light kernels
        assert e.value.status == 8              # RTC_ERR_UNSUPPORTED
    finally:
        dw.close()


def test_lua_render_uses_every_light_of_the_script(rtc, gpu):
    text = """
local L = { { color = { r = 1, g = 0.9, b = 0.8 }, position = { x = -6, y = 8.5, z = -4 } },
            { color = { r = 0.2, g = 0.3, b = 0.6 }, position = { x = 4, y = 1.5, z = -3 } } }
local W = { lights = L, shapes = {
   { type = "plane", material = { specular = 0, reflectiveness = 0.2, pattern = { type = "checks", scale = 0.5,
                                  color_a = { r = 0.3, g = 0.3, b = 0.3 }, color_b = { r = 0.7, g = 0.7, b = 0.7 } } } },
   { type = "sphere", position = { x = -1, y = 1, z = 0 }, color = { r = 0.9, g = 0.2, b = 0.2 } },
   { type = "cube", position = { x = 1.5, y = 0.5, z = 1 }, scale = 0.5, color = { r = 0.2, g = 0.7, b = 0.3 } } } }
local C = { screenwidth = 70, screenheight = 45, fov = 1.0,
            position = { x = 0, y = 2.5, z = -7 }, lookat = { x = 0, y = 0.8, z = 0 }, up = { x = 0, y = 1, z = 0 } }
Render(W, C, "a.ppm")
L[2].position.x = -4
Render(W, C, "b.ppm")
"""
    prog = rtc.LuaProgram(text=text)
    try:
        frames = prog.render(gpu)
        jobs = prog.jobs
        assert len(frames) == 2 and [len(j.lights) for j in jobs] == [2, 2] and not jobs[1].same_world_as_previous
        want = []
        for j in jobs:
            dw = gpu.upload(j.world)   # created directly with the job's lights
            want.append(dw.render_rgb8(j.camera))
            one = rtc.World(j.lights[0])
            one.shapes = j.world.shapes
            dw1 = gpu.upload(one)
            assert not np.array_equal(dw1.render_rgb8(j.camera), want[-1])   # the second light shows
            dw.close()
            dw1.close()
        for f, q in zip(frames, want):
            assert np.array_equal(np.asarray(f).reshape(-1), q.reshape(-1))
        assert not np.array_equal(want[0], want[1])   # the update carried the moved second light
    finally:
        prog.close()
