"""Area lights on the HIP path (rtc_world_create_area_lights, k_trace's light-table instantiations).

An area light is its usteps x vsteps sample point lights in the multi-light semantics (include/rtc.h). Up to 8 samples
travel in the kernel arguments exactly like rtc_world_create_lights' lights; more live in a device table per World
generation, which the same light loop reads. RTC_LIGHT_TABLE=1 sends Worlds of 2..8 lights through the table kernels too:
that is the bit-exact pin of the new path against the old. Above 8 samples the reference frame is the SUM, in sample
order, of the oracle's single-light frames (color_at is linear in the light: the construction of test_gpu_lights.py),
bound n_samples x 1e-12. Frames are 70x45: partial 8x8 tiles on both edges."""
import ctypes as C
import functools
import importlib
import os
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 70, 45
TIGHT_TOL = 1e-12  # per sample (tests/test_gpu_lights.py, tests/test_gpu_parity.py): one pow per light is not bit-exact
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "pixels")
NO_CULL, LDS_TABLE = 1, 4
ERR_ARG, ERR_UNSUPPORTED = 4, 8
WORLDS = ("s5", "s40", "s300", "refl40", "mixed")  # no lists / small lists / two-level with lists / REFL / REFL + REFR

# point lights as (position, intensity); area lights as (corner, uvec, vvec, usteps, vsteps, intensity)
KEY = ((-10.0, 10.0, -10.0), (1.0, 1.0, 1.0))
AMONG = ((1.5, 1.25, 4.0), (0.2, 0.45, 0.7))
FAR = ((300.0, 400.0, -250.0), (0.55, 0.4, 0.25))
A22 = ((1.0, 1.25, 3.5), (1.0, 0.0, 0.25), (0.0, 0.5, 1.0), 2, 2, (0.2, 0.45, 0.7))          # among the shapes
A32 = ((290.0, 400.0, -260.0), (30.0, 0.0, 10.0), (0.0, 20.0, 5.0), 3, 2, (0.55, 0.4, 0.25))  # far outside every world's bounds
A33 = ((-11.5, 10.0, -11.5), (3.0, 0.0, 0.0), (0.0, 0.5, 3.0), 3, 3, (1.0, 0.95, 0.9))        # around the scenes' own light
A44 = ((-12.0, 10.0, -12.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), 4, 4, (1.0, 1.0, 1.0))
A1616 = ((-12.0, 10.0, -12.0), (4.0, 0.0, 0.0), (0.0, 1.0, 4.0), 16, 16, (1.0, 1.0, 1.0))
# (world, lights) above 8 samples: 9 is the smallest table World
TABLE_CASES = {"s5-3x3": ("s5", (A33,)), "s300-3x3": ("s300", (A33,)), "mixed-3x3": ("mixed", (A33,)),
               "refl40-point+2x2+3x2": ("refl40", (KEY, A22, A32)), "s40-4x4": ("s40", (A44,))}
POINT_SETS = {2: (FAR, AMONG), 3: (KEY, AMONG, FAR), 8: (KEY, AMONG, FAR, ((4.0, 6.0, -3.0), (0.1, 0.1, 0.1)), ((-3.0, 2.0, 1.0), (0.05, 0.1, 0.02)),
                                                         ((0.0, 12.0, 6.0), (0.2, 0.2, 0.25)), ((7.0, 0.75, 2.0), (0.1, 0.02, 0.02)),
                                                         ((-40.0, 30.0, 20.0), (0.15, 0.15, 0.1)))}


def _scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


@functools.lru_cache(maxsize=None)
def _scene(rtc, name):
    S = _scenes(rtc)
    if name == "s5": return S.synthetic(4, W, H)
    if name == "s40": return S.synthetic(39, W, H)
    if name == "s300": return S.synthetic(299, W, H)
    if name == "refl40": return S.synthetic(39, W, H, reflective=True)
    if name == "mixed": return S.mixed(W, H)
    raise KeyError(name)


def _light(rtc, spec):
    return rtc.light(position=spec[0], intensity=spec[1]) if len(spec) == 2 else rtc.area_light(*spec)


def _world(rtc, name, specs):
    w, cam = _scene(rtc, name)
    m = rtc.World([_light(rtc, s) for s in specs])
    m.shapes = w.shapes
    return m, cam


def _sample_specs(rtc, specs):
    """The expanded sample list as hashable (position, intensity) pairs (rtc_area_light_expand)."""
    return tuple((tuple(s.position), tuple(s.intensity)) for s in rtc.World([_light(rtc, s) for s in specs]).samples())


@functools.lru_cache(maxsize=None)
def _oracle_frame(rtc, O, name, sample):
    """The oracle's single-light frame of world `name` under one sample: computed once, shared, never written to."""
    w, cam = _scene(rtc, name)
    out = O.render(w.array(), len(w), rtc.light(position=sample[0], intensity=sample[1]), cam, mode=1, nthreads=8)
    out.setflags(write=False)
    return out


def _oracle_sum(rtc, O, name, samples):
    ref = _oracle_frame(rtc, O, name, samples[0])
    for s in samples[1:]:
        ref = ref + _oracle_frame(rtc, O, name, s)   # in sample order
    return ref


def _render(gpu, world, cam, flags=0):
    """(canvas, stats, light_table of the launch)"""
    dw = gpu.upload(world)
    try:
        got, st = dw.render(cam, flags=flags, with_stats=True)
        return got, st, gpu.last_launch_info()["light_table"]
    finally:
        dw.close()


def _ctx_env(rtc, **env):
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ[k] = str(v)
        return rtc.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def table_ctx(rtc):
    ctx = _ctx_env(rtc, RTC_LIGHT_TABLE=1)
    yield ctx
    ctx.close()


# ---- 1
@pytest.mark.parametrize("name", ["s40", "mixed"])
def test_up_to_eight_samples_is_the_multi_light_world(rtc, gpu, name):
    area, cam = _world(rtc, name, (KEY, A22))
    assert area.needs_area_entries() and len(area.samples()) == 5
    expanded = rtc.World(area.samples())   # five RtcLight: rtc_world_create_lights
    expanded.shapes = area.shapes
    assert not expanded.needs_area_entries()
    dw = gpu.upload(area)
    assert rtc.lib().rtc_world_light_count(dw._h) == 5
    dw.close()
    for flags in (0, NO_CULL):
        a, sa, ta = _render(gpu, area, cam, flags)
        b, sb, tb = _render(gpu, expanded, cam, flags)
        assert a.tobytes() == b.tobytes() and sa == sb and a.any() and ta is False and tb is False


# ---- 2
@pytest.mark.parametrize("flags", [0, NO_CULL], ids=["culled", "no_cull"])
@pytest.mark.parametrize("n_lights", [2, 3, 8])
@pytest.mark.parametrize("name", WORLDS)
def test_the_table_kernels_are_the_kernarg_kernels(rtc, gpu, table_ctx, name, n_lights, flags):
    m, cam = _world(rtc, name, POINT_SETS[n_lights])
    a, sa, ta = _render(gpu, m, cam, flags)
    b, sb, tb = _render(table_ctx, m, cam, flags)
    assert ta is False and tb is True
    assert a.tobytes() == b.tobytes() and sa == sb and a.any()


def _hit_record(h):
    """Every field of an rtc_hit that is defined: a miss has its index alone."""
    if h.hit_index < 0:
        return (h.hit_index,)
    vecs = tuple(tuple(getattr(h, k)) for k in ("point", "over_point", "under_point", "eyev", "normal", "reflectv"))
    return (h.hit_index, h.inside, h.shadowed, h.t, h.n1, h.n2) + vecs


def test_the_table_kernels_rgba8_and_color_at(rtc, gpu, table_ctx):
    m, cam = _world(rtc, "mixed", POINT_SETS[3])
    rays = np.array([rtc.ray_for_pixel(cam, x, y) for x, y in ((5, 40), (20, 30), (35, 22), (50, 35), (64, 44), (33, 28), (12, 25), (60, 20))])
    got = []
    for ctx in (gpu, table_ctx):
        dw = ctx.upload(m)
        try:
            rgba = dw.render_rgba8(cam, gamma=2.2)
            table = ctx.last_launch_info()["light_table"]
            per_flags = []
            for flags in (0, NO_CULL):
                rgb, hits = dw.color_at(rays, remaining=5, want_hits=True, flags=flags)
                per_flags.append((rgb.tobytes(), [_hit_record(h) for h in hits]))
            got.append((rgba.tobytes(), table, per_flags))
        finally:
            dw.close()
    assert got[0][1] is False and got[1][1] is True
    assert got[0][0] == got[1][0] and got[0][2] == got[1][2]
    rgb = np.frombuffer(got[0][2][0][0], dtype=np.float64).reshape(-1, 3)
    assert int(np.count_nonzero(rgb.any(axis=1))) >= 4 and got[0][2][0] == got[0][2][1]   # culled == brute force, hit records included


# ---- 3, 4, 5
def _check_linear(got, ref, n_samples, what):
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max|gpu - sum(oracle_i)| = {err:.3e} (bound {n_samples * TIGHT_TOL:.1e})")
    assert err <= n_samples * TIGHT_TOL, (what, err)
    assert np.array_equal(got != 0, ref != 0), what


@pytest.mark.parametrize("case", list(TABLE_CASES))
def test_above_eight_samples_frames_are_the_sum_of_the_oracles_single_light_frames(rtc, gpu, O, case):
    name, specs = TABLE_CASES[case]
    samples = _sample_specs(rtc, specs)
    n = len(samples)
    assert n > 8
    m, cam = _world(rtc, name, specs)
    got, st, table = _render(gpu, m, cam)
    brute, sb, table_b = _render(gpu, m, cam, NO_CULL)
    assert table is True and table_b is True
    # culled == brute force, stats included
    assert brute.tobytes() == got.tobytes() and all(st[k] == sb[k] for k in COUNTERS)
    ref = _oracle_sum(rtc, O, name, samples)
    _check_linear(got, ref, n, f"{case} ({n} samples)")
    # counters: one shadow ray per sample per shade_hit, everything else as for one light
    w, _ = _scene(rtc, name)
    _, o1 = O.render(w.array(), len(w), rtc.light(position=samples[0][0], intensity=samples[0][1]), cam, mode=1, want_stats=True, nthreads=8)
    assert st["rays_shadow"] == n * o1["rays_shadow"] and o1["rays_shadow"] > 0
    assert all(st[k] == o1[k] for k in COUNTERS if k != "rays_shadow")


def test_the_cap_of_256_samples_culled_equals_brute_force(rtc, gpu):
    m, cam = _world(rtc, "s5", (A1616,))
    assert len(m.samples()) == 256
    one, s1, _ = _render(gpu, _world(rtc, "s5", (KEY,))[0], cam)
    got, st, table = _render(gpu, m, cam)
    brute, sb, _ = _render(gpu, m, cam, NO_CULL)
    assert table is True and got.tobytes() == brute.tobytes() and all(st[k] == sb[k] for k in COUNTERS) and got.any()
    assert st["rays_shadow"] == 256 * s1["rays_shadow"] and all(st[k] == s1[k] for k in COUNTERS if k != "rays_shadow")
    dw = gpu.upload(m)
    assert rtc.lib().rtc_world_light_count(dw._h) == 256
    dw.close()


# ---- 6
def test_update_area_lights_on_a_resident_world(rtc, gpu):
    """1 light -> 3x3 -> [point, 2x2] -> 4x4 with renders in between: each frame is the freshly created World's."""
    name = "s40"
    steps = [((KEY,), 1, False), ((A33,), 9, True), ((KEY, A22), 5, False), ((A44,), 16, True), ((KEY,), 1, False)]
    fresh = [_render(gpu, _world(rtc, name, specs)[0], _scene(rtc, name)[1]) for specs, _, _ in steps]
    assert len({f[0].tobytes() for f in fresh[:4]}) == 4
    first, cam = _world(rtc, name, steps[0][0])
    dw = gpu.upload(first)
    try:
        for (specs, n, table), want in zip(steps, fresh):
            dw.update(_world(rtc, name, specs)[0])
            assert rtc.lib().rtc_world_light_count(dw._h) == n
            for _ in range(2):   # a render between the updates, and one more on the same generation
                got, st = dw.render(cam, with_stats=True)
                assert gpu.last_launch_info()["light_table"] is table
                assert got.tobytes() == want[0].tobytes() and st == want[1], n
        # rejected calls leave the World as it was
        w = _world(rtc, name, (A1616, KEY))[0]
        assert rtc.lib().rtc_world_update_area_lights(gpu._h, dw._h, w.array(), len(w), w.area_light_array(), 2) == ERR_ARG
        assert rtc.lib().rtc_world_update_area_lights(gpu._h, dw._h, w.array(), len(w), w.area_light_array(), 0) == ERR_ARG
        assert rtc.lib().rtc_world_light_count(dw._h) == 1 and dw.render(cam).tobytes() == fresh[0][0].tobytes()
    finally:
        dw.close()


# ---- 7
FLOOR_LIGHT = ((-1.5, 6.0, -1.5), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0), 3, 3, (1.0, 1.0, 1.0))


def test_a_penumbra_exists(rtc, gpu, O):
    """A sphere over a floor under a 3x3 light. From the oracle's hit records, floor pixels that some samples shadow and
    others do not; there the GPU colour lies strictly between the all-shadowed sum (every sample's ambient term: what the
    oracle returns for a shadowed sample) and the all-lit sum (the oracle's colours of the floor alone)."""
    floor = rtc.plane(rtc.Matrix.identity(), rtc.material(color=(0.8, 0.8, 0.8), specular=0.0))
    w = rtc.World(rtc.area_light(*FLOOR_LIGHT))
    w.add_shape(floor)
    w.add_shape(rtc.sphere(rtc.Matrix.identity().translation(0.0, 1.5, 0.0), rtc.material(color=(0.9, 0.2, 0.2))))
    bare = rtc.World(rtc.area_light(*FLOOR_LIGHT))
    bare.add_shape(floor)
    cam = rtc.camera(W, H, 0.9, rtc.Matrix.make_view_transform((0.0, 5.0, -8.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0)))
    samples = w.samples()
    assert len(samples) == 9
    dw = gpu.upload(w)
    try:
        got = dw.render(cam)
        assert gpu.last_launch_info()["light_table"] is True
    finally:
        dw.close()
    partial = 0
    for y in range(0, H, 2):
        for x in range(0, W, 2):
            ray = rtc.ray_for_pixel(cam, x, y)
            first = O.color_at(w.array(), len(w), samples[0], ray, want_hit=True)
            if first[1].hit_index != 0:   # not the floor
                continue
            recs = [first] + [O.color_at(w.array(), len(w), s, ray, want_hit=True) for s in samples[1:]]
            n_shadowed = sum(bool(h.shadowed) for _, h in recs)
            if n_shadowed in (0, len(samples)):
                continue
            partial += 1
            all_shadowed, all_lit = np.zeros(3), np.zeros(3)
            ambient = next(np.asarray(c) for c, h in recs if h.shadowed)   # the same for every sample: equal intensities
            for s in samples:
                all_shadowed = all_shadowed + ambient
                all_lit = all_lit + np.asarray(O.color_at(bare.array(), len(bare), s, ray, want_hit=True)[0])
            assert np.all(got[y, x] > all_shadowed) and np.all(got[y, x] < all_lit), (x, y, n_shadowed, got[y, x], all_shadowed, all_lit)
    print(f"penumbra pixels (of every other pixel): {partial}")
    assert partial >= 1


# ---- 8
def test_soft_shadows_scene_file_renders_like_the_world_built_by_hand(rtc, gpu):
    data = Path(rtc.__file__).resolve().parent / "data"
    loaded, _ = rtc.load_yaml(path=data / "soft_shadows.yml")
    M = rtc.Matrix.identity
    hand = rtc.World([rtc.area_light((-3, 6, -5), (2, 0, 0), (0, 0.5, 2), 4, 4, (1.2, 1.15, 1.05)),
                      rtc.light(position=(6, 1.5, -4), intensity=(0.1, 0.13, 0.2))])
    hand.add_shape(rtc.plane(M(), rtc.material(specular=0.0, pattern=("checkers", (0.4, 0.4, 0.4), (0.7, 0.7, 0.7), None))))
    hand.add_shape(rtc.sphere(M().translation(-1.5, 1, 0.5), rtc.material(color=(0.85, 0.25, 0.2), diffuse=0.7, specular=0.6, shininess=120)))
    hand.add_shape(rtc.sphere(M().scaling(0.6, 0.6, 0.6).translation(0.6, 0.6, -1.4), rtc.material(color=(0.2, 0.35, 0.8), diffuse=0.8, specular=0.4)))
    hand.add_shape(rtc.sphere(M().scaling(0.35, 0.35, 0.35).translation(-0.4, 0.35, -2.2), rtc.material(color=(0.9, 0.8, 0.25), specular=0.2)))
    hand.add_shape(rtc.cube(M().scaling(0.5, 0.5, 0.5).rotation_y(0.6).translation(2.3, 0.5, 1.2), rtc.material(color=(0.25, 0.6, 0.35), diffuse=0.8, specular=0.2)))
    cam = rtc.camera(W, H, 0.9, rtc.Matrix.make_view_transform((0, 2.6, -7.5), (0, 0.8, 0), (0, 1, 0)))
    a, sa, ta = _render(gpu, loaded, cam)
    b, sb, tb = _render(gpu, hand, cam)
    assert ta is True and tb is True and sa == sb and a.tobytes() == b.tobytes() and a.any()
    point_only = rtc.World(hand.lights[1])
    point_only.shapes = hand.shapes
    assert sa["rays_shadow"] == 17 * _render(gpu, point_only, cam)[1]["rays_shadow"]
    # the Lua twin renders through rtc_lua_program_render with its full light list
    prog = rtc.LuaProgram(path=data / "soft_shadows.lua")
    try:
        job = prog.jobs[0]
        assert len(job.world.samples()) == 17
        small = "WIDTH, HEIGHT = 70, 45\n" + (data / "soft_shadows.lua").read_text().replace("screenwidth = 320, screenheight = 200", "screenwidth = WIDTH, screenheight = HEIGHT")
    finally:
        prog.close()
    prog = rtc.LuaProgram(text=small)
    try:
        frames = prog.render(gpu)
        job = prog.jobs[0]
        dw = gpu.upload(job.world)
        want = dw.render_rgb8(job.camera)
        dw.close()
        assert len(frames) == 1 and np.array_equal(np.asarray(frames[0]).reshape(-1), want.reshape(-1)) and want.any()
        assert gpu.last_launch_info()["light_table"] is True
    finally:
        prog.close()


# ---- 9
def test_arguments(rtc, gpu):
    L = rtc.lib()
    w, cam = _world(rtc, "s40", (A33,))
    h = C.c_void_p()
    assert L.rtc_world_create_area_lights(gpu._h, w.array(), len(w), w.area_light_array(), 0, C.byref(h)) == ERR_ARG and not h
    assert L.rtc_world_create_area_lights(gpu._h, w.array(), len(w), None, 1, C.byref(h)) == ERR_ARG and not h
    over = _world(rtc, "s40", (A1616, KEY))[0]   # 257 samples
    assert L.rtc_world_create_area_lights(gpu._h, over.array(), len(over), over.area_light_array(), 2, C.byref(h)) == ERR_ARG and not h
    zero = _world(rtc, "s40", (((0, 5, 0), (1, 0, 0), (0, 0, 1), 0, 3, (1, 1, 1)),))[0]   # no sample at all
    assert L.rtc_world_create_area_lights(gpu._h, zero.array(), len(zero), zero.area_light_array(), 1, C.byref(h)) == ERR_ARG and not h
    dw = gpu.upload(w)
    try:
        f64 = dw.render(cam)
        with pytest.raises(rtc.RtcError) as e:
            dw.render(cam, flags=NO_CULL | LDS_TABLE)   # RTC_FLAG_LDS_TABLE: a measurement-only path without multi-light kernels
        assert e.value.status == ERR_UNSUPPORTED
        # the 8-bit entries and rtc_render_views take the World unchanged
        import torch
        assert np.array_equal(dw.render_rgb8(cam), rtc.color_scale255(f64).reshape(H, W, 3))
        assert np.array_equal(dw.render_rgba8(cam, gamma=2.2), rtc.to_rgba8(f64, 2.2))
        rows = 48
        buf = torch.zeros((2 * rows, W, 3), dtype=torch.float64, device="cuda:0")
        dw.render_views([cam, cam], 0, 1, buf.data_ptr(), rows)
        gpu.synchronize()
        host = buf.cpu().numpy()
        assert host[:H].tobytes() == f64.tobytes() and host[rows:rows + H].tobytes() == f64.tobytes()
    finally:
        dw.close()


def test_facade_add_area_light(rtc):
    """tests/cpp/test_facade_area_light.cpp: ch1::World::add_area_light renders what rtc_world_create_area_lights renders,
    and adding or dropping an area light updates the resident World in place."""
    import importlib.util
    import subprocess
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("_rtc_build", root / "raytracer-challenge_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = b.build_facade_area_light_test()
    assert exe is not None and exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade area light: ok" in r.stdout
