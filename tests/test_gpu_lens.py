"""The thin-lens camera on the HIP path (rtc_render_lens*, k_trace's lens instantiations).

A thin-lens pixel is Color::average_over of usteps x vsteps ordinary rays (include/rtc.h), so the reference frame is built
here, pixel by pixel, from the oracle's color_at of rtc_lens_ray's rays: sums from 0.0 in sample order, one division by n.
Bound 1e-12 per light (the project's TIGHT_TOL: the mean of n colours each within 1e-12 is within 1e-12, and both sides add
in the same order). Frames are 70x45: partial 8x8 tiles on both edges.

Worlds. `scenes.mixed` is the small mixed world; it has reflective and transparent shapes, so it runs the frame-stack
kernel, not the flat one. The flat kernel's cases (2x2, 3x2, 16x16) therefore run on the flat 39-sphere world of the
area-light tests (one-level cull), and the mixed world is checked at 2x2 and 3x2 as well, beside scenes.criterion."""
import ctypes as C
import functools
import importlib
from pathlib import Path

import numpy as np
import pytest

from adversarial_worlds import oracle_lens_frame

pytestmark = pytest.mark.gpu

W, H = 70, 45
TIGHT_TOL = 1e-12  # per light (tests/test_gpu_lights.py, tests/test_gpu_parity.py)
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "pixels")
NO_CULL, AA_RESAMPLE, LDS_TABLE = 1, 2, 4
ERR_ARG, ERR_UNSUPPORTED = 4, 8
MODE_RENDER, MODE_RENDER_ASYNC = 0, 1
# (aperture, focal_distance, usteps, vsteps): the scenes' shapes lie 5 .. 25 units from their cameras
L22 = (0.3, 9.0, 2, 2)
L32 = (0.9, 5.0, 3, 2)      # strongly defocused: the sample order shows
L1616 = (0.4, 8.0, 16, 16)  # the cap of 256 samples
PINHOLE = (0.0, 1.0, 1, 1)
AMONG = ((1.5, 1.25, 4.0), (0.2, 0.45, 0.7))
A33 = ((-11.5, 10.0, -11.5), (3.0, 0.0, 0.0), (0.0, 0.5, 3.0), 3, 3, (1.0, 0.95, 0.9))


def _scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


@functools.lru_cache(maxsize=None)
def _scene(rtc, name):
    S = _scenes(rtc)
    if name == "flat": return S.synthetic(39, W, H)
    if name == "mixed": return S.mixed(W, H)
    if name == "criterion": return S.criterion(W, H)
    if name == "s300": return S.synthetic(299, 40, 24)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle_lens_frame(rtc, O, name, lens_spec, light_spec=None, u_outer=False, mode=MODE_RENDER_ASYNC):
    """Color::average_over of the oracle's color_at(rtc_lens_ray(x, y, k)), k in sample order (u_outer: in the WRONG, u-outer
    order). light_spec: (position, intensity) instead of the scene's own light. Computed once, shared, never written to."""
    w, cam = _scene(rtc, name)
    light = w.light if light_spec is None else rtc.light(position=light_spec[0], intensity=light_spec[1])
    return oracle_lens_frame(rtc, O, w.array(), len(w), light, cam, lens_spec, u_outer=u_outer, mode=mode)


def _lens_render(gpu, rtc, world, cam, lens_spec, flags=0, mode=MODE_RENDER_ASYNC):
    """(canvas, stats, launch info)"""
    dw = gpu.upload(world)
    try:
        got, st = dw.render_lens(cam, rtc.lens(*lens_spec), mode=mode, flags=flags, with_stats=True)
        return got, st, gpu.last_launch_info()
    finally:
        dw.close()


def _check(got, ref, n_lights, what):
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max|gpu - oracle| = {err:.3e} (bound {n_lights * TIGHT_TOL:.1e})")
    assert err <= n_lights * TIGHT_TOL, (what, err)
    assert np.array_equal(got != 0, ref != 0), what


def _culled_and_brute(gpu, rtc, name, lens_spec, source):
    """The culled frame, after checking that the RTC_FLAG_NO_CULL frame and its stats are the same bytes."""
    w, cam = _scene(rtc, name)
    n = lens_spec[2] * lens_spec[3]
    got, st, info = _lens_render(gpu, rtc, w, cam, lens_spec)
    brute, sb, info_b = _lens_render(gpu, rtc, w, cam, lens_spec, NO_CULL)
    assert info["source"] == source and info_b["source"] == 0, (info, info_b)
    assert got.tobytes() == brute.tobytes() and st == sb and got.any()
    for i in (info, info_b):
        assert i["lens_samples"] == n and i["binned_primary_pass"] is False and i["multi_tile_workgroups"] == 0
    assert st["rays_primary"] == cam.hsize * cam.vsize * n and st["pixels"] == cam.hsize * cam.vsize
    assert st["rays_primary_proven_miss"] == 0 and st["rays_shadow"] > 0
    return got, st, info


# ---- oracle parity
@pytest.mark.parametrize("lens_spec", [L22, L32, L1616], ids=["2x2", "3x2", "16x16"])
def test_flat_world_matches_the_oracle(rtc, gpu, O, lens_spec):
    got, st, info = _culled_and_brute(gpu, rtc, "flat", lens_spec, source=3)
    assert info["reflective"] is False
    ref = _oracle_lens_frame(rtc, O, "flat", lens_spec)
    _check(got, ref, 1, f"flat {lens_spec}")
    assert st["rays_reflect"] == 0 and st["rays_refract"] == 0


def test_the_3x2_case_cannot_pass_with_the_steps_mixed_up(rtc, O):
    """CPU only: both frames are the oracle's. What the 3x2 grid pins. Adding the same six colours in u-outer instead of
    v-outer order moves a pixel by rounding only (measured: 1.7e-16, far inside the tolerance; printed and bounded below),
    so the frame cannot tell the two summation orders apart. What it does tell apart is a kernel that decodes k with the
    step counts mixed up (u = k % vsteps, v = k / vsteps): that kernel samples the lens on the transposed, 2x3 grid, and
    the oracle's frame for that grid differs from the 3x2 frame by far more than the tolerance. A square grid (2x2,
    16x16) cannot see this, the 3x2 case can: it does not pass vacuously."""
    ref = _oracle_lens_frame(rtc, O, "flat", L32)
    reordered = _oracle_lens_frame(rtc, O, "flat", L32, u_outer=True)
    transposed = _oracle_lens_frame(rtc, O, "flat", (L32[0], L32[1], L32[3], L32[2]))
    d_order, d_steps = float(np.max(np.abs(ref - reordered))), float(np.max(np.abs(ref - transposed)))
    print(f"3x2: summed u-outer against v-outer {d_order:.3e}; sampled on the transposed 2x3 grid {d_steps:.3e}")
    assert d_steps > TIGHT_TOL
    assert d_order <= 6 * 2.0 ** -52   # six addends of at most 1: a reordering is rounding, nothing else
    # and the lens does something: the frame is not the pinhole frame
    w, cam = _scene(rtc, "flat")
    pin = O.render(w.array(), len(w), w.light, cam, mode=1, nthreads=8)
    assert float(np.max(np.abs(ref - pin))) > 0.05


@pytest.mark.parametrize("name,lens_spec", [("mixed", L22), ("mixed", L32), ("criterion", L22)], ids=["mixed-2x2", "mixed-3x2", "criterion-2x2"])
def test_reflective_and_refractive_worlds_match_the_oracle(rtc, gpu, O, name, lens_spec):
    got, st, info = _culled_and_brute(gpu, rtc, name, lens_spec, source=3)
    assert info["reflective"] is True and info["refractive"] is True
    _check(got, _oracle_lens_frame(rtc, O, name, lens_spec), 1, f"{name} {lens_spec}")
    assert st["rays_refract"] > 0


def test_two_level_cull_matches_brute_force_and_the_oracle(rtc, gpu, O):
    w, cam = _scene(rtc, "s300")
    assert len(w) > 256 and (cam.hsize, cam.vsize) == (40, 24)
    got, st, info = _culled_and_brute(gpu, rtc, "s300", L22, source=4)
    _check(got, _oracle_lens_frame(rtc, O, "s300", L22), 1, "s300 2x2")


# ---- the pinhole case
@pytest.mark.parametrize("name", ["flat", "mixed", "s300"])
@pytest.mark.parametrize("mode", [MODE_RENDER, MODE_RENDER_ASYNC], ids=["render", "render_async"])
def test_the_degenerate_lens_is_rtc_render_byte_for_byte(rtc, gpu, name, mode):
    w, cam = _scene(rtc, name)
    dw = gpu.upload(w)
    try:
        want, sw = dw.render(cam, mode=mode, with_stats=True)
        assert gpu.last_launch_info()["lens_samples"] == 0
        for flags in (0, NO_CULL):
            got, sg = dw.render_lens(cam, rtc.lens(*PINHOLE), mode=mode, flags=flags, with_stats=True)
            assert gpu.last_launch_info()["lens_samples"] == 1
            assert got.tobytes() == want.tobytes() and want.any()
            assert all(sg[k] == sw[k] for k in COUNTERS) and sg["rays_primary_proven_miss"] == 0
        if mode == MODE_RENDER:
            assert not want[-1].any() and not want[:, -1].any()
            assert sw["pixels"] == (cam.hsize - 1) * (cam.vsize - 1)
    finally:
        dw.close()


def test_render_mode_with_a_real_lens(rtc, gpu, O):
    """RTC_MODE_RENDER through a 2x2 lens: the last row and column stay black, the rest is the oracle's."""
    w, cam = _scene(rtc, "flat")
    got, st, info = _lens_render(gpu, rtc, w, cam, L22, mode=MODE_RENDER)
    assert not got[-1].any() and not got[:, -1].any() and got[:-1, :-1].any()
    _check(got, _oracle_lens_frame(rtc, O, "flat", L22, mode=MODE_RENDER), 1, "flat 2x2 RTC_MODE_RENDER")
    assert st["pixels"] == (W - 1) * (H - 1) and st["rays_primary"] == 4 * (W - 1) * (H - 1)


# ---- other World forms
def _with_lights(rtc, name, lights):
    w, cam = _scene(rtc, name)
    m = rtc.World(lights)
    m.shapes = w.shapes
    return m, cam


def test_a_two_light_world_matches_the_summed_oracle_frames(rtc, gpu, O):
    w, _ = _scene(rtc, "flat")
    key = (tuple(w.light.position), tuple(w.light.intensity))
    m, cam = _with_lights(rtc, "flat", [rtc.light(position=key[0], intensity=key[1]), rtc.light(position=AMONG[0], intensity=AMONG[1])])
    got, st, info = _lens_render(gpu, rtc, m, cam, L22)
    brute, sb, _ = _lens_render(gpu, rtc, m, cam, L22, NO_CULL)
    assert got.tobytes() == brute.tobytes() and st == sb
    assert info["light_table"] is False and info["lens_samples"] == 4
    ref = _oracle_lens_frame(rtc, O, "flat", L22, key) + _oracle_lens_frame(rtc, O, "flat", L22, AMONG)   # in light order
    _check(got, ref, 2, "flat, two lights, 2x2")
    one = _lens_render(gpu, rtc, w, cam, L22)[1]
    assert st["rays_shadow"] == 2 * one["rays_shadow"] and st["rays_primary"] == one["rays_primary"]


def test_an_area_light_through_the_light_table_matches_the_summed_oracle_frames(rtc, gpu, O):
    m, cam = _with_lights(rtc, "flat", [rtc.area_light(*A33)])
    samples = [(tuple(s.position), tuple(s.intensity)) for s in m.samples()]
    assert len(samples) == 9
    got, st, info = _lens_render(gpu, rtc, m, cam, L22)
    brute, sb, _ = _lens_render(gpu, rtc, m, cam, L22, NO_CULL)
    assert got.tobytes() == brute.tobytes() and st == sb
    assert info["light_table"] is True and info["lens_samples"] == 4
    ref = _oracle_lens_frame(rtc, O, "flat", L22, samples[0])
    for s in samples[1:]:
        ref = ref + _oracle_lens_frame(rtc, O, "flat", L22, s)   # in sample order
    _check(got, ref, 9, "flat, 3x3 area light, 2x2 lens")


def test_an_updated_world_renders_like_a_fresh_one(rtc, gpu):
    a, cam = _scene(rtc, "flat")
    b, _ = _with_lights(rtc, "flat", [rtc.light(position=AMONG[0], intensity=AMONG[1])])
    b.shapes = a.shapes[:20] + a.shapes[-1:]
    fresh = _lens_render(gpu, rtc, b, cam, L22)
    dw = gpu.upload(a)
    try:
        first = dw.render_lens(cam, rtc.lens(*L22))
        dw.update(b)
        got, st = dw.render_lens(cam, rtc.lens(*L22), with_stats=True)
        assert got.tobytes() == fresh[0].tobytes() and st == fresh[1] and got.tobytes() != first.tobytes()
    finally:
        dw.close()


# ---- stats and launch info
def test_stats_and_launch_info(rtc, gpu):
    w, cam = _scene(rtc, "flat")
    dw = gpu.upload(w)
    try:
        _, pin = dw.render(cam, with_stats=True)
        assert gpu.last_launch_info()["lens_samples"] == 0
        for spec in (L22, L32):
            n = spec[2] * spec[3]
            _, st = dw.render_lens(cam, rtc.lens(*spec), with_stats=True)
            info = gpu.last_launch_info()
            assert st["rays_primary"] == W * H * n and st["pixels"] == W * H and st["rays_primary_proven_miss"] == 0
            assert 0 < st["rays_shadow"] <= st["rays_primary"]
            assert info["lens_samples"] == n and info["binned_primary_pass"] is False and info["source"] == 3
            # RTC_FLAG_AA_RESAMPLE is ignored
            again, st2 = dw.render_lens(cam, rtc.lens(*spec), flags=AA_RESAMPLE, with_stats=True)
            assert st2 == st
        dw.render(cam)
        assert gpu.last_launch_info()["lens_samples"] == 0
    finally:
        dw.close()


# ---- rows and the 8-bit frame
def test_rows_compose_and_rgb8_is_color_scale_of_the_f64_rows(rtc, gpu):
    import torch
    w, cam = _scene(rtc, "mixed")
    lens = rtc.lens(*L22)
    dw = gpu.upload(w)
    try:
        whole = dw.render_lens(cam, lens)
        f64 = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
        u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        split = 16   # a multiple of the tile height; the second range ends in a partial tile row
        dw.render_lens_rows(cam, lens, 0, split, f64.data_ptr(), d_ptr8=u8.data_ptr())
        dw.render_lens_rows(cam, lens, split, H, f64[split:].data_ptr(), d_ptr8=u8[split:].data_ptr())
        dw.render_lens_rows(cam, lens, 7, 7, f64.data_ptr())   # an empty range: nothing happens
        gpu.synchronize()
        assert gpu.last_launch_info()["lens_samples"] == 4
        host = f64.cpu().numpy()
        assert host.tobytes() == whole.tobytes() and whole.any()
        assert np.array_equal(u8.cpu().numpy(), rtc.color_scale255(host).reshape(H, W, 3))
        # 8-bit rows only, and the synchronous 8-bit entry
        only8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dw.render_lens_rows(cam, lens, 0, H, None, d_ptr8=only8.data_ptr())
        gpu.synchronize()
        assert np.array_equal(only8.cpu().numpy(), u8.cpu().numpy())
        assert np.array_equal(dw.render_lens(cam, lens, rgb8=True), u8.cpu().numpy())
    finally:
        dw.close()


def test_pipelined_lens_launches(rtc, gpu):
    import torch
    w, cam = _scene(rtc, "flat")
    lens = rtc.lens(*L22)
    dw = gpu.upload(w)
    try:
        want = dw.render_lens(cam, lens)
        gpu.set_pipeline(3)
        ring = [torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        for t in ring:
            dw.render_lens_rows(cam, lens, 0, H, t.data_ptr())
        gpu.synchronize()
        assert all(t.cpu().numpy().tobytes() == want.tobytes() for t in ring)
    finally:
        gpu.set_pipeline(1)
        dw.close()


# ---- error returns
def test_error_returns(rtc, gpu):
    A = importlib.import_module(rtc.__name__ + ".abi")
    L = rtc.lib()
    w, cam = _scene(rtc, "flat")
    dw = gpu.upload(w)
    out = np.zeros((H, W, 3), dtype=np.float64)
    p = out.ctypes.data_as(C.POINTER(C.c_double))

    def lens(aperture, focal, us, vs):
        l = A.RtcLens()
        l.aperture, l.focal_distance, l.usteps, l.vsteps = aperture, focal, us, vs
        return l
    try:
        ok = lens(*L22)
        aa = A.RtcCamera()
        C.memmove(C.byref(aa), C.byref(cam), C.sizeof(A.RtcCamera))
        aa.samples = 4
        assert L.rtc_render_lens(gpu._h, dw._h, C.byref(aa), C.byref(ok), 1, 0, p, None) == ERR_ARG
        assert L.rtc_render_lens(gpu._h, dw._h, C.byref(cam), C.byref(ok), 1, NO_CULL | LDS_TABLE, p, None) == ERR_UNSUPPORTED
        assert L.rtc_render_lens(gpu._h, dw._h, C.byref(cam), C.byref(lens(0.1, 5.0, 17, 16)), 1, 0, p, None) == ERR_ARG
        assert L.rtc_render_lens(gpu._h, dw._h, C.byref(cam), C.byref(lens(-0.1, 5.0, 2, 2)), 1, 0, p, None) == ERR_ARG
        assert L.rtc_render_lens(gpu._h, dw._h, C.byref(cam), C.byref(lens(0.1, 0.0, 2, 2)), 1, 0, p, None) == ERR_ARG
        assert L.rtc_render_lens(gpu._h, dw._h, C.byref(cam), None, 1, 0, p, None) == ERR_ARG
        assert L.rtc_render_lens(gpu._h, dw._h, C.byref(cam), C.byref(ok), 2, 0, p, None) == ERR_ARG          # no such mode
        u8 = out.view(np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        assert L.rtc_render_lens_rgb8(gpu._h, dw._h, C.byref(aa), C.byref(ok), 1, 0, u8, None) == ERR_ARG
        assert L.rtc_render_lens_rows(gpu._h, dw._h, C.byref(cam), C.byref(ok), 1, 0, H, None, None, 0) == ERR_ARG   # no buffer
        assert L.rtc_render_lens_rows(gpu._h, dw._h, C.byref(cam), C.byref(ok), 1, 0, H + 1, 8, None, 0) == ERR_ARG  # rows outside the canvas
        assert L.rtc_render_lens_rows(gpu._h, dw._h, C.byref(aa), C.byref(ok), 1, 0, H, 8, None, 0) == ERR_ARG
        assert not out.any()
        # and the World still renders
        assert dw.render_lens(cam, rtc.lens(*L22)).any()
    finally:
        dw.close()


def test_depth_of_field_scene_file(rtc, gpu):
    """data/depth_of_field.yml at test size: the loaded lens renders, the sphere in focus stays sharp, the others blur."""
    data = Path(rtc.__file__).resolve().parent / "data"
    w, big, lens = rtc.load_yaml_lens(path=data / "depth_of_field.yml")
    cam = rtc.camera(W, H, big.fov, rtc.Matrix.make_view_transform((0, 1.5, -7), (0, 1, 0), (0, 1, 0)))
    dw = gpu.upload(w)
    try:
        sharp = dw.render(cam)
        got, st = dw.render_lens(cam, lens, with_stats=True)
        assert gpu.last_launch_info()["lens_samples"] == 16 and st["rays_primary"] == 16 * W * H
        diff = np.abs(got - sharp).max(axis=2)
        assert diff.max() > 0.05                       # edges out of focus are smeared
        assert diff[H // 2 - 3: H // 2 + 3, W // 2 - 1: W // 2 + 5].max() < 0.02   # the middle of the sphere in focus
    finally:
        dw.close()


def test_facade_set_lens(rtc):
    """tests/cpp/test_facade_lens.cpp: ch1::Camera::set_lens followed by render / render_async gives rtc_render_lens's canvas."""
    import importlib.util
    import subprocess
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("_rtc_build", root / "raytracer-challenge_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = b.build_facade_lens_test()
    assert exe is not None and exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade lens: ok" in r.stdout
