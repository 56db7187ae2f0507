"""Orthographic and panorama cameras on the HIP path (rtc_render_projection*, k_trace's projection instantiations).

A projection pixel is the oracle's color_at of ONE normative ray (rtc_projection_ray, include/rtc.h), so the reference frame
is built pixel by pixel from those rays (tests/projection_cases.py: computed once, shared, never written to). Bound 1e-12 per
light, the project's TIGHT_TOL, plus equality of the non-zero masks. Every parity case also checks that the culled and the
RTC_FLAG_NO_CULL frames and stats are the same bytes, the launch info, and the primary-ray counters.

Frames are 70x45 (partial 8x8 tiles on both edges) unless the case says otherwise; cameras stand among the shapes. That the
cases can tell a wrong kernel from a right one, and that they reach all three of make_bundle's decisions, is shown on the CPU
in tests/test_host_projection.py."""
import ctypes as C
import importlib
from pathlib import Path

import numpy as np
import pytest

import projection_cases as PC
from projection_cases import ORTHO, PANO, TIGHT_TOL, W, H

pytestmark = pytest.mark.gpu

NO_CULL, AA_RESAMPLE, LDS_TABLE = 1, 2, 4
ERR_ARG, ERR_UNSUPPORTED = 4, 8
MODE_RENDER, MODE_RENDER_ASYNC = 0, 1
AMONG = ((1.5, 1.25, 4.0), (0.2, 0.45, 0.7))
A33 = ((-11.5, 10.0, -11.5), (3.0, 0.0, 0.0), (0.0, 0.5, 3.0), 3, 3, (1.0, 0.95, 0.9))


def _render(gpu, world, cam, proj, flags=0, mode=MODE_RENDER_ASYNC):
    """(canvas, stats, launch info)"""
    dw = gpu.upload(world)
    try:
        got, st = dw.render_projection(cam, proj, mode=mode, flags=flags, with_stats=True)
        return got, st, gpu.last_launch_info()
    finally:
        dw.close()


def _check(got, ref, n_lights, what):
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max|gpu - oracle| = {err:.3e} (bound {n_lights * TIGHT_TOL:.1e})")
    assert err <= n_lights * TIGHT_TOL, (what, err)
    assert np.array_equal(got != 0, ref != 0), what


def _culled_and_brute(gpu, world, cam, proj, source):
    """The culled frame, after checking that the RTC_FLAG_NO_CULL frame and its stats are the same bytes."""
    got, st, info = _render(gpu, world, cam, proj)
    brute, sb, info_b = _render(gpu, world, cam, proj, NO_CULL)
    assert info["source"] == source and info_b["source"] == 0, (info, info_b)
    assert got.tobytes() == brute.tobytes() and st == sb and got.any()
    for i in (info, info_b):
        assert i["projection"] == proj.kind and i["lens_samples"] == 0 and i["binned_primary_pass"] is False and i["multi_tile_workgroups"] == 0
    assert st["rays_primary"] == cam.hsize * cam.vsize == st["pixels"]
    assert st["rays_primary_proven_miss"] == 0 and st["rays_shadow"] > 0
    return got, st, info


def _parity(rtc, gpu, O, name):
    w, cam, proj = PC.build(rtc, name)
    got, st, info = _culled_and_brute(gpu, w, cam, proj, PC.CASES[name].source)
    _check(got, PC.reference(rtc, O, name), 1, name)
    return got, st, info


# ---- oracle parity
@pytest.mark.parametrize("name", PC.FLAT_CASES)
def test_flat_world_matches_the_oracle(rtc, gpu, O, name):
    got, st, info = _parity(rtc, gpu, O, name)
    assert info["reflective"] is False and st["rays_reflect"] == 0 and st["rays_refract"] == 0


def test_the_straddled_sphere_is_hit_from_inside(rtc, gpu, O):
    """flat-ortho-straddle (parity above): the origin plane passes through a sphere's centre, so the rays that start inside
    it hit it from inside, and whatever lies wholly behind the plane has only t < 0 to offer: the oracle, whose frame the
    GPU's equals, does not show it. Here: the case is what it claims to be, and a pinhole at the same place sees something else."""
    w, cam, proj = PC.build(rtc, "flat-ortho-straddle")
    got, _, _ = _render(gpu, w, cam, proj)
    ray = rtc.projection_ray(cam, proj, cam.hsize // 2, cam.vsize // 2)
    _, hit = O.color_at(w.array(), len(w), w.light, list(ray), want_hit=True)
    assert hit.hit_index >= 0 and hit.inside == 1
    assert float(np.max(np.abs(got - _pinhole(gpu, w, cam)))) > 0.05


def _pinhole(gpu, world, cam):
    dw = gpu.upload(world)
    try:
        return dw.render(cam)
    finally:
        dw.close()


@pytest.mark.parametrize("name", PC.STACK_CASES)
def test_reflective_and_refractive_worlds_match_the_oracle(rtc, gpu, O, name):
    got, st, info = _parity(rtc, gpu, O, name)
    assert info["reflective"] is True and info["refractive"] is True
    assert st["rays_refract"] > 0


@pytest.mark.parametrize("name", PC.S300_CASES)
def test_two_level_cull_matches_brute_force_and_the_oracle(rtc, gpu, O, name):
    w, cam, proj = PC.build(rtc, name)
    assert len(w) > 256 and (cam.hsize, cam.vsize) == (40, 24)
    _parity(rtc, gpu, O, name)


# ---- RTC_MODE_RENDER
@pytest.mark.parametrize("name", ["flat-ortho", "flat-pano"])
def test_render_mode_leaves_the_last_row_and_column_black(rtc, gpu, O, name):
    w, cam, proj = PC.build(rtc, name)
    got, st, info = _render(gpu, w, cam, proj, mode=MODE_RENDER)
    brute, sb, _ = _render(gpu, w, cam, proj, NO_CULL, mode=MODE_RENDER)
    assert got.tobytes() == brute.tobytes() and st == sb
    assert not got[-1].any() and not got[:, -1].any() and got[:-1, :-1].any()
    _check(got, PC.reference(rtc, O, name, mode=MODE_RENDER), 1, f"{name} RTC_MODE_RENDER")
    assert st["pixels"] == (W - 1) * (H - 1) == st["rays_primary"] and info["projection"] == proj.kind


# ---- other World forms
def _with_lights(rtc, name, lights):
    w, cam, proj = PC.build(rtc, name)
    m = rtc.World(lights)
    m.shapes = w.shapes
    return m, cam, proj


@pytest.mark.parametrize("name", ["flat-ortho", "flat-pano"])
def test_a_two_light_world_matches_the_summed_oracle_frames(rtc, gpu, O, name):
    w, _, _ = PC.build(rtc, name)
    key = (tuple(w.light.position), tuple(w.light.intensity))
    m, cam, proj = _with_lights(rtc, name, [rtc.light(position=key[0], intensity=key[1]), rtc.light(position=AMONG[0], intensity=AMONG[1])])
    got, st, info = _render(gpu, m, cam, proj)
    brute, sb, _ = _render(gpu, m, cam, proj, NO_CULL)
    assert got.tobytes() == brute.tobytes() and st == sb
    assert info["light_table"] is False and info["projection"] == proj.kind
    ref = PC.reference(rtc, O, name, key) + PC.reference(rtc, O, name, AMONG)   # in light order
    _check(got, ref, 2, f"{name}, two lights")
    one = _render(gpu, w, cam, proj)[1]
    assert st["rays_shadow"] == 2 * one["rays_shadow"] and st["rays_primary"] == one["rays_primary"]


@pytest.mark.parametrize("name", ["flat-ortho", "flat-pano"])
def test_an_area_light_through_the_light_table_matches_the_summed_oracle_frames(rtc, gpu, O, name):
    m, cam, proj = _with_lights(rtc, name, [rtc.area_light(*A33)])
    samples = [(tuple(s.position), tuple(s.intensity)) for s in m.samples()]
    assert len(samples) == 9
    got, st, info = _render(gpu, m, cam, proj)
    brute, sb, _ = _render(gpu, m, cam, proj, NO_CULL)
    assert got.tobytes() == brute.tobytes() and st == sb
    assert info["light_table"] is True and info["projection"] == proj.kind
    ref = PC.reference(rtc, O, name, samples[0])
    for s in samples[1:]:
        ref = ref + PC.reference(rtc, O, name, s)   # in sample order
    _check(got, ref, 9, f"{name}, 3x3 area light")


@pytest.mark.parametrize("name", ["flat-ortho", "flat-pano"])
def test_an_updated_world_renders_like_a_fresh_one(rtc, gpu, name):
    a, cam, proj = PC.build(rtc, name)
    b = rtc.World([rtc.light(position=AMONG[0], intensity=AMONG[1])])
    b.shapes = a.shapes[:20] + a.shapes[-1:]
    fresh = _render(gpu, b, cam, proj)
    dw = gpu.upload(a)
    try:
        first = dw.render_projection(cam, proj)
        dw.update(b)
        got, st = dw.render_projection(cam, proj, with_stats=True)
        assert got.tobytes() == fresh[0].tobytes() and st == fresh[1] and got.tobytes() != first.tobytes()
    finally:
        dw.close()


# ---- stats and launch info
def test_stats_and_launch_info(rtc, gpu):
    w, cam, pano = PC.build(rtc, "flat-pano")
    _, _, ortho = PC.build(rtc, "flat-ortho")
    dw = gpu.upload(w)
    try:
        dw.render(cam)
        assert gpu.last_launch_info()["projection"] == 0
        for proj in (ortho, pano):
            _, st = dw.render_projection(cam, proj, with_stats=True)
            info = gpu.last_launch_info()
            assert st["rays_primary"] == W * H == st["pixels"] and st["rays_primary_proven_miss"] == 0
            assert 0 < st["rays_shadow"] <= st["rays_primary"]
            assert info["projection"] == proj.kind and info["lens_samples"] == 0 and info["binned_primary_pass"] is False and info["source"] == 3
            again, st2 = dw.render_projection(cam, proj, flags=AA_RESAMPLE, with_stats=True)   # RTC_FLAG_AA_RESAMPLE is ignored
            assert st2 == st
        dw.render_lens(cam, rtc.lens(0.2, 8.0, 2, 2))
        info = gpu.last_launch_info()
        assert info["projection"] == 0 and info["lens_samples"] == 4
    finally:
        dw.close()


# ---- rows and the 8-bit frame
@pytest.mark.parametrize("name", ["mixed-ortho", "mixed-pano"])
def test_rows_compose_and_rgb8_is_color_scale_of_the_f64_rows(rtc, gpu, name):
    import torch
    w, cam, proj = PC.build(rtc, name)
    dw = gpu.upload(w)
    try:
        whole = dw.render_projection(cam, proj)
        f64 = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
        u8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        split = 16   # a multiple of the tile height; the second range ends in a partial tile row
        dw.render_projection_rows(cam, proj, 0, split, f64.data_ptr(), d_ptr8=u8.data_ptr())
        dw.render_projection_rows(cam, proj, split, H, f64[split:].data_ptr(), d_ptr8=u8[split:].data_ptr())
        dw.render_projection_rows(cam, proj, 7, 7, f64.data_ptr())   # an empty range: nothing happens
        gpu.synchronize()
        assert gpu.last_launch_info()["projection"] == proj.kind
        host = f64.cpu().numpy()
        assert host.tobytes() == whole.tobytes() and whole.any()
        assert np.array_equal(u8.cpu().numpy(), rtc.color_scale255(host).reshape(H, W, 3))
        # 8-bit rows only, and the synchronous 8-bit entry
        only8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dw.render_projection_rows(cam, proj, 0, H, None, d_ptr8=only8.data_ptr())
        gpu.synchronize()
        assert np.array_equal(only8.cpu().numpy(), u8.cpu().numpy())
        assert np.array_equal(dw.render_projection(cam, proj, rgb8=True), u8.cpu().numpy())
    finally:
        dw.close()


# ---- pipelined launches and the panorama tables
def _uploads(rtc, gpu):
    f = rtc.lib().rtc_debug_projection_uploads
    f.argtypes, f.restype = [C.c_void_p, C.POINTER(C.c_ulonglong)], C.c_int32
    out = C.c_ulonglong(0)
    assert f(gpu._h, C.byref(out)) == 0
    return out.value


def test_pipelined_launches_and_a_change_of_panorama_size(rtc, gpu, O):
    """Depth 3: a ring of three buffers holds the in-order bytes; then a panorama of ANOTHER size on the same pipelined context
    (its tables replace the first size's, which launches in flight on other lanes may still read), then the first size again.
    One size in a loop uploads its tables once."""
    import torch
    w, cam, proj = PC.build(rtc, "flat-pano")
    small = rtc.camera(40, 24, 1.0, rtc.Matrix.make_view_transform(*PC.FLAT_AMONG))
    half = rtc.projection(PANO, h_span=PC.PI, v_span=PC.PI / 2.0)
    _, _, ortho = PC.build(rtc, "flat-ortho")
    dw = gpu.upload(w)
    try:
        want, want_small, want_ortho = dw.render_projection(cam, proj), dw.render_projection(small, half), dw.render_projection(cam, ortho)
        _check(want, PC.reference(rtc, O, "flat-pano"), 1, "flat-pano in order")
        _check(want_small, PC.reference_of(rtc, O, w, w.light, small, half), 1, "flat, 40x24 half panorama in order")
        gpu.set_pipeline(3)
        u0 = _uploads(rtc, gpu)
        ring = [torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0") for _ in range(3)]
        other = torch.zeros((24, 40, 3), dtype=torch.float64, device="cuda:0")
        again = [torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        for t in ring:
            dw.render_projection_rows(cam, proj, 0, H, t.data_ptr())
        assert _uploads(rtc, gpu) == u0 + 1   # the size changed back once, before the ring; the ring itself uploads nothing
        dw.render_projection_rows(small, half, 0, 24, other.data_ptr())
        dw.render_projection_rows(cam, proj, 0, H, again[0].data_ptr())
        dw.render_projection_rows(cam, ortho, 0, H, again[1].data_ptr())   # an orthographic launch has no tables
        assert _uploads(rtc, gpu) == u0 + 3
        gpu.synchronize()
        assert all(t.cpu().numpy().tobytes() == want.tobytes() for t in ring)
        assert other.cpu().numpy().tobytes() == want_small.tobytes()
        assert again[0].cpu().numpy().tobytes() == want.tobytes() and again[1].cpu().numpy().tobytes() == want_ortho.tobytes()
    finally:
        gpu.set_pipeline(1)
        dw.close()


# ---- error returns
def test_error_returns(rtc, gpu):
    A = importlib.import_module(rtc.__name__ + ".abi")
    L = rtc.lib()
    w, cam, ok = PC.build(rtc, "flat-pano")
    dw = gpu.upload(w)
    out = np.zeros((H, W, 3), dtype=np.float64)
    p = out.ctypes.data_as(C.POINTER(C.c_double))

    def proj(kind, width=0.0, h_span=0.0, v_span=0.0):
        q = A.RtcProjection()
        q.kind, q.width, q.h_span, q.v_span = kind, width, h_span, v_span
        return q
    try:
        aa = A.RtcCamera()
        C.memmove(C.byref(aa), C.byref(cam), C.sizeof(A.RtcCamera))
        aa.samples = 4
        render = lambda c, q, mode=1, flags=0: L.rtc_render_projection(gpu._h, dw._h, c, q, mode, flags, p, None)
        assert render(C.byref(aa), C.byref(ok)) == ERR_ARG
        assert render(C.byref(cam), C.byref(ok), flags=NO_CULL | LDS_TABLE) == ERR_UNSUPPORTED
        assert render(C.byref(cam), C.byref(proj(ORTHO, 5.0)), flags=NO_CULL | LDS_TABLE) == ERR_UNSUPPORTED
        for bad in (proj(0, 1.0, 1.0, 1.0), proj(3, 1.0, 1.0, 1.0), proj(ORTHO, 0.0), proj(ORTHO, -2.0), proj(ORTHO, float("inf")),
                    proj(PANO, 0.0, 0.0, 1.0), proj(PANO, 0.0, 7.0, 1.0), proj(PANO, 0.0, 1.0, 0.0), proj(PANO, 0.0, 1.0, 3.2),
                    proj(PANO, 0.0, float("nan"), 1.0)):
            assert render(C.byref(cam), C.byref(bad)) == ERR_ARG, (bad.kind, bad.width, bad.h_span, bad.v_span)
        assert render(C.byref(cam), None) == ERR_ARG
        assert render(None, C.byref(ok)) == ERR_ARG
        assert L.rtc_render_projection(gpu._h, None, C.byref(cam), C.byref(ok), 1, 0, p, None) == ERR_ARG
        assert L.rtc_render_projection(None, dw._h, C.byref(cam), C.byref(ok), 1, 0, p, None) == ERR_ARG
        assert L.rtc_render_projection(gpu._h, dw._h, C.byref(cam), C.byref(ok), 1, 0, None, None) == ERR_ARG
        assert render(C.byref(cam), C.byref(ok), mode=2) == ERR_ARG          # no such mode
        u8 = out.view(np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
        assert L.rtc_render_projection_rgb8(gpu._h, dw._h, C.byref(aa), C.byref(ok), 1, 0, u8, None) == ERR_ARG
        assert L.rtc_render_projection_rgb8(gpu._h, dw._h, C.byref(cam), None, 1, 0, u8, None) == ERR_ARG
        rows = L.rtc_render_projection_rows
        assert rows(gpu._h, dw._h, C.byref(cam), C.byref(ok), 1, 0, H, None, None, 0) == ERR_ARG   # no buffer
        assert rows(gpu._h, dw._h, C.byref(cam), C.byref(ok), 1, 0, H + 1, 8, None, 0) == ERR_ARG  # rows outside the canvas
        assert rows(gpu._h, dw._h, C.byref(cam), C.byref(ok), 1, 9, 8, 8, None, 0) == ERR_ARG      # y0 > y1
        assert rows(gpu._h, dw._h, C.byref(aa), C.byref(ok), 1, 0, H, 8, None, 0) == ERR_ARG
        assert rows(gpu._h, dw._h, C.byref(cam), None, 1, 0, H, 8, None, 0) == ERR_ARG
        assert not out.any()
        # and the World still renders
        assert dw.render_projection(cam, ok).any()
    finally:
        dw.close()


# ---- the scene files
@pytest.mark.parametrize("name,kind", [("panorama.yml", PANO), ("orthographic.yml", ORTHO)])
def test_projection_scene_files(rtc, gpu, O, name, kind):
    """data/panorama.yml and data/orthographic.yml at test size: they load, render, match the oracle, and are not the pinhole frame."""
    data = Path(rtc.__file__).resolve().parent / "data"
    w, big, lens, proj = rtc.load_yaml_projection(path=data / name)
    assert lens is None and proj.kind == kind
    cam = rtc.camera(W, H, big.fov)
    C.memmove(cam.view_inv, big.view_inv, C.sizeof(cam.view_inv))
    dw = gpu.upload(w)
    try:
        pinhole = dw.render(cam)
        got, st = dw.render_projection(cam, proj, with_stats=True)
        assert gpu.last_launch_info()["projection"] == kind and st["rays_primary"] == W * H
        _check(got, PC.reference_of(rtc, O, w, w.light, cam, proj), 1, name)
        assert float(np.max(np.abs(got - pinhole))) > 0.05 and got.any()
    finally:
        dw.close()


def test_the_render_tool_writes_a_png(rtc, gpu, tmp_path):
    """tools/render_yaml_projection.py scene.yml out.png at a small size"""
    import subprocess
    import sys
    root = Path(__file__).resolve().parents[1]
    data = Path(rtc.__file__).resolve().parent / "data"
    out = tmp_path / "pano.png"
    r = subprocess.run([sys.executable, str(root / "tools" / "render_yaml_projection.py"), str(data / "panorama.yml"), str(out), "--width", "64", "--height", "32"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and "panorama" in r.stdout


def test_facade_set_projection(rtc):
    """tests/cpp/test_facade_projection.cpp: ch1::Camera::set_projection followed by render / render_async gives
    rtc_render_projection's canvas; set_lens with a projection throws, and so does render_aov."""
    import importlib.util
    import subprocess
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("_rtc_build", root / "raytracer-challenge_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = b.build_facade_projection_test()
    assert exe is not None and exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade projection: ok" in r.stdout
