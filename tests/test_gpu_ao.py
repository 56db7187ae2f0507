"""The ambient-occlusion pass on the HIP path (rtc_render_ao*, k_ao; rtc_canvas_apply_ao_device, k_apply_ao).

The expected plane is ao_cases.expected_ao: the CPU oracle's centre-ray records, then one oracle color_at per sample on
rtc_ao_ray of the oracle's normal and over_point, a sample counting when the oracle reports a hit at t < radius. Every
comparison is exact (np.array_equal): the plane holds integers. tests/test_host_ao.py checks, without a GPU, that each case
holds open, occluded and partly occluded pixels."""
import ctypes as C
import importlib
import importlib.util
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ao_cases as AO

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ASYNC, SERIAL = 1, 0
NO_CULL, LDS_TABLE = 1, 4
IDS = [f"{n}-{a[0]}-{a[1]}x{a[2]}" for n, a in AO.CASES]


def _torch():
    import torch
    return torch


def _render(rtc, gpu, name, ao, mode=ASYNC, flags=0):
    w, cam = AO.world(rtc, name)
    dw = gpu.upload(w)
    try:
        return dw.render_ao(cam, rtc.ao(*ao), mode, flags)
    finally:
        dw.close()


def _assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    d = np.argwhere(got != want)
    assert len(d) == 0, f"{what}: {len(d)} pixels differ, first at {d[0].tolist()}: got {got[tuple(d[0])]}, want {want[tuple(d[0])]}"


@pytest.mark.parametrize("name,ao", AO.CASES, ids=IDS)
def test_plane_equals_the_oracles_counts(rtc, gpu, O, name, ao):
    """Oracle parity, culled (SRC_CULL for the 3-shape worlds, SRC_CULL2 for grid290) and brute force (RTC_FLAG_NO_CULL)."""
    want = AO.expected_ao(rtc, O, name, ao, ASYNC)
    _assert_same(_render(rtc, gpu, name, ao), want, f"{name} {ao}")
    _assert_same(_render(rtc, gpu, name, ao, flags=NO_CULL), want, f"{name} {ao} no-cull")


@pytest.mark.parametrize("name,ao", AO.SERIAL_CASES)
def test_render_mode_leaves_the_last_row_and_column_zero(rtc, gpu, O, name, ao):
    want = AO.expected_ao(rtc, O, name, ao, SERIAL)
    got = _render(rtc, gpu, name, ao, SERIAL)
    _assert_same(got, want, f"{name} {ao} serial")
    assert (got[-1, :] == 0).all() and (got[:, -1] == 0).all() and (got > 0).any()
    _assert_same(_render(rtc, gpu, name, ao, SERIAL, NO_CULL), want, f"{name} {ao} serial no-cull")


def test_errors_launch_nothing(rtc, gpu):
    """RTC_FLAG_LDS_TABLE is RTC_ERR_UNSUPPORTED (8); a World of another context, a bad pass, a bad mode, a NULL or misaligned
    plane are RTC_ERR_ARG (4) — and the plane keeps its fill."""
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    L = rtc.lib()
    w, cam = AO.world(rtc, "contact")
    npx = cam.hsize * cam.vsize
    dev = torch.full((npx + 1,), 0x5A5A, dtype=torch.int16, device="cuda:0")
    host = np.full((cam.vsize, cam.hsize), 0x5A5A, dtype=np.uint16)
    hp = host.ctypes.data_as(C.POINTER(C.c_uint16))
    torch.cuda.synchronize()
    good = abi.RtcAo(1.5, 2, 2)
    dw = gpu.upload(w)
    other = rtc.Context(0)
    try:
        for entry, plane in ((L.rtc_render_ao_device, dev.data_ptr()), (L.rtc_render_ao, hp)):
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, LDS_TABLE, plane) == 8
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, NO_CULL | LDS_TABLE, plane) == 8
            assert entry(other._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, plane) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), 2, 0, plane) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), None, ASYNC, 0, plane) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, None) == 4
            for radius, us, vs in [(0.0, 2, 2), (-1.0, 2, 2), (math.nan, 2, 2), (1.0, 0, 2), (1.0, 2, 0), (1.0, 257, 1), (1.0, 17, 16)]:
                assert entry(gpu._h, dw._h, C.byref(cam), C.byref(abi.RtcAo(radius, us, vs)), ASYNC, 0, plane) == 4, (radius, us, vs)
        assert L.rtc_render_ao_device(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, dev.data_ptr() + 1) == 4
        gpu.synchronize()
        assert (dev.cpu().numpy() == 0x5A5A).all() and (host == 0x5A5A).all()
        # ... and the same arguments with nothing wrong write every pixel
        assert L.rtc_render_ao_device(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, dev.data_ptr()) == 0
        assert L.rtc_render_ao(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, hp) == 0
        d = dev.cpu().numpy().view(np.uint16)
        assert np.array_equal(d[:npx].reshape(host.shape), host) and d[npx] == 0x5A5A and int(host.max()) <= 4
        # compositing on the device refuses what the host entry refuses
        rgb = torch.ones(npx * 3, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        for n, strength in [(0, 0.5), (4, -0.1), (4, 1.5), (4, math.nan)]:
            assert L.rtc_canvas_apply_ao_device(gpu._h, rgb.data_ptr(), dev.data_ptr(), n, strength, cam.hsize, cam.vsize) == 4
        assert L.rtc_canvas_apply_ao_device(gpu._h, None, dev.data_ptr(), 4, 0.5, cam.hsize, cam.vsize) == 4
        assert L.rtc_canvas_apply_ao_device(gpu._h, rgb.data_ptr(), dev.data_ptr() + 1, 4, 0.5, cam.hsize, cam.vsize) == 4
        assert L.rtc_canvas_apply_ao_device(gpu._h, rgb.data_ptr() + 4, dev.data_ptr(), 4, 0.5, cam.hsize, cam.vsize) == 4
        gpu.synchronize()
        assert (rgb.cpu().numpy() == 1.0).all()
    finally:
        other.close()
        dw.close()


def test_plane_does_not_depend_on_the_lights(rtc, gpu, O):
    """One light, two lights (kernel arguments of the render kernels) and a 256-sample area light (the device table): the
    same shapes give the same plane — nothing about lights is read."""
    ao = (1.5, 2, 2)
    want = AO.expected_ao(rtc, O, "contact", ao, ASYNC)
    for name in ("contact", "contact+2", "contact+area256"):
        w, cam = AO.world(rtc, name)
        dw = gpu.upload(w)
        try:
            assert rtc.lib().rtc_world_light_count(dw._h) == {"contact": 1, "contact+2": 2, "contact+area256": 256}[name]
            _assert_same(dw.render_ao(cam, rtc.ao(*ao)), want, name)
            _assert_same(dw.render_ao(cam, rtc.ao(*ao), flags=NO_CULL), want, name + " no-cull")
        finally:
            dw.close()


def test_updated_world_gives_a_fresh_worlds_plane(rtc, gpu, O):
    """After DeviceWorld.update moves the sphere, the plane is that of a World uploaded afresh, a launch enqueued in front of
    the update still shows the old World, and the passes' sample tables follow the grid of each launch."""
    torch = _torch()
    w, cam = AO.world(rtc, "contact")
    moved = rtc.World(w.lights)
    for s in w.shapes:
        moved.add_shape(s)
    moved.shapes[1] = rtc.sphere(rtc.Matrix.identity().translation(-0.2, 1.0, -0.8), w.shapes[1].material)
    moved.shapes[1].world_id = w.shapes[1].world_id
    a22, a44 = rtc.ao(1.5, 2, 2), rtc.ao(1.5, 4, 4)
    npx = cam.hsize * cam.vsize
    old_d, new_d = (torch.zeros(npx, dtype=torch.int16, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    try:
        dw.render_ao_device(cam, a22, old_d.data_ptr())
        dw.update(moved)
        dw.render_ao_device(cam, a44, new_d.data_ptr())   # another grid: the table is replaced behind the first launch
        gpu.synchronize()
        after = dw.render_ao(cam, a22)
    finally:
        dw.close()
    fresh = gpu.upload(moved)
    try:
        want_22, want_44 = fresh.render_ao(cam, a22), fresh.render_ao(cam, a44)
    finally:
        fresh.close()
    shape = (cam.vsize, cam.hsize)
    _assert_same(old_d.cpu().numpy().view(np.uint16).reshape(shape), AO.expected_ao(rtc, O, "contact", (1.5, 2, 2), ASYNC), "before the update")
    _assert_same(new_d.cpu().numpy().view(np.uint16).reshape(shape), want_44, "behind the update, 4x4")
    _assert_same(after, want_22, "after the update")
    assert not np.array_equal(want_22, AO.expected_ao(rtc, O, "contact", (1.5, 2, 2), ASYNC))
    # the fresh World's plane is the oracle's for the moved shapes, on a sample of pixels
    arr, n, dirs = moved.array(), len(moved), rtc.ao_expand(a22)
    for (x, y) in [(px, py) for py in range(1, cam.vsize, 4) for px in range(0, cam.hsize, 4)]:
        _, h = O.color_at(arr, n, moved.light, tuple(rtc.ray_for_pixel(cam, x, y)), 0, want_hit=True)
        count = 0
        if h.hit_index >= 0:
            for local in dirs:
                _, s = O.color_at(arr, n, moved.light, tuple(rtc.ao_ray(tuple(h.normal), tuple(h.over_point), local)), 0, want_hit=True)
                count += int(s.hit_index >= 0 and s.t < 1.5)
        assert want_22[y, x] == count, (x, y)


def test_view_and_compositing_on_the_device(rtc, gpu, O):
    """RTC_AOV_VIEW_SHADOW of the device plane with n_lights = n equals the host view byte for byte; apply_ao_device equals
    rtc_canvas_apply_ao on the same canvas; the encoders take the picture as it is."""
    torch = _torch()
    name, ao = "contact", (math.inf, 4, 4)
    n = ao[1] * ao[2]
    w, cam = AO.world(rtc, name)
    want = AO.expected_ao(rtc, O, name, ao, ASYNC)
    width, height = cam.hsize, cam.vsize
    plane = torch.zeros(width * height, dtype=torch.int16, device="cuda:0")
    pic = torch.zeros(width * height * 3, dtype=torch.uint8, device="cuda:0")
    canvas = torch.zeros((height, width, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    enc = rtc.ImageEncoder(gpu)
    try:
        beauty = dw.render(cam)
        dw.render_rows(cam, 0, height, canvas.data_ptr())
        dw.render_ao_device(cam, rtc.ao(*ao), plane.data_ptr())
        gpu.aov_view_device("shadow", {"shadow": plane.data_ptr()}, width, height, pic.data_ptr(), n_lights=n)
        png = enc.encode_device("png", pic.data_ptr(), width, height, 3)
        gpu.apply_ao_device(canvas.data_ptr(), plane.data_ptr(), n, 0.8, width, height)
        gpu.synchronize()
    finally:
        enc.close()
        dw.close()
    _assert_same(plane.cpu().numpy().view(np.uint16).reshape(height, width), want, "device plane")
    host_pic = rtc.aov_view("shadow", {"shadow": want}, n_lights=n)
    assert np.array_equal(pic.cpu().numpy().reshape(height, width, 3), host_pic) and len(np.unique(host_pic)) > 3
    assert png == rtc.image_encode("png", host_pic)
    composited = rtc.apply_ao(beauty, want, n, 0.8)
    assert canvas.cpu().numpy().tobytes() == composited.tobytes()
    assert not np.array_equal(composited, beauty) and np.array_equal(composited[want == 0], beauty[want == 0])
    # the view of index 4 stays an error: the AO plane is viewed as a shadow plane
    assert rtc.lib().rtc_aov_view_rgb8_device(gpu._h, 4, C.byref(importlib.import_module(rtc.__name__ + ".abi").RtcAovBuffers(shadow=plane.data_ptr())),
                                              width, height, 0.0, 1.0, n, pic.data_ptr()) == 4


def test_stats_are_not_touched(rtc, gpu):
    w, cam = AO.world(rtc, "contact")
    dw = gpu.upload(w)
    try:
        dw.render(cam, with_stats=True)
        before = gpu.stats(extended=True)
        assert before["rays_primary"] > 0
        dw.render_ao(cam, rtc.ao(1.5, 4, 4))
        dw.render_ao(cam, rtc.ao(1.5, 4, 4), flags=NO_CULL)
        assert gpu.stats(extended=True) == before
        gpu.reset_stats()
        dw.render_ao(cam, rtc.ao(math.inf, 2, 2))
        assert all(v == 0 for v in gpu.stats(extended=True).values())
    finally:
        dw.close()


def test_full_frame_against_color_at(rtc, gpu):
    """One whole 1920x1080 frame with 4 samples against rtc_color_at over the same rays: rtc_ao_ray of the library's own point,
    normal and over_point records (the probe kernel's), a sample counting when its hit has t < radius."""
    scenes = importlib.import_module(rtc.__name__ + ".scenes")
    w, cam = scenes.synthetic(20, 1920, 1080)
    radius, ao = 1.0, rtc.ao(1.0, 2, 2)
    dirs = rtc.ao_expand(ao)
    dw = gpu.upload(w)
    try:
        got = dw.render_ao(cam, ao)
        brute = dw.render_ao(cam, ao, flags=NO_CULL)
        planes = dw.render_aov(cam, ("index", "normal", "point"))
        hit = planes["index"].reshape(-1) >= 0
        normal, point = planes["normal"].reshape(-1, 3)[hit], planes["point"].reshape(-1, 3)[hit]
        over = point + normal * 0.00000001   # Intersection::compute_vectors: point.add(normal.mul(EPSILON)), one product, one sum (RTC_EPSILON)
        # rtc_ao_ray vectorised over the pixels: the header's arithmetic, term by term (test_host_ao.py pins it bit for bit)
        nx, ny, nz = normal[:, 0], normal[:, 1], normal[:, 2]
        sign = np.copysign(1.0, nz)
        a = -1.0 / (sign + nz)
        b = (nx * ny) * a
        t = np.stack([1.0 + ((sign * nx) * nx) * a, sign * b, -(sign * nx)], axis=1)
        s = np.stack([b, sign + ((ny * ny) * a), -ny], axis=1)
        counts = np.zeros(int(hit.sum()), dtype=np.uint16)
        for lx, ly, lz in dirs:
            rays = np.concatenate([over, ((t * lx) + (s * ly)) + (normal * lz)], axis=1)
            _, hits = dw.color_at(rays, remaining=0, want_hits=True)
            rec = np.frombuffer(hits, dtype=AO.A.HIT_DTYPE)[:len(rays)]
            counts += ((rec["hit_index"] >= 0) & (rec["t"] < radius)).astype(np.uint16)
    finally:
        dw.close()
    # spot-check the vectorised restatement against the library's rtc_ao_ray
    for i in range(0, len(over), max(1, len(over) // 50)):
        assert np.array_equal(rtc.ao_ray(normal[i], over[i], dirs[1])[3:], ((t[i] * dirs[1][0]) + (s[i] * dirs[1][1])) + (normal[i] * dirs[1][2]))
    want = np.zeros(1920 * 1080, dtype=np.uint16)
    want[hit] = counts
    want = want.reshape(1080, 1920)
    assert 0 < int(hit.sum()) < hit.size and (counts == 0).any() and (counts == 4).any() and ((counts > 0) & (counts < 4)).any()
    _assert_same(got, want, "1920x1080")
    _assert_same(brute, want, "1920x1080 no-cull")


def test_facade(rtc):
    spec = importlib.util.spec_from_file_location("_rtc_build", ROOT / "raytracer-challenge_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    exe = b.build_facade_ao_test()
    assert exe is not None and exe.exists()
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "facade ao: ok" in r.stdout
