"""The one-bounce gather pass on the HIP path (rtc_render_gather*, k_gather; rtc_canvas_add_scaled_device, k_add_scaled).

The expected planes are gather_cases.expected: the CPU oracle's centre-ray records, then per sample and per light one oracle
color_at(remaining 0) on rtc_ao_ray of the oracle's normal and over_point, summed in light order, the radius applied to the
record's t, `base` from the oracle's pattern function, all packed by rtc_gather_from_hits. The bound is the project's
(tests/adversarial_worlds.py): 1e-12 per light sample, pow being the only operation that is not bit-exact; a mean of samples
each within n_lights x 1e-12 is within it too. tests/test_host_gather.py checks, without a GPU, that each case exercises the
pass."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest

import aov_cases as A
import gather_cases as G

pytestmark = pytest.mark.gpu

ASYNC, SERIAL = 1, 0
NO_CULL, LDS_TABLE = 1, 4
TIGHT_TOL = 1e-12   # per light sample (tests/adversarial_worlds.py)
PLANES = ("radiance", "bounce")


def _torch():
    import torch
    return torch


def _render(rtc, ctx, name, ao, mode=ASYNC, flags=0, planes=PLANES):
    w, cam = G.world(rtc, name)
    dw = ctx.upload(w)
    try:
        return dw.render_gather(cam, rtc.ao(*ao), mode, flags, planes)
    finally:
        dw.close()


def _same_bytes(got, want, what):
    for p in want:
        assert got[p].shape == want[p].shape and got[p].tobytes() == want[p].tobytes(), f"{what}: plane {p} differs"


def _assert_close(rtc, O, got, name, ao, mode, what):
    want = G.expected(rtc, O, name, ao, mode)
    n_lights = len(G.world(rtc, name)[0].samples())
    tol = n_lights * TIGHT_TOL
    scale = max(1.0, float(np.abs(G.albedo(rtc, O, name)).max()))
    for p, bound in (("radiance", tol), ("bounce", tol * scale)):
        assert got[p].dtype == np.float64 and got[p].shape == want[p].shape, what
        err = float(np.abs(got[p] - want[p]).max())
        print(f"{what}: {p} max |got - want| = {err:.3e} (bound {bound:.1e})")
        assert err <= bound, f"{what}: {p} off by {err:.3e} > {bound:.1e}"
        assert np.array_equal(got[p] == 0.0, want[p] == 0.0), f"{what}: {p}: the exactly-zero entries differ"


@pytest.mark.parametrize("name,ao", G.CASES, ids=G.IDS)
def test_planes_equal_the_oracles(rtc, gpu, O, name, ao):
    """Oracle parity, culled (SRC_CULL for the 3-shape worlds, SRC_CULL2 for grid290); brute force (RTC_FLAG_NO_CULL) gives the
    culled bytes."""
    got = _render(rtc, gpu, name, ao)
    _assert_close(rtc, O, got, name, ao, ASYNC, f"{name} {ao}")
    _same_bytes(_render(rtc, gpu, name, ao, flags=NO_CULL), got, f"{name} {ao} no-cull")


@pytest.mark.parametrize("name,ao", G.SERIAL_CASES)
def test_render_mode_leaves_the_last_row_and_column_zero(rtc, gpu, O, name, ao):
    got = _render(rtc, gpu, name, ao, SERIAL)
    _assert_close(rtc, O, got, name, ao, SERIAL, f"{name} {ao} serial")
    free = _render(rtc, gpu, name, ao)
    for p in PLANES:
        assert not got[p][-1].any() and not got[p][:, -1].any() and got[p].any()
        assert free[p][-1].any() or free[p][:, -1].any()
        assert got[p][:-1, :-1].tobytes() == free[p][:-1, :-1].tobytes()
    _same_bytes(_render(rtc, gpu, name, ao, SERIAL, NO_CULL), got, f"{name} {ao} serial no-cull")


@pytest.mark.parametrize("name,ao", [("bleed", (1.5, 2, 2)), ("grid290", (0.5, 2, 2)), ("bleed+9", (1.5, 2, 2))])
def test_one_plane_alone_holds_the_same_bytes(rtc, gpu, name, ao):
    both = _render(rtc, gpu, name, ao)
    for p in PLANES:
        only = _render(rtc, gpu, name, ao, planes=(p,))
        assert list(only) == [p] and only[p].tobytes() == both[p].tobytes()
    # the device entry leaves the plane that is not asked for alone
    torch = _torch()
    w, cam = G.world(rtc, name)
    n = cam.hsize * cam.vsize * 3
    rad, bounce = (torch.full((n + 1,), 7.0, dtype=torch.float64, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    try:
        dw.render_gather_device(cam, rtc.ao(*ao), {"radiance": rad.data_ptr()})
        gpu.synchronize()
    finally:
        dw.close()
    assert rad.cpu().numpy()[:n].tobytes() == both["radiance"].tobytes() and float(rad[n]) == 7.0 and bool((bounce == 7.0).all())


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


@pytest.mark.parametrize("n_lights", [2, 8])
def test_the_light_table_kernels_are_the_kernel_argument_kernels(rtc, gpu, n_lights):
    """2 and 8 lights travel in the kernel arguments; a context made under RTC_LIGHT_TABLE=1 sends the same Worlds through the
    World's light table, the path the nine-light World takes: the planes are equal byte for byte, culled and brute force
    (tests/test_gpu_area_lights.py's rule for the table kernels)."""
    w9, cam = G.world(rtc, "bleed+9")
    lights = G.world(rtc, "bleed+2")[0].samples() if n_lights == 2 else w9.samples()[:8]
    w = rtc.World([rtc.light(tuple(l.position), tuple(l.intensity)) for l in lights])
    for s in w9.shapes:
        w.add_shape(s)
    ao = rtc.ao(1.5, 2, 2)
    table_ctx = _ctx_env(rtc, RTC_LIGHT_TABLE=1)
    try:
        got = []
        for ctx in (gpu, table_ctx):
            dw = ctx.upload(w)
            try:
                assert rtc.lib().rtc_world_light_count(dw._h) == n_lights
                dw.render(cam)
                got.append((ctx.last_launch_info()["light_table"], dw.render_gather(cam, ao), dw.render_gather(cam, ao, flags=NO_CULL)))
            finally:
                dw.close()
    finally:
        table_ctx.close()
    assert got[0][0] is False and got[1][0] is True
    _same_bytes(got[1][1], got[0][1], f"{n_lights} lights: table against kernel arguments")
    _same_bytes(got[1][2], got[0][1], f"{n_lights} lights: table, no-cull")
    _same_bytes(got[0][2], got[0][1], f"{n_lights} lights: kernel arguments, no-cull")
    assert got[0][1]["radiance"].any()


def test_updated_world_gives_a_fresh_worlds_planes(rtc, gpu, O):
    """After DeviceWorld.update moves the sphere and recolours it, the planes are those of a World uploaded afresh, and a launch
    enqueued in front of the update still shows the old World."""
    torch = _torch()
    name, ao = "bleed", (1.5, 2, 2)
    w, cam = G.world(rtc, name)
    moved = rtc.World(w.lights)
    for s in w.shapes:
        moved.add_shape(s)
    moved.shapes[1] = rtc.sphere(rtc.Matrix.identity().translation(-0.2, 1.0, -0.8), rtc.material(color=G.BLUE, diffuse=0.8, specular=0.3))
    moved.shapes[1].world_id = w.shapes[1].world_id
    a = rtc.ao(*ao)
    n = cam.hsize * cam.vsize * 3
    old_d = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    try:
        dw.render_gather_device(cam, a, {"radiance": old_d.data_ptr()})
        dw.update(moved)
        after = dw.render_gather(cam, a)
    finally:
        dw.close()
    fresh = gpu.upload(moved)
    try:
        want = fresh.render_gather(cam, a)
    finally:
        fresh.close()
    _same_bytes(after, want, "after the update")
    before = old_d.cpu().numpy().reshape(cam.vsize, cam.hsize, 3)
    assert before.tobytes() == _render(rtc, gpu, name, ao)["radiance"].tobytes() and before.tobytes() != want["radiance"].tobytes()
    # the fresh World's radiance is the oracle's for the moved shapes, on a sample of pixels
    arr, nshapes, dirs = moved.array(), len(moved), rtc.ao_expand(a)
    checked = 0
    for (x, y) in [(px, py) for py in range(1, cam.vsize, 4) for px in range(0, cam.hsize, 4)]:
        _, h = O.color_at(arr, nshapes, moved.light, tuple(rtc.ray_for_pixel(cam, x, y)), 0, want_hit=True)
        total = np.zeros(3)
        if h.hit_index >= 0:
            for local in dirs:
                col, s = O.color_at(arr, nshapes, moved.light, tuple(rtc.ao_ray(tuple(h.normal), tuple(h.over_point), local)), 0, want_hit=True)
                total = total + (col if (s.hit_index >= 0 and s.t < ao[0]) else np.zeros(3))
            checked += int(total.any())
        assert np.abs(want["radiance"][y, x] - total / 4.0).max() <= TIGHT_TOL, (x, y)
    assert checked >= 5


def test_whole_frame_against_color_at(rtc, gpu):
    """One 480x270 frame, two lights, 2x2 samples, unbounded, against the library itself: rtc_render_aov's point, normal and
    index, the rays of rtc_ao_ray (vectorised in numpy term by term and spot-checked against the entry), rtc_color_at with
    remaining 0 per sample, rtc_gather_from_hits. The same device arithmetic in the same order: byte-equal."""
    name, ao = "bleed+2:480x270", rtc.ao(math.inf, 2, 2)
    w, cam = G.world(rtc, name)
    width, height, ns = cam.hsize, cam.vsize, 4
    dirs = rtc.ao_expand(ao)
    dw = gpu.upload(w)
    try:
        got = dw.render_gather(cam, ao, planes=("radiance",))["radiance"]
        planes = dw.render_aov(cam, ("index", "normal", "point"))
        index = planes["index"].reshape(-1)
        hit = index >= 0
        normal, point = planes["normal"].reshape(-1, 3)[hit], planes["point"].reshape(-1, 3)[hit]
        over = point + normal * 0.00000001   # Intersection::compute_vectors: point.add(normal.mul(EPSILON)), one product, one sum
        nx, ny, nz = normal[:, 0], normal[:, 1], normal[:, 2]
        sign = np.copysign(1.0, nz)
        a = -1.0 / (sign + nz)
        b = (nx * ny) * a
        t = np.stack([1.0 + ((sign * nx) * nx) * a, sign * b, -(sign * nx)], axis=1)
        s = np.stack([b, sign + ((ny * ny) * a), -ny], axis=1)
        recs = np.zeros((width * height, ns), dtype=A.HIT_DTYPE)
        recs["hit_index"] = -1
        rgb = np.zeros((width * height, ns, 3))
        for k, (lx, ly, lz) in enumerate(dirs):
            rays = np.concatenate([over, ((t * lx) + (s * ly)) + (normal * lz)], axis=1)
            col, hits = dw.color_at(rays, remaining=0, want_hits=True)
            recs[hit, k] = np.frombuffer(hits, dtype=A.HIT_DTYPE)[:len(rays)]
            rgb[hit, k] = col
    finally:
        dw.close()
    for i in range(0, len(over), max(1, len(over) // 50)):   # the vectorised restatement against the library's rtc_ao_ray
        assert np.array_equal(rtc.ao_ray(normal[i], over[i], dirs[1])[3:], ((t[i] * dirs[1][0]) + (s[i] * dirs[1][1])) + (normal[i] * dirs[1][2]))
    primary = np.zeros(width * height, dtype=A.HIT_DTYPE)
    primary["hit_index"] = index
    recs = np.ascontiguousarray(recs.reshape(-1))
    want = rtc.gather_from_hits((rtc.RtcHit * primary.size).from_buffer(primary), (rtc.RtcHit * recs.size).from_buffer(recs), rgb, None,
                                ns, math.inf, width, height, ASYNC, planes=("radiance",))["radiance"]
    assert 0 < int(hit.sum()) < hit.size and want.any() and (want.reshape(-1, 3)[hit] == 0.0).all(axis=1).any()
    d = np.argwhere(got != want)
    assert len(d) == 0, f"{len(d)} components differ, first at {d[0].tolist()}: got {got[tuple(d[0])]!r}, want {want[tuple(d[0])]!r}"
    assert got.tobytes() == want.tobytes()


def test_add_scaled_on_the_device(rtc, gpu):
    """rtc_canvas_add_scaled_device on a rendered frame and its bounce plane, both in device memory, is rtc_canvas_add_scaled
    byte for byte, and the frame goes on to the PNG encoder as it is."""
    torch = _torch()
    name, ao = "bleed", (math.inf, 4, 4)
    w, cam = G.world(rtc, name)
    width, height = cam.hsize, cam.vsize
    canvas = torch.zeros((height, width, 3), dtype=torch.float64, device="cuda:0")
    bounce = torch.zeros((height, width, 3), dtype=torch.float64, device="cuda:0")
    rgba = torch.zeros(width * height * 4, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    enc = rtc.ImageEncoder(gpu)
    try:
        beauty = dw.render(cam)
        host_bounce = dw.render_gather(cam, rtc.ao(*ao))["bounce"]
        dw.render_rows(cam, 0, height, canvas.data_ptr())
        dw.render_gather_device(cam, rtc.ao(*ao), {"bounce": bounce.data_ptr()})
        gpu.add_scaled_device(canvas.data_ptr(), bounce.data_ptr(), 0.8, width, height)
        gpu.canvas_to_rgba8_device(canvas.data_ptr(), width, height, 1.0, rgba.data_ptr())
        png = enc.encode_device("png", rgba.data_ptr(), width, height, 4)
        gpu.synchronize()
    finally:
        enc.close()
        dw.close()
    assert bounce.cpu().numpy().tobytes() == host_bounce.tobytes()
    composited = rtc.add_scaled(beauty, host_bounce, 0.8)
    assert canvas.cpu().numpy().tobytes() == composited.tobytes()
    assert not np.array_equal(composited, beauty) and np.array_equal(composited[host_bounce == 0.0], beauty[host_bounce == 0.0])
    assert (composited >= beauty).all()
    assert png == rtc.image_encode("png", rgba.cpu().numpy().reshape(height, width, 4)) and png[:8] == b"\x89PNG\r\n\x1a\n"


def test_errors_launch_nothing(rtc, gpu):
    """RTC_FLAG_LDS_TABLE is RTC_ERR_UNSUPPORTED (8); both planes NULL, a World of another context, a bad pass, a bad mode, a
    misaligned plane are RTC_ERR_ARG (4) — and the planes keep their fill."""
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    L = rtc.lib()
    w, cam = G.world(rtc, "bleed")
    n = cam.hsize * cam.vsize * 3
    dev = torch.full((2 * n + 1,), 7.0, dtype=torch.float64, device="cuda:0")
    host = np.full((2, cam.vsize, cam.hsize, 3), 7.0)
    torch.cuda.synchronize()
    B = abi.RtcGatherBuffers
    d_planes, h_planes = B(dev.data_ptr(), dev.data_ptr() + 8 * n), B(host[0].ctypes.data, host[1].ctypes.data)
    good = abi.RtcAo(1.5, 2, 2)
    dw = gpu.upload(w)
    other = rtc.Context(0)
    try:
        for entry, planes in ((L.rtc_render_gather_device, d_planes), (L.rtc_render_gather, h_planes)):
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, LDS_TABLE, C.byref(planes)) == 8
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, NO_CULL | LDS_TABLE, C.byref(planes)) == 8
            assert entry(other._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, C.byref(planes)) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), 2, 0, C.byref(planes)) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), None, ASYNC, 0, C.byref(planes)) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, None) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, C.byref(B(None, None))) == 4
            for radius, us, vs in [(0.0, 2, 2), (-1.0, 2, 2), (math.nan, 2, 2), (1.0, 0, 2), (1.0, 2, 0), (1.0, 257, 1), (1.0, 17, 16)]:
                assert entry(gpu._h, dw._h, C.byref(cam), C.byref(abi.RtcAo(radius, us, vs)), ASYNC, 0, C.byref(planes)) == 4, (radius, us, vs)
        assert L.rtc_render_gather_device(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, C.byref(B(dev.data_ptr() + 4, None))) == 4
        assert L.rtc_render_gather_device(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, C.byref(B(None, dev.data_ptr() + 4))) == 4
        gpu.synchronize()
        assert bool((dev == 7.0).all()) and (host == 7.0).all()
        # ... and the same arguments with nothing wrong write every pixel of both planes and nothing behind them
        assert L.rtc_render_gather_device(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, C.byref(d_planes)) == 0
        assert L.rtc_render_gather(gpu._h, dw._h, C.byref(cam), C.byref(good), ASYNC, 0, C.byref(h_planes)) == 0
        d = dev.cpu().numpy()
        assert d[:2 * n].tobytes() == host.tobytes() and d[2 * n] == 7.0 and not (host == 7.0).any()
        # compositing on the device refuses what the host entry refuses
        rgb = torch.ones(n, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        for strength in (-0.1, math.nan, math.inf):
            assert L.rtc_canvas_add_scaled_device(gpu._h, rgb.data_ptr(), dev.data_ptr(), strength, cam.hsize, cam.vsize) == 4
        assert L.rtc_canvas_add_scaled_device(gpu._h, None, dev.data_ptr(), 0.5, cam.hsize, cam.vsize) == 4
        assert L.rtc_canvas_add_scaled_device(gpu._h, rgb.data_ptr(), None, 0.5, cam.hsize, cam.vsize) == 4
        assert L.rtc_canvas_add_scaled_device(gpu._h, rgb.data_ptr() + 4, dev.data_ptr(), 0.5, cam.hsize, cam.vsize) == 4
        assert L.rtc_canvas_add_scaled_device(gpu._h, rgb.data_ptr(), dev.data_ptr() + 4, 0.5, cam.hsize, cam.vsize) == 4
        gpu.synchronize()
        assert bool((rgb == 1.0).all())
    finally:
        other.close()
        dw.close()


def test_stats_are_not_touched(rtc, gpu):
    w, cam = G.world(rtc, "bleed")
    dw = gpu.upload(w)
    try:
        dw.render(cam, with_stats=True)
        before = gpu.stats(extended=True)
        assert before["rays_primary"] > 0
        dw.render_gather(cam, rtc.ao(1.5, 2, 2))
        dw.render_gather(cam, rtc.ao(1.5, 2, 2), flags=NO_CULL)
        assert gpu.stats(extended=True) == before
    finally:
        dw.close()
