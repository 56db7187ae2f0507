"""Motion blur on the HIP path (include/rtc.h "Motion blur": rtc_canvas_average_device, rtc_shutter_*, k_average_over).

Three references, each computed once and never written to:
  * the averaging kernel against the host statement rtc_canvas_average, byte for byte, on adversarial values;
  * a shutter frame against rtc_canvas_average of the library's OWN sub-frames — DeviceWorld.render / render_lens of
    rtc_shutter_shapes / rtc_shutter_camera, one World and camera per shutter time — byte for byte, stats summed;
  * the flat World against the mean, in sample order, of the oracle's renders of the expanded Worlds: bound 1e-12 (the
    project's TIGHT_TOL per light: every sub-frame is within it, both sides add the n sub-frames in the same order and
    divide once, so the mean is within it too), non-zero masks equal.
Frames are 70x45 (partial 8x8 tiles on both edges) or 40x24 for the 299-sphere world."""
import functools
import importlib

import numpy as np
import pytest

from test_host_png import decode as decode_png
from test_host_shutter import adversarial_frames

pytestmark = pytest.mark.gpu

W, H = 70, 45
TIGHT_TOL = 1e-12
NO_CULL, LDS_TABLE = 1, 4
ERR_SINGULAR, ERR_ARG, ERR_UNSUPPORTED = 1, 4, 8
MODE_RENDER, MODE_RENDER_ASYNC = 0, 1
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "pixels", "pixels_resample", "rays_primary_proven_miss")
CAST = COUNTERS[:-1]   # what a culled and a brute-force frame share: the proof of black tiles belongs to binned launches alone
AMONG = ((1.5, 1.25, 4.0), (0.2, 0.45, 0.7))
THIRD = ((6.0, 7.0, -3.0), (0.4, 0.3, 0.3))
A33 = ((-11.5, 10.0, -11.5), (3.0, 0.0, 0.0), (0.0, 0.5, 3.0), 3, 3, (1.0, 0.95, 0.9))
L22 = (0.3, 9.0, 2, 2)


def _scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


@functools.lru_cache(maxsize=None)
def _scene(rtc, name, lights="one", samples=1):
    """(World, camera at the shutter's opening, camera at its close, motions): several spheres move by more than their
    radius (synthetic radii are at most 0.5, mixed scales at most 1.3), and the camera moves."""
    S, M = _scenes(rtc), rtc.Matrix
    if name == "flat": w, cam = S.synthetic(39, W, H, samples=samples)
    elif name == "mixed": w, cam = S.mixed(W, H)
    elif name == "s300": w, cam = S.synthetic(299, 40, 24)
    else: raise KeyError(name)
    if lights == "three":
        w.add_light(rtc.light(*AMONG)).add_light(rtc.light(*THIRD))
    elif lights == "area":
        w.lights = [rtc.area_light(*A33)]
    moves = {0: (1.1, 0.0, 0.3), 1: (-0.9, 0.6, 0.0), 2: (0.0, 0.8, -0.7), 5: (1.6, 0.0, 0.0), 7: (-1.2, 0.2, 0.9), 11: (0.7, 1.0, 0.0)}
    motions = []
    for i, d in moves.items():
        opened = M(list(w.shapes[i].inv)).inverse()
        motions.append(rtc.motion(i, opened, opened.translation(*d)))
    if name == "mixed": frm, to, fov = (0.5, 2.5, -7.0), (0.0, 1.0, 1.0), 1.0
    else: frm, to, fov = (0.0, 2.0, -8.0), (0.0, 1.0, 5.0), 0.7
    cam_close = rtc.camera(cam.hsize, cam.vsize, fov, M.make_view_transform((frm[0] + 0.5, frm[1] + 0.2, frm[2]), to, (0.0, 1.0, 0.0)), samples)
    return w, cam, cam_close, tuple(motions)


def _sum_stats(total, st):
    for k in COUNTERS:
        total[k] = total.get(k, 0) + st.get(k, 0)


@functools.lru_cache(maxsize=None)
def _reference(rtc, gpu, name, n, lights="one", lens_spec=None, samples=1, mode=MODE_RENDER_ASYNC, flags=0):
    """rtc_canvas_average of the library's own sub-frames, and their counters summed."""
    w, cam, cam_close, motions = _scene(rtc, name, lights, samples)
    lens = rtc.lens(*lens_spec) if lens_spec else None
    frames, total = [], {}
    dw = gpu.upload(rtc.shutter_shapes(w, motions, n, 0))
    try:
        for k in range(n):
            if k:
                dw.update(rtc.shutter_shapes(w, motions, n, k))
            ck = rtc.shutter_camera(cam, cam_close, n, k)
            if lens is not None:
                f, st = dw.render_lens(ck, lens, mode=mode, flags=flags, with_stats=True)
            else:
                f, st = dw.render(ck, mode=mode, flags=flags, with_stats=True)
            st = dict(st, rays_primary_proven_miss=gpu.stats(extended=True)["rays_primary_proven_miss"])
            frames.append(f.copy())
            _sum_stats(total, st)
    finally:
        dw.close()
    mean = rtc.canvas_average(np.stack(frames))
    mean.setflags(write=False)
    return mean, total


def _same_stats(st, total, what):
    got = {k: st.get(k, 0) for k in COUNTERS}
    print(f"{what}: stats {got}")
    assert got == {k: total.get(k, 0) for k in COUNTERS}, what


def _check_frame(rtc, gpu, sh, name, n, lights="one", lens_spec=None, samples=1, mode=MODE_RENDER_ASYNC):
    w, cam, cam_close, motions = _scene(rtc, name, lights, samples)
    lens = rtc.lens(*lens_spec) if lens_spec else None
    want, total = _reference(rtc, gpu, name, n, lights, lens_spec, samples, mode)
    got, st = sh.render(w, motions, cam, n, cam_close=cam_close, lens=lens, mode=mode, with_stats=True)
    brute, sb = sh.render(w, motions, cam, n, cam_close=cam_close, lens=lens, mode=mode, flags=NO_CULL, with_stats=True)
    what = f"{name} n={n} lights={lights} lens={lens_spec} samples={samples} mode={mode}"
    print(f"{what}: max|frame - host mean of sub-frames| = {float(np.max(np.abs(got - want))):.3e}")
    assert got.tobytes() == want.tobytes(), what
    assert brute.tobytes() == got.tobytes(), what
    _same_stats(st, total, what)
    assert {k: sb.get(k, 0) for k in CAST} == {k: st.get(k, 0) for k in CAST}, what
    assert got.any() and st["pixels"] == n * (cam.hsize - (mode == MODE_RENDER)) * (cam.vsize - (mode == MODE_RENDER))
    return got


@pytest.fixture(scope="module")
def sh(gpu):
    s = gpu.shutter()
    yield s
    s.close()


# ---- the averaging kernel
@functools.lru_cache(maxsize=None)
def _frames_and_mean(rtc, n, count):
    frames = adversarial_frames(n, count)
    with np.errstate(all="ignore"):
        want = rtc.canvas_average(frames)
    frames.setflags(write=False)
    want.setflags(write=False)
    return frames, want


@pytest.mark.parametrize("count", [1, 2, 3, 191, 4099, 4100])
@pytest.mark.parametrize("n", [1, 2, 8, 9, 19, 256])
def test_average_kernel_is_the_host_statement_byte_for_byte(rtc, gpu, n, count):
    """Both layouts: buffers as allocated (the 16-byte path for one frame or an even count: 2 and 4100; an odd count puts
    every other frame off 16 bytes) and both pushed 8 bytes on (the scalar path at every count)."""
    import torch
    frames, want = _frames_and_mean(rtc, n, count)
    for off in (0, 1):
        d_in = torch.zeros(n * count + 1, dtype=torch.float64, device="cuda:0")
        d_in[off:off + n * count] = torch.from_numpy(frames.reshape(-1).copy())
        d_out = torch.full((count + 3,), 7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        gpu.canvas_average_device(d_in.data_ptr() + 8 * off, n, count, d_out.data_ptr() + 8 * off)
        gpu.synchronize()
        got = d_out.cpu().numpy()
        assert got[off:off + count].tobytes() == want.tobytes(), (n, count, off)
        assert (np.delete(got, np.s_[off:off + count]) == 7.0).all(), "wrote outside its output"


def test_average_kernel_arguments(rtc, gpu):
    import torch
    d = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    f = rtc.lib().rtc_canvas_average_device
    assert f(gpu._h, d.data_ptr(), 0, 4, d.data_ptr() + 256) == ERR_ARG
    assert f(gpu._h, d.data_ptr(), 257, 4, d.data_ptr() + 256) == ERR_ARG
    assert f(gpu._h, None, 2, 4, d.data_ptr()) == ERR_ARG and f(gpu._h, d.data_ptr(), 2, 4, None) == ERR_ARG
    assert f(gpu._h, d.data_ptr() + 4, 2, 4, d.data_ptr() + 256) == ERR_ARG   # not 8-byte aligned


# ---- the frame = the host average of the library's own sub-frames
@pytest.mark.parametrize("n", [3, 8, 9, 19])
@pytest.mark.parametrize("name", ["flat", "mixed", "s300"])
def test_frame_is_the_host_mean_of_the_sub_frames(rtc, gpu, sh, name, n):
    _check_frame(rtc, gpu, sh, name, n)


def test_launch_paths_of_the_three_worlds(rtc, gpu, sh):
    for name, source, refl in (("flat", 3, False), ("mixed", 3, True), ("s300", 4, False)):
        w, cam, cam_close, motions = _scene(rtc, name)
        sh.render(w, motions, cam, 2, cam_close=cam_close)
        info = gpu.last_launch_info()
        assert info["source"] == source and info["reflective"] is refl and info["lens_samples"] == 0, (name, info)


@pytest.mark.parametrize("name", ["flat", "s300"])
def test_three_point_lights(rtc, gpu, sh, name):
    _check_frame(rtc, gpu, sh, name, 3, lights="three")


@pytest.mark.parametrize("name", ["flat", "s300"])
def test_a_3x3_area_light_through_the_light_table(rtc, gpu, sh, name):
    _check_frame(rtc, gpu, sh, name, 3, lights="area")
    assert gpu.last_launch_info()["light_table"] is True


@pytest.mark.parametrize("name", ["flat", "mixed"])
def test_a_2x2_lens(rtc, gpu, sh, name):
    _check_frame(rtc, gpu, sh, name, 3, lens_spec=L22)
    assert gpu.last_launch_info()["lens_samples"] == 4


def test_four_antialiasing_samples_without_a_lens(rtc, gpu, sh):
    _check_frame(rtc, gpu, sh, "flat", 3, samples=4)


# ---- oracle parity
@functools.lru_cache(maxsize=None)
def _oracle_mean(rtc, O, n):
    w, cam, cam_close, motions = _scene(rtc, "flat")
    total = np.zeros((cam.vsize, cam.hsize, 3))
    for k in range(n):
        wk, ck = rtc.shutter_shapes(w, motions, n, k), rtc.shutter_camera(cam, cam_close, n, k)
        total = total + O.render(wk.array(), len(wk), wk.light, ck, mode=1, nthreads=8)   # 0.0 + f0 + f1 + ...: sample order
    mean = total / float(n)
    mid_w, mid_c = rtc.shutter_shapes(w, motions, 1, 0), rtc.shutter_camera(cam, cam_close, 1, 0)   # t = 0.5
    still = O.render(mid_w.array(), len(mid_w), mid_w.light, mid_c, mode=1, nthreads=8)
    mean.setflags(write=False)
    still.setflags(write=False)
    return mean, still


def test_flat_world_matches_the_oracle(rtc, gpu, sh, O):
    n = 5
    w, cam, cam_close, motions = _scene(rtc, "flat")
    want, still = _oracle_mean(rtc, O, n)
    got = sh.render(w, motions, cam, n, cam_close=cam_close)
    err, moved = float(np.max(np.abs(got - want))), float(np.max(np.abs(got - still)))
    print(f"flat n={n}: max|gpu - oracle mean| = {err:.3e} (bound {TIGHT_TOL:.1e}); max|frame - still at t=0.5| = {moved:.3e}")
    assert err <= TIGHT_TOL
    assert np.array_equal(got != 0, want != 0)
    assert moved > 0.05   # the motion shows


# ---- outputs
@pytest.mark.parametrize("name,n", [("flat", 3), ("s300", 9)])
def test_8_bit_outputs_are_the_host_conversions_of_the_mean(rtc, gpu, sh, name, n):
    import torch
    w, cam, cam_close, motions = _scene(rtc, name)
    mean, _ = _reference(rtc, gpu, name, n)
    h, wd = cam.vsize, cam.hsize
    want8 = rtc.color_scale255(mean)
    assert sh.render_rgb8(w, motions, cam, n, cam_close=cam_close).tobytes() == want8.tobytes()
    for gamma in (1.0, 2.2):
        want = rtc.to_rgba8(mean, gamma)
        assert sh.render_rgba8(w, motions, cam, n, gamma, cam_close=cam_close).tobytes() == want.tobytes(), gamma
    assert np.array_equal(rtc.to_rgba8(mean, 1.0)[..., :3], want8)
    # the device entry: all three at once, then each 8-bit output alone (no f64 mean is written then)
    d64 = torch.zeros((h, wd, 3), dtype=torch.float64, device="cuda:0")
    d8 = torch.zeros((h, wd, 3), dtype=torch.uint8, device="cuda:0")
    d32 = torch.zeros((h, wd, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    sh.render_device(w, motions, cam, n, d_rgb=d64.data_ptr(), d_rgb8=d8.data_ptr(), d_rgba8=d32.data_ptr(), gamma=2.2, cam_close=cam_close)
    gpu.synchronize()
    assert d64.cpu().numpy().tobytes() == mean.tobytes()
    assert d8.cpu().numpy().tobytes() == want8.tobytes() and d32.cpu().numpy().tobytes() == rtc.to_rgba8(mean, 2.2).tobytes()
    d8.zero_(); d32.zero_()
    torch.cuda.synchronize()
    sh.render_device(w, motions, cam, n, d_rgb8=d8.data_ptr(), cam_close=cam_close)
    sh.render_device(w, motions, cam, n, d_rgba8=d32.data_ptr(), gamma=1.0, cam_close=cam_close)
    gpu.synchronize()
    assert d8.cpu().numpy().tobytes() == want8.tobytes() and d32.cpu().numpy().tobytes() == rtc.to_rgba8(mean, 1.0).tobytes()
    with pytest.raises(rtc.RtcError) as e:
        sh.render_device(w, motions, cam, n, cam_close=cam_close)   # no output at all
    assert e.value.status == ERR_ARG


def test_an_odd_number_of_pixels(rtc, gpu, sh):
    """15 x 9 = 135 pixels, 405 doubles: the ring canvases are padded to 16 bytes, the last element and the last pixel take
    the scalar tail; 9 samples, so the sum is carried once."""
    S, n = _scenes(rtc), 9
    w, cam = S.synthetic(12, 15, 9)
    opened = rtc.Matrix(list(w.shapes[3].inv)).inverse()
    motions = [rtc.motion(3, opened, opened.translation(-1.5, 0.5, 0.0))]
    frames = []
    dw = gpu.upload(w)
    try:
        for k in range(n):
            dw.update(rtc.shutter_shapes(w, motions, n, k))
            frames.append(dw.render(cam).copy())
    finally:
        dw.close()
    mean = rtc.canvas_average(np.stack(frames))
    assert sh.render(w, motions, cam, n).tobytes() == mean.tobytes() and mean.any()
    assert sh.render_rgb8(w, motions, cam, n).tobytes() == rtc.color_scale255(mean).tobytes()
    assert sh.render_rgba8(w, motions, cam, n, 2.2).tobytes() == rtc.to_rgba8(mean, 2.2).tobytes()


# ---- ring and ordering
def test_mode_render_at_19_samples_straight_after_another_scene(rtc, gpu, sh):
    """RTC_MODE_RENDER leaves the last row and column black: nothing of the frame rendered just before (another scene, every
    pixel written, the ring full) may show through there."""
    w0, cam0, close0, motions0 = _scene(rtc, "mixed")
    sh.render(w0, motions0, cam0, 9, cam_close=close0)
    got = _check_frame(rtc, gpu, sh, "flat", 19, mode=MODE_RENDER)
    assert not got[-1].any() and not got[:, -1].any() and got[:-1, :-1].any()


def test_pipeline_depth_3_gives_the_bytes_of_depth_1(rtc, gpu, sh):
    cases = [("flat", 19, MODE_RENDER), ("s300", 9, MODE_RENDER_ASYNC), ("mixed", 8, MODE_RENDER_ASYNC)]
    gpu.set_pipeline(3)
    try:
        for name, n, mode in cases:
            w, cam, cam_close, motions = _scene(rtc, name)
            want, total = _reference(rtc, gpu, name, n, mode=mode)   # (cached references were made at depth 1; a new one: same bytes by contract)
            for _ in range(2):   # twice: the second frame's renders refill the ring the first frame's last pass reads
                got, st = sh.render(w, motions, cam, n, cam_close=cam_close, mode=mode, with_stats=True)
                assert got.tobytes() == want.tobytes(), (name, n)
                _same_stats(st, total, f"depth 3 {name} n={n}")
        assert gpu.last_launch_info()["lane"] in (0, 1, 2)
    finally:
        gpu.set_pipeline(1)


def test_an_ordinary_world_of_the_context_is_left_alone(rtc, gpu, sh):
    w, cam, cam_close, motions = _scene(rtc, "flat")
    dw = gpu.upload(w)
    try:
        before = dw.render(cam).copy()
        sh.render(w, motions, cam, 9, cam_close=cam_close)
        assert dw.render(cam).tobytes() == before.tobytes()
    finally:
        dw.close()


def test_a_second_frame_with_more_shapes_than_the_first(rtc, gpu):
    """A fresh shutter: its World is created by a 26-shape frame and has to grow for the 300-shape one (and its scratch
    shrinks from 70x45 to 40x24 without a reallocation)."""
    s = gpu.shutter()
    try:
        for name, n in (("mixed", 3), ("s300", 9), ("mixed", 3)):
            w, cam, cam_close, motions = _scene(rtc, name)
            want, _ = _reference(rtc, gpu, name, n)
            assert s.render(w, motions, cam, n, cam_close=cam_close).tobytes() == want.tobytes(), name
    finally:
        s.close()


def test_png_encoder_straight_behind_render_device(rtc, gpu, sh):
    import torch
    w, cam, cam_close, motions = _scene(rtc, "flat")
    mean, _ = _reference(rtc, gpu, "flat", 9)
    d8 = torch.zeros((cam.vsize, cam.hsize, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    enc = rtc.ImageEncoder(gpu)
    try:
        sh.render_device(w, motions, cam, 9, d_rgb8=d8.data_ptr(), cam_close=cam_close)
        png = enc.encode_device("png", d8.data_ptr(), cam.hsize, cam.vsize, 3)   # no synchronisation in between
    finally:
        enc.close()
    assert decode_png(png)[0].tobytes() == rtc.color_scale255(mean).tobytes()


# ---- limits and errors
def test_256_samples(rtc, gpu, sh):
    S = _scenes(rtc)
    w, cam = S.synthetic(12, 16, 10)
    opened = rtc.Matrix(list(w.shapes[0].inv)).inverse()
    motions = [rtc.motion(0, opened, opened.translation(2.0, 0.0, 0.0))]
    frames = []
    dw = gpu.upload(w)
    try:
        for k in range(256):
            dw.update(rtc.shutter_shapes(w, motions, 256, k))
            frames.append(dw.render(cam).copy())
    finally:
        dw.close()
    got, st = sh.render(w, motions, cam, 256, with_stats=True)
    assert got.tobytes() == rtc.canvas_average(np.stack(frames)).tobytes()
    assert st["pixels"] == 256 * 160 and st["rays_primary"] == 256 * 160


def _status(rtc, fn, *a, **kw):
    with pytest.raises(rtc.RtcError) as e:
        fn(*a, **kw)
    return e.value.status


def test_limits_and_errors(rtc, gpu, sh):
    M = rtc.Matrix
    w, cam, cam_close, motions = _scene(rtc, "flat")
    assert _status(rtc, sh.render, w, motions, cam, 257) == ERR_ARG
    assert _status(rtc, sh.render, w, motions, cam, 0) == ERR_ARG
    aa = rtc.camera(W, H, 0.7, samples=4)
    assert _status(rtc, sh.render, w, motions, aa, 3, lens=rtc.lens(*L22)) == ERR_ARG
    assert _status(rtc, sh.render, w, motions, cam, 3, lens=rtc.lens(*L22), flags=NO_CULL | LDS_TABLE) == ERR_UNSUPPORTED
    w3, cam3, close3, motions3 = _scene(rtc, "flat", "three")
    assert _status(rtc, sh.render, w3, motions3, cam3, 3, flags=NO_CULL | LDS_TABLE) == ERR_UNSUPPORTED
    assert _status(rtc, sh.render, w, motions, cam, 3, cam_close=rtc.camera(W + 1, H, 0.7)) == ERR_ARG
    assert _status(rtc, sh.render, w, [rtc.motion(len(w), M.identity(), M.identity())], cam, 3) == ERR_ARG
    assert _status(rtc, sh.render_rgba8, w, motions, cam, 3, 0.0) == ERR_ARG
    # a singular matrix at the LAST shutter time (n = 3: t = 5/6, scale 1 - 1.2 * 5/6 = 0): nothing is launched
    flat_at_the_end = [rtc.motion(0, M.identity(), M.identity().scaling(-0.2, -0.2, -0.2))]
    gpu.reset_stats()
    dw = gpu.upload(w)
    try:
        dw.render(cam)
        before, launches = gpu.stats(extended=True), gpu.last_launch_info()
        assert before["pixels"] == W * H
        assert _status(rtc, sh.render, w, flat_at_the_end, cam, 3, with_stats=True) == ERR_SINGULAR
        assert gpu.stats(extended=True) == before and gpu.last_launch_info() == launches
    finally:
        dw.close()
    # and the shutter still works
    want, _ = _reference(rtc, gpu, "flat", 3)
    assert sh.render(w, motions, cam, 3, cam_close=cam_close).tobytes() == want.tobytes()
