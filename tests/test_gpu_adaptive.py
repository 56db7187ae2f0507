"""Edge-adaptive anti-aliasing on the HIP path (rtc_adaptive_mask_device, rtc_render_adaptive[_device]; k_aa_mask, k_aa_scan,
k_aa_list, k_aa_rays, k_aa_resolve). The mask is compared with the host statement's bytes (pinned without a GPU by
tests/test_host_adaptive.py), the frame bit for bit with the route composed of the library's own public pieces — render, the
host mask, host rays, color_at, the mean — and, within the project's colour tolerance, with the CPU oracle."""
import ctypes as C
import math

import numpy as np
import pytest

import adaptive_cases as AC

pytestmark = pytest.mark.gpu

RENDER, ASYNC = 0, 1
NO_CULL, LDS_TABLE = 1, 4
TOL = 1e-12   # the project's colour tolerance against the oracle


def _torch():
    import torch
    return torch


def _dev_bytes(torch, nbytes):
    """A device allocation of nbytes + 64, every byte 0x5A: what a buffer holds where nothing was written."""
    return torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")


def _put(torch, buf, offset, arr):
    a = np.ascontiguousarray(arr)
    buf[offset:offset + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    return buf.data_ptr() + offset


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    d = np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
    assert len(d) == 0, f"{what}: {len(d)} values differ, first at {d[0].tolist()}: got {got[tuple(d[0])]!r}, want {want[tuple(d[0])]!r}"


# ---- the mask kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AC.CANVAS_NAMES + AC.TILE_NAMES)
def test_mask_kernel_gives_the_host_bytes(rtc, gpu, name):
    torch = _torch()
    rgb = AC.canvas(name)
    h, w = rgb.shape[:2]
    for rgb_off, mask_off in ((0, 0), (8, 8), (8, 3)):
        d_rgb = _dev_bytes(torch, rgb.nbytes)
        p_rgb = _put(torch, d_rgb, rgb_off, rgb)
        assert d_rgb.data_ptr() % 16 == 0
        for mode in (RENDER, ASYNC):
            for threshold in AC.THRESHOLDS:
                d_mask = _dev_bytes(torch, w * h)
                torch.cuda.synchronize()
                gpu.adaptive_mask_device(p_rgb, w, h, mode, threshold, d_mask.data_ptr() + mask_off)
                gpu.synchronize()
                out = d_mask.cpu().numpy()
                want = rtc.adaptive_mask(rgb, mode, threshold)
                got = out[mask_off:mask_off + w * h].reshape(h, w)
                assert got.tobytes() == want.tobytes(), f"{name} mode {mode} threshold {threshold} offsets {rgb_off}/{mask_off}: {np.argwhere(got != want)[:4].tolist()}"
                assert (out[:mask_off] == 0x5A).all() and (out[mask_off + w * h:] == 0x5A).all(), f"{name}: bytes outside the mask were written"
        back = d_rgb.cpu().numpy()
        assert back[rgb_off:rgb_off + rgb.nbytes].tobytes() == rgb.tobytes() and (back[:rgb_off] == 0x5A).all() and (back[rgb_off + rgb.nbytes:] == 0x5A).all()


def test_mask_device_refuses_bad_arguments(rtc, gpu):
    torch = _torch()
    rgb = AC.canvas("random-37x19")
    d_rgb, d_mask = _dev_bytes(torch, rgb.nbytes), _dev_bytes(torch, 37 * 19)
    p = _put(torch, d_rgb, 0, rgb)
    torch.cuda.synchronize()
    L = rtc.lib()
    VP = C.c_void_p
    for args in ((None, VP(p), 37, 19, 1, 0.01, VP(d_mask.data_ptr())), (gpu._h, None, 37, 19, 1, 0.01, VP(d_mask.data_ptr())),
                 (gpu._h, VP(p), 37, 19, 1, 0.01, None), (gpu._h, VP(p + 4), 37, 19, 1, 0.01, VP(d_mask.data_ptr())),
                 (gpu._h, VP(p), 37, 19, 2, 0.01, VP(d_mask.data_ptr())), (gpu._h, VP(p), 37, 19, 1, math.nan, VP(d_mask.data_ptr())),
                 (gpu._h, VP(p), 65536, 65536, 1, 0.01, VP(d_mask.data_ptr()))):
        assert L.rtc_adaptive_mask_device(*args) == 4
    gpu.synchronize()
    assert (d_mask.cpu().numpy() == 0x5A).all()


# ---- the composed route ------------------------------------------------------------------------------------------------------
_worlds, _composed = {}, {}


def _device_world(rtc, gpu, name):
    if name not in _worlds:
        if name == "updated":
            dw = rtc.DeviceWorld(gpu, AC.world(rtc, name, before_update=True))
            dw.render(AC.camera(rtc, name, 9, 5))   # a launch reads the first generation before the update replaces it
            dw.update(AC.world(rtc, name))
        else:
            dw = rtc.DeviceWorld(gpu, AC.world(rtc, name))
        _worlds[name] = dw
    return _worlds[name]


def _mean(colours):
    """Color::average_over of an (P, n, 3) array: sums from 0.0 in sample order, one division."""
    s = np.zeros((colours.shape[0], 3))
    for k in range(colours.shape[1]):
        s = s + colours[:, k]
    return s / float(colours.shape[1])


def _rays(rtc, cam, pixels, spec):
    n = spec.usteps * spec.vsteps
    offs = [rtc.adaptive_offset(spec, k) for k in range(n)]
    rays = np.empty((len(pixels) * n, 6))
    i = 0
    for y, x in pixels:   # pixel-major, samples innermost
        for xo, yo in offs:
            rays[i] = rtc.ray_for_pixel(cam, int(x), int(y), xo, yo)
            i += 1
    return rays


def _compose(rtc, gpu, name, size, steps, mode, threshold=0.01):
    """(frame, mask) by the public pieces: render -> rtc.adaptive_mask -> rtc.ray_for_pixel -> color_at -> the mean. Read-only."""
    key = (name, size, steps, mode, threshold)
    if key not in _composed:
        dw = _device_world(rtc, gpu, name)
        cam = AC.camera(rtc, name, *size)
        spec = rtc.adaptive(threshold, *steps)
        frame = dw.render(cam, mode=mode).copy()
        mask = rtc.adaptive_mask(frame, mode, threshold)
        pixels = np.argwhere(mask != 0)
        if len(pixels):
            n = steps[0] * steps[1]
            colours = dw.color_at(_rays(rtc, cam, pixels, spec), remaining=5).reshape(len(pixels), n, 3)
            frame[pixels[:, 0], pixels[:, 1]] = _mean(colours)
        frame.setflags(write=False)
        mask.setflags(write=False)
        _composed[key] = (frame, mask)
    return _composed[key]


def _check_against_composed(rtc, gpu, name, size, steps, mode, flags=0, max_rays=0, threshold=0.01):
    dw = _device_world(rtc, gpu, name)
    cam = AC.camera(rtc, name, *size)
    want, want_mask = _compose(rtc, gpu, name, size, steps, mode, threshold)
    n = steps[0] * steps[1]
    got, info, mask = dw.render_adaptive(cam, rtc.adaptive(threshold, steps[0], steps[1], max_rays), mode=mode, flags=flags, with_mask=True)
    what = f"{name} {size} {steps} mode {mode} flags {flags} max_rays {max_rays}"
    assert mask.tobytes() == want_mask.tobytes(), what   # the host mask of the library's own centre-sample frame
    _same_bits(got, want, what)
    refined = int(want_mask.sum())
    assert info == {"pixels_refined": refined, "rays_refined": refined * n, "launches": AC.expected_launches(refined, n, max_rays)}, what
    return info


@pytest.mark.parametrize("steps", AC.SPECS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("size", AC.FRAME_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", AC.WORLDS)
def test_adaptive_frame_equals_the_composed_route(rtc, gpu, name, size, steps):
    for mode in (RENDER, ASYNC):
        for flags in (0, NO_CULL):
            info = _check_against_composed(rtc, gpu, name, size, steps, mode, flags)
            assert 0 < info["pixels_refined"] < size[0] * size[1]


@pytest.mark.parametrize("name", AC.WORLDS)
def test_256_samples_on_a_tiny_frame(rtc, gpu, name):
    for mode in (RENDER, ASYNC):
        for flags in (0, NO_CULL):
            info = _check_against_composed(rtc, gpu, name, AC.TINY, (16, 16), mode, flags)
            assert 0 < info["pixels_refined"] < AC.TINY[0] * AC.TINY[1]


def test_chunks_give_the_unchunked_bytes(rtc, gpu):
    """max_rays that forces at least three launches, the last one short; and one pixel per launch on the tiny frame."""
    size, steps = (37, 19), (3, 5)
    refined = int(_compose(rtc, gpu, "trio", size, steps, ASYNC)[1].sum())
    per = refined // 3 - 1          # pixels per launch: three full chunks and a short fourth
    assert per >= 1 and refined % per != 0 and refined // per >= 3
    for max_rays in (per * 15, per * 15 + 14):   # (the second: max_rays is no multiple of n, floor applies)
        info = _check_against_composed(rtc, gpu, "trio", size, steps, ASYNC, max_rays=max_rays)
        assert info["launches"] == refined // per + 1 >= 4
    for steps in ((2, 2), (16, 16)):
        n = steps[0] * steps[1]
        info = _check_against_composed(rtc, gpu, "grid290", AC.TINY, steps, RENDER, max_rays=n)
        assert info["launches"] == info["pixels_refined"] > 1


def test_thresholds_at_the_ends(rtc, gpu):
    dw = _device_world(rtc, gpu, "trio")
    for size in ((37, 19), (1, 1), (1, 7), (7, 1)):
        cam = AC.camera(rtc, "trio", *size)
        for mode in (RENDER, ASYNC):
            base = dw.render(cam, mode=mode)
            got, info, mask = dw.render_adaptive(cam, rtc.adaptive(math.inf, 2, 2), mode=mode, with_mask=True)
            _same_bits(got, base, f"+inf {size} mode {mode}")   # rtc_render's frame, byte for byte
            assert info == {"pixels_refined": 0, "rays_refined": 0, "launches": 0} and not mask.any()
            got, info, mask = dw.render_adaptive(cam, rtc.adaptive(-1.0, 2, 2), mode=mode, with_mask=True)
            rw, rh = (size[0] - 1, size[1] - 1) if mode == RENDER else size
            want = np.zeros((size[1], size[0]), dtype=np.uint8)
            if rw > 0 and rh > 0 and rw * rh > 1:
                want[:rh, :rw] = 1       # every pixel of R that has a neighbour in R
            assert mask.tolist() == want.tolist(), f"-1 {size} mode {mode}"
            assert info["pixels_refined"] == int(want.sum())
            if size != (37, 19) and mode == RENDER:
                assert info["launches"] == 0
                _same_bits(got, base, f"-1 {size} mode {mode}")
    _check_against_composed(rtc, gpu, "trio", (37, 19), (2, 2), ASYNC, threshold=-1.0)
    _check_against_composed(rtc, gpu, "trio", (37, 19), (2, 2), RENDER, threshold=-1.0)


# ---- the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [RENDER, ASYNC])
@pytest.mark.parametrize("name", AC.ORACLE_WORLDS)
def test_against_the_oracle(rtc, gpu, O, name, mode):
    """Refined pixels against the mean of the oracle's color_at over the n normative rays, unrefined ones against its centre
    colour; the library's own mask says which is which, so no pixel near the threshold is left out."""
    size, steps = (37, 19), (2, 2)
    dw = _device_world(rtc, gpu, name)
    cam = AC.camera(rtc, name, *size)
    spec = rtc.adaptive(0.01, *steps)
    got, info, mask = dw.render_adaptive(cam, spec, mode=mode, with_mask=True)
    w = AC.world(rtc, name)
    arr, n_shapes, lgt = w.array(), len(w), w.samples()[0]
    want = O.render(arr, n_shapes, lgt, cam, mode=mode)
    pixels = np.argwhere(mask != 0)
    assert 0 < len(pixels) < size[0] * size[1]
    rays = _rays(rtc, cam, pixels, spec)
    colours = np.array([O.color_at(arr, n_shapes, lgt, tuple(r), 5) for r in rays]).reshape(len(pixels), 4, 3)
    want[pixels[:, 0], pixels[:, 1]] = _mean(colours)
    err = np.abs(got - want).max()
    print(f"{name} mode {mode}: {len(pixels)} refined, max |device - oracle| = {err:.3e}")
    assert err <= TOL


def test_2x2_everywhere_against_the_four_fixed_subsamples(rtc, gpu):
    """A 2 x 2 spec at threshold -1 renders every pixel as rtc_render does with cam.samples = 4 and no resample: the same four
    offsets in the same order, the same mean. Interior pixels, within the colour tolerance; whether they are in fact equal bit
    for bit is printed."""
    for name in ("trio", "grid290"):
        dw = _device_world(rtc, gpu, name)
        cam = AC.camera(rtc, name, 37, 19)
        got, info = dw.render_adaptive(cam, rtc.adaptive(-1.0, 2, 2))
        assert info["pixels_refined"] == 37 * 19
        cam4 = AC.camera(rtc, name, 37, 19)
        cam4.samples = 4
        want = dw.render(cam4)
        a, b = got[1:-1, 1:-1], want[1:-1, 1:-1]
        print(f"{name}: max |adaptive 2x2 - samples=4| = {np.abs(a - b).max():.3e}, byte-equal: {a.tobytes() == b.tobytes()}")
        assert np.abs(a - b).max() <= TOL


# ---- the entry points --------------------------------------------------------------------------------------------------------
def test_second_and_smaller_calls_allocate_nothing(rtc, gpu):
    L = rtc.lib()
    L.rtc_debug_render_allocs.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]

    def allocs():
        out = C.c_ulonglong(0)
        assert L.rtc_debug_render_allocs(gpu._h, C.byref(out)) == 0
        return out.value

    _check_against_composed(rtc, gpu, "grid290", (96, 54), (4, 4), ASYNC)
    before = allocs()
    _check_against_composed(rtc, gpu, "grid290", (96, 54), (4, 4), ASYNC)
    _check_against_composed(rtc, gpu, "grid290", (37, 19), (2, 2), RENDER)
    _check_against_composed(rtc, gpu, "grid290", (37, 19), (4, 4), ASYNC, max_rays=160)
    assert allocs() == before


def test_device_entry_leaves_the_frame_in_the_callers_buffer(rtc, gpu):
    torch = _torch()
    size, steps = (37, 19), (4, 4)
    dw = _device_world(rtc, gpu, "two-lights")
    cam = AC.camera(rtc, "two-lights", *size)
    want, want_mask = _compose(rtc, gpu, "two-lights", size, steps, ASYNC)
    px = size[0] * size[1]
    for with_mask in (True, False):
        d_rgb, d_mask = _dev_bytes(torch, want.nbytes), _dev_bytes(torch, px)
        torch.cuda.synchronize()
        info = dw.render_adaptive_device(cam, rtc.adaptive(0.01, *steps), d_rgb.data_ptr() + 8, d_mask.data_ptr() + 5 if with_mask else None)
        gpu.synchronize()
        assert info["pixels_refined"] == int(want_mask.sum())
        out = d_rgb.cpu().numpy()
        _same_bits(out[8:8 + want.nbytes].view(np.float64).reshape(want.shape), want, "device frame")
        assert (out[:8] == 0x5A).all() and (out[8 + want.nbytes:] == 0x5A).all()
        m = d_mask.cpu().numpy()
        if with_mask:
            assert m[5:5 + px].tobytes() == want_mask.tobytes() and (m[:5] == 0x5A).all() and (m[5 + px:] == 0x5A).all()
        else:
            assert (m == 0x5A).all()


def test_base_frame_counts_as_render_counts_it(rtc, gpu):
    dw = _device_world(rtc, gpu, "trio")
    cam = AC.camera(rtc, "trio", 37, 19)
    for mode in (RENDER, ASYNC):
        _, base_stats = dw.render(cam, mode=mode, with_stats=True)
        _, info, stats = dw.render_adaptive(cam, rtc.adaptive(0.01, 2, 2), mode=mode, with_stats=True)
        assert stats == base_stats and info["rays_refined"] > 0   # the refinement rays count as rtc_color_at's: not at all


def test_pipelined_context(rtc, gpu):
    """On a pipelined context the base frame is dealt to a lane; the pass orders itself behind it."""
    size, steps = (37, 19), (2, 2)
    want, _ = _compose(rtc, gpu, "trio", size, steps, ASYNC)
    dw = _device_world(rtc, gpu, "trio")
    cam = AC.camera(rtc, "trio", *size)
    gpu.set_pipeline(2)
    try:
        for _ in range(3):
            got, _info = dw.render_adaptive(cam, rtc.adaptive(0.01, *steps))
            _same_bits(got, want, "pipelined")
    finally:
        gpu.synchronize()
        gpu.set_pipeline(1)


def test_refusals(rtc, gpu):
    abi_info = rtc.RtcAdaptiveInfo()
    L = rtc.lib()
    dw = _device_world(rtc, gpu, "trio")
    cam = AC.camera(rtc, "trio", 9, 5)
    out = np.full((5, 9, 3), 7.0)
    PD = C.POINTER(C.c_double)

    def call(cam=cam, spec=rtc.adaptive(0.01, 2, 2), mode=ASYNC, flags=0):
        return L.rtc_render_adaptive(gpu._h, dw._h, C.byref(cam), C.byref(spec), mode, flags, out.ctypes.data_as(PD), None, C.byref(abi_info), None)

    cam4 = AC.camera(rtc, "trio", 9, 5)
    cam4.samples = 4
    assert call(cam=cam4) == 4                      # the base frame is the centre-sample frame
    assert call(flags=LDS_TABLE) == 8 and call(flags=LDS_TABLE | NO_CULL) == 8
    assert call(mode=2) == 4
    bad = rtc.RtcAdaptive(0.01, 2, 2, 3, 0)
    assert call(spec=bad) == 4
    assert (out == 7.0).all()
    assert call() == 0 and not (out == 7.0).all()
