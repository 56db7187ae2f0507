"""The post-processing passes on the HIP path (rtc_canvas_luminance_device, rtc_canvas_tonemap_device, rtc_canvas_bloom_device;
csrc/rtc_post.hip). The expected bytes are the host statement's, which tests/test_host_post.py pins against an independent
restatement without a GPU; every comparison is bit for bit."""
import ctypes as C
import importlib
import math
from pathlib import Path

import numpy as np
import pytest

import post_cases as PC

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TONEMAPS = [("linear", dict(exposure=0.37)), ("reinhard", dict(exposure=1.0, white=3.0)), ("reinhard", dict(key=0.18, auto_white=True)),
            ("aces", dict(key=0.5)), ("aces", dict(exposure=0.6))]


def _torch():
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _dev_bytes(torch, nbytes):
    """A device allocation of nbytes + 64, every byte 0x5A: what a buffer holds where nothing was written."""
    return torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")


def _put(torch, buf, offset, arr):
    a = np.ascontiguousarray(arr)
    buf[offset:offset + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    return buf.data_ptr() + offset


def _get(buf, offset, like):
    return buf[offset:offset + like.nbytes].cpu().numpy().view(like.dtype).reshape(like.shape)


def _assert_same_bits(got, want, what):
    assert got.shape == want.shape, what
    d = np.argwhere(_bits(got) != _bits(want))
    assert len(d) == 0, f"{what}: {len(d)} values differ, first at {d[0].tolist()}: got {got[tuple(d[0])]!r}, want {want[tuple(d[0])]!r}"


def _untouched(buf, offset, nbytes):
    host = buf.cpu().numpy()
    return (host[:offset] == 0x5A).all() and (host[offset + nbytes:] == 0x5A).all()


def _stats_bytes(st):
    return bytes(st)


def _on_device(gpu, c, offset, op):
    """The canvas copied `offset` bytes into an allocation of its own (offset 8: 8-byte but not 16-byte aligned) and `op(p_in,
    p_out)` run twice: into a second allocation at the same offset, and in place on a second copy. -> (out of place, in place);
    asserts the sentinels around both outputs and that the input was only read."""
    torch = _torch()
    d_in, d_out, d_both = (_dev_bytes(torch, c.nbytes) for _ in range(3))
    p_in, p_both = _put(torch, d_in, offset, c), _put(torch, d_both, offset, c)
    torch.cuda.synchronize()
    assert d_in.data_ptr() % 16 == 0
    op(p_in, d_out.data_ptr() + offset)
    op(p_both, p_both)
    gpu.synchronize()
    assert _get(d_in, offset, c).tobytes() == c.tobytes(), "the input was written"
    assert _untouched(d_out, offset, c.nbytes) and _untouched(d_both, offset, c.nbytes) and _untouched(d_in, offset, c.nbytes), "bytes outside the canvas were written"
    return _get(d_out, offset, c), _get(d_both, offset, c)


def _luminance_on_device(rtc, gpu, c, offset=0):
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    d_in, d_st = _dev_bytes(torch, c.nbytes), _dev_bytes(torch, 24)
    p_in = _put(torch, d_in, offset, c)
    torch.cuda.synchronize()
    gpu.luminance_device(p_in, c.shape[1], c.shape[0], d_st.data_ptr() + offset)
    gpu.synchronize()
    assert _untouched(d_st, offset, 24) and _get(d_in, offset, c).tobytes() == c.tobytes()
    return abi.RtcLuminance.from_buffer_copy(d_st.cpu().numpy()[offset:offset + 24].tobytes())


@pytest.mark.parametrize("name", PC.NAMES)
def test_statistics_and_tonemap_bytes_equal_host_bytes(rtc, gpu, name):
    torch = _torch()
    c = PC.canvas(name)
    height, width = c.shape[:2]
    want_st = rtc.luminance(c)
    for offset in (0, 8):
        assert _stats_bytes(_luminance_on_device(rtc, gpu, c, offset)) == _stats_bytes(want_st), f"{name} statistics at offset {offset}"
        # the record stays in device memory: auto exposure and auto white never see the host
        d_rgb, d_st = _dev_bytes(torch, c.nbytes), _dev_bytes(torch, 24)
        p_rgb = _put(torch, d_rgb, offset, c)
        torch.cuda.synchronize()
        gpu.luminance_device(p_rgb, width, height, d_st.data_ptr() + offset)
        for curve, kw in TONEMAPS:
            spec = rtc.tonemap_spec(curve, **kw)
            want = rtc.tonemap(c, spec, want_st)
            got, inplace = _on_device(gpu, c, offset, lambda a, b: gpu.tonemap_device(a, width, height, spec, b, d_st.data_ptr() + offset))
            _assert_same_bits(got, want, f"{name} {curve} {kw} at offset {offset}")
            _assert_same_bits(inplace, want, f"{name} {curve} {kw} in place at offset {offset}")


@pytest.mark.parametrize("radius", PC.RADII)
@pytest.mark.parametrize("name", PC.NAMES)
def test_bloom_bytes_equal_host_bytes(rtc, gpu, name, radius):
    c = PC.canvas(name)
    height, width = c.shape[:2]
    spec = rtc.bloom_spec(PC.threshold(), 0.7, {1: 0.6, 2: 1.0, 32: 9.0}[radius], radius)
    want = rtc.bloom(c, spec)
    for offset in (0, 8):
        got, inplace = _on_device(gpu, c, offset, lambda a, b: gpu.bloom_device(a, width, height, spec, b))
        _assert_same_bits(got, want, f"{name} radius {radius} at offset {offset}")
        _assert_same_bits(inplace, want, f"{name} radius {radius} in place at offset {offset}")
    if not name.startswith("black") and width * height >= 8:
        assert (_bits(want) != _bits(c)).any()   # the pass does something on these canvases


@pytest.mark.parametrize("n", PC.STAT_PIXELS)
def test_statistics_at_the_levels_edges(rtc, gpu, n):
    """255, 256 and 257 pixels: the block edge; 65 536: the second level exactly full; 65 537 (as 65 537 x 1): the first frame that
    needs a third launch."""
    c = PC.strip(n)
    want = rtc.luminance(c)
    got = _luminance_on_device(rtc, gpu, c)
    assert _stats_bytes(got) == _stats_bytes(want), ((got.max, got.sum, got.count), (want.max, want.sum, want.count))
    assert 0 < want.count < n


def test_an_empty_frame_gives_the_zero_record(rtc, gpu):
    torch = _torch()
    d_in, d_st = _dev_bytes(torch, 24), _dev_bytes(torch, 24)
    gpu.luminance_device(d_in.data_ptr(), 0, 5, d_st.data_ptr())
    gpu.synchronize()
    assert d_st.cpu().numpy()[:24].tobytes() == bytes(24) and _untouched(d_st, 0, 24)


def _allocs(rtc, gpu):
    L = rtc.lib()
    L.rtc_debug_render_allocs.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    out = C.c_ulonglong(0)
    assert L.rtc_debug_render_allocs(gpu._h, C.byref(out)) == 0
    return out.value


def test_repeated_calls_allocate_nothing_and_smaller_frames_still_match(rtc, gpu):
    """The block results and the horizontal plane are grow-only buffers of the context: a second call of the same size allocates
    nothing, and a smaller frame after a larger one still gives the host's bytes."""
    def run(name, radius):
        c = PC.canvas(name)
        height, width = c.shape[:2]
        spec = rtc.bloom_spec(PC.threshold(), 0.7, 2.0, radius)
        got = _on_device(gpu, c, 0, lambda a, b: gpu.bloom_device(a, width, height, spec, b))[0]
        _assert_same_bits(got, rtc.bloom(c, spec), f"{name} radius {radius}")
        assert _stats_bytes(_luminance_on_device(rtc, gpu, c)) == _stats_bytes(rtc.luminance(c)), name

    run("70x70", 32)
    before = _allocs(rtc, gpu)
    run("70x70", 32)
    for name, radius in (("33x9", 2), ("257x3", 32), ("1x1", 1), ("70x70", 1)):
        run(name, radius)
    assert _allocs(rtc, gpu) == before


def test_errors_launch_nothing(rtc, gpu):
    """NULL and misaligned pointers, bad records and AUTO flags without a record are RTC_ERR_ARG (4), and the outputs keep their fill."""
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    L = rtc.lib()
    c = PC.canvas("31x9")
    width, height = 31, 9
    d_in, d_out, d_st = _dev_bytes(torch, c.nbytes), _dev_bytes(torch, c.nbytes), _dev_bytes(torch, 24)
    p_in, p_out, p_st = _put(torch, d_in, 0, c), d_out.data_ptr(), d_st.data_ptr()
    torch.cuda.synchronize()
    h = gpu._h
    assert L.rtc_canvas_luminance_device(None, p_in, width, height, p_st) == 4 and L.rtc_canvas_luminance_device(h, None, width, height, p_st) == 4
    assert L.rtc_canvas_luminance_device(h, p_in, width, height, None) == 4
    assert L.rtc_canvas_luminance_device(h, p_in + 4, width, height, p_st) == 4 and L.rtc_canvas_luminance_device(h, p_in, width, height, p_st + 4) == 4
    tm, auto = rtc.tonemap_spec("reinhard"), rtc.tonemap_spec("reinhard", key=0.18)
    tone = lambda ctx=h, a=p_in, s=tm, st=None, b=p_out: L.rtc_canvas_tonemap_device(ctx, a, width, height, None if s is None else C.byref(s), st, b)
    assert tone(ctx=None) == 4 and tone(a=None) == 4 and tone(b=None) == 4 and tone(s=None) == 4
    assert tone(a=p_in + 4) == 4 and tone(b=p_out + 4) == 4 and tone(st=p_st + 4) == 4
    assert tone(s=auto) == 4   # an AUTO flag without the record
    for bad in [(0.0, 1.0, 1, 0), (math.nan, 1.0, 1, 0), (1.0, 0.0, 1, 0), (1.0, 1.0, 3, 0), (1.0, 1.0, 1, 4)]:
        assert tone(s=abi.RtcTonemap(*bad)) == 4, bad
    bl = rtc.bloom_spec()
    glare = lambda ctx=h, a=p_in, s=bl, b=p_out: L.rtc_canvas_bloom_device(ctx, a, width, height, None if s is None else C.byref(s), b)
    assert glare(ctx=None) == 4 and glare(a=None) == 4 and glare(b=None) == 4 and glare(s=None) == 4
    assert glare(a=p_in + 4) == 4 and glare(b=p_out + 4) == 4
    for bad in [(-1.0, 0.5, 2.0, 4, 0), (1.0, math.inf, 2.0, 4, 0), (1.0, 0.5, 0.0, 4, 0), (1.0, 0.5, 2.0, 0, 0), (1.0, 0.5, 2.0, 33, 0), (1.0, 0.5, 2.0, 4, 1)]:
        assert glare(s=abi.RtcBloom(*bad)) == 4, bad
    gpu.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all() and (d_st.cpu().numpy() == 0x5A).all() and _get(d_in, 0, c).tobytes() == c.tobytes()
    # ... and the same arguments with nothing wrong write the canvas
    assert glare() == 0
    gpu.synchronize()
    _assert_same_bits(_get(d_out, 0, c), rtc.bloom(c, bl), "after the errors")


def test_end_to_end_bright_lights_to_rgba8(rtc, gpu):
    """data/bright_lights.yml at 96x54 on the device: render, bloom, statistics, REINHARD with auto exposure and auto white,
    rtc_canvas_to_rgba8_device at gamma 2.2. The RGBA8 bytes are the host chain's from the same frame; and the plain to_rgba8 of
    that frame has more 255-valued channels than the tone-mapped one: the feature does something."""
    torch = _torch()
    path = Path(rtc.__file__).resolve().parent / "data" / "bright_lights.yml"
    w, cam, tm, bl = rtc.load_yaml_post(path=path)
    width, height = 96, 54
    cam = _resized(rtc, path, width, height)
    assert tm.flags == 3 and tm.curve == 1
    canvas = torch.zeros(height * width * 3, dtype=torch.float64, device="cuda:0")
    post = torch.zeros_like(canvas)
    stats = torch.zeros(3, dtype=torch.float64, device="cuda:0")
    rgba, plain = (torch.zeros(height * width * 4, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    try:
        dw.render_rows(cam, 0, height, canvas.data_ptr())
        gpu.bloom_device(canvas.data_ptr(), width, height, bl, post.data_ptr())
        gpu.luminance_device(post.data_ptr(), width, height, stats.data_ptr())
        gpu.tonemap_device(post.data_ptr(), width, height, tm, post.data_ptr(), stats.data_ptr())
        _check(rtc, rtc.lib().rtc_canvas_to_rgba8_device(gpu._h, C.c_void_p(post.data_ptr()), width, height, 2.2, C.c_void_p(rgba.data_ptr())))
        _check(rtc, rtc.lib().rtc_canvas_to_rgba8_device(gpu._h, C.c_void_p(canvas.data_ptr()), width, height, 2.2, C.c_void_p(plain.data_ptr())))
        gpu.synchronize()
    finally:
        dw.close()
    frame = canvas.cpu().numpy().reshape(height, width, 3)
    assert frame.max() > 1.5   # components well above 1
    bloomed = rtc.bloom(frame, bl)
    st = rtc.luminance(bloomed)
    assert stats.cpu().numpy().tobytes() == bytes(st)
    mapped = rtc.tonemap(bloomed, tm, st)
    _assert_same_bits(post.cpu().numpy().reshape(height, width, 3), mapped, "bloom, statistics, tone map")
    want8, plain8 = rtc.to_rgba8(mapped, 2.2), rtc.to_rgba8(frame, 2.2)
    got8, gotplain8 = rgba.cpu().numpy().reshape(height, width, 4), plain.cpu().numpy().reshape(height, width, 4)
    assert np.array_equal(got8, np.asarray(want8).reshape(height, width, 4)) and np.array_equal(gotplain8, np.asarray(plain8).reshape(height, width, 4))
    clipped_plain, clipped_mapped = int((gotplain8[..., :3] == 255).sum()), int((got8[..., :3] == 255).sum())
    assert clipped_plain > clipped_mapped and clipped_plain > 100, (clipped_plain, clipped_mapped)


def _check(rtc, status):
    assert status == 0, status


def _resized(rtc, path, width, height):
    """The shipped scene's camera at another frame size: the file's text with its width and height replaced."""
    text = path.read_text().replace("width: 640", f"width: {width}").replace("height: 360", f"height: {height}")
    return rtc.load_yaml_post(text=text)[1]
