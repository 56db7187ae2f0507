"""The resize on the HIP path (rtc_canvas_resize_device; csrc/rtc_resize.hip). The expected bytes are the host statement's, which
tests/test_host_resize.py pins against an independent restatement without a GPU; every comparison of a resize is bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import resize_cases as RC

pytestmark = pytest.mark.gpu

ERR_ARG = 4


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


class _Job:
    """One resize enqueued on the device: the input copied `offset` bytes into an allocation of its own (offset 8: 8-byte but not
    16-byte aligned), the output at the same offset of another; finish() — after a synchronise — checks the sentinels around
    the output and that the input was only read, and returns the output."""

    def __init__(self, gpu, c, w_out, h_out, spec, offset=0):
        torch = _torch()
        self.c, self.offset = c, offset
        self.out_like = np.empty((h_out, w_out, 3), dtype=np.float64)
        self.d_in, self.d_out = _dev_bytes(torch, c.nbytes), _dev_bytes(torch, self.out_like.nbytes)
        self.p_in = _put(torch, self.d_in, offset, c)
        torch.cuda.synchronize()
        assert self.d_in.data_ptr() % 16 == 0 and self.d_out.data_ptr() % 16 == 0
        self.args = (self.p_in, c.shape[1], c.shape[0], spec, self.d_out.data_ptr() + offset, w_out, h_out)
        self.gpu = gpu

    def enqueue(self):
        self.gpu.resize_device(*self.args)
        return self

    def finish(self):
        assert _get(self.d_in, self.offset, self.c).tobytes() == self.c.tobytes(), "the input was written"
        assert _untouched(self.d_out, self.offset, self.out_like.nbytes) and _untouched(self.d_in, self.offset, self.c.nbytes), "bytes outside the canvases were written"
        return _get(self.d_out, self.offset, self.out_like)


def _on_device(gpu, c, w_out, h_out, spec, offset=0):
    job = _Job(gpu, c, w_out, h_out, spec, offset).enqueue()
    gpu.synchronize()
    return job.finish()


def _check(rtc, gpu, c, w_out, h_out, name, offsets=(0, 8)):
    spec = rtc.resize_spec(name)
    want = rtc.resize(c, w_out, h_out, spec)
    for offset in offsets:
        _assert_same_bits(_on_device(gpu, c, w_out, h_out, spec, offset), want, f"{name} {c.shape[1]}x{c.shape[0]} -> {w_out}x{h_out} at offset {offset}")
    return want


def _uploads(rtc, gpu):
    L = rtc.lib()
    L.rtc_debug_resize_uploads.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
    out = C.c_ulonglong(0)
    assert L.rtc_debug_resize_uploads(gpu._h, C.byref(out)) == 0
    return out.value


# ---- host bytes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", RC.FRAME_SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
@pytest.mark.parametrize("name", RC.FILTERS)
def test_device_bytes_equal_host_bytes(rtc, gpu, name, shape):
    """Fails on the parent commit for lack of the entry."""
    w_in, h_in, w_out, h_out = shape
    _check(rtc, gpu, RC.canvas(w_in, h_in), w_out, h_out, name)


@pytest.mark.parametrize("h", [1, 63, 64, 65])
@pytest.mark.parametrize("name", RC.FILTERS)
def test_widths_and_heights_around_the_kernels_constants(rtc, gpu, name, h):
    """Output widths on both sides of 32, 64 and 256 from 300 columns (one segment of 256 and a partial one at 257), heights on both
    sides of 64; the height changes too for one width, so that both passes and the intermediate frame are in it."""
    c = RC.canvas(300, h)
    for w_out in (31, 32, 33, 63, 64, 65, 257):
        _check(rtc, gpu, c, w_out, h, name, offsets=(0,))
    _check(rtc, gpu, c, 65, max(1, h // 2 + 1), name, offsets=(8,))
    _check(rtc, gpu, c, 301, h + 3, name, offsets=(0,))


def test_long_tap_rows(rtc, gpu):
    """2100 x 2 -> 18 x 2 with LANCZOS3 is 700 taps: the eighteen columns' span no longer fits the LDS budget and the segment
    shrinks to eight. (2100 -> 3 has a scale of 700 and a support of 2100, so each of its outputs covers the whole axis: 2100 taps,
    past the cap, refused.) 1024 x 2 -> 1 x 2 is the cap itself. 1000 x 1 -> 1 x 1 is one output of 1000 taps; the same axis
    vertically goes through the scalar-load loop."""
    _check(rtc, gpu, RC.canvas(2100, 2), 18, 2, "lanczos3")
    _check(rtc, gpu, RC.canvas(1024, 2), 1, 2, "lanczos3", offsets=(0,))
    with pytest.raises(rtc.RtcError):
        _on_device(gpu, RC.canvas(2100, 2), 3, 2, rtc.resize_spec("lanczos3"))
    _check(rtc, gpu, RC.canvas(1000, 1), 1, 1, "lanczos3")
    _check(rtc, gpu, RC.canvas(1, 1000), 1, 1, "lanczos3", offsets=(0,))
    _check(rtc, gpu, RC.canvas(5, 1000), 300, 2, "lanczos3", offsets=(0,))
    _check(rtc, gpu, RC.canvas(1000, 3), 2, 7, "box", offsets=(0,))


@pytest.mark.parametrize("name", RC.FILTERS)
def test_an_unchanged_axis_on_either_side(rtc, gpu, name):
    c = RC.canvas(70, 37)
    for w_out, h_out in ((70, 11), (70, 90), (23, 37), (200, 37), (70, 37)):
        want = _check(rtc, gpu, c, w_out, h_out, name)
        if (w_out, h_out) == (70, 37):
            _assert_same_bits(want, c, name)


@pytest.mark.parametrize("size", [(7, 5), (29, 23), (17, 5), (6, 13), (17, 13)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", RC.FILTERS)
def test_nan_and_infinities_give_the_host_bytes(rtc, gpu, name, size):
    c, _ = RC.special_canvas()
    want = _check(rtc, gpu, c, size[0], size[1], name)
    assert not np.isfinite(want).all()


# ---- call sequences --------------------------------------------------------------------------------------------------------

def test_back_to_back_calls_with_different_tables(rtc, gpu):
    """Two different table triples per axis back to back on one stream with no synchronise between the calls, then the first again
    (cached), then more triples than the cache holds and the first once more: each output equals its host bytes. A table or an
    intermediate frame rewritten while a kernel still reads it would show here."""
    lz, bx = rtc.resize_spec("lanczos3"), rtc.resize_spec("box")
    a, b = RC.canvas(300, 120, seed=3), RC.canvas(257, 131, seed=4)
    jobs = [_Job(gpu, a, 97, 55, lz), _Job(gpu, b, 130, 40, bx), _Job(gpu, a, 97, 55, lz), _Job(gpu, b, 400, 200, lz),
            _Job(gpu, a, 33, 120, bx), _Job(gpu, a, 300, 7, lz), _Job(gpu, b, 31, 17, rtc.resize_spec("mitchell")), _Job(gpu, a, 97, 55, lz),
            _Job(gpu, b, 130, 40, bx)]
    for j in jobs:
        j.enqueue()
    gpu.synchronize()
    for k, j in enumerate(jobs):
        want = rtc.resize(j.c, j.args[5], j.args[6], j.args[3])
        _assert_same_bits(j.finish(), want, f"call {k}")


def test_a_cached_triple_uploads_nothing(rtc, gpu):
    spec = rtc.resize_spec("catmull-rom")
    c = RC.canvas(91, 47, seed=9)
    want = rtc.resize(c, 40, 21, spec)
    first = _Job(gpu, c, 40, 21, spec).enqueue()
    before = _uploads(rtc, gpu)
    second = _Job(gpu, c, 40, 21, spec).enqueue()
    third = _Job(gpu, c, 40, 47, spec).enqueue()    # the horizontal table alone: cached too
    assert _uploads(rtc, gpu) == before
    gpu.synchronize()
    for j in (first, second):
        _assert_same_bits(j.finish(), want, "the same triple twice")
    _assert_same_bits(third.finish(), rtc.resize(c, 40, 47, spec), "one cached axis")
    _Job(gpu, c, 40, 22, spec).enqueue()            # a new vertical triple: one upload
    assert _uploads(rtc, gpu) == before + 1
    gpu.synchronize()


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(rtc, gpu):
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    L = rtc.lib()
    c = RC.canvas(3100, 1)
    d_in, d_out = _dev_bytes(torch, c.nbytes), _dev_bytes(torch, 3 * 64 * 8)
    p_in, p_out = _put(torch, d_in, 0, c), d_out.data_ptr()
    torch.cuda.synchronize()
    good = rtc.resize_spec("lanczos3")
    h = gpu._h

    def call(ctx=h, a=p_in, w_in=7, h_in=5, s=good, b=p_out, w_out=3, h_out=2):
        return L.rtc_canvas_resize_device(ctx, a, w_in, h_in, None if s is None else C.byref(s), b, w_out, h_out)

    assert call(ctx=None) == ERR_ARG and call(a=None) == ERR_ARG and call(b=None) == ERR_ARG and call(s=None) == ERR_ARG
    assert call(a=p_in + 4) == ERR_ARG and call(b=p_out + 4) == ERR_ARG
    for bad in ((5, 0), (0xFFFFFFFF, 0), (4, 1)):
        assert call(s=abi.RtcResize(*bad)) == ERR_ARG, bad
    for zero in ("w_in", "h_in", "w_out", "h_out"):
        assert call(**{zero: 0}) == ERR_ARG, zero
    assert call(w_in=3100, h_in=1, w_out=1, h_out=1) == ERR_ARG and call(w_in=1, h_in=3100, w_out=1, h_out=1) == ERR_ARG   # the tap cap
    assert call(b=p_in) == ERR_ARG and call(b=p_in + 8 * 104) == ERR_ARG and call(a=p_out + 8 * 17, b=p_out) == ERR_ARG   # overlapping
    assert call(w_in=8, h_in=8, w_out=1 << 21, h_out=1 << 13) == ERR_ARG   # 2^32 threads and more
    gpu.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all() and _get(d_in, 0, c).tobytes() == c.tobytes()
    # ... and the same arguments with nothing wrong write the canvas
    assert call() == 0
    gpu.synchronize()
    want = rtc.resize(c.reshape(-1)[:105].reshape(5, 7, 3), 3, 2, good)
    _assert_same_bits(_get(d_out, 0, want), want, "after the refusals")


# ---- supersampling end to end ----------------------------------------------------------------------------------------------

def test_box_halving_of_a_2x_frame_is_the_four_fixed_subsamples(rtc, gpu):
    """The north-star World at 64 x 36, one sample, resized with BOX to 32 x 18 on the device, against rtc_render of the same camera
    at 32 x 18 with samples = 4 and no resample flag. pixel_size halves exactly and (2x + 0.5) * ps/2 rounds as (x + 0.25) * ps: the
    64 x 36 pixel centres are the four fixed sub-sample rays bit for bit, and only the order of the four-term sum differs — a few
    ulps of a colour; 1e-12 is the project's own colour tolerance."""
    torch = _torch()
    scenes = importlib.import_module(rtc.__name__ + ".scenes")
    w, cam2 = scenes.synthetic(100, 64, 36)
    _, cam1 = scenes.synthetic(100, 32, 18)
    assert cam2.pixel_size * 2.0 == cam1.pixel_size and cam2.samples == 1
    cam1.samples = 4
    big = torch.zeros(36 * 64 * 3, dtype=torch.float64, device="cuda:0")
    small = _dev_bytes(torch, 18 * 32 * 24)
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    try:
        dw.render_rows(cam2, 0, 36, big.data_ptr(), mode=rtc.MODE_RENDER_ASYNC)
        gpu.resize_device(big.data_ptr(), 64, 36, rtc.resize_spec("box"), small.data_ptr(), 32, 18)
        gpu.synchronize()
        want = dw.render(cam1, mode=rtc.MODE_RENDER_ASYNC)
    finally:
        dw.close()
    got = _get(small, 0, np.empty((18, 32, 3)))
    assert _untouched(small, 0, 18 * 32 * 24)
    _assert_same_bits(got, rtc.resize(big.cpu().numpy().reshape(36, 64, 3), 32, 18, rtc.resize_spec("box")), "device against host")
    err = np.abs(got - np.asarray(want).reshape(18, 32, 3)).max()
    print(f"max |BOX(64x36) - samples=4| = {err:.3e}")
    assert got.max() > 0.2 and err <= 1e-12
