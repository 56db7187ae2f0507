"""k_trace's whole-tile flavour is taken for a launch exactly when whole_tile_launch (csrc/rtc_kernels.hip) holds for its
parameter block: the one host function that decides it, reached here through rtc_debug_whole_tile_launch (an unlisted
export, bound by hand). From a launch that qualifies, every condition is broken alone and must refuse; nothing runs on a GPU.

The qualifying launch is a 16x8 frame, rows [0, 8): one camera, one sample per pixel, one light, RTC_MODE_RENDER_ASYNC, an
f64 canvas at a 16-byte aligned address and no 8-bit output, on the one-level culled source (SRC_CULL), whose workgroups are
one wave — one 8x8 tile — wide; its grid is the frame's 2 x 1 tiles."""
import ctypes as C

import pytest

SRC_SMEM, SRC_LDS1, SRC_LDSN, SRC_CULL, SRC_CULL2 = range(5)
MODE_RENDER, MODE_RENDER_ASYNC = 0, 1
ALIGNED = 0x7F0000001000   # an address only: no pointer of the query is dereferenced


class Query(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("out", "out8", "gamma", "rays", "tile_cnt")] + [(k, C.c_uint32) for k in (
        "samples", "nviews", "band_stride", "mode", "W", "H", "y0", "y1", "grid_x", "grid_y", "tiles_x", "tiles_y")] + [("src", C.c_int32)] + [
        (k, C.c_uint32) for k in ("refl", "refr", "further_lights")]


def frame(W, H, y0=0, y1=None, **over):
    """The qualifying launch of rows [y0, y1) of a W x H camera, its grid and its tile lists as the launch plan lays them out
    (tiles of 8x8, partial ones included), with `over` on top."""
    y1 = H if y1 is None else y1
    q = dict(out=ALIGNED, out8=0, gamma=0, rays=0, tile_cnt=ALIGNED + 65536, samples=1, nviews=1, band_stride=1, mode=MODE_RENDER_ASYNC,
             W=W, H=H, y0=y0, y1=y1, grid_x=(W + 7) // 8, grid_y=(y1 - y0 + 7) // 8, tiles_x=(W + 7) // 8, tiles_y=(H + 7) // 8,
             src=SRC_CULL, refl=0, refr=0, further_lights=0)
    q.update(over)
    return q


def whole(rtc, q):
    f = rtc.lib().rtc_debug_whole_tile_launch
    f.restype, f.argtypes = C.c_int, [C.POINTER(Query)]
    r = f(C.byref(Query(**q)))
    assert r in (0, 1), r
    return bool(r)


REFUSED = {
    "2 views": frame(16, 8, nviews=2),
    "band stride 2": frame(16, 8, band_stride=2),
    "RTC_MODE_RENDER": frame(16, 8, mode=MODE_RENDER),
    "out8 set": frame(16, 8, out8=ALIGNED + 4096),
    "gamma set": frame(16, 8, gamma=ALIGNED + 8192),
    "out misaligned by 8": frame(16, 8, out=ALIGNED + 8),
    "W = 20": frame(20, 8),
    "y1 - y0 = 12": frame(16, 12),
    "y0 = 4": frame(16, 12, y0=4, y1=12),
    "samples = 4": frame(16, 8, samples=4),
    "probe rays": frame(16, 8, rays=ALIGNED + 12288),
    "further lights": frame(16, 8, further_lights=1),
}


def test_the_qualifying_launch_and_the_north_star_accept(rtc):
    assert whole(rtc, frame(16, 8))
    assert whole(rtc, frame(1920, 1080))   # rows 0..1080: 240 x 135 whole tiles
    # every kernel the flavour is instantiated for: the culled sources' flat, reflective and refractive kernels, without the
    # flat two-level one (more VGPRs than its one-sample twin: not instantiated)
    for src in (SRC_CULL, SRC_CULL2):
        for refl, refr in ((0, 0), (1, 0), (1, 1)):
            assert whole(rtc, frame(1920, 1080, src=src, refl=refl, refr=refr)) == ((src, refl) != (SRC_CULL2, 0)), (src, refl, refr)
    assert whole(rtc, frame(32, 32, y0=8, y1=24))   # whole tile rows from y0 != 0


@pytest.mark.parametrize("name", list(REFUSED))
def test_each_condition_flipped_alone_refuses(rtc, name):
    assert not whole(rtc, REFUSED[name]), name


def test_what_else_the_kernel_assumes_refuses(rtc):
    """The one-sample flavour's own sources, a canvas to write to, rows inside the camera's, and a grid that is exactly the
    launch's whole tiles (a workgroup outside them would store outside the canvas)."""
    for src in (SRC_SMEM, SRC_LDS1, SRC_LDSN):
        assert not whole(rtc, frame(16, 8, src=src)), src
    assert not whole(rtc, frame(16, 8, out=0))
    assert not whole(rtc, frame(16, 8, y1=16, grid_y=2))   # rows past the camera's last
    assert not whole(rtc, frame(16, 8, grid_x=3))
    assert not whole(rtc, frame(16, 8, grid_y=2))
    assert not whole(rtc, frame(16, 16, grid_y=1))
    assert not whole(rtc, frame(0, 8))
    assert not whole(rtc, frame(16, 8, y1=0, grid_y=0))
    assert not whole(rtc, frame(16, 8, samples=0))   # (the host normalises 0 to 4: anti-aliased)
    # tile lists laid out for another image; without lists their layout is not read
    assert not whole(rtc, frame(16, 8, tiles_x=3))
    assert not whole(rtc, frame(16, 16, tiles_y=1))
    assert whole(rtc, frame(16, 8, tile_cnt=0, tiles_x=0, tiles_y=0))
