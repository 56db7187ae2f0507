"""rtc_debug_plan_launch (csrc/rtc_launch_plan.h: an unlisted export, bound here by hand) for tests/test_host_launch_plan.py
and tests/test_gpu_launch_plan.py: the two structs, the context's default knobs, and plan(**fields)."""
import ctypes as C

FRAME, PROBE, AOV = 0, 1, 2
SRC_SMEM, SRC_LDS1, SRC_LDSN, SRC_CULL, SRC_CULL2 = range(5)
OK, ERR_UNSUPPORTED = 0, 8
NO_CULL, AA_RESAMPLE, LDS_TABLE = 1, 2, 4   # RTC_FLAG_* (include/rtc.h)
MODE_RENDER, MODE_RENDER_ASYNC = 0, 1
MAX_VIEWS = 8
TILE_LIST_CAP = 64


class Inputs(C.Structure):
    _fields_ = [("force_src", C.c_int32)] + [(k, C.c_uint32) for k in (
        "tile_cap", "tiles_per_wg", "tiles_guided_tenths", "tiles_slots", "tiles_kmax", "binning", "pipelined")] + [
        ("bin_small_pixels", C.c_uint64), ("bin_small_pixels_pipelined", C.c_uint64)] + [(k, C.c_uint32) for k in (
            "n", "n_lights", "any_refl", "any_refr", "kind", "hsize", "vsize", "samples", "nviews", "y0", "y1", "band_stride", "grid_y",
            "mode", "flags", "lens_samples")]


class Plan(C.Structure):
    _fields_ = [("status", C.c_uint32), ("src", C.c_int32)] + [(k, C.c_uint32) for k in (
        "refl", "refr", "flags", "tile_cap", "lds_bytes", "aa_lds_off", "resample_n", "block", "tile_w", "grid_x", "total_blocks", "reps")] + [
        ("chunk_wgs", C.c_uint32 * 4), ("grid_wgs", C.c_uint32), ("bin", C.c_uint32), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32),
        ("tiles", C.c_uint64), ("tiles_alloc", C.c_uint64), ("prims", C.c_uint64), ("prims_alloc", C.c_uint64),
        ("lane_dealt", C.c_uint32), ("needs_prep", C.c_uint32), ("launch_pixels", C.c_uint64), ("counted_pixels", C.c_uint64)]


# rtc_context's defaults (csrc/rtc_internal.h), written out: a changed default has to be changed here on purpose
KNOBS = dict(force_src=-1, tile_cap=512, tiles_per_wg=1, tiles_guided_tenths=20, tiles_slots=0, tiles_kmax=8, binning=1, pipelined=0,
             bin_small_pixels=6000000, bin_small_pixels_pipelined=1500000)


def plan(rtc, **fields):
    """The plan of a launch. Defaults: the context's default knobs, a one-light matte World, one pinhole view, one sample per
    pixel, MODE_RENDER_ASYNC, and — unless y0 / y1 / grid_y are given — the whole frame."""
    f = rtc.lib().rtc_debug_plan_launch
    f.restype, f.argtypes = C.c_int, [C.POINTER(Inputs), C.POINTER(Plan)]
    v = dict(KNOBS, n_lights=1, kind=FRAME, samples=1, nviews=1, band_stride=1, mode=MODE_RENDER_ASYNC)
    v.update(fields)
    if v["kind"] == FRAME:
        v.setdefault("y0", 0)
        v.setdefault("y1", v["vsize"])
        v.setdefault("grid_y", (v["y1"] - v["y0"] + 7) // 8)
    i, p = Inputs(**v), Plan()
    assert f(C.byref(i), C.byref(p)) == 0
    return p


def chunks(p):
    return list(p.chunk_wgs)
