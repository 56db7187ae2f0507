"""The launch plan (csrc/rtc_launch_plan.h) on the CPU: every decision the host makes in front of a launch, pinned without
one. Expected values are the project's records — the decision columns of tests/test_gpu_full_frames.py's CASES, the comments
in rtc_internal.h and rtc_launch_plan.cpp, RTC_BLOCK_FOR — or are worked out by hand below; none is read off the plan.

DESIGN.md ("Launch planning") names the cases that catch three deliberately broken plans."""
import importlib

import pytest

import launch_plan as L
from test_gpu_full_frames import CASES

P1080 = dict(hsize=1920, vsize=1080)
PER_OBJ = 96 + 32 + 4   # bytes of an object in the LDS table (rtc_launch_plan.cpp)


def plan(rtc, **kw):
    """L.plan, and what holds for EVERY planned launch: the chunk levels account for every tile exactly once."""
    p = L.plan(rtc, **kw)
    c = L.chunks(p)
    singles = p.grid_wgs - sum(c)
    if any(c):
        assert p.reps == 1
        assert c[0] * 8 + c[1] * 4 + c[2] * 3 + c[3] * 2 + singles == p.total_blocks, (kw, c, p.grid_wgs, p.total_blocks)
    else:
        assert p.grid_wgs == (p.total_blocks + p.reps - 1) // p.reps, kw
    return p


def guided(p):
    return sum(L.chunks(p)) > 0


# ------------------------------------------------------------------ the full-frame cases
@pytest.fixture(scope="module")
def worlds(rtc):
    scenes = importlib.import_module(rtc.__name__ + ".scenes")
    return {c.name: len(c.make(rtc, scenes)[0]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_full_frame_decisions(rtc, worlds, case):
    kw = dict(n=worlds[case.name], any_refl=int(case.reflective and not case.refractive), any_refr=int(case.refractive),
              hsize=case.size[0], vsize=case.size[1])
    p = plan(rtc, **kw)
    assert (p.status, p.src, bool(p.refl), bool(p.refr)) == (L.OK, case.source, case.reflective, case.refractive)
    assert bool(p.bin) == case.binned_in_order and guided(p) == case.guided
    assert p.lane_dealt == 1 and p.needs_prep == 0
    assert p.launch_pixels == p.counted_pixels == case.size[0] * case.size[1]
    q = plan(rtc, pipelined=1, **kw)
    assert (q.src, bool(q.bin), guided(q)) == (case.source, case.binned_pipelined, case.guided)
    assert not guided(plan(rtc, tiles_guided_tenths=0, **kw))
    assert not plan(rtc, binning=0, **kw).bin
    b = plan(rtc, flags=L.NO_CULL, **kw)
    assert (b.status, b.src, b.bin, b.lane_dealt, b.needs_prep) == (L.OK, case.brute_source, 0, 0, 1)
    assert guided(b) == case.guided   # (test_full_frame pins `guided` for the brute-force launch too)


# ------------------------------------------------------------------ binning
def test_in_order_binning_starts_at_three_1080p_views(rtc):
    """rtc_internal.h: "1080p: from 3 views per launch" (bin_small_pixels = 6 000 000; a 1080p frame has 2 073 600 pixels)."""
    assert [plan(rtc, n=20, nviews=v, **P1080).bin for v in (1, 2, 3)] == [0, 0, 1]


@pytest.mark.parametrize("pipelined, knob, threshold", [(0, "bin_small_pixels", 6000000), (1, "bin_small_pixels_pipelined", 1500000)])
def test_binning_thresholds_at_their_edges(rtc, pipelined, knob, threshold):
    at = dict(n=20, pipelined=pipelined, hsize=threshold, vsize=1)
    below = dict(at, hsize=threshold - 1)
    assert L.KNOBS[knob] == threshold
    assert plan(rtc, **at).launch_pixels == threshold and plan(rtc, **at).bin == 1
    assert plan(rtc, **below).launch_pixels == threshold - 1 and plan(rtc, **below).bin == 0
    # the knob is the threshold, and each kind of context reads its own
    assert plan(rtc, **dict(below, **{knob: threshold - 1})).bin == 1
    assert plan(rtc, **dict(at, pipelined=1 - pipelined)).bin == (1 if pipelined == 0 else 0)
    # a launch is measured by the rows it renders, not by the frame: one rank's bands of a frame above the threshold
    assert plan(rtc, n=20, pipelined=pipelined, hsize=threshold // 8, vsize=32, band_stride=4, grid_y=1).bin == 1
    assert plan(rtc, n=20, pipelined=pipelined, hsize=threshold // 8 - 1, vsize=32, band_stride=4, grid_y=1).bin == 0


def test_two_level_worlds_are_always_binned_and_nothing_else_ever(rtc):
    two = dict(n=300, hsize=8, vsize=8)
    for pipelined in (0, 1):
        assert plan(rtc, pipelined=pipelined, **two).bin == 1
        assert plan(rtc, pipelined=pipelined, **two).src == L.SRC_CULL2
    big = dict(n=300, nviews=3, **P1080)
    assert plan(rtc, **big).bin == 1
    assert plan(rtc, y0=8, y1=1080, **big).bin == 1
    assert plan(rtc, y0=4, y1=1080, **big).bin == 0          # tile rows not aligned with the image's
    assert plan(rtc, **dict(big, n=0)).bin == 0
    assert plan(rtc, **dict(big, nviews=1), lens_samples=4).bin == 0
    assert plan(rtc, binning=0, **big).bin == 0
    assert plan(rtc, flags=L.NO_CULL, **big).bin == 0
    for force in (0, 1, 2):
        assert plan(rtc, force_src=force, **big).bin == 0


def test_binning_memory(rtc):
    """rtc_launch_plan.cpp: RTC_MAX_VIEWS views while that stays within 128 MB per set ("1080p: 67 MB"), else exactly the launch's."""
    per_view = 240 * 135
    p = plan(rtc, n=300, nviews=3, **P1080)
    assert (p.tiles_x, p.tiles_y, p.tiles, p.tiles_alloc) == (240, 135, 3 * per_view, L.MAX_VIEWS * per_view)
    assert (p.prims, p.prims_alloc) == (3 * 300, L.MAX_VIEWS * 300)
    assert round(p.tiles_alloc * 4 * (1 + L.TILE_LIST_CAP) / 1e6) == 67
    p = plan(rtc, n=300, nviews=3, hsize=4096, vsize=4096)
    assert (p.tiles, p.tiles_alloc, p.prims, p.prims_alloc) == (3 * 512 * 512, 3 * 512 * 512, 900, 900)
    # the largest frame that still reserves for every view: 8 x tiles x 260 B <= 128 MiB, tiles <= 64527
    assert plan(rtc, n=300, hsize=8 * 64527, vsize=8).tiles_alloc == 8 * 64527
    assert plan(rtc, n=300, hsize=8 * 64528, vsize=8).tiles_alloc == 64528
    # a pipelined lane's own lists: the launch's size
    p = plan(rtc, n=300, nviews=3, pipelined=1, **P1080)
    assert (p.tiles, p.tiles_alloc, p.prims, p.prims_alloc) == (3 * per_view, 3 * per_view, 900, 900)


# ------------------------------------------------------------------ guided chunks
def test_chunks_of_a_reflective_1080p_frame_by_hand(rtc):
    """32400 tiles, slots = 4096, 2.0 x slots = 8192 tiles per level, from the END: 8192 singles; 8192 in pairs (4096); 8190 in
    threes (2730); then 7824 of the remaining 7826 in fours (1956); the last level takes the 2 left, which make no eight and
    join the singles: 8194."""
    p = plan(rtc, n=20, any_refl=1, **P1080)
    assert (p.block, p.tile_w, p.grid_x, p.total_blocks) == (64, 8, 240, 32400)
    assert L.chunks(p) == [0, 1956, 2730, 4096] and p.grid_wgs == 1956 + 2730 + 4096 + 8194
    p = plan(rtc, n=20, any_refl=1, tiles_kmax=2, **P1080)
    assert L.chunks(p) == [0, 0, 0, 12104] and p.grid_wgs == 12104 + 8192


@pytest.mark.parametrize("label, kw, block, slots", [
    ("frame stack", dict(n=20, any_refl=1), 64, 4096), ("frame stack, refractive", dict(n=300, any_refr=1), 64, 4096),
    ("frame stack, brute force", dict(n=20, any_refr=1, flags=L.NO_CULL), 64, 4096),
    ("flat, one level", dict(n=20), 64, 5120), ("flat, two levels", dict(n=300), 64, 5120),
    ("flat, brute force", dict(n=20, flags=L.NO_CULL), 128, 2560)])
def test_natural_slots(rtc, label, kw, block, slots):
    """1024 x (4 frame stack | 5 flat) / (block / 64), block from RTC_BLOCK_FOR: chunks from 3 x slots tiles on."""
    tile_w = block // 64 * 8
    for tiles, want in ((3 * slots - 1, False), (3 * slots, True)):
        p = plan(rtc, hsize=tile_w, vsize=8 * tiles, **kw)
        assert (p.block, p.tile_w, p.grid_x, p.total_blocks) == (block, tile_w, 1, tiles), label
        assert guided(p) == want, (label, tiles)
    # RTC_TILES_SLOTS replaces the natural value. One slot: 2 tiles per level, so of 54 tiles 2 go singly and 2 as a pair, no
    # three or four fits into 2, and the last level takes 48 of the remaining 50 in eights; 2 more singles
    p = plan(rtc, hsize=tile_w, vsize=8 * 54, tiles_slots=1, **kw)
    assert L.chunks(p) == [6, 0, 0, 1] and p.grid_wgs == 6 + 1 + 4
    assert not guided(plan(rtc, hsize=tile_w, vsize=16, tiles_slots=1, **kw))


def test_launches_without_chunks(rtc):
    kw = dict(n=20, **P1080)
    assert guided(plan(rtc, **kw))
    assert not guided(plan(rtc, tiles_per_wg=2, **kw)) and plan(rtc, tiles_per_wg=2, **kw).grid_wgs == 16200
    assert not guided(plan(rtc, lens_samples=4, **kw))
    assert plan(rtc, lens_samples=4, tiles_per_wg=2, **kw).reps == 1     # a lens launch: one workgroup per tile
    assert not guided(plan(rtc, tiles_guided_tenths=0, **kw))
    assert not guided(plan(rtc, tiles_kmax=1, **kw))
    # a large world on a small frame (10 000 objects at 1080p) — but not on 8192^2, and not a world of 4096
    assert not guided(plan(rtc, n=10000, **P1080))
    assert guided(plan(rtc, n=10000, hsize=8192, vsize=8192))
    assert guided(plan(rtc, n=4096, **P1080)) and not guided(plan(rtc, n=4097, **P1080))
    assert guided(plan(rtc, n=5000, hsize=1000, vsize=8000))             # 8 000 000 pixels
    assert not guided(plan(rtc, n=5000, hsize=1000, vsize=7999))


# ------------------------------------------------------------------ source and LDS
def rounded(nbytes):
    return (nbytes + 15) // 16 * 16


@pytest.mark.parametrize("n, flags, knobs, src, cap", [
    (0, 0, {}, L.SRC_CULL, 0), (256, 0, {}, L.SRC_CULL, 0), (257, 0, {}, L.SRC_CULL2, 0),
    (128, L.NO_CULL, {}, L.SRC_SMEM, 0), (129, L.NO_CULL, {}, L.SRC_LDS1, 129), (201, L.NO_CULL, {}, L.SRC_LDS1, 201),
    (448, L.NO_CULL, {}, L.SRC_LDS1, 448), (449, L.NO_CULL, {}, L.SRC_LDSN, 512), (449, L.NO_CULL, {"tile_cap": 100}, L.SRC_LDSN, 100),
    (0, L.NO_CULL | L.LDS_TABLE, {}, L.SRC_LDS1, 1), (20, L.NO_CULL | L.LDS_TABLE, {}, L.SRC_LDS1, 20),
    (1163, L.NO_CULL | L.LDS_TABLE, {}, L.SRC_LDS1, 1163),   # 153 516 B of the 150 KiB (153 600 B)
    (1164, L.NO_CULL | L.LDS_TABLE, {}, L.SRC_LDSN, 512),    # 153 648 B: LDS tiles
    (20, L.LDS_TABLE, {}, L.SRC_CULL, 0),                    # (the flag means something with RTC_FLAG_NO_CULL only)
    (5000, 0, {"force_src": 1}, L.SRC_LDSN, 512), (300, L.NO_CULL, {"force_src": 3}, L.SRC_CULL, 0), (20, 0, {"force_src": 2}, L.SRC_LDSN, 512)])
def test_source_and_lds_table(rtc, n, flags, knobs, src, cap):
    p = plan(rtc, n=n, flags=flags, hsize=70, vsize=45, **knobs)
    table = rounded(cap * PER_OBJ) if cap else 0
    assert (p.status, p.src, p.tile_cap, p.lds_bytes, p.aa_lds_off, p.resample_n) == (L.OK, src, cap, table, 0, 0)
    assert p.flags == flags
    # anti-aliased: the sub-sample store behind the table, 15 doubles per lane
    for samples in (0, 4, 16):
        a = plan(rtc, n=n, flags=flags, samples=samples, hsize=70, vsize=45, **knobs)
        assert (a.src, a.tile_cap, a.aa_lds_off, a.lds_bytes, a.resample_n) == (src, cap, table, table + a.block * 15 * 8, 0)
        assert a.block == (64 if src in (L.SRC_CULL, L.SRC_CULL2) else 128)


def test_table_sizes_by_hand(rtc):
    assert rounded(201 * PER_OBJ) == 26544 != 201 * PER_OBJ and rounded(1163 * PER_OBJ) == 153520
    assert plan(rtc, n=201, flags=L.NO_CULL, samples=4, hsize=70, vsize=45).lds_bytes == 26544 + 128 * 120


def test_resample_count(rtc):
    kw = dict(n=20, hsize=70, vsize=45)
    assert plan(rtc, samples=16, flags=L.AA_RESAMPLE, **kw).resample_n == 16
    assert plan(rtc, samples=16, **kw).resample_n == 0
    assert plan(rtc, samples=0, flags=L.AA_RESAMPLE, **kw).resample_n == 0
    assert plan(rtc, samples=1, flags=L.AA_RESAMPLE, **kw).resample_n == 0
    assert plan(rtc, samples=255, flags=L.AA_RESAMPLE | L.NO_CULL, **kw).resample_n == 255
    p = plan(rtc, samples=16, flags=L.AA_RESAMPLE | L.NO_CULL, lens_samples=4, **kw)
    assert (p.resample_n, p.flags) == (0, L.NO_CULL)


# ------------------------------------------------------------------ refusals
FLAVOURS = {"two lights": dict(n_lights=2, hsize=70, vsize=45), "lens": dict(lens_samples=4, hsize=70, vsize=45),
            "aov": dict(kind=L.AOV, hsize=70, vsize=45), "two lights, probe": dict(kind=L.PROBE, n_lights=2, hsize=100),
            "two lights, aov": dict(kind=L.AOV, n_lights=2, hsize=70, vsize=45)}


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("n", [0, 3, 300, 2000])
def test_flavours_without_lds_kernels(rtc, flavour, n):
    kw = dict(FLAVOURS[flavour], n=n)
    culled = L.SRC_CULL2 if n > 256 else L.SRC_CULL
    assert (plan(rtc, **kw).status, plan(rtc, **kw).src) == (L.OK, culled)
    # brute force is the scalar-cache source at EVERY size ...
    assert (plan(rtc, flags=L.NO_CULL, **kw).status, plan(rtc, flags=L.NO_CULL, **kw).src) == (L.OK, L.SRC_SMEM)
    # ... and an LDS source is refused, wherever it comes from
    assert plan(rtc, flags=L.NO_CULL | L.LDS_TABLE, **kw).status == L.ERR_UNSUPPORTED
    for force in (1, 2):
        assert plan(rtc, force_src=force, **kw).status == L.ERR_UNSUPPORTED
    for force in (0, 3, 4):
        p = plan(rtc, force_src=force, **kw)
        assert (p.status, p.src) == (L.OK, force)
    # the same requests of a pinhole frame of a one-light World are all planned
    one = dict(n=n, hsize=70, vsize=45)
    assert plan(rtc, flags=L.NO_CULL, **one).src == (L.SRC_SMEM if n <= 128 else L.SRC_LDS1 if n <= 448 else L.SRC_LDSN)
    assert plan(rtc, flags=L.NO_CULL | L.LDS_TABLE, **one).status == L.OK
    for force in range(5):
        assert plan(rtc, force_src=force, **one).status == L.OK


def test_aov_refuses_the_lds_flag_on_its_own(rtc):
    assert plan(rtc, kind=L.AOV, n=3, flags=L.LDS_TABLE, hsize=70, vsize=45).status == L.ERR_UNSUPPORTED


def test_aov_and_probe_grids(rtc):
    p = plan(rtc, kind=L.AOV, n=300, hsize=70, vsize=45)
    assert (p.block, p.grid_x, p.total_blocks, p.grid_wgs, p.lds_bytes) == (64, 9, 54, 54, 0)
    # a probe is one lane per ray: the flat kernels at RTC_BLOCK = 128 whatever their cull level, the frame-stack kernels one wave
    for kw, block in ((dict(n=20), 128), (dict(n=300), 128), (dict(n=20, flags=L.NO_CULL), 128), (dict(n=20, any_refl=1), 64),
                      (dict(n=300, any_refr=1), 64)):
        p = plan(rtc, kind=L.PROBE, hsize=100, **kw)
        assert (p.status, p.block, p.grid_x, p.total_blocks, p.grid_wgs, p.reps, p.needs_prep) == (L.OK, block, -(-100 // block), -(-100 // block), -(-100 // block), 1, 0), kw
        assert not guided(p) and p.bin == 0
    assert plan(rtc, kind=L.PROBE, hsize=100, n=201, flags=L.NO_CULL).lds_bytes == 26544


# ------------------------------------------------------------------ grid, lanes, pixels
def test_grid_and_lanes(rtc):
    p = plan(rtc, n=20, hsize=70, vsize=45, nviews=2)
    assert (p.block, p.tile_w, p.grid_x, p.total_blocks, p.reps, p.lane_dealt, p.needs_prep) == (64, 8, 9, 9 * 6 * 2, 1, 1, 0)
    p = plan(rtc, n=20, hsize=70, vsize=45, flags=L.NO_CULL)
    assert (p.block, p.tile_w, p.grid_x, p.total_blocks, p.lane_dealt, p.needs_prep) == (128, 16, 5, 30, 0, 1)
    p = plan(rtc, n=20, hsize=70, vsize=45, flags=L.NO_CULL, lens_samples=4)    # no per-view table for lens rays
    assert (p.src, p.lane_dealt, p.needs_prep) == (L.SRC_SMEM, 0, 0)
    p = plan(rtc, n=20, hsize=70, vsize=45, tiles_per_wg=4)
    assert (p.reps, p.grid_wgs) == (4, 14)


def test_counted_pixels(rtc):
    kw = dict(n=20, hsize=70, vsize=45)
    assert plan(rtc, **kw).counted_pixels == 70 * 45
    assert plan(rtc, mode=L.MODE_RENDER, **kw).counted_pixels == 69 * 44          # Camera::render: not the last row and column
    assert plan(rtc, nviews=3, mode=L.MODE_RENDER, **kw).counted_pixels == 3 * 69 * 44
    assert plan(rtc, y0=8, y1=40, mode=L.MODE_RENDER, **kw).counted_pixels == 69 * 32
    assert plan(rtc, y0=40, y1=45, **kw).counted_pixels == 70 * 5                 # a last band of 5 rows
    assert plan(rtc, y0=40, y1=45, mode=L.MODE_RENDER, **kw).counted_pixels == 69 * 4
    # bands 0, 2, 4 and 1, 3, 5 of the six (rtc_render_bands): only the rows a caller owns
    assert plan(rtc, y0=0, y1=45, band_stride=2, grid_y=3, **kw).counted_pixels == 70 * 24
    assert plan(rtc, y0=8, y1=45, band_stride=2, grid_y=3, **kw).counted_pixels == 70 * 21
    assert plan(rtc, y0=8, y1=45, band_stride=2, grid_y=3, mode=L.MODE_RENDER, **kw).counted_pixels == 69 * 20
    assert plan(rtc, y0=8, y1=45, band_stride=2, grid_y=3, **kw).launch_pixels == 70 * 24     # (the thresholds' measure: whole tile rows)


def test_bad_arguments(rtc):
    import ctypes as C
    f = rtc.lib().rtc_debug_plan_launch
    f.restype, f.argtypes = C.c_int, [C.POINTER(L.Inputs), C.POINTER(L.Plan)]
    i, p = L.Inputs(kind=3), L.Plan()
    assert f(None, C.byref(p)) == 4 and f(C.byref(i), None) == 4 and f(C.byref(i), C.byref(p)) == 4
