"""The [host] half of the edge-aware filter (include/rtc.h, "edge-aware filter"): the normative statement against the
independent restatement of tests/filter_cases.py, byte for byte; the record's ranges; the fraction and the compositing entry
against rtc_canvas_apply_ao; the ABI; the YAML keys; the statement under AddressSanitizer in a stand-alone program; and what the
defaults are chosen for, on the scene of data/ambient_occlusion.yml with the CPU oracle's counts. No GPU is used."""
import ctypes as C
import importlib
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import filter_cases as FC

ROOT = Path(__file__).resolve().parents[1]
ERR_ARG = 4
PD = C.POINTER(C.c_double)


def _abi(rtc):
    return importlib.import_module(rtc.__name__ + ".abi")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- the statement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.NAMES)
def test_host_statement_equals_the_restatement(rtc, name):
    values, planes = FC.arrays(name)
    got = rtc.plane_filter(values, planes, FC.spec(rtc, name))
    want = FC.expected(name)
    assert got.shape == want.shape
    d = np.argwhere(_bits(got) != _bits(want))
    assert len(d) == 0, f"{name}: {len(d)} values differ, first at {d[0].tolist()}: got {got[tuple(d[0])]!r}, want {want[tuple(d[0])]!r}"
    miss = planes["index"] < 0
    assert np.array_equal(_bits(got)[miss], _bits(values)[miss])   # a miss is copied bit for bit
    if "allmiss" not in name and "tiny" not in name and name != "1x1":
        assert (_bits(got) != _bits(values)).any()   # ... and the filter does something


@pytest.mark.parametrize("name", ["37x29-tiny", "37x29-tiny-c3"])
def test_tiny_sigma_leaves_only_the_centre_tap(rtc, name):
    """With plane_sigma = 1e-300 every neighbour fails the plane test, so a pixel's value is (w * v) / w of its centre tap. That
    is v bit for bit whenever w * v is exact: here w = 0.140625 exactly (axis normals: n.n = 1) and v = k / 256."""
    values, planes = FC.arrays(name)
    assert (planes["index"] >= 0).all()
    got = rtc.plane_filter(values, planes, FC.spec(rtc, name))
    assert got.tobytes() == values.tobytes() and FC.expected(name).tobytes() == values.tobytes()


@pytest.mark.parametrize("name", ["37x29-poison", "37x29-poison-c3"])
def test_inf_and_nan_under_a_zero_weight_reach_no_neighbour(rtc, name):
    values, planes = FC.arrays(name)
    got = rtc.plane_filter(values, planes, FC.spec(rtc, name))
    poisoned = np.zeros(values.shape[:2], dtype=bool)
    for x, y in FC.POISON_AT:
        poisoned[y, x] = True
        assert not np.isfinite(got[y, x]).any() and not np.isfinite(values[y, x]).any()
    assert np.isfinite(got[~poisoned]).all()
    (x, y) = FC.POISON_AT[1]
    assert (_bits(got[y, x]) == 0x7FF8000000000000).all()   # the NaN quotient's bits


@pytest.mark.parametrize("name", ["37x29-planes", "37x29-patches-c3"])
def test_nan_guides_drop_taps_and_poison_nothing(rtc, name):
    values, planes = FC.arrays(name)
    got = rtc.plane_filter(values, planes, FC.spec(rtc, name))
    assert np.isfinite(got).all()
    for x, y in (FC.NAN_NORMAL_AT, FC.NAN_POINT_AT):   # no tap of theirs survives, the centre included: copied
        assert np.array_equal(_bits(got[y, x]), _bits(values[y, x]))


def test_step_16_reaches_what_the_size_allows(rtc):
    """The last of five passes has taps 16 and 32 pixels apart: in a 16 x 16 image none but the centre is in range, in a
    17 x 17 image exactly the corner and edge pixels reach one neighbour per side."""
    for size, reach in ((16, False), (17, True)):
        index = np.zeros((size, size), dtype=np.int32)
        planes = {"index": index, "point": np.zeros((size, size, 3)), "normal": np.tile(np.array([0.0, 0.0, 1.0]), (size, size, 1))}
        four = rtc.filter_spec(math.inf, passes=4, normal_squarings=0, same_object=False)
        five = rtc.filter_spec(math.inf, passes=5, normal_squarings=0, same_object=False)
        values = np.random.default_rng(size).integers(0, 1 << 20, size=(size, size)).astype(np.float64)
        a, b = rtc.plane_filter(values, planes, four), rtc.plane_filter(values, planes, five)
        # centre only: (0.140625 * v) / 0.140625; the four-pass values are sums of few-bit terms, so compare with a tolerance of one ulp
        changed = np.abs(a - b) > np.spacing(np.abs(a))
        assert changed.any() == reach
        if reach:
            assert changed[0, 0] and changed[0, 16] and changed[16, 0] and changed[16, 16] and not changed[1:16, 1:16].any()


# ---- the record and the arguments ---------------------------------------------------------------------------------------------
def test_validate_refuses_every_range_at_its_edge(rtc):
    L, abi = rtc.lib(), _abi(rtc)
    good = [(5e-324, 1, 0, 0), (math.inf, 5, 8, 1), (0.05, 3, 1, 1), (1e308, 1, 8, 0)]
    bad = [(0.0, 3, 1, 0), (-0.0, 3, 1, 0), (-1.0, 3, 1, 0), (-math.inf, 3, 1, 0), (math.nan, 3, 1, 0), (0.05, 0, 1, 0), (0.05, 6, 1, 0),
           (0.05, 2 ** 32 - 1, 1, 0), (0.05, 3, 9, 0), (0.05, 3, 2 ** 32 - 1, 0), (0.05, 3, 1, 2), (0.05, 3, 1, 3), (0.05, 3, 1, 1 << 31)]
    for sigma, passes, squarings, flags in good:
        assert L.rtc_filter_validate(C.byref(abi.RtcFilter(sigma, passes, squarings, flags, 0))) == 0, (sigma, passes, squarings, flags)
    for sigma, passes, squarings, flags in bad:
        assert L.rtc_filter_validate(C.byref(abi.RtcFilter(sigma, passes, squarings, flags, 0))) == ERR_ARG, (sigma, passes, squarings, flags)
    assert L.rtc_filter_validate(C.byref(abi.RtcFilter(0.05, 3, 1, 0, 1))) == ERR_ARG   # _pad
    assert L.rtc_filter_validate(None) == ERR_ARG
    with pytest.raises(rtc.RtcError):
        rtc.filter_spec(0.05, passes=6)
    d = rtc.filter_spec()
    assert (d.plane_sigma, d.passes, d.normal_squarings, d.flags) == (abi.FILTER_DEFAULT_PLANE_SIGMA, abi.FILTER_DEFAULT_PASSES,
                                                                     abi.FILTER_DEFAULT_NORMAL_SQUARINGS, abi.FILTER_SAME_OBJECT)


def test_filter_refuses_bad_arguments_and_writes_nothing(rtc):
    L, abi = rtc.lib(), _abi(rtc)
    values, planes = FC.arrays("5x3-c3")
    src = np.array(values)
    out = np.full(values.shape, 7.0)
    g = {k: np.array(v) for k, v in planes.items()}
    flt = FC.spec(rtc, "5x3-c3")

    def call(inp=src, ch=3, guides=g, f=flt, dst=out, null=None):
        b = abi.RtcAovBuffers(**{k: (None if k == null else v.ctypes.data) for k, v in guides.items()})
        return L.rtc_plane_filter(None if inp is None else inp.ctypes.data_as(PD), ch, C.byref(b), 5, 3, None if f is None else C.byref(f),
                                  None if dst is None else dst.ctypes.data_as(PD))

    assert call(dst=src) == ERR_ARG   # in == out
    for ch in (0, 2, 4):
        assert call(ch=ch) == ERR_ARG
    for null in ("index", "point", "normal"):
        assert call(null=null) == ERR_ARG
    assert call(inp=None) == ERR_ARG and call(dst=None) == ERR_ARG and call(f=None) == ERR_ARG
    assert call(f=abi.RtcFilter(0.0, 3, 1, 0, 0)) == ERR_ARG
    assert L.rtc_plane_filter(src.ctypes.data_as(PD), 3, None, 5, 3, C.byref(flt), out.ctypes.data_as(PD)) == ERR_ARG
    assert (out == 7.0).all() and src.tobytes() == values.tobytes()
    assert call() == 0 and out.tobytes() == FC.expected("5x3-c3").tobytes()
    # the three other planes are ignored
    extra = dict(g, depth=np.zeros(1), flags=np.zeros(1, dtype=np.uint8), shadow=np.zeros(1, dtype=np.uint16))
    out2 = np.empty_like(out)
    assert call(guides=extra, dst=out2) == 0 and out2.tobytes() == out.tobytes()


# ---- the fraction and the compositing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", [1, 9, 16, 256])
def test_fraction_then_occlusion_is_apply_ao(rtc, strength, n):
    rng = np.random.default_rng(n)
    height, width = 7, 11
    rgb = rng.uniform(-0.5, 2.0, size=(height, width, 3))
    rgb[0, 0] = [0.0, -0.0, 1.0]
    counts = rng.integers(0, n + 1, size=(height, width)).astype(np.uint16)
    counts[0, :3] = [0, n, n // 2]
    occ = rtc.counts_to_fraction(counts, n)
    assert occ.tobytes() == (counts.astype(np.float64) / np.float64(n)).tobytes()
    got = rtc.apply_occlusion(rgb, occ, strength)
    assert got.tobytes() == rtc.apply_ao(rgb, counts, n, strength).tobytes()
    assert got.tobytes() == (rgb * (np.float64(1.0) - np.float64(strength) * occ)[:, :, None]).tobytes()


def test_fraction_and_occlusion_refuse_bad_parameters(rtc):
    L = rtc.lib()
    rgb, occ, counts = np.ones(12), np.full(4, 0.25), np.ones(4, dtype=np.uint16)
    rp, op, cp = rgb.ctypes.data_as(PD), occ.ctypes.data_as(PD), counts.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.rtc_counts_to_fraction(cp, 0, 2, 2, op) == ERR_ARG
    assert L.rtc_counts_to_fraction(None, 4, 2, 2, op) == ERR_ARG and L.rtc_counts_to_fraction(cp, 4, 2, 2, None) == ERR_ARG
    for strength in (-0.1, 1.5, math.nan, math.inf):
        assert L.rtc_canvas_apply_occlusion(rp, op, strength, 2, 2) == ERR_ARG
    assert L.rtc_canvas_apply_occlusion(None, op, 0.5, 2, 2) == ERR_ARG and L.rtc_canvas_apply_occlusion(rp, None, 0.5, 2, 2) == ERR_ARG
    assert (rgb == 1.0).all() and (occ == 0.25).all()
    assert L.rtc_canvas_apply_occlusion(rp, op, 1.0, 2, 2) == 0 and (rgb == 0.75).all()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
FILTER_SYMBOLS = ("rtc_filter_validate", "rtc_plane_filter", "rtc_plane_filter_device", "rtc_counts_to_fraction", "rtc_counts_to_fraction_device",
                  "rtc_canvas_apply_occlusion", "rtc_canvas_apply_occlusion_device", "rtc_scene_load_yaml_filter", "rtc_scene_load_yaml_filter_file")


def test_struct_layout_and_symbols(rtc, tmp_path):
    abi = _abi(rtc)
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "rtc.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %u %u %u %u %.17g", sizeof(rtc_filter), offsetof(rtc_filter, plane_sigma), offsetof(rtc_filter, passes),
                           offsetof(rtc_filter, normal_squarings), offsetof(rtc_filter, flags), offsetof(rtc_filter, _pad),
                           (unsigned)RTC_FILTER_SAME_OBJECT, (unsigned)RTC_MAX_FILTER_PASSES, (unsigned)RTC_FILTER_DEFAULT_PASSES,
                           (unsigned)RTC_FILTER_DEFAULT_NORMAL_SQUARINGS, (double)RTC_FILTER_DEFAULT_PLANE_SIGMA); return 0; }'''
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out[:6]] == [24, 0, 8, 12, 16, 20]
    F = abi.RtcFilter
    assert [C.sizeof(F), F.plane_sigma.offset, F.passes.offset, F.normal_squarings.offset, F.flags.offset, F._pad.offset] == [24, 0, 8, 12, 16, 20]
    assert [int(v) for v in out[6:10]] == [abi.FILTER_SAME_OBJECT, abi.MAX_FILTER_PASSES, abi.FILTER_DEFAULT_PASSES, abi.FILTER_DEFAULT_NORMAL_SQUARINGS]
    assert float(out[10]) == abi.FILTER_DEFAULT_PLANE_SIGMA
    header = (ROOT / "include" / "rtc.h").read_text()
    declared = set(re.findall(r"\b(rtc_[a-z0-9_]+)\s*\(", header))
    L = rtc.lib()
    for name in FILTER_SYMBOLS:
        assert name in declared and name in abi.PROTOTYPES and getattr(L, name) is not None, name
    for name in ("filter_spec", "plane_filter", "counts_to_fraction", "apply_occlusion", "load_yaml_filter"):
        assert name in rtc.__all__ and callable(getattr(rtc, name)), name
    assert callable(rtc.Context.plane_filter_device) and callable(rtc.Context.counts_to_fraction_device) and callable(rtc.Context.apply_occlusion_device)
    assert L.rtc_abi_version() == 3 and C.sizeof(abi.RtcAovBuffers) == 48 and C.sizeof(abi.RtcAo) == 16


# ---- YAML -------------------------------------------------------------------------------------------------------------------
SCENE = """
- add: camera
  width: 40
  height: 30
  field-of-view: 0.8
  from: [0, 1.5, -7]
  to: [0, 1, 0]
  up: [0, 1, 0]
%s
- add: light
  at: [-6, 8, -8]
  intensity: [1, 1, 1]
- add: plane
- add: sphere
  transform: [[translate, 0, 1, 0]]
"""


def test_yaml_keys(rtc):
    abi = _abi(rtc)
    w, cam, lens, ao, gather, flt = rtc.load_yaml_filter(text=SCENE % "  filter-plane-sigma: 0.2\n  filter-passes: 4\n  filter-normal-squarings: 2")
    assert len(w) == 2 and (cam.hsize, cam.vsize) == (40, 30) and lens is None and ao is None and gather is None
    assert (flt.plane_sigma, flt.passes, flt.normal_squarings, flt.flags, flt._pad) == (0.2, 4, 2, abi.FILTER_SAME_OBJECT, 0)
    flt = rtc.load_yaml_filter(text=SCENE % "  filter-plane-sigma: 0.5")[5]
    assert (flt.plane_sigma, flt.passes, flt.normal_squarings) == (0.5, abi.FILTER_DEFAULT_PASSES, abi.FILTER_DEFAULT_NORMAL_SQUARINGS)
    for spelling in (".inf", "inf"):
        flt = rtc.load_yaml_filter(text=SCENE % ("  filter-plane-sigma: %s\n  filter-passes: 5\n  filter-normal-squarings: 0" % spelling))[5]
        assert flt.plane_sigma == math.inf and (flt.passes, flt.normal_squarings) == (5, 0)
    assert rtc.load_yaml_filter(text=SCENE % "")[2:] == (None, None, None, None)
    # the other passes' keys travel as rtc_scene_load_yaml_gather has them
    _, _, lens, ao, gather, flt = rtc.load_yaml_filter(text=SCENE % "  ao-radius: 1\n  gather-radius: 2\n  gather-usteps: 2\n  filter-plane-sigma: 1")
    assert lens is None and ao.radius == 1.0 and (gather.radius, gather.usteps, gather.vsteps) == (2.0, 2, 4) and flt.plane_sigma == 1.0
    for bad in ("  filter-passes: 3", "  filter-normal-squarings: 1", "  filter-plane-sigma: 0", "  filter-plane-sigma: -1", "  filter-plane-sigma: nan",
                "  filter-plane-sigma: 1\n  filter-passes: 0", "  filter-plane-sigma: 1\n  filter-passes: 6", "  filter-plane-sigma: 1\n  filter-passes: 2.5",
                "  filter-plane-sigma: 1\n  filter-normal-squarings: 9", "  filter-plane-sigma: 1\n  filter-normal-squarings: -1",
                "  filter-plane-sigma: [1, 2]"):
        with pytest.raises(rtc.RtcError) as e:
            rtc.load_yaml_filter(text=SCENE % bad)
        assert e.value.status == 5 and "line" in str(e.value), bad
    # the keys ask for a pass and change no other entry's result
    text = SCENE % "  ao-radius: 0.75\n  filter-plane-sigma: 0.2\n  filter-passes: 2"
    w2, cam2 = rtc.load_yaml(text=text)
    assert len(w2) == 2 and bytes(cam2) == bytes(cam)
    _, cam3, _, ao3, gather3 = rtc.load_yaml_gather(text=text)
    assert bytes(cam3) == bytes(cam) and ao3.radius == 0.75 and gather3 is None


def test_shipped_scene_loads(rtc):
    abi = _abi(rtc)
    path = Path(rtc.__file__).resolve().parent / "data" / "filtered_occlusion.yml"
    w, cam, lens, ao, gather, flt = rtc.load_yaml_filter(path=path)
    assert lens is None and ao is not None and gather is not None and flt is not None
    assert (ao.usteps, ao.vsteps) == (4, 4) and rtc.lib().rtc_filter_validate(C.byref(flt)) == 0 and flt.flags == abi.FILTER_SAME_OBJECT
    w2, _, _, _, _, flt2 = rtc.load_yaml_filter(text=path.read_text())
    assert len(w2) == len(w) and bytes(flt2) == bytes(flt)


# ---- the statement under the sanitizers -----------------------------------------------------------------------------------------
def test_filter_under_asan_and_ubsan(tmp_path):
    """host_filter.cpp compiled with -fsanitize=address,undefined and driven by tests/cpp/test_filter_asan.cpp over the edge sizes,
    every plane in a heap buffer of exactly its size. (Sanitizers run on the CPU build only; nothing is loaded into Python.)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = ROOT / "raytracer-challenge_amd" / "csrc"
    exe = tmp_path / "test_filter_asan"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", f"-I{ROOT / 'include'}", f"-I{csrc}", str(ROOT / "tests" / "cpp" / "test_filter_asan.cpp"),
           str(csrc / "host_filter.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert re.search(r"no crash: \d+ runs", r.stdout)


# ---- what the defaults are for ---------------------------------------------------------------------------------------------------
def _oracle_planes(rtc, O, w, cam, grids, radius):
    """The oracle's centre-ray records of every pixel, as tests/ao_cases.py takes them, and per grid the occluded-sample counts:
    one oracle color_at per sample on rtc_ao_ray of the oracle's normal and over_point, counting a hit at t < radius."""
    arr, n, lgt = w.array(), len(w), w.samples()[0]
    width, height = cam.hsize, cam.vsize
    hits = (rtc.RtcHit * (width * height))()
    for y in range(height):
        for x in range(width):
            _, h = O.color_at(arr, n, lgt, tuple(rtc.ray_for_pixel(cam, x, y)), 0, want_hit=True)
            C.memmove(C.byref(hits, (y * width + x) * C.sizeof(rtc.RtcHit)), C.byref(h), C.sizeof(rtc.RtcHit))
    color_at, rgb, rec = O.lib().orc_color_at, O.Vec3(), O.RtcHit()   # the call O.color_at makes, without its per-call allocations
    counts = {}
    for us, vs in grids:
        dirs = rtc.ao_expand(rtc.ao(radius, us, vs))
        c = np.zeros(width * height, dtype=np.uint16)
        for i in range(width * height):
            h = hits[i]
            if h.hit_index < 0:
                continue
            normal, over = tuple(h.normal), tuple(h.over_point)
            for local in dirs:
                color_at(arr, n, C.byref(lgt), O.Ray6(*rtc.ao_ray(normal, over, local)), 0, rgb, C.byref(rec))
                c[i] += rec.hit_index >= 0 and rec.t < radius
        counts[(us, vs)] = rtc.ao_from_hits(hits, c, width, height, 1)
    return hits, counts


def test_default_filter_brings_4x4_samples_closer_to_16x16(rtc, O):
    """data/ambient_occlusion.yml at 96 x 54: RMS(filtered 4x4 - 16x16) < RMS(raw 4x4 - 16x16), all fractions, the filter with
    rtc.h's defaults under the oracle's own guides. Measured over all 5184 pixels (profiles/filter_quality.log): raw 4x4
    0.057457, default-filtered 4x4 0.044678. At this size a contact shadow is a few pixels wide: a third pass (taps 4 and 8 pixels
    apart) already blurs it away (0.0576), which is why the default is two."""
    path = Path(rtc.__file__).resolve().parent / "data" / "ambient_occlusion.yml"
    text = path.read_text().replace("width: 320", "width: 96").replace("height: 200", "height: 54")
    w, cam, _, ao = rtc.load_yaml_ao(text=text)
    assert (cam.hsize, cam.vsize) == (96, 54) and (ao.usteps, ao.vsteps) == (4, 4)
    hits, counts = _oracle_planes(rtc, O, w, cam, [(4, 4), (16, 16)], ao.radius)
    guides = rtc.aov_from_hits(hits, 96, 54, 1, planes=("index", "point", "normal"))
    low, ref = rtc.counts_to_fraction(counts[(4, 4)], 16), rtc.counts_to_fraction(counts[(16, 16)], 256)
    filtered = rtc.plane_filter(low, guides, rtc.filter_spec())

    def rms(a):
        return float(np.sqrt(np.mean((a - ref) ** 2)))

    print(f"RMS against the 16x16-sample fraction plane, 96x54: raw 4x4 {rms(low):.6f}, default-filtered 4x4 {rms(filtered):.6f}, "
          f"16x16 {rms(ref):.6f}")
    assert (guides["index"] < 0).any() and len(np.unique(guides["index"])) == 4   # sky, floor, sphere, cube
    assert rms(filtered) < rms(low)
