"""The [host] half of the ambient-occlusion pass (include/rtc.h): the sample table, the ray of a sample, the packing and the
compositing rule, each pinned against an independent numpy restatement; the ABI; the YAML keys; and, with the CPU oracle
alone, that every case tests/test_gpu_ao.py renders exercises the count (ao_cases.conditions). No GPU is used."""
import ctypes as C
import importlib
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ao_cases as AO
import aov_cases as A

ROOT = Path(__file__).resolve().parents[1]
ERR_ARG = 4


def _abi(rtc):
    return importlib.import_module(rtc.__name__ + ".abi")


# ---- the sample table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("usteps,vsteps", [(1, 1), (1, 256), (256, 1), (16, 16), (3, 5)])
def test_sample_table_is_the_formula(rtc, usteps, vsteps):
    dirs = rtc.ao_expand(rtc.ao(1.0, usteps, vsteps))
    assert dirs.shape == (usteps * vsteps, 3)
    v, u = np.divmod(np.arange(usteps * vsteps), usteps)   # k = v*usteps + u: v outer, u inner
    r = np.sqrt((u + 0.5) / usteps)
    phi = 2.0 * np.pi * (v + 0.5) / vsteps
    want = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - r * r)], axis=1)
    assert np.abs(dirs - want).max() <= 1e-15
    assert (dirs[:, 2] > 0.0).all()
    length = np.sqrt((dirs * dirs).sum(axis=1))
    assert np.abs(length - 1.0).max() <= 4 * np.finfo(np.float64).eps
    if usteps > 1:   # the order: u runs first, and with it the distance from the pole grows
        assert (np.diff(dirs[:usteps, 2]) < 0).all() and dirs[usteps - 1, 2] < dirs[0, 2]
    if usteps > 1 and vsteps > 1:
        assert dirs[usteps, 2] == dirs[0, 2] and not np.array_equal(dirs[usteps, :2], dirs[0, :2])


def test_sample_table_does_not_depend_on_the_radius(rtc):
    assert np.array_equal(rtc.ao_expand(rtc.ao(0.25, 4, 4)), rtc.ao_expand(rtc.ao(math.inf, 4, 4)))


@pytest.mark.parametrize("radius,usteps,vsteps", [(1.0, 0, 4), (1.0, 4, 0), (1.0, 257, 1), (1.0, 1, 257), (1.0, 16, 17), (1.0, 65536, 65536),
                                                  (0.0, 2, 2), (-1.0, 2, 2), (-math.inf, 2, 2), (math.nan, 2, 2)])
def test_bad_passes_are_refused(rtc, radius, usteps, vsteps):
    abi = _abi(rtc)
    a = abi.RtcAo(radius, usteps, vsteps)
    L = rtc.lib()
    assert L.rtc_ao_validate(C.byref(a)) == ERR_ARG
    dirs, n = np.full(3 * abi.MAX_AO_SAMPLES, 7.0), C.c_uint32(99)
    assert L.rtc_ao_expand(C.byref(a), dirs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)) == ERR_ARG
    assert (dirs == 7.0).all() and n.value == 99
    with pytest.raises(rtc.RtcError):
        rtc.ao(radius, usteps, vsteps)


def test_good_passes_are_accepted(rtc):
    L, abi = rtc.lib(), _abi(rtc)
    for radius, usteps, vsteps in [(5e-324, 1, 1), (math.inf, 16, 16), (1.0, 256, 1), (1.0, 1, 256)]:
        assert L.rtc_ao_validate(C.byref(abi.RtcAo(radius, usteps, vsteps))) == 0
    assert L.rtc_ao_validate(None) == ERR_ARG
    a = abi.RtcAo(1.0, 2, 2)
    assert L.rtc_ao_expand(C.byref(a), None, C.byref(C.c_uint32())) == ERR_ARG


# ---- the ray --------------------------------------------------------------------------------------------------------------
def _ray_restated(n, over, l):
    """The header's arithmetic in numpy float64 scalars, term by term, left to right."""
    f = np.float64
    nx, ny, nz = f(n[0]), f(n[1]), f(n[2])
    lx, ly, lz = f(l[0]), f(l[1]), f(l[2])
    one = f(1.0)
    with np.errstate(all="ignore"):
        sign = np.copysign(one, nz)
        a = -one / (sign + nz)
        b = (nx * ny) * a
        t = (one + ((sign * nx) * nx) * a, sign * b, -(sign * nx))
        s = (b, sign + ((ny * ny) * a), -ny)
        d = [((t[c] * lx) + (s[c] * ly)) + ((nx, ny, nz)[c] * lz) for c in range(3)]
    return np.array([f(over[0]), f(over[1]), f(over[2])] + d), np.array(t), np.array(s)


def _normals():
    rng = np.random.default_rng(20240607)
    v = rng.normal(size=(200, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    return [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.0, 0.0, -0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)] + [tuple(r) for r in v]


def test_ray_is_the_headers_arithmetic_bit_for_bit(rtc):
    dirs = rtc.ao_expand(rtc.ao(1.0, 4, 4))
    over = (0.3, -1.25, 7.5)
    for i, n in enumerate(_normals()):
        for local in (dirs[i % 16], dirs[(5 * i + 3) % 16], (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)):
            got = rtc.ao_ray(n, over, local)
            want, t, s = _ray_restated(n, over, local)
            assert got.tobytes() == want.tobytes(), (n, tuple(local))
            if n == (0.0, 0.0, -0.0):
                continue   # a zero vector is no normal: its "frame" is pinned bit for bit above and is not orthonormal
            nn = np.array(n)
            for a, b, dot in ((t, t, 1.0), (s, s, 1.0), (t, s, 0.0), (t, nn, 0.0), (s, nn, 0.0)):
                assert abs(float(np.dot(a, b)) - dot) <= 1e-15, (n, a, b)
            assert abs(float(np.dot(got[3:], nn)) - float(local[2])) <= 1e-15
    L = rtc.lib()
    v = (C.c_double * 3)(0.0, 0.0, 1.0)
    assert L.rtc_ao_ray(None, v, v, (C.c_double * 6)()) == ERR_ARG and L.rtc_ao_ray(v, v, v, None) == ERR_ARG


def test_ray_about_the_pole_is_the_local_direction(rtc):
    """About (0, 0, 1) the frame is the identity; about (0, 0, -1) it is a half turn about x: the hemisphere follows the normal."""
    for local in rtc.ao_expand(rtc.ao(1.0, 3, 4)):
        up = rtc.ao_ray((0.0, 0.0, 1.0), (1.0, 2.0, 3.0), local)
        down = rtc.ao_ray((0.0, 0.0, -1.0), (1.0, 2.0, 3.0), local)
        assert np.array_equal(up[:3], [1.0, 2.0, 3.0]) and np.array_equal(up[3:], local)
        assert np.array_equal(down[3:], [local[0], -local[1], -local[2]])


# ---- packing and compositing ------------------------------------------------------------------------------------------------
def test_from_hits_applies_the_mode_and_miss_rules(rtc):
    width, height = 5, 4
    hits = (rtc.RtcHit * (width * height))()
    rec = np.frombuffer(hits, dtype=A.HIT_DTYPE)
    rec["hit_index"] = np.where(np.arange(width * height) % 3 == 0, -1, 2)
    counts = (np.arange(width * height) + 1).astype(np.uint16)
    hit = (rec["hit_index"] >= 0).reshape(height, width)
    want_async = np.where(hit, counts.reshape(height, width), 0).astype(np.uint16)
    assert np.array_equal(rtc.ao_from_hits(hits, counts, width, height, 1), want_async)
    want_serial = want_async.copy()
    want_serial[-1, :] = 0
    want_serial[:, -1] = 0
    assert np.array_equal(rtc.ao_from_hits(hits, counts, width, height, 0), want_serial) and not np.array_equal(want_serial, want_async)
    L = rtc.lib()
    out = np.zeros(width * height, dtype=np.uint16)
    cp, op = counts.ctypes.data_as(C.POINTER(C.c_uint16)), out.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.rtc_ao_from_hits(hits, cp, width, height, 2, op) == ERR_ARG
    assert L.rtc_ao_from_hits(None, cp, width, height, 1, op) == ERR_ARG
    assert L.rtc_ao_from_hits(hits, None, width, height, 1, op) == ERR_ARG
    assert L.rtc_ao_from_hits(hits, cp, width, height, 1, None) == ERR_ARG


@pytest.mark.parametrize("strength", [0.0, 0.5, 1.0, 0.3])
@pytest.mark.parametrize("n", [1, 9, 256])
def test_apply_is_the_rule_bit_for_bit(rtc, strength, n):
    rng = np.random.default_rng(n)
    height, width = 7, 11
    rgb = rng.uniform(-0.5, 2.0, size=(height, width, 3))
    rgb[0, 0] = [0.0, -0.0, 1.0]
    ao = rng.integers(0, n + 1, size=(height, width)).astype(np.uint16)
    ao[0, :3] = [0, n, n // 2]
    want = rgb * (np.float64(1.0) - np.float64(strength) * (ao.astype(np.float64) / np.float64(n)))[:, :, None]
    got = rtc.apply_ao(rgb, ao, n, strength)
    assert got.tobytes() == want.tobytes()
    if strength == 0.0:
        assert got.tobytes() == rgb.tobytes()
    if strength == 1.0:
        assert (got[ao == n] == 0.0).all() and np.array_equal(got[ao == 0], rgb[ao == 0])


def test_apply_refuses_bad_parameters(rtc):
    L = rtc.lib()
    rgb, ao = np.ones(12), np.ones(4, dtype=np.uint16)
    rp, ap = rgb.ctypes.data_as(C.POINTER(C.c_double)), ao.ctypes.data_as(C.POINTER(C.c_uint16))
    for n, strength in [(0, 0.5), (4, -0.1), (4, 1.5), (4, math.nan), (4, math.inf)]:
        assert L.rtc_canvas_apply_ao(rp, ap, n, strength, 2, 2) == ERR_ARG
    assert L.rtc_canvas_apply_ao(None, ap, 4, 0.5, 2, 2) == ERR_ARG and L.rtc_canvas_apply_ao(rp, None, 4, 0.5, 2, 2) == ERR_ARG
    assert (rgb == 1.0).all()
    assert L.rtc_canvas_apply_ao(rp, ap, 4, 1.0, 2, 2) == 0 and (rgb == 0.75).all()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
AO_SYMBOLS = ("rtc_ao_validate", "rtc_ao_expand", "rtc_ao_ray", "rtc_ao_from_hits", "rtc_render_ao_device", "rtc_render_ao", "rtc_canvas_apply_ao",
              "rtc_canvas_apply_ao_device", "rtc_scene_load_yaml_ao", "rtc_scene_load_yaml_ao_file")


def test_struct_layout_and_symbols(rtc, tmp_path):
    abi = _abi(rtc)
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "rtc.h"
    int main(void){ printf("%zu %zu %zu %zu %u", sizeof(rtc_ao), offsetof(rtc_ao, radius), offsetof(rtc_ao, usteps), offsetof(rtc_ao, vsteps),
                           (unsigned)RTC_MAX_AO_SAMPLES); return 0; }'''
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [16, 0, 8, 12, 256]
    assert [C.sizeof(abi.RtcAo), abi.RtcAo.radius.offset, abi.RtcAo.usteps.offset, abi.RtcAo.vsteps.offset, abi.MAX_AO_SAMPLES] == out
    header = (ROOT / "include" / "rtc.h").read_text()
    declared = set(re.findall(r"\b(rtc_[a-z0-9_]+)\s*\(", header))
    L = rtc.lib()
    for name in AO_SYMBOLS:
        assert name in declared and name in abi.PROTOTYPES and getattr(L, name) is not None, name
    for name in ("ao", "ao_expand", "ao_ray", "ao_from_hits", "apply_ao", "load_yaml_ao"):
        assert name in rtc.__all__ and callable(getattr(rtc, name)), name
    assert callable(rtc.DeviceWorld.render_ao) and callable(rtc.DeviceWorld.render_ao_device) and callable(rtc.Context.apply_ao_device)
    # what the pass leaves alone
    assert L.rtc_abi_version() == 3 and C.sizeof(abi.RtcAovBuffers) == 48 and C.sizeof(abi.RtcLaunchInfo) == 48 and C.sizeof(abi.RtcShape) == 528


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
    w, cam, lens, ao = rtc.load_yaml_ao(text=SCENE % "  ao-radius: 0.75\n  ao-usteps: 3\n  ao-vsteps: 5")
    assert len(w) == 2 and (cam.hsize, cam.vsize) == (40, 30) and lens is None
    assert (ao.radius, ao.usteps, ao.vsteps) == (0.75, 3, 5)
    _, _, _, ao = rtc.load_yaml_ao(text=SCENE % "  ao-radius: 2")
    assert (ao.radius, ao.usteps, ao.vsteps) == (2.0, 4, 4)   # the default grid
    for spelling in (".inf", "inf"):
        _, _, _, ao = rtc.load_yaml_ao(text=SCENE % ("  ao-radius: %s\n  ao-usteps: 16\n  ao-vsteps: 16" % spelling))
        assert ao.radius == math.inf and ao.usteps * ao.vsteps == 256
    # absent keys: no pass; lens keys travel as rtc_scene_load_yaml_lens has them
    _, _, lens, ao = rtc.load_yaml_ao(text=SCENE % "")
    assert ao is None and lens is None
    _, _, lens, ao = rtc.load_yaml_ao(text=SCENE % "  aperture: 0.1\n  focal-distance: 7\n  ao-radius: 1")
    assert lens is not None and lens.aperture == 0.1 and ao.radius == 1.0
    for bad in ("  ao-usteps: 4", "  ao-radius: 0", "  ao-radius: -1", "  ao-radius: nan", "  ao-radius: 1\n  ao-usteps: 0",
                "  ao-radius: 1\n  ao-usteps: 2.5", "  ao-radius: 1\n  ao-usteps: 17\n  ao-vsteps: 16", "  ao-radius: 1\n  ao-vsteps: 257",
                "  ao-radius: [1, 2]"):
        with pytest.raises(rtc.RtcError) as e:
            rtc.load_yaml_ao(text=SCENE % bad)
        assert e.value.status == 5 and "line" in str(e.value), bad
    # the keys ask for a pass and change no ray: the other entries load the scene and ignore them
    w2, cam2 = rtc.load_yaml(text=SCENE % "  ao-radius: 0.75")
    assert len(w2) == 2 and bytes(cam2) == bytes(cam)


def test_shipped_scene_loads(rtc):
    path = Path(rtc.__file__).resolve().parent / "data" / "ambient_occlusion.yml"
    w, cam, lens, ao = rtc.load_yaml_ao(path=path)
    assert lens is None and (ao.radius, ao.usteps, ao.vsteps) == (1.5, 4, 4)
    assert sorted(s.kind for s in w.shapes) == sorted([rtc.PLANE, rtc.SPHERE, rtc.CUBE]) and (cam.hsize, cam.vsize) == (320, 200)
    w2, _, _, ao2 = rtc.load_yaml_ao(text=path.read_text())
    assert len(w2) == 3 and bytes(ao2) == bytes(ao)


# ---- the GPU tests' cases, checked with the oracle alone --------------------------------------------------------------------
@pytest.mark.parametrize("name,ao", AO.CASES, ids=[f"{n}-{a[0]}-{a[1]}x{a[2]}" for n, a in AO.CASES])
def test_cases_exercise_the_count(rtc, O, name, ao):
    w, cam = AO.world(rtc, name)
    plane = AO.expected_ao(rtc, O, name, ao, 1)
    c = plane[AO.hit_mask(rtc, O, name)]
    print(name, ao, f"{cam.hsize}x{cam.vsize}", len(w), "objects; counts:", dict(zip(*[v.tolist() for v in np.unique(c, return_counts=True)])))
    assert AO.conditions(rtc, O, name, ao) == []
    assert plane.dtype == np.uint16 and plane.shape == (cam.vsize, cam.hsize) and int(plane.max()) <= ao[1] * ao[2]
    assert (plane[~AO.hit_mask(rtc, O, name)] == 0).all()
    assert cam.hsize % 8 and cam.vsize % 8   # partial tiles on both edges


def test_cases_cover_what_the_kernel_distinguishes(rtc, O):
    worlds = {n.split(":")[0] for n, _ in AO.CASES}
    assert worlds == {"contact", "closeup", "grid290", "inside"}
    assert len(AO.world(rtc, "contact")[0]) == 3 and len(AO.world(rtc, "grid290")[0]) == 290   # one-level and two-level cull
    assert not AO.hit_mask(rtc, O, "contact").all()   # sky pixels: the miss rule
    hits = AO.oracle_hits(rtc, O, "inside")
    assert all(h.inside for h in hits if h.hit_index == 0) and sum(h.hit_index == 0 for h in hits) > 100   # the flipped normal
    grids = {(a[1], a[2]) for _, a in AO.CASES}
    assert {(1, 1), (2, 2), (4, 4), (16, 16)} <= grids
    radii = {a[0] for _, a in AO.CASES}
    assert 0.25 in radii and math.inf in radii and any(1.0 <= r <= 4.0 for r in radii)
    for name, ao in AO.SERIAL_CASES:   # RTC_MODE_RENDER: the last row and column hold 0 and would not otherwise
        serial, free = AO.expected_ao(rtc, O, name, ao, 0), AO.expected_ao(rtc, O, name, ao, 1)
        assert (serial[-1, :] == 0).all() and (serial[:, -1] == 0).all() and (free[-1, :] > 0).any() and (free[:, -1] > 0).any()
        assert np.array_equal(serial[:-1, :-1], free[:-1, :-1])
    # other lights, the same shapes
    for name in ("contact+2", "contact+area256"):
        w, _ = AO.world(rtc, name)
        assert len(w) == 3 and len(w.samples()) == {"contact+2": 2, "contact+area256": 256}[name]
