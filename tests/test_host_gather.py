"""The [host] half of the one-bounce gather pass (include/rtc.h "colour bleeding"): the packing rule on hand-made records, the
compositing rule, the ABI, the YAML keys; and, with the CPU oracle alone, that every case tests/test_gpu_gather.py renders
exercises the pass (gather_cases.conditions). No GPU is used."""
import ctypes as C
import importlib
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aov_cases as A
import gather_cases as G

ROOT = Path(__file__).resolve().parents[1]
ERR_ARG = 4
NAN_BITS = 0x7FF8000000000000


def _abi(rtc):
    return importlib.import_module(rtc.__name__ + ".abi")


# ---- packing ----------------------------------------------------------------------------------------------------------------
def _records(rtc, width, height, ns):
    """Hand-made records: pixel i hits unless i % 4 == 3; sample k of pixel i hits unless (i + k) % 5 == 0, at t = 0.25 * (k + 1)."""
    npx = width * height
    hits, recs = (rtc.RtcHit * npx)(), (rtc.RtcHit * (npx * ns))()
    h, r = np.frombuffer(hits, dtype=A.HIT_DTYPE), np.frombuffer(recs, dtype=A.HIT_DTYPE).reshape(npx, ns)
    i, k = np.arange(npx)[:, None], np.arange(ns)[None, :]
    h["hit_index"] = np.where(np.arange(npx) % 4 == 3, -1, 1)
    r["hit_index"] = np.where((i + k) % 5 == 0, -1, 2)
    r["t"] = 0.25 * (k + 1) + 0 * i
    rng = np.random.default_rng(7)
    rgb = rng.uniform(0.0, 1.5, size=(npx, ns, 3))
    alb = rng.uniform(0.0, 1.0, size=(npx, 3))
    return hits, recs, rgb, alb, h, r


def _restated(h, r, rgb, alb, ns, radius, width, height, mode):
    """The header's rule in numpy float64, sample by sample, left to right."""
    npx = width * height
    rad = np.zeros((npx, 3))
    for i in range(npx):
        x, y = i % width, i // width
        if h["hit_index"][i] < 0 or (mode == 0 and (x + 1 >= width or y + 1 >= height)):
            continue
        s = np.zeros(3)
        for k in range(ns):
            counted = r["hit_index"][i, k] >= 0 and r["t"][i, k] < radius
            s = s + (rgb[i, k] if counted else np.zeros(3))
        rad[i] = s / np.float64(ns)
    bounce = alb * rad
    return rad.reshape(height, width, 3), bounce.reshape(height, width, 3)


@pytest.mark.parametrize("mode", [1, 0], ids=["async", "serial"])
@pytest.mark.parametrize("ns,radius", [(4, 0.75), (4, math.inf), (1, 0.3), (9, 1.0)])
def test_from_hits_is_the_rule_bit_for_bit(rtc, ns, radius, mode):
    width, height = 6, 5
    hits, recs, rgb, alb, h, r = _records(rtc, width, height, ns)
    want_rad, want_bounce = _restated(h, r, rgb, alb, ns, radius, width, height, mode)
    got = rtc.gather_from_hits(hits, recs, rgb, alb, ns, radius, width, height, mode)
    assert got["radiance"].tobytes() == want_rad.tobytes() and got["bounce"].tobytes() == want_bounce.tobytes()
    assert want_rad.any() and want_bounce.any()
    miss = (h["hit_index"] < 0).reshape(height, width)
    assert (got["radiance"][miss] == 0.0).all() and (got["bounce"][miss] == 0.0).all()
    if mode == 0:   # the mode rule: the last row and column hold zeros, and would not otherwise
        other = rtc.gather_from_hits(hits, recs, rgb, alb, ns, radius, width, height, 1)
        assert not got["radiance"][-1].any() and not got["radiance"][:, -1].any() and not got["bounce"][-1].any()
        assert other["radiance"][-1].any() and other["radiance"][:, -1].any()
        assert np.array_equal(other["radiance"][:-1, :-1], got["radiance"][:-1, :-1])
    # one plane alone holds the bytes it holds beside the other
    only = rtc.gather_from_hits(hits, recs, rgb, None, ns, radius, width, height, mode, planes=("radiance",))
    assert list(only) == ["radiance"] and only["radiance"].tobytes() == got["radiance"].tobytes()
    only = rtc.gather_from_hits(hits, recs, rgb, alb, ns, radius, width, height, mode, planes=("bounce",))
    assert list(only) == ["bounce"] and only["bounce"].tobytes() == got["bounce"].tobytes()


def test_from_hits_radius_edge_and_sample_order(rtc):
    """t == radius is not counted, the next double below it is; the sum runs in sample order from 0.0."""
    hits, recs = (rtc.RtcHit * 1)(), (rtc.RtcHit * 4)()
    hits[0].hit_index = 0
    for k in range(4):
        recs[k].hit_index = 5
    recs[0].t, recs[1].t, recs[2].t, recs[3].t = 2.0, math.nextafter(2.0, 0.0), 0.5, 1.0
    rgb = np.array([[100.0, 100.0, 100.0], [1e16, 1.0, -0.0], [1.0, 1.0, -0.0], [1.0, 1e16, -0.0]])
    alb = np.array([0.5, 0.25, 2.0])
    got = rtc.gather_from_hits(hits, recs, rgb, alb, 4, 2.0, 1, 1)
    want = np.array([(((0.0 + 0.0) + 1e16) + 1.0) + 1.0, (((0.0 + 0.0) + 1.0) + 1.0) + 1e16, 0.0]) / 4.0
    assert got["radiance"].reshape(3).tobytes() == want.tobytes()
    assert want[0] != want[1]   # the order shows: 1e16 + 1 + 1 is 1e16, 1 + 1 + 1e16 is not
    assert math.copysign(1.0, got["radiance"][0, 0, 2]) == 1.0   # -0.0 samples: the leading 0.0 makes the mean +0.0
    assert got["bounce"].reshape(3).tobytes() == (alb * want).tobytes()
    # a sample that misses adds nothing, whatever colour travels with it
    recs[3].hit_index = -1
    got = rtc.gather_from_hits(hits, recs, rgb, alb, 4, 2.0, 1, 1)
    assert got["radiance"].reshape(3).tolist() == [1e16 / 4.0, 2.0 / 4.0, 0.0]
    # +inf: every hit counts
    got = rtc.gather_from_hits(hits, recs, rgb, alb, 4, math.inf, 1, 1)
    assert got["radiance"][0, 0, 1] == ((0.0 + 100.0) + 1.0 + 1.0) / 4.0


def test_from_hits_stores_one_nan(rtc):
    hits, recs = (rtc.RtcHit * 2)(), (rtc.RtcHit * 4)()
    hits[0].hit_index = hits[1].hit_index = 0
    for k in range(4):
        recs[k].hit_index, recs[k].t = 1, 0.5
    weird = np.frombuffer(np.array([0xFFF0000000000123], dtype=np.uint64).tobytes(), dtype=np.float64)[0]   # a signalling, negative NaN
    rgb = np.array([[weird, math.inf, 1.0], [1.0, -math.inf, 1.0], [1.0, 2.0, 3.0], [3.0, 2.0, 1.0]])
    alb = np.array([[1.0, 1.0, math.nan], [0.0, math.inf, 1.0]])
    got = rtc.gather_from_hits(hits, recs, rgb, alb, 2, 1.0, 2, 1)
    bits = got["radiance"].reshape(-1).view(np.uint64)
    assert bits[0] == NAN_BITS and bits[1] == NAN_BITS and got["radiance"][0, 0, 2] == 1.0
    assert got["radiance"][0, 1].tolist() == [2.0, 2.0, 2.0]
    b = got["bounce"].reshape(-1).view(np.uint64)
    assert b[0] == NAN_BITS and b[1] == NAN_BITS and b[2] == NAN_BITS   # NaN radiance, NaN albedo
    assert got["bounce"][0, 1, 0] == 0.0 and got["bounce"][0, 1, 1] == math.inf and got["bounce"][0, 1, 2] == 2.0


def test_from_hits_refuses_bad_arguments(rtc):
    L, abi = rtc.lib(), _abi(rtc)
    hits, recs, rgb, alb, _, _ = _records(rtc, 3, 2, 2)
    PD = C.POINTER(C.c_double)
    rad, bounce = np.full(18, 7.0), np.full(18, 7.0)
    both = abi.RtcGatherBuffers(rad.ctypes.data, bounce.ctypes.data)
    rp, ap = rgb.ctypes.data_as(PD), alb.ctypes.data_as(PD)
    call = L.rtc_gather_from_hits
    assert call(None, recs, rp, ap, 2, 1.0, 3, 2, 1, C.byref(both)) == ERR_ARG
    assert call(hits, None, rp, ap, 2, 1.0, 3, 2, 1, C.byref(both)) == ERR_ARG
    assert call(hits, recs, None, ap, 2, 1.0, 3, 2, 1, C.byref(both)) == ERR_ARG
    assert call(hits, recs, rp, None, 2, 1.0, 3, 2, 1, C.byref(both)) == ERR_ARG   # bounce wanted, no albedo
    assert call(hits, recs, rp, ap, 2, 1.0, 3, 2, 1, None) == ERR_ARG
    assert call(hits, recs, rp, ap, 2, 1.0, 3, 2, 1, C.byref(abi.RtcGatherBuffers(None, None))) == ERR_ARG
    assert call(hits, recs, rp, ap, 2, 1.0, 3, 2, 2, C.byref(both)) == ERR_ARG
    for ns in (0, 257):
        assert call(hits, recs, rp, ap, ns, 1.0, 3, 2, 1, C.byref(both)) == ERR_ARG
    for radius in (0.0, -1.0, math.nan, -math.inf):
        assert call(hits, recs, rp, ap, 2, radius, 3, 2, 1, C.byref(both)) == ERR_ARG
    assert (rad == 7.0).all() and (bounce == 7.0).all()
    assert call(hits, recs, rp, ap, 2, 1.0, 3, 2, 1, C.byref(both)) == 0 and not (rad == 7.0).any()


# ---- compositing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength", [0.0, 0.5, 1.0, 0.3, 7.25])
def test_add_scaled_is_the_rule_bit_for_bit(rtc, strength):
    rng = np.random.default_rng(3)
    rgb = rng.uniform(-0.5, 2.0, size=(7, 11, 3))
    plane = rng.uniform(0.0, 1.0, size=(7, 11, 3))
    rgb[0, 0], plane[0, 0] = [0.0, -0.0, 1.0], [0.0, 0.0, 1e-300]
    want = rgb + np.float64(strength) * plane
    got = rtc.add_scaled(rgb, plane, strength)
    assert got.tobytes() == want.tobytes()
    if strength == 0.0:
        assert np.array_equal(got, rgb)
    else:
        assert not np.array_equal(got, rgb)


def test_add_scaled_refuses_bad_parameters(rtc):
    L = rtc.lib()
    rgb, plane = np.ones(12), np.ones(12)
    PD = C.POINTER(C.c_double)
    rp, pp = rgb.ctypes.data_as(PD), plane.ctypes.data_as(PD)
    for strength in (-0.1, -0.0 - 1e-300, math.nan, math.inf, -math.inf):
        assert L.rtc_canvas_add_scaled(rp, pp, strength, 2, 2) == ERR_ARG
    assert L.rtc_canvas_add_scaled(None, pp, 0.5, 2, 2) == ERR_ARG and L.rtc_canvas_add_scaled(rp, None, 0.5, 2, 2) == ERR_ARG
    assert (rgb == 1.0).all()
    assert L.rtc_canvas_add_scaled(rp, pp, 0.5, 2, 2) == 0 and (rgb == 1.5).all()
    with pytest.raises(ValueError):
        rtc.add_scaled(np.ones((2, 2, 3)), np.ones((2, 2)), 1.0)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
GATHER_SYMBOLS = ("rtc_gather_from_hits", "rtc_render_gather_device", "rtc_render_gather", "rtc_canvas_add_scaled", "rtc_canvas_add_scaled_device",
                  "rtc_scene_load_yaml_gather", "rtc_scene_load_yaml_gather_file")


def test_struct_layout_and_symbols(rtc, tmp_path):
    abi = _abi(rtc)
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "rtc.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu", sizeof(rtc_gather_buffers), offsetof(rtc_gather_buffers, radiance),
                           offsetof(rtc_gather_buffers, bounce), sizeof(rtc_ao), sizeof(rtc_aov_buffers), sizeof(rtc_hit)); return 0; }'''
    (tmp_path / "s.c").write_text(src)
    subprocess.run(["gcc", f"-I{ROOT / 'include'}", str(tmp_path / "s.c"), "-o", str(tmp_path / "s")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "s")], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [16, 0, 8, 16, 48, 184]
    B = abi.RtcGatherBuffers
    assert [C.sizeof(B), B.radiance.offset, B.bounce.offset, C.sizeof(abi.RtcAo), C.sizeof(abi.RtcAovBuffers), C.sizeof(abi.RtcHit)] == out
    header = (ROOT / "include" / "rtc.h").read_text()
    declared = set(re.findall(r"\b(rtc_[a-z0-9_]+)\s*\(", header))
    L = rtc.lib()
    for name in GATHER_SYMBOLS:
        assert name in declared and name in abi.PROTOTYPES and getattr(L, name) is not None, name
    for name in ("gather_from_hits", "add_scaled", "load_yaml_gather"):
        assert name in rtc.__all__ and callable(getattr(rtc, name)), name
    assert callable(rtc.DeviceWorld.render_gather) and callable(rtc.DeviceWorld.render_gather_device) and callable(rtc.Context.add_scaled_device)
    # what the pass leaves alone
    assert L.rtc_abi_version() == 3 and C.sizeof(abi.RtcLaunchInfo) == 48 and C.sizeof(abi.RtcShape) == 528 and C.sizeof(abi.RtcMaterial) == 264


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
    w, cam, lens, ao, g = rtc.load_yaml_gather(text=SCENE % "  gather-radius: 0.75\n  gather-usteps: 3\n  gather-vsteps: 5")
    assert len(w) == 2 and (cam.hsize, cam.vsize) == (40, 30) and lens is None and ao is None
    assert (g.radius, g.usteps, g.vsteps) == (0.75, 3, 5)
    *_, g = rtc.load_yaml_gather(text=SCENE % "  gather-radius: 2")
    assert (g.radius, g.usteps, g.vsteps) == (2.0, 4, 4)   # the default grid
    *_, g = rtc.load_yaml_gather(text=SCENE % "  gather-radius: .inf\n  gather-usteps: 16\n  gather-vsteps: 16")
    assert g.radius == math.inf and g.usteps * g.vsteps == 256
    # the two passes are two records: either, both or neither
    *_, ao, g = rtc.load_yaml_gather(text=SCENE % "  ao-radius: 1.5\n  ao-usteps: 2\n  gather-radius: 3\n  gather-vsteps: 8")
    assert (ao.radius, ao.usteps, ao.vsteps) == (1.5, 2, 4) and (g.radius, g.usteps, g.vsteps) == (3.0, 4, 8)
    *_, ao, g = rtc.load_yaml_gather(text=SCENE % "  ao-radius: 1.5")
    assert ao.radius == 1.5 and g is None
    _, _, lens, ao, g = rtc.load_yaml_gather(text=SCENE % "")
    assert lens is None and ao is None and g is None
    _, _, lens, _, g = rtc.load_yaml_gather(text=SCENE % "  aperture: 0.1\n  focal-distance: 7\n  gather-radius: 1")
    assert lens is not None and lens.aperture == 0.1 and g.radius == 1.0
    for bad in ("  gather-usteps: 4", "  gather-radius: 0", "  gather-radius: -1", "  gather-radius: nan", "  gather-radius: 1\n  gather-usteps: 0",
                "  gather-radius: 1\n  gather-usteps: 2.5", "  gather-radius: 1\n  gather-usteps: 17\n  gather-vsteps: 16",
                "  gather-radius: 1\n  gather-vsteps: 257", "  gather-radius: [1, 2]"):
        with pytest.raises(rtc.RtcError) as e:
            rtc.load_yaml_gather(text=SCENE % bad)
        assert e.value.status == 5 and "line" in str(e.value) and "gather-" in str(e.value), bad
    # the keys ask for a pass and change no ray: the other entries load the scene and ignore them
    text = SCENE % "  ao-radius: 0.5\n  gather-radius: 0.75"
    w2, cam2 = rtc.load_yaml(text=text)
    assert len(w2) == 2 and bytes(cam2) == bytes(cam)
    _, cam3, _, ao3 = rtc.load_yaml_ao(text=text)
    assert bytes(cam3) == bytes(cam) and ao3.radius == 0.5


def test_shipped_scene_loads(rtc):
    path = Path(rtc.__file__).resolve().parent / "data" / "colour_bleeding.yml"
    w, cam, lens, ao, g = rtc.load_yaml_gather(path=path)
    assert lens is None and ao is None and (g.radius, g.usteps, g.vsteps) == (math.inf, 4, 4)
    assert sorted(s.kind for s in w.shapes) == sorted([rtc.PLANE, rtc.SPHERE, rtc.CUBE]) and (cam.hsize, cam.vsize) == (320, 200)
    w2, *_, g2 = rtc.load_yaml_gather(text=path.read_text())
    assert len(w2) == 3 and bytes(g2) == bytes(g)
    assert len(rtc.load_yaml_ao(path=path)[0]) == 3   # the AO loader reads it and ignores the gather keys


# ---- the GPU tests' cases, checked with the oracle alone --------------------------------------------------------------------
@pytest.mark.parametrize("name,ao", G.CASES, ids=G.IDS)
def test_cases_exercise_the_pass(rtc, O, name, ao):
    w, cam = G.world(rtc, name)
    s = G.shares(rtc, O, name, ao)
    print(name, ao, f"{cam.hsize}x{cam.vsize}", len(w), "objects;", {k: (round(v, 2) if isinstance(v, float) else v) for k, v in s.items()})
    assert G.conditions(rtc, O, name, ao) == []
    planes = G.expected(rtc, O, name, ao, 1)
    miss = ~G.hit_mask(rtc, O, name)
    for p in ("radiance", "bounce"):
        assert planes[p].dtype == np.float64 and planes[p].shape == (cam.vsize, cam.hsize, 3) and np.isfinite(planes[p]).all()
        assert (planes[p][miss] == 0.0).all() and (planes[p] >= 0.0).all()
    assert planes["bounce"].any() and (planes["bounce"] <= planes["radiance"] + 1e-15).all()   # base * diffuse <= 1 in these worlds
    assert cam.hsize % 8 and cam.vsize % 8   # partial tiles on both edges


def test_cases_cover_what_the_kernel_distinguishes(rtc, O):
    worlds = {n.split(":")[0] for n, _ in G.CASES}
    assert worlds == {"bleed", "bleed+2", "bleed+9", "closeup", "grid290", "inside"}
    assert len(G.world(rtc, "bleed")[0]) == 3 and len(G.world(rtc, "grid290")[0]) == 290   # one-level and two-level cull
    assert [len(G.world(rtc, n)[0].samples()) for n in ("bleed", "bleed+2", "bleed+9")] == [1, 2, 9]   # the three light forms
    assert not G.hit_mask(rtc, O, "bleed").all()   # sky pixels: the miss rule
    hits = G.oracle_hits(rtc, O, "inside")
    assert all(h.inside for h in hits if h.hit_index == 0) and sum(h.hit_index == 0 for h in hits) > 100   # the flipped normal
    recs, _ = G.oracle_samples(rtc, O, "inside", (3.0, 4, 4))
    rec = np.frombuffer(recs, dtype=A.HIT_DTYPE)
    assert ((rec["hit_index"] == 0) & (rec["inside"] != 0)).any()   # ... and on secondary hits of the shell
    assert {(1, 1), (2, 2), (4, 4), (16, 16)} <= {(a[1], a[2]) for _, a in G.CASES}
    radii = {a[0] for _, a in G.CASES}
    assert 0.25 in radii and math.inf in radii
    # patterns on primary hits (base) and on secondary hits (lighting's own base)
    for name in ("bleed", "inside"):
        w, _ = G.world(rtc, name)
        assert any(s.material.pattern_kind != 0 for s in w.shapes)
    for name, ao in G.SERIAL_CASES:   # RTC_MODE_RENDER: the last row and column hold zeros and would not otherwise
        serial, free = G.expected(rtc, O, name, ao, 0), G.expected(rtc, O, name, ao, 1)
        for p in ("radiance", "bounce"):
            assert not serial[p][-1].any() and not serial[p][:, -1].any() and (free[p][-1].any() or free[p][:, -1].any())
            assert np.array_equal(serial[p][:-1, :-1], free[p][:-1, :-1])
