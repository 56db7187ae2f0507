"""The thin-lens camera on the host side: rtc_lens_ray against a restatement of the normative arithmetic (include/rtc.h)
built from the oracle's orc_transform_point and plain Python floats, the pinhole case, rtc_lens_validate's argument errors,
the YAML loader's lens keys (data/depth_of_field.yml, defaults, the old entries' parse error), and the new symbols in the
library and in abi.py. No GPU."""
import ctypes as C
import importlib
import math
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
DATA = ROOT / "raytracer-challenge_amd" / "data"
ERR_ARG, ERR_PARSE = 4, 5
NEW_SYMBOLS = ("rtc_lens_validate", "rtc_lens_ray", "rtc_render_lens_rows", "rtc_render_lens", "rtc_render_lens_rgb8",
               "rtc_scene_load_yaml_lens", "rtc_scene_load_yaml_lens_file")


@pytest.fixture(scope="module")
def A(rtc):
    return importlib.import_module(rtc.__name__ + ".abi")


def _cameras(rtc):
    M = rtc.Matrix
    return {
        "identity": rtc.camera(70, 45, 0.9),
        "looking down a diagonal": rtc.camera(70, 45, 0.7, M.make_view_transform((0.5, 2.5, -7.0), (0.0, 1.0, 1.0), (0.0, 1.0, 0.0))),
        "rotated and translated": rtc.camera(33, 61, 1.3, M.identity().rotation_y(0.7).rotation_x(-0.3).translation(1.5, -2.25, 4.0)),
    }


LENSES = {"1x1": (0.3, 4.5, 1, 1), "2x2": (0.25, 6.0, 2, 2), "3x2": (0.7, 3.25, 3, 2)}


def _restated(O, cam, lens, x, y, k):
    """include/rtc.h's ray in Python floats (IEEE f64, one rounding per operation, nothing fused); transform_point is the
    oracle's (transform.rs:122-128)."""
    def transform_point(p):
        m16 = (C.c_double * 16)(*cam.view_inv)
        out = (C.c_double * 3)()
        O.lib().orc_transform_point(m16, (C.c_double * 3)(*p), out)
        return tuple(out)
    u, v = k % lens.usteps, k // lens.usteps   # v outer, u inner
    xoffset = (float(x) + 0.5) * cam.pixel_size
    yoffset = (float(y) + 0.5) * cam.pixel_size
    world_x = cam.half_width - xoffset
    world_y = cam.half_height - yoffset
    ucell = (2.0 * lens.aperture) / float(lens.usteps)
    vcell = (2.0 * lens.aperture) / float(lens.vsteps)
    lu = -lens.aperture + ucell * (float(u) + 0.5)
    lv = -lens.aperture + vcell * (float(v) + 0.5)
    origin = transform_point((lu, lv, 0.0))
    target = transform_point((world_x * lens.focal_distance, world_y * lens.focal_distance, -lens.focal_distance))
    d = tuple(t - o for t, o in zip(target, origin))
    mag = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])   # Vector::normalize vec.rs:65-76: sqrt of the sum, three divisions
    return origin + (d[0] / mag, d[1] / mag, d[2] / mag)


def _bits(values):
    return bytes((C.c_double * len(values))(*values))


@pytest.mark.parametrize("lens_name", list(LENSES))
@pytest.mark.parametrize("cam_name", ["identity", "looking down a diagonal", "rotated and translated"])
def test_lens_ray_is_the_stated_arithmetic_bit_for_bit(rtc, O, cam_name, lens_name):
    cam = _cameras(rtc)[cam_name]
    lens = rtc.lens(*LENSES[lens_name])
    n = lens.usteps * lens.vsteps
    pixels = [(0, 0), (cam.hsize - 1, cam.vsize - 1), (cam.hsize // 2, cam.vsize // 3), (7, cam.vsize - 2), (cam.hsize - 3, 1)]
    seen = set()
    for x, y in pixels:
        for k in range(n):
            got = rtc.lens_ray(cam, lens, x, y, k)
            want = _restated(O, cam, lens, x, y, k)
            assert _bits(list(got)) == _bits(list(want)), (cam_name, lens_name, x, y, k, list(got), want)
            assert abs(math.sqrt(sum(c * c for c in got[3:])) - 1.0) < 1e-15
            seen.add(tuple(got[:3]))
    assert len(seen) == n   # one origin per lens sample, the same for every pixel


def test_the_sample_order_is_v_outer_u_inner(rtc):
    """Identity view: the origin of sample k IS (lu, lv, 0)."""
    cam = rtc.camera(16, 16, 1.0)
    lens = rtc.lens(0.6, 2.0, 3, 2)
    got = [tuple(rtc.lens_ray(cam, lens, 5, 9, k)[:3]) for k in range(6)]
    us = [-0.6 + (1.2 / 3.0) * (u + 0.5) for u in range(3)]
    vs = [-0.6 + (1.2 / 2.0) * (v + 0.5) for v in range(2)]
    assert got == [(us[k % 3], vs[k // 3], 0.0) for k in range(6)]
    # every ray of a pixel passes through the same point of the plane in focus
    rays = [rtc.lens_ray(cam, lens, 5, 9, k) for k in range(6)]
    hits = [tuple(r[i] + r[3 + i] * ((-2.0 - r[2]) / r[5]) for i in range(3)) for r in rays]
    assert all(max(abs(a - b) for a, b in zip(h, hits[0])) < 1e-14 for h in hits)


@pytest.mark.parametrize("cam_name", ["identity", "looking down a diagonal", "rotated and translated"])
def test_the_degenerate_lens_is_the_pinhole_ray(rtc, cam_name):
    cam = _cameras(rtc)[cam_name]
    lens = rtc.lens(0.0, 1.0)
    for x, y in [(0, 0), (cam.hsize - 1, cam.vsize - 1), (cam.hsize // 2, cam.vsize // 3), (7, cam.vsize - 2), (3, 11)]:
        assert _bits(list(rtc.lens_ray(cam, lens, x, y, 0))) == _bits(list(rtc.ray_for_pixel(cam, x, y, 0.5, 0.5))), (cam_name, x, y)


def test_validate_and_lens_ray_argument_errors(rtc, A):
    L = rtc.lib()

    def lens(aperture, focal, us, vs):
        l = A.RtcLens()
        l.aperture, l.focal_distance, l.usteps, l.vsteps = aperture, focal, us, vs
        return l
    assert L.rtc_lens_validate(None) == ERR_ARG
    bad = {"negative aperture": (-0.1, 1.0, 1, 1), "nan aperture": (math.nan, 1.0, 1, 1), "infinite aperture": (math.inf, 1.0, 1, 1),
           "zero focal distance": (0.1, 0.0, 1, 1), "negative focal distance": (0.1, -2.0, 1, 1), "nan focal distance": (0.1, math.nan, 1, 1),
           "infinite focal distance": (0.1, math.inf, 1, 1), "zero usteps": (0.1, 1.0, 0, 2), "zero vsteps": (0.1, 1.0, 2, 0),
           "257 samples": (0.1, 1.0, 257, 1), "17x16": (0.1, 1.0, 17, 16), "a product that wraps 32 bits": (0.1, 1.0, 65536, 65536)}
    for name, spec in bad.items():
        assert L.rtc_lens_validate(C.byref(lens(*spec))) == ERR_ARG, name
        with pytest.raises(rtc.RtcError):
            rtc.lens(*spec)
    for spec in ((0.0, 1.0, 1, 1), (0.0, 1e-300, 1, 1), (2.5, 1e6, 16, 16), (0.1, 3.0, 256, 1), (0.1, 3.0, 1, 256)):
        assert L.rtc_lens_validate(C.byref(lens(*spec))) == 0, spec
    cam, ray = rtc.camera(8, 8, 1.0), (C.c_double * 6)()
    ok = lens(0.1, 3.0, 3, 2)
    assert L.rtc_lens_ray(C.byref(cam), C.byref(ok), 0, 0, 5, ray) == 0
    assert L.rtc_lens_ray(C.byref(cam), C.byref(ok), 0, 0, 6, ray) == ERR_ARG          # k out of range
    assert L.rtc_lens_ray(None, C.byref(ok), 0, 0, 0, ray) == ERR_ARG
    assert L.rtc_lens_ray(C.byref(cam), None, 0, 0, 0, ray) == ERR_ARG
    raw = C.CDLL(str(rtc.LIB_PATH)).rtc_lens_ray   # no argtypes: a NULL where the binding wants an array
    assert raw(C.byref(cam), C.byref(ok), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), None) == ERR_ARG
    assert L.rtc_lens_ray(C.byref(cam), C.byref(lens(0.1, 0.0, 1, 1)), 0, 0, 0, ray) == ERR_ARG


YAML = """
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
- add: sphere
"""


def _yaml_error(rtc, text):
    with pytest.raises(rtc.RtcError) as e:
        rtc.load_yaml_lens(text=text)
    assert e.value.status == ERR_PARSE
    return str(e.value)


def test_yaml_lens_keys(rtc, A):
    w, cam, lens = rtc.load_yaml_lens(path=DATA / "depth_of_field.yml")
    assert (lens.aperture, lens.focal_distance, lens.usteps, lens.vsteps) == (0.12, 7.0, 4, 4)
    assert (cam.hsize, cam.vsize, cam.samples) == (320, 200, 1) and len(w) == 4 and len(w.lights) == 1
    kinds = [s.kind for s in w.shapes]
    assert kinds == [rtc.PLANE, rtc.SPHERE, rtc.SPHERE, rtc.SPHERE]
    # three spheres at three depths; the middle one lies on the plane in focus
    origin = rtc.lens_ray(cam, rtc.lens(0.0, 1.0), 0, 0, 0)[:3]
    centres = [rtc.Matrix(s.inv).inverse().numpy()[:3, 3] for s in w.shapes[1:]]
    depths = [math.dist(origin, c) for c in centres]
    assert depths[0] < depths[1] - 2.0 and depths[1] < depths[2] - 2.0 and abs(depths[1] - lens.focal_distance) < 0.1
    # steps default to 1
    _, _, l2 = rtc.load_yaml_lens(text=YAML % "  aperture: 0.2\n  focal-distance: 5.5")
    assert (l2.aperture, l2.focal_distance, l2.usteps, l2.vsteps) == (0.2, 5.5, 1, 1)
    _, _, l3 = rtc.load_yaml_lens(text=YAML % "  aperture: 0.2\n  focal-distance: 5.5\n  lens-vsteps: 3")
    assert (l3.usteps, l3.vsteps) == (1, 3)
    # a camera without lens keys: no lens, and the C entry hands out the pinhole
    w0, cam0, none = rtc.load_yaml_lens(text=YAML % "")
    assert none is None and len(w0) == 1
    L = rtc.lib()
    shapes, ns, lg, nl, c = C.POINTER(A.RtcShape)(), C.c_uint32(), (A.RtcAreaLight * 4)(), C.c_uint32(), A.RtcCamera()
    err, ln, has = C.create_string_buffer(256), A.RtcLens(), C.c_uint32(7)
    assert L.rtc_scene_load_yaml_lens((YAML % "").encode(), C.byref(shapes), C.byref(ns), lg, 4, C.byref(nl), C.byref(c), err, 256, C.byref(ln), C.byref(has)) == 0
    L.rtc_free(shapes)
    assert has.value == 0 and (ln.aperture, ln.focal_distance, ln.usteps, ln.vsteps) == (0.0, 1.0, 1, 1)
    assert L.rtc_scene_load_yaml_lens((YAML % "").encode(), C.byref(shapes), C.byref(ns), lg, 4, C.byref(nl), C.byref(c), err, 256, None, C.byref(has)) == ERR_ARG
    # the scene without lens keys loads through the old entries exactly as before
    w1, cam1 = rtc.load_yaml(text=YAML % "")
    assert bytes(cam1) == bytes(cam0) and bytes(w1.shapes[0]) == bytes(w0.shapes[0])


def test_yaml_lens_errors(rtc):
    assert "focal-distance" in _yaml_error(rtc, YAML % "  aperture: 0.2")
    assert "aperture" in _yaml_error(rtc, YAML % "  aperture: -0.2\n  focal-distance: 5")
    assert "focal-distance" in _yaml_error(rtc, YAML % "  aperture: 0.2\n  focal-distance: 0")
    assert "lens-usteps" in _yaml_error(rtc, YAML % "  aperture: 0.2\n  focal-distance: 5\n  lens-usteps: 0")
    assert "lens-usteps" in _yaml_error(rtc, YAML % "  aperture: 0.2\n  focal-distance: 5\n  lens-usteps: 2.5")
    assert "lens-vsteps" in _yaml_error(rtc, YAML % "  aperture: 0.2\n  focal-distance: 5\n  lens-vsteps: nan")
    assert "256" in _yaml_error(rtc, YAML % "  aperture: 0.2\n  focal-distance: 5\n  lens-usteps: 17\n  lens-vsteps: 16")


def test_the_old_yaml_entries_refuse_a_lens_and_name_the_new_one(rtc, A):
    L = rtc.lib()
    text = (DATA / "depth_of_field.yml").read_bytes()
    shapes, ns, c, err = C.POINTER(A.RtcShape)(), C.c_uint32(), A.RtcCamera(), C.create_string_buffer(256)
    lgt, lgts, areas, nl = A.RtcLight(), (A.RtcLight * 8)(), (A.RtcAreaLight * 8)(), C.c_uint32()
    calls = {
        "rtc_scene_load_yaml": lambda: L.rtc_scene_load_yaml(text, C.byref(shapes), C.byref(ns), C.byref(lgt), C.byref(c), err, 256),
        "rtc_scene_load_yaml_lights": lambda: L.rtc_scene_load_yaml_lights(text, C.byref(shapes), C.byref(ns), lgts, 8, C.byref(nl), C.byref(c), err, 256),
        "rtc_scene_load_yaml_area_lights": lambda: L.rtc_scene_load_yaml_area_lights(text, C.byref(shapes), C.byref(ns), areas, 8, C.byref(nl), C.byref(c), err, 256),
        "rtc_scene_load_yaml_file": lambda: L.rtc_scene_load_yaml_file(str(DATA / "depth_of_field.yml").encode(), C.byref(shapes), C.byref(ns), C.byref(lgt),
                                                                        C.byref(c), err, 256),
    }
    for name, call in calls.items():
        err.value = b""
        assert call() == ERR_PARSE and b"rtc_scene_load_yaml_lens" in err.value, name
        assert not shapes, name
    with pytest.raises(rtc.RtcError, match="rtc_scene_load_yaml_lens"):
        rtc.load_yaml(path=DATA / "depth_of_field.yml")


def test_new_symbols_are_exported_and_declared(rtc, A):
    header = (ROOT / "include" / "rtc.h").read_text()
    declared = set(re.findall(r"\b(rtc_[a-z0-9_]+)\s*\(", header))
    L = rtc.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in A.PROTOTYPES and getattr(L, name) is not None, name
    assert A.MAX_LENS_SAMPLES == 256 and "RTC_MAX_LENS_SAMPLES 256u" in header and "RTC_ABI_VERSION 3" in re.sub(r"\s+", " ", header)
    assert C.sizeof(A.RtcLens) == 24 and A.RtcLens.usteps.offset == 16
    # the launch info keeps its size: lens_samples is the word that was _reserved[1]
    assert C.sizeof(A.RtcLaunchInfo) == 48 and A.RtcLaunchInfo.lens_samples.offset == 44 and "uint32_t lens_samples;" in header
    for phrase in ("NO JITTER, NO DISC", "v outer, u"):
        assert phrase in header, phrase
