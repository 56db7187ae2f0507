"""The float file writers on the MI355X (rtc_float_encoder_*, rtc_lua_program_render_saved, the facade): device bytes equal
the host statement (rtc_float_format) for every case of float_cases.py — rows at the wave and token-chunk edges, the flat
and the run-length form of Radiance HDR, a 1920x3 strip whose 16-byte pack threads straddle rows and the header, EXR with
every channel — rendered frames with and without a lens, a multi-channel EXR of the AOV kernel's planes, one encoder across
growing and shrinking frames, a Lua script's float files, and the C++ facade's Canvas::save and Aov::save_exr."""
import importlib
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

import float_cases as F

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CASES = F.cases()


@pytest.fixture(scope="module")
def scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


@pytest.fixture(scope="module")
def enc(rtc, gpu):
    e = rtc.FloatEncoder(gpu)
    yield e
    e.close()


def device_file(enc, fmt, canvas, planes, rgb_type):
    import torch
    def up(a):   # as bytes: torch has no arithmetic on uint16, and none is needed
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")
    t = None if canvas is None else up(canvas)
    d = {k: up(v) for k, v in (planes or {}).items()}
    torch.cuda.synchronize()
    shape = (canvas if canvas is not None else next(iter(planes.values()))).shape
    return enc.encode_device(fmt, None if t is None else t.data_ptr(), shape[1], shape[0], {k: v.data_ptr() for k, v in d.items()}, rgb_type)


def assert_same(got, want, what):
    if got != want:
        k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{what}: device file differs from the host's ({len(got)} vs {len(want)} bytes, first difference at {k})")


@pytest.fixture(scope="module")
def two_lights(rtc, gpu, scenes):
    """A two-light World at 61x37: components above 1.0."""
    w, cam = scenes.default_scene(61, 37)
    w.add_light(rtc.light((6.0, 8.0, -4.0), (0.9, 0.7, 1.2)))
    dw = gpu.upload(w)
    yield dw, cam, len(w.samples())
    dw.close()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_bytes_equal_host_bytes(rtc, enc, case):
    name, fmt, canvas, planes, rgb_type = case
    assert_same(device_file(enc, fmt, canvas, planes, rgb_type), rtc.float_encode(fmt, canvas, planes, rgb_type), name)


def test_render_equals_float_encode_of_the_rendered_canvas(rtc, enc, two_lights):
    dw, cam, _ = two_lights
    canvas = dw.render(cam)
    assert canvas.max() > 1.0     # what the 8-bit writers clip
    for fmt, rgb_type in (("hdr", "half"), ("pfm", "half"), ("exr", "half"), ("exr", "float")):
        assert_same(enc.render(fmt, dw, cam, rgb_type=rgb_type), rtc.float_encode(fmt, canvas, None, rgb_type), f"render {fmt} {rgb_type}")
    F.check_file("hdr", enc.render("hdr", dw, cam), canvas, None, "half")
    plain = dw.render(cam, rtc.MODE_RENDER)    # the mode whose last row and column stay black
    assert_same(enc.render("pfm", dw, cam, mode=rtc.MODE_RENDER), rtc.float_encode("pfm", plain), "render pfm, MODE_RENDER")


def test_render_through_a_lens(rtc, enc, two_lights):
    dw, cam, _ = two_lights
    lens = rtc.lens(0.08, 5.0, 3, 2)
    canvas = dw.render_lens(cam, lens)
    assert not np.array_equal(canvas, dw.render(cam))
    for fmt, rgb_type in (("hdr", "half"), ("pfm", "half"), ("exr", "float")):
        assert_same(enc.render(fmt, dw, cam, lens=lens, rgb_type=rgb_type), rtc.float_encode(fmt, canvas, None, rgb_type), f"lens {fmt}")


def test_multi_channel_exr_of_the_aov_planes(rtc, gpu, enc, two_lights):
    import torch
    dw, cam, n_lights = two_lights
    host = dw.render_aov(cam)
    canvas = dw.render(cam)
    want = rtc.float_encode("exr", canvas, host, "half")
    h, w = cam.vsize, cam.hsize
    d = {name: torch.zeros(h * w * a.itemsize * (a.shape[2] if a.ndim == 3 else 1), dtype=torch.uint8, device="cuda:0") for name, a in host.items()}
    rgb = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dw.render_rows(cam, 0, h, rgb.data_ptr())
    gpu.fence()
    dw.render_aov_device(cam, {k: v.data_ptr() for k, v in d.items()})
    got = enc.encode_device("exr", rgb.data_ptr(), w, h, {k: v.data_ptr() for k, v in d.items()}, "half")
    assert_same(got, want, "colour + all planes")
    chans, _ = F.decode_exr(got)
    assert tuple(chans) == F.EXR_CHANNELS
    assert np.array_equal(chans["id"], (host["index"] + 1).astype(np.uint32)) and np.array_equal(chans["Z"], F.f32_bits(host["depth"]))
    assert chans["shadow"].max() <= n_lights and (chans["id"] == 0).any() and np.isinf(host["depth"]).any()


def test_one_encoder_larger_smaller_larger(rtc, gpu):
    e = rtc.FloatEncoder(gpu)
    assert e.bytes() == b""
    frames = [F.noise_canvas(h, w, 50 + k) for k, (h, w) in enumerate(((9, 33), (70, 300), (5, 12), (90, 640), (2, 8), (1, 7)))]
    for k, c in enumerate(frames + frames[::-1]):
        for fmt in ("hdr", "pfm", "exr"):
            assert_same(device_file(e, fmt, c, None, "half"), rtc.float_encode(fmt, c), f"frame {k} {fmt}")
            assert e.bytes() == rtc.float_encode(fmt, c)
    e.close()


def test_errors_launch_nothing(rtc, gpu, enc, two_lights):
    import torch
    dw, cam, _ = two_lights
    t = torch.zeros((4, 4, 3), dtype=torch.float64, device="cuda:0")
    z = torch.zeros((4, 4), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    good = enc.encode_device("pfm", t.data_ptr(), 4, 4)
    gpu.reset_stats()
    before = gpu.stats()
    for args in (("hdr", None, 4, 4), ("pfm", None, 4, 4, {"depth": z.data_ptr()}), ("exr", None, 4, 4), (3, t.data_ptr(), 4, 4),
                 ("exr", t.data_ptr(), 4, 4, None, 0), ("hdr", t.data_ptr(), 0, 4), ("pfm", t.data_ptr(), 4, 65536)):
        with pytest.raises(rtc.RtcError) as e:
            enc.encode_device(*args)
        assert e.value.status == 4, args
    for fmt, rgb_type in ((3, "half"), ("exr", 0), ("exr", 3)):
        with pytest.raises(rtc.RtcError) as e:
            enc.render(fmt, dw, cam, rgb_type=rgb_type)
        assert e.value.status == 4
    assert gpu.stats() == before and before["pixels"] == 0      # no render was launched
    assert enc.bytes() == good                  # and the last file is still the last good one


LUA = """
local function scene(w, h, x)
  local world = { lights = { { color = { r = 1.7, g = 1.5, b = 1.2 }, position = { x = -10, y = 10, z = -10 } } },
                  shapes = { { type = "sphere", position = { x = x, y = 1, z = 0 }, color = { r = 1, g = 0.2, b = 0.1 } },
                             { type = "plane", pattern = { type = "checks", color_a = { r = 1, g = 1, b = 1 },
                                                           color_b = { r = 0.1, g = 0.1, b = 0.1 } } } } }
  local camera = { screenwidth = w, screenheight = h, fov = 1.0, position = { x = 0, y = 1.5, z = -5 },
                   lookat = { x = 0, y = 1, z = 0 }, up = { x = 0, y = 1, z = 0 } }
  return world, camera
end
local names = { "a.hdr", "b.exr", "c.png", "d.PFM", "e.hdr" }
for k, name in ipairs(names) do
  local w, c = scene(60 + 5 * k, 7 + 10 * k, k * 0.1)
  Render(w, c, NAMEDIR .. name)
end
local enc = StartAnimation("loop.gif")
for i = 1, 2 do
  local w, c = scene(64, 48, i * 0.2)
  enc:AddFrame(w, c)
end
enc:Finish()
"""


def test_lua_render_saved_float_files(rtc, gpu, tmp_path):
    prog = rtc.LuaProgram(text='NAMEDIR = "some/dir/"\n' + LUA)
    jobs = prog.jobs
    frames = prog.render(gpu)     # the 8-bit rows of every job
    paths = prog.render_saved_files(gpu, tmp_path / "out")
    assert [p.name for p in paths] == ["a.hdr", "b.exr", "c.png", "d.PFM", "e.hdr", "loop.gif"]
    for i, (name, fmt) in enumerate((("a.hdr", "hdr"), ("b.exr", "exr"), ("c.png", None), ("d.PFM", "pfm"), ("e.hdr", "hdr"))):
        j = jobs[i]
        got = (tmp_path / "out" / name).read_bytes()
        if fmt is None:
            assert got == rtc.image_encode("png", frames[i])      # every other name exactly as before
            continue
        dw = gpu.upload(j.world)
        canvas = dw.render(j.camera)
        dw.close()
        assert canvas.max() > 1.0 and np.array_equal(rtc.color_scale255(canvas).reshape(frames[i].shape), frames[i])
        assert_same(got, rtc.float_encode(fmt, canvas, None, "half"), name)
    anim = {Path(p).name: Path(p) for p in prog.render_animations(gpu, tmp_path / "anim")}
    assert (tmp_path / "out" / "loop.gif").read_bytes() == anim["loop.gif"].read_bytes()      # AddFrame jobs as before
    # a name in neither table stops the run before anything is rendered or written
    bad = rtc.LuaProgram(text='NAMEDIR = ""\n' + LUA.replace('"e.hdr"', '"e.rgbe"'))
    gpu.reset_stats()
    with pytest.raises(rtc.RtcError) as e:
        bad.render_saved_files(gpu, tmp_path / "bad")
    assert e.value.status == 8 and not (tmp_path / "bad").exists() and gpu.stats()["pixels"] == 0


def _build():
    spec = importlib.util.spec_from_file_location("_rtc_build", ROOT / "raytracer-challenge_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_cpp_facade_saves_float_files(rtc, tmp_path):
    """tests/cpp/test_facade_float.cpp (prebuilt by build()): Canvas::save and Aov::save_exr against the Python bytes."""
    exe = _build().build_facade_float_test()
    assert exe is not None and exe.exists()
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "facade float: ok" in r.stdout, r.stdout + r.stderr
    h, w = 37, 61
    canvas = np.fromfile(tmp_path / "f64.bin", dtype=np.float64).reshape(h, w, 3)
    assert canvas.max() > 1.0
    for name, fmt in (("a.hdr", "hdr"), ("b.PFM", "pfm"), ("c.exr", "exr")):
        assert_same((tmp_path / name).read_bytes(), rtc.float_encode(fmt, canvas, None, "half"), name)
    assert (tmp_path / "still.png").read_bytes() == rtc.image_encode("png", rtc.to_rgba8(canvas, 1.0))
    planes = {"index": np.fromfile(tmp_path / "index.bin", dtype=np.int32).reshape(h, w),
              "depth": np.fromfile(tmp_path / "depth.bin", dtype=np.float64).reshape(h, w),
              "point": np.fromfile(tmp_path / "point.bin", dtype=np.float64).reshape(h, w, 3),
              "normal": np.fromfile(tmp_path / "normal.bin", dtype=np.float64).reshape(h, w, 3),
              "flags": np.fromfile(tmp_path / "flags.bin", dtype=np.uint8).reshape(h, w),
              "shadow": np.fromfile(tmp_path / "shadow.bin", dtype=np.uint16).reshape(h, w)}
    assert (planes["index"] >= 0).any() and (planes["index"] < 0).any()
    assert_same((tmp_path / "aov_colour.exr").read_bytes(), rtc.float_encode("exr", canvas, planes, "half"), "aov_colour.exr")
    assert_same((tmp_path / "aov_colour_float.exr").read_bytes(), rtc.float_encode("exr", canvas, planes, "float"), "aov_colour_float.exr")
    assert_same((tmp_path / "aov_planes.exr").read_bytes(), rtc.float_encode("exr", None, planes), "aov_planes.exr")
    F.check_file("exr", (tmp_path / "aov_colour.exr").read_bytes(), canvas, planes, "half")
    lens = np.fromfile(tmp_path / "lens.bin", dtype=np.float64).reshape(h, w, 3)
    assert_same((tmp_path / "lens.hdr").read_bytes(), rtc.float_encode("hdr", lens), "lens.hdr")
