"""The compressed PNG writer on the MI355X (rtc_png_encoder_*, rtc_lua_program_render_png): device bytes equal the host
statement (rtc_png_format) byte for byte for rendered frames, noise, an all-zero frame, edge sizes, segment-boundary
lengths and a 4096^2 frame, in 3 and 4 channels; encoder reuse; render-and-encode at any gamma; the Lua loop's PNG files;
the stored writer's files unchanged."""
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_host_png import chunks, decode, mixed, noise, sized_for, SEG  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


def device_png(enc, pixels):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(pixels)).to("cuda:0")
    torch.cuda.synchronize()
    return enc.encode_device(t.data_ptr(), pixels.shape[1], pixels.shape[0], pixels.shape[2])


def assert_same(rtc, enc, pixels, what):
    want = rtc.png_encode(pixels)
    got = device_png(enc, pixels)
    if got != want:
        k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{what}: device PNG differs from the host's ({len(got)} vs {len(want)} bytes, first difference at {k})")
    return want


def test_rendered_frames_device_equals_host(rtc, gpu, scenes):
    cases = {"north_star": scenes.synthetic(100, 1920, 1080), "mixed": scenes.mixed(), "criterion": scenes.criterion(1920, 1080),
             "reflect_refract": rtc.load_yaml(path=os.path.join(os.path.dirname(rtc.__file__), "data", "reflect_refract.yml"))}
    enc = rtc.PngEncoder(gpu)
    for name, (w, cam) in cases.items():
        dw = gpu.upload(w)
        f = dw.render_rgb8(cam)
        rgba = dw.render_rgba8(cam, 2.2)
        dw.close()
        b = assert_same(rtc, enc, f, name)
        assert len(b) < len(rtc.format_png(f)), name
        if name == "north_star":   # PNG is lossless: the file decodes to the frame
            try:
                import io
                from PIL import Image
                assert np.array_equal(np.asarray(Image.open(io.BytesIO(b))), f)
            except ImportError:
                import zlib
                assert len(zlib.decompress(b"".join(d for t, d in chunks(b) if t == b"IDAT"))) == 1080 * (1 + 1920 * 3)
        assert_same(rtc, enc, rgba, name + " rgba")
    enc.close()


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (1, 3), (1, 17), (1, 1921), (7, 3), (33, 17), (1, 65535), (97, 101)])
@pytest.mark.parametrize("c", [3, 4])
def test_noise_zero_and_edge_sizes_device_equals_host(rtc, gpu, shape, c):
    enc = rtc.PngEncoder(gpu)
    assert_same(rtc, enc, noise(*shape, c, seed=shape[0] * 131 + shape[1]), f"noise {shape}x{c}")
    assert_same(rtc, enc, np.zeros(shape + (c,), np.uint8), f"zero {shape}x{c}")
    enc.close()


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_segment_boundaries_device_equals_host(rtc, gpu, k, delta):
    px = sized_for(k * SEG + delta)
    enc = rtc.PngEncoder(gpu)
    assert_same(rtc, enc, px, f"{k}*SEG{delta:+d}")
    enc.close()


def test_large_frames_device_equals_host(rtc, gpu):
    """Full-HD noise (every segment stored), an all-zero 1080p frame (longest matches) and a 4096^2 frame."""
    enc = rtc.PngEncoder(gpu)
    assert_same(rtc, enc, noise(1080, 1920, 3, seed=3), "noise 1080p")
    z = assert_same(rtc, enc, np.zeros((1080, 1920, 3), np.uint8), "zero 1080p")
    assert len(z) < 60000
    c = np.arange(1 << 24, dtype=np.uint32)
    f = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    assert_same(rtc, enc, f, "4096^2 all colours")
    assert_same(rtc, enc, np.ascontiguousarray(np.concatenate([f[:2048], np.full((2048, 4096, 3), 9, np.uint8)])), "4096^2 half flat")
    enc.close()


def test_growing_and_shrinking_sizes_and_pipelined_launches(rtc, scenes):
    import torch
    ctx = rtc.Context(0)
    try:
        enc = rtc.PngEncoder(ctx)
        frames = [mixed(1080, 1920, 3), mixed(30, 50, 4), mixed(1080, 1920, 3), noise(5, 3, 3)]
        for f in frames:
            assert device_png(enc, f) == rtc.png_encode(f), f.shape
        w, cam = scenes.synthetic(20, 200, 120)
        dw = ctx.upload(w)
        want = rtc.png_encode(dw.render_rgb8(cam))
        ctx.set_pipeline(3)
        ring = [torch.zeros((120, 200, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        f64 = torch.zeros((120, 200, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        for t in ring:
            dw.render_rows(cam, 0, 120, f64.data_ptr(), d_ptr8=t.data_ptr())
        ctx.fence()
        for t in ring:
            assert enc.encode_device(t.data_ptr(), 200, 120, 3) == want
        ctx.set_pipeline(1)
        dw.close()
        enc.close()
    finally:
        ctx.close()


def test_render_at_gamma_equals_host_encode(rtc, gpu, scenes, tmp_path):
    w, cam = scenes.synthetic(20, 320, 180)
    dw = gpu.upload(w)
    enc = rtc.PngEncoder(gpu)
    assert enc.bytes() == b""
    got = enc.render(dw, cam, 1.0)
    assert got == rtc.png_encode(dw.render_rgb8(cam))
    for g in (2.2, 0.5):
        assert enc.render(dw, cam, g) == rtc.png_encode(dw.render_rgba8(cam, g)), g
    enc.write(tmp_path / "a.png")
    assert (tmp_path / "a.png").read_bytes() == enc.bytes()
    with pytest.raises(rtc.RtcError):
        enc.render(dw, cam, 0.0)
    enc.close()
    dw.close()


LUA = """
local function scene(w, h, x)
  local world = { lights = { { color = { r = 1, g = 1, b = 1 }, position = { x = -10, y = 10, z = -10 } } },
                  shapes = { { type = "sphere", position = { x = x, y = 1, z = 0 }, color = { r = 1, g = 0.2, b = 0.1 } },
                             { type = "plane", pattern = { type = "checks", color_a = { r = 1, g = 1, b = 1 },
                                                           color_b = { r = 0.1, g = 0.1, b = 0.1 } } } } }
  local camera = { screenwidth = w, screenheight = h, fov = 1.0, position = { x = 0, y = 1.5, z = -5 },
                   lookat = { x = 0, y = 1, z = 0 }, up = { x = 0, y = 1, z = 0 } }
  return world, camera
end
local w, c = scene(96, 64, 0)
Render(w, c, "first.jpg")
w, c = scene(40, 30, -0.5)
Render(w, c, "third.png")
Render(w, c, "fourth.PPM")
local enc = StartAnimation("loop.gif")
for i = 1, 3 do
  w, c = scene(64, 48, i * 0.2)
  enc:AddFrame(w, c)
end
enc:Finish()
w, c = scene(33, 17, 1)
Render(w, c, "/some/dir/last")
"""


def check_png_files(rtc, prog, ctx, tmp_path):
    frames = prog.render(ctx)
    paths = prog.render_png_files(ctx, tmp_path / "gpu")
    stored = prog.render_to_files(ctx, tmp_path / "host")
    assert [p.name for p in paths] == [p.name for p in stored]
    for i, (p, q) in enumerate(zip(paths, stored)):
        if p.suffix.lower() == ".ppm":
            assert p.read_bytes() == q.read_bytes(), p.name
            continue
        b = p.read_bytes()
        assert b == rtc.png_encode(frames[i]), p.name
        got, _, _ = decode(b)
        assert np.array_equal(got, frames[i]), p.name
        assert q.read_bytes() == rtc.format_png(frames[i]), q.name   # render_to_files still writes the stored files
    return paths


def test_lua_png_files_mixed(rtc, tmp_path):
    prog = rtc.LuaProgram(text=LUA)
    ctx = rtc.Context(0)
    try:
        paths = check_png_files(rtc, prog, ctx, tmp_path)
        assert sorted(p.name for p in paths) == sorted(["first.jpg.png", "third.png", "fourth.PPM", "loop.gif.0000.png",
                                                        "loop.gif.0001.png", "loop.gif.0002.png", "last.png"])
        paths, stats = prog.render_png_files(ctx, tmp_path / "again", with_stats=True)
        assert len(paths) == 7 and isinstance(stats, dict)
    finally:
        ctx.close()


def test_lua_png_files_orbit(rtc, tmp_path):
    data = Path(rtc.__file__).resolve().parent / "data"
    text = "FRAMES = 5 BALLS = 9 WIDTH, HEIGHT = 200, 136\n" + (data / "orbit_animation.lua").read_text()
    prog = rtc.LuaProgram(text=text, base_dir=data)
    ctx = rtc.Context(0)
    try:
        paths = check_png_files(rtc, prog, ctx, tmp_path)
        assert sum(1 for p in paths if ".gif." in p.name) == 5
    finally:
        ctx.close()


def test_other_lua_paths_unchanged(rtc, tmp_path):
    """render_reference_files without the new entry still writes the stored PNGs of render_to_files."""
    prog = rtc.LuaProgram(text=LUA)
    ctx = rtc.Context(0)
    try:
        frames = prog.render(ctx)
        ref = prog.render_reference_files(ctx, tmp_path / "out")
        third = tmp_path / "out" / "third.png"
        assert third in ref and third.read_bytes() == rtc.format_png(frames[1])
        assert (tmp_path / "out" / "last.png").read_bytes() == rtc.format_png(frames[-1])
    finally:
        ctx.close()
