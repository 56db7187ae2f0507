"""The JPEG writer on the MI355X (rtc_jpeg_encoder_*, rtc_lua_program_render_files): device bytes equal the host statement
(rtc_jpeg_format) byte for byte for rendered frames at several qualities, noise, edge sizes and a 4096^2 frame holding
every 24-bit colour once; render-and-encode at any gamma; the Lua loop's JPEG stills; the C++ facade's write_to_file_jpeg."""
import importlib
import io
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_host_jpeg import decode_coefficients  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


def device_jpeg(rtc, enc, pixels, quality):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(pixels)).to("cuda:0")
    torch.cuda.synchronize()
    return enc.encode_device(t.data_ptr(), pixels.shape[1], pixels.shape[0], pixels.shape[2], quality)


def assert_same(rtc, enc, pixels, quality, what):
    want = rtc.jpeg_encode(pixels, quality)
    got = device_jpeg(rtc, enc, pixels, quality)
    if got != want:
        k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{what}: device JPEG differs from the host's ({len(got)} vs {len(want)} bytes, first difference at {k})")
    return want


def test_rendered_frames_device_equals_host(rtc, gpu, scenes):
    cases = {"north_star": scenes.synthetic(100, 1920, 1080), "mixed": scenes.mixed(), "criterion": scenes.criterion(640, 480),
             "reflect_refract": rtc.load_yaml(path=os.path.join(os.path.dirname(rtc.__file__), "data", "reflect_refract.yml"))}
    enc = rtc.JpegEncoder(gpu)
    for name, (w, cam) in cases.items():
        dw = gpu.upload(w)
        f = dw.render_rgb8(cam)
        dw.close()
        for q in (1, 50, 75, 100):
            b = assert_same(rtc, enc, f, q, f"{name} q{q}")
        co = decode_coefficients(b)
        assert np.array_equal(co, rtc.jpeg_coefficients(f, 100)), name
    enc.close()


@pytest.mark.parametrize("shape", [(1, 1), (9, 1), (7, 7), (8, 8), (8, 9), (33, 17), (1, 65535), (97, 101)])
def test_noise_and_edge_sizes_device_equals_host(rtc, gpu, shape):
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    enc = rtc.JpegEncoder(gpu)
    noise = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    for q in (100, 75, 1):
        assert_same(rtc, enc, noise, q, f"noise {shape} q{q}")
    rgba = np.concatenate([noise, rng.integers(0, 256, shape + (1,), dtype=np.uint8)], -1)
    assert device_jpeg(rtc, enc, rgba, 90) == rtc.jpeg_encode(noise, 90)
    assert_same(rtc, enc, np.full(shape + (3,), (9, 200, 77), dtype=np.uint8), 75, f"flat {shape}")
    enc.close()


def test_every_24bit_colour_once_device_equals_host(rtc, gpu):
    """A 4096x4096 frame holding each of the 2^24 RGB colours once: the device's colour step for every input, exhaustively."""
    c = np.arange(1 << 24, dtype=np.uint32)
    f = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    enc = rtc.JpegEncoder(gpu)
    for q in (100, 75):
        assert_same(rtc, enc, f, q, f"all colours q{q}")
    enc.close()


def test_render_at_gamma_equals_host_encode(rtc, gpu, scenes, tmp_path):
    w, cam = scenes.synthetic(20, 320, 180)
    dw = gpu.upload(w)
    enc = rtc.JpegEncoder(gpu)
    assert enc.bytes() == b""
    got = enc.render(dw, cam, 1.0, 75)
    assert got == rtc.jpeg_encode(dw.render_rgba8(cam, 1.0), 75) == rtc.jpeg_encode(dw.render_rgb8(cam), 75)
    for g in (2.2, 0.5):
        for q in (75, 30):
            assert enc.render(dw, cam, g, q) == rtc.jpeg_encode(dw.render_rgba8(cam, g), q), (g, q)
    enc.write(tmp_path / "a.jpg")
    assert (tmp_path / "a.jpg").read_bytes() == enc.bytes()
    with pytest.raises(rtc.RtcError):
        enc.render(dw, cam, 1.0, 0)
    with pytest.raises(rtc.RtcError):
        enc.render(dw, cam, 0.0, 75)
    enc.close()
    dw.close()


def test_growing_and_shrinking_sizes_and_pipelined_launches(rtc, scenes):
    import torch
    ctx = rtc.Context(0)
    try:
        enc = rtc.JpegEncoder(ctx)
        rng = np.random.default_rng(7)
        frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((16, 16), (300, 500), (1080, 1920), (300, 500), (5, 3))]
        for f in frames:
            assert device_jpeg(rtc, enc, f, 75) == rtc.jpeg_encode(f, 75), f.shape
        for f in frames[::-1]:
            assert device_jpeg(rtc, enc, f, 100) == rtc.jpeg_encode(f, 100), f.shape
        # launches in flight on a pipelined context, then a fence: every ring buffer encodes to its frame's file
        w, cam = scenes.synthetic(20, 200, 120)
        dw = ctx.upload(w)
        want = dw.render_rgb8(cam)
        ctx.set_pipeline(3)
        ring = [torch.zeros((120, 200, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        f64 = torch.zeros((120, 200, 3), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        for t in ring:
            dw.render_rows(cam, 0, 120, f64.data_ptr(), d_ptr8=t.data_ptr())
        ctx.fence()
        for t in ring:
            assert enc.encode_device(t.data_ptr(), 200, 120, 3, 75) == rtc.jpeg_encode(want, 75)
        ctx.set_pipeline(1)
        dw.close()
        enc.close()
    finally:
        ctx.close()


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
w, c = scene(81, 45, 0.5)
Render(w, c, "second.JPEG")
w, c = scene(40, 30, -0.5)
Render(w, c, "third.png")
Render(w, c, "fourth.ppm")
local enc = StartAnimation("loop.gif")
for i = 1, 3 do
  w, c = scene(64, 48, i * 0.2)
  enc:AddFrame(w, c)
end
enc:Finish()
w, c = scene(33, 17, 1)
Render(w, c, "/some/dir/last.jpg")
"""


def _lua_program(rtc):
    return rtc.LuaProgram(text=LUA)


def test_lua_render_files(rtc, tmp_path):
    prog = _lua_program(rtc)
    jobs = prog.jobs
    ctx = rtc.Context(0)
    try:
        frames = prog.render(ctx)
        records = {}
        prog.render_gif(ctx, lambda i, data, outfile, kind: records.__setitem__(i, data) if kind == "AddFrame" else None)
        got = {}
        prog.render_files(ctx, lambda i, fmt, data, outfile, kind: got.__setitem__(i, (fmt, data.copy() if fmt == "rgb8" else data)))
        assert sorted(got) == list(range(len(jobs)))
        for i, j in enumerate(jobs):
            fmt, data = got[i]
            if j.kind == "AddFrame":
                assert fmt == "gif" and data == records[i], i
            elif j.outfile.lower().endswith((".jpg", ".jpeg")):
                assert fmt == "jpeg" and data == rtc.jpeg_encode(frames[i], 75), (i, j.outfile)
            else:
                assert fmt == "rgb8" and np.array_equal(data, frames[i]), i
        # another quality; a callback can stop the run
        q = {}
        prog.render_files(ctx, lambda i, fmt, data, outfile, kind: q.__setitem__(i, data), quality=40)
        assert q[0] == rtc.jpeg_encode(frames[0], 40)
        seen = []
        prog.render_files(ctx, lambda i, *a: seen.append(i) or len(seen) == 2)
        assert seen == [0, 1]
        with pytest.raises(rtc.RtcError):
            prog.render_files(ctx, lambda *a: None, quality=101)
        # the files under the script's names
        paths = prog.render_reference_files(ctx, tmp_path / "out")
        names = sorted(p.name for p in paths)
        assert names == sorted(["first.jpg", "second.JPEG", "third.png", "fourth.ppm", "loop.gif", "last.jpg"]), names
        assert (tmp_path / "out" / "first.jpg").read_bytes() == rtc.jpeg_encode(frames[0], 75)
        assert (tmp_path / "out" / "loop.gif").read_bytes() == rtc.gif_encode([frames[i] for i, j in enumerate(jobs) if j.kind == "AddFrame"])
        ref = prog.render_to_files(ctx, tmp_path / "png")
        for p in ref:
            if p.suffix.lower() in (".png", ".ppm") and ".gif." not in p.name and ".jpg" not in p.name.lower() and ".jpeg" not in p.name.lower():
                assert (tmp_path / "out" / p.name).read_bytes() == p.read_bytes(), p.name
        Image = pytest.importorskip("PIL.Image")
        im = Image.open(io.BytesIO((tmp_path / "out" / "first.jpg").read_bytes()))
        assert im.format == "JPEG" and im.size == (96, 64)
        dec = np.asarray(im.convert("RGB")).astype(np.float64)
        mse = float(np.mean((dec - frames[0]) ** 2))
        assert 10 * np.log10(255.0 ** 2 / max(mse, 1e-12)) > 25.0
    finally:
        ctx.close()


CPP = r'''
#include <cmath>
#include <cstdio>
#include "ch1.hpp"
using namespace ch1;
int main(int argc, char **argv) {
    World world = World::default_();
    Camera camera = Camera::new_with_transform(64, 48, M_PI / 3.0,
        Matrix::make_view_transform(Point::new_(0., 1.5, -5.), Point::new_(0., 0., 0.), Vector::new_(0., 1., 0.)));
    Canvas f64 = camera.render(world);
    f64.write_to_file_jpeg(argv[1]);
    f64.gamma = 2.2f;
    f64.write_to_file_jpeg(argv[2], 90);
    camera.render_rgba8(world, 2.2f).write_to_file_jpeg(argv[3], 90);
    camera.render_rgb8(world).write_to_file_jpeg(argv[4]);
    FILE *f = std::fopen(argv[5], "wb");
    std::fwrite(f64.pixels.data(), sizeof(double), f64.pixels.size(), f);
    std::fclose(f);
    try { camera.render(world).write_to_file("x.jpg"); std::puts("NO THROW"); return 1; } catch (const Panic &) {}
    std::puts("OK");
    return 0;
}
'''


def test_cpp_facade_write_to_file_jpeg(rtc, tmp_path):
    src = tmp_path / "jpeg.cpp"
    src.write_text(CPP)
    exe = tmp_path / "jpeg"
    pkg = ROOT / "raytracer-challenge_amd"
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{pkg / 'host'}", str(src), "-o", str(exe),
                    f"-L{pkg}", "-lrtc", f"-Wl,-rpath,{pkg}"], check=True, timeout=300)
    p = [tmp_path / n for n in ("a.jpg", "b.jpg", "c.jpg", "d.jpg", "f64.bin")]
    r = subprocess.run([str(exe), *map(str, p)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    canvas = np.fromfile(p[4], dtype=np.float64).reshape(48, 64, 3)
    assert p[0].read_bytes() == rtc.jpeg_encode(rtc.to_rgba8(canvas, 1.0), 75)
    assert p[1].read_bytes() == rtc.jpeg_encode(rtc.to_rgba8(canvas, 2.2), 90)
    assert p[2].read_bytes() == p[1].read_bytes()
    assert p[3].read_bytes() == p[0].read_bytes()
