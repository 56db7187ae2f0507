"""The save-by-name writer on the MI355X (rtc_image_encoder_*, rtc_lua_program_render_saved): device bytes equal the host
statement (rtc_image_format) for every format of the save table — rendered scenes at gamma 1 and 2.2, noise in 3 and 4
channels, edge sizes, 4096^2 frames for the uncompressed formats, one encoder across formats and sizes; a Lua script's
stills and animation through render_saved_files; the C++ facade's Canvas::save."""
import importlib
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
FORMATS = ("bmp", "tga", "tiff", "ico", "farbfeld", "pam", "png", "jpeg", "gif", "ppm")
PACKED = ("bmp", "tga", "tiff", "farbfeld", "pam")


@pytest.fixture(scope="module")
def scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


def device_file(enc, fmt, pixels):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(pixels)).to("cuda:0")
    torch.cuda.synchronize()
    return enc.encode_device(fmt, t.data_ptr(), pixels.shape[1], pixels.shape[0], pixels.shape[2])


def assert_same(rtc, enc, fmt, pixels, what):
    want = rtc.image_encode(fmt, pixels)
    got = device_file(enc, fmt, pixels)
    if got != want:
        k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{what} {fmt}: device file differs from the host's ({len(got)} vs {len(want)} bytes, first difference at {k})")


def fits(fmt, h, w):
    return not (fmt == "ico" and max(h, w) > 256)


def test_rendered_scenes_at_gamma_device_equals_host(rtc, gpu, scenes):
    enc = rtc.ImageEncoder(gpu)
    assert enc.bytes() == b""
    for name, (w, cam) in {"synthetic": scenes.synthetic(20, 320, 180), "mixed": scenes.mixed(),
                           "icon": scenes.synthetic(8, 256, 256), "odd": scenes.synthetic(5, 97, 13)}.items():
        dw = gpu.upload(w)
        rgb8 = dw.render_rgb8(cam)
        for fmt in FORMATS:
            if not fits(fmt, cam.vsize, cam.hsize):
                continue
            assert enc.render(fmt, dw, cam, 1.0) == rtc.image_encode(fmt, rgb8), (name, fmt)
            assert enc.render(fmt, dw, cam, 2.2) == rtc.image_encode(fmt, dw.render_rgba8(cam, 2.2)), (name, fmt)
            assert_same(rtc, enc, fmt, rgb8, name)
        dw.close()
    enc.close()


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17), (256, 256), (3, 16385), (2, 16384), (61, 4097)])
def test_noise_and_edge_sizes_device_equals_host(rtc, gpu, shape):
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    enc = rtc.ImageEncoder(gpu)
    rgb = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    rgba = rng.integers(0, 256, shape + (4,), dtype=np.uint8)   # alpha is never read
    for fmt in FORMATS:
        if fits(fmt, *shape):
            assert_same(rtc, enc, fmt, rgb, f"noise {shape}")
            assert_same(rtc, enc, fmt, rgba, f"noise rgba {shape}")
            assert device_file(enc, fmt, rgba) == rtc.image_encode(fmt, rgba[..., :3].copy())
    enc.close()


def test_4096_squared_uncompressed(rtc, gpu):
    rng = np.random.default_rng(4096)
    enc = rtc.ImageEncoder(gpu)
    f = rng.integers(0, 256, (4096, 4096, 3), dtype=np.uint8)
    for fmt in PACKED:
        assert_same(rtc, enc, fmt, f, "4096^2")
    f4 = np.concatenate([f, np.zeros((4096, 4096, 1), np.uint8)], axis=2)
    assert_same(rtc, enc, "bmp", f4, "4096^2 rgba")
    enc.close()


def test_one_encoder_across_formats_and_sizes(rtc, gpu):
    rng = np.random.default_rng(11)
    enc = rtc.ImageEncoder(gpu)
    frames = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((16, 16), (300, 500), (1080, 1920), (200, 256), (5, 3))]
    for f in frames + frames[::-1]:
        for fmt in FORMATS:
            if fits(fmt, *f.shape[:2]):
                assert_same(rtc, enc, fmt, f, f"{f.shape}")
    with pytest.raises(rtc.RtcError):
        device_file(enc, "ico", frames[1])      # 500 wide
    with pytest.raises(rtc.RtcError):
        device_file(enc, 10, frames[0])         # not a format
    enc.close()


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
local names = { "a.bmp", "b.TGA", "c.tif", "d.ico", "e.ff", "f.pam", "g.jpg", "h.png", "i.gif", "j.ppm" }
for k, name in ipairs(names) do
  local w, c = scene(40 + 7 * k, 30 + 3 * k, k * 0.1)
  Render(w, c, NAMEDIR .. name)
end
local enc = StartAnimation("loop.gif")
for i = 1, 3 do
  local w, c = scene(64, 48, i * 0.2)
  enc:AddFrame(w, c)
end
enc:Finish()
"""
EXT = {".bmp": "bmp", ".tga": "tga", ".tif": "tiff", ".ico": "ico", ".ff": "farbfeld", ".pam": "pam", ".jpg": "jpeg",
       ".png": "png", ".gif": "gif", ".ppm": "ppm"}


def test_lua_render_saved_files(rtc, gpu, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    prog = rtc.LuaProgram(text='NAMEDIR = "some/dir/"\n' + LUA)
    jobs = prog.jobs
    frames = prog.render(gpu)
    paths = prog.render_saved_files(gpu, tmp_path / "out")
    names = [p.name for p in paths]
    assert names == ["a.bmp", "b.TGA", "c.tif", "d.ico", "e.ff", "f.pam", "g.jpg", "h.png", "i.gif", "j.ppm", "loop.gif"], names
    for i, j in enumerate(jobs):
        if j.kind != "Render":
            continue
        p = tmp_path / "out" / Path(j.outfile).name
        fmt = EXT[p.suffix.lower()]
        b = p.read_bytes()
        assert b == rtc.image_encode(fmt, frames[i]), p.name
        if fmt in ("bmp", "tga", "tiff", "ico", "png", "ppm"):   # lossless (JPEG is not, nor GIF above 256 colours)
            dec = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
            assert np.array_equal(dec, frames[i]), p.name
    # JPEG, PNG and GIF equal what the existing paths write for the same jobs
    ref = {Path(p).name: Path(p) for p in prog.render_reference_files(gpu, tmp_path / "ref")}
    assert (tmp_path / "out" / "g.jpg").read_bytes() == ref["g.jpg"].read_bytes()
    assert (tmp_path / "out" / "loop.gif").read_bytes() == ref["loop.gif"].read_bytes()
    assert (tmp_path / "out" / "j.ppm").read_bytes() == ref["j.ppm"].read_bytes()
    assert "a.bmp.png" in ref                        # render_reference_files keeps its names
    png = {Path(p).name: Path(p) for p in prog.render_png_files(gpu, tmp_path / "png")}
    assert (tmp_path / "out" / "h.png").read_bytes() == png["h.png"].read_bytes()
    anim = {Path(p).name: Path(p) for p in prog.render_animations(gpu, tmp_path / "anim")}
    assert (tmp_path / "out" / "loop.gif").read_bytes() == anim["loop.gif"].read_bytes()
    assert (tmp_path / "out" / "i.gif").read_bytes() == rtc.gif_encode([frames[8]])
    # an unsupported name: nothing rendered, nothing written
    bad = rtc.LuaProgram(text='NAMEDIR = ""\n' + LUA.replace('"j.ppm"', '"j.xyz"'))
    with pytest.raises(rtc.RtcError) as e:
        bad.render_saved_files(gpu, tmp_path / "bad")
    assert e.value.status == 8
    assert not (tmp_path / "bad").exists()


CPP = r'''
#include <cmath>
#include <cstdio>
#include <string>
#include "ch1.hpp"
using namespace ch1;
int main(int argc, char **argv) {
    World world = World::default_();
    Camera camera = Camera::new_with_transform(64, 48, M_PI / 3.0,
        Matrix::make_view_transform(Point::new_(0., 1.5, -5.), Point::new_(0., 0., 0.), Vector::new_(0., 1., 0.)));
    const std::string dir = argv[1];
    const char *names[] = {"a.bmp", "b.tga", "c.tiff", "d.ico", "e.ff", "f.pam", "g.png", "h.jpeg", "i.gif", "j.ppm"};
    Canvas f64 = camera.render(world);
    Canvas rgba = camera.render_rgba8(world, 2.2f);
    Canvas rgb8 = camera.render_rgb8(world);
    for (const char *n : names) {
        f64.save(dir + "/f64_" + n);
        rgba.save(dir + "/rgba_" + n);
        rgb8.save(dir + "/rgb8_" + n);
    }
    FILE *f = std::fopen((dir + "/f64.bin").c_str(), "wb");
    std::fwrite(f64.pixels.data(), sizeof(double), f64.pixels.size(), f);
    std::fclose(f);
    try { f64.save(dir + "/x.xyz"); std::puts("NO THROW"); return 1; } catch (const Panic &p) { if (p.status != RTC_ERR_UNSUPPORTED) return 2; }
    try { f64.write_to_file(dir + "/x.bmp"); std::puts("NO THROW"); return 1; } catch (const Panic &) {}
    std::puts("OK");
    return 0;
}
'''


def test_cpp_facade_canvas_save(rtc, tmp_path):
    src = tmp_path / "save.cpp"
    src.write_text(CPP)
    exe = tmp_path / "save"
    pkg = ROOT / "raytracer-challenge_amd"
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{pkg / 'host'}", str(src), "-o", str(exe),
                    f"-L{pkg}", "-lrtc", f"-Wl,-rpath,{pkg}"], check=True, timeout=300)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    canvas = np.fromfile(tmp_path / "f64.bin", dtype=np.float64).reshape(48, 64, 3)
    for n, fmt in {"a.bmp": "bmp", "b.tga": "tga", "c.tiff": "tiff", "d.ico": "ico", "e.ff": "farbfeld", "f.pam": "pam",
                   "g.png": "png", "h.jpeg": "jpeg", "i.gif": "gif", "j.ppm": "ppm"}.items():
        assert (tmp_path / f"f64_{n}").read_bytes() == rtc.image_encode(fmt, rtc.to_rgba8(canvas, 1.0)), n
        assert (tmp_path / f"rgba_{n}").read_bytes() == rtc.image_encode(fmt, rtc.to_rgba8(canvas, 2.2)), n
        assert (tmp_path / f"rgb8_{n}").read_bytes() == (tmp_path / f"f64_{n}").read_bytes(), n
    assert not (tmp_path / "x.xyz").exists() and not (tmp_path / "x.bmp").exists()
