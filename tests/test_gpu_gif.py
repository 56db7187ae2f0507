"""The GIF writer on the MI355X (rtc_gif_writer_*, rtc_lua_program_render_gif): device bytes equal the host statement
(rtc_gif_format) byte for byte, for rendered frames, noise and edge sizes, and a 4096^2 frame; render-and-append; the
Lua AddFrame loop written as animated GIFs."""
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_host_gif import parse_gif, decoded_rgb, brute_nearest, S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


def device_gif(rtc, ctx, frames):
    import torch
    g = rtc.GifWriter(ctx)
    try:
        for f in frames:
            t = torch.from_numpy(np.ascontiguousarray(f)).to("cuda:0")
            torch.cuda.synchronize()
            g.append_device(t.data_ptr(), f.shape[1], f.shape[0])
        return g.bytes()
    finally:
        g.close()


def assert_same(rtc, ctx, frames, what):
    want = rtc.gif_encode(frames)
    got = device_gif(rtc, ctx, frames)
    if got != want:
        k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
        pytest.fail(f"{what}: device GIF differs from the host's ({len(got)} vs {len(want)} bytes, first difference at {k})")
    return want


def test_rendered_frames_device_equals_host(rtc, gpu, scenes):
    cases = {"north_star": scenes.synthetic(100, 1920, 1080), "mixed": scenes.mixed(), "criterion": scenes.criterion(640, 480),
             "reflect_refract": rtc.load_yaml(path=os.path.join(os.path.dirname(rtc.__file__), "data", "reflect_refract.yml"))}
    for name, (w, cam) in cases.items():
        dw = gpu.upload(w)
        f = dw.render_rgb8(cam)
        dw.close()
        b = assert_same(rtc, gpu, [f], name)
        g = parse_gif(b)
        pal, idx, used = rtc.gif_quantize(f)
        assert np.array_equal(decoded_rgb(g)[0], pal[idx]), name


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (13, 11), (1, S), (1, S - 1), (1, S + 1), (3, S), (2 * S + 3, 1), (97, 101)])
def test_noise_and_edge_frames_device_equals_host(rtc, gpu, shape):
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    noise = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    few = (rng.integers(0, 3, shape + (3,)) * 100).astype(np.uint8)
    assert_same(rtc, gpu, [noise, few, noise], f"noise/few {shape}")


def test_dictionary_fill_and_single_colour_device_equals_host(rtc, gpu):
    rng = np.random.default_rng(4)
    assert_same(rtc, gpu, [rng.integers(0, 256, (192, 64, 3), dtype=np.uint8)], "noise 3 segments")
    assert_same(rtc, gpu, [np.full((300, 200, 3), (9, 200, 77), dtype=np.uint8)], "one colour")
    v = np.arange(256, dtype=np.uint8)
    assert_same(rtc, gpu, [np.stack([v, v[::-1], v], -1).reshape(16, 16, 3)], "256 colours")


def test_4096_square_frame_device_equals_host(rtc, gpu):
    y, x = np.mgrid[0:4096, 0:4096]
    f = np.stack([x >> 4, y >> 4, (x ^ y) & 255], -1).astype(np.uint8)
    assert_same(rtc, gpu, [f], "4096^2")


def test_size_mismatch_is_an_argument_error(rtc, gpu):
    import torch
    g = rtc.GifWriter(gpu)
    t = torch.zeros(8 * 9 * 3, dtype=torch.uint8, device="cuda:0")
    g.append_device(t.data_ptr(), 9, 8)
    with pytest.raises(rtc.RtcError) as e:
        g.append_device(t.data_ptr(), 8, 9)
    assert "RTC_ERR_ARG" in str(e.value)
    with pytest.raises(rtc.RtcError):
        g.append_device(t.data_ptr(), 70000, 1)
    g.append_device(t.data_ptr(), 9, 8)
    assert len(parse_gif(g.bytes())["frames"]) == 2
    g.close()


def test_render_and_append_equals_render_then_host_encode(rtc, gpu, scenes, tmp_path):
    w, cam = scenes.synthetic(20, 320, 180)
    dw = gpu.upload(w)
    g = rtc.GifWriter(gpu)
    g.render(dw, cam)
    g.render(dw, cam)
    f = dw.render_rgb8(cam)
    want = rtc.gif_encode([f, f])
    assert g.bytes() == want
    g.write(tmp_path / "a.gif")
    assert (tmp_path / "a.gif").read_bytes() == want
    g.close()
    dw.close()


def test_lua_render_animations_orbit(rtc, tmp_path):
    data = Path(rtc.__file__).resolve().parent / "data"
    text = "FRAMES = 5 BALLS = 9 WIDTH, HEIGHT = 200, 136\n" + (data / "orbit_animation.lua").read_text()
    text += "\nenc2 = StartAnimation('second.gif')\nenc2:AddFrame(world, camera)\nenc2:AddFrame(world, camera)\n"
    prog = rtc.LuaProgram(text=text, base_dir=data)
    jobs = prog.jobs
    ctx = rtc.Context(0)
    frames = prog.render(ctx)
    stills = [j for j in jobs if j.kind == "Render"]
    anims = sorted({j.outfile for j in jobs if j.kind == "AddFrame"})
    assert len(anims) == 2 and len(stills) >= 1
    paths = prog.render_animations(ctx, tmp_path / "gif")
    ref = prog.render_to_files(ctx, tmp_path / "png")
    for p in ref:
        if not p.name.endswith(".png") or ".gif." not in p.name:
            assert (tmp_path / "gif" / p.name).read_bytes() == p.read_bytes(), p.name    # stills unchanged
    for a in anims:
        fr = [f for j, f in zip(jobs, frames) if j.kind == "AddFrame" and j.outfile == a]
        gp = tmp_path / "gif" / Path(a).name
        assert gp in paths
        b = gp.read_bytes()
        assert b == rtc.gif_encode(fr), a
        dec = decoded_rgb(parse_gif(b))
        assert len(dec) == len(fr)
        for d, f in zip(dec, fr):
            pal, idx, _ = rtc.gif_quantize(f)
            assert np.array_equal(idx.ravel(), brute_nearest(f, pal)) and np.array_equal(d, pal[idx])
    # a callback can stop the run
    seen = []
    prog.render_gif(ctx, lambda i, *a: seen.append(i) or len(seen) == 2)
    assert seen == [0, 1]
    # the context is in order afterwards: a plain render equals the Lua frame
    assert ctx.last_launch_info()["lane"] in (0, 1, 2, 3)
    dw = ctx.upload(jobs[2].world)
    assert np.array_equal(dw.render_rgb8(jobs[2].camera), frames[2])
    dw.close()
    ctx.close()
