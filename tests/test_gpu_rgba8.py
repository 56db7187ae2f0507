"""Canvas::to_imgbuf on the device (rtc_render_rgba8, rtc_render_views_rgba8, rtc_canvas_to_rgba8_device,
rtc_group_render_host_rgba8, Camera::render_rgba8 in host/ch1.hpp): byte for byte the host conversion rtc_canvas_to_rgba8
(glibc pow) of the f64 render, at every gamma, through every store path of the render kernel."""
import importlib
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _sibling(name):
    spec = importlib.util.spec_from_file_location("_rgba8_" + name, Path(__file__).with_name(name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


HOST = _sibling("test_host_rgba8")   # the CPU tests' sample of special values, thresholds +-50 ulp and random values


@pytest.fixture(scope="module")
def scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


SCENES = {
    "mixed_160x120": lambda s: s.mixed(160, 120),
    "mixed_50x37": lambda s: s.mixed(50, 37),                      # partial tiles: the unaligned (byte) store form
    "test8_aa": lambda s: s.test8(64, 48, samples=4),             # antialiasing; glass + reflective grid
    "default": lambda s: s.default_scene(33, 21),
    "reflective": lambda s: s.synthetic(30, 96, 54, reflective=True),
    "criterion_refractive": lambda s: s.criterion(120, 90),
    "north_star_1080p": lambda s: s.synthetic(100, 1920, 1080),
}


@pytest.mark.parametrize("gamma", HOST.GAMMAS)
def test_canvas_to_rgba8_device_equals_host(rtc, gamma):
    """k_canvas_to_rgba8 on a device canvas holding the CPU tests' sample, at widths 1, 7, 33 and 1920, aligned and not."""
    import torch
    c = HOST.sample(rtc.gamma_thresholds(gamma))
    ctx = rtc.Context(0)
    try:
        for W in (1, 7, 33, 1920):
            rows = -(-len(c) // (3 * W))
            canvas = np.zeros(rows * W * 3)
            canvas[: len(c)] = c
            canvas = canvas.reshape(rows, W, 3)
            want = rtc.to_rgba8(canvas, gamma)
            d_in = torch.from_numpy(canvas).to("cuda:0")
            d_out = torch.zeros(rows * W * 4 + 1, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            for off in (0, 1):   # 4-byte aligned (dword stores) and not (byte stores)
                d_out.fill_(7)
                torch.cuda.synchronize()
                ctx.canvas_to_rgba8_device(d_in.data_ptr(), W, rows, gamma, d_out.data_ptr() + off)
                ctx.synchronize()
                got = d_out.cpu().numpy()[off: off + rows * W * 4].reshape(rows, W, 4)
                bad = np.argwhere(got != want)
                assert bad.size == 0, (gamma, W, off, bad[:5], canvas.reshape(-1, 3)[bad[:5, 0] * W + bad[:5, 1]])
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_render_rgba8_equals_host_conversion(rtc, scenes, name):
    """rtc_render_rgba8 == rtc_canvas_to_rgba8(rtc_render(...), gamma), same ray counts; gamma 1 == rtc_render_rgb8 + alpha."""
    w, cam = SCENES[name](scenes)
    ctx = rtc.Context(0)
    try:
        dw = ctx.upload(w)
        for mode in (rtc.MODE_RENDER, rtc.MODE_RENDER_ASYNC):
            ref, st_ref = dw.render(cam, mode, with_stats=True)
            for gamma in (1.0, 2.2, 0.5):
                got, st = dw.render_rgba8(cam, gamma, mode, with_stats=True)
                want = rtc.to_rgba8(ref, gamma)
                bad = np.argwhere(got != want)
                assert bad.size == 0, (name, mode, gamma, len(bad), bad[:5])
                assert st == st_ref, (name, mode, gamma, st, st_ref)
                if gamma == 1.0:
                    assert np.array_equal(got[..., :3], dw.render_rgb8(cam, mode))
                    assert (got[..., 3] == 255).all()
        dw.close()
    finally:
        ctx.close()


def test_render_views_rgba8_views_and_bands(rtc, scenes):
    """rtc_render_views_rgba8: two views in one launch (culled and brute-force variants), and one frame's bands rendered per
    rank into a (ranks, 1, packed_rows, W, 4) buffer that group_undeal_host puts back together."""
    import torch
    w, cam = scenes.mixed(50, 37)
    W, H = cam.hsize, cam.vsize
    cam_b = rtc.camera(W, H, cam.fov, rtc.Matrix.make_view_transform((0.0, 1.5, -6.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)))
    ctx = rtc.Context(0)
    try:
        dw = ctx.upload(w)
        for gamma in (2.2, 1.0):
            want_a = rtc.to_rgba8(dw.render(cam), gamma)
            want_b = rtc.to_rgba8(dw.render(cam_b), gamma)
            view_rows = 48
            for flags in (0, rtc.FLAG_NO_CULL):
                buf = torch.zeros((2 * view_rows, W, 4), dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                dw.render_views_rgba8([cam, cam_b], 0, 1, buf.data_ptr(), view_rows, gamma, flags=flags)
                ctx.synchronize()
                h = buf.cpu().numpy()
                assert np.array_equal(h[:H], want_a) and np.array_equal(h[view_rows: view_rows + H], want_b), (gamma, flags)
                assert not h[H:view_rows].any() and not h[view_rows + H:].any()   # nothing written outside the views
            for N in (1, 2, 3):
                rows = rtc.group_packed_rows(H, N)
                staging = torch.zeros((N, 1, rows, W, 4), dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                for r in range(N):
                    dw.render_views_rgba8([cam], r, N, staging[r].data_ptr(), rows, gamma)
                ctx.synchronize()
                frame = rtc.group_undeal_host(staging.cpu().numpy(), N, 1, H)[0]
                assert np.array_equal(frame, want_a), (gamma, N)
        with pytest.raises(rtc.RtcError):
            dw.render_views_rgba8([cam], 0, 1, 0, 48, 2.2)             # no buffer
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(rtc.RtcError):
                dw.render_rgba8(cam, bad)
        dw.close()
    finally:
        ctx.close()


def test_pipelined_launches_with_different_gammas(rtc, scenes):
    """Depth 3: launches whose gammas alternate 2.2, 1.8, 1.0 are in flight on different lanes at once, each into its own
    buffer — and then more gammas than the context caches tables for (the cache starts afresh only when nothing can read it)."""
    import torch
    w, cam = scenes.synthetic(30, 160, 96)
    W, H = cam.hsize, cam.vsize
    ctx = rtc.Context(0)
    try:
        dw = ctx.upload(w)
        ref = dw.render(cam)
        for gammas in ([2.2, 1.8, 1.0] * 4, [1.0 + 0.05 * k for k in range(21)]):
            ctx.set_pipeline(3)
            bufs = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in gammas]
            torch.cuda.synchronize()
            for g, b in zip(gammas, bufs):
                dw.render_views_rgba8([cam], 0, 1, b.data_ptr(), 96, g)
            ctx.synchronize()
            for g, b in zip(gammas, bufs):
                assert np.array_equal(b.cpu().numpy(), rtc.to_rgba8(ref, g)), g
            ctx.set_pipeline(1)
        dw.close()
    finally:
        ctx.close()


def test_group_host_rgba8(rtc, scenes):
    """rtc_group_render_host_rgba8 (members rehearsed on one device with peer copies, as test_group_host_rgb8) equals the
    single-context frame."""
    W, H = 200, 117
    w, cam = scenes.synthetic(30, W, H)
    c = rtc.Context(0)
    dw = c.upload(w)
    want, want8 = dw.render_rgba8(cam, 2.2), dw.render_rgb8(cam)
    dw.close()
    c.close()
    for devices in ([0], [0, 0], [0, 0, 0]):
        g = rtc.Group(devices=devices, exchange=rtc.EXCHANGE_P2P)
        gw = g.upload(w)
        for out in (np.zeros((H, W, 4), dtype=np.uint8), rtc.host_canvas_rgba8(H, W)):
            got, st = gw.render_host_rgba8(cam, out, 2.2, with_stats=True)
            assert np.array_equal(got, want), len(devices)
            assert st["rays_primary"] == W * H
        # the RGB frame after the RGBA ones: the same tile buffers, 3 B/pixel again
        assert np.array_equal(gw.render_host_rgb8(cam, np.zeros((H, W, 3), dtype=np.uint8)), want8), len(devices)
        gw.close()
        g.close()


CPP = r'''
#include <cmath>
#include <cstdio>
#include "ch1.hpp"
using namespace ch1;
int main(int argc, char **argv) {
    World world = World::default_();
    Camera camera = Camera::new_with_transform(64, 48, M_PI / 3.0,
        Matrix::make_view_transform(Point::new_(0., 1.5, -5.), Point::new_(0., 0., 0.), Vector::new_(0., 1., 0.)));
    camera.render_rgba8(world, 2.2f).write_to_file(argv[1]);
    Canvas f64 = camera.render(world);
    FILE *f = std::fopen(argv[2], "wb");
    std::fwrite(f64.pixels.data(), sizeof(double), f64.pixels.size(), f);
    std::fclose(f);
    Canvas c = camera.render_async_rgba8(world, 2.2f);
    c.gamma = 1.8f;   // set_gamma after the render: the frame belongs to 2.2
    try { c.write_to_file(argv[1]); std::puts("NO THROW"); return 1; } catch (const Panic &) {}
    std::puts("OK");
    return 0;
}
'''


def test_cpp_facade_render_rgba8_png(rtc, tmp_path):
    """Camera::render_rgba8(world, 2.2f).write_to_file("x.png") through host/ch1.hpp: the decoded PNG equals the host
    conversion of Camera::render(world) at gamma 2.2; write_to_file refuses a frame whose gamma was changed afterwards."""
    src = tmp_path / "rgba8.cpp"
    src.write_text(CPP)
    exe = tmp_path / "rgba8"
    pkg = ROOT / "raytracer-challenge_amd"
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{ROOT / 'include'}", f"-I{pkg / 'host'}", str(src), "-o", str(exe),
                    f"-L{pkg}", "-lrtc", f"-Wl,-rpath,{pkg}"], check=True, timeout=300)
    png, raw = tmp_path / "x.png", tmp_path / "f64.bin"
    r = subprocess.run([str(exe), str(png), str(raw)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    got = _sibling("test_gpu_facade").decode_png(png.read_bytes())
    canvas = np.fromfile(raw, dtype=np.float64).reshape(48, 64, 3)
    assert got.shape == (48, 64, 4) and np.array_equal(got, rtc.to_rgba8(canvas, 2.2))
