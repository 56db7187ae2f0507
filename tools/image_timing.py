"""Save-by-name encoder timing on one GPU (include/rtc.h, csrc/rtc_image.hip), modelled on png_timing.py:
  * per format, one file of a rendered frame: ImageEncoder.render (render + encode on the device, only the file crossing
    PCIe) against rtc_render_rgb8 followed by the host statement (image_encode), and the bytes per file;
  * a Lua loop of N stills saved as `--lua-format` through LuaProgram.render_saved_files, per frame, against the same loop's
    rows (rtc_lua_program_render).
Prints one JSON line. Usage: python tools/image_timing.py [--width 1920 --height 1080 --frames 60 --reps 10 --lua-format bmp]"""
import argparse
import importlib
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from _bootstrap import package  # noqa: E402

FORMATS = ("bmp", "tga", "tiff", "farbfeld", "pam", "ico", "png", "jpeg", "gif", "ppm")
EXT = {"bmp": "bmp", "tga": "tga", "tiff": "tif", "farbfeld": "ff", "pam": "pam", "ico": "ico", "png": "png", "jpeg": "jpg",
       "gif": "gif", "ppm": "ppm"}


def timed(fn, reps):
    for _ in range(2):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lua-format", default="bmp")
    a = ap.parse_args()
    rtc = package()
    scenes = importlib.import_module(rtc.__name__ + ".scenes")
    ctx = rtc.Context(0)
    w, cam = scenes.synthetic(100, a.width, a.height)
    dw = ctx.upload(w)
    enc = rtc.ImageEncoder(ctx)
    res = {"size": f"{a.width}x{a.height}"}
    rows_ms, _ = timed(lambda: dw.render_rgb8(cam), a.reps)
    res["render_rgb8_ms"] = round(rows_ms, 4)
    small_w, small_h = min(a.width, 256), min(a.height, 256)   # ICO holds at most 256 x 256
    for fmt in FORMATS:
        c = cam if fmt != "ico" else scenes.synthetic(100, small_w, small_h)[1]
        dev_ms, b = timed(lambda: enc.render(fmt, dw, c), a.reps)
        host_ms, hb = timed(lambda: rtc.image_encode(fmt, dw.render_rgb8(c)), max(1, a.reps // 5))
        assert b == hb, fmt
        res[fmt] = {"device_ms": round(dev_ms, 4), "rgb8_then_host_ms": round(host_ms, 4), "bytes": len(b)}
        if fmt == "ico":
            res[fmt]["size"] = f"{small_w}x{small_h}"
    enc.close()
    dw.close()
    ext = EXT[a.lua_format]
    data = Path(rtc.__file__).resolve().parent / "data"
    text = (f"FRAMES = {a.frames} BALLS = 20 WIDTH, HEIGHT = {a.width}, {a.height}\n" + (data / "orbit_animation.lua").read_text())
    text = text.replace("film:AddFrame(world, camera)", f'Render(world, camera, string.format("still%04d.{ext}", frame))')
    prog = rtc.LuaProgram(text=text, base_dir=data)
    assert all(j.kind == "Render" for j in prog.jobs), "the orbit script changed: no AddFrame call to turn into stills"
    with tempfile.TemporaryDirectory() as tmp:
        prog.render_saved_files(ctx, Path(tmp) / "warm")
        t0 = time.perf_counter()
        paths = prog.render_saved_files(ctx, Path(tmp) / "saved")
        res[f"lua_saved_{a.lua_format}_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / len(paths), 4)
        prog.render(ctx)
        t0 = time.perf_counter()
        n = len(prog.render(ctx))
        res["lua_rows_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / n, 4)
    prog.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
