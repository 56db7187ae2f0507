"""JPEG encoder timing on one GPU (include/rtc.h, csrc/rtc_jpeg.hip), modelled on gif_timing.py:
  * the encoder chain alone, from a rendered frame already in device memory (rtc_jpeg_encoder_encode_device: chain,
    the 8-byte length, the file's copy to the host), and the bytes per frame;
  * a Lua loop of N stills named .jpg through rtc_lua_program_render_files (render + encode on each lane, only the files
    cross PCIe) against the same loop through rtc_lua_program_render (8-bit rows), per frame.
Prints one JSON line. Usage: python tools/jpeg_timing.py [--width 1920 --height 1080 --frames 120 --quality 75]"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from _bootstrap import package  # noqa: E402


def lua_stills(n, w, h, ext):
    """n Render calls of one world (a reflective sphere on a checkered floor) from cameras on a circle: one world upload,
    then the one-camera-per-launch sequence the lanes overlap."""
    return f"""
local world = {{ lights = {{ {{ color = {{ r = 1, g = 1, b = 1 }}, position = {{ x = -10, y = 10, z = -10 }} }} }},
                shapes = {{ {{ type = "sphere", position = {{ x = 0, y = 1, z = 0 }},
                              color = {{ r = 1, g = 0.3, b = 0.2 }}, material = {{ reflectiveness = 0.3 }} }},
                           {{ type = "plane", pattern = {{ type = "checks", color_a = {{ r = 1, g = 1, b = 1 }},
                                                          color_b = {{ r = 0.1, g = 0.1, b = 0.1 }} }} }} }} }}
for i = 1, {n} do
  local camera = {{ screenwidth = {w}, screenheight = {h}, fov = 1.0,
                   position = {{ x = 5 * math.sin(i / 10), y = 1.5, z = -5 * math.cos(i / 10) }},
                   lookat = {{ x = 0, y = 1, z = 0 }}, up = {{ x = 0, y = 1, z = 0 }} }}
  Render(world, camera, string.format("still%04d.{ext}", i))
end
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    import torch
    rtc = package()
    scenes = importlib.import_module(rtc.__name__ + ".scenes")
    ctx = rtc.Context(0)
    w, cam = scenes.synthetic(100, a.width, a.height)
    dw = ctx.upload(w)
    frame = torch.zeros((a.height, a.width, 3), dtype=torch.uint8, device="cuda:0")
    f64 = torch.zeros((a.height, a.width, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dw.render_rows(cam, 0, a.height, f64.data_ptr(), d_ptr8=frame.data_ptr())
    ctx.synchronize()
    enc = rtc.JpegEncoder(ctx)
    b = enc.encode_device(frame.data_ptr(), a.width, a.height, 3, a.quality)
    assert b == rtc.jpeg_encode(frame.cpu().numpy(), a.quality)
    for _ in range(5):
        enc.encode_device(frame.data_ptr(), a.width, a.height, 3, a.quality)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        enc.encode_device(frame.data_ptr(), a.width, a.height, 3, a.quality)
    chain_ms = (time.perf_counter() - t0) * 1e3 / a.reps
    enc.close()
    dw.close()
    res = {"size": f"{a.width}x{a.height}", "quality": a.quality, "encode_device_ms": round(chain_ms, 4), "jpeg_bytes": len(b),
           "rows_bytes": 3 * a.width * a.height}
    for name, ext in (("rows", "png"), ("jpeg", "jpg")):
        prog = rtc.LuaProgram(text=lua_stills(a.frames, a.width, a.height, ext))
        sizes = []
        run = (lambda: prog.render(ctx, on_frame=lambda *x: False)) if name == "rows" else \
            (lambda: prog.render_files(ctx, lambda i, fmt, data, outfile, kind: sizes.append(len(data)), quality=a.quality))
        run()   # warm-up: worlds, scratch, page-locked buffers
        sizes.clear()
        t0 = time.perf_counter()
        run()
        res[f"lua_{name}_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / a.frames, 4)
        if sizes:
            res["lua_jpeg_mean_bytes"] = int(sum(sizes) / len(sizes))
        prog.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
