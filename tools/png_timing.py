"""Compressed PNG encoder timing on one GPU (include/rtc.h, csrc/rtc_png.hip), modelled on jpeg_timing.py:
  * the encoder chain alone, from a rendered frame already in device memory (rtc_png_encoder_encode_device: chain, the
    8-byte length, the file's copy to the host), and the bytes per file against the stored writer's;
  * a Lua orbit loop of N AddFrame frames written as numbered PNGs: LuaProgram.render_png_files (render + encode on each
    lane, only the files cross PCIe) against render_to_files (8-bit rows over PCIe, the host's stored writer), per frame.
Prints one JSON line. Usage: python tools/png_timing.py [--width 1920 --height 1080 --frames 120 --reps 20]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=20)
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
    enc = rtc.PngEncoder(ctx)
    b = enc.encode_device(frame.data_ptr(), a.width, a.height, 3)
    host = frame.cpu().numpy()
    assert b == rtc.png_encode(host)
    stored = len(rtc.format_png(host))
    for _ in range(3):
        enc.encode_device(frame.data_ptr(), a.width, a.height, 3)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        enc.encode_device(frame.data_ptr(), a.width, a.height, 3)
    chain_ms = (time.perf_counter() - t0) * 1e3 / a.reps
    enc.close()
    dw.close()
    res = {"size": f"{a.width}x{a.height}", "encode_device_ms": round(chain_ms, 4), "png_bytes": len(b), "stored_png_bytes": stored,
           "ratio_vs_stored": round(len(b) / stored, 4)}
    data = Path(rtc.__file__).resolve().parent / "data"
    text = f"FRAMES = {a.frames} BALLS = 20 WIDTH, HEIGHT = {a.width}, {a.height}\n" + (data / "orbit_animation.lua").read_text()
    prog = rtc.LuaProgram(text=text, base_dir=data)
    with tempfile.TemporaryDirectory() as tmp:
        for name, run in (("stored", lambda d: prog.render_to_files(ctx, d)), ("gpu_png", lambda d: prog.render_png_files(ctx, d))):
            run(Path(tmp) / (name + "_warm"))   # warm-up: worlds, scratch, page-locked buffers
            t0 = time.perf_counter()
            paths = run(Path(tmp) / name)
            res[f"lua_{name}_ms_per_frame"] = round((time.perf_counter() - t0) * 1e3 / len(paths), 4)
            frames = [p for p in paths if ".gif." in p.name]
            res[f"lua_{name}_mean_bytes"] = int(sum(p.stat().st_size for p in frames) / max(len(frames), 1))
    prog.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
