"""Time the Lua AddFrame loop written as an animated GIF on the GPU (rtc_lua_program_render_gif: quantiser and LZW behind
each render, only the compressed record copied) against today's rtc_lua_program_render (8-bit rows copied to the host),
for the orbit script at 1920x1080, 120 frames. Also the GIF kernels one by one (device events around each stage of one
frame, k_gif_* in a profiler trace) and the bytes per frame.
    python tools/gif_timing.py [FRAMES]"""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from _bootstrap import package  # noqa: E402


def main(argv):
    import numpy as np
    import torch
    rtc = package()
    data = Path(rtc.__file__).resolve().parent / "data"
    frames = int(argv[1]) if len(argv) > 1 else 120
    w, h = 1920, 1080
    text = f"FRAMES = {frames} BALLS = 100 WIDTH, HEIGHT = {w}, {h}\n" + (data / "orbit_animation.lua").read_text()
    prog = rtc.LuaProgram(text=text, base_dir=data)
    jobs = prog.jobs
    n_add = sum(j.kind == "AddFrame" for j in jobs)
    ctx = rtc.Context(0)
    sizes = []
    prog.render(ctx, on_frame=lambda *a: None)                                       # warm both paths
    prog.render_gif(ctx, lambda i, d, o, k: sizes.append(len(d)) if k == "AddFrame" else None)
    best_rows, best_gif = [], []
    for _ in range(3):                                                               # alternate the two paths
        t = time.perf_counter()
        prog.render(ctx, on_frame=lambda *a: None)
        best_rows.append((time.perf_counter() - t) / len(jobs))
        t = time.perf_counter()
        prog.render_gif(ctx, lambda *a: None)
        best_gif.append((time.perf_counter() - t) / len(jobs))
    rows_b = w * h * 3
    print(f"orbit {w}x{h}, {len(jobs[0].world)} shapes, {len(jobs)} jobs ({n_add} AddFrame)")
    print(f"rtc_lua_program_render     {min(best_rows) * 1e3:.3f} ms per frame (runs: {', '.join(f'{x * 1e3:.3f}' for x in best_rows)}), "
          f"{rows_b} B per frame to the host")
    print(f"rtc_lua_program_render_gif {min(best_gif) * 1e3:.3f} ms per frame (runs: {', '.join(f'{x * 1e3:.3f}' for x in best_gif)}), "
          f"{np.mean(sizes):.0f} B per frame to the host (min {min(sizes)}, max {max(sizes)}; {rows_b / np.mean(sizes):.1f}x fewer)")
    # one frame's GIF chain alone, device time, on a frame already in HBM
    dw = ctx.upload(jobs[0].world)
    f = dw.render_rgb8(jobs[0].camera)
    t = torch.from_numpy(f).to("cuda:0")
    g = rtc.GifWriter(ctx)
    torch.cuda.synchronize()
    for _ in range(3):
        g.append_device(t.data_ptr(), w, h)
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        g.append_device(t.data_ptr(), w, h)
    one = (time.perf_counter() - t0) / reps
    print(f"GifWriter.append_device, one frame in HBM, synchronous (all GIF kernels + length read-back + record copy): {one * 1e3:.3f} ms")
    t0 = time.perf_counter()
    for _ in range(reps):
        rtc.gif_encode([f])
    print(f"host rtc_gif_format, one frame: {(time.perf_counter() - t0) / reps * 1e3:.1f} ms")
    g.close()
    dw.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
