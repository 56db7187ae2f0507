"""Time lua.rs's render_lua on the GPU for the orbit script (rtc_lua_program_render: one launch per AddFrame, pipelined,
frames copied to the host) against the same jobs rendered one by one through rtc_render_rgb8. python tools/lua_animation_timing.py

python tools/lua_animation_timing.py moving [rounds]: the moving-world loops instead — bouncing_animation.lua (120 frames,
1080p, every frame another world), the same script among 9 997 bystanders (10 001 shapes, two balls and the light moving)
and with ONE moving sphere among them — under
RTC_WORLD_UPDATE=0 (destroy and create per frame) and =1 (rtc_world_update), the two settings interleaved, and the orbit
loop (one world) both ways as the control. Prints ms per delivered frame of every round and the medians."""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from _bootstrap import package  # noqa: E402

rtc = package()
data = Path(rtc.__file__).resolve().parent / "data"
rtc.LuaProgram(text="x = 1")   # (loads the library)


def moving(rounds):
    import os
    import statistics
    cases = (("bouncing 4 shapes", "bouncing_animation.lua", "FRAMES = 120 WIDTH, HEIGHT = 1920, 1080\n"),
             ("bouncing 10001 shapes", "bouncing_animation.lua", "FRAMES = 120 BALLS = 9997 WIDTH, HEIGHT = 1920, 1080\n"),
             ("one moving sphere of 10001 shapes", "bouncing_animation.lua", "FRAMES = 120 BALLS = 9997 ONLY_RED = true WIDTH, HEIGHT = 1920, 1080\n"),
             ("orbit 102 shapes (one world)", "orbit_animation.lua", "FRAMES = 120 BALLS = 100 WIDTH, HEIGHT = 1920, 1080\n"))
    for name, script, head in cases:
        prog = rtc.LuaProgram(text=head + (data / script).read_text(), base_dir=data)
        ctxs = {}
        for setting in ("0", "1"):
            os.environ["RTC_WORLD_UPDATE"] = setting
            ctxs[setting] = rtc.Context(0)
            prog.render(ctxs[setting], on_frame=lambda *a: None)     # warm
        del os.environ["RTC_WORLD_UPDATE"]
        ms = {"0": [], "1": []}
        for _ in range(rounds):
            for setting in ("0", "1"):   # interleaved
                t = time.perf_counter()
                prog.render(ctxs[setting], on_frame=lambda *a: None)
                ms[setting].append((time.perf_counter() - t) / len(prog) * 1e3)
        m0, m1 = statistics.median(ms["0"]), statistics.median(ms["1"])
        print(f"{name}, {len(prog)} jobs, 1920x1080 rgb8 delivered, ms per frame: RTC_WORLD_UPDATE=0 {' '.join('%.3f' % v for v in ms['0'])} (median {m0:.3f}); "
              f"=1 {' '.join('%.3f' % v for v in ms['1'])} (median {m1:.3f}); ratio =0/=1 {m0 / m1:.2f}", flush=True)
        for c in ctxs.values():
            c.close()


if len(sys.argv) > 1 and sys.argv[1] == "moving":
    moving(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    sys.exit(0)
for frames, balls, w, h in ((120, 100, 1920, 1080), (120, 24, 600, 400)):
    text = f"FRAMES = {frames} BALLS = {balls} WIDTH, HEIGHT = {w}, {h}\n" + (data / "orbit_animation.lua").read_text()
    t = time.perf_counter()
    prog = rtc.LuaProgram(text=text, base_dir=data)
    t_script = time.perf_counter() - t
    jobs = prog.jobs
    ctx = rtc.Context(0)
    count = [0]
    prog.render(ctx, on_frame=lambda *a: count.__setitem__(0, count[0] + 1))     # warm
    t = time.perf_counter()
    _, st = prog.render(ctx, on_frame=lambda *a: None, with_stats=True)
    t_pipe = time.perf_counter() - t
    dw = ctx.upload(jobs[0].world)
    out = rtc.host_canvas_rgb8(h, w)
    dw.render_rgb8(jobs[0].camera, out=out)
    t = time.perf_counter()
    for j in jobs[:frames]:
        dw.render_rgb8(j.camera, out=out)
    t_serial = time.perf_counter() - t
    rays = sum(st[k] for k in ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract"))
    print(f"{w}x{h}, {len(jobs[0].world)} shapes, {len(jobs)} jobs: script {t_script * 1e3:.1f} ms; rtc_lua_program_render {t_pipe / len(jobs) * 1e3:.3f} ms per frame "
          f"({rays / t_pipe / 1e9:.1f} Grays/s all rays, frames on the host); one rtc_render_rgb8 per frame {t_serial / frames * 1e3:.3f} ms", flush=True)
    ctx.close()
