"""What the AOV, ambient-occlusion and gather passes cost under an orthographic and a full-sphere panorama camera (include/rtc.h
"the three passes under an orthographic or panorama camera"), at 1920x1080, on two Worlds: synthetic(100) — the north star —
and the 10 000 spheres of `bench.py --workload c3`. Per World and projection, four passes:
  (a) k_aov with `index` + `depth` only        (b) all six planes        (c) AO, 16 samples        (d) gather, 16 samples
each beside its PINHOLE TWIN — the same pass, World, camera position and frame size through the pinhole entry — measured
in the same run, interleaved: `rounds` rounds of (projection launch, twin launch), each launch between two HIP events on the
context's stream; the figure is the median over the rounds, beside the smallest and largest (the run-to-run spread to read a
ratio against). The twin is the yardstick; no ratio is asserted. The twin stands where the projection's camera stands but
sees other pixels: `hit_pixels` and `twin_hit_pixels` say how many rays of each hit something, and for the two fan passes,
whose work is per hit pixel, the ratio is given a second time per hit pixel. The orthographic camera stands above the scene and is
--ortho-width world units wide; the panorama stands among the shapes.
  (old) the only other route to the six planes of one frame: rtc_projection_ray per pixel on the host, then rtc_color_at over
      those rays with hit records, wall time, ONE run per World and projection; its index / depth / flags must equal (b)'s.
Prints one JSON line per World and projection, then a table.
usage: python tools/projection_pass_cost.py [--rounds 20] [--warmup 3] [--worlds ns,c3] [--ortho-width 30]"""
import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _bootstrap import package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--worlds", default="ns,c3")
ap.add_argument("--ortho-width", type=float, default=30.0)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--skip-old-route", action="store_true")
args = ap.parse_args()

rtc = package()
abi = __import__("importlib").import_module(rtc.__name__ + ".abi")
scenes = __import__("importlib").import_module(rtc.__name__ + ".scenes")
W, H = args.width, args.height
NPX = W * H
ABOVE = ((0.0, 6.0, -8.0), (0.0, 0.5, 10.0), (0.0, 1.0, 0.0))
AMONG = ((0.3, 1.2, 8.0), (0.0, 1.0, 20.0), (0.0, 1.0, 0.0))


def build(name):
    if name == "ns":
        return scenes.synthetic(100, W, H)[0], "synthetic(100): 100 spheres + checker floor (north star)"
    if name == "c3":
        return scenes.synthetic(10000, W, H, with_plane=False)[0], "10 000 random spheres (bench.py --workload c3)"
    raise KeyError(name)


stream = torch.cuda.Stream()
ctx = rtc.Context(0, stream=stream.cuda_stream)
dev = {p: torch.zeros(NPX * comps, dtype=getattr(torch, d), device="cuda:0") for p, (d, comps) in abi.AOV_PLANES.items()}
d_ao = torch.zeros(NPX * 2, dtype=torch.uint8, device="cuda:0")
d_rad, d_bounce = (torch.zeros(NPX * 3, dtype=torch.float64, device="cuda:0") for _ in range(2))
torch.cuda.synchronize()


def interleaved_ms(launch_a, launch_b):
    """(a, b): median / min / max ms of `rounds` launches each, between two events around every launch, a and b in turn"""
    for _ in range(args.warmup):
        launch_a()
        launch_b()
    ctx.synchronize()
    pairs = ([], [])
    with torch.cuda.stream(stream):
        for _ in range(args.rounds):
            for k, launch in enumerate((launch_a, launch_b)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                pairs[k].append((e0, e1))
    ctx.synchronize()
    out = []
    for ps in pairs:
        ms = sorted(a.elapsed_time(b) for a, b in ps)
        out.append({"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]})
    return out


rows = []
fan = rtc.ao(math.inf, 4, 4)
for name in args.worlds.split(","):
    world, desc = build(name)
    dw = ctx.upload(world)
    ptr = {p: t.data_ptr() for p, t in dev.items()}
    two = {p: ptr[p] for p in ("index", "depth")}
    for kind in ("orthographic", "panorama"):
        cam = rtc.camera(W, H, 1.0, rtc.Matrix.make_view_transform(*(ABOVE if kind == "orthographic" else AMONG)))
        proj = rtc.projection(kind, width=args.ortho_width) if kind == "orthographic" else rtc.projection(kind)
        r = {"world": name, "desc": desc, "projection": kind, "frame": f"{W}x{H}", "objects": len(world), "rounds": args.rounds}
        passes = {
            "a_index_depth": lambda p: dw.render_aov_device(cam, two, projection=p),
            "b_all_six": lambda p: dw.render_aov_device(cam, ptr, projection=p),
            "c_ao_16": lambda p: dw.render_ao_device(cam, fan, d_ao.data_ptr(), projection=p),
            "d_gather_16": lambda p: dw.render_gather_device(cam, fan, {"radiance": d_rad.data_ptr(), "bounce": d_bounce.data_ptr()}, projection=p),
        }
        for key, launch in passes.items():
            got, twin = interleaved_ms(lambda: launch(proj), lambda: launch(None))
            r[key] = {"projection": got, "pinhole_twin": twin, "ratio": got["median_ms"] / twin["median_ms"]}
        dw.render_aov_device(cam, ptr, projection=proj)
        ctx.synchronize()
        r["source"] = ctx.last_launch_info()["source"]
        planes = {p: dev[p].cpu().numpy() for p in ("index", "depth", "flags")}
        r["hit_pixels"] = int((planes["index"] >= 0).sum())
        # the twin sees other pixels: how many of ITS rays hit (every hit pixel runs the shadow passes and the fans)
        dw.render_aov_device(cam, two, projection=None)
        ctx.synchronize()
        r["twin_hit_pixels"] = int((dev["index"] >= 0).sum().item())
        for key in ("c_ao_16", "d_gather_16"):
            r[key]["ratio_per_hit_pixel"] = r[key]["ratio"] * r["twin_hit_pixels"] / max(1, r["hit_pixels"])
        if not args.skip_old_route:
            # the old route: a ray per pixel on the host, rtc_color_at with hit records, the planes from the records
            t = time.perf_counter()
            rays = np.empty((NPX, 6), dtype=np.float64)
            ray, fn, camr, projr = (C.c_double * 6)(), rtc.lib().rtc_projection_ray, C.byref(cam), C.byref(proj)
            for y in range(H):
                for x in range(W):
                    fn(camr, projr, x, y, ray)
                    rays[y * W + x] = ray[:]
            r["old_rays_wall_ms"] = (time.perf_counter() - t) * 1e3
            rgb = np.empty((NPX, 3), dtype=np.float64)
            hits = (rtc.RtcHit * NPX)()
            P = C.POINTER(C.c_double)
            t = time.perf_counter()
            st = rtc.lib().rtc_color_at(ctx._h, dw._h, rays.ctypes.data_as(P), NPX, 5, 0, rgb.ctypes.data_as(P), hits)
            assert st == 0, st
            want = rtc.aov_from_hits(hits, W, H, planes=("index", "depth", "flags"))
            r["old_color_at_wall_ms"] = (time.perf_counter() - t) * 1e3
            r["old_route_equal"] = {p: bool(np.array_equal(planes[p], want[p].reshape(-1))) for p in planes}
            wall = []
            for _ in range(3):   # (fresh pageable arrays every call; the first call also grows the context's scratch)
                t = time.perf_counter()
                dw.render_aov(cam, projection=proj)
                wall.append((time.perf_counter() - t) * 1e3)
            r["new_all_six_with_copy_wall_ms"] = sorted(wall)[1]
            del hits, want, rays, rgb
        rows.append(r)
        print(json.dumps(r), flush=True)
    dw.close()
ctx.close()

print()
print("| world | projection | source | pass | projection, median (min .. max) ms | pinhole twin, median (min .. max) ms | ratio | hit pixels: projection / twin | ratio per hit pixel |")
print("|---|---|---|---|---|---|---|---|---|")
for r in rows:
    for key in ("a_index_depth", "b_all_six", "c_ao_16", "d_gather_16"):
        g, t = r[key]["projection"], r[key]["pinhole_twin"]
        print(f"| {r['world']} ({r['objects']} objects) | {r['projection']} | {r['source']} | {key} | {g['median_ms']:.4f} ({g['min_ms']:.4f} .. {g['max_ms']:.4f}) | "
              f"{t['median_ms']:.4f} ({t['min_ms']:.4f} .. {t['max_ms']:.4f}) | {r[key]['ratio']:.2f} | {r['hit_pixels']} / {r['twin_hit_pixels']} | "
              + (f"{r[key]['ratio_per_hit_pixel']:.2f} |" if "ratio_per_hit_pixel" in r[key] else "|"))
if not args.skip_old_route:
    print()
    print("| world | projection | old route: rays on the host, wall | old route: rtc_color_at + packing, wall | rtc_render_aov_projection, six planes with the copy, wall | planes equal |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['world']} | {r['projection']} | {r['old_rays_wall_ms']:.0f} ms | {r['old_color_at_wall_ms']:.0f} ms | {r['new_all_six_with_copy_wall_ms']:.1f} ms | "
              f"{all(r['old_route_equal'].values())} |")
    sys.exit(0 if all(all(r["old_route_equal"].values()) for r in rows) else 1)
