"""What the AOV planes cost (include/rtc.h "arbitrary output variables"), at 1920x1080, on three Worlds: synthetic(100) — the
north star —, the 10 000 spheres of `bench.py --workload c3`, and data/soft_shadows.yml (17 light samples). Per World:
  (a) k_aov with `index` + `depth` only            (b) every plane but `shadow`            (c) all six planes
  (d) the colour launch rtc_render_rows of the same World and camera
  (e) the only other route to the same data: wall time of rtc_color_at over the frame's 2 073 600 centre rays with hit
      records — ONE run (48 B up and 184 + 24 B down per ray, the whole shading recursion for a colour nobody reads)
  (c+copy) wall time of rtc_render_aov: launch (c) and the copy of the six planes to (pageable) host memory
(a)-(d) are kernel times: the median of --launches launches (after --warmup) between two HIP events recorded around each
launch on the context's stream — the context is created on a torch stream (Context(stream=...)) and the events are
torch.cuda.Event pairs on it; (d) is given a second time from the launch's own dispatch timestamps (rtc_kernel_times_ms,
what rtc_last_kernel_ms reads), which leave out the ~5 us the two marker packets add, beside the time of the launch's binning
kernel (k_bin_tiles, on the side stream: NOT part of (d)) when it has one, and (d walk): the same colour launch from a context
created with RTC_BINNING=0, whose primary pass walks the World as k_aov's does. The planes of (c) are compared with
rtc_aov_from_hits of (e)'s records — k_trace's own — over the whole frame: every byte must agree (the `shadow` plane where the
World has one light). Prints one JSON line per World and a table.
usage: python tools/aov_cost.py [--launches 20] [--warmup 3] [--worlds ns,c3,soft]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _bootstrap import package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--worlds", default="ns,c3,soft")
args = ap.parse_args()
assert args.launches >= 20, "the median of at least 20 launches"

rtc = package()
abi = __import__("importlib").import_module(rtc.__name__ + ".abi")
scenes = __import__("importlib").import_module(rtc.__name__ + ".scenes")
W, H = 1920, 1080
NPX = W * H


def build(name):
    if name == "ns":
        return scenes.synthetic(100, W, H) + ("synthetic(100): 100 spheres + checker floor (north star)",)
    if name == "c3":
        return scenes.synthetic(10000, W, H, with_plane=False) + ("10 000 random spheres (bench.py --workload c3)",)
    if name == "soft":
        w, cam = rtc.load_yaml(path=Path(rtc.__file__).resolve().parent / "data" / "soft_shadows.yml")
        view = rtc.Matrix(list(cam.view_inv)).inverse()
        return w, rtc.camera(W, H, cam.fov, view), "data/soft_shadows.yml: 5 shapes, 4x4 area light + fill light (17 samples)"
    raise KeyError(name)


def centre_rays(cam):
    """rtc_camera_ray_for_pixel(cam, x, 0.5, y, 0.5) for the whole frame, vectorised in the header's operation order (numpy
    does not fuse); checked bit for bit against the library on a sample of pixels."""
    m = np.array(list(cam.view_inv), dtype=np.float64)
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    wx = np.broadcast_to((cam.half_width - (xs + 0.5) * cam.pixel_size)[None, :], (H, W))
    wy = np.broadcast_to((cam.half_height - (ys + 0.5) * cam.pixel_size)[:, None], (H, W))
    pix = [m[4 * r] * wx + m[4 * r + 1] * wy + m[4 * r + 2] * -1.0 + m[4 * r + 3] for r in range(3)]
    org = [m[4 * r] * 0.0 + m[4 * r + 1] * 0.0 + m[4 * r + 2] * 0.0 + m[4 * r + 3] for r in range(3)]
    d = [pix[r] - org[r] for r in range(3)]
    mag = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    rays = np.empty((H, W, 6), dtype=np.float64)
    for r in range(3):
        rays[..., r] = org[r]
        rays[..., 3 + r] = d[r] / mag
    for (x, y) in [(0, 0), (W - 1, H - 1), (959, 540), (1, 1079), (1919, 0), (777, 333), (1234, 17), (5, 999)]:
        assert rays[y, x].tobytes() == rtc.ray_for_pixel(cam, x, y).tobytes(), (x, y)
    return rays.reshape(NPX, 6)


stream = torch.cuda.Stream()
ctx = rtc.Context(0, stream=stream.cuda_stream)
os.environ["RTC_BINNING"] = "0"   # read at rtc_context_create
ctx_walk = rtc.Context(0, stream=stream.cuda_stream)
del os.environ["RTC_BINNING"]
dev = {p: torch.zeros(NPX * comps, dtype=getattr(torch, d), device="cuda:0") for p, (d, comps) in abi.AOV_PLANES.items()}
canvas = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()


def event_ms(launch, ctx=ctx):
    """median / min / max ms between two events around each of `launches` launches on the context's stream"""
    for _ in range(args.warmup):
        launch()
    ctx.synchronize()
    pairs = []
    with torch.cuda.stream(stream):
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            pairs.append((e0, e1))
    ctx.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


rows = []
for name in args.worlds.split(","):
    world, cam, desc = build(name)
    dw = ctx.upload(world)
    n_lights = rtc.lib().rtc_world_light_count(dw._h)
    ptr = {p: t.data_ptr() for p, t in dev.items()}
    r = {"world": name, "desc": desc, "frame": f"{W}x{H}", "objects": len(world), "light_samples": n_lights, "launches": args.launches}
    r["a_index_depth"] = event_ms(lambda: dw.render_aov_device(cam, {p: ptr[p] for p in ("index", "depth")}))
    r["b_no_shadow"] = event_ms(lambda: dw.render_aov_device(cam, {p: ptr[p] for p in ("index", "depth", "point", "normal", "flags")}))
    r["c_all_six"] = event_ms(lambda: dw.render_aov_device(cam, ptr))
    ctx.set_timing(1)
    r["d_colour_rows"] = event_ms(lambda: dw.render_rows(cam, 0, H, canvas.data_ptr()))
    own = sorted(float(v) for v in ctx.kernel_times_ms(args.launches))
    r["d_colour_rows_dispatch_ms"] = own[len(own) // 2]
    bins = sorted(float(v) for v in ctx.binning_times_ms(args.launches))
    r["d_binning_kernel_ms"] = bins[len(bins) // 2] if bins else 0.0
    r["d_launch"] = {k: ctx.last_launch_info()[k] for k in ("source", "binned_primary_pass")}
    dww = ctx_walk.upload(world)
    r["d_walk_colour_rows"] = event_ms(lambda: dww.render_rows(cam, 0, H, canvas.data_ptr()), ctx_walk)
    assert not ctx_walk.last_launch_info()["binned_primary_pass"]
    dww.close()
    # (c) + the copy of the planes to the host: rtc_render_aov, wall time
    wall = []
    for _ in range(args.warmup + 5):
        t = time.perf_counter()
        planes = dw.render_aov(cam)
        wall.append((time.perf_counter() - t) * 1e3)
    wall = sorted(wall[args.warmup:])
    r["c_plus_copy_wall_ms"] = wall[len(wall) // 2]
    r["plane_bytes"] = int(sum(a.nbytes for a in planes.values()))
    # (e) rtc_color_at over the same rays with hit records: once
    rays = centre_rays(cam)
    rgb = np.empty((NPX, 3), dtype=np.float64)
    hits = (rtc.RtcHit * NPX)()
    P = C.POINTER(C.c_double)
    ctx.synchronize()
    t = time.perf_counter()
    st = rtc.lib().rtc_color_at(ctx._h, dw._h, rays.ctypes.data_as(P), NPX, 5, 0, rgb.ctypes.data_as(P), hits)
    r["e_color_at_wall_ms"] = (time.perf_counter() - t) * 1e3
    assert st == 0, st
    r["e_bytes"] = NPX * (48 + 24 + 184)
    r["e_over_c_plus_copy"] = r["e_color_at_wall_ms"] / r["c_plus_copy_wall_ms"]
    r["a_over_d"] = r["a_index_depth"]["median_ms"] / r["d_colour_rows"]["median_ms"]
    r["a_over_d_walk"] = r["a_index_depth"]["median_ms"] / r["d_walk_colour_rows"]["median_ms"]
    # the whole frame against k_trace's own records
    want = rtc.aov_from_hits(hits, W, H)
    compare = [p for p in abi.AOV_PLANES if p != "shadow" or n_lights == 1]
    r["planes_equal_color_at_records"] = {p: bool(np.array_equal(planes[p], want[p])) for p in compare}
    r["hit_pixels"] = int((planes["index"] >= 0).sum())
    r["shadowed_pixels"] = int((planes["shadow"] > 0).sum())
    del hits, want, rays, rgb, planes
    dw.close()
    rows.append(r)
    print(json.dumps(r), flush=True)
ctx_walk.close()
ctx.close()

print()
print("| world | (a) index+depth | (b) no shadow | (c) all six | (d) colour launch | (d) dispatch | (d) binning kernel | (d walk) colour launch, RTC_BINNING=0 | (c)+copy, wall | (e) rtc_color_at, wall | (e) / ((c)+copy) | (a) / (d) |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    print(f"| {r['world']} ({r['objects']} objects, {r['light_samples']} light samples) | {r['a_index_depth']['median_ms']:.4f} ms | {r['b_no_shadow']['median_ms']:.4f} ms | "
          f"{r['c_all_six']['median_ms']:.4f} ms | {r['d_colour_rows']['median_ms']:.4f} ms | {r['d_colour_rows_dispatch_ms']:.4f} ms | "
          f"{r['d_binning_kernel_ms']:.4f} ms | {r['d_walk_colour_rows']['median_ms']:.4f} ms | {r['c_plus_copy_wall_ms']:.1f} ms | {r['e_color_at_wall_ms']:.1f} ms | {r['e_over_c_plus_copy']:.1f}x | {r['a_over_d']:.2f} |")
ok = all(r["e_color_at_wall_ms"] > r["c_plus_copy_wall_ms"] and all(r["planes_equal_color_at_records"].values()) for r in rows)
print("\n(c)+copy faster than (e) on every World, planes equal to rtc_color_at's records:", ok)
sys.exit(0 if ok else 1)
