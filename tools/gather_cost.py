"""What the one-bounce gather pass costs (include/rtc.h "colour bleeding"), at 1920x1080, on two Worlds: synthetic(100) — the
north star — and the 10 000 spheres of `bench.py --workload c3`; at 4 (2x2), 16 (4x4) and 64 (8x8) samples, radius 1.0 and +inf.
Per point:
  (k) k_gather's kernel time, `radiance` alone: the median of --launches launches (after --warmup) between two HIP events
      recorded around each launch on the context's stream (the method of tools/ao_cost.py). A point whose first launch takes
      more than --slow-ms is timed over --slow-launches launches instead, and says so.
  (b) the same with `bounce` asked for as well.
  (ao) k_ao's kernel time for the same pass, by the same events: what asking "anything there?" costs where the gather asks
      "what, and how is it lit?".
  (p) the route the library offered before: rtc_render_aov of `point` + `normal` into host memory, then rtc_color_at(remaining
      0), with hit records, over the same rays from host memory, one call of up to 2 073 600 rays per sample, then the mean on
      the host (rtc_gather_from_hits). Wall time of the library calls alone: building the rays on the host (numpy here) is
      NOT counted. Up to --route-samples sample passes are run; for more samples the measured per-pass mean is multiplied up,
      and the row says how many passes were run.
The 4-sample radiance of (k) is compared with the route's over the whole frame: every byte must agree.
Prints one JSON line per point and a table; exits non-zero unless (k) is faster than (p) at every point and the planes agree.
usage: python tools/gather_cost.py [--launches 20] [--warmup 3] [--worlds ns,c3]"""
import argparse
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
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--slow-ms", type=float, default=150.0)
ap.add_argument("--slow-launches", type=int, default=5)
ap.add_argument("--route-samples", type=int, default=4)
ap.add_argument("--worlds", default="ns,c3")
args = ap.parse_args()
assert args.launches >= 20, "the median of at least 20 launches"

rtc = package()
scenes = __import__("importlib").import_module(rtc.__name__ + ".scenes")
W, H = 1920, 1080
NPX = W * H
GRIDS = ((2, 2), (4, 4), (8, 8))
RADII = (1.0, math.inf)
HIT_DTYPE = np.dtype([("hit_index", "<i4"), ("inside", "<u4"), ("shadowed", "<u4"), ("_pad", "<u4"), ("t", "<f8"), ("point", "<f8", 3),
                      ("over_point", "<f8", 3), ("under_point", "<f8", 3), ("eyev", "<f8", 3), ("normal", "<f8", 3), ("reflectv", "<f8", 3),
                      ("n1", "<f8"), ("n2", "<f8")])


def build(name):
    if name == "ns":
        return scenes.synthetic(100, W, H) + ("synthetic(100): 100 spheres + checker floor (north star)",)
    if name == "c3":
        return scenes.synthetic(10000, W, H, with_plane=False) + ("10 000 random spheres (bench.py --workload c3)",)
    raise KeyError(name)


stream = torch.cuda.Stream()
ctx = rtc.Context(0, stream=stream.cuda_stream)
rad_dev = torch.zeros(NPX * 3, dtype=torch.float64, device="cuda:0")
bounce_dev = torch.zeros(NPX * 3, dtype=torch.float64, device="cuda:0")
ao_dev = torch.zeros(NPX, dtype=torch.int16, device="cuda:0")
torch.cuda.synchronize()


def event_ms(launch):
    """median / min / max ms between two events around each launch on the context's stream"""
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
    ctx.synchronize()
    first = e0.elapsed_time(e1)
    slow = first > args.slow_ms
    warm, n = (0, args.slow_launches) if slow else (args.warmup, args.launches)
    for _ in range(warm):
        launch()
    ctx.synchronize()
    pairs = []
    with torch.cuda.stream(stream):
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            pairs.append((e0, e1))
    ctx.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "launches": n, "first_ms": first}


def sample_rays(normal, over, local):
    """rtc_ao_ray over every pixel that hits, vectorised in the header's operation order (numpy does not fuse)."""
    nx, ny, nz = normal[:, 0], normal[:, 1], normal[:, 2]
    sign = np.copysign(1.0, nz)
    a = -1.0 / (sign + nz)
    b = (nx * ny) * a
    t = np.stack([1.0 + ((sign * nx) * nx) * a, sign * b, -(sign * nx)], axis=1)
    s = np.stack([b, sign + ((ny * ny) * a), -ny], axis=1)
    return np.concatenate([over, ((t * local[0]) + (s * local[1])) + (normal * local[2])], axis=1)


rows = []
for name in args.worlds.split(","):
    world, cam, desc = build(name)
    dw = ctx.upload(world)
    # the first leg of the earlier route, once per World: the point and normal planes into host memory (wall, median of 5)
    wall = []
    for _ in range(args.warmup + 5):
        t0 = time.perf_counter()
        planes = dw.render_aov(cam, ("point", "normal", "index"))
        wall.append((time.perf_counter() - t0) * 1e3)
    aov_wall = sorted(wall[args.warmup:])[2]
    index = planes["index"].reshape(-1)
    hit = index >= 0
    normal, point = planes["normal"].reshape(-1, 3)[hit], planes["point"].reshape(-1, 3)[hit]
    over = point + normal * 0.00000001   # compute_vectors: point.add(normal.mul(EPSILON))
    nrays = int(hit.sum())
    primary = np.zeros(NPX, dtype=HIT_DTYPE)
    primary["hit_index"] = index
    max_passes = min(min(us * vs for us, vs in GRIDS), args.route_samples)   # (every point runs this many: the buffers are made once)
    recs = np.zeros((NPX, max_passes), dtype=HIT_DTYPE)   # pixels that miss keep hit_index -1; the others are rewritten per point
    recs["hit_index"] = -1
    rgb = np.zeros((NPX, max_passes, 3))
    for radius in RADII:
        for us, vs in GRIDS:
            n = us * vs
            ao = rtc.ao(radius, us, vs)
            r = {"world": name, "desc": desc, "frame": f"{W}x{H}", "objects": len(world), "samples": n, "radius": "inf" if radius == math.inf else radius,
                 "hit_pixels": nrays}
            r["k_gather"] = event_ms(lambda: dw.render_gather_device(cam, ao, {"radiance": rad_dev.data_ptr()}))
            r["k_gather_bounce"] = event_ms(lambda: dw.render_gather_device(cam, ao, {"radiance": rad_dev.data_ptr(), "bounce": bounce_dev.data_ptr()}))
            r["k_ao"] = event_ms(lambda: dw.render_ao_device(cam, ao, ao_dev.data_ptr()))
            dirs = rtc.ao_expand(ao)
            passes = max_passes
            route = 0.0
            for k in range(passes):
                rays = sample_rays(normal, over, dirs[k])   # (not timed)
                ctx.synchronize()
                t0 = time.perf_counter()
                col, hits = dw.color_at(rays, remaining=0, want_hits=True)
                route += (time.perf_counter() - t0) * 1e3
                recs[hit, k] = np.frombuffer(hits, dtype=HIT_DTYPE)[:nrays]
                rgb[hit, k] = col
                del hits, rays, col
            flat = recs.reshape(-1)
            t0 = time.perf_counter()
            want = rtc.gather_from_hits((rtc.RtcHit * NPX).from_buffer(primary), (rtc.RtcHit * flat.size).from_buffer(flat), rgb, None, passes,
                                        radius, W, H, planes=("radiance",))["radiance"]
            mean_ms = (time.perf_counter() - t0) * 1e3
            r["route_passes_run"] = passes
            r["route_color_at_ms_per_pass"] = route / passes
            r["route_aov_point_normal_wall_ms"] = aov_wall
            r["route_host_mean_ms_per_pass"] = mean_ms / passes
            r["route_total_ms"] = aov_wall + n * (route / passes) + n * (mean_ms / passes)
            r["route_over_k_gather"] = r["route_total_ms"] / r["k_gather"]["median_ms"]
            r["k_gather_over_k_ao"] = r["k_gather"]["median_ms"] / r["k_ao"]["median_ms"]
            if passes == n:   # the whole frame against the route's own radiance
                got = dw.render_gather(cam, ao, planes=("radiance",))["radiance"]
                r["radiance_equals_route"] = bool(got.tobytes() == want.tobytes())
                r["lit_pixels"] = int(got.reshape(-1, 3).any(axis=1).sum())
            del flat, want
            rows.append(r)
            print(json.dumps(r), flush=True)
    dw.close()
ctx.close()

print()
print("| world | samples | radius | (k) k_gather, kernel | (b) with bounce | launches | (ao) k_ao, kernel | (k) / (ao) | (p) earlier route, wall | passes run | (p) / (k) | radiance == route |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    print(f"| {r['world']} ({r['objects']} objects) | {r['samples']} | {r['radius']} | {r['k_gather']['median_ms']:.3f} ms | {r['k_gather_bounce']['median_ms']:.3f} ms | "
          f"{r['k_gather']['launches']} | {r['k_ao']['median_ms']:.3f} ms | {r['k_gather_over_k_ao']:.1f} | {r['route_total_ms']:.1f} ms | {r['route_passes_run']} | "
          f"{r['route_over_k_gather']:.0f}x | {r.get('radiance_equals_route', '-')} |")
ok = all(r["route_total_ms"] > r["k_gather"]["median_ms"] and r.get("radiance_equals_route", True) for r in rows)
print("\n(k) faster than (p) at every point, 4-sample radiance equal to the route's bytes:", ok)
sys.exit(0 if ok else 1)
