"""What the ambient-occlusion pass costs (include/rtc.h "ambient occlusion"), at 1920x1080, on two Worlds: synthetic(100) — the
north star — and the 10 000 spheres of `bench.py --workload c3`; at 4 (2x2), 16 (4x4) and 64 (8x8) samples, radius 1.0 and +inf.
Per point:
  (k) k_ao's kernel time: the median of --launches launches (after --warmup) between two HIP events recorded around each launch
      on the context's stream (the method of tools/aov_cost.py). A point whose first launch takes more than --slow-ms is timed
      over --slow-launches launches instead, and says so.
  (p) the route the library offered before: rtc_render_aov of `point` + `normal` into host memory, then rtc_color_at, with hit
      records, over the same rays from host memory, one call of 2 073 600 rays per sample. Wall time of the library calls
      alone: building the rays on the host (numpy here) is NOT counted. Up to --route-samples sample passes are run; for more
      samples the measured per-pass mean is multiplied up, and the row says how many passes were run.
  (six) k_aov's six-plane launch of the same World and camera, kernel time by the same events: a scale.
The 4-sample plane of (k) is compared with the counts of (p) over the whole frame: every pixel must agree.
Prints one JSON line per point and a table; exits non-zero unless (k) is faster than (p) at every point and the planes agree.
usage: python tools/ao_cost.py [--launches 20] [--warmup 3] [--worlds ns,c3]"""
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
abi = __import__("importlib").import_module(rtc.__name__ + ".abi")
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
plane_dev = torch.zeros(NPX, dtype=torch.int16, device="cuda:0")
aov_dev = {p: torch.zeros(NPX * comps, dtype=getattr(torch, d), device="cuda:0") for p, (d, comps) in abi.AOV_PLANES.items()}
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
    ptr = {p: t.data_ptr() for p, t in aov_dev.items()}
    six = event_ms(lambda: dw.render_aov_device(cam, ptr))
    # the first leg of the parent's route, once per World: the point and normal planes into host memory (wall, median of 5)
    wall = []
    for _ in range(args.warmup + 5):
        t0 = time.perf_counter()
        planes = dw.render_aov(cam, ("point", "normal", "index"))
        wall.append((time.perf_counter() - t0) * 1e3)
    aov_wall = sorted(wall[args.warmup:])[2]
    hit = planes["index"].reshape(-1) >= 0
    normal, point = planes["normal"].reshape(-1, 3)[hit], planes["point"].reshape(-1, 3)[hit]
    over = point + normal * 0.00000001   # compute_vectors: point.add(normal.mul(EPSILON))
    nrays = int(hit.sum())
    for radius in RADII:
        for us, vs in GRIDS:
            n = us * vs
            ao = rtc.ao(radius, us, vs)
            r = {"world": name, "desc": desc, "frame": f"{W}x{H}", "objects": len(world), "samples": n, "radius": "inf" if radius == math.inf else radius,
                 "hit_pixels": nrays, "six_plane_aov_ms": six["median_ms"]}
            r["k_ao"] = event_ms(lambda: dw.render_ao_device(cam, ao, plane_dev.data_ptr()))
            dirs = rtc.ao_expand(ao)
            passes = min(n, args.route_samples)
            counts = np.zeros(nrays, dtype=np.uint16)
            route = 0.0
            for k in range(passes):
                rays = sample_rays(normal, over, dirs[k])   # (not timed)
                ctx.synchronize()
                t0 = time.perf_counter()
                _, hits = dw.color_at(rays, remaining=0, want_hits=True)
                route += (time.perf_counter() - t0) * 1e3
                rec = np.frombuffer(hits, dtype=HIT_DTYPE)[:nrays]
                counts += ((rec["hit_index"] >= 0) & (rec["t"] < radius)).astype(np.uint16)
                del hits, rec, rays
            r["route_passes_run"] = passes
            r["route_color_at_ms_per_pass"] = route / passes
            r["route_aov_point_normal_wall_ms"] = aov_wall
            r["route_total_ms"] = aov_wall + n * (route / passes)
            r["route_over_k_ao"] = r["route_total_ms"] / r["k_ao"]["median_ms"]
            r["k_ao_over_six_plane_aov"] = r["k_ao"]["median_ms"] / six["median_ms"]
            if passes == n:   # the whole frame against the route's own counts
                got = dw.render_ao(cam, ao).reshape(-1)
                want = np.zeros(NPX, dtype=np.uint16)
                want[hit] = counts
                r["plane_equals_route"] = bool(np.array_equal(got, want))
                r["occluded_pixels"] = int((got > 0).sum())
            rows.append(r)
            print(json.dumps(r), flush=True)
    dw.close()
ctx.close()

print()
print("| world | samples | radius | (k) k_ao, kernel | launches | (p) parent's route, wall | passes run | (p) / (k) | (six) k_aov six planes | (k) / (six) | plane == route |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    print(f"| {r['world']} ({r['objects']} objects) | {r['samples']} | {r['radius']} | {r['k_ao']['median_ms']:.3f} ms | {r['k_ao']['launches']} | {r['route_total_ms']:.1f} ms | "
          f"{r['route_passes_run']} | {r['route_over_k_ao']:.0f}x | {r['six_plane_aov_ms']:.4f} ms | {r['k_ao_over_six_plane_aov']:.1f} | {r.get('plane_equals_route', '-')} |")
ok = all(r["route_total_ms"] > r["k_ao"]["median_ms"] and r.get("plane_equals_route", True) for r in rows)
print("\n(k) faster than (p) at every point, 4-sample planes equal to the route's counts:", ok)
sys.exit(0 if ok else 1)
