"""What edge-adaptive anti-aliasing costs (include/rtc.h "edge-adaptive anti-aliasing"), at 1920x1080, on two Worlds: synthetic(100)
— the north star — and the 10 000 spheres of `bench.py --workload c3`.

Frames (default mode). Per World the configurations
    one       the one-sample frame, rtc_render_rows into a device canvas
    samples4  the same with cam.samples = 4 (four fixed sub-samples per pixel, no resample)
    aa2x2     rtc_render_adaptive_device, 2 x 2, threshold 0.01
    aa4x4     ... 4 x 4, threshold 0.01
    aa-inf    ... 2 x 2, threshold +inf: nothing is refined — the fixed cost: mask + scan + the one wait for the stream
are measured INTERLEAVED: every round times each (World, configuration) once, between two HIP events recorded around the call on
the context's stream, and the host's clock around the same call up to the end of the stream. An adaptive call waits for the
stream once in its middle, so its event time includes that round trip: it is the frame's time, not a sum of kernel times. After
--warmup rounds, the median, least and greatest of --rounds rounds are reported, with the refined fraction and the launch count.

Stages (--stage WORLD,USTEPS,VSTEPS). --rounds adaptive frames of one World and one spec and nothing else, to be run under
`rocprofv3 --kernel-trace --stats`: the profiler's per-kernel averages are the stage times. --stage-report DIR... reads the
kernel_stats.csv files such runs left and prints one table (mask, scan, list, rays, probe, resolve, and the base frame's kernels).

Prints one JSON line per point and a table.
usage: python tools/adaptive_cost.py [--rounds 20] [--warmup 3] [--worlds ns,c3]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/adaptive_cost.py --stage ns,4,4
       python tools/adaptive_cost.py --stage-report DIR [DIR ...]"""
import argparse
import csv
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--worlds", default="ns,c3")
ap.add_argument("--stage", default=None)
ap.add_argument("--stage-report", nargs="+", default=None)
args = ap.parse_args()

STAGES = (("k_aa_mask", "mask"), ("k_aa_scan", "scan"), ("k_aa_list", "list"), ("k_aa_rays", "rays"), ("k_aa_resolve", "resolve"))

if args.stage_report:
    print("| run | kernel | calls | average | total |")
    print("|---|---|---|---|---|")
    for d in args.stage_report:
        for path in sorted(Path(d).rglob("*kernel_stats.csv")):
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Name"]
                    tag = next((t for k, t in STAGES if k in name), None)
                    if tag is None and "k_trace" in name:
                        # k_trace<SRC, refl, refr, probe, ...>: the fourth argument says whether it traced the refinement rays
                        targs = name.split("k_trace<")[1].split(">")[0].split(", ")
                        tag = ("probe " if targs[3] == "true" else "base frame ") + "k_trace<" + ",".join(targs) + ">"
                    if tag is None:
                        tag = "(other) " + name.split("(")[0][:40]
                    print(f"| {Path(d).name} | {tag} | {row['Calls']} | {float(row['AverageNs']) / 1e6:.4f} ms | {float(row['TotalDurationNs']) / 1e6:.3f} ms |")
    sys.exit(0)

import torch  # noqa: E402
from _bootstrap import package  # noqa: E402

rtc = package()
scenes = __import__("importlib").import_module(rtc.__name__ + ".scenes")
W, H = 1920, 1080
NPX = W * H


def build(name):
    if name == "ns":
        return scenes.synthetic(100, W, H) + ("synthetic(100): 100 spheres + checker floor (north star)",)
    if name == "c3":
        return scenes.synthetic(10000, W, H, with_plane=False) + ("10 000 random spheres (bench.py --workload c3)",)
    raise KeyError(name)


stream = torch.cuda.Stream()
ctx = rtc.Context(0, stream=stream.cuda_stream)
canvas = torch.zeros(NPX * 3, dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()

if args.stage:
    name, us, vs = args.stage.split(",")
    world, cam, _ = build(name)
    dw = ctx.upload(world)
    spec = rtc.adaptive(0.01, int(us), int(vs))
    for _ in range(args.warmup + args.rounds):
        info = dw.render_adaptive_device(cam, spec, canvas.data_ptr())
        ctx.synchronize()
    print(json.dumps({"world": name, "spec": f"{us}x{vs}", "frames": args.warmup + args.rounds, **info, "refined_fraction": info["pixels_refined"] / NPX}))
    dw.close()
    ctx.close()
    sys.exit(0)

assert args.rounds >= 20, "the median of at least 20 rounds"
points = []   # (world name, configuration, launch() -> info or None)
keep = []
for name in args.worlds.split(","):
    world, cam, desc = build(name)
    dw = ctx.upload(world)
    cam4 = type(cam).from_buffer_copy(cam)
    cam4.samples = 4
    keep.append((world, dw, cam, cam4))
    points.append((name, desc, len(world), "one", lambda dw=dw, cam=cam: dw.render_rows(cam, 0, H, canvas.data_ptr())))
    points.append((name, desc, len(world), "samples4", lambda dw=dw, cam4=cam4: dw.render_rows(cam4, 0, H, canvas.data_ptr())))
    for tag, spec in (("aa2x2", rtc.adaptive(0.01, 2, 2)), ("aa4x4", rtc.adaptive(0.01, 4, 4)), ("aa-inf", rtc.adaptive(math.inf, 2, 2))):
        points.append((name, desc, len(world), tag, lambda dw=dw, cam=cam, spec=spec: dw.render_adaptive_device(cam, spec, canvas.data_ptr())))

samples = {(p[0], p[3]): {"event_ms": [], "host_ms": [], "info": None} for p in points}
for rnd in range(args.warmup + args.rounds):
    for name, desc, nobj, tag, launch in points:
        ctx.synchronize()
        with torch.cuda.stream(stream):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            info = launch()
            e1.record(stream)
        ctx.synchronize()
        t1 = time.perf_counter()
        if rnd >= args.warmup:
            s = samples[(name, tag)]
            s["event_ms"].append(e0.elapsed_time(e1))
            s["host_ms"].append((t1 - t0) * 1e3)
            s["info"] = info if isinstance(info, dict) else None

rows = []
for name, desc, nobj, tag, _ in points:
    s = samples[(name, tag)]
    ev, host = sorted(s["event_ms"]), sorted(s["host_ms"])
    r = {"world": name, "desc": desc, "objects": nobj, "frame": f"{W}x{H}", "config": tag, "rounds": len(ev), "median_ms": ev[len(ev) // 2], "min_ms": ev[0],
         "max_ms": ev[-1], "host_median_ms": host[len(host) // 2], "host_min_ms": host[0], "host_max_ms": host[-1]}
    if s["info"]:
        r.update(s["info"])
        r["refined_fraction"] = s["info"]["pixels_refined"] / NPX
    rows.append(r)
    print(json.dumps(r), flush=True)
for _, dw, _, _ in keep:
    dw.close()
ctx.close()

print()
print("| world | frame | events, median (least .. greatest) | host clock, median | refined pixels | rays | launches |")
print("|---|---|---|---|---|---|---|")
for r in rows:
    extra = f"{r['pixels_refined']} ({100 * r['refined_fraction']:.1f} %) | {r['rays_refined']} | {r['launches']}" if "launches" in r else " | | "
    print(f"| {r['world']} ({r['objects']} objects) | {r['config']} | {r['median_ms']:.3f} ms ({r['min_ms']:.3f} .. {r['max_ms']:.3f}) | {r['host_median_ms']:.3f} ms | {extra} |")
print()
for name in args.worlds.split(","):
    t = {r["config"]: r for r in rows if r["world"] == name}
    one, s4 = t["one"]["median_ms"], t["samples4"]["median_ms"]
    render_ray_ns = s4 / (4 * NPX) * 1e6
    for tag in ("aa2x2", "aa4x4"):
        a = t[tag]
        per_ray_ns = (a["median_ms"] - t["aa-inf"]["median_ms"]) / max(1, a["rays_refined"]) * 1e6
        print(f"{name} {tag}: {a['median_ms']:.3f} ms against one-sample {one:.3f} ms and samples=4 {s4:.3f} ms; fixed cost (aa-inf minus one) "
              f"{t['aa-inf']['median_ms'] - one:.3f} ms; per refinement ray {per_ray_ns:.3f} ns against {render_ray_ns:.3f} ns per ray of the samples=4 frame: "
              f"ratio {per_ray_ns / render_ray_ns:.2f}")
