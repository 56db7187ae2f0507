"""What the edge-aware filter costs (include/rtc.h "edge-aware filter"), at 1920x1080, on two Worlds: synthetic(100) — the north
star — and the 10 000 spheres of `bench.py --workload c3`; so that "16 samples + filter" can be read against "64 samples".
Per World, in one run:
  (ao)  k_ao's kernel time at 4 (2x2), 16 (4x4) and 64 (8x8) samples, radius 1.0: the median of --launches launches (after
        --warmup) between two HIP events recorded around each launch on the context's stream (the method of tools/ao_cost.py).
        A point whose first launch takes more than --slow-ms is timed over --slow-launches launches instead.
  (f)   rtc_plane_filter_device under the World's own guides (k_aov's index, point and normal planes), for 1 channel (the
        4x4-sample occlusion fraction) and 3 channels (the 4x4-sample bounce plane), plane_sigma 0.05, normal_squarings 3,
        RTC_FILTER_SAME_OBJECT, with passes = 1..5, by the same events. A call of k passes is k launches of k_atrous with steps
        1, 2, ..., 2^(k-1); the time of the pass with step 2^(k-1) is reported as median(k passes) - median(k-1 passes).
  Per pass, from counts kept here (no counter is read):
        operations per pixel that hits = 25 taps x (18 + normal_squarings + 2*channels) f64 adds, subtractions and products
        (3 differences, two 3-term dot products, the plane weight's product and difference, the squarings, h*wz and *m, one
        product and one sum per channel, wsum's sum) + channels divisions counted as one each; against 39.3 T f64 instructions/s
        (the f64 vector peak of 78.6 TFLOP/s counts a fused multiply-add as two; this library never fuses);
        bytes per pixel = 52 + 8*channels read + 8*channels written (every guide and value once: the halo's re-reads come from
        the caches); against 8.0 TB/s.
        The share of peak is the larger of the two least times over the measured time, and the row says which one binds.
Prints one JSON line per point and two tables.
usage: python tools/filter_cost.py [--launches 20] [--warmup 3] [--worlds ns,c3]"""
import argparse
import json
import sys
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
ap.add_argument("--worlds", default="ns,c3")
args = ap.parse_args()
assert args.launches >= 20, "the median of at least 20 launches"

rtc = package()
scenes = __import__("importlib").import_module(rtc.__name__ + ".scenes")
W, H = 1920, 1080
NPX = W * H
PEAK_F64_INSTR, PEAK_HBM = 39.3e12, 8.0e12
SIGMA, SQUARINGS = 0.05, 3


def build(name):
    if name == "ns":
        return scenes.synthetic(100, W, H) + ("synthetic(100): 100 spheres + checker floor (north star)",)
    if name == "c3":
        return scenes.synthetic(10000, W, H, with_plane=False) + ("10 000 random spheres (bench.py --workload c3)",)
    raise KeyError(name)


stream = torch.cuda.Stream()
ctx = rtc.Context(0, stream=stream.cuda_stream)
f64 = dict(dtype=torch.float64, device="cuda:0")
index = torch.zeros(NPX, dtype=torch.int32, device="cuda:0")
point, normal, bounce, out3 = (torch.zeros(NPX * 3, **f64) for _ in range(4))
counts = torch.zeros(NPX, dtype=torch.int16, device="cuda:0")
occ, out1 = (torch.zeros(NPX, **f64) for _ in range(2))
torch.cuda.synchronize()
guides = {"index": index.data_ptr(), "point": point.data_ptr(), "normal": normal.data_ptr()}


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


ao_rows, pass_rows = [], []
for name in args.worlds.split(","):
    world, cam, desc = build(name)
    dw = ctx.upload(world)
    for us, vs in ((2, 2), (4, 4), (8, 8)):
        fan = rtc.ao(1.0, us, vs)
        r = {"world": name, "desc": desc, "frame": f"{W}x{H}", "objects": len(world), "kernel": "k_ao", "samples": us * vs,
             **event_ms(lambda: dw.render_ao_device(cam, fan, counts.data_ptr()))}
        ao_rows.append(r)
        print(json.dumps(r), flush=True)
    # the planes the filter is timed on: the World's guides, its 4x4-sample occlusion fraction and bounce plane
    fan = rtc.ao(1.0, 4, 4)
    dw.render_aov_device(cam, guides)
    dw.render_ao_device(cam, fan, counts.data_ptr())
    dw.render_gather_device(cam, fan, {"bounce": bounce.data_ptr()})
    ctx.counts_to_fraction_device(counts.data_ptr(), 16, W, H, occ.data_ptr())
    ctx.synchronize()
    hits = int((index.cpu().numpy() >= 0).sum())
    for ch, src, dst in ((1, occ, out1), (3, bounce, out3)):
        previous = 0.0
        for passes in range(1, 6):
            flt = rtc.filter_spec(SIGMA, passes=passes, normal_squarings=SQUARINGS, same_object=True)
            t = event_ms(lambda: ctx.plane_filter_device(src.data_ptr(), ch, guides, W, H, flt, dst.data_ptr()))
            ms = t["median_ms"] - previous
            previous = t["median_ms"]
            ops = hits * (25 * (18 + SQUARINGS + 2 * ch) + ch)
            nbytes = NPX * (52 + 16 * ch)
            t_ops, t_bytes = ops / PEAK_F64_INSTR * 1e3, nbytes / PEAK_HBM * 1e3
            r = {"world": name, "kernel": "k_atrous", "channels": ch, "step": 1 << (passes - 1), "pass_ms": ms, "call_of_k_passes": t, "hit_pixels": hits,
                 "f64_instructions": ops, "bytes": nbytes, "f64_instr_per_s": ops / (ms * 1e-3), "bytes_per_s": nbytes / (ms * 1e-3),
                 "fraction_of_f64_valu_peak": t_ops / ms, "fraction_of_hbm_peak": t_bytes / ms, "bound_by": "f64 VALU" if t_ops >= t_bytes else "HBM",
                 "share_of_peak": max(t_ops, t_bytes) / ms}
            pass_rows.append(r)
            print(json.dumps(r), flush=True)
    dw.close()
ctx.close()

print()
print("| world | k_ao samples | kernel time | launches |")
print("|---|---|---|---|")
for r in ao_rows:
    print(f"| {r['world']} ({r['objects']} objects) | {r['samples']} | {r['median_ms']:.3f} ms | {r['launches']} |")
print()
print("| world | channels | step | pass, kernel time | calls of k passes | of the f64 VALU peak | of the HBM peak | bound by | share of peak |")
print("|---|---|---|---|---|---|---|---|---|")
for r in pass_rows:
    print(f"| {r['world']} | {r['channels']} | {r['step']} | {r['pass_ms']:.4f} ms | {r['call_of_k_passes']['median_ms']:.4f} ms | {r['fraction_of_f64_valu_peak']:.3f} | "
          f"{r['fraction_of_hbm_peak']:.3f} | {r['bound_by']} | {r['share_of_peak']:.3f} |")
print()
for name in args.worlds.split(","):
    ao = {r["samples"]: r["median_ms"] for r in ao_rows if r["world"] == name}
    two = [r for r in pass_rows if r["world"] == name and r["channels"] == 1 and r["step"] == 2][0]["call_of_k_passes"]["median_ms"]
    print(f"{name}: 16 samples + the default two passes = {ao[16]:.3f} + {two:.3f} = {ao[16] + two:.3f} ms; 64 samples = {ao[64]:.3f} ms")
