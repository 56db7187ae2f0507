"""What the resize costs on the device (include/rtc.h "resizing f64 canvases"): 3840x2160 -> 1920x1080, 1920x1080 -> 256x144 and
480x270 -> 1920x1080 with BOX, CATMULL_ROM and LANCZOS3, on frames of random values. In one run, each point the median of
--launches calls (after --warmup) between two HIP events recorded around the call on the context's stream (the method of
tools/post_cost.py); the tables are cached by the warm-up, so no timed call uploads or waits.
Per point, from counts kept here (no counter is read):
        HBM bytes: k_resize_h reads 24 per source pixel and writes 24 per pixel of the intermediate w_out x h_in frame, k_resize_v
        reads that frame and writes 24 per output pixel; the tables (a few hundred KB at most) are left out; against 8.0 TB/s.
        A frame that fits the Infinity Cache (256 MB) is not a pure HBM figure: the 3840x2160 frame is 199 MB and its intermediate
        100 MB, the other frames are far below it, so the vertical pass mostly reads what the horizontal pass just wrote.
  (h)  the route the library offered before: rtc_render of the north-star World at the supersampled size into a page-locked host
        canvas, then rtc_canvas_resize on the host; wall time, the median of three runs per step; against the same frame rendered
        into device memory and resized there (events).
  (p)  data/supersampled_panorama.yml end to end on the device: the 3x frame traced and resized to 1x, against the 1x frame traced
        directly (one ray per pixel, no anti-aliasing), events around both.
Prints one JSON line per point and a table. The points are CALL times: the two dependent launches include the gap between them.
For the time of each kernel, run the tool under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/resize_cost.py
--no-host-route` in a run of its own and hand the trace to a second, GPU-less invocation: `python tools/resize_cost.py --kernel-times
DIR/.../*_kernel_trace.csv`; the dispatches of k_resize_h and k_resize_v are then split by point in the order they were made
(--warmup + --launches per point; the same values must be given to both invocations).
usage: python tools/resize_cost.py [--launches 20] [--warmup 3] [--no-host-route] [--kernel-times TRACE.csv]"""
import argparse
import csv
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-host-route", action="store_true")
ap.add_argument("--kernel-times", default=None)
args = ap.parse_args()
assert args.launches >= 20, "the median of at least 20 launches"

SHAPES = [(3840, 2160, 1920, 1080), (1920, 1080, 256, 144), (480, 270, 1920, 1080)]
FILTERS = ["box", "catmull-rom", "lanczos3"]
POINTS = [(s, f) for s in SHAPES for f in FILTERS]
PEAK_HBM = 8.0e12


def pass_bytes(shape):
    w_in, h_in, w_out, h_out = shape
    return 24 * (w_in * h_in + w_out * h_in), 24 * (w_out * h_in + w_out * h_out)


def label(shape, name):
    return f"{shape[0]}x{shape[1]} -> {shape[2]}x{shape[3]}, {name}"


if args.kernel_times:   # no GPU: the kernel trace of an earlier run, split by point
    per = args.warmup + args.launches
    spans = {"k_resize_h": [], "k_resize_v": []}
    with open(args.kernel_times, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        for k in spans:
            if k in r["Kernel_Name"]:
                spans[k].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    for k, v in spans.items():
        assert len(v) == per * len(POINTS), f"{k}: {len(v)} dispatches in the trace, {per * len(POINTS)} expected (--warmup / --launches as in the traced run, with --no-host-route)"
    print("| point | k_resize_h median (min .. max) | of the HBM peak | k_resize_v median (min .. max) | of the HBM peak |")
    print("|---|---|---|---|---|")
    for i, (shape, name) in enumerate(POINTS):
        cells = []
        for k, nbytes in zip(("k_resize_h", "k_resize_v"), pass_bytes(shape)):
            ns = sorted(spans[k][i * per + args.warmup:(i + 1) * per])
            med = ns[len(ns) // 2]
            cells.append(f"{med / 1e3:.1f} us ({ns[0] / 1e3:.1f} .. {ns[-1] / 1e3:.1f}) | {nbytes / PEAK_HBM / (med * 1e-9):.3f}")
        print(f"| {label(shape, name)} | {cells[0]} | {cells[1]} |")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _bootstrap import package  # noqa: E402

rtc = package()
stream = torch.cuda.Stream()
ctx = rtc.Context(0, stream=stream.cuda_stream)
f64 = dict(dtype=torch.float64, device="cuda:0")


def event_ms(launch):
    """median / min / max ms between two events around each call on the context's stream"""
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
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "launches": args.launches}


rows = []
rng = np.random.default_rng(1)
for shape in SHAPES:
    w_in, h_in, w_out, h_out = shape
    src = torch.from_numpy(rng.uniform(0.0, 2.0, size=w_in * h_in * 3)).to("cuda:0")
    dst = torch.zeros(w_out * h_out * 3, **f64)
    torch.cuda.synchronize()
    for name in FILTERS:
        spec = rtc.resize_spec(name)
        r = {"point": label(shape, name), **event_ms(lambda: ctx.resize_device(src.data_ptr(), w_in, h_in, spec, dst.data_ptr(), w_out, h_out))}
        hb, vb = pass_bytes(shape)
        r.update({"taps_h": int(rtc.lib().rtc_resize_taps(w_in, w_out, spec.filter)), "taps_v": int(rtc.lib().rtc_resize_taps(h_in, h_out, spec.filter)),
                  "hbm_bytes": hb + vb, "fraction_of_hbm_peak": (hb + vb) / PEAK_HBM * 1e3 / r["median_ms"]})
        rows.append(r)
        print(json.dumps(r), flush=True)


def table():
    print()
    print("| point | taps h / v | call time, median (min .. max) | HBM bytes | of the HBM peak |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['point']} | {r['taps_h']} / {r['taps_v']} | {r['median_ms']:.4f} ms ({r['min_ms']:.4f} .. {r['max_ms']:.4f}) | {r['hbm_bytes'] / 1e6:.1f} MB | {r['fraction_of_hbm_peak']:.3f} |")
    print()


if args.no_host_route:
    ctx.close()
    table()
    sys.exit(0)

# (h) the route before: the supersampled frame to the host, then the host statement; against the device route
scenes = __import__(rtc.__name__ + ".scenes", fromlist=["synthetic"])
world, cam = scenes.synthetic(100, 3840, 2160)
dw = ctx.upload(world)
canvas = rtc.host_canvas(2160, 3840)
lz = rtc.resize_spec("lanczos3")
dw.render(cam, out=canvas)
runs = []
for _ in range(3):
    t0 = time.perf_counter()
    dw.render(cam, out=canvas)
    t1 = time.perf_counter()
    small = rtc.resize(canvas, 1920, 1080, lz)
    t2 = time.perf_counter()
    runs.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3))
mid = [sorted(col)[1] for col in zip(*runs)]
host = {"stage": "host route, north star 3840x2160 -> 1920x1080, lanczos3", "runs": 3, "render_to_pinned_host_ms": mid[0], "host_resize_ms": mid[1], "total_ms": mid[2]}
print(json.dumps(host), flush=True)
frame, out = torch.zeros(3840 * 2160 * 3, **f64), torch.zeros(1920 * 1080 * 3, **f64)
torch.cuda.synchronize()
dev = event_ms(lambda: (dw.render_rows(cam, 0, 2160, frame.data_ptr()), ctx.resize_device(frame.data_ptr(), 3840, 2160, lz, out.data_ptr(), 1920, 1080)))
only = event_ms(lambda: dw.render_rows(cam, 0, 2160, frame.data_ptr()))
print(json.dumps({"stage": "device route: render 3840x2160 + resize", **dev, "render_alone_median_ms": only["median_ms"]}), flush=True)
ctx.synchronize()
assert out.cpu().numpy().tobytes() == small.tobytes(), "the device route's bytes differ from the host route's"
dw.close()

# (p) the supersampled panorama end to end
path = Path(rtc.__file__).resolve().parent / "data" / "supersampled_panorama.yml"
pw, pcam, _, proj, pspec, ow, oh = rtc.load_yaml_resize(path=path)
pdw = ctx.upload(pw)
import copy  # noqa: E402
cam1 = copy.copy(pcam)
cam1.hsize, cam1.vsize = ow, oh
big, one = torch.zeros(pcam.hsize * pcam.vsize * 3, **f64), torch.zeros(ow * oh * 3, **f64)
torch.cuda.synchronize()
ss = event_ms(lambda: (pdw.render_projection_rows(pcam, proj, 0, pcam.vsize, big.data_ptr()),
                       ctx.resize_device(big.data_ptr(), pcam.hsize, pcam.vsize, pspec, one.data_ptr(), ow, oh)))
trace3 = event_ms(lambda: pdw.render_projection_rows(pcam, proj, 0, pcam.vsize, big.data_ptr()))
plain = event_ms(lambda: pdw.render_projection_rows(cam1, proj, 0, oh, one.data_ptr()))
print(json.dumps({"stage": f"panorama {pcam.hsize}x{pcam.vsize} traced and resized to {ow}x{oh}", **ss, "trace_3x_alone_median_ms": trace3["median_ms"],
                  "trace_1x_median_ms": plain["median_ms"]}), flush=True)
pdw.close()
ctx.close()

table()
print(f"north star 3840x2160 -> 1920x1080, lanczos3: on the device {dev['median_ms']:.3f} ms (render alone {only['median_ms']:.3f}); by the earlier route "
      f"{host['total_ms']:.1f} ms (render into a page-locked canvas {host['render_to_pinned_host_ms']:.1f}, host resize {host['host_resize_ms']:.1f})")
print(f"supersampled panorama, {pcam.hsize}x{pcam.vsize} -> {ow}x{oh}: {ss['median_ms']:.3f} ms (the 3x trace alone {trace3['median_ms']:.3f}) against "
      f"{plain['median_ms']:.3f} ms for the 1x frame without anti-aliasing")
