"""What a motion-blurred frame costs: the north-star World (100 spheres + checker floor, six of the spheres moving by more
than their radius) at 1920x1080 with 4, 8, 16 and 64 shutter samples, two ways, in one process:
  shutter   Shutter.render_rgb8 (rtc_shutter_render_rgb8): sub-frames rendered back to back on the device, averaged by
            k_average_over, 3 bytes per pixel cross PCIe once;
  loop      what a caller had before: DeviceWorld.update + DeviceWorld.render per sample into a page-locked canvas (24
            bytes per pixel cross PCIe per sample), the mean taken on the host (numpy, in sample order) and quantised there.
            The per-sample Worlds are built before the clock starts; the shutter builds its own inside it.
Both are host wall-clock times around calls that end in a device synchronise, median / min / max over --reps frames after
one warm-up frame each, alternating between the two ways; the two 8-bit frames are compared byte for byte.
  average   k_average_over alone: rtc_canvas_average_device over 8 and 16 resident 1080p canvases (one pass, two passes),
            device events around --reps calls, against the bytes a pass moves ((frames + carried sum) read, one canvas
            written): an achieved rate, to be read against the HBM peak of MI355X_MICROARCH.md.
Prints one JSON document. Needs an MI355X.
usage: python tools/shutter_cost.py [--reps 5] [--label NAME]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from _bootstrap import package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--label", default="", help="copied into the document (which build this is)")
args = ap.parse_args()

rtc = package()
scenes = __import__("importlib").import_module(rtc.__name__ + ".scenes")
W, H = args.width, args.height
world, cam = scenes.synthetic(100, W, H)
moves = {0: (1.1, 0.0, 0.3), 1: (-0.9, 0.6, 0.0), 2: (0.0, 0.8, -0.7), 5: (1.6, 0.0, 0.0), 7: (-1.2, 0.2, 0.9), 11: (0.7, 1.0, 0.0)}
motions = []
for i, d in moves.items():
    opened = rtc.Matrix(list(world.shapes[i].inv)).inverse()
    motions.append(rtc.motion(i, opened, opened.translation(*d)))

ctx = rtc.Context(0)
sh = ctx.shutter()
dw = ctx.upload(world)
pinned = rtc.host_canvas(H, W)
out8 = rtc.host_canvas_rgb8(H, W)


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "frames": len(ms)}


def shutter_frame(n):
    t = time.perf_counter()
    sh.render_rgb8(world, motions, cam, n, out=out8)   # synchronous
    return (time.perf_counter() - t) * 1e3


def loop_frame(n, worlds):
    t = time.perf_counter()
    acc = np.zeros((H, W, 3))
    for wk in worlds:
        dw.update(wk)
        dw.render(cam, out=pinned)   # synchronous
        acc += pinned
    frame = rtc.color_scale255(acc / float(n))
    return (time.perf_counter() - t) * 1e3, frame


doc = {"frame": f"{W}x{H}", "world": "north star: 100 spheres + checker floor, 6 spheres moving", "reps": args.reps, "label": args.label,
       "device": ctx.device_info()["name"], "samples": {}}
for n in (4, 8, 16, 64):
    worlds = [rtc.shutter_shapes(world, motions, n, k) for k in range(n)]
    shutter_frame(n)
    loop_frame(n, worlds)
    a, b, frame = [], [], None
    for _ in range(args.reps):   # alternating
        a.append(shutter_frame(n))
        ms, frame = loop_frame(n, worlds)
        b.append(ms)
    doc["samples"][str(n)] = {"shutter": spread(a), "loop": spread(b), "loop_over_shutter": spread(b)["median_ms"] / spread(a)["median_ms"],
                              "same_bytes": bool(np.array_equal(frame, out8)),
                              "pcie_bytes_shutter": 3 * W * H, "pcie_bytes_loop": 24 * W * H * n}

count = 3 * W * H
doc["average"] = {}
for n in (8, 16):
    frames = torch.rand((n, count), dtype=torch.float64, device="cuda:0")
    mean = torch.zeros(count, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(3):
        ctx.canvas_average_device(frames.data_ptr(), n, count, mean.data_ptr())
    ctx.synchronize()
    ms = []
    for _ in range(max(args.reps, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.canvas_average_device(frames.data_ptr(), n, count, mean.data_ptr())
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    passes = (n + 7) // 8
    moved = 8 * count * (n + (passes - 1) + passes)   # frames read, the carried sum read by every pass but the first, one canvas written per pass
    s = spread(ms)
    s.update({"passes": passes, "bytes_moved": moved, "ms_per_pass": s["median_ms"] / passes, "gb_per_s": moved / (s["median_ms"] * 1e-3) / 1e9})
    doc["average"][str(n)] = s
dw.close()
sh.close()
ctx.close()
print(json.dumps(doc, indent=1))
