"""1080p frame time of the north-star World (100 spheres + checker floor) under area lights of growing sample counts, against
its one-light frame and its 8-point-light frame on the same build. Frames in order on one stream into one device canvas,
median / min / max of REPS x FRAMES frames; prints one JSON document.
usage: python tools/area_light_cost.py [--frames 20] [--reps 5]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
from _bootstrap import package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

rtc = package()
scenes = __import__("importlib").import_module(rtc.__name__ + ".scenes")
W, H = 1920, 1080
base, cam = scenes.synthetic(100, W, H)
key = base.light


def area(n):  # an n x n light of side 4 around the scene's own light, the same total intensity
    return rtc.area_light((-12.0, 10.0, -12.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), n, n, (1.0, 1.0, 1.0))


eight = [rtc.light(position=(-12.0 + 0.5 * i, 10.0, -12.0 + 0.5 * i), intensity=(0.125, 0.125, 0.125)) for i in range(8)]
CASES = {"one_light": [key], "eight_point_lights": eight, "area_3x3": [area(3)], "area_4x4": [area(4)], "area_8x8": [area(8)]}

ctx = rtc.Context(0)
canvas = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()
out = {"frame": f"{W}x{H}", "world": "north star: 100 spheres + checker floor", "frames_per_rep": args.frames, "reps": args.reps}
for name, lights in CASES.items():
    w = rtc.World(lights)
    w.shapes = base.shapes
    dw = ctx.upload(w)
    for _ in range(3):
        dw.render_rows(cam, 0, H, canvas.data_ptr())
    ctx.synchronize()
    info = ctx.last_launch_info()
    ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for _ in range(args.frames):
            dw.render_rows(cam, 0, H, canvas.data_ptr())
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / args.frames)
    ms.sort()
    out[name] = {"samples": len(w.samples()), "light_table": info["light_table"], "source": info["source"],
                 "median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}
    dw.close()
one = out["one_light"]["median_ms"]
for name in CASES:
    out[name]["over_one_light"] = out[name]["median_ms"] / one
    out[name]["ms_per_further_sample"] = (out[name]["median_ms"] - one) / max(1, out[name]["samples"] - 1)
ctx.close()
print(json.dumps(out, indent=1))
