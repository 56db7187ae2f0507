"""What a thin-lens frame costs: the north-star World (100 spheres + checker floor) at 1920x1080 through lens grids of
1x1, 2x2, 4x4 and 8x8 samples, against two figures of the same run: n x the pinhole frame with the binned primary pass
(render kernel + binning kernel; an in-order 1080p launch of a small World is only binned when RTC_BIN_SMALL_PIXELS says
so, as the pipelined headline launches are by default: a second context is created with it set to 0) and the pinhole
frame with RTC_FLAG_NO_CULL. Kernel time per frame from the launch's own events (rtc_kernel_times_ms), frames in order on
one stream into one device canvas; median / min / max over --frames timed launches. Prints one JSON document.
usage: python tools/lens_cost.py [--frames 12] [--label NAME]"""
import argparse
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402
from _bootstrap import package  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--label", default="", help="copied into the document (which build this is)")
args = ap.parse_args()

rtc = package()
scenes = __import__("importlib").import_module(rtc.__name__ + ".scenes")
W, H = 1920, 1080
NO_CULL = 1
APERTURE, FOCAL = 0.1, 10.0   # the spheres lie 5 .. 25 units from the camera
world, cam = scenes.synthetic(100, W, H)

os.environ["RTC_BIN_SMALL_PIXELS"] = "0"   # read at rtc_context_create
ctx_binned = rtc.Context(0)
del os.environ["RTC_BIN_SMALL_PIXELS"]
ctx = rtc.Context(0)
canvas = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()
dw = ctx.upload(world)


def timed(launch, ctx=ctx):
    """median / min / max kernel ms of `frames` launches (after 2 warm-up launches), and the binning kernel's median"""
    for _ in range(2):
        launch()
    ctx.synchronize()
    ctx.set_timing(1)   # every launch, and forget the earlier pairs
    for _ in range(args.frames):
        launch()
    ctx.synchronize()
    ms = sorted(float(v) for v in ctx.kernel_times_ms(args.frames))
    bins = sorted(float(v) for v in ctx.binning_times_ms(args.frames))
    info = ctx.last_launch_info()
    return {"kernel_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "launches": len(ms),
            "binning_kernel_ms": bins[len(bins) // 2] if bins else 0.0, "source": info["source"],
            "binned": info["binned_primary_pass"], "lens_samples": info["lens_samples"]}


out = {"frame": f"{W}x{H}", "world": "north star: 100 spheres + checker floor", "lens": {"aperture": APERTURE, "focal_distance": FOCAL},
       "frames": args.frames, "label": args.label}
out["pinhole"] = timed(lambda: dw.render_rows(cam, 0, H, canvas.data_ptr()))
dwb = ctx_binned.upload(world)
out["pinhole_binned"] = timed(lambda: dwb.render_rows(cam, 0, H, canvas.data_ptr()), ctx_binned)
dwb.close()
ctx_binned.close()
out["pinhole_no_cull"] = timed(lambda: dw.render_rows(cam, 0, H, canvas.data_ptr(), flags=NO_CULL))
pin = out["pinhole_binned"]["kernel_ms"] + out["pinhole_binned"]["binning_kernel_ms"]
brute = out["pinhole_no_cull"]["kernel_ms"]
for g in (1, 2, 4, 8):
    lens = rtc.lens(APERTURE, FOCAL, g, g)
    for name, flags in ((f"lens_{g}x{g}", 0), (f"lens_{g}x{g}_no_cull", NO_CULL)):
        r = timed(lambda: dw.render_lens_rows(cam, lens, 0, H, canvas.data_ptr(), flags=flags))
        n = g * g
        r["ms_per_sample"] = r["kernel_ms"] / n
        r["n_x_binned_pinhole_ms"] = n * pin
        r["sample_over_binned_pinhole_frame"] = r["ms_per_sample"] / pin
        r["sample_over_pinhole_no_cull_frame"] = r["ms_per_sample"] / brute
        out[name] = r
dw.close()
ctx.close()
print(json.dumps(out, indent=1))
