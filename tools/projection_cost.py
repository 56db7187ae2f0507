"""What an orthographic and a panorama frame cost: the north-star World (100 spheres + checker floor) at 1920x1080 under
both projections, against two figures of the same run: the unbinned in-order pinhole frame and the thin-lens frame of one
sample (1x1, aperture 0), which is the launch a projection launch is planned as. The orthographic camera is the scene's
own, 24 units wide; the panorama (full sphere) stands among the spheres. Kernel time per frame from the launch's own events
(rtc_kernel_times_ms), frames in order on one stream into one device canvas; median / min / max over --frames timed
launches. Prints one JSON document.
usage: python tools/projection_cost.py [--frames 12] [--label NAME]"""
import argparse
import json
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
AMONG = ((0.3, 1.2, 8.0), (0.0, 1.0, 20.0), (0.0, 1.0, 0.0))   # the spheres lie on the floor, x -10..10, z -5..25
world, cam = scenes.synthetic(100, W, H)
among = rtc.camera(W, H, cam.fov, rtc.Matrix.make_view_transform(*AMONG))

ctx = rtc.Context(0)
canvas = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()
dw = ctx.upload(world)


def timed(launch):
    """median / min / max kernel ms of `frames` launches (after 2 warm-up launches)"""
    for _ in range(2):
        launch()
    ctx.synchronize()
    ctx.set_timing(1)   # every launch, and forget the earlier pairs
    for _ in range(args.frames):
        launch()
    ctx.synchronize()
    ms = sorted(float(v) for v in ctx.kernel_times_ms(args.frames))
    info = ctx.last_launch_info()
    return {"kernel_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "launches": len(ms), "source": info["source"],
            "binned": info["binned_primary_pass"], "lens_samples": info["lens_samples"], "projection": info["projection"]}


out = {"frame": f"{W}x{H}", "world": "north star: 100 spheres + checker floor", "frames": args.frames, "label": args.label}
pinhole_lens = rtc.lens(0.0, 1.0, 1, 1)
ortho, pano = rtc.projection("orthographic", width=24.0), rtc.projection("panorama")
legs = {
    "pinhole": lambda: dw.render_rows(cam, 0, H, canvas.data_ptr()),
    "pinhole_among": lambda: dw.render_rows(among, 0, H, canvas.data_ptr()),
    "lens_1x1": lambda: dw.render_lens_rows(cam, pinhole_lens, 0, H, canvas.data_ptr()),
    "lens_1x1_among": lambda: dw.render_lens_rows(among, pinhole_lens, 0, H, canvas.data_ptr()),
    "orthographic": lambda: dw.render_projection_rows(cam, ortho, 0, H, canvas.data_ptr()),
    "orthographic_no_cull": lambda: dw.render_projection_rows(cam, ortho, 0, H, canvas.data_ptr(), flags=NO_CULL),
    "panorama": lambda: dw.render_projection_rows(among, pano, 0, H, canvas.data_ptr()),
    "panorama_no_cull": lambda: dw.render_projection_rows(among, pano, 0, H, canvas.data_ptr(), flags=NO_CULL),
}
for name, launch in legs.items():
    out[name] = timed(launch)
for name in ("orthographic", "panorama"):
    out[name]["over_pinhole"] = out[name]["kernel_ms"] / out["pinhole"]["kernel_ms"]
    out[name]["over_lens_1x1"] = out[name]["kernel_ms"] / out["lens_1x1"]["kernel_ms"]
out["panorama"]["over_lens_1x1_among"] = out["panorama"]["kernel_ms"] / out["lens_1x1_among"]["kernel_ms"]
dw.close()
ctx.close()
print(json.dumps(out, indent=1))
