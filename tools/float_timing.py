"""Float file timing on one GPU (include/rtc.h "float files", csrc/rtc_float.hip), following image_timing.py: per 1080p
north-star frame (100 spheres + checker floor), for Radiance HDR, PFM, OpenEXR (HALF colour) and OpenEXR with the colour and
every AOV plane —
  * the file's size;
  * device route: FloatEncoder.encode_device of a canvas (and planes) already in device memory, to the file in host memory
    (host clock around the call, which ends in a device synchronise and the copy of exactly the file);
  * host route, the only one without the device writers: the f64 canvas copied into a page-locked host canvas (rtc_render's
    copy, timed alone as its difference to the rows launch) and the host statement (float_encode) on it; for the file with
    planes also rtc_render_aov's copies;
  * both routes whole, render included: FloatEncoder.render against rtc_render + float_encode.
Every figure is the median of --reps runs after two warm-up runs, with the smallest and largest beside it. The two routes
are checked to give the same bytes. Prints one JSON line.

Kernel times come from a run of their own under the kernel trace (tracing slows the host):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/float_timing.py --chains-only
runs each chain --reps times and nothing else; `--kernel-stats DIR` then prints the float kernels' average durations from
the trace's kernel_stats.csv.
Usage: python tools/float_timing.py [--width 1920 --height 1080 --reps 20] [--chains-only | --kernel-stats DIR]"""
import argparse
import csv
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from _bootstrap import package  # noqa: E402

KERNELS = ("k_float_pack", "k_hdr_planes", "k_hdr_rle", "k_hdr_offsets")
PLANES = ("index", "depth", "point", "normal", "shadow")


def timed(fn, reps):
    """(median, min, max) in ms of `reps` calls after two warm-up calls, and the last result."""
    for _ in range(2):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}, out


def kernel_stats(directory):
    rows = {}
    for path in Path(directory).rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(path)):
            name = r.get("Name", "")
            for k in KERNELS:
                if k in name:
                    key = k + ("<emit>" if "true" in name or "1>" in name else "<sizes>" if k == "k_hdr_rle" else "")
                    rows[key] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                                 "max_us": round(float(r["MaxNs"]) / 1e3, 2), "name": name[:80]}
    print(json.dumps({"kernel_stats": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--chains-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)
    import numpy as np
    import torch
    rtc = package()
    scenes = importlib.import_module(rtc.__name__ + ".scenes")
    ctx = rtc.Context(0)
    world, cam = scenes.synthetic(100, a.width, a.height)
    dw = ctx.upload(world)
    enc = rtc.FloatEncoder(ctx)
    w, h = a.width, a.height
    d_rgb = torch.zeros(h * w * 3, dtype=torch.float64, device="cuda:0")
    host_planes = dw.render_aov(cam, PLANES)
    d_planes = {k: torch.from_numpy(v.view(np.uint8).reshape(-1)).to("cuda:0") for k, v in host_planes.items()}
    torch.cuda.synchronize()
    dw.render_rows(cam, 0, h, d_rgb.data_ptr())
    ctx.synchronize()
    pointers = {k: v.data_ptr() for k, v in d_planes.items()}
    configs = {"hdr": ("hdr", None, "half"), "pfm": ("pfm", None, "half"), "exr_half": ("exr", None, "half"),
               "exr_half_all_planes": ("exr", pointers, "half")}
    if a.chains_only:
        for fmt, ptrs, t in configs.values():
            for _ in range(a.reps):
                enc.encode_device(fmt, d_rgb.data_ptr(), w, h, ptrs, t)
        ctx.synchronize()
        print(json.dumps({"chains_only": True, "reps": a.reps}))
        return
    res = {"size": f"{w}x{h}", "reps": a.reps}
    pinned = rtc.host_canvas(h, w)

    def rows_only():
        dw.render_rows(cam, 0, h, d_rgb.data_ptr())
        ctx.synchronize()

    res["render_rows_on_device"], _ = timed(rows_only, a.reps)
    res["rtc_render_into_pinned_canvas"], canvas = timed(lambda: dw.render(cam, out=pinned), a.reps)
    res["canvas_copy_ms"] = round(res["rtc_render_into_pinned_canvas"]["median_ms"] - res["render_rows_on_device"]["median_ms"], 4)
    res["rtc_render_aov_to_host"], _ = timed(lambda: dw.render_aov(cam, PLANES), a.reps)
    for name, (fmt, ptrs, t) in configs.items():
        planes = host_planes if ptrs else None
        dev, b = timed(lambda: enc.encode_device(fmt, d_rgb.data_ptr(), w, h, ptrs, t), a.reps)
        host, hb = timed(lambda: rtc.float_encode(fmt, canvas, planes, t), max(3, a.reps // 4))
        assert b == hb, name
        r = {"bytes": len(b), "device_chain_to_host_file": dev, "host_statement_on_the_copied_canvas": host}
        if not ptrs:
            r["device_render_and_file"], b2 = timed(lambda: enc.render(fmt, dw, cam, rgb_type=t), a.reps)
            r["host_render_copy_and_file"], _ = timed(lambda: rtc.float_encode(fmt, dw.render(cam, out=pinned), None, t), max(3, a.reps // 4))
            assert b2 == b, name
        res[name] = r
    enc.close()
    dw.close()
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
