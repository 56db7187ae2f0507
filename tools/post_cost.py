"""What the post-processing passes cost (include/rtc.h "exposure, tone mapping and bloom"), at 1920x1080, on the frame of
data/bright_lights.yml rendered on the device. In one run, each point the median of --launches calls (after --warmup) between two
HIP events recorded around the call on the context's stream (the method of tools/filter_cost.py):
  (s)  rtc_canvas_luminance_device: three launches (k_lum_pixels, k_lum_records twice);
  (t)  rtc_canvas_tonemap_device per curve, with a fixed exposure and with both AUTO flags (the record read in device memory);
  (b)  rtc_canvas_bloom_device at radius 4, 16 and 32 (k_bloom_h + k_bloom_v).
Per point, from counts kept here (no counter is read):
        HBM bytes = 24 per pixel read (statistics); 24 read + 24 written (tone map); bloom: k_bloom_h reads 24 and writes 24,
        k_bloom_v reads 24 of H and 24 of C and writes 24 = 120 per pixel (the halos' re-reads come from the caches); against 8.0 TB/s;
        LDS bytes read (bloom) = 2 passes x (2R+1) taps x 3 channels x 8 per pixel, against 256 CUs x 256 B/clk x 2.4 GHz: the rate
        of ds_read_b64, which the tap loops are made of (rtc_post.hip). A library built with -DRTC_POST_PAIRED_READS=1 reads with
        ds_read2_b64, served at 128 B/clk: --lds-bytes-per-clk 128 judges that build against its own instruction's rate;
        f64 instructions (bloom) = 2 passes x (2R+1) x 3 x 2 (one product and one sum per tap and channel), against 39.3 T/s.
        The row says which of them leaves the least time and what share of that peak the measured time is.
  (h)  the route the library offered before: rtc_render into a page-locked host canvas, then the host statements (bloom at the
        scene's radius, statistics, tone map), wall time, the median of three runs per step.
Prints one JSON line per point and a table. The points are CALL times: the statistics' three dependent launches and the bloom's
two include the gaps between them. For the time of each kernel run the tool under `rocprofv3 --kernel-trace --stats` with
--radii R --no-host-route (one radius, so that k_bloom_h and k_bloom_v have one size each) and read the kernel statistics.
usage: python tools/post_cost.py [--launches 20] [--warmup 3] [--radii 4,16,32] [--lds-bytes-per-clk 256] [--no-host-route]"""
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
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--radii", default="4,16,32")
ap.add_argument("--lds-bytes-per-clk", type=int, default=256)
ap.add_argument("--no-host-route", action="store_true")
args = ap.parse_args()
assert args.launches >= 20, "the median of at least 20 launches"

rtc = package()
W, H = 1920, 1080
NPX = W * H
PEAK_HBM, PEAK_LDS, PEAK_F64_INSTR = 8.0e12, 256 * args.lds_bytes_per_clk * 2.4e9, 39.3e12

path = Path(rtc.__file__).resolve().parent / "data" / "bright_lights.yml"
text = path.read_text().replace("width: 640", f"width: {W}").replace("height: 360", f"height: {H}")
world, cam, tm_scene, bl_scene = rtc.load_yaml_post(text=text)

stream = torch.cuda.Stream()
ctx = rtc.Context(0, stream=stream.cuda_stream)
f64 = dict(dtype=torch.float64, device="cuda:0")
frame, out = torch.zeros(NPX * 3, **f64), torch.zeros(NPX * 3, **f64)
stats = torch.zeros(3, **f64)
torch.cuda.synchronize()
dw = ctx.upload(world)
dw.render_rows(cam, 0, H, frame.data_ptr())
ctx.luminance_device(frame.data_ptr(), W, H, stats.data_ptr())
ctx.synchronize()


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


def judge(row, hbm_bytes, lds_bytes=0, instr=0):
    ms = row["median_ms"]
    least = {"HBM": hbm_bytes / PEAK_HBM * 1e3, "LDS": lds_bytes / PEAK_LDS * 1e3, "f64 VALU": instr / PEAK_F64_INSTR * 1e3}
    bound = max(least, key=least.get)
    row.update({"hbm_bytes": hbm_bytes, "lds_bytes_read": lds_bytes, "f64_instructions": instr, "fraction_of_hbm_peak": least["HBM"] / ms,
                "fraction_of_lds_peak": least["LDS"] / ms, "fraction_of_f64_valu_peak": least["f64 VALU"] / ms, "bound_by": bound, "share_of_peak": least[bound] / ms})
    return row


rows = []
r = {"stage": "statistics", "frame": f"{W}x{H}", **event_ms(lambda: ctx.luminance_device(frame.data_ptr(), W, H, stats.data_ptr()))}
rows.append(judge(r, 24 * NPX))
print(json.dumps(r), flush=True)
for curve in ("linear", "reinhard", "aces"):
    for label, spec in (("fixed exposure", rtc.tonemap_spec(curve, exposure=0.5, white=4.0)), ("auto exposure + auto white", rtc.tonemap_spec(curve, key=0.18, auto_white=True))):
        r = {"stage": f"tone map, {curve}, {label}", **event_ms(lambda: ctx.tonemap_device(frame.data_ptr(), W, H, spec, out.data_ptr(), stats.data_ptr()))}
        rows.append(judge(r, 48 * NPX))
        print(json.dumps(r), flush=True)
for radius in [int(v) for v in args.radii.split(",")]:
    spec = rtc.bloom_spec(1.0, 0.6, radius / 3.0, radius)
    taps = 2 * radius + 1
    r = {"stage": f"bloom, radius {radius}", **event_ms(lambda: ctx.bloom_device(frame.data_ptr(), W, H, spec, out.data_ptr()))}
    rows.append(judge(r, 120 * NPX, 2 * taps * 24 * NPX, 2 * taps * 6 * NPX))
    print(json.dumps(r), flush=True)

def table():
    print()
    print("| stage | call time, median (min .. max) | HBM bytes | of the HBM peak | of the LDS peak | of the f64 VALU peak | bound by | share of peak |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['stage']} | {r['median_ms']:.4f} ms ({r['min_ms']:.4f} .. {r['max_ms']:.4f}) | {r['hbm_bytes'] / 1e6:.1f} MB | {r['fraction_of_hbm_peak']:.3f} | "
              f"{r['fraction_of_lds_peak']:.3f} | {r['fraction_of_f64_valu_peak']:.3f} | {r['bound_by']} | {r['share_of_peak']:.3f} |")
    print()


if args.no_host_route:
    dw.close()
    ctx.close()
    table()
    sys.exit(0)

# the route before: the frame to the host, then the host statements
canvas = rtc.host_canvas(H, W)
dw.render(cam, out=canvas)
runs = []
for _ in range(3):   # the median of three runs per step
    t0 = time.perf_counter()
    dw.render(cam, out=canvas)
    t1 = time.perf_counter()
    bloomed = rtc.bloom(canvas, bl_scene)
    t2 = time.perf_counter()
    st = rtc.luminance(bloomed)
    t3 = time.perf_counter()
    mapped = rtc.tonemap(bloomed, tm_scene, st)
    t4 = time.perf_counter()
    runs.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, (t4 - t0) * 1e3))
mid = [sorted(col)[1] for col in zip(*runs)]
host = {"stage": "host route", "runs": 3, "render_to_pinned_host_ms": mid[0], "host_bloom_ms": mid[1], "host_bloom_radius": bl_scene.radius,
        "host_statistics_ms": mid[2], "host_tonemap_ms": mid[3], "total_ms": mid[4]}
print(json.dumps(host), flush=True)
# the same chain on the device, for the comparison (the scene's own records)
chain = event_ms(lambda: (ctx.bloom_device(frame.data_ptr(), W, H, bl_scene, out.data_ptr()), ctx.luminance_device(out.data_ptr(), W, H, stats.data_ptr()),
                          ctx.tonemap_device(out.data_ptr(), W, H, tm_scene, out.data_ptr(), stats.data_ptr())))
print(json.dumps({"stage": f"device chain: bloom radius {bl_scene.radius}, statistics, tone map", **chain}), flush=True)
ctx.synchronize()
assert out.cpu().numpy().tobytes() == mapped.tobytes(), "the device chain's bytes differ from the host chain's"
dw.close()
ctx.close()

table()
print(f"device chain (bloom radius {bl_scene.radius}, statistics, tone map): {chain['median_ms']:.4f} ms; the same bytes by the earlier route: "
      f"{host['total_ms']:.1f} ms (render into a page-locked canvas {host['render_to_pinned_host_ms']:.1f}, host bloom {host['host_bloom_ms']:.1f}, "
      f"statistics {host['host_statistics_ms']:.1f}, tone map {host['host_tonemap_ms']:.1f})")
