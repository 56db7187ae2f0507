"""Render a YAML scene through the post-processing passes (tonemap-* / bloom-* on the camera; include/rtc.h "exposure, tone
mapping and bloom") and save it by the output's extension:
    python tools/render_yaml_post.py [--gamma G --no-bloom --plain PLAIN.png] SCENE.yml OUT.png
The frame is rendered into a device canvas, then bloom (rtc_canvas_bloom_device), the frame statistics
(rtc_canvas_luminance_device), the tone map (rtc_canvas_tonemap_device, which reads the statistics in device memory),
rtc_canvas_to_rgba8_device and the encoder, all on one stream: only the finished file crosses PCIe and nothing waits in
between. A scene without tonemap-* keys gets REINHARD with key 0.18 and auto white; one without bloom-* keys gets no bloom.
--plain also writes the frame as it was before (clamped by Color::scale), for comparison. Needs an MI355X."""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]
from _bootstrap import package  # noqa: E402


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("out")
    ap.add_argument("--gamma", type=float, default=2.2)
    ap.add_argument("--no-bloom", action="store_true")
    ap.add_argument("--plain", default=None)
    args = ap.parse_args(argv[1:])
    rtc = package()
    fmt = rtc.image_format_for_name(args.out)   # an unsupported name fails before anything is rendered
    plain_fmt = rtc.image_format_for_name(args.plain) if args.plain else None
    world, cam, tm, bl = rtc.load_yaml_post(path=args.scene)
    tm = tm or rtc.tonemap_spec("reinhard", key=0.18, auto_white=True)
    if args.no_bloom:
        bl = None
    import torch
    ctx = rtc.Context(0)
    enc = rtc.ImageEncoder(ctx)
    dw = ctx.upload(world)
    width, height, px = cam.hsize, cam.vsize, cam.vsize * cam.hsize
    frame = torch.zeros(px * 3, dtype=torch.float64, device="cuda:0")
    post = torch.zeros(px * 3, dtype=torch.float64, device="cuda:0")
    stats = torch.zeros(3, dtype=torch.float64, device="cuda:0")
    rgba = torch.zeros(px * 4, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    t = time.perf_counter()
    dw.render_rows(cam, 0, height, frame.data_ptr())
    src = frame.data_ptr()
    if bl is not None:
        ctx.bloom_device(src, width, height, bl, post.data_ptr())
        src = post.data_ptr()
    ctx.luminance_device(src, width, height, stats.data_ptr())
    ctx.tonemap_device(src, width, height, tm, post.data_ptr(), stats.data_ptr())
    ctx.canvas_to_rgba8_device(post.data_ptr(), width, height, args.gamma, rgba.data_ptr())
    data = enc.encode_device(fmt, rgba.data_ptr(), width, height, 4)
    dt = time.perf_counter() - t
    Path(args.out).write_bytes(data)
    clipped = int((rgba.view(-1, 4)[:, :3] == 255).sum())
    line = f"{args.out}: {width}x{height}, {len(world)} shapes, {len(world.lights)} lights; {len(data)} bytes in {dt * 1e3:.1f} ms; {clipped} channels at 255"
    if args.plain:
        ctx.canvas_to_rgba8_device(frame.data_ptr(), width, height, args.gamma, rgba.data_ptr())
        Path(args.plain).write_bytes(enc.encode_device(plain_fmt, rgba.data_ptr(), width, height, 4))
        line += f" (without the passes: {int((rgba.view(-1, 4)[:, :3] == 255).sum())})"
    print(line)
    dw.close()
    enc.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
