"""Render a YAML scene at the size it is traced at, resize it on the device to the size its camera asks for (output-width /
output-height / output-filter; include/rtc.h "resizing f64 canvases") and save it by the output's extension:
    python tools/render_yaml_resize.py [--gamma G --size WxH --filter NAME --plain PLAIN.png] SCENE.yml OUT.png
The frame is rendered into a device canvas (the camera's projection, when it has one), then rtc_canvas_resize_device,
rtc_canvas_to_rgba8_device and the encoder, all on one stream: only the finished file crosses PCIe. --size and --filter replace
the scene's keys; a scene without them and without the options is delivered at the traced size (a copy). --plain also
writes the frame traced directly at the delivered size, one ray per pixel, for comparison. Needs an MI355X."""
import argparse
import copy
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
    ap.add_argument("--size", default=None)
    ap.add_argument("--filter", default=None)
    ap.add_argument("--plain", default=None)
    args = ap.parse_args(argv[1:])
    rtc = package()
    fmt = rtc.image_format_for_name(args.out)   # an unsupported name fails before anything is rendered
    plain_fmt = rtc.image_format_for_name(args.plain) if args.plain else None
    world, cam, lens, proj, spec, out_w, out_h = rtc.load_yaml_resize(path=args.scene)
    if lens is not None:
        sys.exit("the scene's camera has a lens: this tool renders pinhole and projection cameras")
    if args.size:
        out_w, out_h = (int(v) for v in args.size.lower().split("x"))
    spec = rtc.resize_spec(args.filter) if args.filter else (spec or rtc.resize_spec())
    import torch
    ctx = rtc.Context(0)
    enc = rtc.ImageEncoder(ctx)
    dw = ctx.upload(world)
    width, height = cam.hsize, cam.vsize
    frame = torch.zeros(width * height * 3, dtype=torch.float64, device="cuda:0")
    small = torch.zeros(out_w * out_h * 3, dtype=torch.float64, device="cuda:0")
    rgba = torch.zeros(out_w * out_h * 4, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def trace(c, d_ptr):
        if proj is not None:
            dw.render_projection_rows(c, proj, 0, c.vsize, d_ptr)
        else:
            dw.render_rows(c, 0, c.vsize, d_ptr)

    t = time.perf_counter()
    trace(cam, frame.data_ptr())
    ctx.resize_device(frame.data_ptr(), width, height, spec, small.data_ptr(), out_w, out_h)
    ctx.canvas_to_rgba8_device(small.data_ptr(), out_w, out_h, args.gamma, rgba.data_ptr())
    data = enc.encode_device(fmt, rgba.data_ptr(), out_w, out_h, 4)
    dt = time.perf_counter() - t
    Path(args.out).write_bytes(data)
    names = {v: k for k, v in rtc.RESIZE_FILTERS.items()}
    print(f"{args.out}: traced {width}x{height}, delivered {out_w}x{out_h} ({names[spec.filter]}), {len(world)} shapes; {len(data)} bytes in {dt * 1e3:.1f} ms")
    if args.plain:
        text = Path(args.scene).read_text()
        small_cam = copy.copy(cam)
        if proj is None:   # a pinhole camera of the delivered size: the file's text with its size replaced
            small_cam = rtc.load_yaml_resize(text=text.replace(f"width: {width}", f"width: {out_w}", 1).replace(f"height: {height}", f"height: {out_h}", 1))[1]
        else:              # a projection reads only the size and the view
            small_cam.hsize, small_cam.vsize = out_w, out_h
        trace(small_cam, small.data_ptr())
        ctx.canvas_to_rgba8_device(small.data_ptr(), out_w, out_h, args.gamma, rgba.data_ptr())
        Path(args.plain).write_bytes(enc.encode_device(plain_fmt, rgba.data_ptr(), out_w, out_h, 4))
    dw.close()
    enc.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
