"""Render a YAML scene with motion blur (a shape's `motion:` list, the camera's `shutter-samples`; include/rtc.h "Motion
blur") and save it by the output's extension:
    python tools/render_yaml_motion.py [--samples N] [--gamma G] SCENE.yml OUT.png
The sub-frames are rendered and averaged on the GPU (rtc_shutter_render_device), the 8-bit frame stays there and is
encoded behind it on the same stream (rtc_image_encoder_encode_device): only the finished file crosses PCIe. --samples
overrides the scene's shutter-samples; with --gamma the file holds to_imgbuf's RGBA at that gamma instead of Color::scale's
RGB. A scene with lens keys is rendered through its lens. Needs an MI355X (there is no CPU path)."""
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
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--gamma", type=float, default=0.0)
    args = ap.parse_args(argv[1:])
    rtc = package()
    fmt = rtc.image_format_for_name(args.out)   # an unsupported name fails before anything is rendered
    world, cam, lens, motions, samples = rtc.load_yaml_motion(path=args.scene)
    samples = args.samples or samples
    import torch
    ctx = rtc.Context(0)
    sh, enc = ctx.shutter(), rtc.ImageEncoder(ctx)
    channels = 4 if args.gamma else 3
    frame = torch.zeros((cam.vsize, cam.hsize, channels), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    t = time.perf_counter()
    if args.gamma:
        sh.render_device(world, motions, cam, samples, d_rgba8=frame.data_ptr(), gamma=args.gamma, lens=lens)
    else:
        sh.render_device(world, motions, cam, samples, d_rgb8=frame.data_ptr(), lens=lens)
    data = enc.encode_device(fmt, frame.data_ptr(), cam.hsize, cam.vsize, channels)
    dt = time.perf_counter() - t
    Path(args.out).write_bytes(data)
    print(f"{args.out}: {cam.hsize}x{cam.vsize}, {len(world)} shapes of which {len(motions)} move, {samples} shutter samples, "
          f"{len(data)} bytes in {dt * 1e3:.1f} ms (rendering + averaging + encoding + PCIe)")
    enc.close()
    sh.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
