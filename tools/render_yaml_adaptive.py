"""Render a YAML scene with edge-adaptive anti-aliasing (aa-threshold / aa-usteps / aa-vsteps on the camera; include/rtc.h
"edge-adaptive anti-aliasing") and save it by the output's extension:
    python tools/render_yaml_adaptive.py [--threshold T --usteps U --vsteps V --gamma G --mask MASK.png] SCENE.yml OUT.png
The frame is rendered and refined on the GPU (rtc_render_adaptive_device), converted to RGBA there (rtc_canvas_to_rgba8_device)
and encoded behind it on the same stream: only the finished file crosses PCIe. The options override the scene's keys; a scene
without aa-* keys gets the defaults (0.01, 4 x 4). --mask also writes the refinement mask, white where a pixel was refined.
Needs an MI355X (there is no CPU path)."""
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
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--usteps", type=int, default=None)
    ap.add_argument("--vsteps", type=int, default=None)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--mask", default=None)
    args = ap.parse_args(argv[1:])
    rtc = package()
    fmt = rtc.image_format_for_name(args.out)   # an unsupported name fails before anything is rendered
    mask_fmt = rtc.image_format_for_name(args.mask) if args.mask else None
    world, cam, spec = rtc.load_yaml_adaptive(path=args.scene)
    spec = rtc.adaptive(args.threshold if args.threshold is not None else (spec.threshold if spec else rtc.AA_DEFAULT_THRESHOLD),
                        args.usteps or (spec.usteps if spec else rtc.AA_DEFAULT_STEPS), args.vsteps or (spec.vsteps if spec else rtc.AA_DEFAULT_STEPS))
    import torch
    ctx = rtc.Context(0)
    enc = rtc.ImageEncoder(ctx)
    dw = ctx.upload(world)
    px = cam.vsize * cam.hsize
    frame = torch.zeros(px * 3, dtype=torch.float64, device="cuda:0")
    rgba = torch.zeros(px * 4, dtype=torch.uint8, device="cuda:0")
    mask = torch.zeros(px, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    t = time.perf_counter()
    info = dw.render_adaptive_device(cam, spec, frame.data_ptr(), mask.data_ptr())
    ctx.canvas_to_rgba8_device(frame.data_ptr(), cam.hsize, cam.vsize, args.gamma, rgba.data_ptr())
    data = enc.encode_device(fmt, rgba.data_ptr(), cam.hsize, cam.vsize, 4)
    dt = time.perf_counter() - t
    Path(args.out).write_bytes(data)
    if args.mask:
        white = (mask * 255).repeat_interleave(3).contiguous()
        torch.cuda.synchronize()
        Path(args.mask).write_bytes(enc.encode_device(mask_fmt, white.data_ptr(), cam.hsize, cam.vsize, 3))
    print(f"{args.out}: {cam.hsize}x{cam.vsize}, {len(world)} shapes, {spec.usteps}x{spec.vsteps} samples on {info['pixels_refined']} of {px} pixels "
          f"({100.0 * info['pixels_refined'] / px:.1f} %), {info['rays_refined']} rays in {info['launches']} launches; {len(data)} bytes in {dt * 1e3:.1f} ms "
          f"(rendering + refining + encoding + PCIe)")
    dw.close()
    enc.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
