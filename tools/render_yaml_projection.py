"""Render a YAML scene whose camera has a projection (projection: orthographic | panorama, ortho-width, pano-h-span,
pano-v-span; include/rtc.h "Orthographic and equirectangular panorama cameras") and save it by the output's extension:
    python tools/render_yaml_projection.py [--width W --height H] SCENE.yml OUT.png
The frame is rendered on the GPU (rtc_render_projection_rows), its 8-bit rows stay there and are encoded behind the render
on the same stream (rtc_image_encoder_encode_device): only the finished file crosses PCIe. --width / --height override the
scene's canvas size (a full panorama wants 2:1). A scene without projection keys is rendered as the pinhole (or thin-lens)
camera it describes. Needs an MI355X (there is no CPU path)."""
import argparse
import ctypes as C
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
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    args = ap.parse_args(argv[1:])
    rtc = package()
    fmt = rtc.image_format_for_name(args.out)   # an unsupported name fails before anything is rendered
    world, cam, lens, proj = rtc.load_yaml_projection(path=args.scene)
    if args.width or args.height:
        sized = rtc.camera(args.width or cam.hsize, args.height or cam.vsize, cam.fov, samples=cam.samples)
        C.memmove(sized.view_inv, cam.view_inv, C.sizeof(sized.view_inv))
        cam = sized
    import torch
    ctx = rtc.Context(0)
    enc = rtc.ImageEncoder(ctx)
    dw = ctx.upload(world)
    frame = torch.zeros((cam.vsize, cam.hsize, 3), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    t = time.perf_counter()
    if proj is not None:
        dw.render_projection_rows(cam, proj, 0, cam.vsize, None, d_ptr8=frame.data_ptr())
    elif lens is not None:
        dw.render_lens_rows(cam, lens, 0, cam.vsize, None, d_ptr8=frame.data_ptr())
    else:
        dw.render_rows(cam, 0, cam.vsize, None, d_ptr8=frame.data_ptr())
    data = enc.encode_device(fmt, frame.data_ptr(), cam.hsize, cam.vsize, 3)
    dt = time.perf_counter() - t
    Path(args.out).write_bytes(data)
    kind = {None: "pinhole", rtc.PROJ_ORTHOGRAPHIC: "orthographic", rtc.PROJ_PANORAMA: "panorama"}[proj.kind if proj is not None else None]
    print(f"{args.out}: {cam.hsize}x{cam.vsize} {kind}, {len(world)} shapes, {len(data)} bytes in {dt * 1e3:.1f} ms (rendering + encoding + PCIe)")
    dw.close()
    enc.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
