"""Render a YAML scene and what its pixels saw (the AOV planes, include/rtc.h "arbitrary output variables"):
    python tools/render_aov.py SCENE.yml OUTDIR [--near N --far F] [--exr [PLANES]]
writes OUTDIR/beauty.png (the colour frame) and depth.png, normal.png, index.png, shadow.png (rtc_aov_view_rgb8's pictures of
the planes). Colour frame, planes and pictures stay in device memory; every file is encoded there (ImageEncoder.encode_device)
and only the finished files cross PCIe — plus, when --near / --far are not both given, the depth plane, whose smallest and
largest finite value they default to. --exr also writes OUTDIR/frame.exr: ONE multi-channel OpenEXR file of data, not pictures —
the f64 colour frame as HALF R, G, B plus the planes asked for (a comma-separated list of depth, normal, point, index,
shadow; all five when none is named) as Z, N.*, P.*, id and shadow channels (FloatEncoder.encode_device, include/rtc.h
"float files"). Needs an MI355X (there is no CPU path)."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]
from _bootstrap import package  # noqa: E402


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("outdir")
    ap.add_argument("--near", type=float, default=None)
    ap.add_argument("--far", type=float, default=None)
    ap.add_argument("--exr", nargs="?", const="depth,normal,point,index,shadow", default=None, metavar="PLANES")
    args = ap.parse_args(argv[1:])
    rtc = package()
    abi = __import__("importlib").import_module(rtc.__name__ + ".abi")
    import numpy as np
    import torch
    world, cam = rtc.load_yaml(path=args.scene)
    width, height = cam.hsize, cam.vsize
    out = Path(args.outdir)
    out.mkdir(parents=True, exist_ok=True)
    ctx = rtc.Context(0)
    dw, enc = ctx.upload(world), rtc.ImageEncoder(ctx)
    n_lights = rtc.lib().rtc_world_light_count(dw._h)
    dev = {p: torch.zeros(width * height * comps, dtype=getattr(torch, d), device="cuda:0") for p, (d, comps) in abi.AOV_PLANES.items()}
    pic = torch.zeros(width * height * 3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    sizes = {}
    dw.render_rows(cam, 0, height, None, d_ptr8=pic.data_ptr())   # 8-bit rows only
    sizes["beauty"] = (out / "beauty.png").write_bytes(enc.encode_device("png", pic.data_ptr(), width, height, 3))
    dw.render_aov_device(cam, {p: t.data_ptr() for p, t in dev.items()})
    near, far = args.near, args.far
    if near is None or far is None:
        ctx.synchronize()
        depth = dev["depth"].cpu().numpy()
        finite = depth[np.isfinite(depth)]
        lo, hi = (float(finite.min()), float(finite.max())) if finite.size else (0.0, 1.0)
        near = lo if near is None else near
        far = hi if far is None else far
        if not far > near:   # a flat frame: any interval around it
            far = near + 1.0
    for view in ("depth", "normal", "index", "shadow"):
        ctx.aov_view_device(view, {view: dev[view].data_ptr()}, width, height, pic.data_ptr(), near=near, far=far, n_lights=n_lights)
        sizes[view] = (out / f"{view}.png").write_bytes(enc.encode_device("png", pic.data_ptr(), width, height, 3))
    if args.exr is not None:
        wanted = [p for p in args.exr.split(",") if p]
        unknown = sorted(set(wanted) - {"depth", "normal", "point", "index", "shadow"})
        if unknown:
            ap.error(f"--exr: not a plane of the file: {', '.join(unknown)}")
        rgb = torch.zeros(width * height * 3, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        dw.render_rows(cam, 0, height, rgb.data_ptr())
        fenc = rtc.FloatEncoder(ctx)
        sizes["frame.exr"] = (out / "frame.exr").write_bytes(
            fenc.encode_device("exr", rgb.data_ptr(), width, height, {p: dev[p].data_ptr() for p in wanted}, "half"))
        fenc.close()
    hits = int((dev["index"] >= 0).sum().item())
    print(f"{out}: {width}x{height}, {len(world)} shapes, {n_lights} light sample(s), {hits} of {width * height} pixels hit, "
          f"depth {near:.6g} .. {far:.6g}; bytes: " + ", ".join(f"{k if '.' in k else k + '.png'} {v}" for k, v in sizes.items()))
    enc.close()
    dw.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
