"""Render a YAML scene and what its pixels saw (the AOV planes, include/rtc.h "arbitrary output variables"):
    python tools/render_aov.py SCENE.yml OUTDIR [--near N --far F] [--exr [PLANES]] [--ao [RADIUS,USTEPS,VSTEPS]] [--ao-strength S]
                                                [--gather [RADIUS,USTEPS,VSTEPS]] [--gather-strength S]
                                                [--filter [PLANE_SIGMA,PASSES,NORMAL_SQUARINGS]]
writes OUTDIR/beauty.png (the colour frame) and depth.png, normal.png, index.png, shadow.png (rtc_aov_view_rgb8's pictures of
the planes). Colour frame, planes and pictures stay in device memory; every file is encoded there (ImageEncoder.encode_device)
and only the finished files cross PCIe — plus, when --near / --far are not both given, the depth plane, whose smallest and
largest finite value they default to. --exr also writes OUTDIR/frame.exr: ONE multi-channel OpenEXR file of data, not pictures —
the f64 colour frame as HALF R, G, B plus the planes asked for (a comma-separated list of depth, normal, point, index,
shadow; all five when none is named) as Z, N.*, P.*, id and shadow channels (FloatEncoder.encode_device, include/rtc.h
"float files"). --ao also renders the ambient-occlusion plane (include/rtc.h "ambient occlusion") — with the pass the scene's
camera asks for (ao-radius / ao-usteps / ao-vsteps) or the one given here — and writes OUTDIR/ao.png, the plane seen as a shadow
plane (white: open, black: every sample occluded), and OUTDIR/beauty_ao.png, the colour frame with every pixel multiplied by
1 - S * count / samples (rtc_canvas_apply_ao_device; S = --ao-strength, default 1), both made on the device. --gather also
renders the one-bounce gather pass (include/rtc.h "colour bleeding") — with the pass the scene's camera asks for
(gather-radius / gather-usteps / gather-vsteps) or the one given here — and writes OUTDIR/frame.png (the colour frame again,
through the f64 canvas), OUTDIR/bounce.png (the bounce plane as a picture) and OUTDIR/frame_bounce.png, the colour frame plus
S * bounce (rtc_canvas_add_scaled_device; S = --gather-strength, default 1), all made on the device. --filter, together with
--ao and / or --gather, also smooths their planes with the edge-aware filter (include/rtc.h "edge-aware filter") under the index,
point and normal planes of the same frame — with the filter the scene's camera asks for (filter-plane-sigma / filter-passes /
filter-normal-squarings), the one given here, or rtc.h's defaults — and writes OUTDIR/ao_filtered.png and
beauty_ao_filtered.png (rtc_counts_to_fraction_device, rtc_plane_filter_device, rtc_canvas_apply_occlusion_device),
OUTDIR/bounce_filtered.png and frame_bounce_filtered.png, and, with both passes, OUTDIR/frame_filtered.png: the colour frame times
the filtered occlusion plus the filtered bounce. A scene whose camera has a projection (projection: orthographic | panorama,
data/passes/orthographic_passes.yml) gives the same files under that camera's rays: the colour frame by
rtc_render_projection_rows, the planes by rtc_render_aov_projection_device and its kin. Needs an MI355X (there is no CPU
path)."""
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
    ap.add_argument("--ao", nargs="?", const="", default=None, metavar="RADIUS,USTEPS,VSTEPS")
    ap.add_argument("--ao-strength", type=float, default=1.0)
    ap.add_argument("--gather", nargs="?", const="", default=None, metavar="RADIUS,USTEPS,VSTEPS")
    ap.add_argument("--gather-strength", type=float, default=1.0)
    ap.add_argument("--filter", nargs="?", const="", default=None, metavar="PLANE_SIGMA,PASSES,NORMAL_SQUARINGS")
    args = ap.parse_args(argv[1:])
    rtc = package()
    abi = __import__("importlib").import_module(rtc.__name__ + ".abi")
    import numpy as np
    import torch
    proj = scene_ao = scene_gather = scene_filter = None
    try:
        world, cam = rtc.load_yaml(path=args.scene)
    except rtc.RtcError as refused:   # a camera with a projection: the entry that hands it out with the camera's passes
        world, cam, lens, proj, scene_ao, scene_gather, scene_filter = rtc.load_yaml_projection_passes(path=args.scene)
        if proj is None or lens is not None:
            raise refused
    ao = None
    if args.ao is not None:
        if args.ao:
            radius, usteps, vsteps = args.ao.split(",")
            ao = rtc.ao(float(radius), int(usteps), int(vsteps))
        else:
            ao = scene_ao if proj is not None else rtc.load_yaml_ao(path=args.scene)[3]
            if ao is None:
                ap.error("--ao: the scene's camera has no ao-radius; give RADIUS,USTEPS,VSTEPS")
    gather = None
    if args.gather is not None:
        if args.gather:
            radius, usteps, vsteps = args.gather.split(",")
            gather = rtc.ao(float(radius), int(usteps), int(vsteps))
        else:
            gather = scene_gather if proj is not None else rtc.load_yaml_gather(path=args.scene)[4]
            if gather is None:
                ap.error("--gather: the scene's camera has no gather-radius; give RADIUS,USTEPS,VSTEPS")
    flt = None
    if args.filter is not None:
        if ao is None and gather is None:
            ap.error("--filter smooths the planes of --ao and --gather: give at least one of them")
        if args.filter:
            sigma, passes, squarings = args.filter.split(",")
            flt = rtc.filter_spec(float(sigma), passes=int(passes), normal_squarings=int(squarings))
        else:
            flt = (scene_filter if proj is not None else rtc.load_yaml_filter(path=args.scene)[5]) or rtc.filter_spec()
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

    def render_rows(d_ptr, d_ptr8=None):   # the colour frame: the pinhole's, or the projection's
        if proj is None:
            dw.render_rows(cam, 0, height, d_ptr, d_ptr8=d_ptr8)
        else:
            dw.render_projection_rows(cam, proj, 0, height, d_ptr, d_ptr8=d_ptr8)

    render_rows(None, d_ptr8=pic.data_ptr())   # 8-bit rows only
    sizes["beauty"] = (out / "beauty.png").write_bytes(enc.encode_device("png", pic.data_ptr(), width, height, 3))
    dw.render_aov_device(cam, {p: t.data_ptr() for p, t in dev.items()}, projection=proj)
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
        render_rows(rgb.data_ptr())
        fenc = rtc.FloatEncoder(ctx)
        sizes["frame.exr"] = (out / "frame.exr").write_bytes(
            fenc.encode_device("exr", rgb.data_ptr(), width, height, {p: dev[p].data_ptr() for p in wanted}, "half"))
        fenc.close()
    guides = {p: dev[p].data_ptr() for p in ("index", "point", "normal")}   # what --filter smooths under
    filtered_frame = None
    if ao is not None:
        n = ao.usteps * ao.vsteps
        rgb = torch.zeros(width * height * 3, dtype=torch.float64, device="cuda:0")
        rgba = torch.zeros(width * height * 4, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dw.render_ao_device(cam, ao, dev["shadow"].data_ptr(), projection=proj)   # (the shadow plane's pictures are written: its buffer is free)
        ctx.aov_view_device("shadow", {"shadow": dev["shadow"].data_ptr()}, width, height, pic.data_ptr(), n_lights=n)
        sizes["ao"] = (out / "ao.png").write_bytes(enc.encode_device("png", pic.data_ptr(), width, height, 3))
        render_rows(rgb.data_ptr())
        ctx.apply_ao_device(rgb.data_ptr(), dev["shadow"].data_ptr(), n, args.ao_strength, width, height)
        ctx.canvas_to_rgba8_device(rgb.data_ptr(), width, height, 1.0, rgba.data_ptr())
        sizes["beauty_ao"] = (out / "beauty_ao.png").write_bytes(enc.encode_device("png", rgba.data_ptr(), width, height, 4))
        if flt is not None:
            occ, occ_f = (torch.zeros(width * height, dtype=torch.float64, device="cuda:0") for _ in range(2))
            torch.cuda.synchronize()
            ctx.counts_to_fraction_device(dev["shadow"].data_ptr(), n, width, height, occ.data_ptr())
            ctx.plane_filter_device(occ.data_ptr(), 1, guides, width, height, flt, occ_f.data_ptr())
            rgb.fill_(1.0)   # the plane as a picture: white times 1 - occlusion
            torch.cuda.synchronize()
            ctx.apply_occlusion_device(rgb.data_ptr(), occ_f.data_ptr(), 1.0, width, height)
            ctx.canvas_to_rgba8_device(rgb.data_ptr(), width, height, 1.0, rgba.data_ptr())
            sizes["ao_filtered"] = (out / "ao_filtered.png").write_bytes(enc.encode_device("png", rgba.data_ptr(), width, height, 4))
            render_rows(rgb.data_ptr())
            ctx.apply_occlusion_device(rgb.data_ptr(), occ_f.data_ptr(), args.ao_strength, width, height)
            ctx.canvas_to_rgba8_device(rgb.data_ptr(), width, height, 1.0, rgba.data_ptr())
            sizes["beauty_ao_filtered"] = (out / "beauty_ao_filtered.png").write_bytes(enc.encode_device("png", rgba.data_ptr(), width, height, 4))
            filtered_frame = rgb   # the colour frame times the filtered occlusion; --gather adds its filtered bounce
    if gather is not None:
        rgb = torch.zeros(width * height * 3, dtype=torch.float64, device="cuda:0")
        bounce = torch.zeros(width * height * 3, dtype=torch.float64, device="cuda:0")
        rgba = torch.zeros(width * height * 4, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def save(name, d_canvas):   # Color::scale at gamma 1, then the PNG, on the device
            ctx.canvas_to_rgba8_device(d_canvas, width, height, 1.0, rgba.data_ptr())
            sizes[name] = (out / f"{name}.png").write_bytes(enc.encode_device("png", rgba.data_ptr(), width, height, 4))

        render_rows(rgb.data_ptr())
        dw.render_gather_device(cam, gather, {"bounce": bounce.data_ptr()}, projection=proj)
        save("frame", rgb.data_ptr())
        save("bounce", bounce.data_ptr())
        ctx.add_scaled_device(rgb.data_ptr(), bounce.data_ptr(), args.gather_strength, width, height)
        save("frame_bounce", rgb.data_ptr())
        if flt is not None:
            bounce_f = torch.zeros(width * height * 3, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            ctx.plane_filter_device(bounce.data_ptr(), 3, guides, width, height, flt, bounce_f.data_ptr())
            save("bounce_filtered", bounce_f.data_ptr())
            render_rows(rgb.data_ptr())
            ctx.add_scaled_device(rgb.data_ptr(), bounce_f.data_ptr(), args.gather_strength, width, height)
            save("frame_bounce_filtered", rgb.data_ptr())
            if filtered_frame is not None:
                ctx.add_scaled_device(filtered_frame.data_ptr(), bounce_f.data_ptr(), args.gather_strength, width, height)
                save("frame_filtered", filtered_frame.data_ptr())
    hits = int((dev["index"] >= 0).sum().item())
    print(f"{out}: {width}x{height}{'' if proj is None else ', ' + ('orthographic' if proj.kind == rtc.PROJ_ORTHOGRAPHIC else 'panorama')}, {len(world)} shapes, {n_lights} light sample(s), {hits} of {width * height} pixels hit, "
          f"depth {near:.6g} .. {far:.6g}; bytes: " + ", ".join(f"{k if '.' in k else k + '.png'} {v}" for k, v in sizes.items()))
    enc.close()
    dw.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
