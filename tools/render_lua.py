"""The reference's `render_lua(script)` (ch1/src/lua.rs:50-91) from the command line: run a Lua scene script through the
library's interpreter, render every Render / AddFrame call on the GPU, write the frames (PNG; PPM for ".ppm" names).
    python tools/render_lua.py [--gif | --jpeg | --png-deflate | --saved] SCRIPT.lua [OUT_DIR]
By default every AddFrame frame is a numbered PNG; with --gif each StartAnimation call becomes one animated GIF, encoded
on the GPU; with --jpeg every file gets the name the script gave it: ".jpg" / ".jpeg" stills as JPEG (quality 75) and the
animations as GIFs, both encoded on the GPU; with --png-deflate the default names and layout, every PNG filtered and
deflate-compressed on the GPU (only the file crosses PCIe); with --saved every still under the script's name in the format its
extension names (BMP, TGA, TIFF, ICO, farbfeld, PAM, PNG, JPEG, GIF, PPM) and the animations as GIFs, all encoded on the GPU.
Needs an MI355X (there is no CPU path); prints what the script printed and the files written."""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from _bootstrap import package  # noqa: E402


def main(argv):
    gif, jpeg, deflate, saved = "--gif" in argv, "--jpeg" in argv, "--png-deflate" in argv, "--saved" in argv
    argv = [a for a in argv if a not in ("--gif", "--jpeg", "--png-deflate", "--saved")]
    if len(argv) < 2:
        print(__doc__)
        return 2
    rtc = package()
    prog = rtc.LuaProgram(path=argv[1])
    sys.stdout.write(prog.output)
    ctx = rtc.Context(0)
    t = time.perf_counter()
    out = argv[2] if len(argv) > 2 else "."
    if jpeg:
        paths = prog.render_reference_files(ctx, out)
    elif deflate:
        paths = prog.render_png_files(ctx, out)
    elif saved:
        paths = prog.render_saved_files(ctx, out)
    else:
        paths = prog.render_animations(ctx, out) if gif else prog.render_to_files(ctx, out)
    dt = time.perf_counter() - t
    for p in paths:
        print(p)
    print(f"{len(paths)} frames in {dt * 1e3:.1f} ms (rendering + PCIe + file writes)")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
