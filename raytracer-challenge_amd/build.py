"""Build librtc.so (HIP kernels + C-ABI) for gfx950 with hipcc, in-tree.

`hipcc --offload-arch=gfx950` cross-compiles without a GPU. -ffp-contract=off is part of the
contract: the reference (rustc) never fuses a*b+c, and pixel/hit parity needs the same
roundings (SURVEY.md §7 "hard parts").
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor, as_completed
from functools import partial
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
LIB = PKG / "librtc.so"

# The render path's kernel sources, by far the longest compiles: first in SOURCES, so that they start first. The tools
# (tools/kernel_resources.py, the ISA listings for tools/isa_compare.py) run over exactly these.
KERNEL_SOURCES = ["rtc_kernels.hip"]
FILTER_KERNEL_SOURCES = ["rtc_filter.hip"]  # the edge-aware filter's kernels: tools/kernel_resources.py --filter
ADAPTIVE_SOURCES = ["host_adaptive.cpp", "rtc_adaptive.cpp", "rtc_adaptive.hip"]  # edge-adaptive anti-aliasing: tools/kernel_resources.py --adaptive
POST_SOURCES = ["host_post.cpp", "rtc_post.cpp", "rtc_post.hip"]  # exposure, tone mapping and bloom: tools/kernel_resources.py --post
RESIZE_SOURCES = ["host_resize.cpp", "rtc_resize.cpp", "rtc_resize.hip"]  # resizing f64 canvases: tools/kernel_resources.py --resize
SOURCES = KERNEL_SOURCES + ["host_math.cpp", "host_ppm.cpp", "host_yaml.cpp", "host_lua.cpp", "rtc_api.cpp", "rtc_launch_plan.cpp", "rtc_group.cpp", "rtc_world_build.hip", "host_gif.cpp", "rtc_gif.hip", "host_jpeg.cpp", "rtc_jpeg.hip", "host_png.cpp", "rtc_png.hip", "host_image.cpp", "rtc_image.hip", "rtc_encode.cpp", "rtc_lua_render.cpp", "rtc_shutter.cpp", "rtc_shutter.hip", "host_aov.cpp", "host_ao.cpp", "host_gather.cpp", "host_float.cpp", "rtc_float.hip", "host_filter.cpp", "rtc_filter.cpp", "rtc_filter.hip"] + ADAPTIVE_SOURCES + POST_SOURCES + RESIZE_SOURCES
COMMON = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}", f"-I{CSRC}"]
COMMON += os.environ.get("RTC_CXXFLAGS", "").split()  # experiments, e.g. -DRTC_WAVES_PER_SIMD=4
# Kernel file only: MachineLICM hoists the VGPR materialisation of every f64 literal (pow's ~25
# polynomial coefficients alone are 50 VGPRs) out of the per-sample loop to the kernel entry, where
# they stay live for the whole kernel: 128 VGPRs + 60 B/lane of scratch with it, 112 VGPRs and no
# scratch without (flat culled kernel); 0.129 ms -> 0.113 ms per north-star frame.
KERNEL_ONLY = ["-mllvm", "-disable-machine-licm"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (expected /opt/rocm/bin/hipcc)")


def kernel_compile_line() -> list[str]:
    """hipcc and the flags every .hip file is compiled with; the caller adds -c / -S, the source and the output."""
    return [hipcc(), "--offload-arch=gfx950", *COMMON, *KERNEL_ONLY]


def _stale(target: Path, deps: list[Path]) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(d.stat().st_mtime > t for d in deps)


def jobs() -> int:
    """How many compilers run at once: MAX_JOBS when set, else the CPU count; never more than 16."""
    return max(1, min(16, int(os.environ.get("MAX_JOBS") or os.cpu_count() or 1)))


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile every stale source to an object in build/, jobs() at a time, and link librtc.so next to this file."""
    cc = hipcc()
    objdir = ROOT / "build" / "rtc"
    objdir.mkdir(parents=True, exist_ok=True)
    headers = [ROOT / "include" / "rtc.h", *sorted(CSRC.glob("*.h"))]
    objs = [objdir / (name + ".o") for name in SOURCES]
    cmds = []
    for name, obj in zip(SOURCES, objs):
        src = CSRC / name
        if force or _stale(obj, [src] + headers):
            flags = kernel_compile_line() if name.endswith(".hip") else [cc, "--offload-arch=gfx950", *COMMON]
            cmds.append([*flags, "-c", str(src), "-o", str(obj)])

    def compile_one(cmd: list[str]) -> subprocess.CompletedProcess:
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    with ThreadPoolExecutor(max_workers=jobs()) as pool:
        for done in as_completed([pool.submit(compile_one, cmd) for cmd in cmds]):
            r = done.result()
            sys.stderr.write(r.stdout)  # each compiler's output in one piece, as soon as it has finished
            if r.returncode != 0:  # the first failure to finish is the one raised; queued compiles never start (the
                # `with` still waits for the compilers already running: their objects stay whole)
                pool.shutdown(wait=False, cancel_futures=True)
                r.check_returncode()
    if force or _stale(LIB, objs):
        cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(LIB), *map(str, objs), "-ldl"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
    return LIB


def _build_facade(name: str, force: bool = False) -> Path:
    """Compile tests/cpp/<name>.cpp, a program that drives the facade (host/ch1.hpp), against librtc.so."""
    src = ROOT / "tests" / "cpp" / (name + ".cpp")
    exe = ROOT / "build" / name
    hdr = PKG / "host" / "ch1.hpp"
    if not src.exists() or not hdr.exists():
        return None
    exe.parent.mkdir(parents=True, exist_ok=True)
    if force or _stale(exe, [src, hdr, LIB, ROOT / "include" / "rtc.h"]):
        cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'include'}", f"-I{PKG / 'host'}",
               str(src), "-o", str(exe), f"-L{PKG}", "-lrtc", f"-Wl,-rpath,{PKG}", "-Wl,-rpath,$ORIGIN/../raytracer-challenge_amd"]
        subprocess.run(cmd, check=True)
    return exe


# the fifteen programs, each callable as f(force=False) -> Path
build_facade_tests = partial(_build_facade, "test_facade")  # the C++ mirror of the reference API
build_facade_update_test = partial(_build_facade, "test_facade_update")  # the resident World updated in place
build_facade_area_light_test = partial(_build_facade, "test_facade_area_light")  # World::add_area_light
build_facade_lens_test = partial(_build_facade, "test_facade_lens")  # Camera::set_lens
build_facade_projection_test = partial(_build_facade, "test_facade_projection")  # Camera::set_projection
build_facade_shutter_test = partial(_build_facade, "test_facade_shutter")  # World::set_shape_motion / Camera::set_shutter
build_facade_aov_test = partial(_build_facade, "test_facade_aov")  # Camera::render_aov and Aov::view
build_facade_float_test = partial(_build_facade, "test_facade_float")  # Canvas::save of float files, Aov::save_exr
build_facade_ao_test = partial(_build_facade, "test_facade_ao")  # Camera::render_ao and Canvas::apply_ao
build_facade_gather_test = partial(_build_facade, "test_facade_gather")  # Camera::render_gather and Canvas::add_scaled
build_facade_filter_test = partial(_build_facade, "test_facade_filter")  # Aov::filter and Canvas::apply_occlusion
build_facade_adaptive_test = partial(_build_facade, "test_facade_adaptive")  # Camera::set_adaptive
build_facade_post_test = partial(_build_facade, "test_facade_post")  # Canvas::bloom and Canvas::tonemap
build_facade_resize_test = partial(_build_facade, "test_facade_resize")  # Canvas::resized
build_facade_projection_passes_test = partial(_build_facade, "test_facade_projection_passes")  # Camera::render_aov / render_ao / render_gather with a projection


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
