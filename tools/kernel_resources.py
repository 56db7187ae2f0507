"""Register / scratch / LDS use of every k_trace, k_aov, k_ao and k_gather instantiation (hipcc -Rpass-analysis=kernel-resource-usage); CPU only.
With --filter: of the edge-aware filter's kernels (csrc/rtc_filter.hip) instead; with --adaptive: of the adaptive anti-aliasing
kernels (csrc/rtc_adaptive.hip); with --post: of the post-processing kernels (csrc/rtc_post.hip); with --resize: of the resize
kernels (csrc/rtc_resize.hip; k_resize_h's LDS is dynamic, at most RTC_RESIZE_LDS_BUDGET, and is not in the remark).
usage: python tools/kernel_resources.py [--filter | --adaptive | --post | --resize] [extra -D flags]"""
import importlib.util
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
spec = importlib.util.spec_from_file_location("_rtc_build", ROOT / "raytracer-challenge_amd" / "build.py")
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)


FILTER = "--filter" in sys.argv[1:]
ADAPTIVE = "--adaptive" in sys.argv[1:]
POST = "--post" in sys.argv[1:]
RESIZE = "--resize" in sys.argv[1:]
EXTRA = [a for a in sys.argv[1:] if a not in ("--filter", "--adaptive", "--post", "--resize")]


def remarks(name):  # one kernel unit's remarks
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [*build.kernel_compile_line(), "-Rpass-analysis=kernel-resource-usage", *EXTRA, "-c", str(build.CSRC / name), "-o", tmp + "/k.o"]
        return subprocess.run(cmd, capture_output=True, text=True).stderr


with ThreadPoolExecutor(max_workers=build.jobs()) as pool:
    t = "".join(pool.map(remarks, build.FILTER_KERNEL_SOURCES if FILTER else [n for n in build.ADAPTIVE_SOURCES if n.endswith(".hip")] if ADAPTIVE
                         else [n for n in build.POST_SOURCES if n.endswith(".hip")] if POST
                         else [n for n in build.RESIZE_SOURCES if n.endswith(".hip")] if RESIZE else build.KERNEL_SOURCES))
PROJ = lambda name: ",proj>" if "DevProjection" in name else ">"  # the projection flavour of a tile pass (rtc_render_*_projection*)
rows = []
for blk in re.split(r"remark: [^\n]*Function Name: ", t)[1:]:
    name = blk.split("\n")[0].strip()
    if FILTER or ADAPTIVE or POST or RESIZE:
        pass
    elif "k_trace" not in name and "undeal" not in name and "k_aov" not in name and "k_ao" not in name and "k_apply_ao" not in name and "k_gather" not in name and "k_add_scaled" not in name:
        continue
    def g(k):
        m = re.search(k + r": (\d+)", blk)
        return m.group(1) if m else "?"
    m = re.search(r"k_traceILi(\d)ELb(\d)ELb(\d)ELb(\d)E(?:Lb(\d)E)?(?:Lb(\d)E)?(?:Lb(\d)E)?", name)
    if m:
        tag = "k_trace<%s,refl=%s,refr=%s,probe=%s" % m.groups()[:4] + (",rgba" if m.group(5) == "1" else "")
        tag += ",one" if m.group(6) == "1" else ""  # the one-sample flavour (cameras with samples == 1)
        tag += ",whole" if m.group(7) == "1" else ""  # the whole-tile flavour on top of it (one camera, whole tiles, f64 output)
        # the instantiations for Worlds with several lights: in the kernel arguments, or in the World's device table
        tag += ",multi" if "DevExtraLights" in name else ",table" if "DevLightTable" in name else ""
        # the per-lane twin of a kernel with the uniform shading path (RTC_UNIFORM_SHADE=0 at run time)
        tag += ",perlane" if "DevPerLaneShade" in name else ""
        # the thin-lens flavour (rtc_render_lens*) and the projection flavour (rtc_render_projection*)
        tag += ",lens>" if "DevLens" in name else ",proj>" if "DevProjection" in name else ">"
    elif (a := re.search(r"k_aovILi(\d)ELb(\d)E", name)):  # the AOV kernel: source, shadow passes, where the further lights come from
        tag = "k_aov<%s,shadow=%s" % a.groups() + (",multi" if "DevExtraLights" in name else ",table" if "DevLightTable" in name else "") + PROJ(name)
    elif "k_aov_view" in name:
        tag = "k_aov_view"
    elif (a := re.search(r"k_aoILi(\d)E", name)):  # the ambient-occlusion kernel: source
        tag = "k_ao<%s" % a.group(1) + PROJ(name)
    elif "k_apply_ao" in name:
        tag = "k_apply_ao"
    elif (a := re.search(r"k_gatherILi(\d)E", name)):  # the gather kernel: source, where the further lights come from
        tag = "k_gather<%s" % a.group(1) + (",multi" if "DevExtraLights" in name else ",table" if "DevLightTable" in name else "") + PROJ(name)
    elif "k_add_scaled" in name:
        tag = "k_add_scaled"
    elif (a := re.search(r"k_atrousILj(\d)ELb(\d)E", name)):  # the filter kernel: channels, RTC_FILTER_SAME_OBJECT
        tag = "k_atrous<%s,same=%s>" % a.groups()
    elif "k_counts_to_fraction" in name:
        tag = "k_counts_to_fraction"
    elif "k_apply_occlusion" in name:
        tag = "k_apply_occlusion"
    elif (a := re.search(r"(k_aa_[a-z]+)", name)):  # the adaptive anti-aliasing kernels
        tag = a.group(1)
    elif (a := re.search(r"(k_lum_[a-z]+|k_tonemap|k_bloom_[hv])", name)):  # the post-processing kernels
        tag = a.group(1)
    elif (a := re.search(r"(k_resize_[a-z]+)", name)):  # the resize kernels
        tag = a.group(1)
    else:
        tag = name[:44]
    scratch, occ, lds = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")
    rows.append(f"{tag:44s} VGPR {g('VGPRs'):>4s} SGPR {g('SGPRs'):>4s} scratch {scratch:>5s} occupancy {occ:>2s} LDS {lds:>6s}")
print("\n".join(sorted(rows)))
