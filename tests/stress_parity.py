"""One-off stress campaign (not part of the test suite): many random adversarial worlds, the culled
kernels (one- and two-level) against plain brute force on the GPU, bit for bit (canvas + ray counts);
every 10th world also against the CPU oracle. Usage: python tests/stress_parity.py [n_worlds] [seed0] [pipeline_depth] [flavour]
(RTC_BIN_SMALL_PIXELS=0 / RTC_BIN_SMALL_PIXELS_PIPELINED=0 in the environment force the binned primary pass on these small frames.)

flavour: `pinhole` (default) renders each world as it is, with its one light, through rtc_render. The others put the same
worlds through the kernels behind it, at 52x37 (partial tiles on both edges; tests/adversarial_worlds.py):
  lights — 2 to 9 light samples: the world's own light and hostile_lights drawn by the seed, or (9) a hostile rectangle;
  lens   — one of hostile_lenses, drawn by the seed;
  aov    — all six AOV planes under a light set as for `lights`.
Every world: culled against RTC_FLAG_NO_CULL, bit for bit; every 10th also against the oracle's reference (the summed
single-light frames within n x 1e-12 and the zero pattern; the hit records' planes exactly). The script ends at the first
call that returns a status other than RTC_OK or raises: nothing is caught."""
import importlib
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "oracle"), str(ROOT / "tests")]
import oracle as O  # noqa: E402
from _bootstrap import package  # noqa: E402

rtc = package()
import adversarial_worlds as A  # noqa: E402
from adversarial_worlds import adversarial_scene  # noqa: E402

n_worlds = int(sys.argv[1]) if len(sys.argv) > 1 else 300
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
pipeline = int(sys.argv[3]) if len(sys.argv) > 3 else 1
flavour = sys.argv[4] if len(sys.argv) > 4 else "pinhole"
if flavour not in ("pinhole", "lights", "lens", "aov"):
    sys.exit(f"unknown flavour {flavour!r}: pinhole, lights, lens or aov")


def big_world(seed): return A.big_world(rtc, seed)
def far_world(seed): return A.far_world(rtc, seed)
def mirror_world(seed): return A.mirror_world(rtc, seed)
def list_family(seed): return A.list_family(rtc, seed)


def light_set(w, cam, seed):
    """2 .. 9 light samples for world `w`, drawn by the seed: (lights, description)."""
    rng = np.random.default_rng([seed, 77])
    n = int(rng.integers(2, 10))
    if n == 9:
        name = A.HOSTILE_AREA_LIGHTS[int(rng.integers(0, 3))]
        return [A.hostile_area_light(rtc, w)[name]], "area:" + name
    hl = A.hostile_lights(rtc, O, w, cam, seed)
    picked = [A.HOSTILE_LIGHTS[i] for i in rng.permutation(len(A.HOSTILE_LIGHTS))[:n - 1]]
    return [w.light] + [hl[k] for k in picked], "+".join(picked)


def check_colour(dw, w, cam, lens_spec, samples, seed, k):
    """-> (ok, text): culled == brute force bit for bit; every 10th world also against the oracle."""
    lens = rtc.lens(*lens_spec) if lens_spec else None
    if lens is None:
        got, st = dw.render(cam, rtc.MODE_RENDER_ASYNC, with_stats=True)
        brute, sb = dw.render(cam, rtc.MODE_RENDER_ASYNC, flags=1, with_stats=True)
    else:
        got, st = dw.render_lens(cam, lens, rtc.MODE_RENDER_ASYNC, with_stats=True)
        brute, sb = dw.render_lens(cam, lens, rtc.MODE_RENDER_ASYNC, flags=1, with_stats=True)
    ok = got.tobytes() == brute.tobytes() and st == sb
    text = f"max|d|={np.max(np.abs(got - brute)):.3e} stats {st} vs {sb}"
    if ok and k % 10 == 0:
        ref = A.oracle_sum(rtc, O, ("stress", seed), w, cam, samples, lens_spec)
        err = float(np.max(np.abs(got - ref)))
        worst[0] = max(worst[0], err / len(samples))
        ok = err <= len(samples) * A.TIGHT_TOL and np.array_equal(got != 0, ref != 0)
        if ok and lens is None:
            o1 = A.oracle_stats(rtc, O, ("stress", seed), w, cam, samples[0])
            ok = all(st[c] == o1[c] for c in A.COUNTERS if c != "rays_shadow") and st["rays_shadow"] == len(samples) * o1["rays_shadow"]
        text = f"against the oracle: max|d|={err:.3e} ({len(samples)} samples)"
        A._frames.clear()
    return ok, text


def check_aov(dw, w, cam, samples, seed, k):
    import aov_cases
    culled = dw.render_aov(cam)
    brute = dw.render_aov(cam, flags=1)
    bad = aov_cases.same_planes(culled, brute)
    text = f"planes {bad} differ from brute force"
    if not bad and k % 10 == 0:
        want = A.expected_planes(rtc, O, ("stress", seed), w, cam, samples, A.MODE_RENDER_ASYNC)
        bad = aov_cases.same_planes(culled, want)
        text = f"planes {bad} differ from the oracle's records"
        A._hits.clear()
    return not bad, text


ctx = rtc.Context(0)
if pipeline > 1:
    ctx.set_pipeline(pipeline)
bad = 0
worst = [0.0]   # the largest |gpu - oracle| per light sample seen
t0 = time.time()
for k in range(n_worlds):
    seed = seed0 + k
    w, cam = list_family(seed) if k % 7 == 6 else mirror_world(seed) if k % 5 == 4 else (far_world(seed) if k % 4 == 3 else (big_world(seed) if k % 3 == 2 else adversarial_scene(rtc, seed)))
    if flavour == "pinhole":
        dw = ctx.upload(w)
        got, st = dw.render(cam, rtc.MODE_RENDER_ASYNC, with_stats=True)
        brute, sb = dw.render(cam, rtc.MODE_RENDER_ASYNC, flags=1, with_stats=True)
        ok = np.array_equal(got, brute) and st == sb
        if ok and k % 10 == 0:
            want, ost = O.render(w.array(), len(w), w.light, cam, mode=1, nthreads=16, want_stats=True)
            ok = float(np.max(np.abs(got - want))) <= 1e-12 and st == ost
        if not ok:
            bad += 1
            print(f"MISMATCH seed {seed} objects {len(w)} max|d|={np.max(np.abs(got - brute)):.3e} stats {st} vs {sb}", flush=True)
        dw.close()
    else:
        cam = A.recamera(rtc, cam, *A.FRAME)
        lens_spec, what = None, ""
        if flavour == "lens":
            lenses = A.hostile_lenses(rtc, w, cam)
            what = list(lenses)[int(np.random.default_rng([seed, 78]).integers(0, len(lenses)))]
            lens_spec, cam = lenses[what]
            m = w
        else:
            lights, what = light_set(w, cam, seed)
            m = A.with_lights(rtc, w, lights)
        samples = tuple(A.sample_key(s) for s in m.samples())
        dw = ctx.upload(m)
        ok, text = check_aov(dw, m, cam, samples, seed, k) if flavour == "aov" else check_colour(dw, m, cam, lens_spec, samples, seed, k)
        if not ok:
            bad += 1
            print(f"MISMATCH {flavour} seed {seed} objects {len(w)} {what}: {text}", flush=True)
        dw.close()
    if k % 2000 == 1999:
        print(f"{k + 1} worlds, {bad} mismatches, {time.time() - t0:.0f}s", flush=True)
if flavour != "pinhole":
    print(f"{flavour}: {n_worlds} worlds from seed {seed0}, {bad} mismatches, {time.time() - t0:.0f}s, largest |gpu - oracle| per sample {worst[0]:.3e} (bound {A.TIGHT_TOL:.0e})")
print(f"done: {n_worlds} worlds, {bad} mismatches")
sys.exit(1 if bad else 0)
