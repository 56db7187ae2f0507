"""Shade-domain cases on the HIP path (tests/shade_domain_cases.py): materials and lights with NaN, +-inf, signed zeros,
subnormals, negatives and 1e+-300 where the shade stage decides something, against the oracle.

Every case runs through rtc_color_at on the 153 pixel-centre rays (the PROBE kernels: colour and hit record), rtc_render
culled and rtc_render with RTC_FLAG_NO_CULL, on the small world and on the world padded past 256 objects (the two-level
kernels). rtc_context_last_launch_info must show the flavour the reference's comparisons imply: a NaN-reflective world
runs a reflective kernel. Per channel: NaN where the oracle has NaN, +-inf with its sign, and the finite channels
bit-identical to the oracle's unless the case itself makes the colour depend on a rounded pow (then within
(K + 60) ulp, K the bound tests/test_gpu_parity.py asserts for pow at that shininess). The ray counters are the oracle's and
the culled frame is the brute-force frame byte for byte. Two cases per group also go through a 2x1 lens and through
DeviceWorld.update from the plain scene.

Measured on the MI355X, largest |gpu - oracle| / |oracle| per group: see DESIGN.md section 2."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sibling(name):
    spec = importlib.util.spec_from_file_location("_shd_gpu_" + name, Path(__file__).with_name(name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m          # (dataclasses look their module up)
    spec.loader.exec_module(m)
    return m


S = _sibling("shade_domain_cases")
CASES = S.all_cases()
NO_CULL = 1
LENS = (0.05, 5.0, 2, 1)                # aperture, focal distance, 2 x 1 samples
TWO_LEVEL, BRUTE = (4,), (0, 1, 2)       # rtc_launch_info.source: the two-level per-wave cull; the brute-force sources


def world(rtc, case, padded):
    w = rtc.World([rtc.light(position=p, intensity=i) for p, i in case.lights])
    w.shapes = case.shapes(padded)      # world ids as the case set them
    return w


def counters(st):
    return {k: st[k] for k in S.COUNTERS}


@pytest.fixture(scope="module")
def expected(O):
    """Per case, on the small world (the padded world's oracle frame is the same: tests/test_host_shade_domain.py):
    (frame, counters, color_at colours, hit records, the |terms| frame or None). Computed once, never written to."""
    out = {}
    cam = S.camera()
    for c in CASES:
        f, st = S.oracle_frame(c, cam)
        rgb, hits = S.oracle_probes(c, cam)
        a = S.oracle_frame(c.absolute(), cam)[0] if (not c.exact() and c.negative_terms()) else None
        for x in (f, rgb) + ((a,) if a is not None else ()):
            x.setflags(write=False)
        out[c.name] = (f, st, rgb, hits, a)
    return out


def check_flavour(case, info, source=None, lens_samples=0):
    bad = []
    want = (case.reflects() or case.refracts(), case.refracts())       # refractive Worlds carry the full frame stack
    if (info["reflective"], info["refractive"]) != want:
        bad.append(f"launched refl={info['reflective']} refr={info['refractive']}, the reference's comparisons imply {want}")
    if source is not None and info["source"] not in source:
        bad.append(f"source {info['source']} ({info['source_name']}), expected one of {source}")
    if info["light_table"] != (len(case.lights) > 8) or info["lens_samples"] != lens_samples:
        bad.append(f"light_table={info['light_table']} lens_samples={info['lens_samples']}")
    return bad


def run_routes(rtc, gpu, case, cam, f, st, rgb, hits, a):
    """-> (complaints, largest relative difference)"""
    bad, worst = [], 0.
    rays = np.array(S.pixel_rays(cam))
    for padded in (False, True):
        tag = "padded" if padded else "small"
        dw = gpu.upload(world(rtc, case, padded))
        try:
            g_rgb, g_hits = dw.color_at(rays, 5, want_hits=True)
            b_rgb, b_hits = dw.color_at(rays, 5, want_hits=True, flags=NO_CULL)
            got, gst = dw.render(cam, with_stats=True)
            info = gpu.last_launch_info()
            brute, bst = dw.render(cam, flags=NO_CULL, with_stats=True)
            info_b = gpu.last_launch_info()
        finally:
            dw.close()
        for route, x in (("color_at", g_rgb.reshape(f.shape)), ("color_at NO_CULL", b_rgb.reshape(f.shape)), ("render", got), ("render NO_CULL", brute)):
            c, rel = S.compare(case, x, rgb.reshape(f.shape) if route.startswith("color_at") else f, a)
            bad += [f"{tag} {route}: {m}" for m in c]
            worst = max(worst, rel)
        for route, hh in (("color_at", g_hits), ("color_at NO_CULL", b_hits)):
            n = sum(S.hit_key(hh[i]) != S.hit_key(hits[i]) for i in range(len(hits)))
            if n:
                bad.append(f"{tag} {route}: {n} hit records differ from the oracle's")
        if counters(gst) != st or counters(bst) != st:
            bad.append(f"{tag}: rtc_stats {counters(gst)} (NO_CULL {counters(bst)}), the oracle counts {st}")
        if got.tobytes() != brute.tobytes():
            bad.append(f"{tag}: the culled frame is not the brute-force frame byte for byte")
        bad += [f"{tag} render: {m}" for m in check_flavour(case, info, TWO_LEVEL if padded else None)]
        bad += [f"{tag} render NO_CULL: {m}" for m in check_flavour(case, info_b, BRUTE)]
    return bad, worst


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_through_every_route(rtc, gpu, expected, case):
    bad, worst = run_routes(rtc, gpu, case, S.camera(), *expected[case.name])
    print(f"{case.group} {case.name} ({case.line}): {'exact' if case.exact() else 'pow'} class, largest |gpu - oracle| / |oracle| = {worst:.3e}")
    assert not bad, (case.name, bad)


@pytest.mark.parametrize("name", S.WIDE_FRAME)
def test_case_at_20x12(rtc, gpu, O, name):
    """More than one tile across, a partial tile on both edges."""
    case, cam = S.by_name(name), S.camera(20, 12)
    f, st = S.oracle_frame(case, cam)
    rgb, hits = S.oracle_probes(case, cam)
    assert int(np.isnan(f).sum()) >= 30
    bad, worst = run_routes(rtc, gpu, case, cam, f, st, rgb, hits, None)
    print(f"{case.group} {name} at 20x12: largest |gpu - oracle| / |oracle| = {worst:.3e}")
    assert not bad, (name, bad)


def oracle_lens_frame(rtc, O, case, cam, lens):
    """Color::average_over of the lens samples (sums from 0.0 in sample order, one division), each sample the sum over the
    lights in light order of the oracle's color_at of rtc_lens_ray's ray: the order the kernel adds in."""
    shapes = case.shapes()
    arr, lights = S.arr(shapes), case.light_list()
    ns = lens.usteps * lens.vsteps
    out = np.zeros((cam.vsize, cam.hsize, 3))
    for y in range(cam.vsize):
        for x in range(cam.hsize):
            acc = np.zeros(3)
            for k in range(ns):
                ray = tuple(rtc.lens_ray(cam, lens, x, y, k))
                c = None
                for lgt in lights:
                    one = O.color_at(arr, len(shapes), lgt, ray, 5)
                    c = one if c is None else c + one
                acc = acc + c
            out[y, x] = acc / float(ns)
    return out


@pytest.mark.parametrize("name", S.REPRESENTATIVES)
def test_representatives_through_a_2x1_lens(rtc, gpu, O, name):
    case, cam, lens = S.by_name(name), S.camera(), rtc.lens(*LENS)
    want = oracle_lens_frame(rtc, O, case, cam, lens)
    a = oracle_lens_frame(rtc, O, case.absolute(), cam, lens) if (not case.exact() and case.negative_terms()) else None
    if case.nonfinite and case.group != "rde" and name != "position[over_point]":   # (those two are about ONE pixel-centre ray)
        assert not np.isfinite(want).all()
    bad, worst = [], 0.
    for padded in (False, True):
        dw = gpu.upload(world(rtc, case, padded))
        try:
            got, gst = dw.render_lens(cam, lens, with_stats=True)
            info = gpu.last_launch_info()
            brute, bst = dw.render_lens(cam, lens, flags=NO_CULL, with_stats=True)
        finally:
            dw.close()
        c, rel = S.compare(case, got, want, a)
        bad += [f"{'padded' if padded else 'small'} lens: {m}" for m in c]
        worst = max(worst, rel)
        if got.tobytes() != brute.tobytes() or gst != bst:
            bad.append("the culled lens frame or its counters differ from the brute-force ones")
        if gst["rays_primary"] != 2 * cam.hsize * cam.vsize or gst["pixels"] != cam.hsize * cam.vsize:
            bad.append(f"lens counters {gst}")
        bad += check_flavour(case, info, TWO_LEVEL if padded else None, lens_samples=2)
    print(f"{case.group} {name} through a 2x1 lens: largest |gpu - oracle| / |oracle| = {worst:.3e}")
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", S.REPRESENTATIVES)
def test_representatives_through_update_from_the_plain_scene(rtc, gpu, expected, name):
    """rtc_world_update rebuilds the tables on the device and decides the flavour again: a resident plain World updated to
    the case renders the bytes, counters and flavour of a World created from the case (compared with the oracle above)."""
    case, cam = S.by_name(name), S.camera()
    f, st, _, _, a = expected[name]
    for padded in (False, True):
        fresh = gpu.upload(world(rtc, case, padded))
        dw = gpu.upload(world(rtc, S.PLAIN, padded))
        try:
            want, wst = fresh.render(cam, with_stats=True)
            plain = dw.render(cam)
            assert np.isfinite(plain).all() and gpu.last_launch_info()["reflective"] is False
            dw.update(world(rtc, case, padded))
            got, gst = dw.render(cam, with_stats=True)
            info = gpu.last_launch_info()
        finally:
            fresh.close()
            dw.close()
        assert got.tobytes() == want.tobytes() and gst == wst and counters(gst) == st, (name, padded, gst, st)
        assert not check_flavour(case, info, TWO_LEVEL if padded else None), (name, padded, info)
        assert not S.compare(case, got, f, a)[0], (name, padded)
