"""Hostile worlds through the multi-light, light-table, lens and AOV kernels (tests/adversarial_worlds.py holds the worlds,
the case table and the oracle's references; tests/test_host_adversarial_worlds.py checks on the CPU that no case is vacuous).

Every case is compared with BOTH references, whole frames, nothing sampled:
  - the CPU oracle: a world of n light samples against the sum of the oracle's single-light frames in sample order, bound
    n x 1e-12 (the project's TIGHT_TOL rule), equal zero pattern; AOV planes against the oracle's hit records, exactly;
  - the RTC_FLAG_NO_CULL launch of the same world (SRC_SMEM): the same canvas bytes and the same rtc_stats.
After each k_trace launch rtc_context_last_launch_info must name the instantiation the case stands for (source, reflective,
refractive, light_table, lens_samples) and the World must hold the case's number of light samples. AOV launches leave the
launch info alone (rtc_render_aov_device), so for k_aov the test asserts what selects the instantiation: the object count
(SRC_CULL up to 256 objects, SRC_CULL2 above, SRC_SMEM under RTC_FLAG_NO_CULL) and the light count (one light, up to 8:
kernel arguments, above: the device table)."""
import numpy as np
import pytest

import adversarial_worlds as A
import aov_cases

pytestmark = pytest.mark.gpu

TIGHT_TOL = A.TIGHT_TOL
NO_CULL = A.NO_CULL


def _launch(gpu, rtc, dw, cam, lens_spec, flags=0):
    """(canvas, stats, launch info) of one k_trace launch"""
    if lens_spec is None:
        got, st = dw.render(cam, rtc.MODE_RENDER_ASYNC, flags=flags, with_stats=True)
    else:
        got, st = dw.render_lens(cam, rtc.lens(*lens_spec), rtc.MODE_RENDER_ASYNC, flags=flags, with_stats=True)
    return got, st, gpu.last_launch_info()


def _assert_ran(info, case, lens_spec, source):
    want = {"source": source, "reflective": case.shading != "flat", "refractive": case.shading == "refr",
            "light_table": case.light_form == "table", "lens_samples": lens_spec[2] * lens_spec[3] if lens_spec else 0}
    assert {k: info[k] for k in want} == want, (case.name, info)


def _colour_case(rtc, gpu, O, case):
    facts = A.check_class(rtc, O, case)   # the case is of its class and its reference is not trivial (host data only)
    w, cam, lens_spec, samples, key = A.build(rtc, O, case)
    n = len(samples)
    dw = gpu.upload(w)
    try:
        assert rtc.lib().rtc_world_light_count(dw._h) == n
        got, st, info = _launch(gpu, rtc, dw, cam, lens_spec)
        brute, sb, info_b = _launch(gpu, rtc, dw, cam, lens_spec, NO_CULL)
    finally:
        dw.close()
    _assert_ran(info, case, lens_spec, case.source)
    _assert_ran(info_b, case, lens_spec, A.SRC_SMEM)
    assert got.tobytes() == brute.tobytes(), (case.name, float(np.max(np.abs(got - brute))))
    assert all(st[k] == sb[k] for k in A.COUNTERS), (case.name, st, sb)
    ref = A.reference(rtc, O, case)
    err = float(np.max(np.abs(got - ref)))
    print(f"{case.name}: {facts}; launch {info['source_name']} refl={info['reflective']} refr={info['refractive']} table={info['light_table']} "
          f"lens={info['lens_samples']}; max|gpu - sum(oracle_i)| = {err:.3e} (bound {n * TIGHT_TOL:.1e})")
    assert err <= n * TIGHT_TOL, (case.name, err)
    assert np.array_equal(got != 0, ref != 0), case.name
    pixels = cam.hsize * cam.vsize
    assert st["pixels"] == pixels
    if lens_spec is None:   # every counter but the shadow rays as for one light; one shadow ray per sample per shade_hit
        o1 = A.oracle_stats(rtc, O, key, w, cam, samples[0])
        assert all(st[k] == o1[k] for k in A.COUNTERS if k != "rays_shadow"), (case.name, st, o1)
        assert st["rays_shadow"] == n * o1["rays_shadow"] and o1["rays_shadow"] > 0, (case.name, st, o1)
    else:
        assert st["rays_primary"] == pixels * lens_spec[2] * lens_spec[3] and st["rays_primary_proven_miss"] == 0, (case.name, st)
    return got, st


def _assert_same_planes(got, want, what):
    bad = aov_cases.same_planes(got, want)
    detail = ""
    for p in bad:
        d = np.argwhere(got[p] != want[p])
        detail += f" {p}: {len(d)} entries differ, first at {d[0].tolist() if len(d) else '?'}"
    assert bad == [], what + detail


def _aov_case(rtc, gpu, O, case):
    facts = A.check_class(rtc, O, case)
    w, cam, _, samples, key = A.build(rtc, O, case)
    want = A.expected_planes(rtc, O, key, w, cam, samples, case.mode)
    # what selects k_aov's instantiation
    assert (len(w) > 256) == (case.source == A.SRC_CULL2 or (case.source == A.SRC_SMEM and case.geometry == "two"))
    dw = gpu.upload(w)
    try:
        assert rtc.lib().rtc_world_light_count(dw._h) == len(samples)
        culled = dw.render_aov(cam, A.PLANES, case.mode)
        brute = dw.render_aov(cam, A.PLANES, case.mode, NO_CULL)
    finally:
        dw.close()
    print(f"{case.name}: {facts}")
    _assert_same_planes(culled, want, case.name)
    _assert_same_planes(brute, want, case.name + " no-cull")
    if case.mode == A.MODE_RENDER:
        assert (want["index"][-1, :] == -1).all() and (want["index"][:, -1] == -1).all()


# ---- a. the instantiation matrix
@pytest.mark.parametrize("name", A.names("matrix"))
def test_every_k_trace_cell_of_the_matrix_on_a_hostile_world(rtc, gpu, O, name):
    _colour_case(rtc, gpu, O, A.BY_NAME[name])


@pytest.mark.parametrize("name", A.names("aov_matrix"))
def test_every_k_aov_shadow_cell_of_the_matrix_on_a_hostile_world(rtc, gpu, O, name):
    _aov_case(rtc, gpu, O, A.BY_NAME[name])


# ---- b. hostile lights, pinhole
@pytest.mark.parametrize("name", A.names("lights"))
def test_hostile_lights(rtc, gpu, O, name):
    """Each hostile light as the second of two, all eight at once (the kernel-argument cap), and the three hostile
    rectangles of nine samples (the smallest table), on the one-level and the two-level world in their REFR form."""
    _colour_case(rtc, gpu, O, A.BY_NAME[name])


# ---- c. hostile lenses
@pytest.mark.parametrize("name", A.names("lens"))
def test_hostile_lenses(rtc, gpu, O, name):
    _colour_case(rtc, gpu, O, A.BY_NAME[name])


# ---- d. AOV planes on hostile worlds
@pytest.mark.parametrize("name", A.names("aov"))
def test_aov_planes_on_hostile_worlds(rtc, gpu, O, name):
    _aov_case(rtc, gpu, O, A.BY_NAME[name])


# ---- e. a resident world that got there by update
@pytest.mark.parametrize("name", A.names("update"))
def test_an_updated_world_renders_the_cell_like_a_fresh_upload(rtc, gpu, O, name):
    """A different world first (other shapes, other object count, one light), then DeviceWorld.update to the cell's world
    (tables rebuilt on the device): the bytes and the stats of the fresh upload, which in turn match both references."""
    case = A.BY_NAME[name]
    fresh, fresh_st = _colour_case(rtc, gpu, O, case)
    w, cam, lens_spec, samples, _ = A.build(rtc, O, case)
    other, other_cam = A.shaded(rtc, "inside" if case.geometry == "one" else "far", "refl")
    assert len(other) != len(w) and (len(other) > 256) == (len(w) > 256)
    dw = gpu.upload(other)
    try:
        first, _, _ = _launch(gpu, rtc, dw, other_cam, lens_spec)
        dw.update(w)
        assert rtc.lib().rtc_world_light_count(dw._h) == len(samples)
        got, st, info = _launch(gpu, rtc, dw, cam, lens_spec)
        brute, sb, info_b = _launch(gpu, rtc, dw, cam, lens_spec, NO_CULL)
    finally:
        dw.close()
    _assert_ran(info, case, lens_spec, case.source)
    _assert_ran(info_b, case, lens_spec, A.SRC_SMEM)
    assert got.tobytes() == fresh.tobytes() and st == fresh_st and got.tobytes() != first.tobytes()
    assert brute.tobytes() == fresh.tobytes() and all(sb[k] == fresh_st[k] for k in A.COUNTERS)
