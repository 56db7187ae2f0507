"""Boundary cases on the HIP path (tests/boundary_cases.py): every probe case through rtc_color_at against the oracle, in
every object-source variant, without light lists, on the plain and the padded (two-level Morton cull) worlds; and every
render-level case (horizons and silhouettes on tile edges) binned against unbinned, sky rows off and brute force, bit for
bit, and against the oracle's render."""
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sibling(name):
    spec = importlib.util.spec_from_file_location("_bnd_gpu_" + name, Path(__file__).with_name(name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = m          # (dataclasses look their module up)
    spec.loader.exec_module(m)
    return m


B = _sibling("boundary_cases")
PARITY = _sibling("test_gpu_parity")   # VARIANTS / make_ctx / hit_fields / TIGHT_TOL: the parity suite's own definitions
TIGHT_TOL = PARITY.TIGHT_TOL
CASES, PAIRS = B.all_probe_cases()
RENDER = B.render_cases()


def env_ctx(rtc, **env):
    """A context created with the given RTC_* knobs set (they are read once, at rtc_context_create)."""
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        return rtc.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def world(rtc, shapes, lgt):
    w = rtc.World(lgt)
    w.shapes = list(shapes)     # world ids as the case set them (rtc_world_create honours them)
    return w


@pytest.fixture(scope="module")
def expected(O):
    """The oracle's literal form for every (case, padded, remaining)."""
    out = {}
    for ci, c in enumerate(CASES):
        for padded in (False, True):
            shapes = B.padded(c.shapes) if padded else c.shapes
            a = (O.RtcShape * len(shapes))(*shapes)
            for rem in (0, 5):
                out[ci, padded, rem] = [O.color_at(a, len(shapes), c.light, tuple(r), rem, want_hit=True) for r in c.rays]
    return out


def _check_probes(rtc, ctx, expected):
    bad = []
    for ci, c in enumerate(CASES):
        for padded in (False, True):
            dw = ctx.upload(world(rtc, B.padded(c.shapes) if padded else c.shapes, c.light))
            for rem in (0, 5):
                rgb, hits = dw.color_at(np.array(c.rays, dtype=np.float64), rem, want_hits=True)
                for i, (orgb, oh) in enumerate(expected[ci, padded, rem]):
                    if PARITY.hit_fields(hits[i]) != PARITY.hit_fields(oh) or not np.max(np.abs(rgb[i] - orgb)) <= TIGHT_TOL:
                        bad.append((c.name, "padded" if padded else "plain", rem, i, hits[i].hit_index, oh.hit_index,
                                    float(np.max(np.abs(rgb[i] - orgb)))))
            dw.close()
    return bad


@pytest.mark.parametrize("src,tile_cap", PARITY.VARIANTS)
def test_probe_cases_every_source(rtc, expected, src, tile_cap):
    ctx = PARITY.make_ctx(rtc, src, tile_cap)
    try:
        bad = _check_probes(rtc, ctx, expected)
    finally:
        ctx.close()
    assert not bad, f"{len(bad)} mismatches, first: {bad[:8]}"


def test_probe_cases_without_light_lists(rtc, expected):
    ctx = env_ctx(rtc, RTC_LIGHT_LISTS=0)
    try:
        bad = _check_probes(rtc, ctx, expected)
    finally:
        ctx.close()
    assert not bad, f"{len(bad)} mismatches, first: {bad[:8]}"


@pytest.mark.parametrize("mode", [0, 1], ids=["render", "render_async"])
def test_render_cases_binned_equals_unbinned_and_oracle(rtc, O, mode):
    """k_bin_tiles' tile lists and provably-black tile rows on horizons and silhouettes placed on tile edges: the binned
    render (RTC_BIN_SMALL_PIXELS=0) == sky rows off == binning off == brute force (RTC_FLAG_NO_CULL), canvases and ray
    counts bit for bit; == Camera::render / render_async of the oracle within TIGHT_TOL with equal ray counts."""
    ctxs = {"binned": env_ctx(rtc, RTC_BIN_SMALL_PIXELS=0), "no_sky_rows": env_ctx(rtc, RTC_BIN_SMALL_PIXELS=0, RTC_SKY_ROWS=0),
            "no_binning": env_ctx(rtc, RTC_BINNING=0)}
    try:
        for r in RENDER:
            assert r.cam.samples == 1
            outs = {}
            for name, ctx in ctxs.items():
                dw = ctx.upload(world(rtc, r.shapes, r.light))
                outs[name] = dw.render(r.cam, mode, with_stats=True)
                if name == "binned":
                    outs["no_cull"] = dw.render(r.cam, mode, flags=rtc.FLAG_NO_CULL, with_stats=True)
                dw.close()
            ref, rst = outs["binned"]
            for name, (img, st) in outs.items():
                assert np.array_equal(img, ref) and st == rst, (r.name, name, st, rst)
            want, ost = O.render(r.arr(), len(r.shapes), r.light, r.cam, mode=mode, nthreads=8, want_stats=True)
            assert np.max(np.abs(ref - want)) <= TIGHT_TOL and rst == ost, (r.name, rst, ost)
    finally:
        for ctx in ctxs.values():
            ctx.close()
