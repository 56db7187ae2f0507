"""The launch plan and the launches: after a real launch, every field of rtc_context_last_launch_info that the plan determines
equals rtc_debug_plan_launch for the same inputs (tests/launch_plan.py), and the frame equals the RTC_FLAG_NO_CULL frame of
the same world. tests/test_host_launch_plan.py pins the plan itself, without a device; this ties it to what runs.

Small on purpose: 70x45 frames (partial tiles on both edges, 54 tiles), worlds of 0, 3, 40 and 300 objects (nothing, one
level, light lists, two levels), one reflective and one refractive world."""
import importlib
import os

import numpy as np
import pytest

import adversarial_worlds as A
import aov_cases
import launch_plan as L

pytestmark = pytest.mark.gpu

W, H = 70, 45
ROWS = 48          # view_rows of a two-view launch: six bands of 8
DEV = "cuda:0"
FLAGS = (0, L.NO_CULL, L.NO_CULL | L.LDS_TABLE)


@pytest.fixture(scope="module")
def worlds(rtc):
    S = importlib.import_module(rtc.__name__ + ".scenes")
    out = {"empty": rtc.World(), "three": S.synthetic(2, W, H)[0], "forty": S.synthetic(39, W, H)[0], "big": S.synthetic(299, W, H)[0],
           "mirror": S.synthetic(39, W, H, reflective=True)[0], "glass": S.glass_cluster(40, W, H)[0]}
    out["two lights"] = S.synthetic(2, W, H)[0].add_light(rtc.light(position=(6.0, 9.0, -4.0), intensity=(0.6, 0.5, 0.4)))
    out["two lights, big"] = S.synthetic(299, W, H)[0].add_light(rtc.light(position=(6.0, 9.0, -4.0), intensity=(0.6, 0.5, 0.4)))
    assert [len(out[k]) for k in ("empty", "three", "forty", "big")] == [0, 3, 40, 300]
    return out


def cameras(rtc, samples=1):
    M = rtc.Matrix
    return [rtc.camera(W, H, 0.7, M.make_view_transform(frm, (0.0, 1.0, 5.0), (0.0, 1.0, 0.0)), samples)
            for frm in ((0.0, 2.0, -8.0), (1.5, 2.5, -7.0))]


def facts(w):
    """What the plan needs to know of a World (rtc_world_create derives the same: shape.rs:730, 752)."""
    shapes = w.array()[:len(w)] if len(w) else []
    refr = any(s.material.transparency != 0.0 for s in shapes)
    return dict(n=len(w), n_lights=len(w.lights), any_refl=int(any(s.material.reflective > 0.0 for s in shapes)), any_refr=int(refr))


def canvas(rows=H):
    import torch
    return torch.full((rows, W, 3), -1.0, dtype=torch.float64, device=DEV)


def assert_planned(rtc, ctx, w, knobs, lane=0, **request):
    """The launch the context made last is the one the plan describes."""
    p = L.plan(rtc, hsize=W, vsize=H, **facts(w), **knobs, **request)
    info = ctx.last_launch_info()
    got = {k: info[k] for k in ("source", "reflective", "refractive", "binned_primary_pass", "threads_per_workgroup", "dynamic_lds_bytes",
                                "tiles_per_workgroup", "multi_tile_workgroups", "light_table", "lens_samples", "lane")}
    want = {"source": p.src, "reflective": bool(p.refl), "refractive": bool(p.refr), "binned_primary_pass": bool(p.bin),
            "threads_per_workgroup": p.block, "dynamic_lds_bytes": p.lds_bytes, "tiles_per_workgroup": p.reps,
            "multi_tile_workgroups": sum(L.chunks(p)), "light_table": False, "lens_samples": request.get("lens_samples", 0),
            "lane": lane if p.lane_dealt else 0}
    assert p.status == L.OK and got == want, (request, got, want)
    return p


def render(rtc, ctx, dw, w, cam, flags, knobs, lens=None, lane=0):
    """One frame in one launch, checked against its plan; the canvas."""
    out = canvas()
    if lens is None:
        dw.render_rows(cam, 0, H, out.data_ptr(), flags=flags)
        assert_planned(rtc, ctx, w, knobs, lane, flags=flags, samples=cam.samples)
    else:
        dw.render_lens_rows(cam, lens, 0, H, out.data_ptr(), flags=flags)
        assert_planned(rtc, ctx, w, knobs, lane, flags=flags, lens_samples=lens.usteps * lens.vsteps)
    ctx.synchronize()
    return out


def refused(rtc, w, fn, **request):
    with pytest.raises(rtc.RtcError) as e:
        fn()
    assert e.value.status == L.ERR_UNSUPPORTED
    assert L.plan(rtc, hsize=W, vsize=H, **facts(w), **request).status == L.ERR_UNSUPPORTED


@pytest.mark.parametrize("name", ["empty", "three", "forty", "big", "mirror", "glass"])
def test_frames_and_views(rtc, gpu, worlds, name):
    """Flags 0, NO_CULL and NO_CULL|LDS_TABLE, one view and two: the culled launch takes both views at once, the brute-force
    sources one launch per view (include/rtc.h, rtc_render_views)."""
    import torch
    w, cams = worlds[name], cameras(rtc)
    dw = gpu.upload(w)
    try:
        brute = [render(rtc, gpu, dw, w, c, L.NO_CULL, {}) for c in cams]
        assert not bool((brute[0] == -1.0).all(dim=2).any())
        for flags in FLAGS:
            for c, want in zip(cams, brute):
                assert torch.equal(render(rtc, gpu, dw, w, c, flags, {}), want), (name, flags)
            both = canvas(2 * ROWS)
            dw.render_views(cams, 0, 1, both.data_ptr(), ROWS, flags=flags)
            assert_planned(rtc, gpu, w, {}, flags=flags, nviews=1 if flags & L.NO_CULL else 2)
            gpu.synchronize()
            for v, want in enumerate(brute):
                assert torch.equal(both[v * ROWS:v * ROWS + H], want), (name, flags, v)
                assert bool((both[v * ROWS + H:(v + 1) * ROWS] == -1.0).all())
    finally:
        dw.close()


@pytest.mark.parametrize("name", ["three", "big", "glass"])
def test_lens_launches(rtc, gpu, worlds, name):
    import torch
    w, cam, lens = worlds[name], cameras(rtc)[0], rtc.lens(0.05, 9.0, 2, 2)
    dw = gpu.upload(w)
    try:
        want = render(rtc, gpu, dw, w, cam, L.NO_CULL, {}, lens)
        assert torch.equal(render(rtc, gpu, dw, w, cam, 0, {}, lens), want)
        assert not torch.equal(want, render(rtc, gpu, dw, w, cam, L.NO_CULL, {}))   # (the lens does something)
        refused(rtc, w, lambda: dw.render_lens_rows(cam, lens, 0, H, want.data_ptr(), flags=L.NO_CULL | L.LDS_TABLE),
                flags=L.NO_CULL | L.LDS_TABLE, lens_samples=4)
        gpu.synchronize()
    finally:
        dw.close()


@pytest.mark.parametrize("name", ["two lights", "two lights, big"])
def test_two_lights(rtc, gpu, worlds, name):
    import torch
    w, cam = worlds[name], cameras(rtc)[0]
    dw = gpu.upload(w)
    try:
        want = render(rtc, gpu, dw, w, cam, L.NO_CULL, {})
        assert torch.equal(render(rtc, gpu, dw, w, cam, 0, {}), want)
        refused(rtc, w, lambda: dw.render_rows(cam, 0, H, want.data_ptr(), flags=L.NO_CULL | L.LDS_TABLE), flags=L.NO_CULL | L.LDS_TABLE)
        gpu.synchronize()
    finally:
        dw.close()


@pytest.mark.parametrize("name", ["three", "big", "mirror"])
def test_four_samples_per_pixel(rtc, gpu, worlds, name):
    """samples = 4: the sub-sample store behind the LDS table, with and without the resample branch."""
    import torch
    w, cam = worlds[name], cameras(rtc, 4)[0]
    dw = gpu.upload(w)
    try:
        for aa in (0, L.AA_RESAMPLE):
            want = render(rtc, gpu, dw, w, cam, L.NO_CULL | aa, {})
            for flags in FLAGS:
                assert torch.equal(render(rtc, gpu, dw, w, cam, flags | aa, {}), want), (name, flags, aa)
    finally:
        dw.close()


def context_with(rtc, **env):
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        return rtc.Context(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def test_pipelined_context(rtc, worlds):
    """Depth 3: culled launches are dealt round-robin, brute-force ones stay on lane 0; the pipelined binning threshold."""
    import torch
    ctx = rtc.Context(0)
    try:
        ctx.set_pipeline(3)
        dealt = 0
        for name in ("three", "big", "glass"):
            w, cam = worlds[name], cameras(rtc)[0]
            dw = ctx.upload(w)
            want = render(rtc, ctx, dw, w, cam, L.NO_CULL, {"pipelined": 1})
            for flags in (0, 0, L.NO_CULL | L.LDS_TABLE, 0):
                got = render(rtc, ctx, dw, w, cam, flags, {"pipelined": 1}, lane=dealt % 3)
                dealt += 0 if flags else 1
                assert torch.equal(got, want), (name, flags)
            dw.close()
        assert dealt == 9
    finally:
        ctx.close()


def test_every_chunk_level_of_a_small_launch(rtc, worlds):
    """RTC_TILES_SLOTS=1: 54 tiles are more than three rounds, so the 70x45 launch is split into chunks (flat and frame stack)."""
    import torch
    ctx = context_with(rtc, RTC_TILES_SLOTS=1)
    try:
        for name in ("three", "big", "mirror", "glass"):
            w, cam = worlds[name], cameras(rtc)[0]
            dw = ctx.upload(w)
            want = render(rtc, ctx, dw, w, cam, L.NO_CULL, {"tiles_slots": 1})
            assert ctx.last_launch_info()["multi_tile_workgroups"] > 0
            got = render(rtc, ctx, dw, w, cam, 0, {"tiles_slots": 1})
            assert ctx.last_launch_info()["multi_tile_workgroups"] == 7     # [6, 0, 0, 1]: tests/test_host_launch_plan.py
            assert torch.equal(got, want), name
            dw.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["three", "big"])
def test_probe_and_aov(rtc, gpu, O, worlds, name):
    """rtc_color_at on 100 rays and rtc_render_aov: no launch info to compare, so the results against the oracle's."""
    w, cam = worlds[name], cameras(rtc)[0]
    arr, n = w.array(), len(w)
    rays = np.array([rtc.ray_for_pixel(cam, (7 * i) % W, (3 * i) % H) for i in range(100)])
    want = np.array([O.color_at(arr, n, w.light, tuple(r), 5) for r in rays])
    samples = [A.sample_key(l) for l in w.samples()]
    planes = A.expected_planes(rtc, O, ("launch plan", name), w, cam, samples, A.MODE_RENDER_ASYNC)
    dw = gpu.upload(w)
    try:
        got = dw.color_at(rays)
        assert float(np.max(np.abs(got - want))) <= A.TIGHT_TOL
        assert got.tobytes() == dw.color_at(rays, flags=L.NO_CULL).tobytes()
        for flags in (0, L.NO_CULL):
            assert aov_cases.same_planes(dw.render_aov(cam, A.PLANES, A.MODE_RENDER_ASYNC, flags), planes) == [], (name, flags)
        refused(rtc, w, lambda: dw.render_aov(cam, A.PLANES, A.MODE_RENDER_ASYNC, L.NO_CULL | L.LDS_TABLE), kind=L.AOV, flags=L.NO_CULL | L.LDS_TABLE)
    finally:
        dw.close()
