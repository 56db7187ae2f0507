"""Whole frames at full size for the reflective and refractive kernels, C4 and C5: the launch configuration callers and
bench.py get at these sizes (guided chunks at their natural thresholds, the binned primary pass of one-level worlds,
pipelined lanes, canvases beyond 4 GiB), compared with the CPU oracle and with the A/B contexts bit for bit.

Every case pins the launch it was chosen for (`last_launch_info`, literal expected values below): a threshold change that
moves a case off its path fails here and the case has to be re-chosen on purpose."""
import importlib
import os
from dataclasses import dataclass

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TIGHT_TOL = 1e-12
NTHREADS = 16     # oracle threads: what one job may use on a GPU machine (not os.cpu_count())
DEV = "cuda:0"


@pytest.fixture(scope="module")
def scenes(rtc):
    return importlib.import_module(rtc.__name__ + ".scenes")


def _ctx_env(rtc, **env):
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ[k] = str(v)
        return rtc.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _config1(rtc, scenes):
    w, cam = rtc.load_yaml(path=os.path.join(os.path.dirname(rtc.__file__), "data", "reflect_refract.yml"))
    return w, rtc.camera(1920, 1080, cam.fov, rtc.Matrix(np.array(list(cam.view_inv)).reshape(4, 4)).inverse())


@dataclass
class Case:
    name: str
    make: object          # (rtc, scenes) -> (World, camera)
    size: tuple           # (width, height)
    source: int           # rtc_launch_info::source of the default launch (3 one-level cull, 4 two-level cull)
    reflective: bool      # the info flags name the kernel: <SRC, REFL, REFR, false>
    refractive: bool
    light_lists: bool     # worlds of 32 objects and more carry light-space shadow lists
    binned_in_order: bool     # binned primary pass of the in-order launch
    binned_pipelined: bool    # ... of a launch on a pipelined context (depth 3)
    guided: bool          # multi_tile_workgroups > 0 (guided chunks at the natural `slots`)
    brute_source: int     # the source RTC_FLAG_NO_CULL selects (0 scalar cache, 1 one LDS tile, 2 LDS tiles)
    bands: tuple | None   # None: whole frame against the oracle; else full-width row ranges [y0, y1)
    mode_render: bool = False   # (e) Camera::render at full size
    rgba: bool = False          # (f) render_rgba8(gamma 2.2) against the host conversion


# One-level refractive worlds at 1080p: the in-order launch is the UNBINNED one (2.07 M pixels < 6 M), the pipelined launch
# the BINNED one (>= 1.5 M), both with guided chunks (>= 3 x 4096 tiles of 8x8). C4 is binned in both (16.7 M pixels).
CASES = [
    #    name           make                                                              size          src  refl   refr   lists  bin-io bin-pipe guided brute bands
    Case("config1", _config1,                                                          (1920, 1080), 3, True, True, False, False, True, True, 0, None, mode_render=True, rgba=True),
    Case("criterion", lambda rtc, s: s.criterion(1920, 1080),                          (1920, 1080), 3, True, True, False, False, True, True, 0, None),   # kr = 0, transparent
    Case("test8", lambda rtc, s: s.test8(1920, 1080),                                  (1920, 1080), 3, True, True, False, False, True, True, 0, None),
    Case("mixed", lambda rtc, s: s.mixed(1920, 1080),                                  (1920, 1080), 3, True, True, False, False, True, True, 0, None),
    Case("glass40", lambda rtc, s: s.glass_cluster(40, 1923, 1085),                    (1923, 1085), 3, True, True, True, False, True, True, 0, None),
    Case("glass300", lambda rtc, s: s.glass_cluster(300, 1923, 1085),                  (1923, 1085), 4, True, True, True, True, True, True, 1,
         ((0, 8), (536, 552), (1080, 1085))),
    Case("reflective1000", lambda rtc, s: s.synthetic(1000, 1920, 1080, reflective=True), (1920, 1080), 4, True, False, True, True, True, True, 2,
         ((0, 8), (536, 552), (1072, 1080))),
    Case("c4", lambda rtc, s: s.synthetic(100, 4096, 4096, reflective=True),          (4096, 4096), 3, True, False, True, True, True, True, 0, None,
         mode_render=True, rgba=True),
    Case("c5", lambda rtc, s: s.synthetic(1000, 8192, 8192),                          (8192, 8192), 4, False, False, True, True, True, True, 2,
         ((0, 16), (4088, 4104), (8176, 8192))),
]


def _pin(info, case, **changed):
    want = {"source": case.source, "reflective": case.reflective, "refractive": case.refractive,
            "binned_primary_pass": case.binned_in_order, "light_lists": case.light_lists, "guided": case.guided}
    want.update(changed)
    got = {"source": info["source"], "reflective": info["reflective"], "refractive": info["refractive"],
           "binned_primary_pass": info["binned_primary_pass"], "light_lists": info["light_lists"],
           "guided": info["multi_tile_workgroups"] > 0}
    assert got == want, (case.name, got, want)


def _canvas(H, W, fill=-1.0, dtype=None):
    import torch
    return torch.full((H, W, 3), fill, dtype=dtype or torch.float64, device=DEV)


def _render(ctx, dw, cam, out, mode=1, flags=0, d_ptr8=None):
    """One in-order launch of the whole frame into the device canvas `out`; returns its ray counts."""
    import torch
    torch.cuda.synchronize()
    ctx.reset_stats()
    dw.render_rows(cam, 0, cam.vsize, out.data_ptr(), mode, flags=flags, d_ptr8=d_ptr8)
    return ctx.stats()   # synchronises


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_full_frame(rtc, O, scenes, case):
    import torch
    w, cam = case.make(rtc, scenes)
    W, H = cam.hsize, cam.vsize
    assert (W, H) == case.size
    arr = w.array()
    ctx = rtc.Context(0)
    try:
        dw = ctx.upload(w)
        # (a) in order, default context, into a canvas pre-filled with -1 (an unwritten pixel shows: (-1, -1, -1) is no colour
        # of these scenes; colours can be negative, `mixed` has the book's test pattern)
        full = _canvas(H, W)
        full8 = _canvas(H, W, 7, torch.uint8)
        st = _render(ctx, dw, cam, full, d_ptr8=full8.data_ptr())
        _pin(ctx.last_launch_info(), case)
        assert st["pixels"] == W * H and st["rays_primary"] == W * H
        assert not bool((full == -1.0).all(dim=2).any())
        if case.bands is None:
            want, ost = O.render(arr, len(w), w.light, cam, mode=1, nthreads=NTHREADS, want_stats=True)
            got = full.cpu().numpy()
            assert float(np.max(np.abs(got - want))) <= TIGHT_TOL, case.name
            assert st == ost, (case.name, st, ost)
            del got, want
        else:
            band = _canvas(16, W)
            for y0, y1 in case.bands:
                want, ost = O.render(arr, len(w), w.light, cam, mode=1, y0=y0, y1=y1, nthreads=NTHREADS, want_stats=True)
                assert float(np.max(np.abs(full[y0:y1].cpu().numpy() - want))) <= TIGHT_TOL, (case.name, y0)
                band.fill_(-1.0)
                torch.cuda.synchronize()
                ctx.reset_stats()
                dw.render_rows(cam, y0, y1, band.data_ptr())
                assert ctx.stats() == ost, (case.name, y0)
                assert torch.equal(band[:y1 - y0], full[y0:y1]), (case.name, y0)
            del band
        # the frames exercise what the kernels were chosen for (Criterion's glass has kr = 0: refraction only)
        assert (st["rays_reflect"] > 0) == (case.name not in ("criterion", "c5")), (case.name, st)
        assert (st["rays_refract"] > 0) == case.refractive, (case.name, st)
        # (f) the 8-bit output of the same launch == Color::scale of the f64 canvas (host conversion, in row blocks)
        for r0 in range(0, H, 1024):
            r1 = min(H, r0 + 1024)
            assert np.array_equal(full8[r0:r1].cpu().numpy(), rtc.color_scale255(full[r0:r1].cpu().numpy())), (case.name, r0)
        del full8
        if case.rgba:
            assert np.array_equal(dw.render_rgba8(cam, gamma=2.2), rtc.to_rgba8(full.cpu().numpy(), 2.2)), case.name

        # (c) pipelined, depth 3: 6 launches into a ring of 4 canvases; the timings are read BEFORE any synchronisation
        ctx.set_pipeline(3)
        ring = [_canvas(H, W) for _ in range(4)]
        torch.cuda.synchronize()
        ctx.reset_stats()
        for i in range(6):
            dw.render_rows(cam, 0, H, ring[i % 4].data_ptr())
            info = ctx.last_launch_info()
            assert info["lane"] == i % 3
            _pin(info, case, binned_primary_pass=case.binned_pipelined)
        kt, bt = ctx.kernel_times_ms(6), ctx.binning_times_ms(6)
        assert len(kt) == 6 and np.isfinite(kt).all() and (kt > 0).all(), (case.name, kt)
        assert len(bt) == 6 and np.isfinite(bt).all() and (bt >= 0).all(), (case.name, bt)
        assert (bt > 0).all() == case.binned_pipelined, (case.name, bt)
        pst = ctx.stats()
        assert pst == {k: 6 * v for k, v in st.items()}, (case.name, pst, st)
        for i, r in enumerate(ring):
            assert torch.equal(r, full), (case.name, i)
        del ring
        ctx.set_pipeline(1)

        # (d) A/B contexts on the same frame, whole frame, bit for bit with equal ray counts
        other = _canvas(H, W)
        for label, env, flags, changed in (
                ("guided off", {"RTC_TILES_GUIDED": 0}, 0, {"guided": False}),
                ("no lists", {"RTC_BINNING": 0, "RTC_LIGHT_LISTS": 0}, 0, {"binned_primary_pass": False, "light_lists": False}),
                ("brute force", None, rtc.FLAG_NO_CULL, {"source": case.brute_source, "binned_primary_pass": False})):
            c2 = _ctx_env(rtc, **env) if env else ctx
            try:
                d2 = c2.upload(w) if env else dw
                other.fill_(-1.0)
                s2 = _render(c2, d2, cam, other, flags=flags)
                _pin(c2.last_launch_info(), case, **changed)
                assert s2 == st, (case.name, label, s2, st)
                assert torch.equal(other, full), (case.name, label)
            finally:
                if env:
                    c2.close()

        # (e) Camera::render at full size: the kernel writes the exclusive last row and column as 0, every other pixel as (a)
        if case.mode_render:
            other.fill_(-1.0)
            sm = _render(ctx, dw, cam, other, mode=rtc.MODE_RENDER)
            assert sm["pixels"] == (W - 1) * (H - 1)
            assert not bool(other[H - 1].any()) and not bool(other[:, W - 1].any()), case.name
            assert torch.equal(other[:H - 1, :W - 1], full[:H - 1, :W - 1]), case.name
        del other, full
        dw.close()
    finally:
        ctx.close()
        torch.cuda.empty_cache()


def test_views_beyond_4_gib(rtc, scenes):
    """(g) One rtc_render_views launch of three C5 views: 4.8 GB of f64 output, so rows of the last view lie beyond 4 GiB
    of the launch's base address (every canvas offset must be size_t). Each view equals its own single-view render."""
    import torch
    w, cam = scenes.synthetic(1000, 8192, 8192)
    W = H = 8192
    M = rtc.Matrix
    cams = [cam] + [rtc.camera(W, H, 0.7, M.make_view_transform((dx, 2.0, -8.0), (dx, 1.0, 5.0), (0.0, 1.0, 0.0))) for dx in (0.75, -1.5)]
    ctx = rtc.Context(0)
    try:
        dw = ctx.upload(w)
        views = torch.full((3 * H, W, 3), -1.0, dtype=torch.float64, device=DEV)
        assert views.numel() * 8 > 4 << 30
        torch.cuda.synchronize()
        ctx.reset_stats()
        dw.render_views(cams, 0, 1, views.data_ptr(), H)
        st = ctx.stats()
        assert ctx.last_launch_info()["source"] == 4
        one = _canvas(H, W)
        total = {}
        for v, c in enumerate(cams):
            one.fill_(-1.0)
            s1 = _render(ctx, dw, c, one)
            for k, x in s1.items():
                total[k] = total.get(k, 0) + x
            assert not bool((one == -1.0).all(dim=2).any()), v
            assert torch.equal(views[v * H:(v + 1) * H], one), v
        assert st == total
        del views, one
        dw.close()
    finally:
        ctx.close()
        torch.cuda.empty_cache()


def test_pipelined_kernel_times_wait_for_every_lane(rtc, scenes):
    """rtc_kernel_times_ms / rtc_binning_times_ms on a pipelined context straight after the launches: a long launch on lane 0
    (four C5 views) and a tiny frame on lane 1 that ends first. Both times must be read without an error, so the call has
    to wait for the older launch on the other lane, not only for the newest launch."""
    import torch
    w, cam = scenes.synthetic(1000, 8192, 8192)
    tiny = rtc.camera(16, 16, 0.7, rtc.Matrix.make_view_transform((0.0, 2.0, -8.0), (0.0, 1.0, 5.0), (0.0, 1.0, 0.0)))
    ctx = rtc.Context(0)
    try:
        dw = ctx.upload(w)
        ctx.set_pipeline(2)
        big = torch.empty((4 * 8192, 8192, 3), dtype=torch.float64, device=DEV)
        small = torch.empty((16, 16, 3), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        for _ in range(2):   # the first round allocates each lane's tile lists; the second is the one read without a wait
            ctx.synchronize()
            dw.render_views([cam] * 4, 0, 1, big.data_ptr(), 8192)
            assert ctx.last_launch_info()["lane"] == 0
            dw.render_rows(tiny, 0, 16, small.data_ptr())
            assert ctx.last_launch_info()["lane"] == 1
        kt = ctx.kernel_times_ms(2)
        bt = ctx.binning_times_ms(2)
        assert len(kt) == 2 and np.isfinite(kt).all() and (kt > 0).all(), kt
        assert len(bt) == 2 and np.isfinite(bt).all() and (bt > 0).all(), bt    # two-level world: every launch is binned
        assert kt[0] > kt[1], kt
        ctx.synchronize()
        assert np.array_equal(ctx.kernel_times_ms(2), kt)
        del big, small
        dw.close()
    finally:
        ctx.close()
        torch.cuda.empty_cache()
