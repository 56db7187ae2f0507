"""k_trace's whole-tile flavour: a one-sample launch of one camera, one light and an f64 canvas whose tiles are all whole
(whole_tile_launch, csrc/rtc_kernels.hip; tests/test_host_whole_tile.py pins the condition) runs an instantiation without the
per-lane range state, the view and band terms and the narrow and 8-bit output forms. The one-sample kernel evaluates each of
those to the same constants for such a launch, so nothing may change: every frame here is rendered by a default context and by
one created under RTC_WHOLE_TILES=0 (every launch on the kernels it had before), in order and on a pipeline of depth 3, and
the two are compared bit for bit with each other and with the CPU oracle, ray counters included. Launches that do not qualify
must come out the same in both contexts too: they never reach the new kernels.

Small on purpose (the shape of tests/test_gpu_one_sample.py, whose scenes these are). Qualifying frames: 8x8 (one tile), 16x8,
64x64 with the tile lists forced (RTC_BIN_SMALL_PIXELS=0) and RTC_TILES_PER_WG=3 — 64 tiles over 22 workgroups, so the last
workgroups' last repetition runs past the launch's tiles —, the same frame under RTC_TILES_SLOTS=2, where the launch plan cuts
the tiles into guided chunks, rows [8, 24) of a 32x32 camera (y0 != 0), and, with the 64x64 frame, tile rows the binning
kernel proves black (the sky above the horizon). Worlds: matte spheres on a checker floor (the flat kernel), the same with
mirrors and with a glass sphere (the frame-stack kernels), and 300 spheres (the two-level kernels) matte, with mirrors, with
mirrors and glass — the matte one stays on the one-sample kernel (its whole-tile form is not instantiated). Every material has
specular = 0, so that `pow` — the one operation that is not bit-exact between the device and the oracle — plays no part.

Launches that do not qualify: 20x12 (partial tiles), RTC_MODE_RENDER, an 8-bit output beside the canvas, two views, bands of
stride 2, and a canvas at an address that is 8 but not 16 bytes aligned."""
import numpy as np
import pytest

from test_gpu_one_sample import COUNTERS, FORCE_BINS, Oracle, _ctx_env, other_camera, same_bits, scene

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORLDS = ("floor", "mirror", "glass", "many", "manymirror", "manyglass")
DEPTHS = (1, 3)   # in order; a pipeline of three lanes
CONFIGS = (("binned", {}), ("reps", dict(RTC_TILES_PER_WG=3)), ("chunks", dict(RTC_TILES_SLOTS=2)))
# (context configuration, W, H, y0, y1)
QUALIFYING = (("binned", 8, 8, 0, 8), ("binned", 16, 8, 0, 8), ("reps", 64, 64, 0, 64), ("chunks", 64, 64, 0, 64),
              ("binned", 32, 32, 8, 24), ("binned", 64, 64, 0, 64))


@pytest.fixture(scope="module")
def ctxs(rtc):
    """(default, RTC_WHOLE_TILES=0) per configuration"""
    out = {name: (_ctx_env(rtc, **env, **FORCE_BINS), _ctx_env(rtc, RTC_WHOLE_TILES=0, **env, **FORCE_BINS)) for name, env in CONFIGS}
    yield out
    for pair in out.values():
        for c in pair:
            c.close()


@pytest.fixture(scope="module")
def oracle(O):
    return Oracle(O)


class Uploads:
    """Each world once per context (a world does not depend on the frame size)."""

    def __init__(self, rtc, ctxs):
        self.rtc, self.ctxs, self.held = rtc, ctxs, {}

    def pair(self, kind, config):
        if (kind, config) not in self.held:
            w, _ = scene(self.rtc, kind, 8, 8)
            self.held[kind, config] = (w, [c.upload(w) for c in self.ctxs[config]])
        return self.held[kind, config]

    def close(self):
        for _, dws in self.held.values():
            for d in dws:
                d.close()


@pytest.fixture(scope="module")
def uploads(rtc, ctxs):
    u = Uploads(rtc, ctxs)
    yield u
    u.close()


def run(ctx, depth, rows, W, enqueue, want8=False, offset=0):
    """`depth` launches of enqueue(f64 address, 8-bit address or None) on a pipeline of that depth (1: in order), each into
    canvases of its own, `offset` doubles into their allocation -> (f64 canvases, 8-bit canvases, what lies around the f64
    canvases, the context's counters over the launches)."""
    import torch
    n = rows * W * 3
    raw = [torch.full((n + 4,), -1.0, dtype=torch.float64, device=DEV) for _ in range(depth)]
    q = [torch.full((rows, W, 3), 9, dtype=torch.uint8, device=DEV) if want8 else None for _ in range(depth)]
    torch.cuda.synchronize()
    ctx.set_pipeline(depth)
    try:
        ctx.reset_stats()
        for r, b in zip(raw, q):
            enqueue(r.data_ptr() + 8 * offset, None if b is None else b.data_ptr())
        st = ctx.stats(extended=True)
        ctx.synchronize()
    finally:
        ctx.set_pipeline(1)
    host = [r.cpu().numpy() for r in raw]
    return ([h[offset:offset + n].reshape(rows, W, 3) for h in host], [None if b is None else b.cpu().numpy() for b in q],
            [np.concatenate((h[:offset], h[offset + n:])) for h in host], st)


def check(rtc, pair, depth, rows, W, enqueue_for, wants, what, want8=False, offset=0):
    """Both contexts of `pair` run enqueue_for(its uploaded world); canvases and counters against each other and against the
    oracle's (image, stats) pieces `wants`, stacked in output order — all to the bit."""
    got = [run(c, depth, rows, W, enqueue_for(k), want8, offset) for k, c in enumerate(pair)]
    info = [c.last_launch_info() for c in pair]
    assert info[0] == info[1], (what, info)   # same source, lists and workgroup shape: the launch plan does not know the flavour
    on, off = got
    assert on[3] == off[3], (what, on[3], off[3])
    want_img = np.concatenate([img for img, _ in wants])
    for k in range(depth):
        assert same_bits(on[0][k], off[0][k]), (what, "whole-tile kernel != one-sample kernel", k)
        assert same_bits(on[0][k], want_img), (what, "!= oracle", k)
        assert bool((on[2][k] == -1.0).all()) and bool((off[2][k] == -1.0).all()), (what, "stored outside the canvas", k)
        if want8:
            assert np.array_equal(on[1][k], off[1][k]) and np.array_equal(on[1][k], rtc.color_scale255(want_img).reshape(want_img.shape)), (what, k)
    want_st = {c: depth * sum(s[c] for _, s in wants) for c in COUNTERS}
    assert {c: on[3][c] for c in COUNTERS} == want_st, (what, on[3], want_st)
    return on[3], info[0]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind", WORLDS)
def test_qualifying_frames(rtc, ctxs, uploads, oracle, kind, depth):
    proven = 0
    for config, W, H, y0, y1 in QUALIFYING:
        w, dws = uploads.pair(kind, config)
        cam = scene(rtc, kind, W, H)[1]
        want = oracle.frame(kind, w, cam, rtc.MODE_RENDER_ASYNC, y0, y1)
        st, info = check(rtc, ctxs[config], depth, y1 - y0, W, lambda k: lambda p, p8: dws[k].render_rows(cam, y0, y1, p), [want],
                         (kind, depth, config, W, H, y0, y1))
        assert info["binned_primary_pass"] and info["source"] == (4 if kind.startswith("many") else 3), (kind, config, info)
        assert (info["reflective"], info["refractive"]) == (kind not in ("floor", "many"), kind.endswith("glass")), (kind, info)
        if config == "reps":
            assert info["tiles_per_workgroup"] == 3, info
        if config == "chunks":
            assert info["multi_tile_workgroups"] > 0, info
        if (config, W) == ("binned", 64):
            proven = st["rays_primary_proven_miss"]
    # the 64x64 frame's upper tile rows are sky: proven black, counted as cast, stored by the whole-tile output stage
    assert proven > 0 and proven % (64 * 8) == 0, (kind, depth, proven)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("kind", WORLDS)
def test_launches_that_do_not_qualify_are_unchanged(rtc, ctxs, uploads, oracle, kind, depth):
    pair = ctxs["binned"]
    w, dws = uploads.pair(kind, "binned")
    A, S = rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER
    # 20x12: a partial tile column and a partial tile row
    cam = scene(rtc, kind, 20, 12)[1]
    check(rtc, pair, depth, 12, 20, lambda k: lambda p, p8: dws[k].render_rows(cam, 0, 12, p), [oracle.frame(kind, w, cam, A)], (kind, depth, "20x12"))
    cam = scene(rtc, kind, 16, 8)[1]
    # Camera::render's mode: the last row and column stay untraced
    check(rtc, pair, depth, 8, 16, lambda k: lambda p, p8: dws[k].render_rows(cam, 0, 8, p, S), [oracle.frame(kind, w, cam, S)], (kind, depth, "RTC_MODE_RENDER"))
    # an 8-bit frame beside the canvas
    check(rtc, pair, depth, 8, 16, lambda k: lambda p, p8: dws[k].render_rows(cam, 0, 8, p, A, 0, d_ptr8=p8), [oracle.frame(kind, w, cam, A)],
          (kind, depth, "out8"), want8=True)
    # a canvas 8 bytes off a 16-byte boundary
    check(rtc, pair, depth, 8, 16, lambda k: lambda p, p8: dws[k].render_rows(cam, 0, 8, p), [oracle.frame(kind, w, cam, A)], (kind, depth, "misaligned"), offset=1)
    # two views in one launch, the second 8 rows below the first
    cam_b = other_camera(rtc, 16, 8)
    check(rtc, pair, depth, 16, 16, lambda k: lambda p, p8: dws[k].render_views([cam, cam_b], 0, 1, p, 8),
          [oracle.frame((kind, "a"), w, cam, A), oracle.frame((kind, "b"), w, cam_b, A)], (kind, depth, "two views"))
    # bands 0 and 2 of a 16x32 camera, packed
    cam = scene(rtc, kind, 16, 32)[1]
    check(rtc, pair, depth, 16, 16, lambda k: lambda p, p8: dws[k].render_bands(cam, 0, 2, p),
          [oracle.frame(kind, w, cam, A, 0, 8), oracle.frame(kind, w, cam, A, 16, 24)], (kind, depth, "bands of stride 2"))
