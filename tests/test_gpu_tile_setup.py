"""k_trace's per-tile set-up: one decomposition of the tile index per tile, the black-row pair read once per workgroup, tiles
proven black going straight to the output stage, the camera origin taken from the host when view_inv is finite, and the
patterns' even test (csrc/rtc_parity.h). None of it may change a bit: every frame here is compared bit for bit with the CPU
oracle's canvas and its ray counts, and rays_primary_proven_miss with a context created under RTC_SKY_ROWS=0, where it must be
0 and the frame the same.

Small on purpose. The culled flat kernel's workgroup is one wave, its tile 8x8 pixels. Frames of 1x1, 7x3, 8x8, 9x17 and 20x12
pixels (one tile, partial and whole; 2 x 3 and 3 x 2 tiles with partial ones on either edge) and 72x40 (9 x 5 tiles) under
RTC_TILES_SLOTS=2, where the launch plan cuts the 45 tiles into three chunks of 8, one of 4, one of 3, two of 2 and ten single
tiles — more chunks of 8 with two and three views (tests/test_host_launch_plan.py pins that arithmetic). The binned primary pass is
forced (RTC_BIN_SMALL_PIXELS=0, RTC_BIN_SMALL_PIXELS_PIPELINED=0): without it there are no row words and no tile lists.
Every material has specular = 0, so that `pow` plays no part.

The pattern frames scale the pattern by (s, 1, 1/s), s from 1e-3 down to 1e-308: a uniform scaling that small fails the
reference's determinant rule (|det| <= 1e-8 is singular), this one has determinant 1 and still sends the pattern-space x
past 2^53 and, at 1e-308, to infinity."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FORCE_BINS = dict(RTC_BIN_SMALL_PIXELS=0, RTC_BIN_SMALL_PIXELS_PIPELINED=0)
SMALL_FRAMES = ((1, 1), (7, 3), (8, 8), (9, 17), (20, 12))
CHUNK_FRAME = (72, 40)
WORLDS = ("floor", "noplane", "wall", "under", "negzero", "infscale")
COUNTERS = ("rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "pixels")


def _ctx_env(rtc, **env):
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        return rtc.Context(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.fixture(scope="module")
def ctxs(rtc):
    out = {"binned": _ctx_env(rtc, **FORCE_BINS), "nosky": _ctx_env(rtc, RTC_SKY_ROWS=0, **FORCE_BINS),
           "chunks": _ctx_env(rtc, RTC_TILES_SLOTS=2, **FORCE_BINS), "chunks nosky": _ctx_env(rtc, RTC_TILES_SLOTS=2, RTC_SKY_ROWS=0, **FORCE_BINS)}
    yield out
    for c in out.values():
        c.close()


def scene(rtc, kind, W, H):
    """Three matte spheres, by default on a checker floor seen from above it with the horizon inside the frame."""
    M = rtc.Matrix
    w = rtc.World(rtc.light())
    for x, y, z, r, col in ((-1.5, 0.5, 0.0, 0.5, (0.9, 0.3, 0.2)), (0.2, 1.0, 1.0, 1.0, (0.2, 0.8, 0.3)), (1.7, 0.4, -1.0, 0.4, (0.3, 0.4, 0.9))):
        w.add_shape(rtc.sphere(M.identity().scaling(r, r, r).translation(x, y, z), rtc.material(color=col, ambient=0.2, diffuse=0.7, specular=0.0)))
    if kind != "noplane":
        w.add_shape(rtc.plane(M.identity(), rtc.material(specular=0.0, pattern=("checker", (0.35, 0.35, 0.35), (0.65, 0.65, 0.65), None))))
    if kind == "wall":   # behind the scene: no sky left, nothing may be skipped
        w.add_shape(rtc.plane(M.identity().rotation_x(math.pi / 2.0).translation(0.0, 0.0, 40.0), rtc.material(color=(0.4, 0.5, 0.7), specular=0.0)))
    frm, to = ((0.0, -3.0, -8.0), (0.0, 2.0, 5.0)) if kind == "under" else ((0.0, 2.0, -8.0), (0.0, 3.0, 5.0))
    cam = rtc.camera(W, H, 0.9, M.make_view_transform(frm, to, (0.0, 1.0, 0.0)))
    if kind == "negzero":   # a translation of -0: the origin is (+0) + (-0) in x, not a copy of the column
        cam = rtc.camera(W, H, 0.9, M.make_view_transform((0.0, 2.0, -8.0), (0.0, 2.0, 5.0), (0.0, 1.0, 0.0)))
        cam.view_inv[3] = -0.0
    if kind == "infscale":  # an infinite scale in view_inv: the origin is NaN and the kernel evaluates it itself
        cam.view_inv[0] = math.inf
    return w, cam


def other_camera(rtc, W, H):
    return rtc.camera(W, H, 0.8, rtc.Matrix.make_view_transform((1.0, 3.0, -9.0), (0.0, 2.5, 5.0), (0.0, 1.0, 0.0)))


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float64:
        return bool(np.array_equal(got, want))
    return bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


class Oracle:
    """The CPU oracle's frames and ray counts, each computed once."""

    def __init__(self, O):
        self.O, self.cache = O, {}

    def frame(self, key, w, cam, mode, y0=0, y1=None):
        k = (key, cam.hsize, cam.vsize, mode, y0, y1)
        if k not in self.cache:
            img, st = self.O.render(w.array(), len(w), w.light, cam, mode=mode, y0=y0, y1=y1, want_stats=True)
            img.setflags(write=False)
            self.cache[k] = (img, st)
        return self.cache[k]


@pytest.fixture(scope="module")
def oracle(O):
    return Oracle(O)


def launch(rtc, ctx, dw, cam, mode, output, y0=0):
    """One render_rows launch (RGBA: rtc_render_views_rgba8) -> (f64 rows or None, 8-bit rows or None, stats, proven)."""
    import torch
    W, H = cam.hsize, cam.vsize
    rows = H - y0
    f = torch.full((rows, W, 3), -1.0, dtype=torch.float64, device=DEV) if output in ("f64", "f64+u8") else None
    q = torch.full((rows, W, 3), 9, dtype=torch.uint8, device=DEV) if output in ("f64+u8", "u8") else None
    a = torch.full((-(-H // 8) * 8, W, 4), 9, dtype=torch.uint8, device=DEV) if output == "rgba" else None
    torch.cuda.synchronize()
    ctx.reset_stats()
    if output == "rgba":
        assert y0 == 0
        dw.render_views_rgba8([cam], 0, 1, a.data_ptr(), a.shape[0], 2.2, mode)
    else:
        dw.render_rows(cam, y0, H, f.data_ptr() if f is not None else None, mode, d_ptr8=q.data_ptr() if q is not None else None)
    st = ctx.stats(extended=True)
    proven = st.pop("rays_primary_proven_miss")
    ctx.synchronize()
    return (None if f is None else f.cpu().numpy(), None if q is None else q.cpu().numpy(), None if a is None else a.cpu().numpy(), st, proven)


def check(rtc, got, want_img, want_st, what):
    f, q, a, st, _ = got
    H = want_img.shape[0]
    if f is not None:
        assert same_bits(f, want_img), what
    if q is not None:
        assert np.array_equal(q, rtc.color_scale255(want_img).reshape(want_img.shape)), what
    if a is not None:
        assert np.array_equal(a[:H], rtc.to_rgba8(want_img, 2.2).reshape(H, -1, 4)) and bool((a[H:] == 9).all()), what
    assert {k: st[k] for k in COUNTERS} == {k: want_st[k] for k in COUNTERS}, (what, st, want_st)


@pytest.mark.parametrize("kind", WORLDS)
def test_frames_outputs_and_modes(rtc, ctxs, oracle, kind):
    """Every frame size, output form and mode, with the black-row proof and without it."""
    some_proven = False
    for W, H in SMALL_FRAMES + (CHUNK_FRAME,):
        w, cam = scene(rtc, kind, W, H)
        names = ("chunks", "chunks nosky") if (W, H) == CHUNK_FRAME else ("binned", "nosky")
        dws = [ctxs[n].upload(w) for n in names]
        for mode in (rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER):
            want_img, want_st = oracle.frame(kind, w, cam, mode)
            for output in ("f64", "f64+u8", "u8", "rgba"):
                what = (kind, W, H, mode, output)
                got = launch(rtc, ctxs[names[0]], dws[0], cam, mode, output)
                assert ctxs[names[0]].last_launch_info()["binned_primary_pass"], what
                if (W, H) == CHUNK_FRAME:
                    assert ctxs[names[0]].last_launch_info()["multi_tile_workgroups"] == 7, what   # chunks of 8, 8, 8, 4, 3, 2, 2
                check(rtc, got, want_img, want_st, what)
                plain = launch(rtc, ctxs[names[1]], dws[1], cam, mode, output)
                check(rtc, plain, want_img, want_st, what + ("RTC_SKY_ROWS=0",))
                assert plain[4] == 0, what
                # proven rays are whole rows of pixels of black tiles, never more than the frame's black pixels
                black = np.count_nonzero(~want_img.reshape(-1, 3).any(axis=1))
                assert got[4] <= black, (what, got[4], black)
                if kind == "wall":   # nothing is sky
                    assert got[4] == 0, (what, got[4])
                some_proven = some_proven or got[4] > 0
        for d in dws:
            d.close()
    if kind in ("floor", "noplane"):
        assert some_proven, kind   # the skipped path ran


@pytest.mark.parametrize("kind", ("floor", "under", "negzero", "infscale"))
def test_pipelined_launches(rtc, oracle, kind):
    """Depth 3: three launches in flight on three lanes, each with its own row words and tile lists."""
    import torch
    for (W, H), env in (((20, 12), FORCE_BINS), (CHUNK_FRAME, dict(RTC_TILES_SLOTS=2, **FORCE_BINS))):
        ctx = _ctx_env(rtc, **env)
        try:
            ctx.set_pipeline(3)
            w, cam = scene(rtc, kind, W, H)
            dw = ctx.upload(w)
            for mode in (rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER):
                want_img, want_st = oracle.frame(kind, w, cam, mode)
                ring = [torch.full((H, W, 3), -1.0, dtype=torch.float64, device=DEV) for _ in range(3)]
                ring8 = [torch.full((H, W, 3), 9, dtype=torch.uint8, device=DEV) for _ in range(3)]
                torch.cuda.synchronize()
                ctx.reset_stats()
                for t, t8 in zip(ring, ring8):
                    dw.render_rows(cam, 0, H, t.data_ptr(), mode, d_ptr8=t8.data_ptr())
                    assert ctx.last_launch_info()["binned_primary_pass"]
                ctx.synchronize()
                st = ctx.stats(extended=True)
                assert {k: st[k] for k in COUNTERS} == {k: 3 * want_st[k] for k in COUNTERS}, (kind, W, H, mode)
                for t, t8 in zip(ring, ring8):
                    assert same_bits(t.cpu().numpy(), want_img), (kind, W, H, mode)
                    assert np.array_equal(t8.cpu().numpy(), rtc.color_scale255(want_img).reshape(H, W, 3)), (kind, W, H, mode)
            dw.close()
        finally:
            ctx.close()


@pytest.mark.parametrize("kind", ("floor", "noplane", "under", "infscale"))
def test_views_rows_and_bands(rtc, ctxs, oracle, kind):
    """Two and three views in one launch (a tile reads its own view's row words), row ranges from y0 = 8 and y0 = 5, and bands
    with stride 2 and 3 from band 0 and band 1."""
    import torch
    for (W, H), name in (((9, 17), "binned"), ((20, 12), "binned"), (CHUNK_FRAME, "chunks")):
        ctx = ctxs[name]
        w, cam = scene(rtc, kind, W, H)
        cam_b = other_camera(rtc, W, H)
        dw = ctx.upload(w)
        full = {c: oracle.frame((kind, c), w, cm, rtc.MODE_RENDER_ASYNC) for c, cm in (("a", cam), ("b", cam_b))}
        HP = -(-H // 8) * 8
        for order in ("ab", "bab"):
            cams = [cam if c == "a" else cam_b for c in order]
            for mode in (rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER):
                wants = [oracle.frame((kind, c), w, cm, mode) for c, cm in zip(order, cams)]
                v = torch.full((len(cams) * HP, W, 3), -1.0, dtype=torch.float64, device=DEV)
                v8 = torch.full((len(cams) * HP, W, 3), 9, dtype=torch.uint8, device=DEV)
                torch.cuda.synchronize()
                ctx.reset_stats()
                dw.render_views(cams, 0, 1, v.data_ptr(), HP, mode, d_ptr8=v8.data_ptr())
                st = ctx.stats(extended=True)
                ctx.synchronize()
                vh, v8h = v.cpu().numpy(), v8.cpu().numpy()
                for k, (img, _) in enumerate(wants):
                    assert same_bits(vh[k * HP:k * HP + H], img), (kind, W, H, order, mode, k)
                    assert np.array_equal(v8h[k * HP:k * HP + H], rtc.color_scale255(img).reshape(H, W, 3)), (kind, W, H, order, mode, k)
                    assert bool((vh[k * HP + H:(k + 1) * HP] == -1.0).all()), (kind, W, H, order, mode, k)   # rows past the frame stay untouched
                assert {k: st[k] for k in COUNTERS} == {k: sum(s[k] for _, s in wants) for k in COUNTERS}, (kind, W, H, order, mode)
        for y0 in (8, 5):
            if y0 >= H:
                continue
            for mode in (rtc.MODE_RENDER_ASYNC, rtc.MODE_RENDER):
                want_img, want_st = oracle.frame(kind, w, cam, mode, y0, H)
                check(rtc, launch(rtc, ctx, dw, cam, mode, "f64+u8", y0), want_img, want_st, (kind, W, H, "rows from", y0, mode))
        nbands = -(-H // 8)
        for first, stride in ((0, 2), (1, 2), (0, 3), (1, 3)):
            if first >= nbands:
                continue
            t = torch.full((rtc.group_packed_rows(H, stride), W, 3), -1.0, dtype=torch.float64, device=DEV)
            torch.cuda.synchronize()
            dw.render_bands(cam, first, stride, t.data_ptr())
            ctx.synchronize()
            got = t.cpu().numpy()
            for k in range(rtc.group_bands_owned(H, stride, first)):
                y0 = rtc.group_packed_row_to_image(first, 8 * k, stride)
                assert same_bits(got[8 * k:8 * k + min(8, H - y0)], full["a"][0][y0:y0 + 8]), (kind, W, H, first, stride, k)
        dw.close()


@pytest.mark.parametrize("pattern", ("stripe", "ring", "checker"))
def test_patterns_far_from_the_origin(rtc, gpu, ctxs, oracle, pattern):
    """16x16 frames of a patterned floor and a patterned sphere around the origin (negative coordinates on the left and below),
    the pattern scaled until floor(x) passes 2^53 and reaches infinity; the default context and the binned one."""
    M = rtc.Matrix
    W = H = 16
    cam = rtc.camera(W, H, 1.0, M.make_view_transform((0.5, 3.0, -6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    for s in (1.0, 1e-3, 1e-6, 1e-9, 1e-12, 1e-16, 1e-308):
        xf = M.identity().scaling(s, 1.0, 1.0 / s)
        m = rtc.material(ambient=0.3, diffuse=0.7, specular=0.0, pattern=(pattern, (0.9, 0.2, 0.1), (0.1, 0.3, 0.8), xf))
        w = rtc.World(rtc.light())
        w.add_shape(rtc.plane(M.identity(), m))
        w.add_shape(rtc.sphere(M.identity().translation(-1.0, 0.5, 0.5), m))
        want_img, want_st = oracle.frame((pattern, s), w, cam, rtc.MODE_RENDER_ASYNC)
        assert len(np.unique(want_img.reshape(-1, 3), axis=0)) > 2, (pattern, s)   # something is drawn
        for ctx in (gpu, ctxs["binned"]):
            dw = ctx.upload(w)
            img, st = dw.render(cam, with_stats=True)
            assert same_bits(img, want_img), (pattern, s)
            assert {k: st[k] for k in COUNTERS} == {k: want_st[k] for k in COUNTERS}, (pattern, s)
            dw.close()
