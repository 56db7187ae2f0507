"""k_bin_tiles' sorted packed tile lists and k_trace's scalar walk over them.

The lists are read back through rtc_debug_tile_lists (an unlisted export next to rtc_debug_tile_counts, bound here by hand):
in a one-level launch (RTC_SRC=3) every packed list of at most SORT_CAP entries is strictly ascending; in every launch
each list holds, as a set, exactly what a context with the sort switched off (RTC_BIN_SORT=0) collects, under the same
counts (a two-level launch, RTC_SRC=4, sorts nothing: DESIGN.md §5). The walks' edges — lists of 0, 1, 8, 9, 16, 17 and 64
entries, an overflowing one, entries whose truncated keys are equal, columns of spheres that end different tiles' walks at
different entries, a sphere on a tile corner — are built into one world, whose read-back counts must show them; that
world (flat, reflective and refractive) and the cases of candidate_list_cases.py render bit for bit, ray counters
included, what a context with RTC_BINNING=0 renders: one and four samples, two views in one launch, interleaved bands,
pipeline depth 3."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).parent))
K = __import__("candidate_list_cases").sibling("candidate_list_cases")
G = K.sibling("test_gpu_candidate_lists")
_ctx_env = K.sibling("test_gpu_group")._ctx_env
TIGHT_TOL = K.sibling("test_gpu_parity").TIGHT_TOL
O = K.O
CAP = K.TILE_CAP
SORT_CAP = 16                     # RTC_TILE_SORT_CAP
FORCED = dict(RTC_BIN_SMALL_PIXELS=0, RTC_BIN_SMALL_PIXELS_PIPELINED=0)
W = H = 64
# tile (tx, ty) -> what stands in it (edge_world)
T_ONE, T_EIGHT, T_NINE, T_FULL, T_OVER, T_EQUAL, T_COVER_FIRST, T_COVER_MID, T_EMPTY = (1, 1), (3, 1), (5, 1), (1, 3), (3, 3), (5, 3), (1, 5), (5, 5), (7, 0)


def tile_lists(rtc, ctx, dw):
    """lists[view, ty, tx, slot] of the context's last launch (rtc_debug_tile_lists), or None when it built none."""
    f = rtc.lib().rtc_debug_tile_lists
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
    probe, dims = np.zeros(1, dtype=np.uint32), (C.c_uint32 * 4)()
    counts = G.tile_counts(rtc, ctx, dw)
    if counts is None:
        assert f(ctx._h, dw._h, dims, probe.ctypes.data, 0) == 0 and dims[0] == 0
        return None
    views, ty, tx = counts[0].shape
    assert f(ctx._h, dw._h, dims, probe.ctypes.data, 1) != 0, "a buffer too small for the lists must be refused"
    out = np.zeros(views * ty * tx * CAP, dtype=np.uint32)
    assert f(ctx._h, dw._h, dims, out.ctypes.data, out.size) == 0 and tuple(dims) == (1, views, tx, ty)
    return out.reshape(views, ty, tx, CAP)


def edge_cam(samples=1, frm=(0., 2., -8.)):
    return O.camera(W, H, 0.9, O.view_transform(frm, (0., 1., 5.), (0., 1., 0.)), samples)


def edge_world(variant="flat"):
    """Spheres placed on the rays through tile centres of edge_cam(): tile -> its list's length, by construction."""
    cam = edge_cam()
    shapes = []

    def put(tile, d, r, dx=0., dy=0.):
        ray = K.pixel_ray(cam, 8 * tile[0] + 3, 8 * tile[1] + 3, 1.0 + dx, 1.0 + dy)   # (offset 1.0: the tile's very centre)
        i = len(shapes)
        m = dict(color=(0.2 + 0.1 * (i % 7), 0.9 - 0.1 * (i % 5), 0.3 + 0.1 * (i % 3)), specular=0.3)
        if variant == "reflective" and i % 3 == 0:
            m["reflective"] = 0.5
        if variant == "glass" and i % 3 == 0:
            m.update(transparency=0.8, refractive_index=1.5, reflective=0.2)
        shapes.append(K.ball(tuple(ray[k] + d * ray[3 + k] for k in range(3)), r, **m))

    def column(tile, n, d0=3.0, step=0.5):      # n small spheres one behind the other, each under a pixel across
        for k in range(n):
            put(tile, d0 + step * k, 0.008 * (d0 + step * k))

    column(T_ONE, 1)
    column(T_EIGHT, 8)
    column(T_NINE, 9)
    column(T_FULL, CAP)
    column(T_OVER, CAP + 6)
    for dx, dy in ((-2., -2.), (2., -2.), (-2., 2.), (2., 2.)):    # equal distances: equal truncated keys, the index orders them
        put(T_EQUAL, 6.56, 0.03, dx, dy)      # (keys near 6.52: between two steps, 6.5 and 6.53125, of the 16-bit truncation)
    put(T_COVER_FIRST, 5.0, 0.6)         # covers the tile: every lane's hit is nearer than the 16 keys behind it; 17: not sorted
    column(T_COVER_FIRST, 16, 7.0)
    column(T_COVER_MID, 5, 3.0, 0.4)     # five in front, the cover, ten behind; 16: the longest list that is sorted
    put(T_COVER_MID, 6.0, 0.75)
    column(T_COVER_MID, 10, 8.0)
    put((3, 6), 6.0, 0.05, 4., 4.)        # on the corner of tiles (3,6) (4,6) (3,7) (4,7)
    fm = dict(pattern=("checker", (0.3,) * 3, (0.7,) * 3, None), specular=0.)
    if variant == "reflective":
        fm["reflective"] = 0.3
    shapes.append(K.shp(K.PLANE, m=K.mat(**fm)))
    return K.number(shapes), O.light((-4., 6., -6.))


@pytest.fixture(scope="module")
def ctxs(rtc):
    out = {"binned": _ctx_env(rtc, **FORCED), "walk": _ctx_env(rtc, RTC_BINNING=0), "pipelined": _ctx_env(rtc, **FORCED)}
    for src in (3, 4):
        out[f"sorted{src}"] = _ctx_env(rtc, RTC_SRC=src, **FORCED)
        out[f"unsorted{src}"] = _ctx_env(rtc, RTC_SRC=src, RTC_BIN_SORT=0, **FORCED)
    out["pipelined"].set_pipeline(3)
    yield out
    for c in out.values():
        c.close()


def check_sorted(name, counts, lists, counts_u, lists_u, sorted_launch):
    bad = []
    if not np.array_equal(counts, counts_u):
        bad.append((name, "counts differ from the unsorted run's"))
    for v, ty, tx in np.ndindex(*counts.shape):
        c = int(counts[v, ty, tx])
        got, ref = lists[v, ty, tx, :min(c, CAP)], lists_u[v, ty, tx, :min(c, CAP)]
        if sorted_launch and c <= SORT_CAP and not (np.diff(got.astype(np.int64)) > 0).all():
            bad.append((name, v, tx, ty, "not strictly ascending", got.tolist()))
        if sorted(got.tolist()) != sorted(ref.tolist()):
            bad.append((name, v, tx, ty, "not the unsorted run's entries"))
    return bad


@pytest.mark.parametrize("src", [3, 4])
def test_lists_are_sorted_and_complete(rtc, ctxs, src):
    """src 3: the sorted launch against the RTC_BIN_SORT=0 launch. src 4: the host asks no two-level launch to sort, so both
    contexts run the same binning kernel — the case only pins that: the lists, counts and frames of a two-level launch
    are what they were, in table order, whatever RTC_BIN_SORT says."""
    worlds = {"edges": (*edge_world(), edge_cam()),
              "field": (K.field_world(150, seed=5), O.light((-4., 6., -3.)), K.cam_of(W, H, 0.9, (0., 2., -8.), (0., 1., 5.)))}
    bad, disorder = [], 0
    for name, (shapes, lgt, cam) in worlds.items():
        w = K.as_world(rtc, shapes, lgt)
        res = {}
        for kind in ("sorted", "unsorted"):
            ctx = ctxs[f"{kind}{src}"]
            dw = ctx.upload(w)
            img = dw.render(cam)
            info = ctx.last_launch_info()
            assert info["source"] == src and info["binned_primary_pass"], info
            res[kind] = (G.tile_counts(rtc, ctx, dw)[0], tile_lists(rtc, ctx, dw), img)
            dw.close()
        assert res["sorted"][0].max() > 1 and np.array_equal(res["sorted"][2], res["unsorted"][2])
        bad += check_sorted(name, res["sorted"][0], res["sorted"][1], res["unsorted"][0], res["unsorted"][1], src == 3)
        cu, lu = res["unsorted"][0], res["unsorted"][1]
        disorder += sum(1 for i in zip(*np.nonzero(cu <= SORT_CAP)) if (np.diff(lu[i][:cu[i]].astype(np.int64)) < 0).any())
    assert not bad, bad[:10]
    assert disorder > 0, "not vacuous: table order is not ascending order in some short list of the unsorted runs"


def test_edge_world_has_the_lists_it_was_built_for(rtc, ctxs):
    shapes, lgt = edge_world()
    ctx = ctxs["binned"]
    dw = ctx.upload(K.as_world(rtc, shapes, lgt))
    dw.render(edge_cam())
    counts, lists = G.tile_counts(rtc, ctx, dw)[0][0], tile_lists(rtc, ctx, dw)[0]
    dw.close()
    at = lambda t: int(counts[t[1], t[0]])
    print("edge world tile counts:\n", counts)
    assert (at(T_EMPTY), at(T_ONE), at(T_EIGHT), at(T_NINE), at(T_FULL)) == (0, 1, 8, 9, CAP)
    assert at(T_OVER) == CAP + 6 and at(T_COVER_FIRST) == SORT_CAP + 1 and at(T_COVER_MID) == SORT_CAP
    eq = lists[T_EQUAL[1], T_EQUAL[0], :at(T_EQUAL)]
    assert at(T_EQUAL) == 4 and len(set((eq >> 16).tolist())) == 1 and (np.diff(eq & 0xffff) > 0).all(), eq
    corner = [lists[ty, tx, :counts[ty, tx]] & 0xffff for tx, ty in ((3, 6), (4, 6), (3, 7), (4, 7))]
    assert all((len(shapes) - 2) in c.tolist() for c in corner), corner      # the sphere before the floor: on all four lists
    # the cover comes after the five in front of it in its tile's sorted list: the walk there ends at entry 6
    mid = lists[T_COVER_MID[1], T_COVER_MID[0], :SORT_CAP]
    assert (np.diff(mid.astype(np.int64)) > 0).all() and shapes[mid[5] & 0xffff].inv[0] == pytest.approx(1. / 0.75)


def launches(rtc, ctx, dw, cams_by_launch):
    """Canvases and the ray counters of a context's renders of one World: {launch name: array}, stats."""
    import torch
    out = {}
    ctx.reset_stats()
    for name, cam in cams_by_launch.items():
        if name == "two_views":
            t = torch.zeros((2 * H, W, 3), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            dw.render_views(cam, 0, 1, t.data_ptr(), H)
        elif name == "bands":
            t = torch.zeros((4 * 8, W, 3), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            dw.render_bands(cam, 1, 2, t.data_ptr())
        else:
            t = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            dw.render_rows(cam, 0, H, t.data_ptr())
        ctx.synchronize()
        out[name] = t.cpu().numpy()
    return out, ctx.stats(extended=True)


@pytest.mark.parametrize("variant", ["flat", "reflective", "glass"])
def test_edge_world_renders_what_the_walk_renders(rtc, O, ctxs, variant):
    shapes, lgt = edge_world(variant)
    w = K.as_world(rtc, shapes, lgt)
    cams = {"one": edge_cam(), "four": edge_cam(4), "two_views": [edge_cam(), edge_cam(frm=(1., 3., -9.))], "bands": edge_cam()}
    got = {}
    for name in ("binned", "walk", "pipelined"):
        dw = ctxs[name].upload(w)
        got[name] = launches(rtc, ctxs[name], dw, cams)
        if name != "walk":
            assert ctxs[name].last_launch_info()["binned_primary_pass"]
        dw.close()
    for name in ("binned", "pipelined"):
        for launch, img in got[name][0].items():
            assert img.any() and np.array_equal(img, got["walk"][0][launch]), (variant, name, launch)
        st, sw = dict(got[name][1]), dict(got["walk"][1])
        st.pop("rays_primary_proven_miss"), sw.pop("rays_primary_proven_miss")   # (the walk has no tile rows to prove black)
        assert st == sw, (variant, name, st, sw)
    a = (O.RtcShape * len(shapes))(*shapes)
    want = O.render(a, len(shapes), lgt, cams["one"], mode=1, nthreads=16)
    err = float(np.max(np.abs(got["binned"][0]["one"] - want)))
    print(f"edge world {variant}: max|d oracle| {err:.3e}")
    assert err <= TIGHT_TOL


def test_tile_cases_render_what_the_walk_renders(rtc, ctxs):
    bad = []
    for case in K.tile_cases():
        w = K.as_world(rtc, case.shapes, case.light)
        res = {}
        for name in ("binned", "walk"):
            dw = ctxs[name].upload(w)
            res[name] = dw.render(case.cam, with_stats=True)
            dw.close()
        if not (np.array_equal(res["binned"][0], res["walk"][0]) and res["binned"][1] == res["walk"][1]):
            bad.append(case.name)
    assert not bad, bad
