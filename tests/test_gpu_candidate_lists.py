"""The candidate-list cases on the HIP path (tests/candidate_list_cases.py): every case on the default, a forced-binned,
the walking and a pipelined forced-binned context — canvas and ray counts equal to the same context's brute force
(RTC_FLAG_NO_CULL) bit for bit and to the oracle within TIGHT_TOL with exact counts, the launch on the path the case is for,
and the read-backs (rtc_debug_world_lists, rtc_debug_tile_counts: unlisted exports, bound here by hand) showing the list
count, n_unb, cap or reach the case was built to produce."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


sys.path.insert(0, str(Path(__file__).parent))
K = __import__("candidate_list_cases").sibling("candidate_list_cases")     # (one copy per process: the helper's own loader)
_ctx_env = K.sibling("test_gpu_group")._ctx_env
TIGHT_TOL = K.sibling("test_gpu_parity").TIGHT_TOL
CASES = K.all_cases()
CELLS = 6 * K.LIGHT_R * K.LIGHT_R


# ------------------------------------------------------------------ the read-backs
def world_lists(rtc, dw, cells=False, bounds=False):
    f = rtc.lib().rtc_debug_world_lists
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    info, reach = (C.c_uint32 * 4)(), C.c_double()
    cnt = np.zeros(CELLS, dtype=np.uint32) if cells else None
    bnd = np.zeros((max(1, dw.n), 6), dtype=np.float64) if bounds else None
    assert f(dw._h, info, C.byref(reach), cnt.ctypes.data if cells else None, bnd.ctypes.data if bounds else None) == 0
    return {"n_unb": info[0], "ngroups": info[1], "cap": info[2], "n": info[3], "reach": reach.value, "cells": cnt, "bounds": bnd}


def tile_counts(rtc, ctx, dw):
    """(counts[view, ty, tx], rows[view] = (smallest, largest non-empty tile row)) of the context's last launch, or None."""
    f = rtc.lib().rtc_debug_tile_counts
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    dims = (C.c_uint32 * 4)()
    assert f(ctx._h, dw._h, dims, None, 0, None, 0) == 0
    if not dims[0]:
        return None
    cnt, rows = np.zeros(dims[1] * dims[2] * dims[3], dtype=np.uint32), np.zeros(2 * dims[1], dtype=np.uint32)
    assert f(ctx._h, dw._h, dims, cnt.ctypes.data, cnt.size, rows.ctypes.data, rows.size) == 0 and dims[0] == 1
    return cnt.reshape(dims[1], dims[3], dims[2]), [(int(rows[2 * v]), int(~rows[2 * v + 1] & 0xffffffff)) for v in range(dims[1])]


@pytest.fixture(scope="module")
def ctxs(rtc):
    out = {"default": rtc.Context(0), "binned": _ctx_env(rtc, RTC_BIN_SMALL_PIXELS=0), "walk": _ctx_env(rtc, RTC_BINNING=0, RTC_LIGHT_LISTS=0),
           "pipelined": _ctx_env(rtc, RTC_BIN_SMALL_PIXELS=0, RTC_BIN_SMALL_PIXELS_PIPELINED=0)}
    out["pipelined"].set_pipeline(3)
    yield out
    for c in out.values():
        c.close()


def render_on(rtc, name, ctx, dw, cam, mode):
    """(canvas, stats, rays_primary_proven_miss, launch info) of the culled render; the pipelined context: three launches
    into distinct buffers."""
    if name != "pipelined":
        img, st = dw.render(cam, mode, with_stats=True)
        return img, st, ctx.stats(extended=True)["rays_primary_proven_miss"], ctx.last_launch_info()
    import torch
    ring = [torch.full((cam.vsize, cam.hsize, 3), -1.0, dtype=torch.float64, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    ctx.reset_stats()
    for t in ring:
        dw.render_rows(cam, 0, cam.vsize, t.data_ptr(), mode)
    ctx.synchronize()
    info, st = ctx.last_launch_info(), ctx.stats(extended=True)
    imgs = [t.cpu().numpy() for t in ring]
    assert np.array_equal(imgs[0], imgs[1]) and np.array_equal(imgs[0], imgs[2]), "pipelined lanes differ"
    assert all(v % 3 == 0 for v in st.values()), st
    st = {k: v // 3 for k, v in st.items()}
    return imgs[0], st, st.pop("rays_primary_proven_miss"), info


def proven_rays(cam, mode, rows):
    """The primary rays of the tile rows outside the row words [rows[0], rows[1]]: what k_trace answers without a ray."""
    serial = 1 if mode == 0 else 0
    n = 0
    for ty in range((cam.vsize + 7) // 8):
        if ty < rows[0] or ty > rows[1]:
            traced = min(8, cam.vsize - 8 * ty) - (serial if 8 * ty + 8 >= cam.vsize else 0)
            n += traced * (cam.hsize - serial)
    return n


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_on_every_context(rtc, O, ctxs, case):
    w = K.as_world(rtc, case.shapes, case.light)
    src = 3 if case.n <= 256 else 4
    bad = []
    for mode in case.modes:
        want, ost = O.render(case.arr(), case.n, case.light, case.cam, mode=mode, nthreads=16, want_stats=True)
        for name, ctx in ctxs.items():
            dw = ctx.upload(w)
            try:
                img, st, proven, info = render_on(rtc, name, ctx, dw, case.cam, mode)
                tiles = tile_counts(rtc, ctx, dw)
                # rays_primary_proven_miss (as test_tile_rows_proven_black_are_skipped_exactly takes it: apart from the other
                # counters): exactly the rays of the tile rows outside the row words, none without lists, and never more than
                # the black pixels
                want_proven = proven_rays(case.cam, mode, tiles[1][0]) if tiles is not None else 0
                if proven != want_proven or proven > st["rays_primary"] - np.count_nonzero(img.reshape(-1, 3).any(axis=1)):
                    bad.append((name, mode, "proven-miss rays", proven, want_proven))
                brute, sb = dw.render(case.cam, mode, flags=rtc.FLAG_NO_CULL, with_stats=True)
                err = float(np.max(np.abs(img - want)))
                print(f"{case.name} mode {mode} {name}: max|d oracle| {err:.3e} equal brute {np.array_equal(img, brute)} stats {st} "
                      f"proven {proven} binned {info['binned_primary_pass']} lists {info['light_lists']} source {info['source']}")
                if not (np.array_equal(img, brute) and st == sb):
                    bad.append((name, mode, "differs from brute force", int(np.count_nonzero((img != brute).any(axis=2))), st, sb))
                if not (err <= TIGHT_TOL and st == ost):
                    bad.append((name, mode, "differs from the oracle", err, st, ost))
                binned = {"default": src == 4, "binned": True, "pipelined": True, "walk": False}[name]
                lists = case.lists and name != "walk"
                if (info["source"], info["binned_primary_pass"], info["light_lists"]) != (src, binned, lists):
                    bad.append((name, mode, "launch path", info["source"], info["binned_primary_pass"], info["light_lists"]))
                if (tiles is not None) != binned:
                    bad.append((name, mode, "tile read-back", tiles is not None))
                if name == "binned":
                    bad += [(name, mode) + b for b in check_readbacks(rtc, case, dw, tiles)]
            finally:
                dw.close()
    assert not bad, bad


def check_readbacks(rtc, case, dw, tiles):
    bad = []
    wl = world_lists(rtc, dw, cells=True)
    counts, rows = tiles
    print(f"{case.name}: n {wl['n']} n_unb {wl['n_unb']} ngroups {wl['ngroups']} cap {wl['cap']} reach {wl['reach']:.6g} rows {rows[0]} "
          f"max tile count {counts.max()} max cell count {wl['cells'].max()} cells over cap {int((wl['cells'] > max(1, wl['cap'])).sum())}")
    if (wl["n"], wl["ngroups"], wl["cap"]) != (case.n, (case.n + 63) // 64, case.cap):
        bad.append(("world", wl["n"], wl["ngroups"], wl["cap"]))
    if "n_unb" in case.want and wl["n_unb"] != case.want["n_unb"]:
        bad.append(("n_unb", wl["n_unb"]))
    if "tile" in case.want:
        tx, ty, k = case.want["tile"]
        if counts[0, ty, tx] != k:
            bad.append(("tile count", int(counts[0, ty, tx]), k))
    if "rows" in case.want and rows[0] != case.want["rows"]:
        bad.append(("row words", rows[0], case.want["rows"]))
    if "cell" in case.want:
        cell, k = case.want["cell"]
        if wl["cells"][cell] != k:
            bad.append(("cell count", int(wl["cells"][cell]), k))
    if "cell_min" in case.want and wl["cells"].min() < case.want["cell_min"]:
        bad.append(("cell minimum", int(wl["cells"].min())))
    if "reach" in case.want and not case.want["reach"][0] <= wl["reach"] <= case.want["reach"][1]:
        bad.append(("reach", wl["reach"], case.want["reach"]))
    if case.decision == "light_reach":      # with the World's own reach: hit points on both sides
        ds = [K.light_dist(case, h) for _, _, h in K.hits_of(case, 2) if h.hit_index == case.n - 1]
        if not (min(ds) < wl["reach"] < max(ds)):
            bad.append(("reach sides", min(ds), wl["reach"], max(ds)))
    return bad


def test_eight_views_in_one_launch_equal_the_single_renders(rtc, ctxs):
    """One binned launch of 8 views — the cases' camera poses over one world: roll, straight down, inside a sphere, a cube
    and a glass sphere (each around its own camera), a scaled and a mirrored view matrix — against the walking context's
    and brute force's single renders. (The pose 1e6 away needs its world moved with it: camera_pose[far_1e6] only.)"""
    import torch
    W, H = 64, 48
    eyes = {"sphere": (-7., 2., -9.), "cube": (7., 2., -9.), "glass": (0., 2., -16.)}
    shapes = list(K.field_world(61, seed=7))
    shapes += [K.ball(eyes["sphere"], 2.5, color=(0.6, 0.7, 0.9)),
               K.shp(K.CUBE, ("scaling", 3., 3., 3.), ("rotation_y", 0.4), ("translation", *eyes["cube"]), m=K.mat(color=(0.6, 0.9, 0.7))),
               K.ball(eyes["glass"], 2.5, color=(0.1, 0.1, 0.1), transparency=0.9, refractive_index=1.5, reflective=0.2)]
    cams = [K.cam_of(W, H, 0.9, (0., 2., -8.), (0., 1., 5.), up=(1., 1., 0.)), K.cam_of(W, H, 0.9, (0., 5., 0.), (0., 0., 0.), up=(0., 0., 1.)),
            K.cam_of(W, H, 0.9, eyes["sphere"], (0., 1., 5.)), K.cam_of(W, H, 0.9, eyes["cube"], (0., 1., 5.)), K.cam_of(W, H, 0.9, eyes["glass"], (0., 1., 5.)),
            K.cam_of(W, H, 0.9, (0., 2., -8.), (0., 1., 5.), pre=("scaling", 2., 1., 1.)), K.cam_of(W, H, 0.9, (0., 2., -8.), (0., 1., 5.), pre=("scaling", -1., 1., 1.)),
            K.cam_of(W, H, 0.9, (0., 2., -8.), (0., 1., 5.))]
    w = K.as_world(rtc, K.number(shapes), K.O.light((-4., 6., -3.)))
    dwb, dww = ctxs["binned"].upload(w), ctxs["walk"].upload(w)
    t = torch.zeros((8 * H, W, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dwb.render_views(cams, 0, 1, t.data_ptr(), H)
    ctxs["binned"].synchronize()
    counts, rows = tile_counts(rtc, ctxs["binned"], dwb)
    assert counts.shape == (8, 6, 8) and ctxs["binned"].last_launch_info()["binned_primary_pass"]
    th = t.cpu().numpy()
    for v, cam in enumerate(cams):
        single, brute = dww.render(cam), dwb.render(cam, flags=rtc.FLAG_NO_CULL)
        assert single.any() and np.array_equal(th[v * H:(v + 1) * H], single) and np.array_equal(single, brute), v
    dwb.close()
    dww.close()


@pytest.mark.parametrize("name", ["light_count[320]", "plane_count[4]"])
def test_one_ranks_bands_equal_the_rows_of_the_full_frame(rtc, ctxs, name):
    import torch
    case = next(c for c in CASES if c.name == name)
    w = K.as_world(rtc, case.shapes, case.light)
    dwb, dww = ctxs["binned"].upload(w), ctxs["walk"].upload(w)
    full = dww.render(case.cam)
    H, W = case.cam.vsize, case.cam.hsize
    nb = -(-H // 8)
    mine = list(range(1, nb, 3))
    t = torch.zeros((len(mine) * 8, W, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    dwb.render_bands(case.cam, 1, 3, t.data_ptr())
    ctxs["binned"].synchronize()
    assert ctxs["binned"].last_launch_info()["binned_primary_pass"]
    th = t.cpu().numpy()
    for k, band in enumerate(mine):
        rows = min(8, H - band * 8)
        assert np.array_equal(th[k * 8:k * 8 + rows], full[band * 8:band * 8 + rows]), (name, band)
    assert full.any()
    dwb.close()
    dww.close()


@pytest.mark.parametrize("size", ["small", "large"])
def test_seeded_list_worlds_equal_brute_force_and_the_oracle(rtc, O, ctxs, size):
    """40 seeds per size class (as test_cull_is_exact_on_adversarial_scenes) on the forced-binned context against brute force;
    every small world and every fourth large one against the oracle."""
    bad = []
    for seed in range(40):
        shapes, lgt, cam = K.list_world(seed, size)
        dw = ctxs["binned"].upload(K.as_world(rtc, shapes, lgt))
        img, st = dw.render(cam, with_stats=True)
        info = ctxs["binned"].last_launch_info()
        brute, sb = dw.render(cam, flags=rtc.FLAG_NO_CULL, with_stats=True)
        if not (np.array_equal(img, brute) and st == sb):
            bad.append((seed, "brute force", int(np.count_nonzero((img != brute).any(axis=2))), st, sb))
        if not (info["binned_primary_pass"] and info["light_lists"] == (world_lists(rtc, dw)["cap"] != 0)):
            bad.append((seed, "launch path", info))
        if size == "small" or seed % 4 == 0:
            a = (O.RtcShape * len(shapes))(*shapes)
            want, ost = O.render(a, len(shapes), lgt, cam, mode=1, nthreads=16, want_stats=True)
            err = float(np.max(np.abs(img - want)))
            if not (err <= TIGHT_TOL and st == ost):
                bad.append((seed, "oracle", err, st, ost))
        dw.close()
    assert not bad, bad


def test_bound_of_encloses_every_surface_point(rtc, gpu):
    """bound_of (rtc_api.cpp) against a plain reference: for spheres and cubes under shear, anisotropic scale and rotation,
    surface points computed in numpy longdouble from F = inv^-1 (unit-sphere points; the cube's corners and edges) all lie
    inside the (c, r) sphere read back from the World. Exactly the two ill-conditioned objects are reported unbounded."""
    rng = np.random.default_rng(2024)
    u = lambda a, b: float(rng.uniform(a, b))
    shapes = []
    for i in range(240):
        ops = (("scaling", 10. ** u(-2, 1), 10. ** u(-2, 1), 10. ** u(-2, 1)), ("shearing", *[u(-2, 2) for _ in range(6)]), ("rotation_x", u(0, 6.3)),
               ("rotation_y", u(0, 6.3)), ("rotation_z", u(0, 6.3)), ("translation", 10. ** u(-1, 4) * u(-1, 1), u(-50, 50), u(-50, 50)))
        try:
            shapes.append(K.shp(K.CUBE if i % 2 else K.SPHERE, *ops))
        except ValueError:
            pass
    assert len(shapes) > 200
    shapes += [K.ill_conditioned(K.SPHERE, (0.5, 1., 6.)), K.ill_conditioned(K.CUBE, (-1., 0.5, 7.))]
    dw = gpu.upload(K.as_world(rtc, K.number(shapes), K.O.light()))
    wl = world_lists(rtc, dw, bounds=True)
    dw.close()
    LD = np.longdouble
    v = rng.normal(size=(3000, 3))
    sphere_pts = (v / np.linalg.norm(v, axis=1)[:, None]).astype(LD)
    s = np.linspace(-1., 1., 41)
    edges = [np.stack([np.full_like(s, a), np.full_like(s, b), s], axis=1) for a in (-1., 1.) for b in (-1., 1.)]
    cube_pts = np.concatenate([np.roll(e, k, axis=1) for e in edges for k in range(3)]).astype(LD)   # 12 edges incl. the 8 corners
    unbounded, worst = 0, 0.
    for i, sh in enumerate(shapes):
        cx, cy, cz, r = wl["bounds"][i, :4]
        if not np.isfinite(r):
            unbounded += 1
            continue
        m = np.array(list(sh.inv), dtype=LD).reshape(4, 4)
        a, t = m[:3, :3], m[:3, 3]
        det = (a[0, 0] * (a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) - a[0, 1] * (a[1, 0] * a[2, 2] - a[1, 2] * a[2, 0]) +
               a[0, 2] * (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]))
        F = np.array([[a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
                      [a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
                      [a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]], dtype=LD) / det
        pts = (sphere_pts if sh.kind == K.SPHERE else cube_pts) @ F.T - F @ t
        d = np.sqrt(((pts - np.array([cx, cy, cz], dtype=LD)) ** 2).sum(axis=1))
        worst = max(worst, float(d.max() / LD(r)))
        assert d.max() <= LD(r), (i, sh.kind, float(d.max()), r)
        # (not vacuous: the sphere is the surface's own scale, not a huge one)
        assert r <= 2.5 * float(d.max()) + 1e-6, (i, sh.kind, float(d.max()), r)
    print(f"bound_of: {len(shapes)} objects, {unbounded} unbounded, worst distance / radius {worst:.9f}")
    assert unbounded == 2 and wl["n_unb"] == 2
