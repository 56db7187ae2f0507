"""The AOV, ambient-occlusion and gather passes under orthographic and panorama cameras on the HIP path
(rtc_render_aov_projection*, rtc_render_ao_projection*, rtc_render_gather_projection*; the projection instantiations of k_aov,
k_ao and k_gather).

A pixel's ray is rtc_projection_ray's. The expected planes are the normative host packing (rtc_aov_from_hits,
rtc_ao_from_hits, rtc_gather_from_hits) of the CPU oracle's color_at(ray, want_hit=True) records
(tests/projection_pass_cases.py: computed once per case, shared, read-only). AOV planes and AO counts are compared exactly;
radiance and bounce within 1e-12 per light sample, tests/test_gpu_gather.py's TIGHT_TOL. The cases are
tests/projection_cases.py's; every culled launch is checked against its rtc_launch_info::source, so that the one-level walk,
the two-level unordered walk (orthographic) and the two-level ordered walk (panorama) are all reached."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import aov_cases as A
import projection_cases as PC
import projection_pass_cases as PP
from projection_cases import ORTHO, PANO, TIGHT_TOL

pytestmark = pytest.mark.gpu

ASYNC, SERIAL = 1, 0
NO_CULL, LDS_TABLE = 1, 4
ERR_ARG, ERR_UNSUPPORTED = 4, 8
INF = math.inf
CASES = ("flat-ortho", "flat-ortho-straddle", "flat-pano", "flat-pano-16x9", "flat-pano-32x16", "mixed-ortho", "s300-ortho", "s300-pano")
SIZES = {"flat-ortho": (70, 45), "flat-pano-16x9": (16, 9), "flat-pano-32x16": (32, 16), "s300-ortho": (40, 24), "s300-pano": (40, 24)}
NOT_SHADOW = tuple(p for p in A.PLANES if p != "shadow")


def _torch():
    import torch
    return torch


def _assert_same(got, want, what, planes=A.PLANES):
    bad = A.same_planes(got, want, planes)
    assert not bad, f"{what}: planes {bad} differ from the oracle's"


def _info(gpu, proj, source, table=False):
    i = gpu.last_launch_info()
    assert i["source"] == source and i["projection"] == proj.kind, i
    assert i["light_table"] is table and i["lens_samples"] == 0 and i["binned_primary_pass"] is False, i
    return i


# ---- AOV
@pytest.mark.parametrize("name", CASES)
def test_aov_planes_are_the_oracles_in_both_modes_culled_and_brute(rtc, gpu, O, name):
    w, cam, proj = PP.build(rtc, name)
    assert name not in SIZES or (cam.hsize, cam.vsize) == SIZES[name]
    source = PC.CASES[name].source
    assert (source == 4) == (len(w) > 256)
    want = PP.expected_aov(rtc, O, name, ASYNC)
    hit = want["index"] >= 0
    assert hit.any() and (want["shadow"][hit] > 0).any() and (want["shadow"][hit] == 0).any(), name
    if name == "flat-ortho-straddle":   # rays that start inside the sphere the plane cuts: `inside`, the normal flipped
        assert (want["flags"] == 3).any() and (want["flags"] == 1).any()
    dw = gpu.upload(w)
    try:
        got = dw.render_aov(cam, projection=proj)
        _info(gpu, proj, source)
        _assert_same(got, want, name)
        brute = dw.render_aov(cam, flags=NO_CULL, projection=proj)
        _info(gpu, proj, 0)
        assert all(got[p].tobytes() == brute[p].tobytes() for p in A.PLANES), name
        # the instantiation without shadow rays: the other five planes, the same bytes
        five = dw.render_aov(cam, planes=NOT_SHADOW, projection=proj)
        assert sorted(five) == sorted(NOT_SHADOW) and all(five[p].tobytes() == got[p].tobytes() for p in NOT_SHADOW), name
        five_brute = dw.render_aov(cam, planes=NOT_SHADOW, flags=NO_CULL, projection=proj)
        assert all(five_brute[p].tobytes() == got[p].tobytes() for p in NOT_SHADOW), name
        # RTC_MODE_RENDER: the last row and column keep the miss values
        serial = dw.render_aov(cam, mode=SERIAL, projection=proj)
        _assert_same(serial, PP.expected_aov(rtc, O, name, SERIAL), name + " RTC_MODE_RENDER")
        assert (serial["index"][-1] == -1).all() and (serial["index"][:, -1] == -1).all() and np.isinf(serial["depth"][-1]).all()
        assert all(dw.render_aov(cam, mode=SERIAL, flags=NO_CULL, projection=proj)[p].tobytes() == serial[p].tobytes() for p in A.PLANES)
    finally:
        dw.close()


@pytest.mark.parametrize("lights,table", [("two", False), ("nine", True)])
@pytest.mark.parametrize("name", ["flat-ortho", "flat-pano", "s300-ortho", "s300-pano"])
def test_aov_shadow_counts_under_several_lights(rtc, gpu, O, name, lights, table):
    """Two lights ride in the kernel arguments, a 3x3 area light's nine samples in the World's device table."""
    w, cam, proj = PP.build(rtc, name, lights)
    n = len(w.samples())
    assert n == (9 if table else 2)
    want = PP.expected_aov(rtc, O, name, ASYNC, lights)
    counts = want["shadow"][want["index"] >= 0]
    assert counts.max() <= n and ((counts > 0) & (counts < n)).any(), (name, lights)
    dw = gpu.upload(w)
    try:
        got = dw.render_aov(cam, projection=proj)
        _info(gpu, proj, PC.CASES[name].source, table)
        _assert_same(got, want, f"{name}, {lights} lights")
        brute = dw.render_aov(cam, flags=NO_CULL, projection=proj)
        assert all(got[p].tobytes() == brute[p].tobytes() for p in A.PLANES)
        _assert_same(dw.render_aov(cam, mode=SERIAL, projection=proj), PP.expected_aov(rtc, O, name, SERIAL, lights), f"{name}, {lights} lights, RTC_MODE_RENDER")
    finally:
        dw.close()


@pytest.mark.parametrize("name", ["flat-ortho", "flat-pano", "s300-ortho"])
def test_device_entries_write_the_host_entries_bytes(rtc, gpu, O, name):
    """rtc_render_aov_projection_device, rtc_render_ao_projection_device and rtc_render_gather_projection_device into device
    buffers: the bytes of the host entries, and nothing outside the planes asked for."""
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    w, cam, proj = PP.build(rtc, name)
    npx = cam.hsize * cam.vsize
    ao = rtc.ao(0.25, 2, 2)
    dw = gpu.upload(w)
    try:
        host = dw.render_aov(cam, projection=proj)
        host_ao = dw.render_ao(cam, ao, projection=proj)
        host_g = dw.render_gather(cam, ao, projection=proj)
        dev = {p: torch.full((npx * comps * np.dtype(d).itemsize + 16,), 0xA5, dtype=torch.uint8, device="cuda:0") for p, (d, comps) in abi.AOV_PLANES.items()}
        d_ao = torch.full((npx * 2 + 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        d_g = {p: torch.full((npx * 24 + 16,), 0xA5, dtype=torch.uint8, device="cuda:0") for p in ("radiance", "bounce")}
        torch.cuda.synchronize()
        dw.render_aov_device(cam, {p: t.data_ptr() for p, t in dev.items()}, projection=proj)
        dw.render_ao_device(cam, ao, d_ao.data_ptr(), projection=proj)
        dw.render_gather_device(cam, ao, {p: t.data_ptr() for p, t in d_g.items()}, projection=proj)
        gpu.synchronize()
        _info(gpu, proj, PC.CASES[name].source)
        for p in A.PLANES:
            b = dev[p].cpu().numpy()
            assert b[:-16].tobytes() == host[p].tobytes() and (b[-16:] == 0xA5).all(), p
        b = d_ao.cpu().numpy()
        assert b[:-16].tobytes() == host_ao.tobytes() and (b[-16:] == 0xA5).all()
        for p in ("radiance", "bounce"):
            b = d_g[p].cpu().numpy()
            assert b[:-16].tobytes() == host_g[p].tobytes() and (b[-16:] == 0xA5).all(), p
        assert host_ao.any() and host_g["radiance"].any()
    finally:
        dw.close()


# ---- ambient occlusion
@pytest.mark.parametrize("ao", [(0.25, 1, 1), (0.25, 4, 4), (INF, 1, 1), (INF, 4, 4)], ids=lambda a: "r%s-%dx%d" % a)
@pytest.mark.parametrize("name", ["flat-ortho", "flat-pano-32x16", "s300-ortho"])
def test_ao_counts_are_the_oracles(rtc, gpu, O, name, ao):
    w, cam, proj = PP.build(rtc, name)
    want = PP.expected_ao(rtc, O, name, ao, ASYNC)
    n = ao[1] * ao[2]
    assert want.max() <= n
    if n > 1:   # (from the oracle alone: the 4x4 fans of these frames hold open, closed and partly occluded pixels)
        assert want.any() and ((want > 0) & (want < n)).any(), "no pixel is partly occluded"
    spec = rtc.ao(*ao)
    dw = gpu.upload(w)
    try:
        got = dw.render_ao(cam, spec, projection=proj)
        _info(gpu, proj, PC.CASES[name].source)
        assert got.dtype == want.dtype and np.array_equal(got, want), f"{name} {ao}: {int((got != want).sum())} counts differ"
        assert dw.render_ao(cam, spec, flags=NO_CULL, projection=proj).tobytes() == got.tobytes()
        _info(gpu, proj, 0)
        serial = dw.render_ao(cam, spec, mode=SERIAL, projection=proj)
        assert np.array_equal(serial, PP.expected_ao(rtc, O, name, ao, SERIAL)) and not serial[-1].any() and not serial[:, -1].any()
    finally:
        dw.close()


# ---- gather
@pytest.mark.parametrize("lights,table", [("one", False), ("nine", True)])
@pytest.mark.parametrize("name", ["mixed-ortho", "flat-pano"])
def test_gather_planes_are_within_the_tight_bound_of_the_oracle(rtc, gpu, O, name, lights, table):
    ao = (INF if name == "flat-pano" else 1.5, 2, 2)
    w, cam, proj = PP.build(rtc, name, lights)
    n_lights = len(w.samples())
    want = PP.expected_gather(rtc, O, name, ao, ASYNC, lights)
    assert want["radiance"].any() and want["bounce"].any()
    dw = gpu.upload(w)
    try:
        got = dw.render_gather(cam, rtc.ao(*ao), projection=proj)
        _info(gpu, proj, PC.CASES[name].source, table)
        for p in ("radiance", "bounce"):
            err = float(np.max(np.abs(got[p] - want[p])))
            print(f"{name}, {lights} light(s), {p}: max|gpu - oracle| = {err:.3e} (bound {n_lights * TIGHT_TOL:.1e})")
            assert err <= n_lights * TIGHT_TOL, (name, lights, p, err)
            assert np.array_equal(got[p] != 0, want[p] != 0), (name, lights, p)
        brute = dw.render_gather(cam, rtc.ao(*ao), flags=NO_CULL, projection=proj)
        assert all(got[p].tobytes() == brute[p].tobytes() for p in got)
        only = dw.render_gather(cam, rtc.ao(*ao), planes=("bounce",), projection=proj)
        assert list(only) == ["bounce"] and only["bounce"].tobytes() == got["bounce"].tobytes()
    finally:
        dw.close()


# ---- whole frames
@pytest.mark.parametrize("kind", [ORTHO, PANO])
def test_a_480x270_frame_of_the_north_star_world_equals_the_librarys_own_hit_records(rtc, gpu, kind):
    """index, depth and flags of every pixel against rtc_color_at's records of rtc_projection_ray's rays"""
    S = importlib.import_module(rtc.__name__ + ".scenes")
    w, _ = S.synthetic(100, 480, 270)
    view = PC.FLAT_ABOVE if kind == ORTHO else PC.FLAT_AMONG
    cam = rtc.camera(480, 270, 1.0, rtc.Matrix.make_view_transform(*view))
    proj = rtc.projection(ORTHO, width=30.0) if kind == ORTHO else rtc.projection(PANO)
    rays = np.empty((270 * 480, 6))
    ray, fn, camr, projr = (C.c_double * 6)(), rtc.lib().rtc_projection_ray, C.byref(cam), C.byref(proj)
    for y in range(270):
        for x in range(480):
            assert fn(camr, projr, x, y, ray) == 0
            rays[y * 480 + x] = ray[:]
    dw = gpu.upload(w)
    try:
        _, hits = dw.color_at(rays, want_hits=True)
        rec = np.frombuffer(hits, dtype=A.HIT_DTYPE)[:270 * 480].reshape(270, 480)
        got = dw.render_aov(cam, planes=("index", "depth", "flags"), projection=proj)
        _info(gpu, proj, 3)
        hit = rec["hit_index"] >= 0
        assert 0.2 < hit.mean() and len(np.unique(rec["hit_index"])) > 20
        assert np.array_equal(got["index"], rec["hit_index"])
        assert np.array_equal(got["depth"], np.where(hit, rec["t"], np.inf))
        assert np.array_equal(got["flags"], np.where(hit, 1 | (rec["inside"] << 1), 0).astype(np.uint8))
    finally:
        dw.close()


# ---- composition with the filter and the views
def test_the_filter_and_the_depth_view_take_the_new_planes_on_the_device(rtc, gpu, O):
    """rtc_plane_filter_device of an orthographic AO fraction under the orthographic guide planes, and
    rtc_aov_view_rgb8_device of the orthographic depth plane: the host functions' bytes."""
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    name = "flat-ortho"
    w, cam, proj = PP.build(rtc, name)
    width, height, npx = cam.hsize, cam.vsize, cam.hsize * cam.vsize
    spec, flt = rtc.ao(INF, 4, 4), rtc.filter_spec()
    guides = ("index", "point", "normal", "depth")
    dev = {p: torch.zeros(npx * abi.AOV_PLANES[p][1] * np.dtype(abi.AOV_PLANES[p][0]).itemsize, dtype=torch.uint8, device="cuda:0") for p in guides}
    d_ao = torch.zeros(npx * 2, dtype=torch.uint8, device="cuda:0")
    d_frac, d_out = torch.zeros(npx, dtype=torch.float64, device="cuda:0"), torch.zeros(npx, dtype=torch.float64, device="cuda:0")
    pic = torch.zeros(npx * 3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    try:
        host = dw.render_aov(cam, planes=guides, projection=proj)
        counts = dw.render_ao(cam, spec, projection=proj)
        want = rtc.plane_filter(rtc.counts_to_fraction(counts, 16), {p: host[p] for p in ("index", "point", "normal")}, flt)
        finite = host["depth"][np.isfinite(host["depth"])]
        near, far = float(finite.min()), float(finite.max())
        want_pic = rtc.aov_view("depth", host, near=near, far=far)
        dw.render_aov_device(cam, {p: t.data_ptr() for p, t in dev.items()}, projection=proj)
        dw.render_ao_device(cam, spec, d_ao.data_ptr(), projection=proj)
        gpu.counts_to_fraction_device(d_ao.data_ptr(), 16, width, height, d_frac.data_ptr())
        gpu.plane_filter_device(d_frac.data_ptr(), 1, {p: dev[p].data_ptr() for p in ("index", "point", "normal")}, width, height, flt, d_out.data_ptr())
        gpu.aov_view_device("depth", {"depth": dev["depth"].data_ptr()}, width, height, pic.data_ptr(), near=near, far=far)
        gpu.synchronize()
        got = d_out.cpu().numpy().reshape(height, width)
        assert got.tobytes() == want.tobytes() and len(np.unique(want)) > 8
        assert np.array_equal(pic.cpu().numpy().reshape(height, width, 3), want_pic) and len(np.unique(want_pic)) > 8
    finally:
        dw.close()


# ---- the panorama's tables, and the pinhole pass afterwards
def _uploads(rtc, gpu):
    f = rtc.lib().rtc_debug_projection_uploads
    f.argtypes, f.restype = [C.c_void_p, C.POINTER(C.c_ulonglong)], C.c_int32
    out = C.c_ulonglong(0)
    assert f(gpu._h, C.byref(out)) == 0
    return out.value


def test_a_pass_and_a_colour_launch_of_one_panorama_size_upload_the_tables_once(rtc, gpu):
    w, cam, proj = PP.build(rtc, "flat-pano")
    odd = rtc.camera(41, 23, 1.0, rtc.Matrix.make_view_transform(*PC.FLAT_AMONG))   # a size no other test renders
    dw = gpu.upload(w)
    try:
        u0 = _uploads(rtc, gpu)
        dw.render_aov(odd, planes=("index",), projection=proj)
        assert _uploads(rtc, gpu) == u0 + 1
        dw.render_projection(odd, proj)
        dw.render_ao(odd, rtc.ao(1.0, 1, 1), projection=proj)
        dw.render_gather(odd, rtc.ao(1.0, 1, 1), projection=proj)
        assert _uploads(rtc, gpu) == u0 + 1
        dw.render_aov(cam, planes=("index",), projection=proj)   # another size: once more
        _, _, ortho = PP.build(rtc, "flat-ortho")
        dw.render_aov(cam, planes=("index",), projection=ortho)  # an orthographic pass has no tables
        assert _uploads(rtc, gpu) == u0 + 2
    finally:
        dw.close()


def test_a_pinhole_pass_after_a_projection_pass_gives_the_bytes_it_gave_before(rtc, gpu):
    w, cam, pano = PP.build(rtc, "flat-pano")
    _, _, ortho = PP.build(rtc, "flat-ortho")
    ao = rtc.ao(1.0, 2, 2)
    dw = gpu.upload(w)
    try:
        before = dw.render_aov(cam), dw.render_ao(cam, ao), dw.render_gather(cam, ao)
        for proj in (ortho, pano):
            other = dw.render_aov(cam, projection=proj)
            assert other["index"].tobytes() != before[0]["index"].tobytes()
            dw.render_ao(cam, ao, projection=proj)
            dw.render_gather(cam, ao, projection=proj)
            assert gpu.last_launch_info()["projection"] == proj.kind
            after = dw.render_aov(cam), dw.render_ao(cam, ao), dw.render_gather(cam, ao)
            assert all(after[0][p].tobytes() == before[0][p].tobytes() for p in A.PLANES)
            assert after[1].tobytes() == before[1].tobytes()
            assert all(after[2][p].tobytes() == before[2][p].tobytes() for p in before[2])
        dw.render(cam)
        assert gpu.last_launch_info()["projection"] == 0
    finally:
        dw.close()


# ---- error returns
def test_error_returns(rtc, gpu):
    abi = importlib.import_module(rtc.__name__ + ".abi")
    L = rtc.lib()
    w, cam, ok = PP.build(rtc, "flat-pano")
    npx = cam.hsize * cam.vsize
    idx = np.full(npx, 7, dtype=np.int32)
    b = abi.RtcAovBuffers()
    b.index = idx.ctypes.data
    none = abi.RtcAovBuffers()
    counts = np.full(npx, 7, dtype=np.uint16)
    pc = counts.ctypes.data_as(C.POINTER(C.c_uint16))
    rad = np.full(npx * 3, 7.0)
    g = abi.RtcGatherBuffers()
    g.radiance = rad.ctypes.data
    ao, bad_ao = rtc.ao(1.0, 2, 2), rtc.ao(1.0, 2, 2)
    bad_ao.usteps = 0

    def proj(kind, width=0.0, h_span=0.0, v_span=0.0):
        q = abi.RtcProjection()
        q.kind, q.width, q.h_span, q.v_span = kind, width, h_span, v_span
        return q
    aa = abi.RtcCamera()
    C.memmove(C.byref(aa), C.byref(cam), C.sizeof(abi.RtcCamera))
    aa.samples = 4
    dw = gpu.upload(w)
    try:
        aov = lambda c, q, mode=1, flags=0, buf=b: L.rtc_render_aov_projection(gpu._h, dw._h, c, q, mode, flags, C.byref(buf))
        occ = lambda c, q, a=ao, mode=1: L.rtc_render_ao_projection(gpu._h, dw._h, c, q, C.byref(a), mode, 0, pc)
        gat = lambda c, q, a=ao, mode=1: L.rtc_render_gather_projection(gpu._h, dw._h, c, q, C.byref(a), mode, 0, C.byref(g))
        for call in (aov, occ, gat):
            for bad in (proj(0, 1.0, 1.0, 1.0), proj(3, 1.0, 1.0, 1.0), proj(ORTHO, 0.0), proj(ORTHO, -2.0), proj(ORTHO, float("inf")),
                        proj(PANO, 0.0, 0.0, 1.0), proj(PANO, 0.0, 7.0, 1.0), proj(PANO, 0.0, 1.0, 3.2), proj(PANO, 0.0, float("nan"), 1.0)):
                assert call(C.byref(cam), C.byref(bad)) == ERR_ARG, (bad.kind, bad.width, bad.h_span, bad.v_span)
            assert call(C.byref(cam), None) == ERR_ARG
            assert call(None, C.byref(ok)) == ERR_ARG
            assert call(C.byref(aa), C.byref(ok)) == ERR_ARG          # anti-aliasing and the projections do not compose
            assert call(C.byref(cam), C.byref(ok), mode=2) == ERR_ARG  # no such mode
        assert aov(C.byref(cam), C.byref(ok), buf=none) == ERR_ARG     # the pinhole pass's own checks
        assert occ(C.byref(cam), C.byref(ok), a=bad_ao) == ERR_ARG and gat(C.byref(cam), C.byref(ok), a=bad_ao) == ERR_ARG
        assert aov(C.byref(cam), C.byref(ok), flags=NO_CULL | LDS_TABLE) == L.rtc_render_aov(gpu._h, dw._h, C.byref(cam), 1, NO_CULL | LDS_TABLE, C.byref(b)) == ERR_UNSUPPORTED
        assert L.rtc_render_aov_projection(None, dw._h, C.byref(cam), C.byref(ok), 1, 0, C.byref(b)) == ERR_ARG
        assert L.rtc_render_aov_projection(gpu._h, None, C.byref(cam), C.byref(ok), 1, 0, C.byref(b)) == ERR_ARG
        assert L.rtc_render_aov_projection(gpu._h, dw._h, C.byref(cam), C.byref(ok), 1, 0, None) == ERR_ARG
        assert L.rtc_render_aov_projection_device(gpu._h, dw._h, C.byref(cam), None, 1, 0, C.byref(b)) == ERR_ARG
        assert L.rtc_render_ao_projection_device(gpu._h, dw._h, C.byref(cam), None, C.byref(ao), 1, 0, pc) == ERR_ARG
        assert L.rtc_render_gather_projection_device(gpu._h, dw._h, C.byref(cam), None, C.byref(ao), 1, 0, C.byref(g)) == ERR_ARG
        assert (idx == 7).all() and (counts == 7).all() and (rad == 7.0).all()   # nothing was written
        gpu.reset_stats()   # the passes stay uncounted in rtc_stats
        dw.render_aov(cam, projection=ok)
        dw.render_ao(cam, ao, projection=ok)
        assert all(v == 0 for v in gpu.stats().values())
        assert (dw.render_aov(cam, planes=("index",), projection=ok)["index"] >= 0).any()   # and the World still renders
    finally:
        dw.close()


# ---- the scene file and the tool
def test_the_aov_tool_renders_the_orthographic_scene_with_its_passes(rtc, gpu, tmp_path):
    """tools/render_aov.py data/passes/orthographic_passes.yml OUT --ao --filter --exr: the files it writes for a pinhole scene,
    under the scene's orthographic camera; and the scene's index plane through the loader entry is not the pinhole's."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    scene = Path(rtc.__file__).resolve().parent / "data" / "passes" / "orthographic_passes.yml"
    r = subprocess.run([sys.executable, str(root / "tools" / "render_aov.py"), str(scene), str(tmp_path), "--ao", "--filter", "--exr"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "orthographic" in r.stdout and "480x270" in r.stdout
    for name in ("beauty", "depth", "normal", "index", "shadow", "ao", "beauty_ao", "ao_filtered", "beauty_ao_filtered"):
        assert (tmp_path / f"{name}.png").read_bytes()[:8] == b"\x89PNG\r\n\x1a\n", name
    assert (tmp_path / "frame.exr").read_bytes()[:4] == b"\x76\x2f\x31\x01"
    w, cam, lens, proj, ao, gather, flt = rtc.load_yaml_projection_passes(path=scene)
    dw = gpu.upload(w)
    try:
        ortho = dw.render_aov(cam, planes=("index",), projection=proj)["index"]
        assert set(np.unique(ortho)) == {-1, 0, 1, 2, 3, 4} or set(np.unique(ortho)) == {0, 1, 2, 3, 4}   # every shape is in view
        assert ortho.tobytes() != dw.render_aov(cam, planes=("index",))["index"].tobytes()
        counts = dw.render_ao(cam, ao, projection=proj)
        assert ((counts > 0) & (counts < 16)).any() and (counts == 0).any()
    finally:
        dw.close()
