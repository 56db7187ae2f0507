"""AOV planes on the HIP path (rtc_render_aov*, k_aov; rtc_aov_view_rgb8_device, k_aov_view).

The expected planes are rtc_aov_from_hits of the CPU oracle's color_at(..., want_hit=True) for every pixel's centre ray; the
shadow counts are the sum, over the World's light samples (rtc_area_light_expand), of the oracle's `shadowed` under that sample
alone. Every comparison is exact (np.array_equal, +inf == +inf): the kernels' hit records are bit-identical to the oracle's.
Each test asserts from the expected data that the classes it is about are in its frame."""
import ctypes as C
import importlib

import numpy as np
import pytest

import aov_cases as A

pytestmark = pytest.mark.gpu

ASYNC, SERIAL = 1, 0
NO_CULL, LDS_TABLE, AA_RESAMPLE = 1, 4, 2
ROWS = ("mixed", "s21", "default", "shell", "s301", "twice", "s40x2")
SENTINEL = 0xA5


def _torch():
    import torch
    return torch


def _render(rtc, gpu, name, mode=ASYNC, flags=0, planes=A.PLANES):
    w, cam = A.world(rtc, name)
    dw = gpu.upload(w)
    try:
        return dw.render_aov(cam, planes, mode, flags)
    finally:
        dw.close()


def _assert_same(got, want, what, planes=A.PLANES):
    bad = A.same_planes(got, want, planes)
    detail = ""
    for p in bad:
        d = np.argwhere(got[p] != want[p])
        detail += f" {p}: {len(d)} entries differ, first at {d[0].tolist() if len(d) else '?'}"
    assert bad == [], what + detail


def _classes(want):
    """What an expected frame contains."""
    hit = want["index"] >= 0
    return {"hits": int(hit.sum()), "misses": int((~hit).sum()), "inside": int(((want["flags"] & 2) != 0).sum()),
            "shadowed": int((want["shadow"] > 0).sum()), "counts": sorted(set(want["shadow"][hit].tolist()))}


@pytest.mark.parametrize("name", ROWS)
def test_all_planes_equal_the_oracles_records(rtc, gpu, O, name):
    """1. All six planes for every row of the table (RTC_MODE_RENDER_ASYNC); the first two also in RTC_MODE_RENDER."""
    w, cam = A.world(rtc, name)
    want = A.expected(rtc, O, name, ASYNC)
    c = _classes(want)
    print(name, f"{cam.hsize}x{cam.vsize}", len(w), "objects:", c)
    kinds = {w.shapes[i].kind for i in set(want["index"][want["index"] >= 0].tolist())}
    if name == "mixed":
        assert kinds == {rtc.SPHERE, rtc.PLANE, rtc.CUBE} and c["inside"] > 0 and c["shadowed"] > 0 and c["misses"] == 0 and len(w) == 26
        assert cam.hsize % 8 and cam.vsize % 8   # partial tiles on both edges
    elif name == "s21":
        assert c["hits"] > 0 and c["misses"] > 0 and c["shadowed"] > 0 and len(w) == 21
    elif name == "default":
        assert 0 < c["hits"] < c["misses"] and len(w) == 2
    elif name == "shell":
        assert c["inside"] > c["hits"] // 2 and c["misses"] == 0 and len(w) == 3
    elif name == "s301":
        assert c["hits"] > 0 and c["misses"] > 0 and c["shadowed"] > 0 and len(w) == 301   # two-level cull
    elif name == "twice":
        sphere_px = want["index"][(want["index"] >= 0) & (want["index"] < 300)]
        assert len(w) == 301 and sphere_px.size > 0 and (sphere_px < 150).all()   # the lower index wins every tie
    elif name == "s40x2":
        assert c["counts"] == [0, 1, 2] and len(w) == 40
    got = _render(rtc, gpu, name, ASYNC)
    _assert_same(got, want, f"{name} async")
    if name in ("mixed", "s21"):
        ws = A.expected(rtc, O, name, SERIAL)
        assert (ws["index"][-1, :] == -1).all() and (ws["index"][:, -1] == -1).all() and (want["index"][-1, :] >= 0).any()
        _assert_same(_render(rtc, gpu, name, SERIAL), ws, f"{name} serial")


@pytest.mark.parametrize("name", ROWS)
def test_no_cull_gives_the_same_bytes(rtc, gpu, O, name):
    """2. RTC_FLAG_NO_CULL (SRC_SMEM) against the culled kernels (SRC_CULL up to 256 objects, SRC_CULL2 above)."""
    want = A.expected(rtc, O, name, ASYNC)
    _assert_same(_render(rtc, gpu, name, ASYNC, NO_CULL), want, f"{name} no-cull")
    # RTC_FLAG_AA_RESAMPLE is ignored
    _assert_same(_render(rtc, gpu, name, ASYNC, AA_RESAMPLE, ("index", "depth")), want, f"{name} aa flag", ("index", "depth"))


@pytest.mark.parametrize("size", ["1x1", "8x8", "9x7", "65x9"])
def test_frame_sizes(rtc, gpu, O, size):
    """3. One pixel, exactly one tile, one tile and a bit both ways, more than eight tiles with a one-pixel last column."""
    name = "s21:" + size
    want = A.expected(rtc, O, name, ASYNC)
    if size != "1x1":
        assert (want["index"] >= 0).any()
    _assert_same(_render(rtc, gpu, name, ASYNC), want, name)
    _assert_same(_render(rtc, gpu, name, SERIAL), A.expected(rtc, O, name, SERIAL), name + " serial")
    _assert_same(_render(rtc, gpu, name, ASYNC, NO_CULL), want, name + " no-cull")


@pytest.mark.parametrize("name,n_samples", [("s40x2", 2), ("s40area9", 9), ("s40area256", 256)])
def test_shadow_counts_per_light_sample(rtc, gpu, O, name, n_samples):
    """4. Two lights (kernel arguments), a 3x3 area light (the device table), a 16x16 area light (256 samples: the cap)."""
    w, cam = A.world(rtc, name)
    assert len(w.samples()) == n_samples and len(w) == 40
    want = A.expected(rtc, O, name, ASYNC)
    counts = want["shadow"][want["index"] >= 0]
    print(name, "shadow counts:", dict(zip(*[v.tolist() for v in np.unique(counts, return_counts=True)])))
    assert counts.max() > 0 and counts.min() == 0 and counts.max() <= n_samples
    if n_samples > 2:
        assert ((counts > 0) & (counts < n_samples)).any()   # a penumbra: some samples hidden, not all
    dw = gpu.upload(w)
    try:
        assert rtc.lib().rtc_world_light_count(dw._h) == n_samples
        culled = dw.render_aov(cam)
        brute = dw.render_aov(cam, flags=NO_CULL)
    finally:
        dw.close()
    _assert_same(culled, want, name)
    _assert_same(brute, want, name + " no-cull")


@pytest.mark.parametrize("wanted", [("index",), ("shadow",), ("index", "depth", "point", "normal", "flags")])
def test_plane_selection_on_the_device(rtc, gpu, O, wanted):
    """5. Only the planes asked for are written: the other device buffers keep their sentinel fill."""
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    w, cam = A.world(rtc, "s21")
    want = A.expected(rtc, O, "s21", ASYNC)
    npx = cam.hsize * cam.vsize
    bufs = {p: torch.full((npx * comps * np.dtype(d).itemsize,), SENTINEL, dtype=torch.uint8, device="cuda:0") for p, (d, comps) in abi.AOV_PLANES.items()}
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    try:
        dw.render_aov_device(cam, {p: bufs[p].data_ptr() for p in wanted})
        gpu.synchronize()
    finally:
        dw.close()
    for p, (d, comps) in abi.AOV_PLANES.items():
        host = bufs[p].cpu().numpy()
        if p in wanted:
            assert host.tobytes() == want[p].tobytes(), p
        else:
            assert (host == SENTINEL).all(), p


def test_update_is_ordered_with_the_launches(rtc, gpu, O):
    """6. After DeviceWorld.update with a moved sphere the next AOV launch shows the new World; the one enqueued before it
    shows the old."""
    torch = _torch()
    w, cam = A.world(rtc, "s21")
    moved = rtc.World(w.lights)
    for s in w.shapes:
        moved.add_shape(s)
    # the sphere most pixels see, lifted by one unit
    want_old = A.expected(rtc, O, "s21", ASYNC)
    j = int(np.bincount(want_old["index"][(want_old["index"] >= 0) & (want_old["index"] < 20)]).argmax())
    t = rtc.Matrix(list(w.shapes[j].inv)).inverse().translation(0.0, 1.0, 0.0)
    moved.shapes[j] = rtc.sphere(t, w.shapes[j].material)
    moved.shapes[j].world_id = j + 1
    npx = cam.hsize * cam.vsize
    old_d, new_d = (torch.zeros(npx, dtype=torch.int32, device="cuda:0") for _ in range(2))
    old_t, new_t = (torch.zeros(npx, dtype=torch.float64, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    dw = gpu.upload(w)
    try:
        dw.render_aov_device(cam, {"index": old_d.data_ptr(), "depth": old_t.data_ptr()})
        dw.update(moved)
        dw.render_aov_device(cam, {"index": new_d.data_ptr(), "depth": new_t.data_ptr()})
        gpu.synchronize()
        after = dw.render_aov(cam)
    finally:
        dw.close()
    fresh = gpu.upload(moved)
    try:
        want_new = fresh.render_aov(cam)
    finally:
        fresh.close()
    shape = (cam.vsize, cam.hsize)
    assert np.array_equal(old_d.cpu().numpy().reshape(shape), want_old["index"]) and np.array_equal(old_t.cpu().numpy().reshape(shape), want_old["depth"])
    assert np.array_equal(new_d.cpu().numpy().reshape(shape), want_new["index"]) and np.array_equal(new_t.cpu().numpy().reshape(shape), want_new["depth"])
    assert not np.array_equal(want_new["depth"], want_old["depth"])
    _assert_same(after, want_new, "after the update")
    # ... and the updated World's planes are the oracle's for the moved World
    arr, n = moved.array(), len(moved)
    for (x, y) in [(px, py) for py in range(0, cam.vsize, 3) for px in range(0, cam.hsize, 3)]:
        _, h = O.color_at(arr, n, moved.light, tuple(rtc.ray_for_pixel(cam, x, y)), 5, want_hit=True)
        assert want_new["index"][y, x] == h.hit_index and (h.hit_index < 0 or (want_new["depth"][y, x] == h.t and want_new["shadow"][y, x] == h.shadowed))


@pytest.mark.parametrize("name", ["mixed", "s21"])
def test_views_on_the_device_equal_the_host_views(rtc, gpu, O, name):
    """7. rtc_aov_view_rgb8_device writes rtc_aov_view_rgb8's bytes, and the device picture goes straight into the encoders."""
    torch = _torch()
    abi = importlib.import_module(rtc.__name__ + ".abi")
    w, cam = A.world(rtc, name)
    want = A.expected(rtc, O, name, ASYNC)
    assert np.isinf(want["depth"]).any() == (name == "s21")
    width, height = cam.hsize, cam.vsize
    npx = width * height
    dev = {p: torch.zeros(npx * comps * np.dtype(d).itemsize, dtype=torch.uint8, device="cuda:0") for p, (d, comps) in abi.AOV_PLANES.items()}
    pic = torch.zeros(npx * 3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    finite = want["depth"][np.isfinite(want["depth"])]
    near, far = float(finite.min()), float(finite.max())
    dw = gpu.upload(w)
    enc = rtc.ImageEncoder(gpu)
    try:
        dw.render_aov_device(cam, {p: t.data_ptr() for p, t in dev.items()})
        gpu.synchronize()
        planes = {p: dev[p].cpu().numpy().view(abi.AOV_PLANES[p][0]).reshape(want[p].shape) for p in A.PLANES}
        _assert_same(planes, want, name + " device planes")
        for view in ("depth", "normal", "index", "shadow"):
            host_pic = rtc.aov_view(view, planes, near=near, far=far, n_lights=1)
            pic.fill_(SENTINEL)
            torch.cuda.synchronize()
            gpu.aov_view_device(view, {view: dev[view].data_ptr()}, width, height, pic.data_ptr(), near=near, far=far, n_lights=1)
            gpu.synchronize()
            assert np.array_equal(pic.cpu().numpy().reshape(height, width, 3), host_pic), view
            assert len(np.unique(host_pic.reshape(-1, 3), axis=0)) > 1, view
            png = enc.encode_device("png", pic.data_ptr(), width, height, 3)
            assert png == rtc.image_encode("png", host_pic), view
    finally:
        enc.close()
        dw.close()


def test_errors(rtc, gpu, O):
    """8. All-NULL is RTC_ERR_ARG (4), RTC_FLAG_LDS_TABLE is RTC_ERR_UNSUPPORTED (8), a World of another context is 4."""
    abi = importlib.import_module(rtc.__name__ + ".abi")
    torch = _torch()
    w, cam = A.world(rtc, "s21")
    L = rtc.lib()
    idx = torch.zeros(cam.hsize * cam.vsize, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    one = abi.RtcAovBuffers(index=idx.data_ptr())
    none = abi.RtcAovBuffers()
    host_idx = np.zeros((cam.vsize, cam.hsize), dtype=np.int32)
    host_one = abi.RtcAovBuffers(index=host_idx.ctypes.data)
    dw = gpu.upload(w)
    other = rtc.Context(0)
    try:
        for entry, ok in ((L.rtc_render_aov_device, one), (L.rtc_render_aov, host_one)):
            assert entry(gpu._h, dw._h, C.byref(cam), ASYNC, 0, C.byref(none)) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), ASYNC, 0, None) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), ASYNC, LDS_TABLE, C.byref(ok)) == 8
            assert entry(gpu._h, dw._h, C.byref(cam), ASYNC, NO_CULL | LDS_TABLE, C.byref(ok)) == 8
            assert entry(other._h, dw._h, C.byref(cam), ASYNC, 0, C.byref(ok)) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), 2, 0, C.byref(ok)) == 4
            assert entry(gpu._h, dw._h, C.byref(cam), ASYNC, 0, C.byref(ok)) == 0
        gpu.synchronize()
        misaligned = abi.RtcAovBuffers(index=idx.data_ptr() + 2)
        assert L.rtc_render_aov_device(gpu._h, dw._h, C.byref(cam), ASYNC, 0, C.byref(misaligned)) == 4
        assert np.array_equal(host_idx, A.expected(rtc, O, "s21", ASYNC)["index"])
        # AOV launches do not touch rtc_stats
        gpu.reset_stats()
        dw.render_aov(cam)
        assert all(v == 0 for v in gpu.stats().values())
        # the device view entry refuses what the host entry refuses
        pic = torch.zeros(cam.hsize * cam.vsize * 3, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        assert L.rtc_aov_view_rgb8_device(gpu._h, 0, C.byref(one), cam.hsize, cam.vsize, 0.0, 1.0, 1, pic.data_ptr()) == 4   # no depth plane
        assert L.rtc_aov_view_rgb8_device(gpu._h, 2, C.byref(one), cam.hsize, cam.vsize, 0.0, 1.0, 1, None) == 4
        assert L.rtc_aov_view_rgb8_device(gpu._h, 2, C.byref(one), cam.hsize, cam.vsize, 0.0, 1.0, 1, pic.data_ptr()) == 0
        gpu.synchronize()
    finally:
        other.close()
        dw.close()
