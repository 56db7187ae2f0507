"""raytracer-challenge_amd — MI355X-native renderer for the hot path of joedane/raytracer-challenge.

This package is a thin ctypes binding of ``librtc.so`` (``include/rtc.h``): HIP kernels for
``Camera::render -> World::color_at -> World::intersect -> shade_hit`` behind a C-ABI, plus the
host-side setup arithmetic (Matrix / Camera / Shape constructors, the jamis.yml loader, the PPM
writer). The directory name carries a hyphen; import it through ``_bootstrap.py`` at the repo
root, which registers it as ``raytracer_challenge_amd``.

There is no CPU fallback: if ``librtc.so`` is missing, or no gfx950 device is usable, the
calls raise.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from pathlib import Path

import numpy as np

from .abi import (LUA_FRAME_FN, LUA_GIF_FN, LUA_FILE_FN, LUA_OUT_RGB8, LUA_OUT_GIF_RECORD, LUA_OUT_JPEG, LUA_OUT_PNG, LUA_OUT_FILE, IMAGE_FORMATS, IMAGE_JPEG_QUALITY, TIFF_STRIP_BYTES, PNG_SEGMENT, PNG_CHAIN, GIF_SEGMENT, GIF_DELAY_CS, RtcLuaJob, RtcCamera, RtcHit, RtcLaunchInfo, RtcLight, RtcAreaLight, RtcLens, RtcAo, MAX_AO_SAMPLES, RtcGatherBuffers, RtcAdaptive, RtcAdaptiveInfo, MAX_AA_SAMPLES, AA_DEFAULT_THRESHOLD, AA_DEFAULT_STEPS, AA_DEFAULT_MAX_RAYS, RtcLuminance, RtcTonemap, RtcBloom, TONEMAP_LINEAR, TONEMAP_REINHARD, TONEMAP_ACES, TONEMAP_CURVES, TONEMAP_AUTO_EXPOSURE, TONEMAP_AUTO_WHITE, MAX_BLOOM_RADIUS, RtcResize, RESIZE_BOX, RESIZE_TRIANGLE, RESIZE_CATMULL_ROM, RESIZE_MITCHELL, RESIZE_LANCZOS3, RESIZE_FILTERS, MAX_RESIZE_TAPS, RtcFilter, FILTER_SAME_OBJECT, MAX_FILTER_PASSES, FILTER_DEFAULT_PLANE_SIGMA, FILTER_DEFAULT_PASSES, FILTER_DEFAULT_NORMAL_SQUARINGS, RtcProjection, PROJ_ORTHOGRAPHIC, PROJ_PANORAMA, RtcMotion, RtcShutterScene, RtcMaterial, RtcShape, RtcStats, Mat16, Vec3, SOURCE_NAMES,
                  SPHERE, PLANE, CUBE, MODE_RENDER, MODE_RENDER_ASYNC, FLAG_NONE, FLAG_NO_CULL, FLAG_AA_RESAMPLE, FLAG_LDS_TABLE,
                  EXCHANGE_RCCL, EXCHANGE_P2P, GATHER_NONE, GATHER_F64, GATHER_U8, GROUP_ID_BYTES, MAX_LIGHTS, MAX_LIGHT_SAMPLES, MAX_LENS_SAMPLES, MAX_SHUTTER_SAMPLES, SHUTTER_RING, PATTERNS, STATUS_NAMES, declare,
                  RtcAovBuffers, AOV_PLANES, AOV_VIEWS, AOV_VIEW_DEPTH, AOV_VIEW_NORMAL, AOV_VIEW_INDEX, AOV_VIEW_SHADOW,
                  RtcFloatPlanes, FLOAT_FORMATS, FLOAT_HDR, FLOAT_PFM, FLOAT_EXR, EXR_TYPES, EXR_HALF, EXR_FLOAT)

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / "librtc.so"

_lib = None


class RtcError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        name = STATUS_NAMES.get(status, str(status))
        super().__init__(f"{where}: {name}" + (f" ({detail})" if detail else ""))


def lib() -> C.CDLL:
    """Load librtc.so (built by ``build.build()`` / ``__graft_entry__.build()``). Fails loudly."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} is missing: run `python __graft_entry__.py build` (hipcc, gfx950). "
                               "There is no CPU fallback for the render path.")
        # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.so.7 (same soname
        # as /opt/rocm's). Import torch first so that librtc.so binds to the runtime torch uses —
        # otherwise two HSA runtimes race for the device and the second one sees "no GPUs".
        try:
            import torch  # noqa: F401
        except Exception:  # torch is plumbing (device tensors, streams, RCCL), not a hard dependency
            pass
        _lib = C.CDLL(str(LIB_PATH))
        declare(_lib)
    return _lib


_fn_cache: dict = {}


def _render_rows():
    f = _fn_cache.get("rows")
    if f is None:
        f = _fn_cache["rows"] = lib().rtc_render_rows
    return f


def _render_bands():
    f = _fn_cache.get("bands")
    if f is None:
        f = _fn_cache["bands"] = lib().rtc_render_bands
    return f


def _check(status: int, where: str, detail: str = "") -> None:
    if status != 0:
        raise RtcError(status, where, detail)


# ---------------------------------------------------------------------------------------
# host-side mirror of the reference's setup API (names follow ch1/src/*.rs)
# ---------------------------------------------------------------------------------------
class Matrix:
    """Matrix (transform.rs:23-27) with the fluent, LEFT-multiplying builders (transform.rs:53-105)."""

    __slots__ = ("m",)

    def __init__(self, m=None):
        self.m = Mat16()
        if m is None:
            lib().rtc_matrix_identity(self.m)
        else:
            flat = np.asarray(m, dtype=np.float64).reshape(16)
            for i in range(16):
                self.m[i] = flat[i]

    @staticmethod
    def identity() -> "Matrix":
        return Matrix()

    def _apply(self, fn, *args) -> "Matrix":
        out = Matrix.__new__(Matrix)
        out.m = Mat16()
        fn(self.m, *[C.c_double(a) for a in args], out.m)
        return out

    def translation(self, x, y, z): return self._apply(lib().rtc_matrix_translation, x, y, z)
    def scaling(self, x, y, z): return self._apply(lib().rtc_matrix_scaling, x, y, z)
    def rotation_x(self, r): return self._apply(lib().rtc_matrix_rotation_x, r)
    def rotation_y(self, r): return self._apply(lib().rtc_matrix_rotation_y, r)
    def rotation_z(self, r): return self._apply(lib().rtc_matrix_rotation_z, r)
    def shearing(self, xy, xz, yx, yz, zx, zy): return self._apply(lib().rtc_matrix_shearing, xy, xz, yx, yz, zx, zy)

    def multiply(self, other: "Matrix") -> "Matrix":
        out = Matrix.__new__(Matrix)
        out.m = Mat16()
        lib().rtc_matrix_multiply(self.m, other.m, out.m)
        return out

    def inverse(self) -> "Matrix":
        out = Matrix.__new__(Matrix)
        out.m = Mat16()
        _check(lib().rtc_matrix_inverse(self.m, out.m), "Matrix.inverse")
        return out

    def transpose(self) -> "Matrix":
        out = Matrix.__new__(Matrix)
        out.m = Mat16()
        lib().rtc_matrix_transpose(self.m, out.m)
        return out

    def determinant(self) -> float:
        return float(lib().rtc_matrix_determinant(self.m))

    @staticmethod
    def make_view_transform(frm, to, up) -> "Matrix":
        out = Matrix.__new__(Matrix)
        out.m = Mat16()
        lib().rtc_view_transform(Vec3(*frm), Vec3(*to), Vec3(*up), out.m)
        return out

    def numpy(self) -> np.ndarray:
        return np.array(list(self.m), dtype=np.float64).reshape(4, 4)


def material(color=(1.0, 1.0, 1.0), ambient=0.1, diffuse=0.9, specular=0.9, shininess=200.0, reflective=0.0,
             transparency=0.0, refractive_index=1.0, pattern=None) -> RtcMaterial:
    """Material (material.rs:244-254) starting from Material::default() (white). `pattern` is
    (kind_name, color_a, color_b, Matrix|None) or None; `color=None` means Material.color = None."""
    m = RtcMaterial()
    lib().rtc_material_default(C.byref(m))
    if color is None:
        m.has_color = 0
    else:
        m.has_color = 1
        for i in range(3):
            m.color[i] = float(color[i])
    m.ambient, m.diffuse, m.specular, m.shininess = float(ambient), float(diffuse), float(specular), float(shininess)
    m.reflective, m.transparency, m.refractive_index = float(reflective), float(transparency), float(refractive_index)
    if pattern is not None:
        kind, a, b, xf = pattern
        xf = xf if xf is not None else Matrix.identity()
        _check(lib().rtc_material_set_pattern(C.byref(m), PATTERNS[kind], Vec3(*a), Vec3(*b), xf.m), "Pattern.set_transform")
    return m


def _shape(kind: int, transform: Matrix | None, mat: RtcMaterial | None) -> RtcShape:
    s = RtcShape()
    t = transform if transform is not None else Matrix.identity()
    _check(lib().rtc_shape_init(kind, t.m, C.byref(mat) if mat is not None else None, C.byref(s)), "Shape.new_with_transform_and_material")
    return s


def sphere(transform=None, mat=None) -> RtcShape: return _shape(SPHERE, transform, mat)   # shape.rs:308
def plane(transform=None, mat=None) -> RtcShape: return _shape(PLANE, transform, mat)     # shape.rs:436
def cube(transform=None, mat=None) -> RtcShape: return _shape(CUBE, transform, mat)       # shape.rs:525


def light(position=(-10.0, 10.0, -10.0), intensity=(1.0, 1.0, 1.0)) -> RtcLight:
    l = RtcLight()
    for i in range(3):
        l.position[i] = float(position[i])
        l.intensity[i] = float(intensity[i])
    return l


def area_light(corner, uvec, vvec, usteps: int, vsteps: int, intensity=(1.0, 1.0, 1.0)) -> RtcAreaLight:
    """The book's area light: the rectangle corner + s*uvec + t*vvec sampled at the centres of usteps x vsteps cells
    (rtc_area_light, include/rtc.h; no jitter)."""
    a = RtcAreaLight()
    for i in range(3):
        a.corner[i], a.uvec[i], a.vvec[i], a.intensity[i] = float(corner[i]), float(uvec[i]), float(vvec[i]), float(intensity[i])
    a.usteps, a.vsteps = int(usteps), int(vsteps)
    return a


def _copy_light(l):
    """A loader's light as the binding's: the degenerate 1x1 area light of a point light becomes an RtcLight."""
    if l.usteps == 1 and l.vsteps == 1 and not any(l.uvec) and not any(l.vvec):
        return light(position=tuple(l.corner), intensity=tuple(l.intensity))
    a = RtcAreaLight()
    C.memmove(C.byref(a), C.byref(l), C.sizeof(RtcAreaLight))
    return a


class World:
    """World (shape.rs:633-637): host-side list of shapes + lights (one light or a list of them, RtcLight point lights and
    RtcAreaLight area lights in any mix, 1..MAX_LIGHT_SAMPLES samples in all); `add_shape` assigns world ids like the
    reference (shape.rs:661-667). `light` is `lights[0]`, the one the reference shades with; a DeviceWorld shades with
    all of them (rtc_world_create_lights / rtc_world_create_area_lights)."""

    def __init__(self, lgt=None):
        if lgt is None:
            self.lights: list[RtcLight] = [light()]
        elif isinstance(lgt, (RtcLight, RtcAreaLight)):
            self.lights = [lgt]
        else:
            self.lights = list(lgt)
        self.shapes: list[RtcShape] = []

    @property
    def light(self) -> RtcLight:
        return self.lights[0]

    @light.setter
    def light(self, lgt: RtcLight) -> None:
        self.lights[0] = lgt

    def add_light(self, lgt: RtcLight) -> "World":
        self.lights.append(lgt)
        return self

    def light_array(self):
        arr = (RtcLight * max(1, len(self.lights)))()
        for i, l in enumerate(self.lights):
            arr[i] = l
        return arr

    def needs_area_entries(self) -> bool:
        """An area light, or more point lights than rtc_world_create_lights takes."""
        return len(self.lights) > MAX_LIGHTS or any(isinstance(l, RtcAreaLight) for l in self.lights)

    def area_light_array(self):
        """Every light as an rtc_area_light (point lights: the degenerate 1x1 case)."""
        arr = (RtcAreaLight * max(1, len(self.lights)))()
        for i, l in enumerate(self.lights):
            if isinstance(l, RtcAreaLight):
                arr[i] = l
            else:
                _check(lib().rtc_area_light_from_point(C.byref(l), C.byref(arr[i])), "rtc_area_light_from_point")
        return arr

    def samples(self) -> list:
        """The World's sample list: the point lights a DeviceWorld shades with (rtc_area_light_expand)."""
        out, n = (RtcLight * MAX_LIGHT_SAMPLES)(), C.c_uint32(0)
        _check(lib().rtc_area_light_expand(self.area_light_array(), len(self.lights), out, MAX_LIGHT_SAMPLES, C.byref(n)), "rtc_area_light_expand")
        return _copy_lights(out, n.value)

    def add_shape(self, s: RtcShape) -> "World":
        s.world_id = len(self.shapes) + 1
        self.shapes.append(s)
        return self

    @staticmethod
    def default() -> "World":
        """impl Default for World (shape.rs:784-795)."""
        w = World()
        w.add_shape(sphere(Matrix.identity(), material(color=(0.8, 1.0, 0.6), diffuse=0.7, specular=0.2)))
        w.add_shape(sphere(Matrix.identity().scaling(0.5, 0.5, 0.5)))
        return w

    def array(self):
        arr = (RtcShape * max(1, len(self.shapes)))()
        for i, s in enumerate(self.shapes):
            arr[i] = s
        return arr

    def __len__(self):
        return len(self.shapes)


def camera(hsize: int, vsize: int, fov: float, view: Matrix | None = None, samples: int = 1) -> RtcCamera:
    """Camera::new_with_transform (camera.rs:33-58)."""
    cam = RtcCamera()
    v = view if view is not None else Matrix.identity()
    _check(lib().rtc_camera_init(hsize, vsize, float(fov), v.m, C.byref(cam)), "Camera.new_with_transform")
    cam.samples = samples
    return cam


def ray_for_pixel(cam: RtcCamera, x: int, y: int, xo: float = 0.5, yo: float = 0.5) -> np.ndarray:
    out = (C.c_double * 6)()
    lib().rtc_camera_ray_for_pixel(C.byref(cam), x, C.c_double(xo), y, C.c_double(yo), out)
    return np.array(list(out))


def lens(aperture: float, focal_distance: float, usteps: int = 1, vsteps: int = 1) -> RtcLens:
    """A thin lens for DeviceWorld.render_lens: a square of half-width `aperture` in the camera's z = 0 plane, sampled at
    the centres of usteps x vsteps cells, in focus `focal_distance` in front of the camera (rtc_lens, include/rtc.h; no
    jitter, no disc). lens(0, 1) is the pinhole."""
    l = RtcLens()
    l.aperture, l.focal_distance, l.usteps, l.vsteps = float(aperture), float(focal_distance), int(usteps), int(vsteps)
    _check(lib().rtc_lens_validate(C.byref(l)), "rtc_lens_validate")
    return l


def lens_ray(cam: RtcCamera, lens: RtcLens, x: int, y: int, k: int) -> np.ndarray:
    """The ray of pixel (x, y) through lens sample k = v*usteps + u: origin xyz, direction xyz (rtc_lens_ray)."""
    out = (C.c_double * 6)()
    _check(lib().rtc_lens_ray(C.byref(cam), C.byref(lens), x, y, k, out), "rtc_lens_ray")
    return np.array(list(out))


def ao(radius: float, usteps: int = 4, vsteps: int = 4) -> RtcAo:
    """An ambient-occlusion pass for DeviceWorld.render_ao (rtc_ao, include/rtc.h): usteps x vsteps cosine-weighted rays per
    pixel into the hemisphere over the centre ray's hit, each asking for something nearer than `radius` (math.inf:
    unbounded). No jitter: the samples sit at the cell centres."""
    a = RtcAo()
    a.radius, a.usteps, a.vsteps = float(radius), int(usteps), int(vsteps)
    _check(lib().rtc_ao_validate(C.byref(a)), "rtc_ao_validate")
    return a


def ao_expand(ao: RtcAo) -> np.ndarray:
    """The pass's sample directions about the normal (0, 0, 1), an (n, 3) array in the order k = v*usteps + u (rtc_ao_expand)."""
    dirs, n = np.empty((MAX_AO_SAMPLES, 3)), C.c_uint32(0)
    _check(lib().rtc_ao_expand(C.byref(ao), dirs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)), "rtc_ao_expand")
    return dirs[:n.value].copy()


def ao_ray(normal, over_point, local) -> np.ndarray:
    """The ray of the sample direction `local` from `over_point` about `normal`: origin xyz, direction xyz (rtc_ao_ray)."""
    out = (C.c_double * 6)()
    _check(lib().rtc_ao_ray(Vec3(*[float(v) for v in normal]), Vec3(*[float(v) for v in over_point]), Vec3(*[float(v) for v in local]), out), "rtc_ao_ray")
    return np.array(list(out))


def ao_from_hits(hits, counts, width: int, height: int, mode: int = MODE_RENDER_ASYNC) -> np.ndarray:
    """rtc_ao_from_hits: width * height hit records (an RtcHit array, row-major) and their occluded-sample counts packed into
    the (height, width) uint16 plane, the mode rule included."""
    c = np.ascontiguousarray(counts, dtype=np.uint16).reshape(-1)
    if len(hits) != width * height or c.size != width * height:
        raise ValueError("ao_from_hits needs width * height hit records and counts")
    out = np.empty((height, width), dtype=np.uint16)
    _check(lib().rtc_ao_from_hits(hits, c.ctypes.data_as(C.POINTER(C.c_uint16)), width, height, mode, out.ctypes.data_as(C.POINTER(C.c_uint16))),
           "rtc_ao_from_hits")
    return out


def apply_ao(rgb: np.ndarray, ao_plane: np.ndarray, n_samples: int, strength: float = 1.0) -> np.ndarray:
    """rtc_canvas_apply_ao: a copy of the (H, W, 3) f64 canvas with every component multiplied by
    1 - strength * count / n_samples of its pixel."""
    out = np.array(rgb, dtype=np.float64, order="C", copy=True)
    a = np.ascontiguousarray(ao_plane, dtype=np.uint16)
    if out.ndim != 3 or out.shape[2] != 3 or a.shape != out.shape[:2]:
        raise ValueError("apply_ao needs an (H, W, 3) canvas and an (H, W) plane")
    _check(lib().rtc_canvas_apply_ao(out.ctypes.data_as(C.POINTER(C.c_double)), a.ctypes.data_as(C.POINTER(C.c_uint16)), int(n_samples), float(strength),
                                     out.shape[1], out.shape[0]), "rtc_canvas_apply_ao")
    return out


def gather_from_hits(hits, sample_hits, sample_rgb, albedo, n_samples: int, radius: float, width: int, height: int,
                     mode: int = MODE_RENDER_ASYNC, planes=("radiance", "bounce")) -> dict:
    """rtc_gather_from_hits: width * height centre-ray records (an RtcHit array, row-major), per pixel n_samples sample records
    (an RtcHit array of width * height * n_samples) and their colours (..., 3), and the per-pixel base * diffuse (..., 3; may
    be None when "bounce" is not asked for) packed into the planes asked for: {"radiance": (H, W, 3), "bounce": (H, W, 3)},
    the radius rule, the mean, the NaN rule and the mode rule included."""
    npx = width * height
    rgb = np.ascontiguousarray(sample_rgb, dtype=np.float64).reshape(-1)
    if len(hits) != npx or len(sample_hits) != npx * n_samples or rgb.size != npx * n_samples * 3:
        raise ValueError("gather_from_hits needs width * height records and n_samples records and colours for each")
    alb = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float64).reshape(-1)
    if alb is not None and alb.size != npx * 3:
        raise ValueError("gather_from_hits needs width * height * 3 albedo values")
    out = {name: np.empty((height, width, 3)) for name in planes}
    b = RtcGatherBuffers(**{name: a.ctypes.data for name, a in out.items()})
    _check(lib().rtc_gather_from_hits(hits, sample_hits, rgb.ctypes.data_as(C.POINTER(C.c_double)),
                                      None if alb is None else alb.ctypes.data_as(C.POINTER(C.c_double)), int(n_samples), float(radius),
                                      width, height, mode, C.byref(b)), "rtc_gather_from_hits")
    return out


def add_scaled(rgb: np.ndarray, plane: np.ndarray, strength: float = 1.0) -> np.ndarray:
    """rtc_canvas_add_scaled: a copy of the (H, W, 3) f64 canvas with strength * plane added, component by component."""
    out = np.array(rgb, dtype=np.float64, order="C", copy=True)
    pl = np.ascontiguousarray(plane, dtype=np.float64)
    if out.ndim != 3 or out.shape[2] != 3 or pl.shape != out.shape:
        raise ValueError("add_scaled needs an (H, W, 3) canvas and a plane of its shape")
    _check(lib().rtc_canvas_add_scaled(out.ctypes.data_as(C.POINTER(C.c_double)), pl.ctypes.data_as(C.POINTER(C.c_double)), float(strength),
                                       out.shape[1], out.shape[0]), "rtc_canvas_add_scaled")
    return out


def filter_spec(plane_sigma: float = FILTER_DEFAULT_PLANE_SIGMA, passes: int = FILTER_DEFAULT_PASSES,
                normal_squarings: int = FILTER_DEFAULT_NORMAL_SQUARINGS, same_object: bool = True) -> RtcFilter:
    """An edge-aware filter for plane_filter (rtc_filter, include/rtc.h): `passes` à-trous passes with taps 1, 2, 4, ... pixels
    apart; a tap counts less the farther it lies off the pixel's tangent plane (`plane_sigma`, world units; math.inf: no plane
    test) and the more its normal turns away ((n_p . n_q) squared `normal_squarings` times), and with `same_object` not at all
    when it belongs to another object."""
    f = RtcFilter()
    f.plane_sigma, f.passes, f.normal_squarings, f.flags = float(plane_sigma), int(passes), int(normal_squarings), FILTER_SAME_OBJECT if same_object else 0
    _check(lib().rtc_filter_validate(C.byref(f)), "rtc_filter_validate")
    return f


def _filter_guides(planes: dict, height: int, width: int) -> dict:
    """The index, point and normal planes of `planes` (a dict as DeviceWorld.render_aov returns it) as the filter reads them."""
    out = {}
    for name in ("index", "point", "normal"):
        dtype, comps = AOV_PLANES[name]
        a = np.ascontiguousarray(planes[name], dtype=dtype)  # KeyError: the filter needs all three
        if a.shape != ((height, width) if comps == 1 else (height, width, comps)):
            raise ValueError(f"guide plane {name!r} does not have the values' size")
        out[name] = a
    return out


def plane_filter(values: np.ndarray, planes: dict, flt: RtcFilter) -> np.ndarray:
    """rtc_plane_filter: the (H, W) or (H, W, 3) f64 plane `values` (an occlusion fraction, a radiance or bounce plane) filtered
    under the guides `planes` = {"index", "point", "normal"}; a new array of the same shape."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.ndim not in (2, 3) or (v.ndim == 3 and v.shape[2] != 3):
        raise ValueError("plane_filter needs an (H, W) or (H, W, 3) plane")
    g = _filter_guides(planes, v.shape[0], v.shape[1])
    out = np.empty_like(v)
    b = _aov_host_buffers(g)
    _check(lib().rtc_plane_filter(v.ctypes.data_as(C.POINTER(C.c_double)), 1 if v.ndim == 2 else 3, C.byref(b), v.shape[1], v.shape[0], C.byref(flt),
                                  out.ctypes.data_as(C.POINTER(C.c_double))), "rtc_plane_filter")
    return out


def counts_to_fraction(counts: np.ndarray, n: int) -> np.ndarray:
    """rtc_counts_to_fraction: an (H, W) uint16 count plane (DeviceWorld.render_ao's, or an AOV `shadow` plane) as the f64
    fraction count / n that plane_filter and apply_occlusion take."""
    c = np.ascontiguousarray(counts, dtype=np.uint16)
    if c.ndim != 2:
        raise ValueError("counts_to_fraction needs an (H, W) plane")
    out = np.empty(c.shape, dtype=np.float64)
    _check(lib().rtc_counts_to_fraction(c.ctypes.data_as(C.POINTER(C.c_uint16)), int(n), c.shape[1], c.shape[0], out.ctypes.data_as(C.POINTER(C.c_double))),
           "rtc_counts_to_fraction")
    return out


def apply_occlusion(rgb: np.ndarray, occ: np.ndarray, strength: float = 1.0) -> np.ndarray:
    """rtc_canvas_apply_occlusion: a copy of the (H, W, 3) f64 canvas with every component multiplied by
    1 - strength * occ of its pixel; apply_ao's bytes when occ is counts_to_fraction of its plane."""
    out = np.array(rgb, dtype=np.float64, order="C", copy=True)
    o = np.ascontiguousarray(occ, dtype=np.float64)
    if out.ndim != 3 or out.shape[2] != 3 or o.shape != out.shape[:2]:
        raise ValueError("apply_occlusion needs an (H, W, 3) canvas and an (H, W) plane")
    _check(lib().rtc_canvas_apply_occlusion(out.ctypes.data_as(C.POINTER(C.c_double)), o.ctypes.data_as(C.POINTER(C.c_double)), float(strength),
                                            out.shape[1], out.shape[0]), "rtc_canvas_apply_occlusion")
    return out


def adaptive(threshold: float = AA_DEFAULT_THRESHOLD, usteps: int = AA_DEFAULT_STEPS, vsteps: int = AA_DEFAULT_STEPS, max_rays: int = 0) -> RtcAdaptive:
    """A spec for DeviceWorld.render_adaptive (rtc_adaptive, include/rtc.h): pixels whose colour is farther than `threshold`
    (Color::distance_from) from a 4-neighbour's are re-rendered as the mean of usteps x vsteps sub-samples; `max_rays` bounds the
    rays of one refinement launch (0: the library's default)."""
    a = RtcAdaptive()
    a.threshold, a.usteps, a.vsteps, a.max_rays = float(threshold), int(usteps), int(vsteps), int(max_rays)
    _check(lib().rtc_adaptive_validate(C.byref(a)), "rtc_adaptive_validate")
    return a


def adaptive_offset(spec: RtcAdaptive, k: int) -> tuple:
    """rtc_adaptive_offset: (x_offset, y_offset) of sample k of the spec's grid."""
    xo, yo = C.c_double(0.0), C.c_double(0.0)
    _check(lib().rtc_adaptive_offset(C.byref(spec), int(k), C.byref(xo), C.byref(yo)), "rtc_adaptive_offset")
    return xo.value, yo.value


def adaptive_mask(rgb: np.ndarray, mode: int, threshold: float) -> np.ndarray:
    """rtc_adaptive_mask: the (H, W) uint8 mask of the (H, W, 3) f64 canvas — 1 where a pixel of the rendered area differs from
    a 4-neighbour in it by more than `threshold`."""
    c = np.ascontiguousarray(rgb, dtype=np.float64)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("adaptive_mask needs an (H, W, 3) canvas")
    mask = np.empty(c.shape[:2], dtype=np.uint8)
    _check(lib().rtc_adaptive_mask(c.ctypes.data_as(C.POINTER(C.c_double)), c.shape[1], c.shape[0], int(mode), float(threshold),
                                   mask.ctypes.data_as(C.POINTER(C.c_uint8)), None), "rtc_adaptive_mask")
    return mask


def _canvas_arg(rgb: np.ndarray, what: str) -> np.ndarray:
    c = np.ascontiguousarray(rgb, dtype=np.float64)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError(what + " needs an (H, W, 3) canvas")
    return c


def tonemap_spec(curve="reinhard", exposure: float = 1.0, white: float = math.inf, key: float | None = None, auto_white: bool = False) -> RtcTonemap:
    """A record for rtc.tonemap / Context.tonemap_device (rtc_tonemap, include/rtc.h). `curve`: "linear", "reinhard", "aces" or
    a TONEMAP_* value. `exposure` multiplies every channel; `key`, when given, replaces it: the frame's mean luminance is mapped
    to that value (TONEMAP_AUTO_EXPOSURE, needs the statistics). `white` is the luminance REINHARD maps to 1 (inf: the plain
    curve); `auto_white` takes the frame's largest luminance (TONEMAP_AUTO_WHITE, needs the statistics)."""
    t = RtcTonemap()
    t.curve = TONEMAP_CURVES[curve] if isinstance(curve, str) else int(curve)
    t.exposure = float(exposure if key is None else key)
    t.white = float(white)
    t.flags = (TONEMAP_AUTO_EXPOSURE if key is not None else 0) | (TONEMAP_AUTO_WHITE if auto_white else 0)
    _check(lib().rtc_tonemap_validate(C.byref(t)), "rtc_tonemap_validate")
    return t


def bloom_spec(threshold: float = 1.0, strength: float = 0.5, sigma: float = 2.0, radius: int = 6) -> RtcBloom:
    """A record for rtc.bloom / Context.bloom_device (rtc_bloom, include/rtc.h): luminance above `threshold` is blurred by a
    separable Gaussian of `sigma` pixels cut at `radius` (1..MAX_BLOOM_RADIUS) and added `strength` times."""
    b = RtcBloom()
    b.threshold, b.strength, b.sigma, b.radius = float(threshold), float(strength), float(sigma), int(radius)
    _check(lib().rtc_bloom_validate(C.byref(b)), "rtc_bloom_validate")
    return b


def luminance(rgb: np.ndarray) -> RtcLuminance:
    """rtc_canvas_luminance: the frame statistics {max, sum, count} of an (H, W, 3) f64 canvas, the sum in the header's tree order."""
    c = _canvas_arg(rgb, "luminance")
    out = RtcLuminance()
    _check(lib().rtc_canvas_luminance(c.ctypes.data_as(C.POINTER(C.c_double)), c.shape[1], c.shape[0], C.byref(out)), "rtc_canvas_luminance")
    return out


def tonemap_resolve(spec: RtcTonemap, stats: RtcLuminance | None = None) -> tuple:
    """rtc_tonemap_resolve: (m, inv_w2), the multiplier and white term `spec` gives a frame with the statistics `stats`."""
    m, iw = C.c_double(0.0), C.c_double(0.0)
    _check(lib().rtc_tonemap_resolve(C.byref(spec), C.byref(stats) if stats is not None else None, C.byref(m), C.byref(iw)), "rtc_tonemap_resolve")
    return m.value, iw.value


def tonemap(rgb: np.ndarray, spec: RtcTonemap, stats: RtcLuminance | None = None) -> np.ndarray:
    """rtc_canvas_tonemap: the tone-mapped copy of an (H, W, 3) f64 canvas. With an AUTO flag in `spec` the statistics are
    `stats`, or the canvas's own when none are given."""
    c = _canvas_arg(rgb, "tonemap")
    if stats is None and spec.flags:
        stats = luminance(c)
    out = np.empty_like(c)
    _check(lib().rtc_canvas_tonemap(c.ctypes.data_as(C.POINTER(C.c_double)), c.shape[1], c.shape[0], C.byref(spec),
                                    C.byref(stats) if stats is not None else None, out.ctypes.data_as(C.POINTER(C.c_double))), "rtc_canvas_tonemap")
    return out


def bloom_weights(spec: RtcBloom) -> np.ndarray:
    """rtc_bloom_weights: the 2*radius + 1 normalised Gaussian weights of `spec`."""
    w = np.empty(2 * spec.radius + 1, dtype=np.float64)
    _check(lib().rtc_bloom_weights(C.byref(spec), w.ctypes.data_as(C.POINTER(C.c_double))), "rtc_bloom_weights")
    return w


def bloom(rgb: np.ndarray, spec: RtcBloom) -> np.ndarray:
    """rtc_canvas_bloom: a copy of an (H, W, 3) f64 canvas with the blurred bright pass added."""
    c = _canvas_arg(rgb, "bloom")
    out = np.empty_like(c)
    _check(lib().rtc_canvas_bloom(c.ctypes.data_as(C.POINTER(C.c_double)), c.shape[1], c.shape[0], C.byref(spec),
                                  out.ctypes.data_as(C.POINTER(C.c_double))), "rtc_canvas_bloom")
    return out


def resize_spec(filter="lanczos3") -> RtcResize:
    """A record for rtc.resize / Context.resize_device (rtc_resize, include/rtc.h). `filter`: "box", "triangle", "catmull-rom",
    "mitchell", "lanczos3" or a RESIZE_* value."""
    r = RtcResize()
    r.filter = RESIZE_FILTERS[filter] if isinstance(filter, str) else int(filter)
    _check(lib().rtc_resize_validate(C.byref(r)), "rtc_resize_validate")
    return r


def resize_weights(n_in: int, n_out: int, spec: RtcResize) -> tuple:
    """rtc_resize_weights: (first, count, w), the normative table of the axis n_in -> n_out: two uint32 arrays of n_out and an
    (n_out, rtc_resize_taps) f64 array, each row zero-padded past its count."""
    taps = lib().rtc_resize_taps(n_in, n_out, spec.filter)
    if taps == 0:
        raise RtcError(4, "rtc_resize_taps")
    first, count = np.zeros(n_out, dtype=np.uint32), np.zeros(n_out, dtype=np.uint32)
    w = np.zeros((n_out, taps), dtype=np.float64)
    _check(lib().rtc_resize_weights(n_in, n_out, C.byref(spec), first.ctypes.data_as(C.POINTER(C.c_uint32)), count.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    w.ctypes.data_as(C.POINTER(C.c_double))), "rtc_resize_weights")
    return first, count, w


def resize(rgb: np.ndarray, width: int, height: int, spec: RtcResize | None = None) -> np.ndarray:
    """rtc_canvas_resize: an (H, W, 3) f64 canvas filtered to (height, width, 3): the horizontal pass first, an unchanged axis
    copied. `spec`: resize_spec(); LANCZOS3 when none is given."""
    c = _canvas_arg(rgb, "resize")
    out = np.empty((int(height), int(width), 3), dtype=np.float64)
    spec = resize_spec() if spec is None else spec
    _check(lib().rtc_canvas_resize(c.ctypes.data_as(C.POINTER(C.c_double)), c.shape[1], c.shape[0], C.byref(spec),
                                   out.ctypes.data_as(C.POINTER(C.c_double)), int(width), int(height)), "rtc_canvas_resize")
    return out


def _adaptive_info_dict(info: RtcAdaptiveInfo) -> dict:
    return {"pixels_refined": int(info.pixels_refined), "rays_refined": int(info.rays_refined), "launches": int(info.launches)}


def projection(kind, width: float = 0.0, h_span: float = 2.0 * math.pi, v_span: float = math.pi) -> RtcProjection:
    """A projection for DeviceWorld.render_projection (rtc_projection, include/rtc.h). kind "orthographic" (or
    PROJ_ORTHOGRAPHIC): parallel rays, `width` the world-space width of the view. kind "panorama" (PROJ_PANORAMA): the
    equirectangular frame of every direction around the camera, `h_span` radians of longitude across it (at most 2 pi) and
    `v_span` of latitude down it (at most pi); its centre looks where the pinhole camera looks."""
    k = {"orthographic": PROJ_ORTHOGRAPHIC, "panorama": PROJ_PANORAMA}.get(kind, kind)
    p = RtcProjection()
    p.kind, p.width, p.h_span, p.v_span = int(k), float(width), float(h_span), float(v_span)
    _check(lib().rtc_projection_validate(C.byref(p)), "rtc_projection_validate")
    return p


def projection_ray(cam: RtcCamera, proj: RtcProjection, x: int, y: int) -> np.ndarray:
    """The ray of pixel (x, y) under `proj`: origin xyz, direction xyz (rtc_projection_ray)."""
    out = (C.c_double * 6)()
    _check(lib().rtc_projection_ray(C.byref(cam), C.byref(proj), x, y, out), "rtc_projection_ray")
    return np.array(list(out))


def projection_tables(cam: RtcCamera, proj: RtcProjection):
    """A panorama's (col, row) tables, (hsize, 2) and (vsize, 2) arrays of {sin, cos} (rtc_projection_tables)."""
    col, row = np.empty((cam.hsize, 2)), np.empty((cam.vsize, 2))
    _check(lib().rtc_projection_tables(C.byref(cam), C.byref(proj), col.ctypes.data_as(C.POINTER(C.c_double)), row.ctypes.data_as(C.POINTER(C.c_double))),
           "rtc_projection_tables")
    return col, row


def motion(shape_index: int, open_transform: Matrix, close_transform: Matrix) -> RtcMotion:
    """One moving shape of a motion-blurred frame (rtc_motion, include/rtc.h): shape `shape_index` of the World has the
    OBJECT transform `open_transform` when the shutter opens and `close_transform` when it closes; in between the matrix is
    interpolated element by element (exact for translations and scalings; a rotation is sheared: keep the shutter short)."""
    m = RtcMotion()
    m.shape = int(shape_index)
    C.memmove(m.transform_open, open_transform.m, C.sizeof(Mat16))
    C.memmove(m.transform_close, close_transform.m, C.sizeof(Mat16))
    return m


def _motion_array(motions):
    motions = list(motions or [])
    arr = (RtcMotion * max(1, len(motions)))()
    for i, m in enumerate(motions):
        arr[i] = m
    return arr, len(motions)


def shutter_time(n: int, k: int) -> float:
    """t_k = (k + 0.5) / n, the centre of cell k of the shutter interval (rtc_shutter_time); NaN unless k < n <= 256."""
    return float(lib().rtc_shutter_time(n, k))


def shutter_shapes(world: "World", motions, samples: int, k: int) -> "World":
    """The World of sub-frame k of a motion-blurred frame (rtc_shutter_shapes): `world` with every moving shape's inverse
    recomputed from its interpolated transform; shapes without a motion record and the lights are copied as they are."""
    arr, n = world.array(), len(world.shapes)
    marr, nm = _motion_array(motions)
    out = (RtcShape * max(1, n))()
    _check(lib().rtc_shutter_shapes(arr, n, marr, nm, samples, k, out), "rtc_shutter_shapes")
    w = World(list(world.lights))
    for i in range(n):
        s = RtcShape()
        C.memmove(C.byref(s), C.byref(out[i]), C.sizeof(RtcShape))
        w.shapes.append(s)
    return w


def shutter_camera(cam: RtcCamera, cam_close, samples: int, k: int) -> RtcCamera:
    """The camera of sub-frame k (rtc_shutter_camera): `cam` with view_inv interpolated towards `cam_close` (None: static)."""
    out = RtcCamera()
    _check(lib().rtc_shutter_camera(C.byref(cam), C.byref(cam_close) if cam_close is not None else None, samples, k, C.byref(out)), "rtc_shutter_camera")
    return out


def canvas_average(frames) -> np.ndarray:
    """Color::average_over of whole frames on the host (rtc_canvas_average): `frames` = (n, ...) float64, n = 1..256; the
    result has the shape of one frame. Sums start at 0.0, add in frame order and are divided once by n."""
    a = np.ascontiguousarray(frames, dtype=np.float64)
    if a.ndim < 1:
        raise ValueError("frames must be an (n, ...) array")
    out = np.empty(a.shape[1:], dtype=np.float64)
    P = C.POINTER(C.c_double)
    _check(lib().rtc_canvas_average(a.ctypes.data_as(P), a.shape[0], out.size, out.ctypes.data_as(P)), "rtc_canvas_average")
    return out


def _copy_lights(arr, n: int) -> list:
    out = []
    for i in range(n):
        l = RtcLight()
        C.memmove(C.byref(l), C.byref(arr[i]), C.sizeof(RtcLight))
        out.append(l)
    return out


def _load_scene(entry: str, text: str | None, path: str | None, records=(), extra=(), where: str | None = None) -> tuple:
    """What the load_yaml* functions share: `entry` (its `_file` twin when `path` is given) called with the common buffers, then a
    (record, has) pair for each ctypes type of `records`, then `extra`, the entry point's further out-arguments, each by
    reference; failures raise under `where` (default: `entry`). -> (World with every `add: light` of the file and the shapes
    copied out of the library's array, RtcCamera, then for each of `records` the record, or None where the camera lacks its keys)."""
    shapes, n = C.POINTER(RtcShape)(), C.c_uint32(0)
    lgts, nl, cam = (RtcAreaLight * MAX_LIGHT_SAMPLES)(), C.c_uint32(0), RtcCamera()
    err = C.create_string_buffer(512)
    pairs = [(ctype(), C.c_uint32(0)) for ctype in records]
    fn = getattr(lib(), entry + "_file" if path is not None else entry)
    st = fn(str(path).encode() if path is not None else text.encode(), C.byref(shapes), C.byref(n), lgts, MAX_LIGHT_SAMPLES, C.byref(nl), C.byref(cam),
            err, 512, *[C.byref(x) for pair in pairs for x in pair], *map(C.byref, extra))
    _check(st, where or entry, err.value.decode(errors="replace"))
    w = World([_copy_light(lgts[i]) for i in range(nl.value)])
    for i in range(n.value):
        s = RtcShape()
        C.memmove(C.byref(s), C.byref(shapes[i]), C.sizeof(RtcShape))
        w.shapes.append(s)
    lib().rtc_free(shapes)
    return (w, cam, *[record if has.value else None for record, has in pairs])


def load_yaml(text: str | None = None, path: str | None = None):
    """jamis.yml-vocabulary loader -> (World, RtcCamera); the World holds every `add: light` of the file."""
    return _load_scene("rtc_scene_load_yaml_area_lights", text, path, where="rtc_scene_load_yaml")


def load_yaml_lens(text: str | None = None, path: str | None = None):
    """load_yaml for scenes whose camera may have a thin lens (aperture / focal-distance / lens-usteps / lens-vsteps):
    -> (World, RtcCamera, RtcLens or None)."""
    return _load_scene("rtc_scene_load_yaml_lens", text, path, [RtcLens])


def load_yaml_ao(text: str | None = None, path: str | None = None):
    """load_yaml_lens for scenes whose camera may ask for ambient occlusion (ao-radius / ao-usteps / ao-vsteps):
    -> (World, RtcCamera, RtcLens or None, RtcAo or None)."""
    return _load_scene("rtc_scene_load_yaml_ao", text, path, [RtcLens, RtcAo])


def load_yaml_gather(text: str | None = None, path: str | None = None):
    """load_yaml_ao for scenes whose camera may also ask for a gather pass (gather-radius / gather-usteps / gather-vsteps):
    -> (World, RtcCamera, RtcLens or None, RtcAo or None, RtcAo or None), the last the gather pass."""
    return _load_scene("rtc_scene_load_yaml_gather", text, path, [RtcLens, RtcAo, RtcAo])


def load_yaml_filter(text: str | None = None, path: str | None = None):
    """load_yaml_gather for scenes whose camera may also ask for the edge-aware filter (filter-plane-sigma / filter-passes /
    filter-normal-squarings): -> (World, RtcCamera, RtcLens or None, RtcAo or None, RtcAo or None, RtcFilter or None)."""
    return _load_scene("rtc_scene_load_yaml_filter", text, path, [RtcLens, RtcAo, RtcAo, RtcFilter])


def load_yaml_adaptive(text: str | None = None, path: str | None = None):
    """load_yaml for scenes whose camera may ask for adaptive anti-aliasing (aa-threshold / aa-usteps / aa-vsteps):
    -> (World, RtcCamera, RtcAdaptive or None)."""
    return _load_scene("rtc_scene_load_yaml_adaptive", text, path, [RtcAdaptive])


def load_yaml_post(text: str | None = None, path: str | None = None):
    """load_yaml for scenes whose camera may ask for post-processing (tonemap-curve / tonemap-exposure / tonemap-key /
    tonemap-white, bloom-threshold / bloom-strength / bloom-sigma / bloom-radius): -> (World, RtcCamera, RtcTonemap or None,
    RtcBloom or None)."""
    return _load_scene("rtc_scene_load_yaml_post", text, path, [RtcTonemap, RtcBloom])


def load_yaml_resize(text: str | None = None, path: str | None = None):
    """load_yaml_projection for scenes whose camera may ask for a delivered size (output-width / output-height / output-filter):
    -> (World, RtcCamera, RtcLens or None, RtcProjection or None, RtcResize or None, out_width, out_height); without the keys
    the size is the camera's own."""
    rs, ow, oh, has_rs = RtcResize(), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)  # (the sizes sit between the record and its flag)
    w, cam, ln, pj = _load_scene("rtc_scene_load_yaml_resize", text, path, [RtcLens, RtcProjection], extra=(rs, ow, oh, has_rs))
    return w, cam, ln, pj, (rs if has_rs.value else None), ow.value, oh.value


def load_yaml_projection(text: str | None = None, path: str | None = None):
    """load_yaml_lens for scenes whose camera may have a projection (projection: orthographic | panorama, ortho-width,
    pano-h-span, pano-v-span): -> (World, RtcCamera, RtcLens or None, RtcProjection or None)."""
    return _load_scene("rtc_scene_load_yaml_projection", text, path, [RtcLens, RtcProjection])


def load_yaml_projection_passes(text: str | None = None, path: str | None = None):
    """load_yaml_projection and load_yaml_filter in one: scenes whose camera has a projection and asks for passes under it (ao-*,
    gather-*, filter-* keys; data/orthographic_passes.yml): -> (World, RtcCamera, RtcLens or None, RtcProjection or None,
    RtcAo or None, RtcAo or None, RtcFilter or None) — what DeviceWorld.render_aov / render_ao / render_gather take as
    `projection` and `ao`, and plane_filter as `flt`."""
    return _load_scene("rtc_scene_load_yaml_projection_passes", text, path, [RtcLens, RtcProjection, RtcAo, RtcAo, RtcFilter])


def load_yaml_motion(text: str | None = None, path: str | None = None):
    """load_yaml_lens for scenes with motion blur (a shape's `motion:` transform list, the camera's `shutter-samples`):
    -> (World, RtcCamera, RtcLens or None, [RtcMotion], samples) — what Shutter.render takes."""
    mots, nm, samples = C.POINTER(RtcMotion)(), C.c_uint32(0), C.c_uint32(1)
    w, cam, ln = _load_scene("rtc_scene_load_yaml_motion", text, path, [RtcLens], extra=(mots, nm, samples))
    motions = []
    for i in range(nm.value):
        m = RtcMotion()
        C.memmove(C.byref(m), C.byref(mots[i]), C.sizeof(RtcMotion))
        motions.append(m)
    lib().rtc_free(mots)
    return w, cam, ln, motions, samples.value


class LuaJob:
    """One Render(world, camera, file) or encoder:AddFrame(world, camera) call of a script (rtc_lua_job), converted by
    lua.rs's *_from_table rules at the moment of the call."""

    def __init__(self, j: RtcLuaJob, index: int, lights=None):
        self.index = index
        self.kind = "AddFrame" if j.kind == 1 else "Render"
        self.outfile = (j.outfile or b"").decode(errors="replace")
        self.animation, self.frame, self.line = j.animation, j.frame, j.line
        self.same_world_as_previous = bool(j.same_world_as_previous)
        self.camera = RtcCamera()
        C.memmove(C.byref(self.camera), C.byref(j.camera), C.sizeof(RtcCamera))
        lgt = RtcLight()
        C.memmove(C.byref(lgt), C.byref(j.light), C.sizeof(RtcLight))
        self.lights = list(lights) if lights else [lgt]  # every light of the job's world; lights[0] is rtc_lua_job.light
        self.world = World(self.lights)
        for i in range(j.n_shapes):
            s = RtcShape()
            C.memmove(C.byref(s), C.byref(j.shapes[i]), C.sizeof(RtcShape))
            self.world.shapes.append(s)


class _Animations:
    """The GIF files of a run: each StartAnimation's records collected in order, written as header + records + 0x3B."""

    def __init__(self, where: str):
        self.where, self.anims = where, {}

    def add(self, job, name: str, record: bytes) -> None:
        a = self.anims.setdefault(job.animation, {"name": name, "size": (job.camera.hsize, job.camera.vsize), "records": []})
        if (job.camera.hsize, job.camera.vsize) != a["size"]:
            raise RtcError(4, self.where, f"frame {job.frame} of {name} is not {a['size'][0]}x{a['size'][1]}")
        a["records"].append(record)

    def write(self, out: Path, paths: list) -> None:
        for k in sorted(self.anims):
            a = self.anims[k]
            out.mkdir(parents=True, exist_ok=True)
            target = out / (a["name"] if a["name"].lower().endswith(".gif") else a["name"] + ".gif")
            target.write_bytes(gif_file_header(*a["size"]) + b"".join(a["records"]) + b"\x3b")
            paths.append(target)


class LuaProgram:
    """A scene script of the reference's Lua front-end, interpreted (rtc_lua_run: csrc/host_lua.cpp carries its own
    interpreter of the Lua 5.3 subset those scripts use): `jobs` = its Render / AddFrame calls in order, `output` = what it
    print()ed. render(ctx) is lua.rs's render_lua: every job rendered on the GPU, 8-bit frames back in job order."""

    def __init__(self, text: str | None = None, path=None, base_dir=None, step_limit: int = 0):
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        if path is not None:
            st = lib().rtc_lua_run_file(str(path).encode(), step_limit, C.byref(h), err, 1024)
        else:
            st = lib().rtc_lua_run(text.encode(), None if base_dir is None else str(base_dir).encode(), step_limit, C.byref(h), err, 1024)
        _check(st, "rtc_lua_run", err.value.decode(errors="replace"))
        self._h = h
        self.output = lib().rtc_lua_program_output(h).decode(errors="replace")

    def __len__(self):
        return lib().rtc_lua_program_jobs(self._h) if self._h else 0

    def job(self, index: int) -> LuaJob:
        j = RtcLuaJob()
        _check(lib().rtc_lua_program_job(self._h, index, C.byref(j)), "rtc_lua_program_job")
        lgts, nl = (RtcAreaLight * MAX_LIGHT_SAMPLES)(), C.c_uint32(0)
        _check(lib().rtc_lua_program_job_area_lights(self._h, index, lgts, MAX_LIGHT_SAMPLES, C.byref(nl)), "rtc_lua_program_job_area_lights")
        return LuaJob(j, index, [_copy_light(lgts[i]) for i in range(nl.value)])

    @property
    def jobs(self):
        return [self.job(i) for i in range(len(self))]

    def _run(self, ctx: "Context", entry: str, fn_type, cb, args, with_stats: bool):
        """Run rtc_lua_program_<entry>(ctx, prog, *args, fn, NULL, stats) with `cb` (the C callback's arguments after
        `user`) as its callback: a true return value stops the run; an exception stops it and is raised here."""
        raised = []

        def trampoline(_user, *a):
            try:
                return 1 if cb(*a) else 0
            except BaseException as e:  # never unwind through the C frames
                raised.append(e)
                return 1

        st = RtcStats()
        rc = getattr(lib(), entry)(ctx._h, self._h, *args, fn_type(trampoline), None, C.byref(st) if with_stats else None)
        if raised:
            raise raised[0]
        _check(rc, entry)
        return _stats_dict(st, True) if with_stats else None

    def render(self, ctx: "Context", on_frame=None, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False):
        """rtc_lua_program_render: returns the list of (vsize, hsize, 3) uint8 frames in job order — or, with `on_frame`
        (called as on_frame(job_index, frame, outfile, kind); a true return value stops), nothing is kept."""
        frames = []

        def cb(jp, index, rgb8):
            cam = jp.contents.camera
            frame = np.ctypeslib.as_array(rgb8, shape=(cam.vsize, cam.hsize, 3))
            if on_frame is None:
                frames.append(frame.copy())
                return False
            j = jp.contents
            return on_frame(index, frame, (j.outfile or b"").decode(errors="replace"), "AddFrame" if j.kind == 1 else "Render")

        st = self._run(ctx, "rtc_lua_program_render", LUA_FRAME_FN, cb, (mode, flags), with_stats)
        return (frames, st) if with_stats else frames

    def render_to_files(self, ctx: "Context", out_dir, mode: int = MODE_RENDER_ASYNC, flags: int = 0) -> list:
        """render_lua with the files written: Render(world, camera, "x.png") -> out_dir/x.png, "x.ppm" -> the P3 file of
        Canvas::write_to_file_simple; any other extension -> the name + ".png" (render_reference_files writes the JPEGs and
        GIFs). AddFrame frames of StartAnimation("a.gif") -> out_dir/a.gif.0000.png, a.gif.0001.png, ...
        Only the file's base name is used. Returns the paths in job order."""
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        paths = []

        def on_frame(index, frame, outfile, kind):
            name = Path(outfile).name or f"job{index}"
            if kind == "AddFrame":
                target = out / f"{name}.{self.job(index).frame:04d}.png"
            elif name.lower().endswith((".png", ".ppm")):
                target = out / name
            else:
                target = out / (name + ".png")
            if target.suffix.lower() == ".ppm":
                write_ppm_rgb8(target, frame)
            else:
                write_png(target, frame)
            paths.append(target)
            return False

        self.render(ctx, on_frame=on_frame, mode=mode, flags=flags)
        return paths

    def render_gif(self, ctx: "Context", on_frame, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False):
        """rtc_lua_program_render_gif: every job rendered as by render(); on_frame(job_index, data, outfile, kind) gets an
        AddFrame job's GIF record (bytes, quantised and LZW-coded on the GPU) or a Render job's (vsize, hsize, 3) uint8 frame.
        A true return value stops the run."""
        def cb(jp, index, data, nbytes):
            j = jp.contents
            outfile = (j.outfile or b"").decode(errors="replace")
            if j.kind == 1:
                payload = C.string_at(data, nbytes)
            else:
                payload = np.ctypeslib.as_array(data, shape=(j.camera.vsize, j.camera.hsize, 3))
            return on_frame(index, payload, outfile, "AddFrame" if j.kind == 1 else "Render")

        return self._run(ctx, "rtc_lua_program_render_gif", LUA_GIF_FN, cb, (mode, flags), with_stats)

    def render_animations(self, ctx: "Context", out_dir, mode: int = MODE_RENDER_ASYNC, flags: int = 0, on_frame=None) -> list:
        """render_lua with the reference's files: one out_dir/<basename>.gif per StartAnimation call (frames encoded on the
        GPU, rtc_lua_program_render_gif), Render stills written exactly as render_to_files writes them. `on_frame` (optional,
        same arguments as render_gif's) sees every job first; a true return value stops the run (files of the frames so
        far are still written). Returns the paths: stills in job order, then the animations in StartAnimation order."""
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        paths, anims = [], _Animations("render_animations")

        def cb(index, data, outfile, kind):
            stop = bool(on_frame(index, data, outfile, kind)) if on_frame is not None else False
            name = Path(outfile).name or f"job{index}"
            if kind == "AddFrame":
                anims.add(self.job(index), name, data)
            else:
                target = out / name if name.lower().endswith((".png", ".ppm")) else out / (name + ".png")
                if target.suffix.lower() == ".ppm":
                    write_ppm_rgb8(target, data)
                else:
                    write_png(target, data)
                paths.append(target)
            return stop

        try:
            self.render_gif(ctx, cb, mode=mode, flags=flags)
        finally:
            anims.write(out, paths)
        return paths

    def render_files(self, ctx: "Context", on_output, quality: int = 75, mode: int = MODE_RENDER_ASYNC, flags: int = 0,
                     with_stats: bool = False):
        """rtc_lua_program_render_files: every job rendered as by render(); on_output(job_index, fmt, data, outfile, kind) gets,
        by `fmt`, an AddFrame job's GIF record ("gif", bytes), a .jpg / .jpeg Render job's whole JPEG file at `quality`
        ("jpeg", bytes, encoded on the GPU) or any other Render job's (vsize, hsize, 3) uint8 rows ("rgb8").
        A true return value stops the run."""
        names = {LUA_OUT_RGB8: "rgb8", LUA_OUT_GIF_RECORD: "gif", LUA_OUT_JPEG: "jpeg"}

        def cb(jp, index, fmt, data, nbytes):
            j = jp.contents
            outfile = (j.outfile or b"").decode(errors="replace")
            if fmt == LUA_OUT_RGB8:
                payload = np.ctypeslib.as_array(data, shape=(j.camera.vsize, j.camera.hsize, 3))
            else:
                payload = C.string_at(data, nbytes)
            return on_output(index, names[fmt], payload, outfile, "AddFrame" if j.kind == 1 else "Render")

        return self._run(ctx, "rtc_lua_program_render_files", LUA_FILE_FN, cb, (mode, flags, quality), with_stats)

    def render_reference_files(self, ctx: "Context", out_dir, quality: int = 75, mode: int = MODE_RENDER_ASYNC, flags: int = 0) -> list:
        """render_lua with every file under the name the script gave it (only its base name is used): ".jpg" / ".jpeg"
        stills as JPEG encoded on the GPU at `quality` (the reference's `save` uses 75), ".png" / ".ppm" as render_to_files
        writes them, any other extension + ".png", and one GIF per StartAnimation call (+ ".gif" unless the name has it).
        Returns the paths: stills in job order, then the animations in StartAnimation order."""
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        paths, anims = [], _Animations("render_reference_files")

        def cb(index, fmt, data, outfile, kind):
            name = Path(outfile).name or f"job{index}"
            if fmt == "gif":
                anims.add(self.job(index), name, data)
                return False
            if fmt == "jpeg":
                target = out / name
                target.write_bytes(data)
            else:
                target = out / name if name.lower().endswith((".png", ".ppm")) else out / (name + ".png")
                if target.suffix.lower() == ".ppm":
                    write_ppm_rgb8(target, data)
                else:
                    write_png(target, data)
            paths.append(target)
            return False

        try:
            self.render_files(ctx, cb, quality=quality, mode=mode, flags=flags)
        finally:
            anims.write(out, paths)
        return paths

    def render_png_files(self, ctx: "Context", out_dir, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False):
        """render_to_files' files under render_to_files' names, the PNGs compressed on the GPU behind each render
        (rtc_lua_program_render_png: png_encode's bytes, only the file crossing PCIe); ".ppm" stills as render_to_files
        writes them. Returns the paths in job order (and the stats with `with_stats`)."""
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        paths = []

        def cb(jp, index, fmt, data, nbytes):
            j = jp.contents
            name = Path((j.outfile or b"").decode(errors="replace")).name or f"job{index}"
            if j.kind == 1:
                target = out / f"{name}.{j.frame:04d}.png"
            elif name.lower().endswith((".png", ".ppm")):
                target = out / name
            else:
                target = out / (name + ".png")
            if fmt == LUA_OUT_PNG:
                target.write_bytes(C.string_at(data, nbytes))
            else:
                write_ppm_rgb8(target, np.ctypeslib.as_array(data, shape=(j.camera.vsize, j.camera.hsize, 3)))
            paths.append(target)
            return False

        st = self._run(ctx, "rtc_lua_program_render_png", LUA_FILE_FN, cb, (mode, flags), with_stats)
        return (paths, st) if with_stats else paths

    def render_saved_files(self, ctx: "Context", out_dir, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False):
        """render_lua with every file saved as the reference saves it: each Render still under the base name the script gave
        it, in the format its extension names (the save table of include/rtc.h: image_format_for_name), encoded on the GPU
        behind its render (rtc_lua_program_render_saved); one GIF per StartAnimation call (+ ".gif" unless the name has it).
        An unsupported name raises RtcError (RTC_ERR_UNSUPPORTED) before anything is rendered or written. Returns the paths:
        stills in job order, then the animations in StartAnimation order (and the stats with `with_stats`)."""
        out = Path(out_dir)
        paths, anims = [], _Animations("render_saved_files")

        def cb(jp, index, fmt, data, nbytes):
            j = jp.contents
            name = Path((j.outfile or b"").decode(errors="replace")).name or f"job{index}"
            if fmt == LUA_OUT_GIF_RECORD:
                anims.add(j, name, C.string_at(data, nbytes))
            else:
                out.mkdir(parents=True, exist_ok=True)
                target = out / name
                target.write_bytes(C.string_at(data, nbytes))
                paths.append(target)
            return False

        try:
            st = self._run(ctx, "rtc_lua_program_render_saved", LUA_FILE_FN, cb, (mode, flags), with_stats)
        finally:
            anims.write(out, paths)
        return (paths, st) if with_stats else paths

    def close(self):
        if getattr(self, "_h", None):
            lib().rtc_lua_program_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_lua(text: str | None = None, path: str | None = None, render_index: int = 0):
    """One job of a Lua scene script (rtc_scene_load_lua) -> (World, RtcCamera, outfile, n_jobs)."""
    shapes = C.POINTER(RtcShape)()
    n, renders = C.c_uint32(0), C.c_uint32(0)
    lgts, nl, cam = (RtcAreaLight * MAX_LIGHT_SAMPLES)(), C.c_uint32(0), RtcCamera()
    err, outfile = C.create_string_buffer(512), C.create_string_buffer(512)
    if path is not None:
        st = lib().rtc_scene_load_lua_area_lights_file(str(path).encode(), render_index, C.byref(shapes), C.byref(n), lgts, MAX_LIGHT_SAMPLES, C.byref(nl),
                                                       C.byref(cam), outfile, 512, C.byref(renders), err, 512)
    else:
        st = lib().rtc_scene_load_lua_area_lights(text.encode(), render_index, C.byref(shapes), C.byref(n), lgts, MAX_LIGHT_SAMPLES, C.byref(nl),
                                                  C.byref(cam), outfile, 512, C.byref(renders), err, 512)
    _check(st, "rtc_scene_load_lua", err.value.decode(errors="replace"))
    w = World([_copy_light(lgts[i]) for i in range(nl.value)])
    for i in range(n.value):
        s = RtcShape()
        C.memmove(C.byref(s), C.byref(shapes[i]), C.sizeof(RtcShape))
        w.shapes.append(s)
    lib().rtc_free(shapes)
    return w, cam, outfile.value.decode(errors="replace"), renders.value


def format_ppm(rgb: np.ndarray) -> bytes:
    """Canvas::write_to_file_simple (canvas.rs:86-109) into memory."""
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    h, w = a.shape[0], a.shape[1]
    p = a.ctypes.data_as(C.POINTER(C.c_double))
    need = lib().rtc_canvas_format_ppm(p, w, h, None, 0)
    buf = C.create_string_buffer(need + 1)
    lib().rtc_canvas_format_ppm(p, w, h, buf, need + 1)
    return buf.raw[:need]


def to_rgba8(canvas: np.ndarray, gamma: float = 1.0) -> np.ndarray:
    """Canvas::to_imgbuf (canvas.rs:61-79): (H, W, 4) uint8, gamma-corrected, alpha 255."""
    c = np.ascontiguousarray(canvas, dtype=np.float64)
    h, w = c.shape[0], c.shape[1]
    out = np.empty((h, w, 4), dtype=np.uint8)
    lib().rtc_canvas_to_rgba8(c.ctypes.data_as(C.POINTER(C.c_double)), w, h, gamma, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def gamma_thresholds(gamma: float) -> np.ndarray:
    """The 255 quantisation thresholds T[1..255] behind the device's to_imgbuf at `gamma` (rtc_gamma_thresholds): byte(c) =
    #{k : T[k] <= c} for c >= +0. Raises RtcError (RTC_ERR_ARG) unless gamma is positive and finite."""
    out = np.empty(255, dtype=np.float64)
    _check(lib().rtc_gamma_thresholds(gamma, out.ctypes.data_as(C.POINTER(C.c_double))), "rtc_gamma_thresholds")
    return out


def color_scale255(rgb: np.ndarray) -> np.ndarray:
    """Color::scale(c, 255) (color.rs:100-114) element-wise on the host."""
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    out = np.empty(a.shape, dtype=np.uint8)
    lib().rtc_color_scale255(a.ctypes.data_as(C.POINTER(C.c_double)), a.size, out.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out


def format_ppm_rgb8(rgb8: np.ndarray) -> bytes:
    """The PPM of a frame that is already quantised ((H, W, 3) uint8, Color::scale'd: rtc_render_rgb8)."""
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w = a.shape[0], a.shape[1]
    p = a.ctypes.data_as(C.POINTER(C.c_uint8))
    need = lib().rtc_canvas_format_ppm_rgb8(p, w, h, None, 0)
    buf = C.create_string_buffer(need + 1)
    lib().rtc_canvas_format_ppm_rgb8(p, w, h, buf, need + 1)
    return buf.raw[:need]


def write_ppm_rgb8(path, rgb8: np.ndarray) -> None:
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    _check(lib().rtc_canvas_write_ppm_rgb8(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0]),
           "Canvas.write_to_file_simple (rgb8)")


def format_png(pixels: np.ndarray) -> bytes:
    """An 8-bit PNG (rtc_canvas_format_png8) of a (H, W, 3) or (H, W, 4) uint8 frame — Canvas::write_to_file's ".png" case."""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError("pixels must be (H, W, 3) or (H, W, 4) uint8")
    h, w, c = a.shape
    P8 = C.POINTER(C.c_uint8)
    need = lib().rtc_canvas_format_png8(a.ctypes.data_as(P8), w, h, c, None, 0)
    if need == 0:
        raise ValueError("empty frame")
    buf = np.empty(need, dtype=np.uint8)
    lib().rtc_canvas_format_png8(a.ctypes.data_as(P8), w, h, c, buf.ctypes.data_as(P8), need)
    return buf.tobytes()


def write_png(path, pixels: np.ndarray) -> None:
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError("pixels must be (H, W, 3) or (H, W, 4) uint8")
    _check(lib().rtc_canvas_write_png8(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0], a.shape[2]), "rtc_canvas_write_png8")


def gif_file_header(width: int, height: int) -> bytes:
    """The 13 bytes in front of a GIF's first frame (include/rtc.h): GIF89a, the logical screen, no global table."""
    if not (0 < width <= 65535 and 0 < height <= 65535):
        raise RtcError(4, "gif_file_header", f"{width}x{height}")
    return b"GIF89a" + int(width).to_bytes(2, "little") + int(height).to_bytes(2, "little") + b"\0\0\0"


def _frames_u8(frames) -> np.ndarray:
    fs = [np.asarray(f) for f in frames]
    if not fs:
        raise ValueError("no frames")
    for f in fs:
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError("frames must be (H, W, 3) uint8")
        if f.shape != fs[0].shape:
            raise RtcError(4, "gif_encode", f"frame of {f.shape[1]}x{f.shape[0]} in a {fs[0].shape[1]}x{fs[0].shape[0]} animation")
    return np.ascontiguousarray(np.stack(fs))


def gif_quantize(frame: np.ndarray):
    """The GIF quantiser of include/rtc.h on the host (rtc_gif_quantize): (palette (256, 3) uint8, indices (H, W) uint8,
    used entries)."""
    a = np.ascontiguousarray(frame, dtype=np.uint8)
    h, w = a.shape[0], a.shape[1]
    P8 = C.POINTER(C.c_uint8)
    pal = np.empty((256, 3), dtype=np.uint8)
    idx = np.empty((h, w), dtype=np.uint8)
    used = C.c_uint32()
    _check(lib().rtc_gif_quantize(a.ctypes.data_as(P8), w, h, pal.ctypes.data_as(P8), idx.ctypes.data_as(P8), C.byref(used)), "rtc_gif_quantize")
    return pal, idx, used.value


def gif_lzw(indices: np.ndarray) -> bytes:
    """The segmented LZW code stream of include/rtc.h for an index stream (rtc_gif_lzw), before sub-blocking."""
    a = np.ascontiguousarray(indices, dtype=np.uint8).ravel()
    P8 = C.POINTER(C.c_uint8)
    need = lib().rtc_gif_lzw(a.ctypes.data_as(P8), a.size, None, 0)
    buf = np.empty(need, dtype=np.uint8)
    lib().rtc_gif_lzw(a.ctypes.data_as(P8), a.size, buf.ctypes.data_as(P8), need)
    return buf.tobytes()


def gif_encode(frames) -> bytes:
    """An animated GIF of equal-sized (H, W, 3) uint8 frames, encoded on the host (rtc_gif_format): what
    StartAnimation / AddFrame write, by the rules of include/rtc.h. Frames of different sizes, or a side above 65535, raise
    RtcError (RTC_ERR_ARG)."""
    a = _frames_u8(frames)
    n, h, w = a.shape[0], a.shape[1], a.shape[2]
    P8 = C.POINTER(C.c_uint8)
    need = lib().rtc_gif_format(a.ctypes.data_as(P8), n, w, h, None, 0)
    if need == 0:
        raise RtcError(4, "rtc_gif_format", f"{w}x{h}")
    buf = np.empty(need, dtype=np.uint8)
    lib().rtc_gif_format(a.ctypes.data_as(P8), n, w, h, buf.ctypes.data_as(P8), need)
    return buf.tobytes()


def _pixels_u8(pixels) -> np.ndarray:
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError("pixels must be an (H, W, 3) or (H, W, 4) uint8 array")
    return a


def jpeg_quant_tables(quality: int = 75) -> np.ndarray:
    """The (2, 64) luma and chroma quantisation tables at `quality`, natural order (rtc_jpeg_quant_tables)."""
    out = np.empty((2, 64), dtype=np.uint16)
    _check(lib().rtc_jpeg_quant_tables(quality, out.ctypes.data_as(C.POINTER(C.c_uint16))), "rtc_jpeg_quant_tables", f"quality {quality}")
    return out


def jpeg_fdct(samples: np.ndarray) -> np.ndarray:
    """The integer forward DCT of include/rtc.h (libjpeg's ISLOW, output scaled by 8) of an 8x8 block of samples 0..255
    (rtc_jpeg_fdct): an (8, 8) int32 array, natural order."""
    a = np.ascontiguousarray(samples, dtype=np.uint8).reshape(64)
    out = np.empty(64, dtype=np.int32)
    _check(lib().rtc_jpeg_fdct(a.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_int32))), "rtc_jpeg_fdct")
    return out.reshape(8, 8)


def jpeg_coefficients(pixels: np.ndarray, quality: int = 75) -> np.ndarray:
    """The quantised blocks of a JPEG of `pixels` (rtc_jpeg_coefficients): (MCUs, 3, 64) int16, MCUs in raster order, Y, Cb,
    Cr per MCU, natural order."""
    a = _pixels_u8(pixels)
    h, w, c = a.shape
    out = np.empty((((w + 7) // 8) * ((h + 7) // 8), 3, 64), dtype=np.int16)
    _check(lib().rtc_jpeg_coefficients(a.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, c, quality, out.ctypes.data_as(C.POINTER(C.c_int16))),
           "rtc_jpeg_coefficients", f"{w}x{h}x{c} quality {quality}")
    return out


def jpeg_encode(pixels: np.ndarray, quality: int = 75) -> bytes:
    """A baseline 4:4:4 JPEG of an (H, W, 3) or (H, W, 4) uint8 frame, encoded on the host (rtc_jpeg_format): what
    Canvas::write_to_file writes for a ".jpg" name (include/rtc.h; alpha ignored)."""
    a = _pixels_u8(pixels)
    h, w, c = a.shape
    P8 = C.POINTER(C.c_uint8)
    need = lib().rtc_jpeg_format(a.ctypes.data_as(P8), w, h, c, quality, None, 0)
    if need == 0:
        raise RtcError(4, "rtc_jpeg_format", f"{w}x{h}x{c} quality {quality}")
    buf = np.empty(need, dtype=np.uint8)
    lib().rtc_jpeg_format(a.ctypes.data_as(P8), w, h, c, quality, buf.ctypes.data_as(P8), need)
    return buf.tobytes()


def write_jpeg(path, pixels: np.ndarray, quality: int = 75) -> None:
    """rtc_canvas_write_jpeg: jpeg_encode's bytes to `path`."""
    a = _pixels_u8(pixels)
    _check(lib().rtc_canvas_write_jpeg(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0], a.shape[2], quality),
           "rtc_canvas_write_jpeg")


def png_filter(pixels: np.ndarray):
    """The row filters of the compressed PNG writer (rtc_png_filter): (types, filtered) — each row's filter type (H uint8)
    and the filtered stream, H * (1 + W * C) uint8 (per row the type byte, then the filtered row)."""
    a = _pixels_u8(pixels)
    h, w, c = a.shape
    P8 = C.POINTER(C.c_uint8)
    types = np.empty(h, dtype=np.uint8)
    filtered = np.empty(h * (1 + w * c), dtype=np.uint8)
    _check(lib().rtc_png_filter(a.ctypes.data_as(P8), w, h, c, types.ctypes.data_as(P8), filtered.ctypes.data_as(P8)),
           "rtc_png_filter", f"{w}x{h}x{c}")
    return types, filtered


def png_encode(pixels: np.ndarray) -> bytes:
    """A filtered, deflate-compressed 8-bit PNG of an (H, W, 3) or (H, W, 4) uint8 frame, encoded on the host
    (rtc_png_format): the bytes PngEncoder produces on the GPU. format_png stays the stored writer."""
    a = _pixels_u8(pixels)
    h, w, c = a.shape
    P8 = C.POINTER(C.c_uint8)
    need = lib().rtc_png_format(a.ctypes.data_as(P8), w, h, c, None, 0)
    if need == 0:
        raise RtcError(4, "rtc_png_format", f"{w}x{h}x{c}")
    buf = np.empty(need, dtype=np.uint8)
    lib().rtc_png_format(a.ctypes.data_as(P8), w, h, c, buf.ctypes.data_as(P8), need)
    return buf.tobytes()


def write_png_deflate(path, pixels: np.ndarray) -> None:
    """rtc_canvas_write_png: png_encode's bytes to `path`."""
    a = _pixels_u8(pixels)
    _check(lib().rtc_canvas_write_png(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0], a.shape[2]),
           "rtc_canvas_write_png")


def image_format_for_name(name) -> int:
    """The save table's format for a file name (rtc_image_format_for_name): one of IMAGE_FORMATS' values. The extension is
    the last one of the name's last component, any case; an unsupported or missing one raises RtcError
    (RTC_ERR_UNSUPPORTED)."""
    f = C.c_uint32()
    _check(lib().rtc_image_format_for_name(str(name).encode(), C.byref(f)), "rtc_image_format_for_name", str(name))
    return f.value


def _image_format(fmt) -> int:
    return IMAGE_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)


def image_encode(fmt, pixels: np.ndarray) -> bytes:
    """The file of an (H, W, 3) or (H, W, 4) uint8 frame in format `fmt` (a name of IMAGE_FORMATS or its value), encoded on
    the host (rtc_image_format): what Canvas::write_to_file saves for a name of that format, and what ImageEncoder makes on
    the GPU. The 3- and the 4-channel form of a frame give the same bytes."""
    a = _pixels_u8(pixels)
    h, w, c = a.shape
    f = _image_format(fmt)
    P8 = C.POINTER(C.c_uint8)
    need = lib().rtc_image_format(f, a.ctypes.data_as(P8), w, h, c, None, 0)
    if need == 0:
        raise RtcError(4, "rtc_image_format", f"format {fmt}, {w}x{h}x{c}")
    buf = np.empty(need, dtype=np.uint8)
    lib().rtc_image_format(f, a.ctypes.data_as(P8), w, h, c, buf.ctypes.data_as(P8), need)
    return buf.tobytes()


def save(path, pixels: np.ndarray) -> None:
    """rtc_canvas_save: image_encode's bytes for the format `path`'s extension names, written to `path`. A float64 (H, W, 3)
    canvas under a name of the float table (.hdr, .pfm, .exr) is saved as data (rtc_canvas_save_f64: float_encode's bytes,
    EXR as HALF); every other array and name goes through the 8-bit table as before."""
    if isinstance(pixels, np.ndarray) and pixels.dtype == np.float64 and lib().rtc_float_format_for_name(str(path).encode(), C.byref(C.c_uint32())) == 0:
        a = _canvas_f64(pixels)
        _check(lib().rtc_canvas_save_f64(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[1], a.shape[0]),
               "rtc_canvas_save_f64", str(path))
        return
    a = _pixels_u8(pixels)
    _check(lib().rtc_canvas_save(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0], a.shape[2]),
           "rtc_canvas_save", str(path))


# ---- float files (include/rtc.h, "float files"): Radiance HDR, PFM, OpenEXR ----------------------------------------------
def float_format_for_name(name) -> int:
    """The float table's format for a file name (rtc_float_format_for_name): one of FLOAT_FORMATS' values; any other
    extension raises RtcError (RTC_ERR_UNSUPPORTED)."""
    f = C.c_uint32()
    _check(lib().rtc_float_format_for_name(str(name).encode(), C.byref(f)), "rtc_float_format_for_name", str(name))
    return f.value


def _float_format(fmt) -> int:
    return FLOAT_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)


def _canvas_f64(rgb) -> np.ndarray:
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("the canvas must be an (H, W, 3) float64 array")
    return a


def _float_planes(rgb_address, plane_addresses: dict, rgb_type) -> RtcFloatPlanes:
    """rtc_float_planes from the canvas' address (or None) and {plane: address}."""
    p = RtcFloatPlanes()
    p.rgb = rgb_address
    p.aov = _aov_buffers(plane_addresses or {})
    p.rgb_type = EXR_TYPES[rgb_type] if isinstance(rgb_type, str) else int(rgb_type)
    return p


def float_encode(fmt, rgb=None, planes=None, rgb_type="half") -> bytes:
    """The float file of an (H, W, 3) float64 canvas in format `fmt` ("hdr", "pfm", "exr" or its value), encoded on the host
    (rtc_float_format): what FloatEncoder makes on the GPU. EXR also stores the AOV planes of `planes` ({plane: array}, as
    DeviceWorld.render_aov returns them; "flags" is not stored) — with or without a canvas — and its R, G, B as `rgb_type`
    ("half" or "float")."""
    a = None if rgb is None else _canvas_f64(rgb)
    arrays = dict(planes or {})
    b = _aov_host_buffers(arrays) if arrays else RtcAovBuffers()
    shapes = {x.shape[:2] for x in ([a] if a is not None else []) + list(arrays.values())}
    if len(shapes) != 1:
        raise ValueError("float_encode needs a canvas or planes, all of one height and width")
    h, w = shapes.pop()
    p = _float_planes(None if a is None else a.ctypes.data, {}, rgb_type)
    p.aov = b
    f = _float_format(fmt)
    P8 = C.POINTER(C.c_uint8)
    need = lib().rtc_float_format(f, C.byref(p), w, h, None, 0)
    if need == 0:
        raise RtcError(4, "rtc_float_format", f"format {fmt}, {w}x{h}")
    buf = np.empty(need, dtype=np.uint8)
    lib().rtc_float_format(f, C.byref(p), w, h, buf.ctypes.data_as(P8), need)
    return buf.tobytes()


def hdr_rle_row(plane) -> bytes:
    """One byte plane of one Radiance scanline, run-length coded by the maximal-run rule (rtc_hdr_rle_row)."""
    a = np.ascontiguousarray(plane, dtype=np.uint8).reshape(-1)
    n = C.c_size_t()
    P8 = C.POINTER(C.c_uint8)
    _check(lib().rtc_hdr_rle_row(a.ctypes.data_as(P8), a.size, None, 0, C.byref(n)), "rtc_hdr_rle_row")
    buf = np.empty(n.value, dtype=np.uint8)
    _check(lib().rtc_hdr_rle_row(a.ctypes.data_as(P8), a.size, buf.ctypes.data_as(P8), n.value, C.byref(n)), "rtc_hdr_rle_row")
    return buf.tobytes()


def write_ppm(path, rgb: np.ndarray) -> None:
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    _check(lib().rtc_canvas_write_ppm(str(path).encode(), a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[1], a.shape[0]), "Canvas.write_to_file_simple")


# ---------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------
# ---- AOV planes (include/rtc.h, "arbitrary output variables") ----------------------------------------------------------
def _aov_view_id(view) -> int:
    return AOV_VIEWS[view] if isinstance(view, str) else int(view)


def _aov_arrays(planes, height: int, width: int) -> dict:
    """Fresh host arrays for the named planes: (H, W) or (H, W, 3), dtypes of include/rtc.h."""
    out = {}
    for name in planes:
        dtype, comps = AOV_PLANES[name]  # KeyError: not a plane
        out[name] = np.empty((height, width) if comps == 1 else (height, width, comps), dtype=dtype)
    if not out:
        raise ValueError("at least one AOV plane must be asked for")
    return out


def _aov_buffers(addresses: dict) -> RtcAovBuffers:
    """rtc_aov_buffers from {plane: address}; planes that are missing or None stay NULL (not wanted)."""
    b = RtcAovBuffers()
    for name, addr in addresses.items():
        if name not in AOV_PLANES:
            raise KeyError(name)
        setattr(b, name, addr)
    return b


def _aov_host_buffers(arrays: dict) -> RtcAovBuffers:
    for name, a in arrays.items():
        dtype, comps = AOV_PLANES[name]
        if a.dtype != np.dtype(dtype) or not a.flags.c_contiguous:
            raise ValueError(f"plane {name!r} must be a C-contiguous {dtype} array")
    return _aov_buffers({name: a.ctypes.data for name, a in arrays.items()})


def aov_from_hits(hits, width: int, height: int, mode: int = MODE_RENDER_ASYNC, shadow_counts=None,
                  planes=("index", "depth", "point", "normal", "flags", "shadow")) -> dict:
    """rtc_aov_from_hits: width * height hit records (an RtcHit array, row-major) packed into the AOV planes, the mode
    rule included. `shadow_counts`: per-pixel shadowed-sample counts (default: each record's own `shadowed`)."""
    out = _aov_arrays(planes, height, width)
    sc = None
    if shadow_counts is not None:
        sc = np.ascontiguousarray(shadow_counts, dtype=np.uint16).reshape(-1)
        if sc.size != width * height:
            raise ValueError("shadow_counts must hold one count per pixel")
    if len(hits) < width * height:
        raise ValueError("hits must hold one record per pixel")
    b = _aov_host_buffers(out)
    _check(lib().rtc_aov_from_hits(hits, sc.ctypes.data_as(C.POINTER(C.c_uint16)) if sc is not None else None, width, height, mode,
                                   C.byref(b)), "rtc_aov_from_hits")
    return out


def aov_view(view, planes: dict, near: float = 0.0, far: float = 1.0, n_lights: int = 1) -> np.ndarray:
    """rtc_aov_view_rgb8: one plane ("depth", "normal", "index" or "shadow") of `planes` as an (H, W, 3) uint8 picture."""
    v = _aov_view_id(view)
    arrays = {k: np.ascontiguousarray(a, dtype=AOV_PLANES[k][0]) for k, a in planes.items() if a is not None}
    first = next(iter(arrays.values()), None)
    if first is None:
        raise ValueError("no plane given")
    h, w = first.shape[:2]
    out = np.empty((h, w, 3), dtype=np.uint8)
    b = _aov_host_buffers(arrays)
    _check(lib().rtc_aov_view_rgb8(v, C.byref(b), w, h, near, far, n_lights, out.ctypes.data_as(C.POINTER(C.c_uint8))), "rtc_aov_view_rgb8")
    return out


def _stats_dict(s: RtcStats, with_resample: bool = False) -> dict:
    d = {"rays_primary": s.rays_primary, "rays_shadow": s.rays_shadow, "rays_reflect": s.rays_reflect,
         "rays_refract": s.rays_refract, "pixels": s.pixels}
    if with_resample or s.pixels_resample:
        d["pixels_resample"] = s.pixels_resample
    return d


class Context:
    """One GPU + one stream (rtc_context). `stream` is a raw hipStream_t value (int) or None."""

    def __init__(self, device: int = 0, stream: int | None = None, _borrowed=None):
        self._worlds = []  # weak references to the worlds uploaded through this context
        self._owned = _borrowed is None
        if _borrowed is not None:   # a group member's context: owned by the group
            self._h = C.c_void_p(_borrowed)
            self.device = device
            return
        self._h = C.c_void_p()
        _check(lib().rtc_context_create(device, C.c_void_p(stream or None), C.byref(self._h)), "rtc_context_create",
               "no usable MI355X (gfx950); this library has no CPU fallback")
        self.device = device

    def close(self):
        if self._h:
            for ref in self._worlds:
                w = ref()
                if w is not None:
                    w.close()
            self._worlds = []
            if self._owned:
                lib().rtc_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().rtc_context_synchronize(self._h), "rtc_context_synchronize")

    def device_info(self):
        name = C.create_string_buffer(128)
        cu, mhz = C.c_int32(), C.c_int32()
        _check(lib().rtc_context_device_info(self._h, name, 128, C.byref(cu), C.byref(mhz)), "rtc_context_device_info")
        return {"name": name.value.decode(), "compute_units": cu.value, "clock_mhz": mhz.value}

    def upload(self, world: World) -> "DeviceWorld":
        return DeviceWorld(self, world)

    def stats(self, extended: bool = False) -> dict:
        """Ray counters since the last reset. extended=True adds `rays_primary_proven_miss` (of rays_primary: primary rays of
        tiles the binning kernel proved black — counted as cast, answered without generating a ray; include/rtc.h)."""
        s = RtcStats()
        _check(lib().rtc_stats_read(self._h, C.byref(s)), "rtc_stats_read")
        d = _stats_dict(s)
        if extended:
            d["rays_primary_proven_miss"] = s.rays_primary_proven_miss
        return d

    def reset_stats(self):
        _check(lib().rtc_stats_reset(self._h), "rtc_stats_reset")

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(lib().rtc_last_kernel_ms(self._h, C.byref(ms)), "rtc_last_kernel_ms")
        return ms.value

    def set_timing(self, every: int) -> None:
        """Time every `every`-th render launch (1 = all, 0 = none); see include/rtc.h."""
        _check(lib().rtc_context_set_timing(self._h, every), "rtc_context_set_timing")

    def kernel_times_ms(self, last: int = 1024) -> np.ndarray:
        """Durations (ms) of the most recent `last` render launches, oldest first (include/rtc.h)."""
        buf = (C.c_float * max(1, last))()
        n = C.c_uint32()
        _check(lib().rtc_kernel_times_ms(self._h, buf, last, C.byref(n)), "rtc_kernel_times_ms")
        return np.frombuffer(buf, dtype=np.float32, count=n.value).copy()

    def set_pipeline(self, depth: int) -> None:
        """Deal consecutive render launches over `depth` streams of the context's own (rtc_context_set_pipeline):
        outputs of `depth` consecutive launches must not overlap; results are complete after synchronize()."""
        _check(lib().rtc_context_set_pipeline(self._h, depth), "rtc_context_set_pipeline")

    def fence(self) -> None:
        """Make the context's stream wait for every launch enqueued so far (no host wait)."""
        _check(lib().rtc_context_fence(self._h), "rtc_context_fence")

    def last_launch_info(self) -> dict:
        """Object source, lists and lane the most recent render launch ran with (rtc_context_last_launch_info)."""
        i = RtcLaunchInfo()
        _check(lib().rtc_context_last_launch_info(self._h, C.byref(i)), "rtc_context_last_launch_info")
        pk = C.c_uint32(0)
        _check(lib().rtc_context_last_launch_projection(self._h, C.byref(pk)), "rtc_context_last_launch_projection")
        return {"source": i.source, "source_name": SOURCE_NAMES.get(i.source, "?"), "reflective": bool(i.reflective),
                "refractive": bool(i.refractive), "binned_primary_pass": bool(i.binned), "light_lists": bool(i.light_lists),
                "lane": i.lane, "threads_per_workgroup": i.block, "dynamic_lds_bytes": i.lds_bytes,
                "tiles_per_workgroup": i.tiles_per_workgroup, "multi_tile_workgroups": i.multi_tile_workgroups,
                "light_table": bool(i.light_table), "lens_samples": i.lens_samples, "projection": pk.value}

    def binning_times_ms(self, last: int = 1024) -> np.ndarray:
        """Durations (ms) of the binning kernels of the most recent `last` timed launches (0 where a launch had none)."""
        buf = (C.c_float * max(1, last))()
        n = C.c_uint32()
        _check(lib().rtc_binning_times_ms(self._h, buf, last, C.byref(n)), "rtc_binning_times_ms")
        return np.frombuffer(buf, dtype=np.float32, count=n.value).copy()

    def canvas_to_rgba8_device(self, d_ptr: int, width: int, height: int, gamma: float, d_out: int) -> None:
        """Canvas::to_imgbuf of an f64 canvas in DEVICE memory (address `d_ptr`, height x width x 3 doubles) into the device
        buffer `d_out` (height x width x 4 bytes), enqueued on the context's stream (rtc_canvas_to_rgba8_device)."""
        _check(lib().rtc_canvas_to_rgba8_device(self._h, d_ptr, width, height, gamma, d_out), "rtc_canvas_to_rgba8_device")

    def aov_view_device(self, view, pointers: dict, width: int, height: int, d_out: int, near: float = 0.0, far: float = 1.0,
                        n_lights: int = 1) -> None:
        """aov_view of planes in DEVICE memory ({plane: address}) into the device buffer `d_out` (height x width x 3 bytes),
        enqueued on the context's stream (rtc_aov_view_rgb8_device): the same bytes as the host function."""
        b = _aov_buffers(pointers)
        _check(lib().rtc_aov_view_rgb8_device(self._h, _aov_view_id(view), C.byref(b), width, height, near, far, n_lights, C.c_void_p(d_out)),
               "rtc_aov_view_rgb8_device")

    def apply_ao_device(self, d_rgb: int, d_ao: int, n_samples: int, strength: float, width: int, height: int) -> None:
        """apply_ao in place on an f64 canvas and a uint16 plane in DEVICE memory, enqueued on the context's stream
        (rtc_canvas_apply_ao_device): the same bytes as the host function."""
        _check(lib().rtc_canvas_apply_ao_device(self._h, C.c_void_p(d_rgb), C.c_void_p(d_ao), int(n_samples), float(strength), width, height),
               "rtc_canvas_apply_ao_device")

    def add_scaled_device(self, d_rgb: int, d_plane: int, strength: float, width: int, height: int) -> None:
        """add_scaled in place on an f64 canvas and an f64 plane in DEVICE memory, enqueued on the context's stream
        (rtc_canvas_add_scaled_device): the same bytes as the host function."""
        _check(lib().rtc_canvas_add_scaled_device(self._h, C.c_void_p(d_rgb), C.c_void_p(d_plane), float(strength), width, height),
               "rtc_canvas_add_scaled_device")

    def plane_filter_device(self, d_in: int, channels: int, pointers: dict, width: int, height: int, flt: RtcFilter, d_out: int) -> None:
        """plane_filter of an f64 plane of `channels` values per pixel in DEVICE memory into the device buffer `d_out`, under the
        guides `pointers` = {"index", "point", "normal"} (device addresses), enqueued on the context's stream
        (rtc_plane_filter_device): the same bytes as the host function."""
        b = _aov_buffers(pointers)
        _check(lib().rtc_plane_filter_device(self._h, C.c_void_p(d_in), int(channels), C.byref(b), width, height, C.byref(flt), C.c_void_p(d_out)),
               "rtc_plane_filter_device")

    def counts_to_fraction_device(self, d_counts: int, n: int, width: int, height: int, d_out: int) -> None:
        """counts_to_fraction of a uint16 plane in DEVICE memory into the f64 device buffer `d_out`, enqueued on the context's
        stream (rtc_counts_to_fraction_device): the same bytes as the host function."""
        _check(lib().rtc_counts_to_fraction_device(self._h, C.c_void_p(d_counts), int(n), width, height, C.c_void_p(d_out)),
               "rtc_counts_to_fraction_device")

    def apply_occlusion_device(self, d_rgb: int, d_occ: int, strength: float, width: int, height: int) -> None:
        """apply_occlusion in place on an f64 canvas and an f64 fraction plane in DEVICE memory, enqueued on the context's stream
        (rtc_canvas_apply_occlusion_device): the same bytes as the host function."""
        _check(lib().rtc_canvas_apply_occlusion_device(self._h, C.c_void_p(d_rgb), C.c_void_p(d_occ), float(strength), width, height),
               "rtc_canvas_apply_occlusion_device")

    def adaptive_mask_device(self, d_rgb: int, width: int, height: int, mode: int, threshold: float, d_mask: int) -> None:
        """adaptive_mask of an f64 canvas in DEVICE memory into the device bytes `d_mask`, enqueued on the context's stream
        (rtc_adaptive_mask_device): the same bytes as the host function."""
        _check(lib().rtc_adaptive_mask_device(self._h, C.c_void_p(d_rgb), width, height, mode, float(threshold), C.c_void_p(d_mask)),
               "rtc_adaptive_mask_device")

    def luminance_device(self, d_rgb: int, width: int, height: int, d_out: int) -> None:
        """rtc.luminance of an f64 canvas in DEVICE memory into the 24 device bytes at `d_out`, enqueued on the context's stream
        (rtc_canvas_luminance_device): the host function's bytes, no host wait."""
        _check(lib().rtc_canvas_luminance_device(self._h, C.c_void_p(d_rgb), width, height, C.c_void_p(d_out)), "rtc_canvas_luminance_device")

    def tonemap_device(self, d_in: int, width: int, height: int, spec: RtcTonemap, d_out: int, d_stats: int | None = None) -> None:
        """rtc.tonemap of a canvas in DEVICE memory into `d_out` (may be `d_in`), enqueued on the context's stream
        (rtc_canvas_tonemap_device); `d_stats`: the record luminance_device left in device memory, needed with an AUTO flag."""
        _check(lib().rtc_canvas_tonemap_device(self._h, C.c_void_p(d_in), width, height, C.byref(spec), C.c_void_p(d_stats) if d_stats else None,
                                               C.c_void_p(d_out)), "rtc_canvas_tonemap_device")

    def bloom_device(self, d_in: int, width: int, height: int, spec: RtcBloom, d_out: int) -> None:
        """rtc.bloom of a canvas in DEVICE memory into `d_out` (may be `d_in`), enqueued on the context's stream
        (rtc_canvas_bloom_device)."""
        _check(lib().rtc_canvas_bloom_device(self._h, C.c_void_p(d_in), width, height, C.byref(spec), C.c_void_p(d_out)), "rtc_canvas_bloom_device")

    def resize_device(self, d_in: int, w_in: int, h_in: int, spec: RtcResize, d_out: int, w_out: int, h_out: int) -> None:
        """rtc.resize of a canvas in DEVICE memory into `d_out` (w_out * h_out * 3 doubles, not overlapping `d_in`), enqueued on
        the context's stream (rtc_canvas_resize_device). A new (n_in, n_out, filter) axis waits for the stream once, to upload its table."""
        _check(lib().rtc_canvas_resize_device(self._h, C.c_void_p(d_in), w_in, h_in, C.byref(spec), C.c_void_p(d_out), w_out, h_out),
               "rtc_canvas_resize_device")

    def shutter(self) -> "Shutter":
        """A motion-blur renderer bound to this context (rtc_shutter): Shutter.render and its 8-bit / device forms."""
        return Shutter(self)

    def canvas_average_device(self, d_frames: int, n: int, count: int, d_out: int) -> None:
        """canvas_average of n frames of `count` doubles at DEVICE address `d_frames` into the device buffer `d_out`, enqueued
        on the context's stream (rtc_canvas_average_device): the same bytes as the host function."""
        _check(lib().rtc_canvas_average_device(self._h, C.c_void_p(d_frames), n, count, C.c_void_p(d_out)), "rtc_canvas_average_device")

    def device_arith(self, op: int, a: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.float64)
        bb = np.ascontiguousarray(b if b is not None else a, dtype=np.float64)
        out = np.empty_like(a)
        P = C.POINTER(C.c_double)
        _check(lib().rtc_device_arith(self._h, op, a.ctypes.data_as(P), bb.ctypes.data_as(P), a.size, out.ctypes.data_as(P)), "rtc_device_arith")
        return out


class _Pinned:
    """Owner of one rtc_host_alloc block; freed when the last array viewing it is gone."""

    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        _check(lib().rtc_host_alloc(nbytes, C.byref(self.ptr)), "rtc_host_alloc")
        self.buf = (C.c_char * nbytes).from_address(self.ptr.value)
        self.buf._owner = self  # numpy views hold `buf`; the cycle keeps this owner exactly as long

    def __del__(self):
        try:
            if self.ptr:
                lib().rtc_host_free(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def host_canvas(vsize: int, hsize: int) -> np.ndarray:
    """A zeroed (vsize, hsize, 3) float64 canvas in page-locked memory (rtc_host_alloc)."""
    arr = np.frombuffer(_Pinned(vsize * hsize * 24).buf, dtype=np.float64).reshape(vsize, hsize, 3)
    arr[...] = 0.0
    return arr


class DeviceWorld:
    """Flattened World resident in HBM (rtc_world)."""

    def __init__(self, ctx: Context, world: World):
        self.ctx = ctx
        self._h = C.c_void_p()
        arr = world.array()
        if world.needs_area_entries():
            _check(lib().rtc_world_create_area_lights(ctx._h, arr, len(world.shapes), world.area_light_array(), len(world.lights), C.byref(self._h)),
                   "rtc_world_create_area_lights")
        else:
            _check(lib().rtc_world_create_lights(ctx._h, arr, len(world.shapes), world.light_array(), len(world.lights), C.byref(self._h)),
                   "rtc_world_create_lights")
        self.n = len(world.shapes)
        ctx._worlds.append(weakref.ref(self))

    def update(self, world: World) -> None:
        """Replace the resident World's contents by `world` (rtc_world_update): ordered like a launch, rebuilt on the
        device, no allocation while the World does not grow."""
        arr = world.array()
        if world.needs_area_entries():
            _check(lib().rtc_world_update_area_lights(self.ctx._h, self._h, arr, len(world.shapes), world.area_light_array(), len(world.lights)),
                   "rtc_world_update_area_lights")
        else:
            _check(lib().rtc_world_update_lights(self.ctx._h, self._h, arr, len(world.shapes), world.light_array(), len(world.lights)),
                   "rtc_world_update_lights")
        self.n = len(world.shapes)

    def close(self):
        if self._h:
            lib().rtc_world_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, cam: RtcCamera, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False,
               out: np.ndarray | None = None):
        """Camera::render(&World) -> Canvas as a (vsize, hsize, 3) float64 array (host). `out` = a
        canvas to reuse, e.g. one from host_canvas() (page-locked: the copy runs at link speed)."""
        if out is None:
            out = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        elif out.shape != (cam.vsize, cam.hsize, 3) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (vsize, hsize, 3) float64 array")
        st = RtcStats()
        _check(lib().rtc_render(self.ctx._h, self._h, C.byref(cam), mode, flags, out.ctypes.data_as(C.POINTER(C.c_double)),
                                C.byref(st) if with_stats else None), "rtc_render")
        if with_stats:
            return out, _stats_dict(st, cam.samples != 1)
        return out

    def render_rgb8(self, cam: RtcCamera, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False,
                    out: np.ndarray | None = None):
        """Camera::render for a caller that only writes the image: the (vsize, hsize, 3) uint8 frame of
        Color::scale(c, 255), quantised on the device — 3 bytes per pixel cross PCIe (rtc_render_rgb8)."""
        if out is None:
            out = np.empty((cam.vsize, cam.hsize, 3), dtype=np.uint8)
        elif out.shape != (cam.vsize, cam.hsize, 3) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (vsize, hsize, 3) uint8 array")
        st = RtcStats()
        _check(lib().rtc_render_rgb8(self.ctx._h, self._h, C.byref(cam), mode, flags, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     C.byref(st) if with_stats else None), "rtc_render_rgb8")
        if with_stats:
            return out, _stats_dict(st, cam.samples != 1)
        return out

    def render_lens(self, cam: RtcCamera, lens: RtcLens, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False,
                    out: np.ndarray | None = None, rgb8: bool = False):
        """render() through a thin lens (rtc.lens): every pixel is the mean of usteps x vsteps rays from the lens to the
        pixel's point on the plane in focus — depth of field (rtc_render_lens; rgb8=True: rtc_render_lens_rgb8's uint8 frame)."""
        dtype = np.uint8 if rgb8 else np.float64
        if out is None:
            out = np.empty((cam.vsize, cam.hsize, 3), dtype=dtype)
        elif out.shape != (cam.vsize, cam.hsize, 3) or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (vsize, hsize, 3) array of float64 (uint8 with rgb8)")
        st = RtcStats()
        fn, name = (lib().rtc_render_lens_rgb8, "rtc_render_lens_rgb8") if rgb8 else (lib().rtc_render_lens, "rtc_render_lens")
        _check(fn(self.ctx._h, self._h, C.byref(cam), C.byref(lens), mode, flags, out.ctypes.data_as(C.POINTER(C.c_uint8 if rgb8 else C.c_double)),
                  C.byref(st) if with_stats else None), name)
        if with_stats:
            d = _stats_dict(st)
            d["rays_primary_proven_miss"] = st.rays_primary_proven_miss   # 0: no black proof applies when the origin moves
            return out, d
        return out

    def render_lens_rows(self, cam: RtcCamera, lens: RtcLens, y0: int, y1: int, d_ptr: int | None, mode: int = MODE_RENDER_ASYNC,
                         flags: int = 0, d_ptr8: int | None = None) -> None:
        """render_rows through a thin lens: rows [y0, y1) into the DEVICE buffer at `d_ptr` (rtc_render_lens_rows)."""
        st = lib().rtc_render_lens_rows(self.ctx._h, self._h, C.byref(cam), C.byref(lens), mode, y0, y1, d_ptr, d_ptr8, flags)
        if st != 0:
            raise RtcError(st, "rtc_render_lens_rows")

    def render_projection(self, cam: RtcCamera, proj: RtcProjection, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False,
                          out: np.ndarray | None = None, rgb8: bool = False):
        """render() with the rays of an orthographic or panorama camera (rtc.projection) instead of the pinhole's; cam gives
        the size and the view (rtc_render_projection; rgb8=True: rtc_render_projection_rgb8's uint8 frame)."""
        dtype = np.uint8 if rgb8 else np.float64
        if out is None:
            out = np.empty((cam.vsize, cam.hsize, 3), dtype=dtype)
        elif out.shape != (cam.vsize, cam.hsize, 3) or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (vsize, hsize, 3) array of float64 (uint8 with rgb8)")
        st = RtcStats()
        fn, name = (lib().rtc_render_projection_rgb8, "rtc_render_projection_rgb8") if rgb8 else (lib().rtc_render_projection, "rtc_render_projection")
        _check(fn(self.ctx._h, self._h, C.byref(cam), C.byref(proj), mode, flags, out.ctypes.data_as(C.POINTER(C.c_uint8 if rgb8 else C.c_double)),
                  C.byref(st) if with_stats else None), name)
        if with_stats:
            d = _stats_dict(st)
            d["rays_primary_proven_miss"] = st.rays_primary_proven_miss   # 0: the black proof is for pinhole rays
            return out, d
        return out

    def render_projection_rows(self, cam: RtcCamera, proj: RtcProjection, y0: int, y1: int, d_ptr: int | None, mode: int = MODE_RENDER_ASYNC,
                               flags: int = 0, d_ptr8: int | None = None) -> None:
        """render_rows with a projection's rays: rows [y0, y1) into the DEVICE buffer at `d_ptr` (rtc_render_projection_rows)."""
        st = lib().rtc_render_projection_rows(self.ctx._h, self._h, C.byref(cam), C.byref(proj), mode, y0, y1, d_ptr, d_ptr8, flags)
        if st != 0:
            raise RtcError(st, "rtc_render_projection_rows")

    def render_rgba8(self, cam: RtcCamera, gamma: float = 1.0, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False,
                     out: np.ndarray | None = None):
        """Camera::render + Canvas::set_gamma(gamma) + to_imgbuf: the (vsize, hsize, 4) uint8 RGBA frame, quantised on the
        device — 4 bytes per pixel cross PCIe (rtc_render_rgba8). `out` as for render_rgb8 (host_canvas_rgba8: page-locked)."""
        if out is None:
            out = np.empty((cam.vsize, cam.hsize, 4), dtype=np.uint8)
        elif out.shape != (cam.vsize, cam.hsize, 4) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (vsize, hsize, 4) uint8 array")
        st = RtcStats()
        _check(lib().rtc_render_rgba8(self.ctx._h, self._h, C.byref(cam), mode, flags, gamma, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                      C.byref(st) if with_stats else None), "rtc_render_rgba8")
        if with_stats:
            return out, _stats_dict(st, cam.samples != 1)
        return out

    def render_views_rgba8(self, cams, first_band: int, band_stride: int, d_ptr: int, view_rows: int, gamma: float = 1.0,
                           mode: int = MODE_RENDER_ASYNC, flags: int = 0) -> None:
        """render_views with to_imgbuf's RGBA at `gamma` as the only output: DEVICE buffer `d_ptr`, 4 bytes per pixel
        (rtc_render_views_rgba8)."""
        arr = cams if isinstance(cams, C.Array) else (RtcCamera * len(cams))(*cams)
        st = lib().rtc_render_views_rgba8(self.ctx._h, self._h, arr, len(arr), mode, first_band, band_stride, gamma, d_ptr, view_rows, flags)
        if st != 0:
            raise RtcError(st, "rtc_render_views_rgba8")

    def render_rows(self, cam: RtcCamera, y0: int, y1: int, d_ptr: int, mode: int = MODE_RENDER_ASYNC, flags: int = 0,
                    d_ptr8: int | None = None) -> None:
        """Enqueue rows [y0, y1) into the DEVICE buffer at address `d_ptr` (no synchronisation);
        `d_ptr8` optionally receives the rows quantised to 8 bits (Color::scale)."""
        st = _render_rows()(self.ctx._h, self._h, cam, mode, y0, y1, d_ptr, d_ptr8, flags)  # launch path: no temporaries
        if st != 0:
            raise RtcError(st, "rtc_render_rows")

    def render_bands(self, cam: RtcCamera, first_band: int, band_stride: int, d_ptr: int, mode: int = MODE_RENDER_ASYNC,
                     flags: int = 0, d_ptr8: int | None = None) -> None:
        """Enqueue the 8-row bands first_band, first_band + band_stride, ... packed one after the
        other into the DEVICE buffer at `d_ptr` (interleaved row tiles, include/rtc.h)."""
        st = _render_bands()(self.ctx._h, self._h, cam, mode, first_band, band_stride, d_ptr, d_ptr8, flags)
        if st != 0:
            raise RtcError(st, "rtc_render_bands")

    def render_views(self, cams, first_band: int, band_stride: int, d_ptr: int, view_rows: int, mode: int = MODE_RENDER_ASYNC,
                     flags: int = 0, d_ptr8: int | None = None) -> None:
        """Enqueue ONE launch that renders every camera of `cams` (a list of RtcCamera, or a prebuilt
        ctypes array of them) onto this World; view v lands `v * view_rows` rows below view 0
        (rtc_render_views, include/rtc.h)."""
        arr = cams if isinstance(cams, C.Array) else (RtcCamera * len(cams))(*cams)
        st = lib().rtc_render_views(self.ctx._h, self._h, arr, len(arr), mode, first_band, band_stride, d_ptr, d_ptr8, view_rows, flags)
        if st != 0:
            raise RtcError(st, "rtc_render_views")

    def _tile_pass(self, entry: str, cam: RtcCamera, projection, *rest) -> None:
        """rtc_render_<entry>(ctx, world, cam, ...), or with `projection` (an RtcProjection: the orthographic or panorama
        camera's rays in place of the pinhole's centre rays) rtc_render_<entry with _projection>(ctx, world, cam, proj, ...)."""
        if projection is None:
            _check(getattr(lib(), "rtc_render_" + entry)(self.ctx._h, self._h, C.byref(cam), *rest), "rtc_render_" + entry)
            return
        head, dev, _ = entry.partition("_device")
        name = "rtc_render_" + head + "_projection" + dev
        _check(getattr(lib(), name)(self.ctx._h, self._h, C.byref(cam), C.byref(projection), *rest), name)

    def render_aov(self, cam: RtcCamera, planes=("index", "depth", "point", "normal", "flags", "shadow"), mode: int = MODE_RENDER_ASYNC,
                   flags: int = 0, projection: RtcProjection | None = None) -> dict:
        """What each pixel's centre ray saw (rtc_render_aov): {plane: array} for the planes asked for — index int32 (H, W),
        depth float64 (H, W), point / normal float64 (H, W, 3), flags uint8 (H, W), shadow uint16 (H, W). A plane that is
        not named is neither computed nor copied; without "shadow" no shadow ray is cast. With `projection` the pixel's ray
        is that camera's (rtc_render_aov_projection); so for the five passes below."""
        out = _aov_arrays(planes, cam.vsize, cam.hsize)
        b = _aov_host_buffers(out)
        self._tile_pass("aov", cam, projection, mode, flags, C.byref(b))
        return out

    def render_aov_device(self, cam: RtcCamera, pointers: dict, mode: int = MODE_RENDER_ASYNC, flags: int = 0,
                          projection: RtcProjection | None = None) -> None:
        """The same into DEVICE buffers ({plane: address}; rtc_render_aov_device): enqueued on the context's stream."""
        b = _aov_buffers(pointers)
        self._tile_pass("aov_device", cam, projection, mode, flags, C.byref(b))

    def render_ao(self, cam: RtcCamera, ao: RtcAo, mode: int = MODE_RENDER_ASYNC, flags: int = 0, projection: RtcProjection | None = None) -> np.ndarray:
        """The ambient-occlusion plane (rtc_render_ao): a (vsize, hsize) uint16 array, per pixel the number of the pass's
        samples that meet something within its radius; 0 where the centre ray misses."""
        out = np.empty((cam.vsize, cam.hsize), dtype=np.uint16)
        self._tile_pass("ao", cam, projection, C.byref(ao), mode, flags, out.ctypes.data_as(C.POINTER(C.c_uint16)))
        return out

    def render_ao_device(self, cam: RtcCamera, ao: RtcAo, d_ao: int, mode: int = MODE_RENDER_ASYNC, flags: int = 0,
                         projection: RtcProjection | None = None) -> None:
        """The same into a DEVICE buffer of vsize * hsize uint16 (rtc_render_ao_device): enqueued on the context's stream."""
        self._tile_pass("ao_device", cam, projection, C.byref(ao), mode, flags, C.c_void_p(d_ao))

    def render_gather(self, cam: RtcCamera, ao: RtcAo, mode: int = MODE_RENDER_ASYNC, flags: int = 0, planes=("radiance", "bounce"),
                      projection: RtcProjection | None = None) -> dict:
        """The one-bounce gather pass (rtc_render_gather): {"radiance": (vsize, hsize, 3), "bounce": (vsize, hsize, 3)} f64 for
        the planes asked for — the mean colour the fan `ao` sees from the centre ray's hit within its radius, and that mean
        times the hit's own base colour and diffuse coefficient, ready for add_scaled. Zeros where the centre ray misses."""
        out = {name: np.empty((cam.vsize, cam.hsize, 3)) for name in planes}
        b = RtcGatherBuffers(**{name: a.ctypes.data for name, a in out.items()})
        self._tile_pass("gather", cam, projection, C.byref(ao), mode, flags, C.byref(b))
        return out

    def render_adaptive(self, cam: RtcCamera, spec: RtcAdaptive, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_mask: bool = False,
                        with_stats: bool = False):
        """The edge-adaptively anti-aliased frame (rtc_render_adaptive; rtc.adaptive makes `spec`): the one-sample frame with
        every pixel whose 4-neighbourhood has contrast replaced by the mean of usteps x vsteps sub-samples.
        -> (frame (vsize, hsize, 3) float64, info dict {pixels_refined, rays_refined, launches}), then the (vsize, hsize) uint8
        mask with `with_mask` and the rtc_stats dict with `with_stats`."""
        out = np.empty((cam.vsize, cam.hsize, 3), dtype=np.float64)
        mask = np.empty((cam.vsize, cam.hsize), dtype=np.uint8) if with_mask else None
        info, st = RtcAdaptiveInfo(), RtcStats()
        _check(lib().rtc_render_adaptive(self.ctx._h, self._h, C.byref(cam), C.byref(spec), mode, flags, out.ctypes.data_as(C.POINTER(C.c_double)),
                                         mask.ctypes.data_as(C.POINTER(C.c_uint8)) if with_mask else None, C.byref(info),
                                         C.byref(st) if with_stats else None), "rtc_render_adaptive")
        res = [out, _adaptive_info_dict(info)]
        if with_mask:
            res.append(mask)
        if with_stats:
            res.append(_stats_dict(st))
        return tuple(res)

    def render_adaptive_device(self, cam: RtcCamera, spec: RtcAdaptive, d_rgb: int, d_mask: int | None = None, mode: int = MODE_RENDER_ASYNC,
                               flags: int = 0) -> dict:
        """render_adaptive into the DEVICE canvas `d_rgb` (vsize*hsize*3 doubles) and, when given, the device mask `d_mask`
        (vsize*hsize bytes), on the context's stream (rtc_render_adaptive_device): waits once, for the number of flagged pixels,
        and returns the info dict with the refinement enqueued."""
        info = RtcAdaptiveInfo()
        _check(lib().rtc_render_adaptive_device(self.ctx._h, self._h, C.byref(cam), C.byref(spec), mode, flags, C.c_void_p(d_rgb),
                                                C.c_void_p(d_mask) if d_mask else None, C.byref(info)), "rtc_render_adaptive_device")
        return _adaptive_info_dict(info)

    def render_gather_device(self, cam: RtcCamera, ao: RtcAo, pointers: dict, mode: int = MODE_RENDER_ASYNC, flags: int = 0,
                             projection: RtcProjection | None = None) -> None:
        """The same into DEVICE buffers of vsize * hsize * 3 doubles, {"radiance": pointer, "bounce": pointer} with either left
        out (rtc_render_gather_device): enqueued on the context's stream."""
        b = RtcGatherBuffers(**{name: int(p) for name, p in pointers.items()})
        self._tile_pass("gather_device", cam, projection, C.byref(ao), mode, flags, C.byref(b))

    def color_at(self, rays: np.ndarray, remaining: int = 5, want_hits: bool = False, flags: int = 0):
        """World::color_at for an (n, 6) array of rays; returns rgb (n,3) [and the rtc_hit array]."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = r.shape[0]
        rgb = np.empty((n, 3), dtype=np.float64)
        hits = (RtcHit * max(1, n))() if want_hits else None
        P = C.POINTER(C.c_double)
        _check(lib().rtc_color_at(self.ctx._h, self._h, r.ctypes.data_as(P), n, remaining, flags, rgb.ctypes.data_as(P), hits), "rtc_color_at")
        return (rgb, hits) if want_hits else rgb


class _Encoder:
    """What the device encoders share: an rtc_<kind>_* object bound to a context (closed with it), its file's bytes."""
    _kind = ""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()
        _check(self._fn("create")(ctx._h, C.byref(self._h)), f"rtc_{self._kind}_create")
        ctx._worlds.append(weakref.ref(self))   # closed with the context

    def _fn(self, name: str):
        return getattr(lib(), f"rtc_{self._kind}_{name}")

    def bytes(self) -> bytes:
        need = self._fn("bytes")(self._h, None, 0)
        if need == 0:
            return b""
        buf = np.empty(need, dtype=np.uint8)
        self._fn("bytes")(self._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), need)
        return buf.tobytes()

    def write(self, path) -> None:
        _check(self._fn("write")(self._h, str(path).encode()), f"rtc_{self._kind}_write")

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GifWriter(_Encoder):
    """An animated GIF encoded on the GPU (rtc_gif_writer): frames already in device memory or rendered straight into the
    writer; only each frame's compressed record crosses PCIe. The bytes equal gif_encode's for the same frames."""
    _kind = "gif_writer"

    def append_device(self, d_ptr: int, width: int, height: int) -> None:
        """Append the height x width x 3 uint8 frame at device address d_ptr (enqueued on the context's stream)."""
        _check(lib().rtc_gif_writer_append_device(self._h, C.c_void_p(d_ptr), width, height), "rtc_gif_writer_append_device")

    def render(self, world: "DeviceWorld", cam: RtcCamera, mode: int = MODE_RENDER_ASYNC, flags: int = 0) -> None:
        """Render `cam` on the device and append the frame without copying it to the host."""
        _check(lib().rtc_gif_writer_render(self._h, world._h, C.byref(cam), mode, flags), "rtc_gif_writer_render")


class JpegEncoder(_Encoder):
    """A JPEG encoder on the GPU (rtc_jpeg_encoder): frames already in device memory or rendered straight into the encoder;
    only the finished file crosses PCIe. The bytes equal jpeg_encode's for the same pixels."""
    _kind = "jpeg_encoder"

    def encode_device(self, d_ptr: int, width: int, height: int, channels: int = 3, quality: int = 75) -> bytes:
        """Encode the height x width x channels uint8 frame at device address d_ptr (enqueued on the context's stream)."""
        _check(lib().rtc_jpeg_encoder_encode_device(self._h, C.c_void_p(d_ptr), width, height, channels, quality),
               "rtc_jpeg_encoder_encode_device")
        return self.bytes()

    def render(self, world: "DeviceWorld", cam: RtcCamera, gamma: float = 1.0, quality: int = 75, mode: int = MODE_RENDER_ASYNC,
               flags: int = 0) -> bytes:
        """Camera::render + set_gamma(gamma) + write_to_file("x.jpg"), the frame never leaving the device."""
        _check(lib().rtc_jpeg_encoder_render(self._h, world._h, C.byref(cam), mode, flags, gamma, quality), "rtc_jpeg_encoder_render")
        return self.bytes()


class PngEncoder(_Encoder):
    """A compressed PNG encoder on the GPU (rtc_png_encoder): frames already in device memory or rendered straight into the
    encoder; only the finished file crosses PCIe. The bytes equal png_encode's for the same pixels."""
    _kind = "png_encoder"

    def encode_device(self, d_ptr: int, width: int, height: int, channels: int = 3) -> bytes:
        """Encode the height x width x channels uint8 frame at device address d_ptr (enqueued on the context's stream)."""
        _check(lib().rtc_png_encoder_encode_device(self._h, C.c_void_p(d_ptr), width, height, channels), "rtc_png_encoder_encode_device")
        return self.bytes()

    def render(self, world: "DeviceWorld", cam: RtcCamera, gamma: float = 1.0, mode: int = MODE_RENDER_ASYNC, flags: int = 0) -> bytes:
        """Camera::render + set_gamma(gamma) + write_to_file("x.png"), the frame never leaving the device."""
        _check(lib().rtc_png_encoder_render(self._h, world._h, C.byref(cam), mode, flags, gamma), "rtc_png_encoder_render")
        return self.bytes()


class ImageEncoder(_Encoder):
    """The save-by-name encoder on the GPU (rtc_image_encoder): frames already in device memory or rendered straight into
    the encoder, any format of the save table; only the finished file crosses PCIe. The bytes equal image_encode's."""
    _kind = "image_encoder"

    def encode_device(self, fmt, d_ptr: int, width: int, height: int, channels: int = 3) -> bytes:
        """Encode the height x width x channels uint8 frame at device address d_ptr as `fmt` (on the context's stream)."""
        _check(lib().rtc_image_encoder_encode_device(self._h, _image_format(fmt), C.c_void_p(d_ptr), width, height, channels),
               "rtc_image_encoder_encode_device", f"format {fmt}, {width}x{height}x{channels}")
        return self.bytes()

    def render(self, fmt, world: "DeviceWorld", cam: RtcCamera, gamma: float = 1.0, mode: int = MODE_RENDER_ASYNC, flags: int = 0) -> bytes:
        """Camera::render + set_gamma(gamma) + write_to_file(name of format `fmt`), the frame never leaving the device."""
        _check(lib().rtc_image_encoder_render(self._h, _image_format(fmt), world._h, C.byref(cam), mode, flags, gamma),
               "rtc_image_encoder_render", f"format {fmt}")
        return self.bytes()


class FloatEncoder(_Encoder):
    """The float file writers on the GPU (rtc_float_encoder): Radiance HDR, PFM and OpenEXR of an f64 canvas (and, for EXR,
    AOV planes) already in device memory, or of a frame rendered straight into the encoder; only the finished file crosses
    PCIe. The bytes equal float_encode's."""
    _kind = "float_encoder"

    def encode_device(self, fmt, d_rgb: int | None, width: int, height: int, pointers: dict | None = None, rgb_type="half") -> bytes:
        """Encode the height x width x 3 float64 canvas at device address d_rgb (None: an EXR of planes only) and the AOV
        planes at `pointers` ({plane: device address}, EXR) as `fmt`, on the context's stream."""
        p = _float_planes(d_rgb, pointers, rgb_type)
        _check(lib().rtc_float_encoder_encode_device(self._h, _float_format(fmt), C.byref(p), width, height),
               "rtc_float_encoder_encode_device", f"format {fmt}, {width}x{height}")
        return self.bytes()

    def render(self, fmt, world: "DeviceWorld", cam: RtcCamera, lens: RtcLens | None = None, rgb_type="half", mode: int = MODE_RENDER_ASYNC,
               flags: int = 0) -> bytes:
        """Camera::render (through `lens` when given) + save under a name of format `fmt`, the f64 canvas never leaving the
        device."""
        t = EXR_TYPES[rgb_type] if isinstance(rgb_type, str) else int(rgb_type)
        _check(lib().rtc_float_encoder_render_lens(self._h, _float_format(fmt), world._h, C.byref(cam), C.byref(lens) if lens is not None else None,
                                                   mode, flags, t), "rtc_float_encoder_render", f"format {fmt}")
        return self.bytes()


class Shutter(_Encoder):
    """Motion blur on the GPU (rtc_shutter, include/rtc.h): a frame is Color::average_over of `samples` ordinary frames of
    the World at the shutter's cell centres, rendered back to back on the device and averaged by one kernel; only the mean,
    or its 8-bit form, crosses PCIe. `motions` is a list of rtc.motion records (or None), `cam_close` the camera at the
    shutter's close (None: the camera stands still), `lens` a thin lens (rtc.lens; cam.samples must then be 1). The shutter
    keeps a World of its own: `world` is the host-side World, and no DeviceWorld of the caller is touched."""
    _kind = "shutter"
    bytes = write = None   # a shutter delivers frames, not a file

    def _scene(self, world: World, motions, cam: RtcCamera, samples: int, cam_close, lens):
        sc = RtcShutterScene()
        shapes, lights = world.array(), world.area_light_array()
        marr, nm = _motion_array(motions)
        sc.shapes, sc.n_shapes = shapes, len(world.shapes)
        sc.motions, sc.n_motions = marr, nm
        sc.lights, sc.n_lights = lights, len(world.lights)
        sc.cam_open = C.pointer(cam)
        if cam_close is not None:
            sc.cam_close = C.pointer(cam_close)
        if lens is not None:
            sc.lens = C.pointer(lens)
        sc.samples = int(samples)
        return sc, (shapes, lights, marr)   # the arrays the scene points into

    def _host(self, entry: str, shape, dtype, scene_args, mode, flags, with_stats, out, extra=()):
        cam = scene_args[2]
        if out is None:
            out = np.empty((cam.vsize, cam.hsize) + shape, dtype=dtype)
        elif out.shape != (cam.vsize, cam.hsize) + shape or out.dtype != dtype or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous (vsize, hsize, {shape[0]}) {np.dtype(dtype).name} array")
        sc, _keep = self._scene(*scene_args)
        st = RtcStats()
        ptr = out.ctypes.data_as(C.POINTER(C.c_double if dtype == np.float64 else C.c_uint8))
        _check(getattr(lib(), entry)(self._h, C.byref(sc), mode, flags, *extra, ptr, C.byref(st) if with_stats else None), entry)
        if with_stats:
            d = _stats_dict(st, True)
            d["rays_primary_proven_miss"] = st.rays_primary_proven_miss
            return out, d
        return out

    def render(self, world: World, motions, cam: RtcCamera, samples: int, cam_close=None, lens=None, mode: int = MODE_RENDER_ASYNC,
               flags: int = 0, with_stats: bool = False, out: np.ndarray | None = None):
        """The motion-blurred frame as a (vsize, hsize, 3) float64 array (rtc_shutter_render). Stats are the sums over the
        sub-frames."""
        return self._host("rtc_shutter_render", (3,), np.float64, (world, motions, cam, samples, cam_close, lens), mode, flags, with_stats, out)

    def render_rgb8(self, world: World, motions, cam: RtcCamera, samples: int, cam_close=None, lens=None, mode: int = MODE_RENDER_ASYNC,
                    flags: int = 0, with_stats: bool = False, out: np.ndarray | None = None):
        """Color::scale of the mean, (vsize, hsize, 3) uint8, quantised on the device (rtc_shutter_render_rgb8)."""
        return self._host("rtc_shutter_render_rgb8", (3,), np.uint8, (world, motions, cam, samples, cam_close, lens), mode, flags, with_stats, out)

    def render_rgba8(self, world: World, motions, cam: RtcCamera, samples: int, gamma: float = 1.0, cam_close=None, lens=None,
                     mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False, out: np.ndarray | None = None):
        """to_imgbuf of the mean at `gamma`, (vsize, hsize, 4) uint8 (rtc_shutter_render_rgba8)."""
        return self._host("rtc_shutter_render_rgba8", (4,), np.uint8, (world, motions, cam, samples, cam_close, lens), mode, flags, with_stats, out,
                          extra=(C.c_float(gamma),))

    def render_device(self, world: World, motions, cam: RtcCamera, samples: int, d_rgb: int | None = None, d_rgb8: int | None = None,
                      d_rgba8: int | None = None, gamma: float = 1.0, cam_close=None, lens=None, mode: int = MODE_RENDER_ASYNC,
                      flags: int = 0) -> None:
        """The frame into DEVICE buffers, any non-empty subset of the f64 mean (`d_rgb`), Color::scale's bytes (`d_rgb8`) and
        to_imgbuf's RGBA at `gamma` (`d_rgba8`); ordered on the context's stream, no host wait (rtc_shutter_render_device)."""
        sc, _keep = self._scene(world, motions, cam, samples, cam_close, lens)
        _check(lib().rtc_shutter_render_device(self._h, C.byref(sc), mode, flags, gamma, d_rgb, d_rgb8, d_rgba8), "rtc_shutter_render_device")


def host_canvas_rgb8(vsize: int, hsize: int) -> np.ndarray:
    """A zeroed (vsize, hsize, 3) uint8 frame in page-locked memory (rtc_host_alloc)."""
    arr = np.frombuffer(_Pinned(vsize * hsize * 3).buf, dtype=np.uint8).reshape(vsize, hsize, 3)
    arr[...] = 0
    return arr


def host_canvas_rgba8(vsize: int, hsize: int) -> np.ndarray:
    """A zeroed (vsize, hsize, 4) uint8 frame in page-locked memory (rtc_host_alloc), for render_rgba8's `out`."""
    arr = np.frombuffer(_Pinned(vsize * hsize * 4).buf, dtype=np.uint8).reshape(vsize, hsize, 4)
    arr[...] = 0
    return arr


def host_register(arr: np.ndarray) -> None:
    """rtc_host_register: page-lock a canvas the caller allocated (a Vec<Color> on the Rust side)."""
    _check(lib().rtc_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes), "rtc_host_register")


def host_unregister(arr: np.ndarray) -> None:
    _check(lib().rtc_host_unregister(C.c_void_p(arr.ctypes.data)), "rtc_host_unregister")


def group_unique_id() -> bytes:
    """ncclGetUniqueId through the C-ABI (rank 0 calls it and ships the 128 bytes to the other ranks)."""
    buf = (C.c_uint8 * GROUP_ID_BYTES)()
    _check(lib().rtc_group_unique_id(buf), "rtc_group_unique_id", "RCCL not loadable")
    return bytes(buf)


class Group:
    """N GPUs rendering one frame together (rtc_group): 8-row bands dealt round-robin, RCCL gather of the
    f64 tiles to member 0, un-deal on member 0's device. Group(devices=[...]) drives all devices from this
    process; Group(device=d, nranks=N, rank=r, uid=...) is one member of a one-process-per-GPU group."""

    def __init__(self, devices=None, exchange: int = EXCHANGE_RCCL, device: int | None = None, nranks: int | None = None,
                 rank: int | None = None, uid: bytes | None = None):
        self._h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*devices)
            _check(lib().rtc_group_create(arr, len(devices), exchange, C.byref(self._h)), "rtc_group_create")
        else:
            idb = (C.c_uint8 * GROUP_ID_BYTES)(*uid)
            _check(lib().rtc_group_create_rank(device, nranks, rank, idb, C.byref(self._h)), "rtc_group_create_rank")
        self.size = lib().rtc_group_size(self._h)
        self.local_size = lib().rtc_group_local_size(self._h)
        self.contexts = []
        for i in range(self.local_size):   # member i's context, on member i's device (in-process: devices[i]; rank mode: device)
            ptr = lib().rtc_group_context(self._h, i)
            if not ptr:
                raise RtcError(4, "rtc_group_context", f"member {i} has no context")
            self.contexts.append(Context(device=(devices[i] if devices is not None else device), _borrowed=ptr))
        self._worlds = []

    def close(self):
        if self._h:
            for ref in self._worlds:
                w = ref()
                if w is not None:
                    w.close()
            self._worlds = []
            for c in self.contexts:
                c.close()
            lib().rtc_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().rtc_group_synchronize(self._h), "rtc_group_synchronize")

    def upload(self, world: World) -> "GroupWorld":
        return GroupWorld(self, world)

    def stats(self) -> dict:
        s = RtcStats()
        _check(lib().rtc_group_stats_read(self._h, C.byref(s)), "rtc_group_stats_read")
        return _stats_dict(s)

    def reset_stats(self):
        _check(lib().rtc_group_stats_reset(self._h), "rtc_group_stats_reset")


class GroupWorld:
    """World replicated on every local member of a Group (rtc_group_world)."""

    def __init__(self, group: Group, world: World):
        self.group = group
        self._h = C.c_void_p()
        if not isinstance(world.light, RtcLight):
            raise ValueError("group worlds are lit by a single point light: world.light is an area light (rtc_group_world_* stays single-light)")
        _check(lib().rtc_group_world_create(group._h, world.array(), len(world.shapes), C.byref(world.light), C.byref(self._h)),
               "rtc_group_world_create")
        group._worlds.append(weakref.ref(self))

    def close(self):
        if self._h:
            lib().rtc_group_world_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render(self, cams, what: int = GATHER_F64, d_canvas: int | None = None, d_rgb8: int | None = None,
               mode: int = MODE_RENDER_ASYNC, flags: int = 0) -> None:
        """Enqueue one batch (<= 8 cameras of one size): every member renders its bands, the tiles are gathered to
        member 0 and un-dealt into `d_canvas` (DEVICE address on member 0's device; frames back to back)."""
        arr = cams if isinstance(cams, C.Array) else (RtcCamera * len(cams))(*cams)
        st = lib().rtc_group_render(self.group._h, self._h, arr, len(arr), mode, flags, what, d_canvas, d_rgb8)
        if st != 0:
            raise RtcError(st, "rtc_group_render")

    def render_host(self, cam: RtcCamera, out: np.ndarray, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False):
        """Camera::render_async -> host Canvas: every local member DMAs its bands straight into `out`."""
        if out.shape != (cam.vsize, cam.hsize, 3) or out.dtype != np.float64 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (vsize, hsize, 3) float64 array")
        st = RtcStats()
        _check(lib().rtc_group_render_host(self.group._h, self._h, C.byref(cam), mode, flags, out.ctypes.data_as(C.POINTER(C.c_double)),
                                           C.byref(st) if with_stats else None), "rtc_group_render_host")
        return (out, _stats_dict(st, cam.samples != 1)) if with_stats else out

    def render_host_rgb8(self, cam: RtcCamera, out: np.ndarray, mode: int = MODE_RENDER_ASYNC, flags: int = 0, with_stats: bool = False):
        """The same for the 8-bit frame (Color::scale'd on the device; rtc_group_render_host_rgb8)."""
        if out.shape != (cam.vsize, cam.hsize, 3) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (vsize, hsize, 3) uint8 array")
        st = RtcStats()
        _check(lib().rtc_group_render_host_rgb8(self.group._h, self._h, C.byref(cam), mode, flags, out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                C.byref(st) if with_stats else None), "rtc_group_render_host_rgb8")
        return (out, _stats_dict(st, cam.samples != 1)) if with_stats else out

    def render_host_rgba8(self, cam: RtcCamera, out: np.ndarray, gamma: float = 1.0, mode: int = MODE_RENDER_ASYNC, flags: int = 0,
                          with_stats: bool = False):
        """The same for to_imgbuf's RGBA at `gamma` ((vsize, hsize, 4) uint8; rtc_group_render_host_rgba8)."""
        if out.shape != (cam.vsize, cam.hsize, 4) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (vsize, hsize, 4) uint8 array")
        st = RtcStats()
        _check(lib().rtc_group_render_host_rgba8(self.group._h, self._h, C.byref(cam), mode, flags, gamma,
                                                 out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st) if with_stats else None),
               "rtc_group_render_host_rgba8")
        return (out, _stats_dict(st, cam.samples != 1)) if with_stats else out


# ---- [host] the dealing of rows over the members of a group (csrc/rtc_bands.h through the C-ABI) ------------------
def group_packed_rows(vsize: int, nranks: int) -> int:
    return lib().rtc_group_packed_rows(vsize, nranks)


def group_bands_owned(vsize: int, nranks: int, rank: int) -> int:
    return lib().rtc_group_bands_owned(vsize, nranks, rank)


def group_row_owner(y: int, nranks: int) -> tuple[int, int]:
    m, r = C.c_uint32(), C.c_uint32()
    lib().rtc_group_row_owner(y, nranks, C.byref(m), C.byref(r))
    return m.value, r.value


def group_packed_row_to_image(member: int, packed_row: int, nranks: int) -> int:
    return lib().rtc_group_packed_row_to_image(member, packed_row, nranks)


def group_undeal_host(staging: np.ndarray, nranks: int, nframes: int, vsize: int) -> np.ndarray:
    """Member 0's un-deal step on host memory: `staging` = (nranks, nframes, packed_rows, ...row) in rank order
    (what the gather delivers) -> (nframes, vsize, ...row)."""
    st = np.ascontiguousarray(staging)
    rows = group_packed_rows(vsize, nranks)
    assert st.shape[:3] == (nranks, nframes, rows), (st.shape, (nranks, nframes, rows))
    row_bytes = int(np.prod(st.shape[3:], dtype=np.int64)) * st.itemsize
    out = np.empty((nframes, vsize) + st.shape[3:], dtype=st.dtype)
    _check(lib().rtc_group_undeal_host(C.c_void_p(st.ctypes.data), C.c_void_p(out.ctypes.data), nranks, nframes, vsize, row_bytes),
           "rtc_group_undeal_host")
    return out


__all__ = ["lib", "RtcError", "Matrix", "material", "sphere", "plane", "cube", "light", "area_light", "World", "camera", "ray_for_pixel", "lens", "lens_ray", "ao", "ao_expand", "ao_ray", "ao_from_hits", "apply_ao", "load_yaml_ao", "RtcAo", "MAX_AO_SAMPLES", "gather_from_hits", "add_scaled", "load_yaml_gather", "RtcGatherBuffers", "tonemap_spec", "bloom_spec", "luminance", "tonemap_resolve", "tonemap", "bloom", "bloom_weights", "load_yaml_post", "resize_spec", "resize_weights", "resize", "load_yaml_resize", "RtcResize", "RESIZE_BOX", "RESIZE_TRIANGLE", "RESIZE_CATMULL_ROM", "RESIZE_MITCHELL", "RESIZE_LANCZOS3", "MAX_RESIZE_TAPS", "RtcLuminance", "RtcTonemap", "RtcBloom", "TONEMAP_LINEAR", "TONEMAP_REINHARD", "TONEMAP_ACES", "TONEMAP_AUTO_EXPOSURE", "TONEMAP_AUTO_WHITE", "MAX_BLOOM_RADIUS", "adaptive", "adaptive_offset", "adaptive_mask", "load_yaml_adaptive", "RtcAdaptive", "RtcAdaptiveInfo", "MAX_AA_SAMPLES", "AA_DEFAULT_THRESHOLD", "AA_DEFAULT_STEPS", "AA_DEFAULT_MAX_RAYS", "filter_spec", "plane_filter", "counts_to_fraction", "apply_occlusion", "load_yaml_filter", "RtcFilter", "FILTER_SAME_OBJECT", "MAX_FILTER_PASSES", "FILTER_DEFAULT_PLANE_SIGMA", "FILTER_DEFAULT_PASSES", "FILTER_DEFAULT_NORMAL_SQUARINGS", "projection", "projection_ray", "projection_tables", "PROJ_ORTHOGRAPHIC", "PROJ_PANORAMA", "motion", "shutter_time", "shutter_shapes", "shutter_camera", "canvas_average", "Shutter",
           "load_yaml", "load_yaml_lens", "load_yaml_projection", "load_yaml_projection_passes", "load_yaml_motion", "load_lua", "LuaProgram", "LuaJob", "format_ppm", "write_ppm", "format_png", "write_png", "color_scale255", "to_rgba8", "gamma_thresholds", "Context", "DeviceWorld", "MODE_RENDER", "MODE_RENDER_ASYNC", "FLAG_NONE", "FLAG_NO_CULL", "FLAG_AA_RESAMPLE", "Group", "GroupWorld", "group_unique_id",
           "host_register", "host_unregister", "host_canvas", "host_canvas_rgb8", "host_canvas_rgba8", "format_ppm_rgb8", "write_ppm_rgb8",
           "group_packed_rows", "group_bands_owned", "group_row_owner", "group_packed_row_to_image", "group_undeal_host", "EXCHANGE_RCCL", "EXCHANGE_P2P", "GATHER_NONE", "GATHER_F64", "GATHER_U8",
           "SPHERE", "PLANE", "CUBE", "RtcCamera", "RtcHit", "RtcLight", "RtcAreaLight", "RtcLens", "RtcMotion", "RtcMaterial", "RtcShape", "RtcStats"]
