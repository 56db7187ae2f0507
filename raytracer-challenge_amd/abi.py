"""ctypes mirror of include/rtc.h (struct layouts, constants, prototypes)."""
from __future__ import annotations

import ctypes as C

Mat16 = C.c_double * 16
Vec3 = C.c_double * 3

SPHERE, PLANE, CUBE = 0, 1, 2
MODE_RENDER, MODE_RENDER_ASYNC = 0, 1
FLAG_NONE, FLAG_NO_CULL, FLAG_AA_RESAMPLE, FLAG_LDS_TABLE = 0, 1, 2, 4
EXCHANGE_RCCL, EXCHANGE_P2P = 0, 1
GATHER_NONE, GATHER_F64, GATHER_U8 = 0, 1, 2
GROUP_ID_BYTES = 128
MAX_LIGHTS = 8
MAX_LIGHT_SAMPLES = 256
MAX_LENS_SAMPLES = 256
MAX_AO_SAMPLES = 256
PROJ_ORTHOGRAPHIC, PROJ_PANORAMA = 1, 2  # rtc_projection::kind
MAX_SHUTTER_SAMPLES = 256
SHUTTER_RING = 8
PATTERNS = {"none": 0, "test": 1, "stripe": 2, "stripes": 2, "gradient": 3, "ring": 4, "checker": 5, "checkers": 5, "grid": 6}
STATUS_NAMES = {0: "RTC_OK", 1: "RTC_ERR_SINGULAR", 2: "RTC_ERR_NO_COLOR", 3: "RTC_ERR_DEVICE", 4: "RTC_ERR_ARG",
                5: "RTC_ERR_PARSE", 6: "RTC_ERR_IO", 7: "RTC_ERR_NOMEM", 8: "RTC_ERR_UNSUPPORTED"}


class RtcMaterial(C.Structure):
    _fields_ = [("pattern_kind", C.c_uint32), ("has_color", C.c_uint32), ("color", Vec3),
                ("ambient", C.c_double), ("diffuse", C.c_double), ("specular", C.c_double), ("shininess", C.c_double),
                ("reflective", C.c_double), ("transparency", C.c_double), ("refractive_index", C.c_double),
                ("pat_inv", Mat16), ("pat_a", Vec3), ("pat_b", Vec3)]


class RtcShape(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("world_id", C.c_uint32), ("inv", Mat16), ("inv_t", Mat16), ("material", RtcMaterial)]


class RtcLight(C.Structure):
    _fields_ = [("intensity", Vec3), ("position", Vec3)]


class RtcAreaLight(C.Structure):
    _fields_ = [("intensity", Vec3), ("corner", Vec3), ("uvec", Vec3), ("vvec", Vec3), ("usteps", C.c_uint32), ("vsteps", C.c_uint32)]


class RtcLens(C.Structure):
    _fields_ = [("aperture", C.c_double), ("focal_distance", C.c_double), ("usteps", C.c_uint32), ("vsteps", C.c_uint32)]


class RtcAo(C.Structure):
    _fields_ = [("radius", C.c_double), ("usteps", C.c_uint32), ("vsteps", C.c_uint32)]


class RtcFilter(C.Structure):
    _fields_ = [("plane_sigma", C.c_double), ("passes", C.c_uint32), ("normal_squarings", C.c_uint32), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


FILTER_SAME_OBJECT = 1
MAX_FILTER_PASSES = 5
FILTER_DEFAULT_PLANE_SIGMA, FILTER_DEFAULT_PASSES, FILTER_DEFAULT_NORMAL_SQUARINGS = 0.05, 2, 3  # RTC_FILTER_DEFAULT_*


class RtcAdaptive(C.Structure):
    _fields_ = [("threshold", C.c_double), ("usteps", C.c_uint32), ("vsteps", C.c_uint32), ("max_rays", C.c_uint32), ("_pad", C.c_uint32)]


class RtcAdaptiveInfo(C.Structure):
    _fields_ = [("pixels_refined", C.c_uint64), ("rays_refined", C.c_uint64), ("launches", C.c_uint32), ("_pad", C.c_uint32)]


MAX_AA_SAMPLES = 256
AA_DEFAULT_THRESHOLD, AA_DEFAULT_STEPS, AA_DEFAULT_MAX_RAYS = 0.01, 4, 1 << 21  # RTC_AA_DEFAULT_*


class RtcLuminance(C.Structure):
    _fields_ = [("max", C.c_double), ("sum", C.c_double), ("count", C.c_uint64)]


class RtcTonemap(C.Structure):
    _fields_ = [("exposure", C.c_double), ("white", C.c_double), ("curve", C.c_uint32), ("flags", C.c_uint32)]


class RtcBloom(C.Structure):
    _fields_ = [("threshold", C.c_double), ("strength", C.c_double), ("sigma", C.c_double), ("radius", C.c_uint32), ("_pad", C.c_uint32)]


TONEMAP_LINEAR, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2  # rtc_tonemap::curve
TONEMAP_CURVES = {"linear": 0, "reinhard": 1, "aces": 2}
TONEMAP_AUTO_EXPOSURE, TONEMAP_AUTO_WHITE = 1, 2  # rtc_tonemap::flags
MAX_BLOOM_RADIUS = 32


class RtcResize(C.Structure):
    _fields_ = [("filter", C.c_uint32), ("_pad", C.c_uint32)]


RESIZE_BOX, RESIZE_TRIANGLE, RESIZE_CATMULL_ROM, RESIZE_MITCHELL, RESIZE_LANCZOS3 = range(5)  # rtc_resize::filter
RESIZE_FILTERS = {"box": 0, "triangle": 1, "catmull-rom": 2, "mitchell": 3, "lanczos3": 4}
MAX_RESIZE_TAPS = 1024


class RtcGatherBuffers(C.Structure):
    _fields_ = [("radiance", C.c_void_p), ("bounce", C.c_void_p)]


class RtcProjection(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("_pad", C.c_uint32), ("width", C.c_double), ("h_span", C.c_double), ("v_span", C.c_double)]


class RtcCamera(C.Structure):
    _fields_ = [("hsize", C.c_uint32), ("vsize", C.c_uint32), ("fov", C.c_double), ("half_width", C.c_double),
                ("half_height", C.c_double), ("pixel_size", C.c_double), ("view_inv", Mat16), ("samples", C.c_uint32),
                ("_pad", C.c_uint32)]


class RtcMotion(C.Structure):
    _fields_ = [("shape", C.c_uint32), ("_pad", C.c_uint32), ("transform_open", Mat16), ("transform_close", Mat16)]


class RtcShutterScene(C.Structure):
    _fields_ = [("shapes", C.POINTER(RtcShape)), ("n_shapes", C.c_uint32), ("motions", C.POINTER(RtcMotion)), ("n_motions", C.c_uint32),
                ("lights", C.POINTER(RtcAreaLight)), ("n_lights", C.c_uint32), ("cam_open", C.POINTER(RtcCamera)),
                ("cam_close", C.POINTER(RtcCamera)), ("lens", C.POINTER(RtcLens)), ("samples", C.c_uint32), ("_pad", C.c_uint32)]


class RtcStats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_shadow", C.c_uint64), ("rays_reflect", C.c_uint64),
                ("rays_refract", C.c_uint64), ("pixels", C.c_uint64), ("pixels_resample", C.c_uint64), ("rays_primary_proven_miss", C.c_uint64),
                ("_reserved", C.c_uint64 * 1)]


class RtcHit(C.Structure):
    _fields_ = [("hit_index", C.c_int32), ("inside", C.c_uint32), ("shadowed", C.c_uint32), ("_pad", C.c_uint32),
                ("t", C.c_double), ("point", Vec3), ("over_point", Vec3), ("under_point", Vec3), ("eyev", Vec3),
                ("normal", Vec3), ("reflectv", Vec3), ("n1", C.c_double), ("n2", C.c_double)]


class RtcLaunchInfo(C.Structure):
    _fields_ = [("source", C.c_uint32), ("reflective", C.c_uint32), ("refractive", C.c_uint32), ("binned", C.c_uint32),
                ("light_lists", C.c_uint32), ("lane", C.c_uint32), ("block", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("tiles_per_workgroup", C.c_uint32), ("multi_tile_workgroups", C.c_uint32), ("light_table", C.c_uint32), ("lens_samples", C.c_uint32)]


class RtcLuaJob(C.Structure):
    _fields_ = [("shapes", C.POINTER(RtcShape)), ("n_shapes", C.c_uint32), ("kind", C.c_uint32), ("light", RtcLight), ("camera", RtcCamera),
                ("outfile", C.c_char_p), ("animation", C.c_uint32), ("frame", C.c_uint32), ("same_world_as_previous", C.c_uint32),
                ("line", C.c_uint32)]


class RtcAovBuffers(C.Structure):
    _fields_ = [("index", C.c_void_p), ("depth", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p), ("flags", C.c_void_p),
                ("shadow", C.c_void_p)]


class RtcFloatPlanes(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("aov", RtcAovBuffers), ("rgb_type", C.c_uint32), ("_pad", C.c_uint32)]


FLOAT_FORMATS = {"hdr": 0, "pfm": 1, "exr": 2}
FLOAT_HDR, FLOAT_PFM, FLOAT_EXR = range(3)
EXR_TYPES = {"half": 1, "float": 2}
EXR_HALF, EXR_FLOAT = 1, 2
AOV_PLANES = {"index": ("int32", 1), "depth": ("float64", 1), "point": ("float64", 3), "normal": ("float64", 3),
              "flags": ("uint8", 1), "shadow": ("uint16", 1)}  # plane -> (numpy dtype, components per pixel)
AOV_VIEWS = {"depth": 0, "normal": 1, "index": 2, "shadow": 3}
AOV_VIEW_DEPTH, AOV_VIEW_NORMAL, AOV_VIEW_INDEX, AOV_VIEW_SHADOW = range(4)

LUA_FRAME_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(RtcLuaJob), C.c_uint32, C.POINTER(C.c_uint8))
LUA_GIF_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(RtcLuaJob), C.c_uint32, C.POINTER(C.c_uint8), C.c_size_t)
GIF_SEGMENT, GIF_DELAY_CS = 4096, 7
LUA_FILE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(RtcLuaJob), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_size_t)
LUA_OUT_RGB8, LUA_OUT_GIF_RECORD, LUA_OUT_JPEG, LUA_OUT_PNG, LUA_OUT_FILE = 0, 1, 2, 3, 4
IMAGE_FORMATS = {"png": 0, "jpeg": 1, "gif": 2, "ppm": 3, "bmp": 4, "tga": 5, "tiff": 6, "ico": 7, "farbfeld": 8, "pam": 9}
(IMAGE_PNG, IMAGE_JPEG, IMAGE_GIF, IMAGE_PPM, IMAGE_BMP, IMAGE_TGA, IMAGE_TIFF, IMAGE_ICO, IMAGE_FARBFELD,
 IMAGE_PAM) = range(10)
IMAGE_JPEG_QUALITY, TIFF_STRIP_BYTES = 75, 65536
PNG_SEGMENT, PNG_CHAIN = 32768, 8

SOURCE_NAMES = {0: "brute force, records through the scalar cache", 1: "brute force, object table staged in LDS (one tile)",
                2: "brute force, object table staged in LDS tiles", 3: "one-level per-wave cull", 4: "two-level per-wave cull"}

assert C.sizeof(RtcMaterial) == 264 and C.sizeof(RtcShape) == 528 and C.sizeof(RtcHit) == 184
assert C.sizeof(RtcAreaLight) == 104 and C.sizeof(RtcLaunchInfo) == 48 and C.sizeof(RtcLens) == 24 and C.sizeof(RtcProjection) == 32
assert C.sizeof(RtcMotion) == 264 and C.sizeof(RtcShutterScene) == 80
assert C.sizeof(RtcLuminance) == 24 and C.sizeof(RtcTonemap) == 24 and C.sizeof(RtcBloom) == 32
assert C.sizeof(RtcResize) == 8
assert C.sizeof(RtcAovBuffers) == 48 and C.sizeof(RtcFloatPlanes) == 64 and C.sizeof(RtcAo) == 16 and C.sizeof(RtcGatherBuffers) == 16

D = C.c_double
PD = C.POINTER(C.c_double)
U32 = C.c_uint32
VP = C.c_void_p

# name -> (restype, argtypes); every symbol include/rtc.h declares
PROTOTYPES = {
    "rtc_abi_version": (U32, []),
    "rtc_strerror": (C.c_char_p, [C.c_int32]),
    "rtc_matrix_identity": (None, [Mat16]),
    "rtc_matrix_multiply": (None, [Mat16, Mat16, Mat16]),
    "rtc_matrix_translation": (None, [Mat16, D, D, D, Mat16]),
    "rtc_matrix_scaling": (None, [Mat16, D, D, D, Mat16]),
    "rtc_matrix_rotation_x": (None, [Mat16, D, Mat16]),
    "rtc_matrix_rotation_y": (None, [Mat16, D, Mat16]),
    "rtc_matrix_rotation_z": (None, [Mat16, D, Mat16]),
    "rtc_matrix_shearing": (None, [Mat16, D, D, D, D, D, D, Mat16]),
    "rtc_matrix_determinant": (D, [Mat16]),
    "rtc_matrix_inverse": (C.c_int32, [Mat16, Mat16]),
    "rtc_matrix_transpose": (None, [Mat16, Mat16]),
    "rtc_view_transform": (None, [Vec3, Vec3, Vec3, Mat16]),
    "rtc_camera_init": (C.c_int32, [U32, U32, D, Mat16, C.POINTER(RtcCamera)]),
    "rtc_camera_ray_for_pixel": (None, [C.POINTER(RtcCamera), U32, D, U32, D, C.c_double * 6]),
    "rtc_lens_validate": (C.c_int32, [C.POINTER(RtcLens)]),
    "rtc_lens_ray": (C.c_int32, [C.POINTER(RtcCamera), C.POINTER(RtcLens), U32, U32, U32, C.c_double * 6]),
    "rtc_projection_validate": (C.c_int32, [C.POINTER(RtcProjection)]),
    "rtc_projection_ray": (C.c_int32, [C.POINTER(RtcCamera), C.POINTER(RtcProjection), U32, U32, C.c_double * 6]),
    "rtc_projection_tables": (C.c_int32, [C.POINTER(RtcCamera), C.POINTER(RtcProjection), PD, PD]),
    "rtc_material_default": (None, [C.POINTER(RtcMaterial)]),
    "rtc_shape_init": (C.c_int32, [U32, Mat16, C.POINTER(RtcMaterial), C.POINTER(RtcShape)]),
    "rtc_material_set_pattern": (C.c_int32, [C.POINTER(RtcMaterial), U32, Vec3, Vec3, Mat16]),
    "rtc_light_default": (None, [C.POINTER(RtcLight)]),
    "rtc_canvas_write_png8": (C.c_int32, [C.c_char_p, C.POINTER(C.c_uint8), U32, U32, U32]),
    "rtc_canvas_format_png8": (C.c_size_t, [C.POINTER(C.c_uint8), U32, U32, U32, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_lua_run": (C.c_int32, [C.c_char_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
    "rtc_lua_run_file": (C.c_int32, [C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
    "rtc_lua_program_jobs": (C.c_uint32, [C.c_void_p]),
    "rtc_lua_program_job": (C.c_int32, [C.c_void_p, C.c_uint32, C.POINTER(RtcLuaJob)]),
    "rtc_lua_program_output": (C.c_char_p, [C.c_void_p]),
    "rtc_lua_program_free": (None, [C.c_void_p]),
    "rtc_lua_program_render": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, LUA_FRAME_FN, C.c_void_p, C.POINTER(RtcStats)]),
    "rtc_lua_program_render_gif": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, LUA_GIF_FN, C.c_void_p, C.POINTER(RtcStats)]),
    "rtc_gif_quantize": (C.c_int32, [C.POINTER(C.c_uint8), U32, U32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(U32)]),
    "rtc_gif_lzw": (C.c_size_t, [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_gif_format": (C.c_size_t, [C.POINTER(C.c_uint8), U32, U32, U32, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_gif_writer_create": (C.c_int32, [VP, C.POINTER(VP)]),
    "rtc_gif_writer_append_device": (C.c_int32, [VP, VP, U32, U32]),
    "rtc_gif_writer_render": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32]),
    "rtc_gif_writer_bytes": (C.c_size_t, [VP, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_gif_writer_write": (C.c_int32, [VP, C.c_char_p]),
    "rtc_gif_writer_destroy": (None, [VP]),
    "rtc_jpeg_quant_tables": (C.c_int32, [C.c_int32, C.POINTER(C.c_uint16)]),
    "rtc_jpeg_fdct": (C.c_int32, [C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    "rtc_jpeg_coefficients": (C.c_int32, [C.POINTER(C.c_uint8), U32, U32, U32, C.c_int32, C.POINTER(C.c_int16)]),
    "rtc_jpeg_format": (C.c_size_t, [C.POINTER(C.c_uint8), U32, U32, U32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_canvas_write_jpeg": (C.c_int32, [C.c_char_p, C.POINTER(C.c_uint8), U32, U32, U32, C.c_int32]),
    "rtc_jpeg_encoder_create": (C.c_int32, [VP, C.POINTER(VP)]),
    "rtc_jpeg_encoder_encode_device": (C.c_int32, [VP, VP, U32, U32, U32, C.c_int32]),
    "rtc_jpeg_encoder_render": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, C.c_float, C.c_int32]),
    "rtc_jpeg_encoder_bytes": (C.c_size_t, [VP, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_jpeg_encoder_write": (C.c_int32, [VP, C.c_char_p]),
    "rtc_jpeg_encoder_destroy": (None, [VP]),
    "rtc_lua_program_render_files": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, LUA_FILE_FN, C.c_void_p, C.POINTER(RtcStats)]),
    "rtc_png_filter": (C.c_int32, [C.POINTER(C.c_uint8), U32, U32, U32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "rtc_png_format": (C.c_size_t, [C.POINTER(C.c_uint8), U32, U32, U32, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_canvas_write_png": (C.c_int32, [C.c_char_p, C.POINTER(C.c_uint8), U32, U32, U32]),
    "rtc_png_encoder_create": (C.c_int32, [VP, C.POINTER(VP)]),
    "rtc_png_encoder_encode_device": (C.c_int32, [VP, VP, U32, U32, U32]),
    "rtc_png_encoder_render": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, C.c_float]),
    "rtc_png_encoder_bytes": (C.c_size_t, [VP, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_png_encoder_write": (C.c_int32, [VP, C.c_char_p]),
    "rtc_png_encoder_destroy": (None, [VP]),
    "rtc_lua_program_render_png": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, LUA_FILE_FN, C.c_void_p, C.POINTER(RtcStats)]),
    "rtc_image_format_for_name": (C.c_int32, [C.c_char_p, C.POINTER(U32)]),
    "rtc_image_format": (C.c_size_t, [U32, C.POINTER(C.c_uint8), U32, U32, U32, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_canvas_save": (C.c_int32, [C.c_char_p, C.POINTER(C.c_uint8), U32, U32, U32]),
    "rtc_image_encoder_create": (C.c_int32, [VP, C.POINTER(VP)]),
    "rtc_image_encoder_encode_device": (C.c_int32, [VP, U32, VP, U32, U32, U32]),
    "rtc_image_encoder_render": (C.c_int32, [VP, U32, VP, C.POINTER(RtcCamera), U32, U32, C.c_float]),
    "rtc_image_encoder_bytes": (C.c_size_t, [VP, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_image_encoder_write": (C.c_int32, [VP, C.c_char_p]),
    "rtc_image_encoder_destroy": (None, [VP]),
    "rtc_lua_program_render_saved": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, LUA_FILE_FN, C.c_void_p, C.POINTER(RtcStats)]),
    "rtc_lua_program_job_lights": (C.c_int32, [C.c_void_p, U32, C.POINTER(RtcLight), U32, C.POINTER(U32)]),
    "rtc_area_light_from_point": (C.c_int32, [C.POINTER(RtcLight), C.POINTER(RtcAreaLight)]),
    "rtc_area_light_expand": (C.c_int32, [C.POINTER(RtcAreaLight), U32, C.POINTER(RtcLight), U32, C.POINTER(U32)]),
    "rtc_shutter_time": (D, [U32, U32]),
    "rtc_shutter_shapes": (C.c_int32, [C.POINTER(RtcShape), U32, C.POINTER(RtcMotion), U32, U32, U32, C.POINTER(RtcShape)]),
    "rtc_shutter_camera": (C.c_int32, [C.POINTER(RtcCamera), C.POINTER(RtcCamera), U32, U32, C.POINTER(RtcCamera)]),
    "rtc_canvas_average": (C.c_int32, [PD, U32, C.c_size_t, PD]),
    "rtc_canvas_average_device": (C.c_int32, [VP, VP, U32, C.c_size_t, VP]),
    "rtc_shutter_create": (C.c_int32, [VP, C.POINTER(VP)]),
    "rtc_shutter_destroy": (None, [VP]),
    "rtc_shutter_render": (C.c_int32, [VP, C.POINTER(RtcShutterScene), U32, U32, PD, C.POINTER(RtcStats)]),
    "rtc_shutter_render_rgb8": (C.c_int32, [VP, C.POINTER(RtcShutterScene), U32, U32, C.POINTER(C.c_uint8), C.POINTER(RtcStats)]),
    "rtc_shutter_render_rgba8": (C.c_int32, [VP, C.POINTER(RtcShutterScene), U32, U32, C.c_float, C.POINTER(C.c_uint8), C.POINTER(RtcStats)]),
    "rtc_shutter_render_device": (C.c_int32, [VP, C.POINTER(RtcShutterScene), U32, U32, C.c_float, VP, VP, VP]),
    "rtc_lua_program_job_area_lights": (C.c_int32, [C.c_void_p, U32, C.POINTER(RtcAreaLight), U32, C.POINTER(U32)]),
    "rtc_free": (None, [VP]),
    "rtc_canvas_write_ppm": (C.c_int32, [C.c_char_p, PD, U32, U32]),
    "rtc_canvas_format_ppm": (C.c_size_t, [PD, U32, U32, C.c_char_p, C.c_size_t]),
    "rtc_color_scale255": (None, [PD, C.c_size_t, C.POINTER(C.c_uint8)]),
    "rtc_canvas_to_rgba8": (None, [PD, U32, U32, C.c_float, C.POINTER(C.c_uint8)]),
    "rtc_gamma_thresholds": (C.c_int32, [C.c_float, PD]),
    "rtc_context_create": (C.c_int32, [C.c_int32, VP, C.POINTER(VP)]),
    "rtc_context_destroy": (None, [VP]),
    "rtc_context_synchronize": (C.c_int32, [VP]),
    "rtc_context_device_info": (C.c_int32, [VP, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rtc_world_create": (C.c_int32, [VP, C.POINTER(RtcShape), U32, C.POINTER(RtcLight), C.POINTER(VP)]),
    "rtc_world_update": (C.c_int32, [VP, VP, C.POINTER(RtcShape), U32, C.POINTER(RtcLight)]),
    "rtc_world_create_lights": (C.c_int32, [VP, C.POINTER(RtcShape), U32, C.POINTER(RtcLight), U32, C.POINTER(VP)]),
    "rtc_world_update_lights": (C.c_int32, [VP, VP, C.POINTER(RtcShape), U32, C.POINTER(RtcLight), U32]),
    "rtc_world_light_count": (U32, [VP]),
    "rtc_world_create_area_lights": (C.c_int32, [VP, C.POINTER(RtcShape), U32, C.POINTER(RtcAreaLight), U32, C.POINTER(VP)]),
    "rtc_world_update_area_lights": (C.c_int32, [VP, VP, C.POINTER(RtcShape), U32, C.POINTER(RtcAreaLight), U32]),
    "rtc_world_destroy": (None, [VP]),
    "rtc_render_rows": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, U32, VP, VP, U32]),
    "rtc_render_lens_rows": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcLens), U32, U32, U32, VP, VP, U32]),
    "rtc_render_lens": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcLens), U32, U32, PD, C.POINTER(RtcStats)]),
    "rtc_render_lens_rgb8": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcLens), U32, U32, C.POINTER(C.c_uint8), C.POINTER(RtcStats)]),
    "rtc_render_projection_rows": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), U32, U32, U32, VP, VP, U32]),
    "rtc_render_projection": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), U32, U32, PD, C.POINTER(RtcStats)]),
    "rtc_render_projection_rgb8": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), U32, U32, C.POINTER(C.c_uint8), C.POINTER(RtcStats)]),
    "rtc_context_last_launch_projection": (C.c_int32, [VP, C.POINTER(U32)]),
    "rtc_render_bands": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, U32, VP, VP, U32]),
    "rtc_render_views": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, U32, U32, VP, VP, U32, U32]),
    "rtc_render": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, PD, C.POINTER(RtcStats)]),
    "rtc_render_rgb8": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, C.POINTER(C.c_uint8), C.POINTER(RtcStats)]),
    "rtc_render_rgba8": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, C.c_float, C.POINTER(C.c_uint8), C.POINTER(RtcStats)]),
    "rtc_render_views_rgba8": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, U32, U32, C.c_float, VP, U32, U32]),
    "rtc_canvas_to_rgba8_device": (C.c_int32, [VP, VP, U32, U32, C.c_float, VP]),
    "rtc_canvas_write_ppm_rgb8": (C.c_int32, [C.c_char_p, C.POINTER(C.c_uint8), U32, U32]),
    "rtc_canvas_format_ppm_rgb8": (C.c_size_t, [C.POINTER(C.c_uint8), U32, U32, C.c_char_p, C.c_size_t]),
    "rtc_context_set_pipeline": (C.c_int32, [VP, U32]),
    "rtc_context_fence": (C.c_int32, [VP]),
    "rtc_context_last_launch_info": (C.c_int32, [VP, C.POINTER(RtcLaunchInfo)]),
    "rtc_host_alloc": (C.c_int32, [C.c_size_t, C.POINTER(VP)]),
    "rtc_host_free": (None, [VP]),
    "rtc_stats_read": (C.c_int32, [VP, C.POINTER(RtcStats)]),
    "rtc_stats_reset": (C.c_int32, [VP]),
    "rtc_kernel_times_ms": (C.c_int32, [VP, C.POINTER(C.c_float), U32, C.POINTER(U32)]),
    "rtc_binning_times_ms": (C.c_int32, [VP, C.POINTER(C.c_float), U32, C.POINTER(U32)]),
    "rtc_context_set_timing": (C.c_int32, [VP, U32]),
    "rtc_last_kernel_ms": (C.c_int32, [VP, C.POINTER(C.c_float)]),
    "rtc_host_register": (C.c_int32, [VP, C.c_size_t]),
    "rtc_host_unregister": (C.c_int32, [VP]),
    "rtc_group_create": (C.c_int32, [C.POINTER(C.c_int32), U32, U32, C.POINTER(VP)]),
    "rtc_group_unique_id": (C.c_int32, [C.POINTER(C.c_uint8)]),
    "rtc_group_create_rank": (C.c_int32, [C.c_int32, U32, U32, C.POINTER(C.c_uint8), C.POINTER(VP)]),
    "rtc_group_destroy": (None, [VP]),
    "rtc_group_size": (U32, [VP]),
    "rtc_group_local_size": (U32, [VP]),
    "rtc_group_context": (VP, [VP, U32]),
    "rtc_group_synchronize": (C.c_int32, [VP]),
    "rtc_group_world_create": (C.c_int32, [VP, C.POINTER(RtcShape), U32, C.POINTER(RtcLight), C.POINTER(VP)]),
    "rtc_group_world_destroy": (None, [VP]),
    "rtc_group_render": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, U32, U32, VP, VP]),
    "rtc_group_render_host": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, PD, C.POINTER(RtcStats)]),
    "rtc_group_render_host_rgb8": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, C.POINTER(C.c_uint8), C.POINTER(RtcStats)]),
    "rtc_group_render_host_rgba8": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, C.c_float, C.POINTER(C.c_uint8), C.POINTER(RtcStats)]),
    "rtc_group_packed_rows": (U32, [U32, U32]),
    "rtc_group_bands_owned": (U32, [U32, U32, U32]),
    "rtc_group_row_owner": (None, [U32, U32, C.POINTER(U32), C.POINTER(U32)]),
    "rtc_group_packed_row_to_image": (U32, [U32, U32, U32]),
    "rtc_group_undeal_host": (C.c_int32, [VP, VP, U32, U32, U32, C.c_size_t]),
    "rtc_group_stats_read": (C.c_int32, [VP, C.POINTER(RtcStats)]),
    "rtc_group_stats_reset": (C.c_int32, [VP]),
    "rtc_color_at": (C.c_int32, [VP, VP, PD, U32, U32, U32, PD, C.POINTER(RtcHit)]),
    "rtc_device_arith": (C.c_int32, [VP, U32, PD, PD, U32, PD]),
    "rtc_aov_from_hits": (C.c_int32, [C.POINTER(RtcHit), C.POINTER(C.c_uint16), U32, U32, U32, C.POINTER(RtcAovBuffers)]),
    "rtc_render_aov_device": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, C.POINTER(RtcAovBuffers)]),
    "rtc_render_aov": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), U32, U32, C.POINTER(RtcAovBuffers)]),
    "rtc_aov_view_rgb8": (C.c_int32, [U32, C.POINTER(RtcAovBuffers), U32, U32, D, D, U32, C.POINTER(C.c_uint8)]),
    "rtc_aov_view_rgb8_device": (C.c_int32, [VP, U32, C.POINTER(RtcAovBuffers), U32, U32, D, D, U32, VP]),
    "rtc_ao_validate": (C.c_int32, [C.POINTER(RtcAo)]),
    "rtc_ao_expand": (C.c_int32, [C.POINTER(RtcAo), PD, C.POINTER(U32)]),
    "rtc_ao_ray": (C.c_int32, [PD, PD, PD, PD]),
    "rtc_ao_from_hits": (C.c_int32, [C.POINTER(RtcHit), C.POINTER(C.c_uint16), U32, U32, U32, C.POINTER(C.c_uint16)]),
    "rtc_render_ao_device": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcAo), U32, U32, VP]),
    "rtc_render_ao": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcAo), U32, U32, C.POINTER(C.c_uint16)]),
    "rtc_canvas_apply_ao": (C.c_int32, [PD, C.POINTER(C.c_uint16), U32, D, U32, U32]),
    "rtc_canvas_apply_ao_device": (C.c_int32, [VP, VP, VP, U32, D, U32, U32]),
    "rtc_gather_from_hits": (C.c_int32, [C.POINTER(RtcHit), C.POINTER(RtcHit), PD, PD, U32, D, U32, U32, U32, C.POINTER(RtcGatherBuffers)]),
    "rtc_render_gather_device": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcAo), U32, U32, C.POINTER(RtcGatherBuffers)]),
    "rtc_render_gather": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcAo), U32, U32, C.POINTER(RtcGatherBuffers)]),
    # the three passes with a projection's rays: the pinhole entry's signature with the projection after the camera
    "rtc_render_aov_projection_device": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), U32, U32, C.POINTER(RtcAovBuffers)]),
    "rtc_render_aov_projection": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), U32, U32, C.POINTER(RtcAovBuffers)]),
    "rtc_render_ao_projection_device": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), C.POINTER(RtcAo), U32, U32, VP]),
    "rtc_render_ao_projection": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), C.POINTER(RtcAo), U32, U32, C.POINTER(C.c_uint16)]),
    "rtc_render_gather_projection_device": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), C.POINTER(RtcAo), U32, U32, C.POINTER(RtcGatherBuffers)]),
    "rtc_render_gather_projection": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcProjection), C.POINTER(RtcAo), U32, U32, C.POINTER(RtcGatherBuffers)]),
    "rtc_canvas_add_scaled": (C.c_int32, [PD, PD, D, U32, U32]),
    "rtc_canvas_add_scaled_device": (C.c_int32, [VP, VP, VP, D, U32, U32]),
    "rtc_float_format_for_name": (C.c_int32, [C.c_char_p, C.POINTER(U32)]),
    "rtc_float_format": (C.c_size_t, [U32, C.POINTER(RtcFloatPlanes), U32, U32, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_canvas_save_f64": (C.c_int32, [C.c_char_p, PD, U32, U32]),
    "rtc_hdr_rle_row": (C.c_int32, [C.POINTER(C.c_uint8), U32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "rtc_float_encoder_create": (C.c_int32, [VP, C.POINTER(VP)]),
    "rtc_float_encoder_encode_device": (C.c_int32, [VP, U32, C.POINTER(RtcFloatPlanes), U32, U32]),
    "rtc_float_encoder_render": (C.c_int32, [VP, U32, VP, C.POINTER(RtcCamera), U32, U32, U32]),
    "rtc_float_encoder_render_lens": (C.c_int32, [VP, U32, VP, C.POINTER(RtcCamera), C.POINTER(RtcLens), U32, U32, U32]),
    "rtc_float_encoder_bytes": (C.c_size_t, [VP, C.POINTER(C.c_uint8), C.c_size_t]),
    "rtc_float_encoder_write": (C.c_int32, [VP, C.c_char_p]),
    "rtc_float_encoder_destroy": (None, [VP]),
    "rtc_filter_validate": (C.c_int32, [C.POINTER(RtcFilter)]),
    "rtc_plane_filter": (C.c_int32, [PD, U32, C.POINTER(RtcAovBuffers), U32, U32, C.POINTER(RtcFilter), PD]),
    "rtc_plane_filter_device": (C.c_int32, [VP, VP, U32, C.POINTER(RtcAovBuffers), U32, U32, C.POINTER(RtcFilter), VP]),
    "rtc_counts_to_fraction": (C.c_int32, [C.POINTER(C.c_uint16), U32, U32, U32, PD]),
    "rtc_counts_to_fraction_device": (C.c_int32, [VP, VP, U32, U32, U32, VP]),
    "rtc_canvas_apply_occlusion": (C.c_int32, [PD, PD, D, U32, U32]),
    "rtc_canvas_apply_occlusion_device": (C.c_int32, [VP, VP, VP, D, U32, U32]),
    "rtc_adaptive_validate": (C.c_int32, [C.POINTER(RtcAdaptive)]),
    "rtc_adaptive_offset": (C.c_int32, [C.POINTER(RtcAdaptive), U32, PD, PD]),
    "rtc_adaptive_mask": (C.c_int32, [PD, U32, U32, U32, D, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]),
    "rtc_adaptive_mask_device": (C.c_int32, [VP, VP, U32, U32, U32, D, VP]),
    "rtc_render_adaptive_device": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcAdaptive), U32, U32, VP, VP, C.POINTER(RtcAdaptiveInfo)]),
    "rtc_render_adaptive": (C.c_int32, [VP, VP, C.POINTER(RtcCamera), C.POINTER(RtcAdaptive), U32, U32, PD, C.POINTER(C.c_uint8),
                                        C.POINTER(RtcAdaptiveInfo), C.POINTER(RtcStats)]),
    "rtc_canvas_luminance": (C.c_int32, [PD, U32, U32, C.POINTER(RtcLuminance)]),
    "rtc_canvas_luminance_device": (C.c_int32, [VP, VP, U32, U32, VP]),
    "rtc_tonemap_validate": (C.c_int32, [C.POINTER(RtcTonemap)]),
    "rtc_tonemap_resolve": (C.c_int32, [C.POINTER(RtcTonemap), C.POINTER(RtcLuminance), PD, PD]),
    "rtc_canvas_tonemap": (C.c_int32, [PD, U32, U32, C.POINTER(RtcTonemap), C.POINTER(RtcLuminance), PD]),
    "rtc_canvas_tonemap_device": (C.c_int32, [VP, VP, U32, U32, C.POINTER(RtcTonemap), VP, VP]),
    "rtc_bloom_validate": (C.c_int32, [C.POINTER(RtcBloom)]),
    "rtc_bloom_weights": (C.c_int32, [C.POINTER(RtcBloom), PD]),
    "rtc_canvas_bloom": (C.c_int32, [PD, U32, U32, C.POINTER(RtcBloom), PD]),
    "rtc_canvas_bloom_device": (C.c_int32, [VP, VP, U32, U32, C.POINTER(RtcBloom), VP]),
    "rtc_resize_validate": (C.c_int32, [C.POINTER(RtcResize)]),
    "rtc_resize_taps": (U32, [U32, U32, U32]),
    "rtc_resize_weights": (C.c_int32, [U32, U32, C.POINTER(RtcResize), C.POINTER(U32), C.POINTER(U32), PD]),
    "rtc_canvas_resize": (C.c_int32, [PD, U32, U32, C.POINTER(RtcResize), PD, U32, U32]),
    "rtc_canvas_resize_device": (C.c_int32, [VP, VP, U32, U32, C.POINTER(RtcResize), VP, U32, U32]),
}

# The scene loaders (include/rtc.h): one common argument list per family, then the entry's own out-arguments. Each `_file`
# twin takes a path where the text entry takes the text: the same list by construction.
P = C.POINTER


def _loader(lights, capped=True, lua=False, extra=()):
    return ([C.c_char_p] + ([U32] if lua else []) + [P(P(RtcShape)), P(U32), P(lights)] + ([U32, P(U32)] if capped else []) + [P(RtcCamera)]
            + ([C.c_char_p, C.c_size_t, P(U32)] if lua else []) + [C.c_char_p, C.c_size_t] + list(extra))


def _record(ctype):  # an optional record and its "the camera has the keys" flag
    return [P(ctype), P(U32)]


_LENS, _AO = _record(RtcLens), _record(RtcAo)
_YAML_EXTRA = {  # entry -> what follows errbuf_len
    "lens": _LENS, "motion": _LENS + [P(P(RtcMotion)), P(U32), P(U32)], "projection": _LENS + _record(RtcProjection), "ao": _LENS + _AO,
    "gather": _LENS + _AO + _AO, "filter": _LENS + _AO + _AO + _record(RtcFilter), "adaptive": _record(RtcAdaptive),
    "post": _record(RtcTonemap) + _record(RtcBloom), "resize": _LENS + _record(RtcProjection) + [P(RtcResize), P(U32), P(U32), P(U32)],
    "projection_passes": _LENS + _record(RtcProjection) + _AO + _AO + _record(RtcFilter),
}
_LOADERS = {"rtc_scene_load_yaml": _loader(RtcLight, capped=False), "rtc_scene_load_yaml_lights": _loader(RtcLight),
            "rtc_scene_load_yaml_area_lights": _loader(RtcAreaLight),
            **{"rtc_scene_load_yaml_" + entry: _loader(RtcAreaLight, extra=extra) for entry, extra in _YAML_EXTRA.items()},
            "rtc_scene_load_lua": _loader(RtcLight, capped=False, lua=True), "rtc_scene_load_lua_lights": _loader(RtcLight, lua=True),
            "rtc_scene_load_lua_area_lights": _loader(RtcAreaLight, lua=True)}
for _name, _args in _LOADERS.items():
    PROTOTYPES[_name] = PROTOTYPES[_name + "_file"] = (C.c_int32, _args)


def declare(lib: C.CDLL) -> None:
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
