/*
 * rtc.h — C-ABI of the MI355X-native renderer for the per-pixel hot path of
 * joedane/raytracer-challenge (crate `ch1`):
 *
 *     Camera::render / render_async  ->  World::color_at  ->  World::intersect
 *                                    ->  shade_hit (lighting, shadow, reflect, refract)
 *
 * The reference has no FFI of its own (plain Rust `pub` methods); every
 * entry point below cites the reference item (file:line under ch1/src/) whose job it
 * takes over, so that a Rust `extern "C"` block binding these names is mechanical
 * (the stub is shown in INTEGRATION.md).
 *
 * Conventions
 *   - plain pointers and sizes only; nothing unwinds across this boundary;
 *     every function returns an rtc_status (0 = RTC_OK) unless stated otherwise.
 *   - all arithmetic on the path is IEEE f64 (vec.rs:7-12, color.rs:5-10), evaluated in
 *     the reference's operation order with no FMA contraction.
 *   - matrices are 4x4 row-major `double[16]` (transform.rs:23-27).
 *   - a canvas is `double[height][width][3]`, row-major, idx = y*width + x
 *     (canvas.rs:16-22,43-51).
 *   - functions marked [host] never touch the GPU; functions marked [device] need a
 *     context and fail with RTC_ERR_DEVICE when no MI355X is usable. There is no CPU
 *     fallback inside this library.
 */
#ifndef RTC_H
#define RTC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTC_ABI_VERSION 3u

/* ---- status codes (the reference panics instead) -------------------- */
typedef int32_t rtc_status;
enum {
    RTC_OK             = 0,
    RTC_ERR_SINGULAR   = 1, /* Matrix::inverse on |det| <= 1e-8      transform.rs:35-38,175-177 */
    RTC_ERR_NO_COLOR   = 2, /* material with neither colour nor pattern  material.rs:328-331    */
    RTC_ERR_DEVICE     = 3, /* no usable gfx950 device / HIP runtime error                      */
    RTC_ERR_ARG        = 4, /* null pointer, zero size, row range outside the canvas ...        */
    RTC_ERR_PARSE      = 5, /* scene description rejected (lua.rs:216,322-326 analogue)         */
    RTC_ERR_IO         = 6, /* file could not be opened / written     canvas.rs:87-91           */
    RTC_ERR_NOMEM      = 7,
    RTC_ERR_UNSUPPORTED= 8  /* a build or device without what the call needs (e.g. no RCCL library)   */
};

/* ---- enumerations ------------------------------------------------------------------ */
enum { /* rtc_shape.kind                        */
    RTC_SPHERE = 0, /* shape.rs:281-394 */
    RTC_PLANE  = 1, /* shape.rs:405-498 */
    RTC_CUBE   = 2  /* shape.rs:500-630 */
};
enum { /* rtc_material.pattern_kind              */
    RTC_PATTERN_NONE     = 0,
    RTC_PATTERN_TEST     = 1, /* material.rs:48-70   */
    RTC_PATTERN_STRIPE   = 2, /* material.rs:72-104  */
    RTC_PATTERN_GRADIENT = 3, /* material.rs:106-136 */
    RTC_PATTERN_RING     = 4, /* material.rs:138-171 */
    RTC_PATTERN_CHECKER  = 5, /* material.rs:173-206 */
    RTC_PATTERN_GRID     = 6  /* material.rs:208-242 */
};
enum { /* render mode */
    RTC_MODE_RENDER       = 0, /* Camera::render: y in 0..vsize-1, x in 0..hsize-1 EXCLUSIVE,
                                  last row and column stay black        camera.rs:116-126 */
    RTC_MODE_RENDER_ASYNC = 1  /* Camera::render_async / render_async1: all pixels
                                                                        camera.rs:128-160 */
};
enum { /* render flags (bit set) */
    RTC_FLAG_NONE      = 0,
    RTC_FLAG_NO_CULL   = 1u << 0, /* visit every object for every ray (plain brute force); the
                                     default culls objects with a conservative bound first and
                                     produces bit-identical results */
    RTC_FLAG_AA_RESAMPLE = 1u << 1, /* antialiasing_samples > 1 only: take render_pixel's adaptive resample branch
                                     (camera.rs:84-92,108-111) on the device, with the counter-based offsets
                                     documented at rtc_camera.samples (the reference draws them from thread_rng).
                                     Without this flag such pixels keep the mean of the 4 fixed sub-samples and are
                                     COUNTED in rtc_stats.pixels_resample, so the caller knows how many differ.      */
    RTC_FLAG_LDS_TABLE = 1u << 2  /* with RTC_FLAG_NO_CULL: loop over the object table STAGED IN LDS by the workgroup (one tile
                                     when it fits, tiles with a barrier each otherwise) instead of fetching the records through
                                     the scalar cache — BASELINE.json north_star's literal kernel, kept for measurement
                                     (bench.py `brute_force_lds`); identical results */
};

#define RTC_MAX_REFLECTIONS 5u /* Camera::MAX_REFLECTIONS camera.rs:31 */
#define RTC_EPSILON 0.00000001 /* Vector::EPSILON         vec.rs:16    */

/* ---- flattened world --------------------------------------------------------------- */

/* Material (material.rs:244-254) with its optional pattern flattened in. */
typedef struct rtc_material {
    uint32_t pattern_kind;   /* RTC_PATTERN_*; NONE <=> Material.pattern == None           */
    uint32_t has_color;      /* Material.color.is_some()                                    */
    double   color[3];
    double   ambient, diffuse, specular, shininess;
    double   reflective;     /* Material.reflectiveness                                     */
    double   transparency;
    double   refractive_index;
    double   pat_inv[16];    /* Pattern.xf_inv (inverse of the pattern transform)           */
    double   pat_a[3];       /* color_a / color_base                                        */
    double   pat_b[3];       /* color_b / color_grid                                        */
} rtc_material;              /* 264 bytes */

/* One shape of World.shapes (shape.rs:633-637). `inv` is what the reference stores in the
 * field misleadingly called `transform` (the INVERSE of the object transform,
 * shape.rs:300,311); `inv_t` is `transform_transpose` (shape.rs:301,312). Both are carried
 * explicitly so that a caller can reproduce the stale-transpose quirk of
 * Plane::set_transform (shape.rs:446-449). */
typedef struct rtc_shape {
    uint32_t     kind;       /* RTC_SPHERE / RTC_PLANE / RTC_CUBE                           */
    uint32_t     world_id;   /* World::add_shape assigns last_world_id+1 (shape.rs:661-667);
                                only compared for equality (shape.rs:127). rtc_world_create
                                numbers the shapes 1..n itself when EVERY id is 0 (what
                                rtc_shape_init leaves), and otherwise honours the ids given:
                                two shapes with the same id are one "container" to
                                compute_refractive, exactly as in the reference. The
                                reference's own ids are u8 and wrap at 256 shapes
                                (shape.rs:287): a caller that passes `get_world_id()` as
                                it is reproduces that domain too.                           */
    double       inv[16];
    double       inv_t[16];
    rtc_material material;
} rtc_shape;                 /* 528 bytes */

/* Light (material.rs:10-31). World has exactly one (shape.rs:635). */
typedef struct rtc_light {
    double intensity[3];
    double position[3];
} rtc_light;

/* Camera (camera.rs:17-27). */
typedef struct rtc_camera {
    uint32_t hsize, vsize;
    double   fov;
    double   half_width, half_height, pixel_size;
    double   view_inv[16];   /* view_transform_inv: inverse of the view matrix camera.rs:35 */
    uint32_t samples;        /* antialiasing_samples (camera.rs:24). 1 = one ray through the pixel
                                centre. ANY other value, 0 included, takes render_pixel's second
                                branch (camera.rs:99-113): the 4 fixed sub-samples at offsets
                                (.25|.75, .25|.75) are averaged (Color::average_over), and if any of
                                them is farther than 0.01 (Euclidean RGB, Color::distance_from
                                color.rs:122-126) from that mean, `samples` MORE rays are traced,
                                appended to the same list and the mean is taken again (resample,
                                camera.rs:84-92). The trigger is deterministic and reproduced
                                exactly; the reference draws the extra offsets from thread_rng
                                (non-reproducible), so the resample itself is only taken with
                                RTC_FLAG_AA_RESAMPLE, with offsets from a documented counter-based
                                generator: for pixel (x, y) and extra sample k = 0..samples-1,
                                  c = (uint64(y)*hsize + x) << 16
                                  x_offset = (splitmix64(c | 2k)   >> 11) * 2^-53
                                  y_offset = (splitmix64(c | 2k+1) >> 11) * 2^-53
                                with splitmix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) *
                                0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB; z ^ z>>31
                                (uniform in [0,1) like rng.gen::<f64>()). samples == 0 resamples
                                zero rays: the mean of the four is recomputed and is the result.
                                Values above 255 are rejected (the reference's field is a u8).       */
    uint32_t _pad;
} rtc_camera;

/* Ray counters. A ray = one call of World::intersect (shape.rs:677). */
typedef struct rtc_stats {
    uint64_t rays_primary;   /* color_at from render_pixel          camera.rs:97-105   */
    uint64_t rays_shadow;    /* is_shadowed, one per shade_hit      shape.rs:688,712   */
    uint64_t rays_reflect;   /* reflected_color recursion           shape.rs:734-735   */
    uint64_t rays_refract;   /* refracted_color recursion           shape.rs:764-765   */
    uint64_t pixels;         /* pixels written by the last render                        */
    uint64_t pixels_resample;/* pixels whose 4 sub-samples trip the resample test
                                (camera.rs:108-111); 0 when samples == 1                 */
    uint64_t rays_primary_proven_miss; /* of rays_primary: primary rays of image tiles the binning kernel PROVED to hit nothing
                                (empty candidate list, cone clear of every plane): counted as cast — the reference casts
                                them — but answered by the proof, no ray is generated for them (one-sample renders of
                                binned launches; 0 otherwise)                                  */
    uint64_t _reserved[1];
} rtc_stats;

/* Per-ray probe record filled by rtc_color_at: the fields of CachedVectors
 * (shape.rs:58-71) for the ray's FIRST hit. hit_index = position in World.shapes
 * (insertion order) or -1. */
typedef struct rtc_hit {
    int32_t  hit_index;
    uint32_t inside;
    uint32_t shadowed;       /* World::is_shadowed(over_point)      shape.rs:712-727   */
    uint32_t _pad;
    double   t;
    double   point[3];
    double   over_point[3];
    double   under_point[3];
    double   eyev[3];
    double   normal[3];
    double   reflectv[3];
    double   n1, n2;         /* compute_refractive; 1.0/1.0 unless the hit material has
                                transparency != 0 (the only case the reference reads them,
                                shape.rs:692,752)                                       */
} rtc_hit;

typedef struct rtc_context rtc_context; /* one GPU + one stream; single-threaded use (N GPUs: rtc_group) */
typedef struct rtc_world   rtc_world;   /* flattened World resident in HBM                */

/* ==== [host] reference-faithful setup arithmetic =================================== */

/* ABI / build identification. Returns RTC_ABI_VERSION. */
uint32_t    rtc_abi_version(void);
const char *rtc_strerror(rtc_status s);

/* Matrix::identity / multiply (transform.rs:44-51, 8-21,31-33). out may alias neither input. */
void        rtc_matrix_identity(double out[16]);
void        rtc_matrix_multiply(const double a[16], const double b[16], double out[16]);
/* Fluent builders: each LEFT-multiplies, `out = new * m` (transform.rs:53-105). out may alias m. */
void        rtc_matrix_translation(const double m[16], double x, double y, double z, double out[16]);
void        rtc_matrix_scaling    (const double m[16], double x, double y, double z, double out[16]);
void        rtc_matrix_rotation_x (const double m[16], double r, double out[16]);
void        rtc_matrix_rotation_y (const double m[16], double r, double out[16]);
void        rtc_matrix_rotation_z (const double m[16], double r, double out[16]);
void        rtc_matrix_shearing   (const double m[16], double xy, double xz, double yx, double yz,
                                   double zx, double zy, double out[16]);
/* Matrix::determinant by cofactor expansion along row 0 (transform.rs:130-169). */
double      rtc_matrix_determinant(const double m[16]);
/* Matrix::inverse, cofactor method; RTC_ERR_SINGULAR when |det| <= 1e-8 (transform.rs:35-38,175-190). */
rtc_status  rtc_matrix_inverse(const double m[16], double out[16]);
void        rtc_matrix_transpose(const double m[16], double out[16]); /* transform.rs:192-202 */
/* Matrix::make_view_transform(from, to, up) (transform.rs:204-217). */
void        rtc_view_transform(const double from[3], const double to[3], const double up[3], double out[16]);

/* Camera::new_with_transform(hsize, vsize, fov, view) (camera.rs:33-58): derives
 * half_width/half_height/pixel_size and stores inverse(view). samples = 1. */
rtc_status  rtc_camera_init(uint32_t hsize, uint32_t vsize, double fov, const double view[16], rtc_camera *out);
/* Camera::ray_for_pixel_offset (camera.rs:64-76); ray = {origin xyz, direction xyz}. */
void        rtc_camera_ray_for_pixel(const rtc_camera *cam, uint32_t x, double x_offset,
                                     uint32_t y, double y_offset, double ray[6]);

/* Material::default() (white, .1/.9/.9/200, 0/0/1.0; material.rs:273-283,364-369). */
void        rtc_material_default(rtc_material *out);
/* {Sphere,Plane,Cube}::new_with_transform_and_material(m, mat) (shape.rs:308-317,436-444,
 * 525-533): inv = m.inverse(), inv_t = inv.transpose(). world_id is left 0. */
rtc_status  rtc_shape_init(uint32_t kind, const double transform[16], const rtc_material *mat, rtc_shape *out);
/* Pattern::set_transform (material.rs:61-63 etc.): mat->pat_inv = inverse(transform). */
rtc_status  rtc_material_set_pattern(rtc_material *mat, uint32_t pattern_kind, const double a[3],
                                     const double b[3], const double transform[16]);
/* Light::default(): white at (-10,10,-10) (material.rs:26-31). */
void        rtc_light_default(rtc_light *out);

/* Scene loader for the `jamis.yml` vocabulary (ch1/jamis.yml:1-183; the reference ships the
 * data file but no loader). Parses `text` (NUL-terminated YAML subset),
 * applies transform lists in listed order (transform.rs:53-69 left-multiplication), starts
 * materials from Material::default() (lua.rs:187) and assigns world ids like
 * World::add_shape. On success *shapes_out is a malloc'ed array the caller releases with
 * rtc_free. Returns the first light (lua.rs:148-150); rtc_scene_load_yaml_lights returns all of them. */
rtc_status  rtc_scene_load_yaml(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                rtc_light *light_out, rtc_camera *camera_out,
                                char *errbuf, size_t errbuf_len);
rtc_status  rtc_scene_load_yaml_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                     rtc_light *light_out, rtc_camera *camera_out,
                                     char *errbuf, size_t errbuf_len);
/* The reference's Lua front-end (ch1/src/lua.rs:50-330; scripts ch1/jamis.lua, ex1.lua, ex2.lua + functions.lua) without a
 * Lua library: csrc/host_lua.cpp interprets the part of Lua 5.3 those scripts are written in (functions and closures,
 * numeric / generic for, while, repeat, if, multiple assignment, tables, integer / float numbers, strings; print, require of
 * files beside the script, math.*, string.format, table.insert ...; no metatables, coroutines, goto or bitwise operators)
 * and gives a script the reference's three entry points:
 *   Render(world, camera, outfile)                              lua.rs:57-71
 *   enc = StartAnimation(outfile); enc:AddFrame(world, camera); enc:Finish()     lua.rs:34-45,75-79
 * Every Render / AddFrame call converts its tables AT THE CALL by lua.rs's own rules — transform_from_table's fixed order
 * rotate_x, rotate_y, rotate_z, scale, position; materials from Material::default() with the keys ambient, diffuse,
 * specular, shininess, reflectiveness, transparency, refractive_index, color, pattern (anything else is an error) and the
 * shape-level color / pattern override; patterns "checks" / "stripes" / "grid"; every light of world.lights (the job's
 * `light` field is lights[1], rtc_lua_program_job_lights hands out all); camera screenwidth /
 * screenheight / samples as Lua integers — and becomes one JOB: a world, a camera, the output file's name. The caller renders
 * the jobs in order (one rtc_render* launch each: an AddFrame loop is the one-camera-per-launch sequence a pipelined
 * context overlaps). The library writes PNG / PPM stills (rtc_canvas_write_png8, rtc_canvas_write_ppm_rgb8) and the
 * animation's GIF (rtc_gif_format, rtc_gif_writer_*, rtc_lua_program_render_gif), JPEG stills (rtc_jpeg_format,
 * rtc_jpeg_encoder_*, rtc_lua_program_render_files) and compressed PNGs (rtc_png_format, rtc_png_encoder_*,
 * rtc_lua_program_render_png).
 * math.random is Lua 5.3's on POSIX (glibc random(), restated), so `math.randomseed(13)` worlds are reproducible.
 * A script runs under a step budget (`step_limit` statements / loop iterations / calls, 0 = 100 000 000), may nest 200 calls
 * (the interpreter recurses on the caller's stack: up to about 2 MB of it at that depth) and cannot touch
 * the file system except through require (`base_dir`/name.lua; NULL = require is an error). Syntax and runtime errors,
 * and tables lua.rs would reject, are RTC_ERR_PARSE with the message in errbuf (the reference unwrap()s: it panics).
 * PARITY UNPINNED: the reference has no test of its Lua path. [host] */
typedef struct rtc_lua_program rtc_lua_program;
enum { RTC_LUA_JOB_RENDER = 0, RTC_LUA_JOB_ADD_FRAME = 1 };
typedef struct rtc_lua_job {
    const rtc_shape *shapes;          /* owned by the program; NULL when the world is empty                            */
    uint32_t         n_shapes;
    uint32_t         kind;            /* RTC_LUA_JOB_RENDER | RTC_LUA_JOB_ADD_FRAME                                    */
    rtc_light        light;
    rtc_camera       camera;
    const char      *outfile;         /* Render's third argument / the animation's file name; owned by the program     */
    uint32_t         animation;       /* AddFrame: which StartAnimation call (0, 1, ...) the encoder came from         */
    uint32_t         frame;           /* AddFrame: index of the frame inside that animation                            */
    uint32_t         same_world_as_previous; /* 1: shapes and ALL lights equal the previous job's byte for byte (same arrays) */
    uint32_t         line;            /* script line of the call                                                      */
} rtc_lua_job;
rtc_status  rtc_lua_run(const char *text, const char *base_dir, uint64_t step_limit, rtc_lua_program **out,
                        char *errbuf, size_t errbuf_len);
rtc_status  rtc_lua_run_file(const char *path, uint64_t step_limit, rtc_lua_program **out, char *errbuf, size_t errbuf_len);
uint32_t    rtc_lua_program_jobs(const rtc_lua_program *prog);
rtc_status  rtc_lua_program_job(const rtc_lua_program *prog, uint32_t index, rtc_lua_job *job);
const char *rtc_lua_program_output(const rtc_lua_program *prog);   /* everything the script print()ed */
void        rtc_lua_program_free(rtc_lua_program *prog);
/* The single-scene form: runs the script as above and hands out job `render_index` (0 = the first Render / AddFrame call;
 * a script that makes none falls back to its globals `world` and `camera`) as a malloc'ed shape array (rtc_free);
 * *renders_out (may be NULL) = how many jobs the script made; `outfile` (may be NULL) receives that job's file name. */
rtc_status  rtc_scene_load_lua(const char *text, uint32_t render_index, rtc_shape **shapes_out, uint32_t *n_out,
                               rtc_light *light_out, rtc_camera *camera_out, char *outfile, size_t outfile_len,
                               uint32_t *renders_out, char *errbuf, size_t errbuf_len);
rtc_status  rtc_scene_load_lua_file(const char *path, uint32_t render_index, rtc_shape **shapes_out, uint32_t *n_out,
                                    rtc_light *light_out, rtc_camera *camera_out, char *outfile, size_t outfile_len,
                                    uint32_t *renders_out, char *errbuf, size_t errbuf_len);
/* All lights of a scene. The _lights forms of the loaders return every `add: light` entry (YAML, file order) / every
 * element of world.lights (Lua, index order) in lights_out[0..*n_lights_out); the forms above keep returning the first.
 * `lights_cap` is the room in lights_out: a scene with more lights than that is RTC_ERR_ARG, one with more than
 * RTC_MAX_LIGHTS is RTC_ERR_PARSE with a message, whichever entry loads it. */
rtc_status  rtc_scene_load_yaml_lights(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                       rtc_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                       rtc_camera *camera_out, char *errbuf, size_t errbuf_len);
rtc_status  rtc_scene_load_yaml_lights_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                            rtc_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                            rtc_camera *camera_out, char *errbuf, size_t errbuf_len);
rtc_status  rtc_scene_load_lua_lights(const char *text, uint32_t render_index, rtc_shape **shapes_out, uint32_t *n_out,
                                      rtc_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                      rtc_camera *camera_out, char *outfile, size_t outfile_len,
                                      uint32_t *renders_out, char *errbuf, size_t errbuf_len);
rtc_status  rtc_scene_load_lua_lights_file(const char *path, uint32_t render_index, rtc_shape **shapes_out, uint32_t *n_out,
                                           rtc_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                           rtc_camera *camera_out, char *outfile, size_t outfile_len,
                                           uint32_t *renders_out, char *errbuf, size_t errbuf_len);
/* Every light of job `index` (rtc_lua_job::light is lights_out[0]). RTC_ERR_ARG when cap is too small. RTC_ERR_PARSE
 * (there is no message buffer here) when the job's world has an area light: rtc_lua_program_job_area_lights hands those
 * out; rtc_lua_job::light is then the area light's first sample. */
rtc_status  rtc_lua_program_job_lights(const rtc_lua_program *prog, uint32_t index, rtc_light *lights_out, uint32_t cap,
                                       uint32_t *n_out);
/* Scenes with area lights (struct rtc_area_light, below). YAML: an `add: light` entry with corner / uvec / vvec / usteps
 * / vsteps / intensity (the book's vocabulary; `jitter: false` is accepted, `jitter: true` is RTC_ERR_PARSE: not
 * supported; `at` together with `corner` is a parse error). Lua: an element of world.lights with the keys corner, uvec,
 * vvec, usteps, vsteps (Lua integers, by the rules of the camera's `samples`) beside `color`. These entries return every
 * light as an rtc_area_light, point lights as the degenerate case; a scene with an area light may hold up to
 * RTC_MAX_LIGHT_SAMPLES samples (more: RTC_ERR_PARSE with a message), one of point lights only RTC_MAX_LIGHTS lights as
 * before. The entries above return RTC_ERR_PARSE for a scene with an area light, with a message naming these. */
struct rtc_area_light;
rtc_status  rtc_scene_load_yaml_area_lights(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                            struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                            rtc_camera *camera_out, char *errbuf, size_t errbuf_len);
rtc_status  rtc_scene_load_yaml_area_lights_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                                 struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                                 rtc_camera *camera_out, char *errbuf, size_t errbuf_len);
rtc_status  rtc_scene_load_lua_area_lights(const char *text, uint32_t render_index, rtc_shape **shapes_out, uint32_t *n_out,
                                           struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                           rtc_camera *camera_out, char *outfile, size_t outfile_len,
                                           uint32_t *renders_out, char *errbuf, size_t errbuf_len);
rtc_status  rtc_scene_load_lua_area_lights_file(const char *path, uint32_t render_index, rtc_shape **shapes_out, uint32_t *n_out,
                                                struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                                rtc_camera *camera_out, char *outfile, size_t outfile_len,
                                                uint32_t *renders_out, char *errbuf, size_t errbuf_len);
/* Scenes whose camera has a thin lens (struct rtc_lens, below). YAML: `add: camera` with `aperture` (>= 0) and
 * `focal-distance` (> 0, required when `aperture` is given), optionally `lens-usteps` / `lens-vsteps` (integers, default 1,
 * at most RTC_MAX_LENS_SAMPLES samples in all). These entries are rtc_scene_load_yaml_area_lights plus the lens:
 * *has_lens_out = 1 and *lens_out filled when the camera has any of those keys, else 0 and the pinhole lens (aperture 0,
 * focal distance 1, 1x1). Every other YAML entry returns RTC_ERR_PARSE for a scene with lens keys, with a message naming
 * these. */
struct rtc_lens;
rtc_status  rtc_scene_load_yaml_lens(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                     struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                     rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                     struct rtc_lens *lens_out, uint32_t *has_lens_out);
rtc_status  rtc_scene_load_yaml_lens_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                          struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                          rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                          struct rtc_lens *lens_out, uint32_t *has_lens_out);
/* Scenes with motion blur (struct rtc_motion, below). YAML: a shape key `motion:` takes a transform list in the
 * `transform:` vocabulary — the shape's transform at the shutter's close is that list applied on top of its `transform:`,
 * by the same left-multiplication (transform_open = the shape's transform) — and `add: camera` takes `shutter-samples`
 * (an integer in 1..RTC_MAX_SHUTTER_SAMPLES, default 1). These entries are rtc_scene_load_yaml_lens plus the motions:
 * *motions_out is a malloc'ed array (rtc_free) of *n_motions_out records in file order, *samples_out the shutter samples.
 * Every other YAML entry returns RTC_ERR_PARSE for a scene with those keys, with a message naming these. The camera does
 * not move in a scene file (rtc_shutter_scene::cam_close is for callers of the C-ABI). */
struct rtc_motion;
rtc_status  rtc_scene_load_yaml_motion(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                       struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                       rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                       struct rtc_lens *lens_out, uint32_t *has_lens_out,
                                       struct rtc_motion **motions_out, uint32_t *n_motions_out, uint32_t *samples_out);
rtc_status  rtc_scene_load_yaml_motion_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                            struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                            rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                            struct rtc_lens *lens_out, uint32_t *has_lens_out,
                                            struct rtc_motion **motions_out, uint32_t *n_motions_out, uint32_t *samples_out);
/* Scenes whose camera has a projection (struct rtc_projection, below). YAML: `add: camera` with `projection: orthographic`
 * and `ortho-width` (> 0, required), or `projection: panorama` with, optionally, `pano-h-span` / `pano-v-span` (radians,
 * defaults 2*pi and pi); `field-of-view` may then be left out (it is not read; pi/2 is stored). These entries are
 * rtc_scene_load_yaml_lens plus the projection: *has_projection_out = 1 and *proj_out filled when the camera has any of
 * those keys, else 0 and *proj_out zeroed. Every other YAML entry returns RTC_ERR_PARSE for a scene with those keys, with a
 * message naming these. A camera with both lens keys and a projection is RTC_ERR_PARSE. Lua cameras stay pinholes. */
struct rtc_projection;
rtc_status  rtc_scene_load_yaml_projection(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                           struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                           rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                           struct rtc_lens *lens_out, uint32_t *has_lens_out,
                                           struct rtc_projection *proj_out, uint32_t *has_projection_out);
rtc_status  rtc_scene_load_yaml_projection_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                                struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                                rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                                struct rtc_lens *lens_out, uint32_t *has_lens_out,
                                                struct rtc_projection *proj_out, uint32_t *has_projection_out);
/* Every light of job `index` as an area light. RTC_ERR_ARG when cap is too small. */
rtc_status  rtc_lua_program_job_area_lights(const rtc_lua_program *prog, uint32_t index, struct rtc_area_light *lights_out,
                                            uint32_t cap, uint32_t *n_out);
void        rtc_free(void *p);

/* Canvas::write_to_file_simple: ASCII PPM P3 (canvas.rs:86-109) with Color::scale's
 * truncating, saturating cast and clamp (color.rs:100-114). `rgb` is a host canvas. */
rtc_status  rtc_canvas_write_ppm(const char *path, const double *rgb, uint32_t width, uint32_t height);
/* The same encoder into memory: returns bytes needed (excluding NUL); writes at most cap. */
size_t      rtc_canvas_format_ppm(const double *rgb, uint32_t width, uint32_t height, char *buf, size_t cap);
/* The same file from a frame that is ALREADY quantised — `rgb8` = height*width*3 bytes, each Color::scale(c, 255), as
 * rtc_render_rgb8 / rtc_render_rows' d_rgb8 deliver it: byte for byte the file rtc_canvas_write_ppm writes for the f64
 * canvas of the same render (canvas.rs:98-104 quantises with the same function). */
rtc_status  rtc_canvas_write_ppm_rgb8(const char *path, const uint8_t *rgb8, uint32_t width, uint32_t height);
size_t      rtc_canvas_format_ppm_rgb8(const uint8_t *rgb8, uint32_t width, uint32_t height, char *buf, size_t cap);
/* Color::scale(c, 255) for n colour components (color.rs:100-114) on the host. */
void        rtc_color_scale255(const double *components, size_t n, uint8_t *out);
/* Canvas::to_imgbuf (canvas.rs:61-79), the pixel buffer behind write_to_file / frame_to_file:
 * RGBA8, each channel Color::scale(c.powf(1/gamma), 255) (color.rs:55-65; the reciprocal taken in
 * f32 as the reference does), alpha 255. Canvas::new sets gamma = 1.0 (canvas.rs:30). `out` holds
 * width*height*4 bytes. Host. */
void        rtc_canvas_to_rgba8(const double *rgb, uint32_t width, uint32_t height, float gamma, uint8_t *out);
/* The quantisation table behind every DEVICE form of to_imgbuf (rtc_render_rgba8, rtc_render_views_rgba8,
 * rtc_canvas_to_rgba8_device, rtc_group_render_host_rgba8). With e = (double)(1.0f / gamma) (color.rs:55-65),
 * out[k-1] = T[k] for k = 1..255: the smallest double c >= +0 with Color::scale(pow(c, e), 255) >= k (+inf when only
 * +inf gets there), found by bisection over the bit patterns of doubles with the host's own pow — the function
 * rtc_canvas_to_rgba8 calls. The device then computes each channel as #{k : T[k] <= c} for c >= +0 (and follows pow's C99
 * Annex F rules for NaN and inputs with the sign bit set), so its bytes are rtc_canvas_to_rgba8's, bit for bit, without
 * evaluating pow. About 16 000 calls of pow per gamma; the device entries build a table once per gamma and context.
 * RTC_ERR_ARG unless gamma is positive and finite. `out` holds 255 doubles. [host] */
rtc_status  rtc_gamma_thresholds(float gamma, double *out);
/* Canvas::write_to_file for a ".png" name (canvas.rs:80-84: to_imgbuf().save(path); the `image` crate encodes by
 * extension): an 8-bit PNG of `pixels` = height*width*channels bytes, channels = 4 (to_imgbuf's RGBA, colour type 6) or 3
 * (the device's Color::scale frame, colour type 2; a decoder supplies alpha 255, which is what to_imgbuf stores). PNG is
 * lossless: decoding gives back exactly these pixels, as it does for the reference's file. No compressor is built in —
 * the zlib stream uses stored blocks, so the file is a little larger than the pixels. GIF and JPEG are below.
 * format: bytes needed; writes at most cap. Host. */
rtc_status  rtc_canvas_write_png8(const char *path, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels);
size_t      rtc_canvas_format_png8(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint8_t *buf, size_t cap);
/* Animated GIF: what StartAnimation(file) / enc:AddFrame(world, camera) write in the reference (lua.rs:17-45,75-79,
 * Canvas::frame_to_file canvas.rs:53-59, the `image` crate's GIF encoder with a 75 ms delay per frame).
 * LAYOUT PARITY UNPINNED: no copy of the reference's encoder is at hand; the layout below is what it is understood to emit,
 * and the quantiser is this project's own (the reference uses NeuQuant, which learns one pixel at a time).
 *   File:  "GIF89a"; logical screen = the first frame's width x height; no global colour table; no loop extension;
 *          then one record per frame; trailer 0x3B.
 *   Record: graphic control extension (disposal 0, no transparency, delay 7 cs = Delay 75 ms / 10, truncated); image
 *          descriptor at (0,0) covering the frame, not interlaced, 256-entry local colour table; the table; LZW minimum
 *          code size 8; the code stream in sub-blocks of at most 255 bytes; a 0-length block.
 * Quantiser, on the frame's 8-bit RGB (Color::scale bytes, as rtc_render_rgb8 delivers them), deterministic:
 *   Exact: a frame of at most 256 distinct colours gets those colours in ascending (r<<16)|(g<<8)|b order, padded with
 *          black; lossless.
 *   Median cut otherwise, over the 32768 bins (r>>3, g>>3, b>>3), each with its pixel count and sums of the 8-bit r, g, b.
 *          A box is always shrunk to the bounding box of its occupied bins; the first is that of all of them. While there
 *          are fewer than 256 boxes: among the boxes holding more than one occupied bin take the one with the most pixels
 *          (ties: the box created first; none left: stop); split it along its longest axis in bins (ties: r, then g, then
 *          b) after the first bin plane p at which 2 * (pixels in planes lo..p) >= the box's pixels, but at most at plane
 *          hi-1; the lower part keeps the box's number, the upper part is the next box. Entry i = box i's mean over its
 *          pixels, per channel (2*sum + n) / (2*n) in integers; entries past the last box are black.
 *   Index: every pixel gets the argmin over all 256 entries of dr*dr + dg*dg + db*db, ties to the lowest index (in the exact
 *          case that is the rank of its colour).
 * Segmented LZW: the index stream is cut into segments of RTC_GIF_SEGMENT indices (the last may be shorter), each
 * encoded on its own with a fresh dictionary — the stream is a clear code (256), segment 0's codes, a clear code, segment
 * 1's codes, ..., the last segment's codes, EOI (257): each segment's terminator is written at that segment's final code
 * width. Codes start at 9 bits; after a code is emitted the dictionary takes the next entry and the width grows by one
 * when the next free code exceeds 2^width (at most 12 bits); when the dictionary holds 4096 codes, a clear code is emitted
 * instead and the dictionary restarts at 9 bits. Segments are packed LSB-first into one stream. A segment of 4096
 * indices keeps a whole frame's worth of encoders running at once (one wave each on the device, 507 for 1920x1080) and
 * is long enough for noise to fill the dictionary inside it (3838 codes).
 * rtc_gif_quantize: palette (768 bytes, 256 RGB entries) and one index per pixel; *used (may be NULL) = the entries that
 * are distinct colours or boxes. rtc_gif_lzw: the packed code stream of `indices` (bytes needed; writes at most cap).
 * rtc_gif_format: the whole file of `nframes` frames of width x height (rgb8, one after the other) — bytes needed, 0 for
 * a size of 0 or above 65535; writes at most cap. Host. */
enum { RTC_GIF_SEGMENT = 4096, RTC_GIF_DELAY_CS = 7 };
rtc_status  rtc_gif_quantize(const uint8_t *rgb8, uint32_t width, uint32_t height, uint8_t *palette, uint8_t *indices, uint32_t *used);
size_t      rtc_gif_lzw(const uint8_t *indices, size_t n, uint8_t *buf, size_t cap);
size_t      rtc_gif_format(const uint8_t *frames, uint32_t nframes, uint32_t width, uint32_t height, uint8_t *buf, size_t cap);
/* JPEG: what Canvas::write_to_file writes for a ".jpg" / ".jpeg" name (canvas.rs:80-84, the `image` crate's encoder at
 * quality 75; Render(world, camera, "jamis.jpg") in jamis.lua).
 * LAYOUT PARITY UNPINNED: no copy of the reference's encoder is at hand; what follows is what it is understood to emit, and
 * byte parity with the reference's files is not claimed. Deterministic:
 *   Input: `pixels` = height*width*channels bytes, channels 3 (Color::scale rows: rtc_render_rgb8, rtc_render_rows' d_rgb8)
 *          or 4 (to_imgbuf's RGBA; alpha is ignored: the same RGB in 3 or 4 channels gives the same file). Width and height
 *          1..65535, quality 1..100; anything else is RTC_ERR_ARG (0 bytes from rtc_jpeg_format).
 *   File:  SOI; APP0 JFIF 1.02 (no density units, density 1:1, no thumbnail); DQT table 0 (luma) and DQT table 1 (chroma),
 *          one segment each, 8-bit entries in zigzag order; SOF0 (baseline, 8-bit, components 1, 2, 3, each sampled 1x1 —
 *          4:4:4 —, quantisation tables 0, 1, 1); four DHT segments with the Annex K.3 tables, DC0, AC0, DC1, AC1; SOS (one
 *          interleaved scan of the three components, tables 0/0, 1/1, 1/1, Ss 0, Se 63, Ah Al 0); the entropy-coded data;
 *          EOI. No restart markers. The 623 bytes in front of the data depend on the size and quality only.
 *   Quantisation tables: libjpeg's scaling of the Annex K.1 tables: s = q < 50 ? 5000 / q : 200 - 2q, entry =
 *          clamp((std * s + 50) / 100, 1, 255), integer arithmetic. rtc_jpeg_quant_tables gives both tables, natural order.
 *   Colour, per pixel, in f32 with the coefficients the f32 quotients written here, evaluated exactly in this order (products
 *          first, sums left to right, no fused multiply-add):
 *              Y  = ((( 76.245/255)*r + (149.685/255)*g) + ( 29.07/255)*b)
 *              Cb = ((((-43.0185/255)*r + (-84.4815/255)*g) + (127.5/255)*b) + 128)
 *              Cr = ((((127.5/255)*r + (-106.7685/255)*g) + (-20.7315/255)*b) + 128)
 *          each converted to a byte by truncation toward zero with saturation (Rust's `as u8`: NaN and negatives -> 0,
 *          >= 255 -> 255).
 *   Blocks: 8x8 per component, MCUs in raster order, each MCU the Y, Cb and Cr blocks of the same pixels; pixels past the
 *          right or bottom edge replicate the last column / row.
 *   DCT:   libjpeg's integer LLM forward DCT (ISLOW: CONST_BITS 13, PASS1_BITS 2, constants round(c * 2^13), DESCALE(x, n)
 *          = (x + 2^(n-1)) >> n arithmetic) of the samples minus 128, rows then columns; the output is scaled by 8.
 *          rtc_jpeg_fdct: that DCT of 64 samples (0..255, natural order, not level-shifted).
 *   Quantised coefficient of DCT output d and table entry q: round(trunc(d / 8) / q) with halves away from zero, computed
 *          as sign(t) * ((2|t| + q) / (2q)), t = trunc(d / 8) — the same number as the f32 ((d/8) as f32 / q as f32).round().
 *          rtc_jpeg_coefficients: every MCU's three blocks of 64 (Y, Cb, Cr, natural order), MCUs in raster order.
 *   Entropy coding: DC predicted per component from the previous MCU's (0 for the first); AC as runs of zeros with ZRL (0xF0)
 *          for runs of 16 and EOB only when the block ends in zeros; bits MSB-first; the last byte padded with 1-bits; every
 *          0xFF byte of the data, the padded one included, followed by 0x00.
 * rtc_jpeg_format: the whole file — bytes needed (0 on bad arguments); writes at most cap. rtc_canvas_write_jpeg: the same to
 * `path`. Host. */
rtc_status  rtc_jpeg_quant_tables(int32_t quality, uint16_t *out);
rtc_status  rtc_jpeg_fdct(const uint8_t *samples, int32_t *out);
rtc_status  rtc_jpeg_coefficients(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, int32_t quality,
                                  int16_t *out);
size_t      rtc_jpeg_format(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, int32_t quality, uint8_t *buf,
                            size_t cap);
rtc_status  rtc_canvas_write_jpeg(const char *path, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                                  int32_t quality);
/* Compressed PNG: a filtered, deflate-coded 8-bit PNG of the same input as rtc_canvas_format_png8 (which stays the stored
 * writer). LAYOUT PARITY UNPINNED: no copy of the reference's `png` / `deflate` crates is at hand, so byte parity with its
 * files is not claimed; its pixels are pinned (PNG is lossless: decoding gives back exactly `pixels`). Deterministic:
 *   Input: `pixels` = height*width*channels bytes, channels 3 (colour type 2) or 4 (colour type 6), bit depth 8, no
 *          interlace; width and height 1..65535. Anything else is RTC_ERR_ARG (0 bytes from rtc_png_format).
 *   Filters (ISO 15948 §9, bpp = channels): every row is filtered with None, Sub, Up, Average and Paeth (row 0's prior row
 *          is zeros); the row takes the filter with the least sum of min(v, 256 - v) over its filtered bytes, ties to the
 *          lower type. The filtered stream (n = height * (1 + width*channels) bytes) is, per row, the type byte and the row.
 *   Segments: the stream is cut into segments of RTC_PNG_SEGMENT bytes (the last may be shorter). Each is one deflate
 *          block; every segment but the last is followed by an empty stored block (a sync flush: 3 bits, zero bits to the
 *          byte, 00 00 FF FF), so every segment starts on a byte; the last block has BFINAL = 1 and is padded with zero bits.
 *   Matches: hash(p) = ((s[p] << 10) ^ (s[p+1] << 5) ^ s[p+2]) & 0x7fff, for p + 3 <= n. The candidates of p are the
 *          RTC_PNG_CHAIN nearest q < p with p - q <= 32768 and hash(q) = hash(p) (every position counts, those inside matches
 *          and in earlier segments included). A candidate's length is the common prefix of s[q..] and s[p..], capped at 258
 *          and at the end of p's segment. L(p) = the longest length >= 3 (ties: the nearest candidate), else 0.
 *   Parse: from the segment's start, at p: if L(p) >= 3 and not L(p+1) > L(p), the match (L(p), its distance) and p += L(p);
 *          otherwise the literal s[p] and p += 1 (zlib's one-step lazy rule).
 *   Block type: stored, fixed or dynamic Huffman, whichever has the fewest bits (exact, without padding or flush); ties go
 *          to stored, then fixed. Stored: 3 bits, zero bits to the byte, LEN, NLEN, the bytes.
 *   Dynamic codes: literal/length (symbols 0..285, end-of-block counted once) and distance codes limited to 15 bits, the
 *          code-length code to 7, built by package-merge: symbols of non-zero count sorted by (count, symbol); the deepest
 *          level lists the leaves, each level above merges the leaves with the pairs of the level below (a leaf first on
 *          equal weight) and keeps its first 2m - 2 items (m symbols used); the top's first 2m - 2 items are taken, each
 *          taken leaf adds one bit, each taken package takes two items of the level below. A code of fewer than two used
 *          symbols gives length 1 to the used one and then to the lowest-numbered unused symbols until two have it (a block
 *          without matches codes distances 0 and 1 with one bit each). Codes are canonical (RFC 1951 §3.2.2).
 *          HLIT = max(257, 1 + the last literal/length symbol with a length), HDIST = max(1, 1 + the last distance symbol
 *          with one), HCLEN = max(4, 1 + the last position of the code-length order with a length). The HLIT + HDIST lengths
 *          are one sequence (runs cross from one code to the other); a run of r equal values v: v = 0: symbol 18 for
 *          min(r, 138) while r >= 11, then 17 if r >= 3, else r zeros; v != 0: v once, then 16 for min(r, 6) while r >= 3,
 *          then v for the rest.
 *   Framing: signature, IHDR, one IDAT chunk per segment, IEND. The first IDAT also carries the zlib header 78 9C in front,
 *          the last the Adler-32 of the filtered stream (big-endian) behind, so each chunk's CRC stands alone.
 *   The file is never larger than n + 22 * segments + 51 bytes (every segment stored).
 * rtc_png_filter: each row's filter type (`types`, height bytes) and the filtered stream (`filtered`, n bytes); either may be
 * null. rtc_png_format: the whole file — bytes needed (0 on bad arguments); writes at most cap. rtc_canvas_write_png: the
 * same to `path`. Host. */
enum { RTC_PNG_SEGMENT = 32768, RTC_PNG_CHAIN = 8 };
rtc_status  rtc_png_filter(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint8_t *types,
                           uint8_t *filtered);
size_t      rtc_png_format(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint8_t *buf, size_t cap);
rtc_status  rtc_canvas_write_png(const char *path, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels);
/* Save by file name: Canvas::write_to_file's `to_imgbuf().save(path)` (canvas.rs:80-84), where the `image` crate picks the
 * codec from the extension. The extension is what follows the last '.' of the name's last component (after the last '/'),
 * compared without regard to case; a component that starts with its only '.' (".png") has none, as in Rust's
 * Path::extension. The table, one for every layer (host, device, Lua, Python, C++):
 *   png                RTC_IMAGE_PNG       rtc_png_format's bytes of the RGB channels (3 channels, colour type 2)
 *   jpg, jpeg          RTC_IMAGE_JPEG      rtc_jpeg_format's bytes at quality 75 (the crate's `save` default)
 *   gif                RTC_IMAGE_GIF       rtc_gif_format's bytes for the one frame (what rtc_gif_writer writes for it)
 *   ppm                RTC_IMAGE_PPM       rtc_canvas_format_ppm_rgb8's bytes (the P3 file of write_to_file_simple)
 *   bmp                RTC_IMAGE_BMP       below
 *   tga                RTC_IMAGE_TGA       below
 *   tif, tiff          RTC_IMAGE_TIFF      below
 *   ico                RTC_IMAGE_ICO       below
 *   ff                 RTC_IMAGE_FARBFELD  below
 *   pam                RTC_IMAGE_PAM       below
 *   anything else, or no extension: RTC_ERR_UNSUPPORTED, and nothing is written.
 * Input: `pixels` = height*width*channels bytes, channels 3 (Color::scale's rows, rtc_render_rgb8) or 4 (to_imgbuf's RGBA,
 * rtc_render_rgba8). Every file is a function of the R, G, B bytes alone and stores alpha 255 where it has alpha (to_imgbuf
 * stores nothing else), so the 3- and the 4-channel form of a frame give the same file, byte for byte. LAYOUT PARITY
 * UNPINNED: the crate's encoders are not at hand, so byte parity with its files is not claimed; pixels are pinned (every
 * format but JPEG, and GIF above 256 colours, is lossless: decoding gives back the R, G, B bytes with alpha 255). The new
 * layouts (all integers little-endian unless stated; no field not listed is written):
 *   BMP:  BITMAPFILEHEADER: "BM", file size (u32), 0 (u32), pixel offset 122 (u32). BITMAPV4HEADER: 108, width, height
 *         (positive: rows stored bottom-up), planes 1 (u16), 32 bpp (u16), BI_BITFIELDS 3, pixel bytes 4*width*height,
 *         resolution 0 and 0, colours used 0, important 0, masks R 0x00FF0000, G 0x0000FF00, B 0x000000FF, A 0xFF000000,
 *         colour space 0x73524742 ("sRGB"), end points and gamma 0 (48 bytes). Pixels B,G,R,A, rows without padding.
 *         Width and height 1..2^31-1; RTC_ERR_ARG when the file size does not fit in a u32.
 *   TGA:  18 bytes: ID length 0, colour map type 0, image type 2, colour map spec 0 (5 bytes), origin 0,0 (u16 each), width,
 *         height (u16), 32 bpp, descriptor 0x28 (8 alpha bits, top-left origin). Pixels B,G,R,A top row first; no ID, no
 *         colour map, no footer. Width and height 1..65535.
 *   TIFF: "II", 42, IFD offset 8; the IFD: 14 entries (u16 count, 12 bytes each, next-IFD offset 0) in tag order:
 *         256 ImageWidth LONG, 257 ImageLength LONG, 258 BitsPerSample SHORT[4] = 8,8,8,8 (at 182), 259 Compression 1,
 *         262 Photometric 2, 273 StripOffsets LONG[S], 277 SamplesPerPixel 4, 278 RowsPerStrip LONG R, 279 StripByteCounts
 *         LONG[S], 282 XResolution RATIONAL 1/1 (at 190), 283 YResolution 1/1 (at 198), 284 PlanarConfiguration 1,
 *         296 ResolutionUnit 1, 338 ExtraSamples 2 (unassociated alpha); SHORT values sit in the low half of the entry's
 *         value field. R = max(1, floor(RTC_TIFF_STRIP_BYTES / (4*width))) rows per strip, S = ceil(height / R) strips, the
 *         last strip holds the rest. S = 1: both arrays' one value is inline; S > 1: StripOffsets at 206, StripByteCounts at
 *         206 + 4S. The strips follow the header (206 + (S > 1 ? 8S : 0) bytes) as one contiguous block of R,G,B,A rows,
 *         top row first. Width and height >= 1; RTC_ERR_ARG when the file size does not fit in a u32.
 *   ICO:  ICONDIR: 0, type 1, count 1 (u16 each); ICONDIRENTRY: width, height (one byte each, 0 = 256), colours 0,
 *         reserved 0, planes 1, 32 bpp (u16 each), bytes of the PNG (u32), its offset 22 (u32); then rtc_png_format's file
 *         of the RGBA frame (4 channels, colour type 6, alpha 255). Width and height 1..256.
 *   farbfeld: "farbfeld", width, height (big-endian u32), then R,G,B,A of each pixel as big-endian u16 v * 257, top row first.
 *   PAM:  "P7\nWIDTH w\nHEIGHT h\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n" (w, h in decimal), then R,G,B,A bytes.
 *   PPM, farbfeld and PAM take any width and height >= 1 whose file size fits in 64 bits; PNG, JPEG and GIF keep their
 *   own limits (1..65535).
 * rtc_image_format_for_name: the table's format for `name` (RTC_ERR_UNSUPPORTED if none; RTC_ERR_ARG for NULL).
 * rtc_image_format: the whole file of `format` — bytes needed (0 on bad arguments or an unknown format); writes at most cap.
 * rtc_canvas_save: that file to `path`, the format from the name; RTC_ERR_UNSUPPORTED before anything is opened. Host. */
enum {
    RTC_IMAGE_PNG = 0, RTC_IMAGE_JPEG = 1, RTC_IMAGE_GIF = 2, RTC_IMAGE_PPM = 3, RTC_IMAGE_BMP = 4, RTC_IMAGE_TGA = 5,
    RTC_IMAGE_TIFF = 6, RTC_IMAGE_ICO = 7, RTC_IMAGE_FARBFELD = 8, RTC_IMAGE_PAM = 9
};
enum { RTC_IMAGE_JPEG_QUALITY = 75, RTC_TIFF_STRIP_BYTES = 65536 };
rtc_status  rtc_image_format_for_name(const char *name, uint32_t *format);
size_t      rtc_image_format(uint32_t format, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                             uint8_t *buf, size_t cap);
rtc_status  rtc_canvas_save(const char *path, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels);

/* ==== [device] the hot path on one MI355X ========================================== */

/* Create a context on HIP device `device`. `stream` is an existing hipStream_t passed as
 * void* (e.g. torch's current stream); NULL is the device's default stream. The context never
 * owns the stream. */
rtc_status  rtc_context_create(int32_t device, void *stream, rtc_context **out);
void        rtc_context_destroy(rtc_context *ctx);
rtc_status  rtc_context_synchronize(rtc_context *ctx);
/* Device facts for reports: name (<= cap bytes), compute units, clock MHz. */
rtc_status  rtc_context_device_info(rtc_context *ctx, char *name, size_t cap,
                                    int32_t *compute_units, int32_t *clock_mhz);

/* World::new(light) + add_shape* (shape.rs:642-667): flatten and upload once; the world
 * stays resident in HBM across renders. Validates materials (RTC_ERR_NO_COLOR). */
rtc_status  rtc_world_create(rtc_context *ctx, const rtc_shape *shapes, uint32_t n_shapes,
                             const rtc_light *light, rtc_world **out);
/* Replace the contents of a resident World of `ctx`: shapes, materials, light and n_shapes may all
 * change. Validates as rtc_world_create does (plus RTC_ERR_ARG for a World of another context); a
 * rejected call leaves the World as it was. Ordered like a launch: every render launched before the
 * call sees the old contents, on whichever lane it runs, every render launched after it the new
 * ones. `shapes` may be freed on return. The derived tables (bounds, Morton order, group spheres,
 * prefilter records, light lists) are rebuilt on the device beside the renders in flight, with the
 * bits a fresh World would hold. The call waits for no render kernel and, while n_shapes is no
 * larger than the World has held and its light lists no larger (the 32 / 256 shape thresholds),
 * allocates no device memory; a growing World waits for the context and reallocates first, and if
 * that fails (RTC_ERR_NOMEM) the World has no contents: renders of it return RTC_ERR_NOMEM until
 * an update succeeds. The first update of a World also creates its build stream, its events and
 * one page-locked staging block. Three scalars of the build are kernel arguments of the render
 * kernels, so the FIRST render launch after an update blocks the host until the build kernels of
 * that update (not any render kernel) have finished and their 32-byte header has arrived. */
rtc_status  rtc_world_update(rtc_context *ctx, rtc_world *w, const rtc_shape *shapes,
                             uint32_t n_shapes, const rtc_light *light);
void        rtc_world_destroy(rtc_world *w);

/* Worlds with several lights. The reference's World holds a list of lights, and its shade_hit uses the first and marks
 * the rest `FIXME -- multiple lights` (shape.rs:642-650, 686). Here a World of lights L[0..n), 1 <= n <= RTC_MAX_LIGHTS,
 * shades with
 *     surface = lighting(L[0], .., is_shadowed_by_light(over_point, L[0]))
 *     for i in 1..n:  surface = surface + lighting(L[i], .., is_shadowed_by_light(over_point, L[i]))    (shape.rs:716)
 * added in f64 in light order; every term carries its own ambient part (the book's multi-light form). Everything after
 * `surface` (reflected_color, refracted_color, the Schlick branch) is as for one light, and n == 1 IS the one-light
 * arithmetic, kernels included: rtc_world_create / rtc_world_update are these calls with n_lights == 1.
 * rtc_stats::rays_shadow counts one ray per light per shade_hit; rtc_hit::shadowed stays L[0]'s. Every render entry
 * takes such a World unchanged (rtc_render*, the rgb8 / rgba8 forms, rtc_render_views*, rtc_color_at, the encoders'
 * _render entries, RTC_FLAG_NO_CULL included, culled and brute-force frames bit-identical). Only L[0] has light-space
 * shadow lists; the further lights' shadow passes take the bundle cull. With n_lights > 1 the measurement-only
 * RTC_FLAG_LDS_TABLE path (and an RTC_SRC override naming an LDS source) is RTC_ERR_UNSUPPORTED. rtc_group_world_*
 * stays single-light. n_lights == 0, n_lights > RTC_MAX_LIGHTS or lights == NULL: RTC_ERR_ARG.
 * rtc_world_update_lights has rtc_world_update's ordering and no-allocation promises; n_lights may change between
 * updates. */
#define RTC_MAX_LIGHTS 8u
rtc_status  rtc_world_create_lights(rtc_context *ctx, const rtc_shape *shapes, uint32_t n_shapes,
                                    const rtc_light *lights, uint32_t n_lights, rtc_world **out);
rtc_status  rtc_world_update_lights(rtc_context *ctx, rtc_world *w, const rtc_shape *shapes, uint32_t n_shapes,
                                    const rtc_light *lights, uint32_t n_lights);
uint32_t    rtc_world_light_count(const rtc_world *w); /* 0 for NULL; the number of SAMPLES of a World of area lights */

/* Area lights: soft shadows. An area light is a rectangle (`corner`, full edge vectors `uvec`, `vvec`) sampled at the
 * centres of a usteps x vsteps grid of cells — the book's area light, written in scene files as corner / uvec / vvec /
 * usteps / vsteps / intensity. It IS exactly usteps*vsteps point lights in the multi-light semantics above: every term
 * carries its own ambient part, terms are summed in f64 in sample order. The arithmetic is f64 without fused
 * multiply-add, in this order, per component:
 *     ucell = uvec / (double)usteps          vcell = vvec / (double)vsteps
 *     for v in 0..vsteps { for u in 0..usteps {
 *         position  = (corner + ucell*(u + 0.5)) + vcell*(v + 0.5)
 *         intensity = intensity / (double)(usteps*vsteps) } }
 * A point light is the degenerate case corner = position, uvec = vvec = 0, 1x1: its single sample is that point light
 * bit for bit. A World's lights are a list of rtc_area_light; its sample list is the concatenation of the expansions in
 * list order, 1..RTC_MAX_LIGHT_SAMPLES samples in all. rtc_area_light_expand is the normative sample list.
 * NO JITTER: samples sit at the cell centres. (The book's jittered form draws a random offset per hit; that is not
 * expressible through the single-light oracle the frames are checked against, and is out of scope.) */
typedef struct rtc_area_light {
    double   intensity[3];
    double   corner[3], uvec[3], vvec[3];   /* full edge vectors of the rectangle */
    uint32_t usteps, vsteps;                /* >= 1 each */
} rtc_area_light;
#define RTC_MAX_LIGHT_SAMPLES 256u
/* [host] The degenerate area light of a point light. */
rtc_status  rtc_area_light_from_point(const rtc_light *light, rtc_area_light *out);
/* [host] The sample list of lights[0..n) into out[0..*n_out). RTC_ERR_ARG (and *n_out = 0): a NULL pointer, n == 0, a
 * step count of 0, more than RTC_MAX_LIGHT_SAMPLES samples in all, or more than `cap`. */
rtc_status  rtc_area_light_expand(const rtc_area_light *lights, uint32_t n, rtc_light *out, uint32_t cap, uint32_t *n_out);
/* [device] rtc_world_create_lights / rtc_world_update_lights for a list of area lights: the same validation (plus
 * rtc_area_light_expand's), ordering and no-allocation promises; the number of samples may change between updates.
 * An expansion of at most RTC_MAX_LIGHTS samples IS the rtc_world_create_lights World of the expanded list: the same
 * kernels, the same kernel-argument path, the same bytes. Above that, samples 1..n-1 live in a device table of 6 doubles
 * per sample — one per World generation, sized for RTC_MAX_LIGHT_SAMPLES when the World is created and written in stream
 * order with the World's other tables — which k_trace's light loop reads instead of its kernel arguments
 * (rtc_launch_info::light_table). Sample 0 keeps the World's light-space shadow lists; rtc_hit::shadowed stays sample
 * 0's; rtc_stats::rays_shadow counts one ray per sample per shade_hit. Every render entry takes such a World unchanged
 * (as above); RTC_FLAG_LDS_TABLE is RTC_ERR_UNSUPPORTED, RTC_FLAG_NO_CULL renders it through the scalar-cache brute
 * force, bit-identical to the culled frame. rtc_group_world_* stays single-light. The environment switch
 * RTC_LIGHT_TABLE=1 (measurement only, read at rtc_context_create) sends Worlds of 2..RTC_MAX_LIGHTS lights through the
 * table kernels too. */
rtc_status  rtc_world_create_area_lights(rtc_context *ctx, const rtc_shape *shapes, uint32_t n_shapes,
                                         const rtc_area_light *lights, uint32_t n_lights, rtc_world **out);
rtc_status  rtc_world_update_area_lights(rtc_context *ctx, rtc_world *w, const rtc_shape *shapes, uint32_t n_shapes,
                                         const rtc_area_light *lights, uint32_t n_lights);

/* Thin-lens camera: depth of field. The camera's rays start on a SQUARE lens of half-width `aperture` in the camera's
 * z = 0 plane (camera space) and meet on the plane in focus, `focal_distance` along -z; the lens is sampled at the centres
 * of a usteps x vsteps grid of cells. A thin-lens pixel IS Color::average_over (color.rs:128-139) of usteps*vsteps ordinary
 * rays, each answered by World::color_at as it stands. For pixel (x, y) and lens sample k = v*usteps + u (v outer, u
 * inner) the ray is, in f64 without fused multiply-add, in exactly this order (the first four lines are
 * Camera::ray_for_pixel_offset with offsets 0.5, camera.rs:65-68):
 *     xoffset = (x + 0.5) * pixel_size            yoffset = (y + 0.5) * pixel_size
 *     world_x = half_width - xoffset              world_y = half_height - yoffset
 *     ucell = (2.0*aperture) / (double)usteps     vcell = (2.0*aperture) / (double)vsteps
 *     lu = -aperture + ucell*(u + 0.5)            lv = -aperture + vcell*(v + 0.5)
 *     origin = transform_point(view_inv, (lu, lv, 0.0))
 *     target = transform_point(view_inv, (world_x*focal_distance, world_y*focal_distance, -focal_distance))
 *     direction = normalize(target - origin)
 * and the pixel's colour is Color::average_over of color_at(ray_k, MAX_REFLECTIONS) for k = 0..n-1 in that order: three
 * sums that start at 0.0, add in k order and are divided once by (double)n. aperture = 0, focal_distance = 1, 1x1 is the
 * pinhole ray of camera.rs:64-76 bit for bit, and its frame is rtc_render's byte for byte.
 * NO JITTER, NO DISC: the lens is a square sampled at its cell centres. A jittered or disc-shaped lens needs random
 * numbers or rejection, which the single-ray oracle the frames are checked against cannot follow; both are out of scope. */
typedef struct rtc_lens {
    double   aperture;        /* half-width of the square lens in camera space, >= 0, finite */
    double   focal_distance;  /* distance of the plane in focus along -z of camera space, > 0, finite */
    uint32_t usteps, vsteps;  /* >= 1 each; usteps*vsteps <= RTC_MAX_LENS_SAMPLES */
} rtc_lens;
#define RTC_MAX_LENS_SAMPLES 256u
/* [host] RTC_ERR_ARG for NULL, a non-finite or negative aperture, a non-positive or non-finite focal distance, a step
 * count of 0, or more than RTC_MAX_LENS_SAMPLES samples; else RTC_OK. */
rtc_status  rtc_lens_validate(const rtc_lens *lens);
/* [host] The normative ray above for pixel (x, y) and lens sample k < usteps*vsteps; ray = {origin xyz, direction xyz}.
 * RTC_ERR_ARG for a NULL pointer, an invalid lens or k out of range. Extends rtc_camera_ray_for_pixel (camera.rs:64-76). */
rtc_status  rtc_lens_ray(const rtc_camera *cam, const rtc_lens *lens, uint32_t x, uint32_t y, uint32_t k, double ray[6]);
/* [device] rtc_render_rows through the lens: same buffers, row range, ordering and pipelining contract (and timing events,
 * rtc_launch_info with lens_samples = usteps*vsteps). cam->samples must be 1 (RTC_ERR_ARG otherwise: anti-aliasing and
 * the lens do not compose); both render modes keep their meaning, RTC_MODE_RENDER's black last row and column included.
 * RTC_FLAG_NO_CULL is bit-identical to the culled frame, RTC_FLAG_LDS_TABLE (or an RTC_SRC override naming an LDS source)
 * is RTC_ERR_UNSUPPORTED, RTC_FLAG_AA_RESAMPLE is ignored. The launch has no binning kernel and no per-view table: tile
 * lists, the black tile-row proof and the per-object primary-ray constants all assume the pinhole origin, so every ray
 * takes the per-wave cull with the lens sample's origin as the shared apex (rtc_launch_info::binned = 0). rtc_stats:
 * rays_primary = pixels written x n, rays_primary_proven_miss = 0, the other counters count what those rays spawn. Every
 * World form works: one light, several, area lights through the light table, updated Worlds. */
rtc_status  rtc_render_lens_rows(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_lens *lens,
                                 uint32_t mode, uint32_t y0, uint32_t y1, void *d_rgb, void *d_rgb8, uint32_t flags);
/* [device] rtc_render / rtc_render_rgb8 through the lens: all rows, copied into host memory. Synchronous; `stats` may be NULL. */
rtc_status  rtc_render_lens(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_lens *lens,
                            uint32_t mode, uint32_t flags, double *rgb, rtc_stats *stats);
rtc_status  rtc_render_lens_rgb8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_lens *lens,
                                 uint32_t mode, uint32_t flags, uint8_t *rgb8, rtc_stats *stats);

/* Orthographic and equirectangular panorama cameras: other primary rays, everything behind the primary hit unchanged. `cam`
 * supplies hsize, vsize and view_inv; fov, half_width, half_height and pixel_size are not read. The ray of pixel (x, y) is,
 * in f64 without fused multiply-add, in exactly this order:
 *   ORTHOGRAPHIC (parallel rays; the first three lines are Camera::new's aspect rule, camera.rs:33-58, with width/2 in
 *   place of tan(fov/2), evaluated once, on the host):
 *     aspect = (double)hsize / (double)vsize
 *     half_w = width / 2.0          (aspect >= 1)    or   (width / 2.0) * aspect   (aspect < 1)
 *     half_h = half_w / aspect      (aspect >= 1)    or   width / 2.0
 *     pixel  = (half_w * 2.0) / (double)hsize
 *     world_x = half_w - (x + 0.5) * pixel           world_y = half_h - (y + 0.5) * pixel
 *     origin    = transform_point(view_inv, (world_x, world_y, 0.0))
 *     direction = normalize(transform_point(view_inv, (world_x, world_y, -1.0)) - origin)
 *   PANORAMA (every ray leaves the camera origin; longitude across the frame, latitude down it). rtc_projection_tables is
 *   the normative statement of the trigonometry, evaluated on the host with the C library's sin and cos:
 *     phi_x   = h_span * (0.5 - ((double)x + 0.5) / (double)hsize)        col[x] = { sin(phi_x), cos(phi_x) }
 *     theta_y = v_span * (0.5 - ((double)y + 0.5) / (double)vsize)        row[y] = { sin(theta_y), cos(theta_y) }
 *     origin    = transform_point(view_inv, (0, 0, 0))
 *     d_cam     = ( row[y].cos * col[x].sin,  row[y].sin,  -(row[y].cos * col[x].cos) )
 *     direction = normalize(transform_point(view_inv, d_cam) - origin)
 *   The frame's centre looks down the camera's -z axis and column 0 is on the side of the pinhole camera's column 0. The
 *   device never evaluates sin or cos: it reads the two tables and multiplies, so its rays are rtc_projection_ray's bit for
 *   bit whatever the machine's libm does.
 * The pixel's colour is World::color_at(ray, MAX_REFLECTIONS) as it stands. */
enum { RTC_PROJ_ORTHOGRAPHIC = 1, RTC_PROJ_PANORAMA = 2 };
typedef struct rtc_projection {
    uint32_t kind;     /* RTC_PROJ_ORTHOGRAPHIC or RTC_PROJ_PANORAMA */
    double   width;    /* orthographic: world-space width of the view, > 0, finite (ignored for panorama) */
    double   h_span;   /* panorama: longitude covered by the frame, radians, 0 < h_span <= 2*pi (ignored for orthographic) */
    double   v_span;   /* panorama: latitude covered, radians, 0 < v_span <= pi */
} rtc_projection;
/* [host] RTC_ERR_ARG for NULL, a kind that is neither; orthographic: a width that is not finite or not > 0; panorama: a span
 * that is NaN, not > 0, or above 2*pi (h_span) / pi (v_span), the doubles nearest to them as M_PI gives them; else RTC_OK. */
rtc_status  rtc_projection_validate(const rtc_projection *p);
/* [host] The normative ray above; ray = {origin xyz, direction xyz}. RTC_ERR_ARG for a NULL pointer, an invalid projection,
 * a canvas without pixels, or (x, y) outside it. */
rtc_status  rtc_projection_ray(const rtc_camera *cam, const rtc_projection *p, uint32_t x, uint32_t y, double ray[6]);
/* [host] The panorama's tables: col[hsize][2] and row[vsize][2], {sin, cos} each. RTC_ERR_ARG for a NULL pointer, an invalid
 * projection, a canvas without pixels, or the orthographic kind (it has no tables). */
rtc_status  rtc_projection_tables(const rtc_camera *cam, const rtc_projection *p, double *col, double *row);
/* [device] rtc_render_rows with the projection's rays: same buffers, row range, ordering and pipelining contract (and timing
 * events; rtc_context_last_launch_projection reports the kind, rtc_launch_info lens_samples = 0 and binned = 0). cam->samples must be 1 (RTC_ERR_ARG
 * otherwise); both render modes keep their meaning, RTC_MODE_RENDER's black last row and column included. RTC_FLAG_NO_CULL
 * is byte-identical to the culled frame, RTC_FLAG_LDS_TABLE (or an RTC_SRC override naming an LDS source) is
 * RTC_ERR_UNSUPPORTED, RTC_FLAG_AA_RESAMPLE is ignored. The launch is planned as a thin-lens launch of one sample: no
 * binning kernel, no per-view table, one workgroup per tile. A panorama's primary rays take the per-wave cull with the
 * camera origin as the shared apex (a tile too wide to bound, near the poles or in a small frame, tests every object); an
 * orthographic tile's bundle has its apex at one lane's origin and its spread measured. rtc_stats: rays_primary = pixels
 * written, rays_primary_proven_miss = 0. Every World form works: one light, several, area lights through the light table,
 * updated Worlds.
 * The panorama's tables live in two grow-only device buffers of the context, keyed by (hsize, vsize, h_span, v_span) and
 * uploaded only when the key changes. Before such an upload the context WAITS for all its streams (every pipeline lane and
 * the in-order stream), so no launch in flight still reads the tables that are overwritten; a loop that renders one
 * panorama size never uploads, or waits, after its first frame. */
rtc_status  rtc_render_projection_rows(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                       uint32_t mode, uint32_t y0, uint32_t y1, void *d_rgb, void *d_rgb8, uint32_t flags);
/* [device] rtc_render / rtc_render_rgb8 with the projection's rays: all rows, copied into host memory. Synchronous; `stats` may be NULL. */
rtc_status  rtc_render_projection(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                  uint32_t mode, uint32_t flags, double *rgb, rtc_stats *stats);
rtc_status  rtc_render_projection_rgb8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                       uint32_t mode, uint32_t flags, uint8_t *rgb8, rtc_stats *stats);

/* Motion blur: shutter-averaged frames. A motion-blurred frame IS Color::average_over (color.rs:128-139) of n ordinary
 * frames of the World at n shutter times, the cell centres of the shutter interval [0, 1]:
 *     t_k = ((double)k + 0.5) / (double)n                    k = 0..n-1, 1 <= n <= RTC_MAX_SHUTTER_SAMPLES
 *     lerp(a, b, t) = (a == b) ? a : a + (b - a) * t         per matrix element, f64, no fused multiply-add (an element
 *                                                            that does not move keeps its bits, signed zeros included)
 * Sub-frame k of a scene (shapes, motions, lights, cam_open, cam_close, lens, n):
 *   - a shape without a motion record is used verbatim, its `inv` / `inv_t` (and a stale transpose) included;
 *   - a shape with one keeps kind, world_id and material; inv = rtc_matrix_inverse(M_k) with M_k[i] = lerp(open[i],
 *     close[i], t_k) and inv_t = transpose(inv): what rtc_shape_init computes from M_k. An index out of range or a shape
 *     named twice is RTC_ERR_ARG, a singular M_k for any k RTC_ERR_SINGULAR;
 *   - cam_close == NULL is a static camera; otherwise both cameras agree in every field but view_inv (else RTC_ERR_ARG)
 *     and cam_k is cam_open with view_inv[i] = lerp(open, close, t_k);
 *   - the lights (rtc_area_light, the general World form; rtc_area_light_from_point for point lights) do not move;
 *   - the sub-frame is rtc_render of that World and camera, or rtc_render_lens with a lens (cam->samples must then be 1).
 * The frame is, per component, a sum that starts at 0.0, adds sub-frames 0..n-1 in that order and is divided once by
 * (double)n. NO JITTER: the shutter times are the cell centres. INTERPOLATION IS ELEMENT-WISE: translations and scalings
 * are followed exactly, a rotation is sheared between its end points (the chord, not the arc) — keep the shutter short
 * against the rotation, or cut the move into several frames. */
#define RTC_MAX_SHUTTER_SAMPLES 256u
#define RTC_SHUTTER_RING 8u            /* sub-frame canvases a shutter keeps on the device */
typedef struct rtc_motion {            /* one moving shape */
    uint32_t shape;                    /* index into the shape list */
    uint32_t _pad;
    double   transform_open[16];       /* the OBJECT transform (not its inverse) at t = 0 */
    double   transform_close[16];      /* ... at t = 1 */
} rtc_motion;
/* [host] t_k above; NaN unless k < n <= RTC_MAX_SHUTTER_SAMPLES. */
double      rtc_shutter_time(uint32_t n, uint32_t k);
/* [host] The shapes of sub-frame k into out[0..n_shapes) (out may not overlap shapes). RTC_ERR_ARG: a NULL pointer
 * (motions may be NULL when n_motions == 0), samples outside 1..RTC_MAX_SHUTTER_SAMPLES, k >= samples, a motion index out
 * of range or named twice. RTC_ERR_SINGULAR: M_k of a moving shape has no inverse. */
rtc_status  rtc_shutter_shapes(const rtc_shape *shapes, uint32_t n_shapes, const rtc_motion *motions, uint32_t n_motions,
                               uint32_t samples, uint32_t k, rtc_shape *out);
/* [host] The camera of sub-frame k. close == NULL: *out = *open. RTC_ERR_ARG: NULL open / out, samples or k as above,
 * cameras that differ in anything but view_inv. */
rtc_status  rtc_shutter_camera(const rtc_camera *open, const rtc_camera *close, uint32_t samples, uint32_t k, rtc_camera *out);
/* [host] Color::average_over of n frames: `frames` = n consecutive frames of `count` doubles; out[i] = (((0.0 +
 * frames[0][i]) + frames[1][i]) + ...) / (double)n. A mean that is a NaN is stored as the quiet NaN 0x7FF8000000000000:
 * IEEE 754 leaves the sign and payload of a NaN to the platform (inf - inf is negative on x86-64 and positive on gfx950),
 * and host and device must agree in every byte. n = 1..RTC_MAX_SHUTTER_SAMPLES; n = 0, n above that or a NULL pointer is
 * RTC_ERR_ARG. out may not overlap frames. */
rtc_status  rtc_canvas_average(const double *frames, uint32_t n, size_t count, double *out);
/* [device] The same bytes as rtc_canvas_average for frames already in device memory (8-byte aligned), by k_average_over
 * (csrc/rtc_shutter.hip): RTC_SHUTTER_RING frames per pass, added in sample order to the sum carried in d_out. Enqueued on
 * the context's stream (after launches of a pipelined context: rtc_context_fence first). d_out must not overlap the frames. */
rtc_status  rtc_canvas_average_device(rtc_context *ctx, const void *d_frames, uint32_t n, size_t count, void *d_out);
/* [device] A shutter is bound to a context, like the encoders. It owns a World of its own, created by its first frame and
 * kept current with rtc_world_update_area_lights (the caller's Worlds are never touched), and grow-only scratch of at most
 * RTC_SHUTTER_RING f64 sub-frame canvases, one f64 sum canvas and the 8-bit output, however many samples are asked for.
 * The sub-frames are ordinary launches (rtc_render_rows / rtc_render_lens_rows), back to back on the device — on the
 * lanes of a pipelined context — into the ring; whenever the ring is full, and behind the last sub-frame, ONE pass of
 * k_average_over adds the ring to the sum in sample order, and the last pass divides and writes the outputs asked for:
 * only the finished mean, or its 8-bit form, crosses PCIe. The whole scene is validated for every k before anything is
 * launched. rtc_stats counters are the sums over the sub-frames, `pixels` included; rtc_launch_info describes the last
 * sub-frame's launch. Flags follow the sub-frame entry: RTC_FLAG_NO_CULL gives the same bytes, RTC_FLAG_LDS_TABLE with a
 * lens or several lights is RTC_ERR_UNSUPPORTED.
 *   render / render_rgb8 / render_rgba8: the mean in host memory — vsize*hsize*3 doubles, Color::scale of the mean
 *     (vsize*hsize*3 bytes) or to_imgbuf of the mean at `gamma` (vsize*hsize*4 bytes). Synchronous; `stats` may be NULL.
 *   render_device: any non-empty subset of the three outputs into DEVICE buffers (d_rgb 8-byte aligned); `gamma` is read
 *     only with d_rgba8. An 8-bit-only caller's f64 mean is never written to HBM. The result is ordered on the context's
 *     stream: rtc_image_encoder_encode_device may follow directly. */
typedef struct rtc_shutter_scene {
    const rtc_shape      *shapes;  uint32_t n_shapes;
    const rtc_motion     *motions; uint32_t n_motions;  /* motions may be NULL when n_motions == 0 */
    const rtc_area_light *lights;  uint32_t n_lights;
    const rtc_camera     *cam_open, *cam_close;         /* cam_close may be NULL */
    const rtc_lens       *lens;                         /* may be NULL */
    uint32_t              samples;                      /* 1..RTC_MAX_SHUTTER_SAMPLES */
    uint32_t              _pad;
} rtc_shutter_scene;             /* 80 bytes */
typedef struct rtc_shutter rtc_shutter;
rtc_status  rtc_shutter_create(rtc_context *ctx, rtc_shutter **out);
void        rtc_shutter_destroy(rtc_shutter *s);
rtc_status  rtc_shutter_render(rtc_shutter *s, const rtc_shutter_scene *scene, uint32_t mode, uint32_t flags, double *rgb,
                               rtc_stats *stats);
rtc_status  rtc_shutter_render_rgb8(rtc_shutter *s, const rtc_shutter_scene *scene, uint32_t mode, uint32_t flags, uint8_t *rgb8,
                                    rtc_stats *stats);
rtc_status  rtc_shutter_render_rgba8(rtc_shutter *s, const rtc_shutter_scene *scene, uint32_t mode, uint32_t flags, float gamma,
                                     uint8_t *rgba8, rtc_stats *stats);
rtc_status  rtc_shutter_render_device(rtc_shutter *s, const rtc_shutter_scene *scene, uint32_t mode, uint32_t flags, float gamma,
                                      void *d_rgb, void *d_rgb8, void *d_rgba8);

/* Camera::render / render_async for canvas rows [y0, y1) into a DEVICE buffer of
 * (y1-y0)*hsize*3 doubles (row y0 first). Enqueues on the context stream and returns
 * without synchronising. Row-tiling hook for multi-GPU (each rank renders its rows).
 * d_rgb8 (may be NULL): additionally receives the same rows quantised to 8 bits per channel,
 * (y1-y0)*hsize*3 bytes, exactly as the reference's file writers quantise a Canvas
 * (Color::scale(c, 255): truncating saturating cast, clamp; color.rs:100-114, canvas.rs:104).
 * d_rgb may be NULL when d_rgb8 is not: then only the 8-bit rows are written (24 B/pixel of HBM
 * writes less); the same holds for rtc_render_bands and rtc_render_views. */
rtc_status  rtc_render_rows(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam,
                            uint32_t mode, uint32_t y0, uint32_t y1, void *d_rgb, void *d_rgb8,
                            uint32_t flags);
/* Interleaved row tiles (multi-GPU load balance). The canvas is cut into bands of RTC_BAND_ROWS
 * rows (band b = rows [8b, 8b+8) of the image, the last one possibly short); this call renders
 * bands first_band, first_band + band_stride, first_band + 2*band_stride, ... and packs them one
 * after the other into d_rgb / d_rgb8 (the k-th band of this call at rows [8k, 8k+8) of the
 * buffer; buffers hold ceil((nbands - first_band) / band_stride) * 8 rows). With one process per
 * GPU, rank r of N calls (first_band = r, band_stride = N): every rank gets an even share of sky,
 * floor and objects, where contiguous ranges of rows (rtc_render_rows) leave the ranks with the
 * sky idle. Same per-pixel contract as rtc_render_rows (camera.rs:151-156). [device] */
#define RTC_BAND_ROWS 8u
rtc_status  rtc_render_bands(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam,
                             uint32_t mode, uint32_t first_band, uint32_t band_stride,
                             void *d_rgb, void *d_rgb8, uint32_t flags);
/* Several cameras, one World, ONE launch: the frames of a camera move over a static scene (the
 * reference's AddFrame loop orbits the camera, lua.rs / functions.lua:3-11), a stereo pair, or — with
 * one process per GPU — several frames' worth of one rank's bands, so that a launch fills the chip
 * even when a rank owns an eighth of the image. `cams[0..nviews)` must agree in hsize, vsize and
 * samples; nviews <= RTC_MAX_VIEWS_PER_LAUNCH. Rows are selected as in rtc_render_bands
 * (first_band = 0, band_stride = 1 for whole frames); view v is written `v * view_rows` rows
 * below view 0 in d_rgb / d_rgb8 (view_rows >= the rows one view produces). Per pixel the result is
 * exactly that of rtc_render_bands with the same camera. [device] */
#define RTC_MAX_VIEWS_PER_LAUNCH 8u
rtc_status  rtc_render_views(rtc_context *ctx, const rtc_world *w, const rtc_camera *cams, uint32_t nviews,
                             uint32_t mode, uint32_t first_band, uint32_t band_stride,
                             void *d_rgb, void *d_rgb8, uint32_t view_rows, uint32_t flags);
/* Camera::render(&World) -> Canvas with host memory: renders all rows and copies the
 * canvas into `rgb` (vsize*hsize*3 doubles). Synchronous. `stats` may be NULL. */
rtc_status  rtc_render(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam,
                       uint32_t mode, uint32_t flags, double *rgb, rtc_stats *stats);
/* Camera::render(&World) for a caller that only WRITES THE IMAGE (every file writer of the reference consumes
 * Color::scale'd bytes and nothing else: PPM canvas.rs:86-109, to_imgbuf canvas.rs:61-79 with gamma 1): renders all
 * rows and copies only the 8-bit frame — vsize*hsize*3 bytes, Color::scale(c, 255) of every component, evaluated on
 * the device bit-exactly (color.rs:100-114) — into `rgb8`: 3 bytes per pixel cross PCIe instead of 24, and the f64
 * canvas is not even written to HBM. Feed it to rtc_canvas_write_ppm_rgb8. Synchronous. `stats` may be NULL. */
rtc_status  rtc_render_rgb8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam,
                            uint32_t mode, uint32_t flags, uint8_t *rgb8, rtc_stats *stats);
/* Camera::render(&World) followed by canvas.set_gamma(gamma) and canvas.write_to_file(name) — to_imgbuf
 * (canvas.rs:61-79): RGBA8, each channel Color::scale(c.powf(1/gamma), 255) with the reciprocal taken in f32
 * (color.rs:55-65), alpha 255. Renders all rows, quantises them on the device in the render kernel's epilogue through the
 * gamma's threshold table (rtc_gamma_thresholds) and copies only vsize*hsize*4 bytes into `rgba8`: byte for byte what
 * rtc_canvas_to_rgba8 gives for the f64 canvas of rtc_render, which is never written to HBM. Feed it to
 * rtc_canvas_write_png8 with channels = 4. gamma = 1.0 gives Color::scale's channels (rtc_render_rgb8's bytes) with alpha.
 * RTC_ERR_ARG unless gamma is positive and finite. Synchronous. `stats` may be NULL. [device] */
rtc_status  rtc_render_rgba8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                             float gamma, uint8_t *rgba8, rtc_stats *stats);
/* rtc_render_views with to_imgbuf's RGBA at `gamma` as its only output: view v's rows land `v * view_rows` rows below
 * view 0 in the DEVICE buffer d_rgba8, 4 bytes per pixel; rows, bands and views follow rtc_render_views' rules exactly
 * (one view with first_band = 0, band_stride = 1 is a whole frame). Enqueues and returns; in a pipelined context the
 * launches of different gammas may be in flight together (each gamma's table is uploaded once and never overwritten
 * while a launch may read it). [device] */
rtc_status  rtc_render_views_rgba8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cams, uint32_t nviews, uint32_t mode,
                                   uint32_t first_band, uint32_t band_stride, float gamma, void *d_rgba8, uint32_t view_rows,
                                   uint32_t flags);
/* to_imgbuf (canvas.rs:61-79) of a canvas ALREADY IN DEVICE MEMORY — the reference's own order of calls, where the gamma
 * is chosen after the render: `d_rgb` = rows*width*3 doubles (8-byte aligned), `d_rgba8` = rows*width*4 bytes; the same
 * bytes as rtc_canvas_to_rgba8 on the host. Enqueued on the context's stream, in order with what the caller put there
 * before (after launches of a pipelined context: rtc_context_fence first). RTC_ERR_ARG unless gamma is positive and
 * finite. [device] */
rtc_status  rtc_canvas_to_rgba8_device(rtc_context *ctx, const void *d_rgb, uint32_t width, uint32_t rows, float gamma,
                                       void *d_rgba8);
/* render_lua (lua.rs:50-91) for an interpreted script: renders every job of `prog` in order — one launch per Render /
 * AddFrame call, 8-bit rows only (what the reference's file writers consume), a new device World whenever a job's world
 * differs from the previous one — and hands each frame (vsize*hsize*3 bytes, Color::scale, valid during the call only) to
 * `fn` in job order. The launches are pipelined over the context's lanes (depth 3 for the duration when the context is in
 * order) with each frame's copy to the host on its own lane: an AddFrame loop is the one-camera-per-launch sequence of
 * Camera::render_async calls. A non-zero return from `fn` stops the rendering (RTC_OK). `stats` (may be NULL) = the ray
 * counts of all frames. Blocking. [device] */
typedef int (*rtc_lua_frame_fn)(void *user, const rtc_lua_job *job, uint32_t job_index, const uint8_t *rgb8);
rtc_status  rtc_lua_program_render(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags,
                                   rtc_lua_frame_fn fn, void *user, rtc_stats *stats);
/* The GIF writer on the device: the same bytes as rtc_gif_format, frame by frame, with quantiser and LZW on the GPU
 * (csrc/rtc_gif.hip) — only the compressed record of a frame crosses PCIe. A writer is bound to a context and owns its
 * scratch (about 3 MB + 4 B per pixel, grow-only).
 *   append_device: `d_rgb8` = height*width*3 bytes in device memory (rtc_render_rows' d_rgb8 rows), encoded on the
 *     context's stream in order with what the caller put there before (after launches of a pipelined context:
 *     rtc_context_fence first); blocks until the record is on the host.
 *   render: renders `cam` through the rows path (8-bit rows only) into the writer's scratch and appends that frame; the
 *     frame never leaves the device.
 *   The first frame fixes the logical screen; a later frame of another size, or a size above 65535, is RTC_ERR_ARG.
 *   bytes: the file so far with its trailer (bytes needed; writes at most cap; 0 before the first frame); write: the same
 *     to `path`. [device] */
typedef struct rtc_gif_writer rtc_gif_writer;
rtc_status  rtc_gif_writer_create(rtc_context *ctx, rtc_gif_writer **out);
rtc_status  rtc_gif_writer_append_device(rtc_gif_writer *g, const void *d_rgb8, uint32_t width, uint32_t height);
rtc_status  rtc_gif_writer_render(rtc_gif_writer *g, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags);
size_t      rtc_gif_writer_bytes(const rtc_gif_writer *g, uint8_t *buf, size_t cap);
rtc_status  rtc_gif_writer_write(const rtc_gif_writer *g, const char *path);
void        rtc_gif_writer_destroy(rtc_gif_writer *g);
/* rtc_lua_program_render with the animations encoded on the device: the same launches, lanes and job order, but for an
 * AddFrame job the frame is quantised and LZW-coded on the GPU behind its render (on the same lane) and `fn` receives that
 * frame's GIF record (extension + descriptor + table + sub-blocks, nbytes of them) instead of the 8-bit rows; a Render
 * job is delivered as by rtc_lua_program_render (rows, nbytes = vsize*hsize*3). A file is the 13-byte header of its first
 * frame, its records in order, 0x3B. The record's size is known only on the device: its length (8 bytes) is copied
 * behind each frame, and when the frame is delivered exactly that many bytes follow on a copy stream of this call — no
 * worst-case buffer crosses PCIe, and the lanes keep rendering meanwhile. [device] */
typedef int (*rtc_lua_gif_fn)(void *user, const rtc_lua_job *job, uint32_t job_index, const uint8_t *bytes, size_t nbytes);
rtc_status  rtc_lua_program_render_gif(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags,
                                       rtc_lua_gif_fn fn, void *user, rtc_stats *stats);
/* The JPEG writer on the device: the same bytes as rtc_jpeg_format for a frame already in device memory (csrc/rtc_jpeg.hip);
 * only the finished file crosses PCIe. An encoder is bound to a context and owns its scratch, grow-only and sized from the
 * worst case of a block (22 + 63 * 26 + 3 * 11 + 4 = 1697 entropy-coded bits, doubled by byte stuffing at most), so no input
 * can overflow it: about 2.3 KB per 8x8 pixels (for 1920x1080, 75 MB).
 *   encode_device: `d_pixels` = height*width*channels bytes in device memory (rtc_render_rows' d_rgb8 rows, channels 3, or
 *     rtc_render_views_rgba8's frame, channels 4), encoded on the context's stream in order with what the caller put there
 *     before (after launches of a pipelined context: rtc_context_fence first); blocks until the file is on the host.
 *   render: Camera::render + set_gamma(gamma) + write_to_file("x.jpg"): at gamma 1 through the rows path (3 channels), at
 *     any other gamma through rtc_render_views_rgba8 (4 channels), into the encoder's scratch; the frame never leaves the
 *     device. The bytes equal rtc_jpeg_format of rtc_render_rgba8(..., gamma).
 *   bytes: the last file (bytes needed; writes at most cap; 0 before the first); write: the same to `path`. [device] */
typedef struct rtc_jpeg_encoder rtc_jpeg_encoder;
rtc_status  rtc_jpeg_encoder_create(rtc_context *ctx, rtc_jpeg_encoder **out);
rtc_status  rtc_jpeg_encoder_encode_device(rtc_jpeg_encoder *e, const void *d_pixels, uint32_t width, uint32_t height,
                                           uint32_t channels, int32_t quality);
rtc_status  rtc_jpeg_encoder_render(rtc_jpeg_encoder *e, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                                    float gamma, int32_t quality);
size_t      rtc_jpeg_encoder_bytes(const rtc_jpeg_encoder *e, uint8_t *buf, size_t cap);
rtc_status  rtc_jpeg_encoder_write(const rtc_jpeg_encoder *e, const char *path);
void        rtc_jpeg_encoder_destroy(rtc_jpeg_encoder *e);
/* rtc_lua_program_render_gif with every file of the reference delivered: the same launches, lanes and job order; `fn`
 * receives, per job, `format` and its bytes —
 *   RTC_LUA_OUT_GIF_RECORD  an AddFrame job's GIF record (as rtc_lua_program_render_gif delivers it);
 *   RTC_LUA_OUT_JPEG        a Render job whose file name ends in ".jpg" or ".jpeg" (any case): the whole JPEG file of its
 *                           rows at `quality`, encoded on the GPU behind the render on the same lane (rtc_jpeg_format's bytes);
 *   RTC_LUA_OUT_RGB8        any other Render job: the 8-bit rows, nbytes = vsize*hsize*3.
 * Encoded outputs cross PCIe as their 8-byte length, then exactly that many bytes. RTC_ERR_ARG unless quality is 1..100.
 * [device] */
enum { RTC_LUA_OUT_RGB8 = 0u, RTC_LUA_OUT_GIF_RECORD = 1u, RTC_LUA_OUT_JPEG = 2u };
typedef int (*rtc_lua_file_fn)(void *user, const rtc_lua_job *job, uint32_t job_index, uint32_t format, const uint8_t *bytes,
                               size_t nbytes);
rtc_status  rtc_lua_program_render_files(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags,
                                         int32_t quality, rtc_lua_file_fn fn, void *user, rtc_stats *stats);
/* The compressed PNG writer on the device: the same bytes as rtc_png_format for a frame already in device memory
 * (csrc/rtc_png.hip); only the finished file crosses PCIe. An encoder is bound to a context and owns its scratch, grow-only
 * and sized from the input (no segment costs more than its stored form): about 11 bytes per filtered byte.
 *   encode_device / render / bytes / write / destroy: as rtc_jpeg_encoder_* (render at gamma 1 through the rows path with
 *     3 channels, at any other gamma through rtc_render_views_rgba8 with 4; its bytes equal rtc_png_format of
 *     rtc_render_rgba8(..., gamma)). [device] */
typedef struct rtc_png_encoder rtc_png_encoder;
rtc_status  rtc_png_encoder_create(rtc_context *ctx, rtc_png_encoder **out);
rtc_status  rtc_png_encoder_encode_device(rtc_png_encoder *e, const void *d_pixels, uint32_t width, uint32_t height,
                                          uint32_t channels);
rtc_status  rtc_png_encoder_render(rtc_png_encoder *e, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                                   float gamma);
size_t      rtc_png_encoder_bytes(const rtc_png_encoder *e, uint8_t *buf, size_t cap);
rtc_status  rtc_png_encoder_write(const rtc_png_encoder *e, const char *path);
void        rtc_png_encoder_destroy(rtc_png_encoder *e);
/* rtc_lua_program_render with the files LuaProgram.render_to_files writes, the PNGs compressed on the GPU: the same
 * launches, lanes and job order as rtc_lua_program_render_gif; `fn` receives, per job —
 *   RTC_LUA_OUT_PNG   an AddFrame job, or a Render job whose file name does not end in ".ppm" (any case): the whole file
 *                     (rtc_png_format's bytes of its rows, 3 channels), encoded behind the render on the same lane;
 *   RTC_LUA_OUT_RGB8  a Render job named ".ppm": the 8-bit rows, nbytes = vsize*hsize*3.
 * The file crosses PCIe as its 8-byte length, then exactly that many bytes. [device] */
enum { RTC_LUA_OUT_PNG = 3u };
rtc_status  rtc_lua_program_render_png(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags,
                                       rtc_lua_file_fn fn, void *user, rtc_stats *stats);
/* The save-by-name writer on the device: rtc_image_format's bytes for a frame already in device memory (csrc/rtc_image.hip,
 * csrc/rtc_encode.cpp); only what the device made crosses PCIe, in one copy behind its 8-byte length. BMP, TGA, TIFF,
 * farbfeld and PAM are packed by one kernel (header computed on the host, written by the kernel with the pixels); ICO is the
 * PNG chain (4 channels) behind its header; PNG, JPEG and GIF are their chains (the JPEG and GIF headers, the GIF trailer
 * and the ICO header are written on the host); PPM is the one text format, and its 3 bytes per pixel cross PCIe and are
 * printed on the host (the P3 text is about four times as large). An encoder is bound to a context and owns its scratch,
 * grow-only.
 *   encode_device: `d_pixels` = height*width*channels bytes in device memory, channels 3 or 4, encoded as `format` on the
 *     context's stream in order with what the caller put there before (after launches of a pipelined context:
 *     rtc_context_fence first); blocks until the file is on the host.
 *   render: Camera::render + set_gamma(gamma) + save: at gamma 1 through the rows path (3 channels), at any other gamma
 *     through rtc_render_views_rgba8 (4 channels), into the encoder's scratch; the bytes equal rtc_image_format of
 *     rtc_render_rgba8(..., gamma).
 *   bytes: the last file (bytes needed; writes at most cap; 0 before the first); write: the same to `path`. [device] */
typedef struct rtc_image_encoder rtc_image_encoder;
rtc_status  rtc_image_encoder_create(rtc_context *ctx, rtc_image_encoder **out);
rtc_status  rtc_image_encoder_encode_device(rtc_image_encoder *e, uint32_t format, const void *d_pixels, uint32_t width,
                                            uint32_t height, uint32_t channels);
rtc_status  rtc_image_encoder_render(rtc_image_encoder *e, uint32_t format, const rtc_world *w, const rtc_camera *cam,
                                     uint32_t mode, uint32_t flags, float gamma);
size_t      rtc_image_encoder_bytes(const rtc_image_encoder *e, uint8_t *buf, size_t cap);
rtc_status  rtc_image_encoder_write(const rtc_image_encoder *e, const char *path);
void        rtc_image_encoder_destroy(rtc_image_encoder *e);
/* rtc_lua_program_render with every file of the script saved by its name: the same launches, lanes and job order as
 * rtc_lua_program_render_gif; `fn` receives, per job —
 *   RTC_LUA_OUT_FILE        a Render job: the whole file the save table gives its name (rtc_image_format's bytes of its
 *                           rows), encoded on the GPU behind the render on the same lane (PPM: printed on the host); a
 *                           name of the float table (hdr, pfm, exr — consulted first, see "float files" below): the job
 *                           renders its f64 canvas instead and the file is rtc_float_format's bytes of it (EXR: HALF);
 *   RTC_LUA_OUT_GIF_RECORD  an AddFrame job: its GIF record, as rtc_lua_program_render_gif delivers it.
 * Before the first launch every Render name is looked up (RTC_ERR_UNSUPPORTED) and every Render size checked against its
 * format (RTC_ERR_ARG); then nothing is rendered. [device] */
enum { RTC_LUA_OUT_FILE = 4u };
rtc_status  rtc_lua_program_render_saved(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags,
                                         rtc_lua_file_fn fn, void *user, rtc_stats *stats);
/* Page-locked host memory for canvases handed to rtc_render: a canvas from rtc_host_alloc is
 * filled by one DMA at link speed, ordinary (pageable) memory goes through the runtime's bounce
 * buffers and is several times slower. What the reference would use for Canvas.pixels
 * (canvas.rs:16-22) when it renders every frame through this library. [device] */
rtc_status  rtc_host_alloc(size_t bytes, void **out);
void        rtc_host_free(void *p);
/* Ray counters accumulated since the last reset (synchronises the stream). */
rtc_status  rtc_stats_read(rtc_context *ctx, rtc_stats *out);
rtc_status  rtc_stats_reset(rtc_context *ctx);
/* Kernel timing. Every render launch (rtc_render_rows / _bands / _views) carries its own pair of HIP events that receive
 * the dispatch's begin and end timestamps on the context stream (hipExtLaunchKernel: no marker
 * packets, the same quantity rocprofv3's kernel trace reports FOR THE RENDER KERNEL k_trace; a launch's binning
 * kernel is timed separately, rtc_binning_times_ms) unless rtc_context_set_timing says
 * otherwise. The context keeps the most recent 1024 pairs. rtc_kernel_times_ms writes the
 * durations (ms) of the latest min(cap, kept) launches, oldest first, and their number to *n; rtc_last_kernel_ms is the newest one alone
 * (RTC_ERR_ARG if nothing was launched yet). Both wait for every launch they report to finish: on a pipelined context
 * (rtc_context_set_pipeline) those launches may still run on several lanes. */
rtc_status  rtc_kernel_times_ms(rtc_context *ctx, float *out, uint32_t cap, uint32_t *n);
/* The same ring for the launches' BINNING kernels (k_bin_tiles: per-tile candidate lists, built per launch for large
 * launches; 0 for a launch that had none): out[k] belongs to the same launch as rtc_kernel_times_ms' out[k]. The render
 * kernel's time does not include it — in order on one stream it runs beside the PREVIOUS launch's render kernel, in a
 * pipelined context beside the other lanes'. */
rtc_status  rtc_binning_times_ms(rtc_context *ctx, float *out, uint32_t cap, uint32_t *n);
/* Which launches carry an event pair: every `every`-th one (1 = all, the default; 0 = none). The
 * events cost about 9 us of host time and 5 us of GPU time per launch, which matters to callers
 * that issue many short launches (one rank's share of a frame); they sample instead. Also forgets
 * the pairs recorded so far: the next launch is the first of a new series. */
rtc_status  rtc_context_set_timing(rtc_context *ctx, uint32_t every);
rtc_status  rtc_last_kernel_ms(rtc_context *ctx, float *ms);

/* Pipelined launches. Camera::render_async returns a NEW Canvas per call (camera.rs:144-160, Canvas::new canvas.rs:26-41),
 * so the frames of a render loop never alias and nothing orders frame i+1 behind frame i except the caller's own use of
 * the result. depth = 1 (the default): every render launch goes, in order, to the context's stream. depth = 2..4: the
 * context deals consecutive launches (rtc_render_rows / _bands / _views) round-robin over `depth` streams of its own, so
 * launch i+1 starts on the CUs that launch i's last waves leave idle (a lone 1080p launch spends a fifth of its time
 * draining) and its per-launch binning kernel runs beside launch i's render. CONTRACT in this mode: the output buffers of
 * `depth` consecutive launches must not overlap; launches are NOT ordered against work on the stream passed to
 * rtc_context_create — the results are complete after rtc_context_synchronize (or rtc_stats_read), and
 * rtc_context_fence makes that stream wait for every launch enqueued so far without blocking the host.
 * Per pixel the results are those of depth 1, bit for bit. Synchronises before switching. [device] */
rtc_status  rtc_context_set_pipeline(rtc_context *ctx, uint32_t depth);
rtc_status  rtc_context_fence(rtc_context *ctx);
/* What the most recent render launch of this context ran with (reports; the choice depends on the World's size, the
 * launch's size and — for A/B runs only — on the RTC_* environment switches read at rtc_context_create). */
typedef struct rtc_launch_info {
    uint32_t source;      /* object loop: 0 brute force through the scalar cache, 1 brute force over ONE LDS-staged table,
                             2 brute force over LDS tiles, 3 one-level per-wave cull, 4 two-level cull              */
    uint32_t reflective;  /* frame-stack kernel (World has reflective materials)                                    */
    uint32_t refractive;  /* ... with refraction frames                                                             */
    uint32_t binned;      /* primary pass reads per-tile candidate lists built by the launch's binning kernel       */
    uint32_t light_lists; /* shadow pass may use the World's light-space lists                                      */
    uint32_t lane;        /* pipeline lane the launch went to (0 when depth = 1)                                    */
    uint32_t block;       /* threads per workgroup                                                                  */
    uint32_t lds_bytes;   /* dynamic LDS per workgroup (LDS-staged object tables, AA sample store)                  */
    uint32_t tiles_per_workgroup; /* tiles one workgroup renders in sequence (1 unless RTC_TILES_PER_WG says otherwise)   */
    uint32_t multi_tile_workgroups; /* guided chunks: of a launch of several rounds of workgroups the FIRST ones render four, three,
                                     then two tiles each (a tile's stores drain under the next one) and the launch ends with
                                     single-tile workgroups (a short tail); this many render more than one. 0: none
                                     (RTC_TILES_GUIDED, RTC_TILES_KMAX)                                                  */
    uint32_t light_table; /* 1: the launch read lights 1..n-1 from the World's device table (more than RTC_MAX_LIGHTS
                             samples, or RTC_LIGHT_TABLE=1), 0: from its kernel arguments / a one-light World           */
    uint32_t lens_samples; /* thin-lens launches (rtc_render_lens*): lens samples per pixel, usteps*vsteps; 0 for every other launch */
} rtc_launch_info;
rtc_status  rtc_context_last_launch_info(rtc_context *ctx, rtc_launch_info *out);
/* The projection of the most recent render launch: RTC_PROJ_ORTHOGRAPHIC or RTC_PROJ_PANORAMA for a projection launch
 * (rtc_render_projection*), 0 for every other launch. An entry of its own: rtc_launch_info has no reserved word left and
 * keeps its 48 bytes. RTC_ERR_ARG for a NULL pointer or before the first launch, as rtc_context_last_launch_info. */
rtc_status  rtc_context_last_launch_projection(rtc_context *ctx, uint32_t *out);

/* Page-lock a canvas the CALLER allocated (a Rust `Vec<Color>`, canvas.rs:16-22: 24 bytes per pixel,
 * the layout rtc_render writes) so that rtc_render / rtc_group_render_host fill it by DMA at link speed
 * instead of through the runtime's bounce buffers. Unregister before the memory is freed. [device] */
rtc_status  rtc_host_register(void *p, size_t bytes);
rtc_status  rtc_host_unregister(void *p);

/* ==== [device] row tiles across the GPUs of one node ================================ */
/* Camera::render_async shards over pixels with no data dependency (camera.rs:144-160: every pixel is an
 * independent work item of the rayon pool). A group is N GPUs that render one frame together: member r
 * renders the 8-row bands r, r+N, r+2N, ... (rtc_render_bands), then ONE exchange step — an RCCL gather
 * of the f64 tiles to member 0 over xGMI (ncclGather) — and one un-deal kernel on member 0's device puts
 * the bands back in the reference's row-major Canvas (canvas.rs:43-51). The World is
 * replicated: its tables are 0.7 KB per object (7 MB for 10 000 objects), plus — per member — the light-space shadow
 * lists of a World above 256 objects (~50 MB: 6 x 128^2 direction cells of 128 entries) and, allocated by the first binned
 * launch, two sets of per-tile candidate lists (8.4 MB per 1080p view, up to 8 views per set while a set stays within 128 MB).
 * Both kinds of lists are optimisations: when their allocation fails the launch renders through the walk instead. Two ways to form a group:
 *   rtc_group_create       one process drives all `ndev` devices (ncclCommInitAll) — what a Rust host
 *                          calling Camera::render_async would use;
 *   rtc_group_create_rank  one process per GPU (torchrun / MPI style): every process creates its member
 *                          with the same 128-byte id (ncclGetUniqueId on rank 0, shipped by the caller's
 *                          launcher) — ncclCommInitRank.
 * Each member owns two HIP streams (render, exchange) and two tile buffers: the gather of frame j
 * overlaps the render of frame j+1. Calls enqueue and return; rtc_group_synchronize waits.
 * A group is used from one thread at a time. */
typedef struct rtc_group       rtc_group;
typedef struct rtc_group_world rtc_group_world;
#define RTC_GROUP_ID_BYTES 128u
enum { /* rtc_group_create / rtc_group_create_rank `exchange` */
    RTC_EXCHANGE_RCCL = 0, /* ncclGather of the f64 tiles (and of the 8-bit tiles when asked for) to member 0     */
    RTC_EXCHANGE_P2P  = 1  /* in-process groups only: hipMemcpyPeerAsync of each tile into member 0's staging
                              buffer (SDMA engines over xGMI, no CUs taken from the render); also the only
                              exchange that accepts the same device more than once (rehearsal on a 1-GPU box) */
};
rtc_status  rtc_group_create(const int32_t *devices, uint32_t ndev, uint32_t exchange, rtc_group **out);
rtc_status  rtc_group_unique_id(uint8_t id[RTC_GROUP_ID_BYTES]);
rtc_status  rtc_group_create_rank(int32_t device, uint32_t nranks, uint32_t rank, const uint8_t id[RTC_GROUP_ID_BYTES],
                                  rtc_group **out);
void        rtc_group_destroy(rtc_group *g);
uint32_t    rtc_group_size(const rtc_group *g);        /* N: members of the whole group                    */
uint32_t    rtc_group_local_size(const rtc_group *g);  /* members this process drives (N, or 1)            */
/* The i-th local member's context (stats, kernel timing, device info); owned by the group. */
rtc_context *rtc_group_context(rtc_group *g, uint32_t i);
rtc_status  rtc_group_synchronize(rtc_group *g);
/* World::new + add_shape on every local member (replicated upload). */
rtc_status  rtc_group_world_create(rtc_group *g, const rtc_shape *shapes, uint32_t n_shapes, const rtc_light *light,
                                   rtc_group_world **out);
void        rtc_group_world_destroy(rtc_group_world *w);
/* Camera::render_async(&World) -> Canvas on all members, `nframes` (<= RTC_MAX_VIEWS_PER_LAUNCH) cameras of
 * one size per call (one launch per member, as rtc_render_views). d_canvas: DEVICE memory on member 0's
 * device, nframes consecutive canvases of vsize*hsize*3 doubles (frame f at f*vsize*hsize*3); required in
 * the process that drives member 0, ignored elsewhere. d_rgb8 (may be NULL): the same frames quantised by
 * Color::scale(c, 255), nframes*vsize*hsize*3 bytes. `what` (the same value in every process of the group)
 * selects the exchange payload, a bit set: */
enum {
    RTC_GATHER_NONE = 0u, /* render only: the tiles stay on their GPUs                                         */
    RTC_GATHER_F64  = 1u, /* the f64 Canvas (24 B/pixel), the path's own output -> d_canvas                     */
    RTC_GATHER_U8   = 2u  /* the 8-bit frame (3 B/pixel, what every file writer of the reference consumes,
                             canvas.rs:98-104) -> d_rgb8; RTC_GATHER_F64 | RTC_GATHER_U8 delivers both         */
};
rtc_status  rtc_group_render(rtc_group *g, const rtc_group_world *w, const rtc_camera *cams, uint32_t nframes,
                             uint32_t mode, uint32_t flags, uint32_t what, void *d_canvas, void *d_rgb8);
/* Camera::render_async(&World) -> Canvas in HOST memory: every local member renders its bands and DMAs them
 * straight to their rows of `rgb` over its own PCIe link (no gather: N links fill the canvas side by side).
 * `rgb` = vsize*hsize*3 doubles, ideally page-locked (rtc_host_alloc / rtc_host_register); with one process
 * per GPU it is each process's mapping of one shared-memory canvas. Synchronous for the local members.
 * `stats` (may be NULL) = the local members' ray counters for this frame. */
rtc_status  rtc_group_render_host(rtc_group *g, const rtc_group_world *w, const rtc_camera *cam, uint32_t mode,
                                  uint32_t flags, double *rgb, rtc_stats *stats);
/* The same for the 8-bit frame (rtc_render_rgb8 across the group): `rgb8` = vsize*hsize*3 bytes. */
rtc_status  rtc_group_render_host_rgb8(rtc_group *g, const rtc_group_world *w, const rtc_camera *cam, uint32_t mode,
                                       uint32_t flags, uint8_t *rgb8, rtc_stats *stats);
/* The same for to_imgbuf's RGBA at `gamma` (rtc_render_rgba8 across the group, canvas.rs:61-79 / color.rs:55-65):
 * `rgba8` = vsize*hsize*4 bytes. RTC_ERR_ARG unless gamma is positive and finite. */
rtc_status  rtc_group_render_host_rgba8(rtc_group *g, const rtc_group_world *w, const rtc_camera *cam, uint32_t mode,
                                        uint32_t flags, float gamma, uint8_t *rgba8, rtc_stats *stats);
/* [host] The dealing of a frame's rows over the members (csrc/rtc_bands.h — the one definition rtc_group's tile sizes,
 * gather layout, host-canvas offsets and the un-deal kernel all use), for callers that lay out their own buffers:
 *   rtc_group_packed_rows          rows of one member's packed tile (= of one gather chunk per frame)
 *   rtc_group_bands_owned          bands member `rank` renders: rank, rank + nranks, ...
 *   rtc_group_row_owner            image row y -> (member, row inside its packed tile)
 *   rtc_group_packed_row_to_image  the inverse (results >= vsize are padding)
 *   rtc_group_undeal_host          what member 0's un-deal kernel does, on host memory: `staging` = nranks chunks of
 *                                  [nframes][packed_rows][row_bytes] in rank order (the gather's receive buffer) ->
 *                                  `canvas` = nframes row-major frames of vsize rows. None of these touches a GPU. */
uint32_t    rtc_group_packed_rows(uint32_t vsize, uint32_t nranks);
uint32_t    rtc_group_bands_owned(uint32_t vsize, uint32_t nranks, uint32_t rank);
void        rtc_group_row_owner(uint32_t y, uint32_t nranks, uint32_t *member, uint32_t *packed_row);
uint32_t    rtc_group_packed_row_to_image(uint32_t member, uint32_t packed_row, uint32_t nranks);
rtc_status  rtc_group_undeal_host(const void *staging, void *canvas, uint32_t nranks, uint32_t nframes, uint32_t vsize,
                                  size_t row_bytes);
/* Ray counters of the local members, summed (per member: rtc_stats_read on rtc_group_context). */
rtc_status  rtc_group_stats_read(rtc_group *g, rtc_stats *out);
rtc_status  rtc_group_stats_reset(rtc_group *g);

/* World::color_at(ray, remaining) (shape.rs:702-710) for `n` arbitrary host rays
 * (n x {origin xyz, direction xyz}); writes n x rgb and, if hits != NULL, the hit record
 * of each ray's first intersection. remaining <= RTC_MAX_REFLECTIONS (what Camera::render_pixel passes,
 * camera.rs:98; the kernels' frame stack holds that many suspended shade_hit calls). Synchronous. */
rtc_status  rtc_color_at(rtc_context *ctx, const rtc_world *w, const double *rays, uint32_t n,
                         uint32_t remaining, uint32_t flags, double *rgb, rtc_hit *hits);

/* Device arithmetic probe: applies op (0 sqrt, 1 a/b, 2 pow(a,b), 3 floor, 4 fmod(a,2))
 * element-wise on the GPU; used by the tests to prove f64 sqrt and division are correctly
 * rounded on gfx950 (they must be bit-identical to the host's). op 5 / 6: Vector::normalize (vec.rs:65-76) of
 * every consecutive triple of `a` (n a multiple of 3) — 6 with three IEEE divisions, 5 with the shared-divisor form
 * of the division expansion (rtc_kernels.hip vnormalize_shared; an experiment, must equal 6 bit for bit). op 7: the
 * patterns' even test (csrc/rtc_parity.h), 1.0 where fmod(a, 2) == 0 and 0.0 elsewhere, decided without fmod.
 * op 8: Vector::normalize as 5 / 6, in the form the flat render kernels run (rtc_kernels.hip vnormalize_wave: the
 * shared-divisor form or the three divisions, chosen per wave of 64 consecutive triples); must equal 6 bit for bit.
 * op 9: sqrt as the flat render kernels call it (rtc_kernels.hip sqrt_wave: the expansion's bare core or plain sqrt,
 * chosen per wave of 64 consecutive values); must equal 0 bit for bit. */
rtc_status  rtc_device_arith(rtc_context *ctx, uint32_t op, const double *a, const double *b,
                             uint32_t n, double *out);

/* ==== arbitrary output variables (AOVs): what a pixel SAW ============================== */
/* Besides its colour a frame can say, per pixel, which object the pixel's ray hit, how far away, where, with which
 * normal, and how many of the World's light samples are hidden from that point: image planes for picking, masks, depth
 * compositing and debugging ("why is this pixel black?"), rendered by a small kernel of their own (k_aov,
 * csrc/rtc_kernels.hip) that runs the primary pass and — only when asked — the shadow passes, and shades nothing.
 *
 * For pixel (x, y) the AOV ray is rtc_camera_ray_for_pixel(cam, x, 0.5, y, 0.5): the CENTRE ray, whatever cam->samples
 * says (centre-sample AOVs beside an anti-aliased colour frame). Let Hit be that ray's rtc_hit as rtc_color_at defines it:
 * Intersections::get_hit (the smallest t >= 0.0, ties to the lower shape index) with the vectors of
 * Intersection::compute_vectors. The planes are row-major, idx = y*hsize + x:
 *
 *   plane    type        pixel that hits                                   pixel that misses
 *   index    int32_t     Hit.hit_index                                     -1
 *   depth    double      Hit.t                                             +infinity
 *   point    double[3]   Hit.point                                         0.0, 0.0, 0.0
 *   normal   double[3]   Hit.normal (after the `inside` flip)              0.0, 0.0, 0.0
 *   flags    uint8_t     1 | (Hit.inside << 1)                             0
 *   shadow   uint16_t    number of the World's light samples i (all        0
 *                        rtc_world_light_count(w) of them, in order) with
 *                        is_shadowed_by_light(Hit.over_point, L[i])
 *
 * For a one-light World `shadow` is Hit.shadowed.
 *   Modes.   RTC_MODE_RENDER gives the pixels of the last row and the last column the miss values: that is where
 *            Camera::render leaves the canvas black.
 *   Flags.   RTC_FLAG_NO_CULL gives the same bytes. RTC_FLAG_LDS_TABLE is RTC_ERR_UNSUPPORTED. RTC_FLAG_AA_RESAMPLE is
 *            ignored.
 *   Planes.  A NULL plane pointer means "not wanted": that plane is neither computed nor written. With shadow == NULL no
 *            shadow ray is cast. All six NULL is RTC_ERR_ARG.
 *   Counters. AOV launches do not touch rtc_stats: they are not renders of the reference.
 *   Worlds.  Every World form works: one light, several, area lights (up to RTC_MAX_LIGHTS samples in the kernel
 *            arguments, more from the World's device table), and updated Worlds.
 *   Ordering. The launch goes on the context's stream and waits for a pending rtc_world_update build exactly as
 *            rtc_color_at does. After launches of a pipelined context call rtc_context_fence first
 *            (rtc_canvas_to_rgba8_device's rule). */
typedef struct rtc_aov_buffers {   /* 48 bytes; NULL = plane not wanted */
    int32_t *index; double *depth; double *point; double *normal; uint8_t *flags; uint16_t *shadow;
} rtc_aov_buffers;
enum { RTC_AOV_VIEW_DEPTH = 0, RTC_AOV_VIEW_NORMAL = 1, RTC_AOV_VIEW_INDEX = 2, RTC_AOV_VIEW_SHADOW = 3 };

/* [host] the normative packing: per-pixel hit records (+ per-pixel shadowed-sample counts, may be NULL = use
 * hits[i].shadowed) into the planes above, mode rule included. RTC_ERR_ARG: NULL hits / out, all six planes NULL, a mode
 * that does not exist. */
rtc_status  rtc_aov_from_hits(const rtc_hit *hits, const uint16_t *shadow_counts, uint32_t width, uint32_t height,
                              uint32_t mode, const rtc_aov_buffers *out);
/* [device] enqueue; buffers are DEVICE pointers (depth/point/normal 8-byte aligned, index 4, shadow 2) */
rtc_status  rtc_render_aov_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                                  const rtc_aov_buffers *d);
/* [device] the same into HOST buffers; synchronous; scratch is grow-only and owned by the context (rtc_devmem.h) */
rtc_status  rtc_render_aov(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                           const rtc_aov_buffers *host);
/* A plane as an 8-bit RGB picture (height*width*3 bytes) that every existing encoder takes. The rules are f64 with no
 * fused multiply-add; scale = Color::scale(c, 255) (rtc_color_scale255: truncating, saturating, NaN gives 0).
 *   DEPTH   needs `depth`. All three channels are scale((far - t) / (far - near)): +inf gives 0, t <= near gives 255.
 *           near and far must be finite with far > near, otherwise RTC_ERR_ARG.
 *   NORMAL  needs `normal`. Channel c is scale((n_c + 1.0) * 0.5); a miss is the neutral 127, 127, 127.
 *   INDEX   needs `index`. A miss (index < 0) is black. Otherwise z = splitmix64((uint64_t)index) — the function written
 *           out at rtc_camera.samples — and r = (z & 255) | 0x40, g = ((z >> 8) & 255) | 0x40, b = ((z >> 16) & 255) | 0x40.
 *   SHADOW  needs `shadow`. All channels are scale(1.0 - (double)count / (double)n_lights). n_lights == 0 is RTC_ERR_ARG.
 * A view whose plane is NULL, or a view that does not exist, is RTC_ERR_ARG. near, far and n_lights are read only by the
 * views that name them. */
rtc_status  rtc_aov_view_rgb8(uint32_t view, const rtc_aov_buffers *b, uint32_t width, uint32_t height,
                              double near, double far, uint32_t n_lights, uint8_t *rgb8);            /* [host], normative */
/* [device] the same bytes for planes in DEVICE memory, by k_aov_view (one thread per pixel), enqueued on the context's
 * stream: rtc_image_encoder_encode_device may follow directly. */
rtc_status  rtc_aov_view_rgb8_device(rtc_context *ctx, uint32_t view, const rtc_aov_buffers *d, uint32_t width, uint32_t height,
                                     double near, double far, uint32_t n_lights, void *d_rgb8);      /* [device], same bytes */

/* ==== ambient occlusion: how much of the hemisphere over a pixel's hit is blocked nearby ===== */
/* One more plane of the AOV family: per pixel, how many of a fixed fan of rays leaving the centre ray's hit into the
 * hemisphere about its normal meet something within `radius`. It is what puts the contact shadow under a sphere resting on
 * a floor, which the point-light shading (one `ambient` term for every surface) cannot. Rendered by a kernel of its own
 * (k_ao, csrc/rtc_kernels.hip): k_aov's primary pass and compute_vectors, then one bounded any-hit pass per sample.
 *
 *   Samples. Cosine-weighted directions at the centres of a usteps x vsteps grid of the unit square, NO JITTER (the area
 *   light's and the lens's rule). For sample k = v*usteps + u (v outer, u inner) the HOST evaluates, in f64:
 *       r   = sqrt(((double)u + 0.5) / (double)usteps)
 *       phi = ((2.0 * M_PI) * ((double)v + 0.5)) / (double)vsteps
 *       local_k = ( r * cos(phi),  r * sin(phi),  sqrt(1.0 - r * r) )
 *   rtc_ao_expand is the normative list. The device reads that table and never evaluates sin or cos
 *   (rtc_projection_tables' rule), so its rays are the host's bit for bit whatever the machine's libm does.
 *
 *   The ray of a sample, rtc_ao_ray: f64, no fused multiply-add, every product and sum in exactly this order. With
 *   n = normal and l = local:
 *       sign = copysign(1.0, n.z)
 *       a    = -1.0 / (sign + n.z)
 *       b    = (n.x * n.y) * a
 *       t    = ( 1.0 + ((sign * n.x) * n.x) * a,   sign * b,                   -(sign * n.x) )
 *       s    = ( b,                                sign + ((n.y * n.y) * a),   -n.y )
 *       origin      = over_point
 *       direction.c = ((t.c * l.x) + (s.c * l.y)) + (n.c * l.z)          c = x, y, z
 *   (t, s, n) is the branch-free orthonormal basis of Duff et al., "Building an Orthonormal Basis, Revisited" (JCGT 2017).
 *   The direction is NOT renormalised: it is unit to a few ulp, and leaving it so saves a square root and three IEEE
 *   divisions per ray. Distances along the ray (`t` below) are measured in the direction's own length.
 *
 *   The plane. For pixel (x, y) let Hit be the centre ray's rtc_hit exactly as the AOV section defines it. `ao` is
 *   uint16_t, row-major, and for a pixel that hits holds the number of samples k for which
 *   World::intersect(rtc_ao_ray(Hit.normal, Hit.over_point, local_k)) has a hit (Intersections::get_hit: the smallest
 *   t >= 0.0) with t < radius — is_shadowed_by_light's comparison (shape.rs:716-727) with `radius` in place of the distance
 *   to the light. A pixel that misses holds 0; so do the last row and column under RTC_MODE_RENDER.
 *
 *   Viewing and saving need no view of their own: the plane has the `shadow` plane's type. Put it in
 *   rtc_aov_buffers::shadow and pass n_lights = usteps*vsteps: RTC_AOV_VIEW_SHADOW is then scale(1 - count/n), on the host
 *   and on the device, and the EXR writer stores it as its `shadow` channel.
 *   Flags, ordering, counters, Worlds: as rtc_render_aov_device. RTC_FLAG_NO_CULL gives the same bytes, RTC_FLAG_LDS_TABLE
 *   is RTC_ERR_UNSUPPORTED; rtc_stats is not touched; nothing about the lights is read, so every World form works.
 *   Limits. The centre ray only (whatever cam->samples says), no jitter, and no AO of lens, shutter, group or Lua launches:
 *   composite the plane over those frames with rtc_canvas_apply_ao. */
#define RTC_MAX_AO_SAMPLES 256u
typedef struct rtc_ao {            /* 16 bytes */
    double   radius;               /* > 0; +infinity = unbounded. Anything else, NaN included, is RTC_ERR_ARG */
    uint32_t usteps, vsteps;       /* >= 1 each; usteps*vsteps <= RTC_MAX_AO_SAMPLES */
} rtc_ao;
/* [host] RTC_ERR_ARG for NULL or a field outside the ranges above; else RTC_OK. */
rtc_status  rtc_ao_validate(const rtc_ao *ao);
/* [host] the normative sample list: dirs[3*k + c] = local_k.c for k < usteps*vsteps, and *n = usteps*vsteps. `dirs` needs
 * room for 3*usteps*vsteps doubles (at most 3*RTC_MAX_AO_SAMPLES). RTC_ERR_ARG: NULL, an invalid rtc_ao. */
rtc_status  rtc_ao_expand(const rtc_ao *ao, double *dirs, uint32_t *n);
/* [host] the normative ray; ray = {origin xyz, direction xyz}. RTC_ERR_ARG: a NULL pointer. */
rtc_status  rtc_ao_ray(const double normal[3], const double over_point[3], const double local[3], double ray[6]);
/* [host] the normative packing: per-pixel hit records and per-pixel occluded-sample counts into the plane, mode rule
 * included, a miss gives 0. RTC_ERR_ARG: a NULL pointer, a mode that does not exist. */
rtc_status  rtc_ao_from_hits(const rtc_hit *hits, const uint16_t *counts, uint32_t width, uint32_t height, uint32_t mode,
                             uint16_t *out);
/* [device] enqueue on the context's stream; d_ao is a DEVICE pointer, 2-byte aligned, hsize*vsize entries. The sample table
 * lives in a grow-only buffer of the context and is written in stream order in front of the launch. */
rtc_status  rtc_render_ao_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_ao *ao, uint32_t mode,
                                 uint32_t flags, uint16_t *d_ao);
/* [device] the same into HOST memory; synchronous; scratch is grow-only and owned by the context */
rtc_status  rtc_render_ao(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_ao *ao, uint32_t mode,
                          uint32_t flags, uint16_t *ao_out);
/* Compositing, in place: every component c of pixel i becomes c * (1.0 - strength * ((double)ao[i] / (double)n_samples)),
 * f64 in that order. 0 <= strength <= 1 and n_samples >= 1, else RTC_ERR_ARG (NaN included); so are NULL pointers and a
 * d_rgb that is not 8-byte aligned or a d_ao that is not 2-byte aligned. [host] normative; [device] one thread per pixel on
 * the context's stream, the same bytes — every encoder can follow directly. */
rtc_status  rtc_canvas_apply_ao(double *rgb, const uint16_t *ao, uint32_t n_samples, double strength, uint32_t width, uint32_t height);
rtc_status  rtc_canvas_apply_ao_device(rtc_context *ctx, void *d_rgb, const void *d_ao, uint32_t n_samples, double strength,
                                       uint32_t width, uint32_t height);
/* Scenes whose camera asks for ambient occlusion. YAML: `add: camera` with `ao-radius` (> 0, or .inf) and, optionally,
 * `ao-usteps` / `ao-vsteps` (integers, default 4, at most RTC_MAX_AO_SAMPLES samples in all; they need an `ao-radius`).
 * These entries are rtc_scene_load_yaml_lens plus the AO record: *has_ao_out = 1 and *ao_out filled when the camera has any
 * of those keys, else 0 and *ao_out zeroed. The keys ask for a pass; they change no other entry's result, so every other
 * YAML entry loads such a scene and ignores them. */
rtc_status  rtc_scene_load_yaml_ao(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                   struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                   rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                   struct rtc_lens *lens_out, uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out);
rtc_status  rtc_scene_load_yaml_ao_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                        struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                        rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                        struct rtc_lens *lens_out, uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out);

/* ==== colour bleeding: one bounce of light gathered over the ambient-occlusion fan ============ */
/* The light that reaches a pixel's hit by way of ONE other surface: a red sphere on a white floor tints the floor. The pass
 * is an rtc_ao — the same struct and rtc_ao_validate, the same fan (rtc_ao_expand, rtc_ao_ray), at most RTC_MAX_AO_SAMPLES
 * samples — and every sample's ray is shaded where the AO pass only asks whether it meets something. Rendered by a kernel of
 * its own (k_gather, csrc/rtc_kernels.hip): k_ao's primary pass and tangent frame, then per sample a closest-hit walk, the
 * light loop with its any-hit walks, and lighting() — the function k_trace shades with.
 *
 *   The sample. For pixel (x, y) let Hit be the centre ray's rtc_hit exactly as the AOV section defines it, and for sample k
 *   let ray_k = rtc_ao_ray(Hit.normal, Hit.over_point, local_k). Then
 *       L_k = shade_hit's `surface` for ray_k's first hit (Intersections::get_hit: the smallest t >= 0.0), if that hit
 *             exists and has t < radius: the sum over the World's light samples, in light order, of Material::lighting at the
 *             hit's over_point with eyev = -ray_k.direction, each with its own is_shadowed_by_light ("Worlds with several
 *             lights");
 *       L_k = (0, 0, 0) otherwise.
 *   This is World::color_at of the reference with remaining == 0 whenever `reflectance` is finite: reflected_color and
 *   refracted_color are BLACK there (shape.rs:730, 752), and adding them only turns -0.0 into +0.0, which the mean's leading
 *   `0.0 +` does anyway. No compute_refractive, no reflectv and no Schlick term is evaluated.
 *
 *   The planes. Row-major f64, three doubles per pixel, for a pass of n = usteps*vsteps samples:
 *       radiance[c] = ((((0.0 + L_0[c]) + L_1[c]) + ...) / (double)n)     Color::average_over, in sample order; a mean that is
 *                                                                          a NaN is stored as 0x7FF8000000000000 (the rule of
 *                                                                          rtc_canvas_average)
 *       bounce[c]   = (base[c] * diffuse) * radiance[c]                    a NaN product is stored as that NaN too
 *   `base` is the colour Material::lighting starts from for the PRIMARY hit — the pattern colour at Hit.over_point (the point
 *   k_trace passes to lighting) or material.color — and `diffuse` that material's coefficient: the Lambertian term of a
 *   cosine-weighted fan, ready to be added to a frame (rtc_canvas_add_scaled). A pixel that misses holds zeros in both
 *   planes; under RTC_MODE_RENDER so do the last row and the last column.
 *   Flags, ordering, counters, Worlds: as rtc_render_aov_device. RTC_FLAG_NO_CULL gives the same bytes, RTC_FLAG_LDS_TABLE is
 *   RTC_ERR_UNSUPPORTED; rtc_stats is not touched; every World form works (one light, 2..RTC_MAX_LIGHTS in the kernel
 *   arguments, more from the World's light table, updated Worlds).
 *   Limits. One bounce; the centre ray only (whatever cam->samples says); no jitter; no gather of lens, shutter, projection,
 *   group or Lua launches; no specular or transmitted indirect light (a mirror reflects no bleeding, glass passes none). */
typedef struct rtc_gather_buffers { /* 16 bytes; NULL = not wanted: that plane is neither computed nor written */
    double *radiance;               /* hsize*vsize*3 */
    double *bounce;                 /* hsize*vsize*3 */
} rtc_gather_buffers;
/* [host] the normative packing. hits: width*height centre-ray records; sample_hits[i*n_samples + k] and
 * sample_rgb[3*(i*n_samples + k) + c]: the record and the colour (World::color_at, remaining 0) of pixel i's sample k, read
 * only where hits[i] hits; albedo[3*i + c] = base[c] * diffuse of pixel i's hit (may be NULL when out->bounce is). Applies
 * the radius rule (t < radius counts), the mean, the NaN rule, the bounce product and the mode rule. RTC_ERR_ARG: a NULL
 * input, both planes NULL, n_samples outside 1..RTC_MAX_AO_SAMPLES, a radius that rtc_ao_validate refuses, a mode that does
 * not exist. */
rtc_status  rtc_gather_from_hits(const rtc_hit *hits, const rtc_hit *sample_hits, const double *sample_rgb, const double *albedo,
                                 uint32_t n_samples, double radius, uint32_t width, uint32_t height, uint32_t mode,
                                 const rtc_gather_buffers *out);
/* [device] enqueue on the context's stream; the planes are DEVICE pointers, 8-byte aligned. Both NULL: RTC_ERR_ARG. The
 * sample table is the context buffer rtc_render_ao_device fills. */
rtc_status  rtc_render_gather_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_ao *ao, uint32_t mode,
                                     uint32_t flags, const rtc_gather_buffers *d);
/* [device] the same into HOST memory; synchronous; scratch is grow-only and owned by the context */
rtc_status  rtc_render_gather(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_ao *ao, uint32_t mode,
                              uint32_t flags, const rtc_gather_buffers *host);
/* Compositing, in place: every component c of pixel i becomes c + strength * plane[3*i + its channel], f64 in that order
 * (one product, one sum). strength is finite and >= 0, else RTC_ERR_ARG (NaN included); so are NULL pointers and a device
 * pointer that is not 8-byte aligned. [host] normative; [device] one thread per pixel on the context's stream, the same
 * bytes — every encoder can follow directly. */
rtc_status  rtc_canvas_add_scaled(double *rgb, const double *plane, double strength, uint32_t width, uint32_t height);
rtc_status  rtc_canvas_add_scaled_device(rtc_context *ctx, void *d_rgb, const void *d_plane, double strength, uint32_t width,
                                         uint32_t height);
/* Scenes whose camera asks for a gather pass. YAML: `add: camera` with `gather-radius` (> 0, or .inf) and, optionally,
 * `gather-usteps` / `gather-vsteps`: the rules and defaults of the ao-* keys. These entries are rtc_scene_load_yaml_ao plus a
 * second rtc_ao record: *has_gather_out = 1 and *gather_out filled when the camera has any of those keys, else 0 and
 * *gather_out zeroed. Like the ao-* keys they ask for a pass, and every other YAML entry ignores them. */
rtc_status  rtc_scene_load_yaml_gather(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                       struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                       rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                       struct rtc_lens *lens_out, uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out,
                                       rtc_ao *gather_out, uint32_t *has_gather_out);
rtc_status  rtc_scene_load_yaml_gather_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                            struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                            rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                            struct rtc_lens *lens_out, uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out,
                                            rtc_ao *gather_out, uint32_t *has_gather_out);

/* ==== the three passes under an orthographic or panorama camera ======================== */
/* rtc_render_aov*, rtc_render_ao* and rtc_render_gather* with the rays of a projection (rtc_projection, above) in place of
 * the pinhole's centre rays: each entry has its pinhole twin's signature with `proj` after `cam`, and everything the twin's
 * text says holds with ONE substitution — the pixel's ray. Normative:
 *   - the ray of pixel (x, y) is rtc_projection_ray(cam, proj, x, y); Hit is World::intersect + get_hit of that ray with
 *     Intersection::compute_vectors, as rtc_color_at reports it; the AOV planes are rtc_aov_from_hits of those records, the
 *     gather planes rtc_gather_from_hits;
 *   - the fan of the AO and gather passes is rtc_ao_ray about that Hit (its over_point, its flipped normal);
 *   - `depth` is t along the UNIT direction. For an orthographic ray that is the distance from the camera's z = 0 plane,
 *     where the ray starts — not from a point. The plane may cut a surface: the rays that start inside it hit it from
 *     inside (flags bit 1, the normal flipped), and what lies wholly behind the plane is not seen;
 *   - modes, flags, NULL planes, Worlds and ordering: the twin's. RTC_FLAG_NO_CULL gives the same bytes;
 *     RTC_FLAG_LDS_TABLE answers what it answers the twin.
 * Arguments are checked in this order: rtc_render_projection's checks first — a NULL context, World, camera or output, a
 * World of another context, a mode that does not exist, a canvas without pixels; then a NULL or invalid projection
 * (rtc_projection_validate) and cam->samples != 1 — then the pinhole pass's own (all planes NULL, an invalid rtc_ao, a
 * misaligned device pointer). Each of them is RTC_ERR_ARG, and nothing has been launched.
 * The launches stay uncounted in rtc_stats, as the twins'. rtc_context_last_launch_projection reports the kind after them
 * and rtc_context_last_launch_info the object loop (source) they took; a pinhole pass leaves both records alone.
 * A panorama's tables are rtc_render_projection's: the same two buffers under the same key, so a colour launch and a pass of
 * one panorama size upload them once, and a change of key waits for every stream of the context first.
 * Kernels: the projection instantiations of k_aov, k_ao and k_gather (a trailing DevProjection; csrc/rtc_kernels.hip). A
 * panorama tile's primary bundle has the camera origin as its shared apex (two-level Worlds: the ordered walk with early
 * stop); an orthographic tile's has its apex at one lane's origin and its spread measured, and every candidate is visited. */
rtc_status  rtc_render_aov_projection_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                             uint32_t mode, uint32_t flags, const rtc_aov_buffers *d);
rtc_status  rtc_render_aov_projection(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                      uint32_t mode, uint32_t flags, const rtc_aov_buffers *host);
rtc_status  rtc_render_ao_projection_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                            const rtc_ao *ao, uint32_t mode, uint32_t flags, uint16_t *d_ao);
rtc_status  rtc_render_ao_projection(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                     const rtc_ao *ao, uint32_t mode, uint32_t flags, uint16_t *ao_out);
rtc_status  rtc_render_gather_projection_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                                const rtc_ao *ao, uint32_t mode, uint32_t flags, const rtc_gather_buffers *d);
rtc_status  rtc_render_gather_projection(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                         const rtc_ao *ao, uint32_t mode, uint32_t flags, const rtc_gather_buffers *host);

/* ==== float files: the f64 canvas and the AOV planes saved as data ==================== */
/* Every writer above takes Color::scale'd 8-bit rows: components above 1.0 are clipped and a depth plane becomes a picture.
 * These three keep the numbers. Input: the f64 canvas, `rgb` = height*width*3 doubles, top row first (what rtc_render,
 * rtc_render_lens, rtc_shutter_render_device and rtc_canvas_average_device produce), and — for EXR — the AOV planes of
 * rtc_aov_buffers. The float table, a table of its own beside rtc_image_format_for_name's (which does not know these
 * names) with the same extension rule:
 *   hdr   RTC_FLOAT_HDR   Radiance RGBE           pfm   RTC_FLOAT_PFM   Portable Float Map           exr   RTC_FLOAT_EXR   OpenEXR
 * Width and height 1..65535. All integers little-endian; no field not listed is written.
 *
 * Conversions (csrc/rtc_float.h, the same integer arithmetic on the host and on the device — no hardware conversion):
 *   f64 -> f32   IEEE round-to-nearest-even; subnormals kept; overflow gives +-inf; any NaN becomes 0x7FC00000.
 *   f64 -> f16   round-to-nearest-even directly from the f64, never through f32 (1 + 2^-11 + 2^-30 is 0x3C01; through f32
 *                it would be 0x3C00); subnormals kept; overflow gives +-inf; any NaN becomes 0x7E00.
 *   f64 -> RGBE  Ward's float2rgbe, made exact. Each component is first mapped: NaN or < 0 -> 0, above 0x1.FEp+126 ->
 *                0x1.FEp+126. v = the largest mapped component. v < 1e-32: the pixel is 0,0,0,0. Otherwise frexp(v) = (m, e),
 *                byte c = floor(ldexp(comp_c, 8 - e)) (always <= 255), E = e + 128. Decoding byte * 2^(E - 136) differs from
 *                the mapped component by less than v / 128.
 *
 *   PFM:  "PF\n<w> <h>\n-1.0\n" (decimal), then the rows BOTTOM to top, R,G,B of each pixel as f32.
 *   HDR:  "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y <h> +X <w>\n", then the scanlines, top row first.
 *         8 <= w <= 32767: a scanline is 02 02 hi(w) lo(w), then the row's R, G, B and E byte planes, each coded on its own:
 *           split the plane into MAXIMAL runs of equal bytes;
 *           every maximal run of length >= 4 is run tokens (128 + n, byte): n = 127 while 127 or more bytes remain, then one
 *           token for the rest (n >= 1);
 *           every stretch between such runs is literal tokens (n, n bytes): n = 128 while 128 or more bytes remain, then
 *           one token for the rest.
 *         Nothing crosses a plane or a row. A coded plane never exceeds w + ceil(w / 128) bytes (alternating bytes reach it).
 *         Any other width: flat R,G,B,E pixels. (The rule is on maximal runs, not on a left-to-right parse, so the tokens of
 *         a row can be found by a segmented scan.)
 *   EXR:  single-part scanline file, NO_COMPRESSION. Magic 76 2F 31 01, version word 2 (i32). Attributes, each
 *         name NUL type NUL size (i32) value, in this order: channels (chlist), compression (compression) = 0 (1 byte),
 *         dataWindow (box2i) = 0,0,w-1,h-1, displayWindow (box2i) = the same, lineOrder (lineOrder) = 0 (1 byte),
 *         pixelAspectRatio (float) = 1.0f, screenWindowCenter (v2f) = 0,0, screenWindowWidth (float) = 1.0f; then a 0 byte.
 *         A chlist entry: name NUL, pixel type (i32: 0 UINT, 1 HALF, 2 FLOAT), pLinear 0 and three reserved 0 bytes,
 *         xSampling 1, ySampling 1 (i32 each); the list ends with a 0 byte. Then h u64 scanline offsets (from the start of
 *         the file), then per scanline, top first: i32 y, i32 bytes of pixel data, and each channel's w values in chlist
 *         order. The channels are those the caller supplies, in byte-wise alphabetical order:
 *           B G N.X N.Y N.Z P.X P.Y P.Z R Z id shadow
 *         R, G, B = `rgb` (HALF or FLOAT: rgb_type); Z = aov.depth (FLOAT; a miss is +inf); N.* = aov.normal, P.* = aov.point
 *         (FLOAT); id = aov.index + 1 (UINT, 0 = miss); shadow = aov.shadow (UINT). Any subset: a NULL plane is not stored;
 *         no canvas and no plane is RTC_ERR_ARG, and so is a canvas with an rgb_type that is neither. aov.flags is not
 *         stored. No ZIP / PIZ compression, no tiles, no multi-part files.
 *   HDR and PFM read `rgb` alone (NULL is RTC_ERR_ARG) and ignore rgb_type.
 *
 * rtc_float_format_for_name: the float table's format for `name` (RTC_ERR_UNSUPPORTED if none; RTC_ERR_ARG for NULL).
 * rtc_float_format: the whole file — bytes needed (0 on bad arguments); writes at most cap. Host, normative.
 * rtc_canvas_save_f64: the file of the canvas to `path`, the format from the name (EXR: HALF); RTC_ERR_UNSUPPORTED before
 *   anything is opened. Host.
 * rtc_hdr_rle_row: one plane of one row by the rule above — *n = bytes needed, at most cap of them written (out may be NULL
 *   when cap is 0). RTC_ERR_ARG for a NULL plane or n, or width 0. Host.
 * The entries that take a NAME and hold f64 data consult the float table first, then the 8-bit table: ch1::Canvas::save of
 * an unquantised Canvas, the Python rtc.save given a float64 array, rtc_lua_program_render_saved (a Render job named *.hdr,
 * *.pfm or *.exr renders its f64 canvas on its lane and delivers the file as RTC_LUA_OUT_FILE; EXR: HALF). */
enum { RTC_FLOAT_HDR = 0, RTC_FLOAT_PFM = 1, RTC_FLOAT_EXR = 2 };
enum { RTC_EXR_HALF = 1, RTC_EXR_FLOAT = 2 };
typedef struct rtc_float_planes {   /* 64 bytes */
    const double *rgb; rtc_aov_buffers aov; uint32_t rgb_type; uint32_t _pad;
} rtc_float_planes;
rtc_status  rtc_float_format_for_name(const char *name, uint32_t *format);
size_t      rtc_float_format(uint32_t format, const rtc_float_planes *p, uint32_t width, uint32_t height, uint8_t *buf, size_t cap);
rtc_status  rtc_canvas_save_f64(const char *path, const double *rgb, uint32_t width, uint32_t height);
rtc_status  rtc_hdr_rle_row(const uint8_t *plane, uint32_t width, uint8_t *out, size_t cap, size_t *n);
/* The float writers on the device: rtc_float_format's bytes for planes already in device memory (csrc/rtc_float.hip); only
 * the finished file crosses PCIe, behind its 8-byte length. PFM, EXR and the flat form of HDR are packed by one kernel (one
 * thread per 16 bytes of the file; the header and EXR's offset table computed on the host); RLE HDR is a chain — planar
 * R,G,B,E bytes, each row-plane's coded size by a wave, a scan over the 4h sizes, the tokens — whose length exists only on
 * the device; its buffer is sized from the worst case above. An encoder is bound to a context and owns its scratch, grow-only.
 *   encode_device: `d` holds DEVICE pointers (rgb and every f64 plane 8-byte aligned, index 4, shadow 2), encoded on the
 *     context's stream in order with what the caller put there before (after launches of a pipelined context:
 *     rtc_context_fence first); blocks until the file is on the host. Bad arguments are RTC_ERR_ARG and launch nothing.
 *   render: Camera::render's f64 canvas through the rows path into the encoder's scratch, then the file; the canvas never
 *     leaves the device. The bytes equal rtc_float_format of rtc_render's canvas. render_lens: the same through
 *     rtc_render_lens_rows (lens == NULL: render). rgb_type is read for EXR only.
 *   bytes: the last file (bytes needed; writes at most cap; 0 before the first); write: the same to `path`. [device] */
typedef struct rtc_float_encoder rtc_float_encoder;
rtc_status  rtc_float_encoder_create(rtc_context *ctx, rtc_float_encoder **out);
rtc_status  rtc_float_encoder_encode_device(rtc_float_encoder *e, uint32_t format, const rtc_float_planes *d, uint32_t width,
                                            uint32_t height);
rtc_status  rtc_float_encoder_render(rtc_float_encoder *e, uint32_t format, const rtc_world *w, const rtc_camera *cam,
                                     uint32_t mode, uint32_t flags, uint32_t rgb_type);
rtc_status  rtc_float_encoder_render_lens(rtc_float_encoder *e, uint32_t format, const rtc_world *w, const rtc_camera *cam,
                                          const rtc_lens *lens, uint32_t mode, uint32_t flags, uint32_t rgb_type);
size_t      rtc_float_encoder_bytes(const rtc_float_encoder *e, uint8_t *buf, size_t cap);
rtc_status  rtc_float_encoder_write(const rtc_float_encoder *e, const char *path);
void        rtc_float_encoder_destroy(rtc_float_encoder *e);

/* ==== edge-aware filter: smoothing an AO, shadow or bounce plane under the AOV guides ================= */
/* The sample fans (rtc_render_ao, rtc_render_gather, the `shadow` plane of an area-light World) place their samples at cell
 * centres with no jitter, so a plane of few samples shows bands. This pass is the other half of the technique: an à-trous
 * ("with holes") wavelet filter — a 5x5 B3-spline kernel applied `passes` times, its taps 1, 2, 4, ... pixels apart — whose
 * every tap is weighted by how well the neighbour's AOV guides (rtc_render_aov's `index`, `point` and `normal` planes) agree
 * with the pixel's own: the scheme of Dammertz et al., "Edge-Avoiding À-Trous Wavelet Transform for fast Global Illumination
 * Filtering" (HPG 2010), with a point-to-plane distance in place of the position distance. It smooths along a surface and
 * not across an edge, a crease or a silhouette.
 *
 * All of it is f64 with no fused multiply-add, every product and sum evaluated in exactly the order written.
 *   inv = 1.0 / plane_sigma, once (0.0 for +infinity);  h = {0.0625, 0.25, 0.375, 0.25, 0.0625}.
 *   Pass i (from 0) reads plane A_i and writes A_{i+1} with step s = 1 << i; A_0 = `in`, the last pass writes `out`.
 *   For pixel p = (x, y):
 *     index[p] < 0: the pixel's values are copied bit for bit. Otherwise acc[c] = 0.0, wsum = 0.0, and for j = 0..4 (outer,
 *     dy = (j - 2)*s) and i = 0..4 (inner, dx = (i - 2)*s), with q = (x + dx, y + dy), the tap is SKIPPED — nothing is added,
 *     and its value is never read into the arithmetic — when
 *       q is outside the image, or index[q] < 0,
 *       or RTC_FILTER_SAME_OBJECT is set and index[q] != index[p],
 *       or !(wz > 0.0), where e.c = point[q].c - point[p].c, d = fabs(((n_p.x*e.x) + (n_p.y*e.y)) + (n_p.z*e.z)),
 *          wz = 1.0 - d*inv,
 *       or !(m > 0.0), where m = ((n_p.x*n_q.x) + (n_p.y*n_q.y)) + (n_p.z*n_q.z); after this test m = m*m is applied
 *          normal_squarings times,
 *       or !(w > 0.0), where w = ((h[j]*h[i])*wz)*m.
 *     Otherwise acc[c] = acc[c] + w*A_i[q][c] and wsum = wsum + w.
 *     After the taps: wsum > 0.0 gives A_{i+1}[p][c] = acc[c] / wsum, a NaN quotient stored as 0x7FF8000000000000
 *     (rtc_canvas_average's rule); otherwise the pixel is copied.
 *   The comparisons are written so that a NaN guide drops a tap and poisons no sum; an inf under a skipped tap is harmless.
 *
 * Defaults, chosen so that a filtered 4x4-sample AO plane of data/ambient_occlusion.yml is closer (RMS) to the 16x16-sample
 * plane than the raw one (profiles/filter_quality.log): RTC_FILTER_DEFAULT_*. plane_sigma is a distance in world units and
 * relative to nothing.
 * Limits. No variance guidance and no temporal accumulation; colour frames are not filtered (their texture is not in the
 * guides); one sigma per call, none per pixel; the guides are those of the centre ray, so no filtering of lens, shutter,
 * projection, group or Lua launches. */
enum { RTC_FILTER_SAME_OBJECT = 1u << 0 };
#define RTC_MAX_FILTER_PASSES 5u
#define RTC_FILTER_DEFAULT_PLANE_SIGMA 0.05
#define RTC_FILTER_DEFAULT_PASSES 2u
#define RTC_FILTER_DEFAULT_NORMAL_SQUARINGS 3u
typedef struct rtc_filter {          /* 24 bytes */
    double   plane_sigma;            /* > 0, +infinity allowed (no plane test); NaN, 0, negative: RTC_ERR_ARG */
    uint32_t passes;                 /* 1..RTC_MAX_FILTER_PASSES; pass i (from 0) has step s = 1 << i */
    uint32_t normal_squarings;       /* 0..8: the normal weight is (n_p . n_q) squared this many times */
    uint32_t flags;                  /* RTC_FILTER_SAME_OBJECT or 0; other bits RTC_ERR_ARG */
    uint32_t _pad;                   /* 0 */
} rtc_filter;
/* [host] RTC_ERR_ARG for NULL or a field outside the ranges above (a nonzero _pad included); else RTC_OK. */
rtc_status  rtc_filter_validate(const rtc_filter *flt);
/* [host] the normative filter. `in` and `out`: row-major f64 planes of `channels` (1 or 3) values per pixel, not the same
 * buffer. Of `guides` only index, point and normal are read; a NULL among the three is RTC_ERR_ARG, like a NULL pointer,
 * another channel count or an invalid rtc_filter. The intermediate planes live in scratch (RTC_ERR_NOMEM without it). */
rtc_status  rtc_plane_filter(const double *in, uint32_t channels, const rtc_aov_buffers *guides, uint32_t width, uint32_t height,
                             const rtc_filter *flt, double *out);
/* [device] the same bytes for planes in DEVICE memory, enqueued on the context's stream under the ordering rule of
 * rtc_canvas_apply_ao_device: k_atrous (csrc/rtc_filter.hip), one launch per pass. d_in, d_out, point and normal 8-byte
 * aligned, index 4; otherwise RTC_ERR_ARG, and nothing is launched. The ping-pong plane is a grow-only buffer of the context:
 * no allocation per call once it has its size. */
rtc_status  rtc_plane_filter_device(rtc_context *ctx, const void *d_in, uint32_t channels, const rtc_aov_buffers *d_guides,
                                    uint32_t width, uint32_t height, const rtc_filter *flt, void *d_out);
/* A count plane (rtc_render_ao's, or rtc_aov_buffers::shadow) as the fraction the filter takes: out[i] = (double)counts[i] /
 * (double)n. n == 0 and NULL pointers are RTC_ERR_ARG; on the device also a d_counts that is not 2-byte or a d_out that is not
 * 8-byte aligned. [host] normative; [device] one thread per pixel on the context's stream, the same bytes. */
rtc_status  rtc_counts_to_fraction(const uint16_t *counts, uint32_t n, uint32_t width, uint32_t height, double *out);
rtc_status  rtc_counts_to_fraction_device(rtc_context *ctx, const void *d_counts, uint32_t n, uint32_t width, uint32_t height,
                                          void *d_out);
/* Compositing an occlusion FRACTION, in place: every component c of pixel i becomes c * (1.0 - strength * occ[i]), f64 in that
 * order: rtc_canvas_apply_ao's f64 sibling, and its bytes whenever occ = count/n. 0 <= strength <= 1, else RTC_ERR_ARG (NaN
 * included); so are NULL pointers and a device pointer that is not 8-byte aligned. [host] normative; [device] the same bytes. */
rtc_status  rtc_canvas_apply_occlusion(double *rgb, const double *occ, double strength, uint32_t width, uint32_t height);
rtc_status  rtc_canvas_apply_occlusion_device(rtc_context *ctx, void *d_rgb, const void *d_occ, double strength, uint32_t width,
                                              uint32_t height);
/* Scenes whose camera asks for the filter. YAML: `add: camera` with `filter-plane-sigma` (> 0, or .inf) and, optionally,
 * `filter-passes` (1..RTC_MAX_FILTER_PASSES) and `filter-normal-squarings` (0..8), which need a `filter-plane-sigma` and
 * default to RTC_FILTER_DEFAULT_*; flags = RTC_FILTER_SAME_OBJECT. These entries are rtc_scene_load_yaml_gather plus the filter
 * record: *has_filter_out = 1 and *filter_out filled when the camera has any of those keys, else 0 and *filter_out zeroed.
 * Like the ao-* keys they ask for a pass, and every other YAML entry ignores them. */
rtc_status  rtc_scene_load_yaml_filter(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                       struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                       rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                       struct rtc_lens *lens_out, uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out,
                                       rtc_ao *gather_out, uint32_t *has_gather_out, rtc_filter *filter_out, uint32_t *has_filter_out);
rtc_status  rtc_scene_load_yaml_filter_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                            struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                            rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                            struct rtc_lens *lens_out, uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out,
                                            rtc_ao *gather_out, uint32_t *has_gather_out, rtc_filter *filter_out, uint32_t *has_filter_out);
/* Scenes whose camera has a projection AND asks for passes (data/orthographic_passes.yml): rtc_scene_load_yaml_filter plus
 * rtc_scene_load_yaml_projection's record — the lens, the projection, and the ao-*, gather-* and filter-* records of the
 * camera, each with its has-flag, under the rules of the entries that introduced them. What the records are for:
 * rtc_render_aov_projection, rtc_render_ao_projection, rtc_render_gather_projection and rtc_plane_filter. Every other entry
 * refuses or ignores what it refused or ignored before: the entries without a projection record still refuse such a scene,
 * naming rtc_scene_load_yaml_projection. */
rtc_status  rtc_scene_load_yaml_projection_passes(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                                  struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                                  rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                                  struct rtc_lens *lens_out, uint32_t *has_lens_out,
                                                  struct rtc_projection *proj_out, uint32_t *has_projection_out,
                                                  rtc_ao *ao_out, uint32_t *has_ao_out, rtc_ao *gather_out, uint32_t *has_gather_out,
                                                  rtc_filter *filter_out, uint32_t *has_filter_out);
rtc_status  rtc_scene_load_yaml_projection_passes_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                                       struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                                       rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                                       struct rtc_lens *lens_out, uint32_t *has_lens_out,
                                                       struct rtc_projection *proj_out, uint32_t *has_projection_out,
                                                       rtc_ao *ao_out, uint32_t *has_ao_out, rtc_ao *gather_out, uint32_t *has_gather_out,
                                                       rtc_filter *filter_out, uint32_t *has_filter_out);

/* ==== edge-adaptive anti-aliasing: extra rays only where the frame has contrast ====================== */
/* A one-sample frame is fast and stair-stepped; cam->samples != 1 pays four or more rays for every pixel, sky and flat floor
 * included. This pass renders the one-sample frame, finds the pixels whose neighbourhood has contrast — Color::distance_from
 * against 0.01, the reference's own "needs more samples" test (camera.rs:109) — and replaces only those by the mean of a
 * usteps x vsteps grid of sub-samples (Color::average_over, the lens's rule), all of it on the device.
 *
 * The statement: f64, no fused multiply-add, in exactly this order.
 *   Rendered area R. RTC_MODE_RENDER_ASYNC: every pixel. RTC_MODE_RENDER: the pixels with x < hsize-1 and y < vsize-1; the
 *     last row and column stay black, are never refined and are never compared against.
 *   Mask, on the centre-sample frame C (rtc_render's bytes with cam->samples == 1): pixel p in R gets mask byte 1 iff some
 *     4-neighbour q (left, right, up, down) that is also in R has d(p, q) > threshold, where dr = C[p].r - C[q].r (dg, db
 *     alike) and d = sqrt(((dr*dr) + (dg*dg)) + (db*db)), an IEEE sqrt: Color::distance_from (color.rs:122-126). A NaN
 *     distance compares false. Every other byte is 0. d is bitwise symmetric in p and q. The mask is taken once: refined
 *     values never feed back into it.
 *   Sample k of n = usteps*vsteps: u = k % usteps, v = k / usteps, x_offset = ((double)u + 0.5) / (double)usteps,
 *     y_offset = ((double)v + 0.5) / (double)vsteps. 2 x 2 gives the reference's four fixed sub-samples in its order
 *     (camera.rs:102-105).
 *   A refined pixel (mask 1) is Color::average_over of color_at(rtc_camera_ray_for_pixel(cam, x, x_offset_k, y, y_offset_k),
 *     RTC_MAX_REFLECTIONS) for k = 0..n-1: three sums that start at 0.0, add in k order and are divided once by (double)n.
 *   An unrefined pixel keeps C's bytes.
 * Limits. Pinhole cameras only: no adaptive form of the lens, the projections, the shutter, rtc_group or Lua launches. One
 * detection pass, 4 neighbours, the colour frame as its only guide; no jitter (the oracle could not follow it). */
#define RTC_MAX_AA_SAMPLES 256u
#define RTC_AA_DEFAULT_THRESHOLD 0.01          /* camera.rs:109 */
#define RTC_AA_DEFAULT_STEPS 4u                /* what an absent aa-usteps / aa-vsteps key means */
#define RTC_AA_DEFAULT_MAX_RAYS (1u << 21)     /* 96 MB of rays and 48 MB of colours at the most */
typedef struct rtc_adaptive {
    double   threshold;        /* any value but NaN; +inf refines nothing, a negative value every pixel that has a neighbour */
    uint32_t usteps, vsteps;   /* >= 1 each, usteps*vsteps <= RTC_MAX_AA_SAMPLES */
    uint32_t max_rays;         /* refinement rays per probe launch; 0 = RTC_AA_DEFAULT_MAX_RAYS; otherwise >= usteps*vsteps */
    uint32_t _pad;             /* 0 */
} rtc_adaptive;                /* 24 bytes */
typedef struct rtc_adaptive_info { /* 24 bytes */
    uint64_t pixels_refined;   /* mask bytes that are 1 */
    uint64_t rays_refined;     /* pixels_refined * usteps*vsteps */
    uint32_t launches;         /* probe launches: ceil(pixels_refined / floor(max_rays / (usteps*vsteps))) */
    uint32_t _pad;
} rtc_adaptive_info;
/* [host] RTC_ERR_ARG for NULL or a field outside the ranges above (a nonzero _pad included); else RTC_OK. */
rtc_status  rtc_adaptive_validate(const rtc_adaptive *spec);
/* [host] the offsets of sample k. RTC_ERR_ARG: a NULL pointer, an invalid spec, k >= usteps*vsteps. */
rtc_status  rtc_adaptive_offset(const rtc_adaptive *spec, uint32_t k, double *x_offset, double *y_offset);
/* [host] the normative mask of the row-major f64 canvas `rgb` into `mask` (width*height bytes); *n_flagged (may be NULL)
 * receives the number of 1 bytes. RTC_ERR_ARG: a NULL rgb or mask, a mode that does not exist, a NaN threshold. */
rtc_status  rtc_adaptive_mask(const double *rgb, uint32_t width, uint32_t height, uint32_t mode, double threshold,
                              uint8_t *mask, uint64_t *n_flagged);
/* [device] the same bytes for any canvas in DEVICE memory, enqueued on the context's stream (k_aa_mask, csrc/rtc_adaptive.hip):
 * d_rgb 8-byte aligned (else RTC_ERR_ARG), d_mask any address. Exactly width*height bytes are written. More than 2^31-1
 * pixels is RTC_ERR_ARG. The per-tile counts go to a grow-only buffer of the context. */
rtc_status  rtc_adaptive_mask_device(rtc_context *ctx, const void *d_rgb, uint32_t width, uint32_t height, uint32_t mode,
                                     double threshold, void *d_mask);
/* [device] the adaptive frame into the caller's DEVICE canvas d_rgb (hsize*vsize*3 doubles, 8-byte aligned), where
 * rtc_canvas_to_rgba8_device and every _encode_device entry take it; d_mask (hsize*vsize bytes, may be NULL) receives the
 * mask; *info (may be NULL) what was refined.
 *   cam->samples must be 1 (RTC_ERR_ARG otherwise). RTC_FLAG_NO_CULL gives the same bytes, RTC_FLAG_LDS_TABLE is
 *   RTC_ERR_UNSUPPORTED, RTC_FLAG_AA_RESAMPLE is ignored. Every World form works: one light, several, area lights through
 *   the light table, updated Worlds.
 *   Pipeline (csrc/rtc_adaptive.hip): the one-sample launch of rtc_render_rows; k_aa_mask; k_aa_scan (prefix sum of the
 *   tile counts); k_aa_list (the flagged pixels, row-major tile by tile, the same order in every run); then per chunk of
 *   floor(max_rays / n) pixels k_aa_rays, rtc_color_at's kernel on device rays, k_aa_resolve.
 *   Ordering. rtc_render_aov_device's rule: everything goes on the context's stream; after launches of a pipelined context
 *   call rtc_context_fence first. The call reads back ONE count, the number of flagged pixels, which sizes the list and the
 *   chunks: it waits for the stream once, after the scan, and returns with the refinement enqueued, not finished.
 *   Counters. The base frame counts in rtc_stats exactly as rtc_render_rows counts it. The refinement rays count as
 *   rtc_color_at counts its rays: not at all (probe launches carry no counters); info->rays_refined says how many there were.
 *   Memory. The tile counts, the list, the chunk's rays and colours (and the mask when d_mask is NULL) are grow-only buffers
 *   of the context: a second call of the same size allocates nothing. */
rtc_status  rtc_render_adaptive_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_adaptive *spec,
                                       uint32_t mode, uint32_t flags, void *d_rgb, void *d_mask, rtc_adaptive_info *info);
/* [device] the same call with the frame (hsize*vsize*3 doubles) and, when `mask` is not NULL, the mask copied into HOST
 * memory. Synchronous. `stats` (may be NULL) as in rtc_render: reset before, read after. */
rtc_status  rtc_render_adaptive(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_adaptive *spec,
                                uint32_t mode, uint32_t flags, double *rgb, uint8_t *mask, rtc_adaptive_info *info, rtc_stats *stats);
/* Scenes whose camera asks for adaptive anti-aliasing. YAML: `add: camera` with any of `aa-threshold` (a number, .inf
 * allowed; default RTC_AA_DEFAULT_THRESHOLD), `aa-usteps` and `aa-vsteps` (integers >= 1 whose product is at most
 * RTC_MAX_AA_SAMPLES; default RTC_AA_DEFAULT_STEPS each); max_rays = 0. These entries are rtc_scene_load_yaml_area_lights
 * plus the record: *has_adaptive_out = 1 and *adaptive_out filled when the camera has any of those keys, else 0 and
 * *adaptive_out zeroed. A camera with aa-* keys and lens or projection keys is RTC_ERR_PARSE with a message that says so,
 * whichever entry loads it; otherwise every other YAML entry ignores the aa-* keys. */
rtc_status  rtc_scene_load_yaml_adaptive(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                         struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                         rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                         rtc_adaptive *adaptive_out, uint32_t *has_adaptive_out);
rtc_status  rtc_scene_load_yaml_adaptive_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                              struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                              rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                              rtc_adaptive *adaptive_out, uint32_t *has_adaptive_out);

/* ==== exposure, tone mapping and bloom: from a linear f64 frame to one that fits 8 bits ============== */
/* A World of several lights, an area light's samples or a bounce plane on top give canvases brighter than 1.0. Every 8-bit
 * path ends in Color::scale, which clamps: a lit floor becomes a flat white patch. These passes are the step between the
 * linear frame and rtc_canvas_to_rgba8[_device] / the encoders: frame statistics, an exposure and a tone curve, and the glare
 * (bloom) around highlights. Each has a normative host statement and a device form that gives the same bytes.
 *
 * Arithmetic: f64 throughout, no fused multiply-add, the operations in exactly the order written here. A NaN result is
 * stored as 0x7FF8000000000000 (rtc_canvas_average's rule). Nothing here calls exp, log or pow on the device — the device's
 * versions are not the host's bit for bit — which is why the curves are the rational ones, why the auto exposure uses the
 * ARITHMETIC mean luminance and not the log-average, and why the bloom's weights are a host table that travels in the kernel
 * arguments.
 *
 * Luminance: Y(c) = ((0.2126*r) + (0.7152*g)) + (0.0722*b). */
typedef struct rtc_luminance { /* 24 bytes */
    double   max;              /* the largest contributing luminance; 0.0 when none contributes */
    double   sum;              /* the contributions' sum in the tree order below */
    uint64_t count;            /* how many pixels contribute */
} rtc_luminance;
/* [host] the normative statistics of the row-major f64 canvas `rgb` (width*height*3 doubles).
 *   A pixel contributes y = Y(c) when y > 0.0 && y < +inf; otherwise it contributes +0.0 and is not counted (NaN, negative,
 *   zero and infinite luminances alike).
 *   max starts at 0.0 and is the largest contributing y: independent of the order.
 *   sum: take the contributions in row-major order; reduce blocks of 256 consecutive values, the last block padded with +0.0:
 *   within a block, for s = 128, 64, ..., 1 do v[i] = v[i] + v[i+s] for every i < s, and v[0] is the block's result; reduce the
 *   block results the same way, level by level, until one value is left (a frame of at most 256 pixels: one level; an empty
 *   frame: one block of padding, sum +0.0).
 *   count is an integer sum.
 * RTC_ERR_ARG: a NULL pointer. RTC_ERR_NOMEM: no room for the block results (width*height/256 doubles). */
rtc_status  rtc_canvas_luminance(const double *rgb, uint32_t width, uint32_t height, rtc_luminance *out);
/* [device] the same record for a canvas in DEVICE memory, written into DEVICE memory at d_out (24 bytes), enqueued on the
 * context's stream (k_lum_pixels, then k_lum_records per further level, csrc/rtc_post.hip: one launch per level, at most three
 * below 2^24 pixels); no host wait, so rtc_canvas_tonemap_device can read it in stream order. Ordering and alignment are
 * rtc_canvas_apply_ao_device's: d_rgb and d_out 8-byte aligned, else RTC_ERR_ARG and nothing is launched. More than 2^32-256
 * pixels (2^24-1 workgroups of 256) is RTC_ERR_ARG. The levels' block results go to a grow-only buffer of the context. */
rtc_status  rtc_canvas_luminance_device(rtc_context *ctx, const void *d_rgb, uint32_t width, uint32_t height, void *d_out);

#define RTC_TONEMAP_LINEAR   0u
#define RTC_TONEMAP_REINHARD 1u
#define RTC_TONEMAP_ACES     2u
#define RTC_TONEMAP_AUTO_EXPOSURE 1u  /* flags: `exposure` is the key (0.18, say) that the frame's mean luminance is mapped to */
#define RTC_TONEMAP_AUTO_WHITE    2u  /* flags: the white point is the frame's largest luminance after exposure */
typedef struct rtc_tonemap {
    double   exposure;         /* finite, > 0: the multiplier, or the key with RTC_TONEMAP_AUTO_EXPOSURE */
    double   white;            /* > 0, +inf allowed (plain Reinhard): the luminance REINHARD maps to 1; ignored with AUTO_WHITE */
    uint32_t curve;            /* RTC_TONEMAP_* */
    uint32_t flags;            /* RTC_TONEMAP_AUTO_* */
} rtc_tonemap;                 /* 24 bytes */
/* [host] RTC_ERR_ARG for NULL, an exposure that is not finite and > 0, a white that is not > 0 (NaN included), an unknown
 * curve or an unknown flag bit; else RTC_OK. */
rtc_status  rtc_tonemap_validate(const rtc_tonemap *spec);
/* [host] the normative multiplier and white term of a frame. `stats` may be NULL without AUTO flags and is RTC_ERR_ARG
 * with them; an invalid spec or a NULL output is RTC_ERR_ARG.
 *   m = exposure. With AUTO_EXPOSURE: mean = sum / (double)count, and m = exposure / mean when count > 0 && mean > 0.0,
 *   else m = 1.0.
 *   Lw = white. With AUTO_WHITE: Lw = max * m.
 *   inv_w2 = 1.0 / (Lw*Lw) when Lw > 0.0 && Lw < +inf, else 0.0. */
rtc_status  rtc_tonemap_resolve(const rtc_tonemap *spec, const rtc_luminance *stats, double *m, double *inv_w2);
/* [host] the normative tone map of `in` (width*height*3 doubles) into `out`, which may be `in`. Per pixel first c' = c * m
 * per channel, then
 *   LINEAR:   c'.
 *   REINHARD  (extended, on luminance): L = Y(c'). If !(L > 0.0) the pixel is c'. Otherwise s = (1.0 + (L*inv_w2)) / (1.0 + L)
 *             and out = c' * s per channel.
 *   ACES      (Narkowicz's fit, per channel x = c'): if !(x > 0.0) the result is 0.0. Otherwise a = (2.51*x) + 0.03,
 *             b = (2.43*x) + 0.59, o = (x*a) / ((x*b) + 0.14); the result is 1.0 if o > 1.0, else o.
 * `stats` as in rtc_tonemap_resolve. RTC_ERR_ARG: a NULL canvas, an invalid spec, AUTO flags without stats. */
rtc_status  rtc_canvas_tonemap(const double *in, uint32_t width, uint32_t height, const rtc_tonemap *spec,
                               const rtc_luminance *stats, double *out);
/* [device] the same bytes for canvases in DEVICE memory (k_tonemap, one thread per pixel). d_stats is the record
 * rtc_canvas_luminance_device left in DEVICE memory: every thread derives m and inv_w2 from it, so an auto-exposed frame
 * never waits for the stream. d_stats may be NULL without AUTO flags. d_out may be d_in. Ordering, alignment and the largest
 * frame as above. */
rtc_status  rtc_canvas_tonemap_device(rtc_context *ctx, const void *d_in, uint32_t width, uint32_t height, const rtc_tonemap *spec,
                                      const void *d_stats, void *d_out);

#define RTC_MAX_BLOOM_RADIUS 32u
typedef struct rtc_bloom {
    double   threshold;        /* finite, >= 0: only luminance above it glares */
    double   strength;         /* finite, >= 0: how much of the blurred bright pass is added */
    double   sigma;            /* finite, > 0, in pixels; (2.0*sigma)*sigma must be > 0.0 too (no underflow) */
    uint32_t radius;           /* 1..RTC_MAX_BLOOM_RADIUS: 2*radius + 1 taps per axis */
    uint32_t _pad;             /* 0 */
} rtc_bloom;                   /* 32 bytes */
/* [host] RTC_ERR_ARG for NULL or a field outside the ranges above; else RTC_OK. */
rtc_status  rtc_bloom_validate(const rtc_bloom *spec);
/* [host only] the normative weights w[0 .. 2*radius]: g[k] = exp(-((double)(k*k)) / ((2.0*sigma)*sigma)) for k = -R..R;
 * sum adds the g[k] in k order, starting at 0.0; w[k+R] = g[k] / sum. The device never evaluates exp: the table travels in
 * the kernel arguments. RTC_ERR_ARG: an invalid spec, a NULL table. */
rtc_status  rtc_bloom_weights(const rtc_bloom *spec, double *w);
/* [host] the normative bloom of `in` (width*height*3 doubles, C) into `out`, which may be `in`.
 *   Bright pass B[p]: L = Y(C[p]). If !(L > threshold) || !(L < +inf), B is (+0.0, +0.0, +0.0). Otherwise
 *     k = (L - threshold) / L and B_c = C_c * k.
 *   Horizontal pass: H[x,y]_c starts acc = 0.0; for k = -R..R in order, acc = acc + (w[k+R] * B[x+k, y]_c). A tap outside
 *     the image has the value +0.0; adding it or skipping it gives the same bytes, since acc can never be -0.0.
 *   Vertical pass: V[x,y]_c the same over H[x, y+k]_c.
 *   Composite: out_c = C_c + (strength * V_c).
 * RTC_ERR_ARG: a NULL canvas, an invalid spec. RTC_ERR_NOMEM: no room for the two planes B and H. */
rtc_status  rtc_canvas_bloom(const double *in, uint32_t width, uint32_t height, const rtc_bloom *spec, double *out);
/* [device] the same bytes for canvases in DEVICE memory: k_bloom_h (bright pass at staging, a row segment and its halo in
 * LDS, H into a grow-only plane of the context), then k_bloom_v (a tile of H with its halo rows in LDS, one channel per
 * sweep, writes the composite). d_out may be d_in: the vertical pass reads C only at its own pixel. Ordering and alignment
 * as above. A frame of more than 2^24-1 row segments (ceil(width/256) * height) or 32 x 64 tiles is RTC_ERR_ARG: a launch
 * holds fewer than 2^32 threads. A second call of the same size allocates nothing. */
rtc_status  rtc_canvas_bloom_device(rtc_context *ctx, const void *d_in, uint32_t width, uint32_t height, const rtc_bloom *spec,
                                    void *d_out);
/* Scenes whose camera asks for post-processing. YAML: `add: camera` with any of
 *   tonemap-curve (linear | reinhard | aces; default reinhard), tonemap-exposure (finite, > 0; default 1.0), tonemap-key (finite,
 *   > 0: sets RTC_TONEMAP_AUTO_EXPOSURE with that key and excludes tonemap-exposure), tonemap-white (a number > 0, .inf, or
 *   `auto`: RTC_TONEMAP_AUTO_WHITE; default .inf);
 *   bloom-threshold (default 1.0), bloom-strength (default 0.5), bloom-sigma (default 2.0), bloom-radius (integer; default 6).
 * These entries are rtc_scene_load_yaml_area_lights plus the two records: *has_tonemap_out = 1 and *tonemap_out filled when
 * the camera has any tonemap-* key, else 0 and the record zeroed; the bloom-* keys and *bloom_out alike. A value outside a
 * record's ranges, or tonemap-key together with tonemap-exposure, is RTC_ERR_PARSE with a message. Every other YAML entry
 * ignores the keys. */
rtc_status  rtc_scene_load_yaml_post(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                     struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                     rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                     rtc_tonemap *tonemap_out, uint32_t *has_tonemap_out, rtc_bloom *bloom_out, uint32_t *has_bloom_out);
rtc_status  rtc_scene_load_yaml_post_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                          struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                          rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                          rtc_tonemap *tonemap_out, uint32_t *has_tonemap_out, rtc_bloom *bloom_out, uint32_t *has_bloom_out);

/* ==== resizing f64 canvases: five filters, a host statement, the same bytes on the device ============= */
/* A frame traced at 2x or 3x and filtered down is anti-aliasing for every launch family that has none of its own
 * (orthographic and panorama frames, the lens, AOV views, AO and gather planes); a small plane filtered up can be composited
 * over a full-size frame. The resize sits between rtc_canvas_bloom / rtc_canvas_tonemap and rtc_canvas_to_rgba8 or an encoder.
 * Frames are linear: there is no gamma-aware resize, no 8-bit resize and no resize of uint16 count planes (convert those with
 * rtc_counts_to_fraction first).
 *
 * Arithmetic: f64 throughout, no fused multiply-add, the operations in exactly the order written here.
 *
 * The filters k(x), each 0.0 outside its radius R; a = fabs(x):
 *   BOX          R = 0.5  1.0 when x > -0.5 && x <= 0.5
 *   TRIANGLE     R = 1    a < 1: 1.0 - a
 *   CATMULL_ROM  R = 2    a < 1: ((((1.5*a) - 2.5)*a)*a) + 1.0;  a < 2: (((((-0.5*a) + 2.5)*a) - 4.0)*a) + 2.0
 *   MITCHELL     R = 2    (B = C = 1/3) a < 1: (((((7.0*a) - 12.0)*a)*a) + (16.0/3.0)) / 6.0;
 *                         a < 2: (((((((-7.0/3.0)*a) + 12.0)*a) - 20.0)*a) + (32.0/3.0)) / 6.0
 *   LANCZOS3     R = 3    x == 0: 1.0;  a < 3: p = 3.141592653589793*x, q = p/3.0, (sin(p)/p) * (sin(q)/q)
 *
 * The table of one axis, n_in -> n_out (what Pillow does: taps outside the image are dropped, the rest renormalised):
 *   scale = (double)n_in / (double)n_out;  fs = scale > 1.0 ? scale : 1.0;  support = R*fs.
 *   For output o: c = ((double)o + 0.5)*scale;
 *     first = max(0, floor((c - support) + 0.5));  end = min(n_in, floor((c + support) + 0.5));  count = end - first.
 *     raw[j] = k(((((double)(first + j)) + 0.5) - c) / fs) for j = 0 .. count-1;
 *     sum adds the raw[j] in j order, starting at 0.0;  w[j] = raw[j] / sum.
 * An axis with n_in == n_out is NOT filtered, whatever the filter (Mitchell, which does not interpolate, included): its
 * table is first = o, count = 1, w = 1.0 and its pass copies the values' bytes. A resize to the same size returns the input.
 *
 * The frame: the horizontal pass first, w_in x h_in -> w_out x h_in, then the vertical pass -> w_out x h_out; the order is
 * fixed. One output channel of a filtered pass is acc = 0.0; for j = 0 .. count-1 in order: acc = acc + (w[j] * v[first + j]);
 * a NaN result is stored as 0x7FF8000000000000. A NaN or an infinity of the input reaches exactly the outputs whose taps
 * cover it on both axes (0.0 * inf is NaN, and is kept). */
enum { RTC_RESIZE_BOX = 0, RTC_RESIZE_TRIANGLE = 1, RTC_RESIZE_CATMULL_ROM = 2, RTC_RESIZE_MITCHELL = 3, RTC_RESIZE_LANCZOS3 = 4 };
/* An axis may have at most this many taps per output (a condition, not a tuning value): one output's source span is then at
 * most 24 KiB of pixels, which fits a workgroup's LDS even when the workgroup handles a single output column. */
#define RTC_MAX_RESIZE_TAPS 1024u
typedef struct rtc_resize {
    uint32_t filter;           /* RTC_RESIZE_* */
    uint32_t _pad;             /* 0 */
} rtc_resize;                  /* 8 bytes */
/* [host] RTC_ERR_ARG for NULL, an unknown filter or _pad != 0; else RTC_OK. */
rtc_status  rtc_resize_validate(const rtc_resize *spec);
/* [host] the largest count of the axis n_in -> n_out under `filter` (1 when n_in == n_out); 0 for a zero size or an unknown
 * filter. The value may exceed RTC_MAX_RESIZE_TAPS: such an axis is refused by the entries below. */
uint32_t    rtc_resize_taps(uint32_t n_in, uint32_t n_out, uint32_t filter);
/* [host] the normative table of one axis: first[o], count[o] and w[o*taps + j] for o < n_out, taps = rtc_resize_taps(n_in,
 * n_out, filter), each row of w zero-padded past count[o]. RTC_ERR_ARG: a NULL pointer, a zero size, an invalid spec, more
 * than RTC_MAX_RESIZE_TAPS taps. RTC_ERR_NOMEM: no room for the raw weights of one output. */
rtc_status  rtc_resize_weights(uint32_t n_in, uint32_t n_out, const rtc_resize *spec, uint32_t *first, uint32_t *count, double *w);
/* [host] the normative resize of `in` (w_in*h_in*3 doubles, row-major) into `out` (w_out*h_out*3 doubles). RTC_ERR_ARG, with
 * `out` untouched: a NULL pointer, a zero size, an invalid spec, an axis of more than RTC_MAX_RESIZE_TAPS taps, `out`
 * overlapping `in`. RTC_ERR_NOMEM: no room for the tables or the intermediate w_out x h_in frame. */
rtc_status  rtc_canvas_resize(const double *in, uint32_t w_in, uint32_t h_in, const rtc_resize *spec, double *out, uint32_t w_out,
                              uint32_t h_out);
/* [device] the same bytes for canvases in DEVICE memory, enqueued on the context's stream (csrc/rtc_resize.hip: k_resize_h,
 * then k_resize_v; an unchanged axis has no pass, and a resize to the same size is k_resize_copy). Nothing on the device
 * evaluates a filter: the tables of an axis are built on the host by rtc_resize_weights' own function, uploaded to a
 * grow-only device buffer and cached by the context for the last four (n_in, n_out, filter) triples. A call whose tables are
 * cached does not wait for the stream and uploads nothing; a MISS WAITS FOR THE CONTEXT'S STREAM before it replaces the
 * least recently used tables, as a new panorama size does. The intermediate frame is a grow-only plane of the context.
 * d_in and d_out 8-byte aligned and not overlapping, else RTC_ERR_ARG; the host entry's refusals hold too, and a pass whose
 * grid would reach 2^32 threads (2^24 - 1 workgroups of 256) is RTC_ERR_ARG. Nothing is launched by a refused call. */
rtc_status  rtc_canvas_resize_device(rtc_context *ctx, const void *d_in, uint32_t w_in, uint32_t h_in, const rtc_resize *spec,
                                     void *d_out, uint32_t w_out, uint32_t h_out);
/* Scenes whose camera asks for a delivered size other than the traced one. YAML: `add: camera` with any of
 *   output-width, output-height (integers, 1 .. 2^31-1; an absent one keeps the frame's aspect: out_h = max(1,
 *   floor(((double)out_w * (double)height) / (double)width + 0.5)), and alike for out_w),
 *   output-filter (box | triangle | catmull-rom | mitchell | lanczos3; default lanczos3).
 * These entries are rtc_scene_load_yaml_projection plus the record: *has_resize_out = 1, *resize_out, *out_w and *out_h
 * filled when the camera has any output-* key; else 0, the record zeroed and *out_w, *out_h the camera's own size. A value
 * outside the ranges, or output-filter alone, is RTC_ERR_PARSE with a message. Every other YAML entry ignores the keys. */
rtc_status  rtc_scene_load_yaml_resize(const char *text, rtc_shape **shapes_out, uint32_t *n_out,
                                       struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                       rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                       rtc_lens *lens_out, uint32_t *has_lens_out, rtc_projection *proj_out, uint32_t *has_proj_out,
                                       rtc_resize *resize_out, uint32_t *out_w, uint32_t *out_h, uint32_t *has_resize_out);
rtc_status  rtc_scene_load_yaml_resize_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out,
                                            struct rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out,
                                            rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                            rtc_lens *lens_out, uint32_t *has_lens_out, rtc_projection *proj_out, uint32_t *has_proj_out,
                                            rtc_resize *resize_out, uint32_t *out_w, uint32_t *out_h, uint32_t *has_resize_out);

#ifdef __cplusplus
}
#endif
#endif /* RTC_H */
