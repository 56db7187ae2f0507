// host_math.cpp — [host] setup arithmetic behind include/rtc.h.
//
// These run once per scene on the CPU (never per pixel) and produce the exact f64 bit
// patterns the Rust reference would hold in its Matrix / Camera / Shape structs, so that
// what is uploaded to the GPU is what `World` would contain. Operation order follows
// ch1/src/transform.rs and ch1/src/camera.rs (cited per function); compiled with
// -ffp-contract=off.
#include "rtc.h"

#include <cmath>
#include <math.h>
#include <cstdlib>
#include <cstring>

namespace {

constexpr double kEpsilon = RTC_EPSILON; // Vector::EPSILON vec.rs:16

struct Mat4 {
    double v[16];
    double &at(int r, int c) { return v[r * 4 + c]; }
    double at(int r, int c) const { return v[r * 4 + c]; }
};

// multiply_arrays (transform.rs:8-21): sum starts at zero, products added in i order.
Mat4 mul(const Mat4 &a, const Mat4 &b) {
    Mat4 out;
    for (int row = 0; row < 4; ++row)
        for (int col = 0; col < 4; ++col) {
            double sum = 0.0;
            for (int i = 0; i < 4; ++i) {
                const double prod = a.at(row, i) * b.at(i, col);
                sum = sum + prod;
            }
            out.at(row, col) = sum;
        }
    return out;
}

// Matrix::determinant / submatrix / minor / cofactor (transform.rs:130-169), generic in the
// order (2, 3 or 4) exactly like the reference's recursion on Array2D.
template <int N> struct Sq { double v[N * N]; };

template <int N> double det(const Sq<N> &m);
template <> double det<2>(const Sq<2> &m) { return m.v[0] * m.v[3] - m.v[1] * m.v[2]; }

template <int N> double cofactor(const Sq<N> &m, int i, int j) {
    Sq<N - 1> sub;
    for (int row = 0; row < N - 1; ++row)
        for (int col = 0; col < N - 1; ++col)
            sub.v[row * (N - 1) + col] = m.v[(row < i ? row : row + 1) * N + (col < j ? col : col + 1)];
    double minor = det<N - 1>(sub);
    if ((i + j) % 2 == 1) minor = -1.0 * minor;
    return minor;
}

template <int N> double det(const Sq<N> &m) {
    double d = 0.0;
    for (int col = 0; col < N; ++col) d += m.v[col] * cofactor<N>(m, 0, col);
    return d;
}

Sq<4> as_sq(const double m[16]) {
    Sq<4> s;
    std::memcpy(s.v, m, sizeof s.v);
    return s;
}

Mat4 load(const double m[16]) {
    Mat4 r;
    std::memcpy(r.v, m, sizeof r.v);
    return r;
}
void store(const Mat4 &m, double out[16]) { std::memcpy(out, m.v, sizeof m.v); }

// new.multiply(self) — every fluent builder left-multiplies (transform.rs:59,68,77,86,95,104).
void left_apply(const double elems[16], const double m[16], double out[16]) {
    store(mul(load(elems), load(m)), out);
}

struct V3 { double x, y, z; };
V3 normalize(V3 a) { // vec.rs:65-76: sqrt of the sum, then three divisions
    const double mag = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    return V3{a.x / mag, a.y / mag, a.z / mag};
}
V3 cross(V3 a, V3 b) { // vec.rs:84-90
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

} // namespace

extern "C" {

uint32_t rtc_abi_version(void) { return RTC_ABI_VERSION; }

const char *rtc_strerror(rtc_status s) {
    switch (s) {
    case RTC_OK: return "ok";
    case RTC_ERR_SINGULAR: return "Matrix is not invertable";
    case RTC_ERR_NO_COLOR: return "must specify a color on materials when no pattern is used";
    case RTC_ERR_DEVICE: return "no usable MI355X (gfx950) device or HIP runtime error";
    case RTC_ERR_ARG: return "invalid argument";
    case RTC_ERR_PARSE: return "scene description rejected";
    case RTC_ERR_IO: return "file i/o failed";
    case RTC_ERR_NOMEM: return "out of memory";
    case RTC_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
    }
}

void rtc_matrix_identity(double out[16]) { // transform.rs:44-51
    for (int i = 0; i < 16; ++i) out[i] = (i % 5 == 0) ? 1. : 0.;
}

void rtc_matrix_multiply(const double a[16], const double b[16], double out[16]) {
    store(mul(load(a), load(b)), out);
}

void rtc_matrix_translation(const double m[16], double x, double y, double z, double out[16]) {
    const double e[16] = {1., 0., 0., x, 0., 1., 0., y, 0., 0., 1., z, 0., 0., 0., 1.};
    left_apply(e, m, out);
}
void rtc_matrix_scaling(const double m[16], double x, double y, double z, double out[16]) {
    const double e[16] = {x, 0., 0., 0., 0., y, 0., 0., 0., 0., z, 0., 0., 0., 0., 1.};
    left_apply(e, m, out);
}
// r.sin() / r.cos() of one angle: an optimised rustc build (x86_64-unknown-linux-gnu) lowers the
// pair to ONE glibc sincos() call, whose results differ from separate sin()/cos() calls by 1 ulp
// for about 0.14 % of angles. We follow the release build explicitly (DESIGN.md "sincos").
static void sin_cos(double r, double &s, double &c) { ::sincos(r, &s, &c); }

void rtc_matrix_rotation_x(const double m[16], double r, double out[16]) { // :71-78
    double sn, cs;
    sin_cos(r, sn, cs);
    const double e[16] = {1., 0., 0., 0., 0., cs, -sn, 0., 0., sn, cs, 0., 0., 0., 0., 1.};
    left_apply(e, m, out);
}
void rtc_matrix_rotation_y(const double m[16], double r, double out[16]) { // :80-87
    double sn, cs;
    sin_cos(r, sn, cs);
    const double e[16] = {cs, 0., sn, 0., 0., 1., 0., 0., -sn, 0., cs, 0., 0., 0., 0., 1.};
    left_apply(e, m, out);
}
void rtc_matrix_rotation_z(const double m[16], double r, double out[16]) { // :89-96
    double sn, cs;
    sin_cos(r, sn, cs);
    const double e[16] = {cs, -sn, 0., 0., sn, cs, 0., 0., 0., 0., 1., 0., 0., 0., 0., 1.};
    left_apply(e, m, out);
}
void rtc_matrix_shearing(const double m[16], double xy, double xz, double yx, double yz,
                         double zx, double zy, double out[16]) { // :98-105
    const double e[16] = {1., xy, xz, 0., yx, 1., yz, 0., zx, zy, 1., 0., 0., 0., 0., 1.};
    left_apply(e, m, out);
}

double rtc_matrix_determinant(const double m[16]) { return det<4>(as_sq(m)); }

rtc_status rtc_matrix_inverse(const double m[16], double out[16]) { // transform.rs:35-38,175-190
    if (!m || !out) return RTC_ERR_ARG;
    const Sq<4> s = as_sq(m);
    const double d = det<4>(s);
    if (!(std::fabs(d) > kEpsilon)) return RTC_ERR_SINGULAR;
    Mat4 inv;
    for (int row = 0; row < 4; ++row)
        for (int col = 0; col < 4; ++col) inv.at(col, row) = cofactor<4>(s, row, col) / d;
    store(inv, out);
    return RTC_OK;
}

void rtc_matrix_transpose(const double m[16], double out[16]) { // transform.rs:192-202
    Mat4 t;
    const Mat4 src = load(m);
    for (int row = 0; row < 4; ++row)
        for (int col = 0; col < 4; ++col) t.at(row, col) = src.at(col, row);
    store(t, out);
}

void rtc_view_transform(const double from[3], const double to[3], const double up[3], double out[16]) {
    // transform.rs:204-217
    const V3 forward = normalize(V3{to[0] - from[0], to[1] - from[1], to[2] - from[2]});
    const V3 upn = normalize(V3{up[0], up[1], up[2]});
    const V3 left = cross(forward, upn);
    const V3 true_up = cross(left, forward);
    const double orient[16] = {left.x, left.y, left.z, 0., true_up.x, true_up.y, true_up.z, 0.,
                               -(forward.x), -(forward.y), -(forward.z), 0., 0., 0., 0., 1.};
    double id[16], shift[16];
    rtc_matrix_identity(id);
    rtc_matrix_translation(id, -from[0], -from[1], -from[2], shift);
    rtc_matrix_multiply(orient, shift, out);
}

rtc_status rtc_camera_init(uint32_t hsize, uint32_t vsize, double fov, const double view[16],
                           rtc_camera *out) { // camera.rs:33-58
    if (!out || !view || hsize == 0 || vsize == 0) return RTC_ERR_ARG;
    std::memset(out, 0, sizeof *out);
    const double half_view = std::tan(fov / 2.0);
    const double aspect = static_cast<double>(hsize) / static_cast<double>(vsize);
    if (aspect < 1.0) {
        out->half_height = half_view;
        out->half_width = half_view * aspect;
    } else {
        out->half_width = half_view;
        out->half_height = half_view / aspect;
    }
    out->pixel_size = (out->half_width * 2.) / static_cast<double>(hsize);
    out->hsize = hsize;
    out->vsize = vsize;
    out->fov = fov;
    out->samples = 1;
    return rtc_matrix_inverse(view, out->view_inv);
}

static void xform_point(const double m[16], double x, double y, double z, double o[3]) {
    // Matrix::transform_point transform.rs:122-128
    o[0] = m[0] * x + m[1] * y + m[2] * z + m[3];
    o[1] = m[4] * x + m[5] * y + m[6] * z + m[7];
    o[2] = m[8] * x + m[9] * y + m[10] * z + m[11];
}

void rtc_camera_ray_for_pixel(const rtc_camera *cam, uint32_t x, double x_offset, uint32_t y,
                              double y_offset, double ray[6]) { // camera.rs:64-76
    const double xoffset = (static_cast<double>(x) + x_offset) * cam->pixel_size;
    const double yoffset = (static_cast<double>(y) + y_offset) * cam->pixel_size;
    const double world_x = cam->half_width - xoffset;
    const double world_y = cam->half_height - yoffset;
    double pixel[3], origin[3];
    xform_point(cam->view_inv, world_x, world_y, -1., pixel);
    xform_point(cam->view_inv, 0., 0., 0., origin);
    const V3 dir = normalize(V3{pixel[0] - origin[0], pixel[1] - origin[1], pixel[2] - origin[2]});
    ray[0] = origin[0]; ray[1] = origin[1]; ray[2] = origin[2];
    ray[3] = dir.x; ray[4] = dir.y; ray[5] = dir.z;
}

rtc_status rtc_lens_validate(const rtc_lens *lens) {
    if (!lens) return RTC_ERR_ARG;
    if (!std::isfinite(lens->aperture) || lens->aperture < 0.) return RTC_ERR_ARG;
    if (!std::isfinite(lens->focal_distance) || !(lens->focal_distance > 0.)) return RTC_ERR_ARG;
    if (lens->usteps == 0u || lens->vsteps == 0u) return RTC_ERR_ARG;
    if ((uint64_t)lens->usteps * lens->vsteps > RTC_MAX_LENS_SAMPLES) return RTC_ERR_ARG;
    return RTC_OK;
}

// (here, beside the other records the scene loader validates; the rest of the ambient-occlusion pass: host_ao.cpp)
rtc_status rtc_ao_validate(const rtc_ao *ao) {
    if (!ao) return RTC_ERR_ARG;
    if (!(ao->radius > 0.)) return RTC_ERR_ARG; // (NaN fails the test; +inf passes: unbounded)
    if (ao->usteps == 0u || ao->vsteps == 0u) return RTC_ERR_ARG;
    if ((uint64_t)ao->usteps * ao->vsteps > RTC_MAX_AO_SAMPLES) return RTC_ERR_ARG;
    return RTC_OK;
}

// The normative thin-lens ray (include/rtc.h): camera.rs:64-76 with the origin moved over the lens and the target on the
// plane in focus; mul, add and div in the stated order (this file is compiled with -ffp-contract=off).
rtc_status rtc_lens_ray(const rtc_camera *cam, const rtc_lens *lens, uint32_t x, uint32_t y, uint32_t k, double ray[6]) {
    if (!cam || !ray || rtc_lens_validate(lens) != RTC_OK || k >= lens->usteps * lens->vsteps) return RTC_ERR_ARG;
    const uint32_t u = k % lens->usteps, v = k / lens->usteps;
    const double xoffset = (static_cast<double>(x) + 0.5) * cam->pixel_size;
    const double yoffset = (static_cast<double>(y) + 0.5) * cam->pixel_size;
    const double world_x = cam->half_width - xoffset;
    const double world_y = cam->half_height - yoffset;
    const double ucell = (2.0 * lens->aperture) / static_cast<double>(lens->usteps);
    const double vcell = (2.0 * lens->aperture) / static_cast<double>(lens->vsteps);
    const double lu = -lens->aperture + ucell * (static_cast<double>(u) + 0.5);
    const double lv = -lens->aperture + vcell * (static_cast<double>(v) + 0.5);
    double origin[3], target[3];
    xform_point(cam->view_inv, lu, lv, 0., origin);
    xform_point(cam->view_inv, world_x * lens->focal_distance, world_y * lens->focal_distance, -lens->focal_distance, target);
    const V3 dir = normalize(V3{target[0] - origin[0], target[1] - origin[1], target[2] - origin[2]});
    ray[0] = origin[0]; ray[1] = origin[1]; ray[2] = origin[2];
    ray[3] = dir.x; ray[4] = dir.y; ray[5] = dir.z;
    return RTC_OK;
}

rtc_status rtc_projection_validate(const rtc_projection *p) {
    if (!p) return RTC_ERR_ARG;
    if (p->kind == RTC_PROJ_ORTHOGRAPHIC) return std::isfinite(p->width) && p->width > 0. ? RTC_OK : RTC_ERR_ARG;
    if (p->kind != RTC_PROJ_PANORAMA) return RTC_ERR_ARG;
    if (!(p->h_span > 0.) || !(p->h_span <= 2.0 * M_PI)) return RTC_ERR_ARG; // (NaN fails the first test)
    if (!(p->v_span > 0.) || !(p->v_span <= M_PI)) return RTC_ERR_ARG;
    return RTC_OK;
}

// half_w, half_h and pixel of the orthographic rays (include/rtc.h): Camera::new's aspect rule with width / 2 for the half view
extern "C" void rtc_projection_ortho_terms(uint32_t hsize, uint32_t vsize, double width, double out[3]) {
    const double half_view = width / 2.0;
    const double aspect = static_cast<double>(hsize) / static_cast<double>(vsize);
    if (aspect < 1.0) {
        out[1] = half_view;
        out[0] = half_view * aspect;
    } else {
        out[0] = half_view;
        out[1] = half_view / aspect;
    }
    out[2] = (out[0] * 2.0) / static_cast<double>(hsize);
}

// {sin, cos} of cell i of n over `span` (include/rtc.h): the one place the panorama's angles are evaluated
static void pano_entry(double span, uint32_t i, uint32_t n, double out[2]) {
    const double a = span * (0.5 - (static_cast<double>(i) + 0.5) / static_cast<double>(n));
    out[0] = std::sin(a);
    out[1] = std::cos(a);
}

rtc_status rtc_projection_tables(const rtc_camera *cam, const rtc_projection *p, double *col, double *row) {
    if (!cam || !col || !row || rtc_projection_validate(p) != RTC_OK || p->kind != RTC_PROJ_PANORAMA) return RTC_ERR_ARG;
    if (cam->hsize == 0u || cam->vsize == 0u) return RTC_ERR_ARG;
    for (uint32_t x = 0; x < cam->hsize; ++x) pano_entry(p->h_span, x, cam->hsize, col + 2u * static_cast<size_t>(x));
    for (uint32_t y = 0; y < cam->vsize; ++y) pano_entry(p->v_span, y, cam->vsize, row + 2u * static_cast<size_t>(y));
    return RTC_OK;
}

// The normative projection ray (include/rtc.h); mul, add and div in the stated order (this file is compiled with -ffp-contract=off).
rtc_status rtc_projection_ray(const rtc_camera *cam, const rtc_projection *p, uint32_t x, uint32_t y, double ray[6]) {
    if (!cam || !ray || rtc_projection_validate(p) != RTC_OK || x >= cam->hsize || y >= cam->vsize) return RTC_ERR_ARG;
    double origin[3], target[3];
    if (p->kind == RTC_PROJ_ORTHOGRAPHIC) {
        double t[3];
        rtc_projection_ortho_terms(cam->hsize, cam->vsize, p->width, t);
        const double world_x = t[0] - (static_cast<double>(x) + 0.5) * t[2];
        const double world_y = t[1] - (static_cast<double>(y) + 0.5) * t[2];
        xform_point(cam->view_inv, world_x, world_y, 0., origin);
        xform_point(cam->view_inv, world_x, world_y, -1., target);
    } else {
        double c[2], r[2];
        pano_entry(p->h_span, x, cam->hsize, c);
        pano_entry(p->v_span, y, cam->vsize, r);
        xform_point(cam->view_inv, 0., 0., 0., origin);
        xform_point(cam->view_inv, r[1] * c[0], r[0], -(r[1] * c[1]), target);
    }
    const V3 dir = normalize(V3{target[0] - origin[0], target[1] - origin[1], target[2] - origin[2]});
    ray[0] = origin[0]; ray[1] = origin[1]; ray[2] = origin[2];
    ray[3] = dir.x; ray[4] = dir.y; ray[5] = dir.z;
    return RTC_OK;
}

void rtc_material_default(rtc_material *out) { // material.rs:273-283 + 364-369 (WHITE)
    std::memset(out, 0, sizeof *out);
    out->pattern_kind = RTC_PATTERN_NONE;
    out->has_color = 1;
    out->color[0] = out->color[1] = out->color[2] = 1.;
    out->ambient = 0.1;
    out->diffuse = 0.9;
    out->specular = 0.9;
    out->shininess = 200.0;
    out->reflective = 0.0;
    out->transparency = 0.0;
    out->refractive_index = 1.0;
    rtc_matrix_identity(out->pat_inv);
}

rtc_status rtc_material_set_pattern(rtc_material *mat, uint32_t pattern_kind, const double a[3],
                                    const double b[3], const double transform[16]) {
    if (!mat || pattern_kind > RTC_PATTERN_GRID) return RTC_ERR_ARG;
    mat->pattern_kind = pattern_kind;
    for (int i = 0; i < 3; ++i) {
        mat->pat_a[i] = a ? a[i] : 0.;
        mat->pat_b[i] = b ? b[i] : 0.;
    }
    if (transform) return rtc_matrix_inverse(transform, mat->pat_inv); // Pattern::set_transform
    rtc_matrix_identity(mat->pat_inv);
    return RTC_OK;
}

void rtc_light_default(rtc_light *out) { // material.rs:26-31
    out->intensity[0] = out->intensity[1] = out->intensity[2] = 1.;
    out->position[0] = -10.;
    out->position[1] = 10.;
    out->position[2] = -10.;
}

rtc_status rtc_area_light_from_point(const rtc_light *light, rtc_area_light *out) {
    if (!light || !out) return RTC_ERR_ARG;
    std::memset(out, 0, sizeof *out);
    for (int k = 0; k < 3; ++k) {
        out->intensity[k] = light->intensity[k];
        out->corner[k] = light->position[k];
    }
    out->usteps = out->vsteps = 1u;
    return RTC_OK;
}

// The normative sample list (include/rtc.h): cell centres, v outer, u inner; mul, add and div in the stated order (this
// file is compiled with -ffp-contract=off).
rtc_status rtc_area_light_expand(const rtc_area_light *lights, uint32_t n, rtc_light *out, uint32_t cap, uint32_t *n_out) {
    if (n_out) *n_out = 0;
    if (!lights || !out || !n_out || n == 0u) return RTC_ERR_ARG;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (lights[i].usteps == 0u || lights[i].vsteps == 0u) return RTC_ERR_ARG;
        total += (uint64_t)lights[i].usteps * lights[i].vsteps; // each product < 2^64; the running sum is checked at once
        if (total > RTC_MAX_LIGHT_SAMPLES) return RTC_ERR_ARG;
    }
    if (total > cap) return RTC_ERR_ARG;
    uint32_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const rtc_area_light &a = lights[i];
        double ucell[3], vcell[3], inten[3];
        for (int k = 0; k < 3; ++k) {
            ucell[k] = a.uvec[k] / (double)a.usteps;
            vcell[k] = a.vvec[k] / (double)a.vsteps;
            inten[k] = a.intensity[k] / (double)(a.usteps * a.vsteps);
        }
        for (uint32_t v = 0; v < a.vsteps; ++v)
            for (uint32_t u = 0; u < a.usteps; ++u, ++at)
                for (int k = 0; k < 3; ++k) {
                    out[at].position[k] = (a.corner[k] + ucell[k] * ((double)u + 0.5)) + vcell[k] * ((double)v + 0.5);
                    out[at].intensity[k] = inten[k];
                }
    }
    *n_out = at;
    return RTC_OK;
}

rtc_status rtc_shape_init(uint32_t kind, const double transform[16], const rtc_material *mat,
                          rtc_shape *out) { // shape.rs:308-317, 436-444, 525-533
    if (!out || !transform || kind > RTC_CUBE) return RTC_ERR_ARG;
    std::memset(out, 0, sizeof *out);
    out->kind = kind;
    const rtc_status st = rtc_matrix_inverse(transform, out->inv);
    if (st != RTC_OK) return st;
    rtc_matrix_transpose(out->inv, out->inv_t);
    if (mat) out->material = *mat;
    else rtc_material_default(&out->material);
    return RTC_OK;
}

// ---- motion blur: the normative shutter arithmetic (include/rtc.h); mul, add and div in the stated order (this file is
// compiled with -ffp-contract=off) ----

static bool shutter_ok(uint32_t n, uint32_t k) { return n >= 1u && n <= RTC_MAX_SHUTTER_SAMPLES && k < n; }

static void shutter_lerp(const double a[16], const double b[16], double t, double out[16]) {
    for (int i = 0; i < 16; ++i) out[i] = (a[i] == b[i]) ? a[i] : a[i] + (b[i] - a[i]) * t;
}

// Every motion names a shape of the list, none twice.
static rtc_status shutter_check_motions(const rtc_motion *motions, uint32_t n_motions, uint32_t n_shapes) {
    if (n_motions && !motions) return RTC_ERR_ARG;
    for (uint32_t i = 0; i < n_motions; ++i) {
        if (motions[i].shape >= n_shapes) return RTC_ERR_ARG;
        for (uint32_t j = 0; j < i; ++j)
            if (motions[j].shape == motions[i].shape) return RTC_ERR_ARG;
    }
    return RTC_OK;
}

double rtc_shutter_time(uint32_t n, uint32_t k) {
    if (!shutter_ok(n, k)) return std::nan("");
    return (static_cast<double>(k) + 0.5) / static_cast<double>(n);
}

rtc_status rtc_shutter_shapes(const rtc_shape *shapes, uint32_t n_shapes, const rtc_motion *motions, uint32_t n_motions,
                              uint32_t samples, uint32_t k, rtc_shape *out) {
    if ((n_shapes && (!shapes || !out)) || !shutter_ok(samples, k)) return RTC_ERR_ARG;
    const rtc_status ms = shutter_check_motions(motions, n_motions, n_shapes);
    if (ms != RTC_OK) return ms;
    const double t = rtc_shutter_time(samples, k);
    for (uint32_t i = 0; i < n_shapes; ++i) out[i] = shapes[i];
    for (uint32_t i = 0; i < n_motions; ++i) {
        double m[16];
        shutter_lerp(motions[i].transform_open, motions[i].transform_close, t, m);
        rtc_shape &s = out[motions[i].shape];
        const rtc_status st = rtc_matrix_inverse(m, s.inv); // what rtc_shape_init computes from M_k
        if (st != RTC_OK) return st;
        rtc_matrix_transpose(s.inv, s.inv_t);
    }
    return RTC_OK;
}

// rtc_shutter_shapes' verdict for EVERY k of the shutter, without building the shapes (csrc/rtc_shutter.cpp validates a
// whole frame before its first launch). Not part of include/rtc.h.
rtc_status rtc_shutter_check_motions(const rtc_motion *motions, uint32_t n_motions, uint32_t n_shapes, uint32_t samples) {
    if (!shutter_ok(samples, 0u)) return RTC_ERR_ARG;
    const rtc_status ms = shutter_check_motions(motions, n_motions, n_shapes);
    if (ms != RTC_OK) return ms;
    for (uint32_t k = 0; k < samples; ++k) {
        const double t = rtc_shutter_time(samples, k);
        for (uint32_t i = 0; i < n_motions; ++i) {
            double m[16], inv[16];
            shutter_lerp(motions[i].transform_open, motions[i].transform_close, t, m);
            const rtc_status st = rtc_matrix_inverse(m, inv);
            if (st != RTC_OK) return st;
        }
    }
    return RTC_OK;
}

rtc_status rtc_shutter_camera(const rtc_camera *open, const rtc_camera *close, uint32_t samples, uint32_t k, rtc_camera *out) {
    if (!open || !out || !shutter_ok(samples, k)) return RTC_ERR_ARG;
    if (!close) {
        *out = *open;
        return RTC_OK;
    }
    // every field but view_inv (and the padding); the doubles bit for bit
    if (open->hsize != close->hsize || open->vsize != close->vsize || open->samples != close->samples ||
        std::memcmp(&open->fov, &close->fov, sizeof(double)) != 0 || std::memcmp(&open->half_width, &close->half_width, sizeof(double)) != 0 ||
        std::memcmp(&open->half_height, &close->half_height, sizeof(double)) != 0 ||
        std::memcmp(&open->pixel_size, &close->pixel_size, sizeof(double)) != 0)
        return RTC_ERR_ARG;
    const double t = rtc_shutter_time(samples, k);
    rtc_camera c = *open;
    shutter_lerp(open->view_inv, close->view_inv, t, c.view_inv);
    *out = c;
    return RTC_OK;
}

// Color::average_over (color.rs:128-139) of whole frames: sums from 0.0 in frame order, one division each.
rtc_status rtc_canvas_average(const double *frames, uint32_t n, size_t count, double *out) {
    if (!frames || !out || n == 0u || n > RTC_MAX_SHUTTER_SAMPLES) return RTC_ERR_ARG;
    const double d = static_cast<double>(n);
    const uint64_t nan_bits = 0x7FF8000000000000ull;
    double kQuietNaN;
    std::memcpy(&kQuietNaN, &nan_bits, sizeof kQuietNaN);
    for (size_t i = 0; i < count; ++i) {
        double s = 0.0;
        for (uint32_t f = 0; f < n; ++f) s = s + frames[(size_t)f * count + i];
        const double m = s / d;
        out[i] = (m != m) ? kQuietNaN : m; // one NaN for every platform (include/rtc.h)
    }
    return RTC_OK;
}

void rtc_free(void *p) { std::free(p); }

} // extern "C"
