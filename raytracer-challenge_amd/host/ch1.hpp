// ch1.hpp — host-side C++ mirror of the reference crate's public surface for the hot path
// (ch1/src/lib.rs:4-11: vec, color, canvas, transform, shape, material, camera), over the C-ABI of
// include/rtc.h. Same type and method names, same argument meaning, same error behaviour (what
// panics in Rust throws ch1::Panic here), so that code written against the Rust API —
//
//     let mut world = World::new(Default::default());
//     world.add_shape(Box::new(Sphere::new_with_transform_and_material(
//         Matrix::identity().scaling(0.5, 0.5, 0.5).translation(1., 0.7, -3.5), material)));
//     let camera = Camera::new_with_transform(800, 600, PI / 2.0,
//         Matrix::make_view_transform(from, to, up));
//     let canvas = camera.render(&world);          // <- runs on the MI355X
//     canvas.write_to_file_simple("out.ppm");
//
// — ports line by line. A Rust maintainer would bind the same C symbols with an `extern "C"`
// block instead; Rust is not available in this build environment, so the
// host side above the C-ABI is C++ (the reference is compiled code).
#ifndef CH1_HPP
#define CH1_HPP

#include <array>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <cctype>
#include <exception>
#include <type_traits>
#include <stdexcept>
#include <string>
#include <utility>
#include <cstring>
#include <vector>

#include "rtc.h"

namespace ch1 {

struct Panic : std::runtime_error { // the reference panics (unwrap/expect/panic!) on these paths
    rtc_status status;
    Panic(rtc_status s, const std::string &where) : std::runtime_error(where + ": " + rtc_strerror(s)), status(s) {}
};
inline void check(rtc_status s, const char *where) {
    if (s != RTC_OK) throw Panic(s, where);
}

struct Vector { double x, y, z; static Vector new_(double x, double y, double z) { return {x, y, z}; } }; // vec.rs:7-23
struct Point { double x, y, z; static Point new_(double x, double y, double z) { return {x, y, z}; } };   // vec.rs:145-160
struct Color {                                                                                             // color.rs:5-24
    double red, green, blue;
    static Color new_(double r, double g, double b) { return {r, g, b}; }
    static Color BLACK() { return {0., 0., 0.}; }
    static Color WHITE() { return {1., 1., 1.}; }
    static Color RED() { return {1., 0., 0.}; }
    static Color GREEN() { return {0., 1., 0.}; }
    static Color BLUE() { return {0., 0., 1.}; }
};

class Matrix { // transform.rs:23-218
  public:
    std::array<double, 16> m;
    static Matrix identity() { Matrix r; rtc_matrix_identity(r.m.data()); return r; }
    Matrix multiply(const Matrix &o) const { Matrix r; rtc_matrix_multiply(m.data(), o.m.data(), r.m.data()); return r; }
    Matrix translation(double x, double y, double z) const { Matrix r; rtc_matrix_translation(m.data(), x, y, z, r.m.data()); return r; }
    Matrix scaling(double x, double y, double z) const { Matrix r; rtc_matrix_scaling(m.data(), x, y, z, r.m.data()); return r; }
    Matrix rotation_x(double a) const { Matrix r; rtc_matrix_rotation_x(m.data(), a, r.m.data()); return r; }
    Matrix rotation_y(double a) const { Matrix r; rtc_matrix_rotation_y(m.data(), a, r.m.data()); return r; }
    Matrix rotation_z(double a) const { Matrix r; rtc_matrix_rotation_z(m.data(), a, r.m.data()); return r; }
    Matrix shearing(double xy, double xz, double yx, double yz, double zx, double zy) const {
        Matrix r; rtc_matrix_shearing(m.data(), xy, xz, yx, yz, zx, zy, r.m.data()); return r;
    }
    bool is_invertable() const { double t[16]; return rtc_matrix_inverse(m.data(), t) == RTC_OK; }
    Matrix inverse() const { Matrix r; check(rtc_matrix_inverse(m.data(), r.m.data()), "Matrix::inverse"); return r; } // panics transform.rs:177
    Matrix transpose() const { Matrix r; rtc_matrix_transpose(m.data(), r.m.data()); return r; }
    static Matrix make_view_transform(Point from, Point to, Vector up) {
        const double f[3] = {from.x, from.y, from.z}, t[3] = {to.x, to.y, to.z}, u[3] = {up.x, up.y, up.z};
        Matrix r; rtc_view_transform(f, t, u, r.m.data()); return r;
    }
};

struct Light { // material.rs:10-31
    Color intensity; Point position;
    static Light new_(Color i, Point p) { return {i, p}; }
    static Light default_() { return {Color::WHITE(), Point::new_(-10., 10., -10.)}; }
};

// The six Pattern implementations (material.rs:48-242) as one value type.
struct Pattern {
    uint32_t kind = RTC_PATTERN_NONE;
    Color a{0, 0, 0}, b{0, 0, 0};
    Matrix xf = Matrix::identity();
    void set_transform(const Matrix &t) { xf = t; }
};
inline Pattern TestPattern() { Pattern p; p.kind = RTC_PATTERN_TEST; return p; }
inline Pattern StripePattern(Color a, Color b) { Pattern p; p.kind = RTC_PATTERN_STRIPE; p.a = a; p.b = b; return p; }
inline Pattern GradientPattern(Color a, Color b) { Pattern p; p.kind = RTC_PATTERN_GRADIENT; p.a = a; p.b = b; return p; }
inline Pattern RingPattern(Color a, Color b) { Pattern p; p.kind = RTC_PATTERN_RING; p.a = a; p.b = b; return p; }
inline Pattern CheckerPattern(Color a, Color b) { Pattern p; p.kind = RTC_PATTERN_CHECKER; p.a = a; p.b = b; return p; }
inline Pattern GridPattern(Color base, Color grid) { Pattern p; p.kind = RTC_PATTERN_GRID; p.a = base; p.b = grid; return p; }

struct Material { // material.rs:244-369
    bool has_pattern = false; Pattern pattern;
    bool has_color = true; Color color = Color::RED();
    double ambient = 0.1, diffuse = 0.9, specular = 0.9, shininess = 200.0, reflectiveness = 0.0, transparency = 0.0,
           refractive_index = 1.0;
    static Material DEFAULT() { return Material{}; }                                             // :273-283 (RED)
    static Material default_() { Material m; m.color = Color::WHITE(); return m; }               // :364-369 (WHITE)
    static Material solid_with_defaults(Color c) { Material m; m.color = c; return m; }          // :295-297
    static Material pattern_with_defaults(const Pattern &p) { Material m; m.set_pattern(p); return m; } // :299-301
    Material &set_pattern(const Pattern &p) { pattern = p; has_pattern = true; return *this; }   // :303-306

    rtc_material flatten() const {
        rtc_material o;
        rtc_material_default(&o);
        o.has_color = has_color ? 1u : 0u;
        o.color[0] = color.red; o.color[1] = color.green; o.color[2] = color.blue;
        o.ambient = ambient; o.diffuse = diffuse; o.specular = specular; o.shininess = shininess;
        o.reflective = reflectiveness; o.transparency = transparency; o.refractive_index = refractive_index;
        if (has_pattern) {
            const double a[3] = {pattern.a.red, pattern.a.green, pattern.a.blue}, b[3] = {pattern.b.red, pattern.b.green, pattern.b.blue};
            check(rtc_material_set_pattern(&o, pattern.kind, a, b, pattern.xf.m.data()), "Pattern::set_transform");
        }
        return o;
    }
};

// Shapes (shape.rs:281-630). Constructors invert the transform exactly like the reference.
struct Shape {
    rtc_shape flat;
    Material material;
    Matrix transform = Matrix::identity(); // the object transform `flat.inv` was made from (World::set_shape_motion starts there)
    static Shape make(uint32_t kind, const Matrix &m, const Material &mat) {
        Shape s; s.material = mat; s.transform = m;
        const rtc_material fm = mat.flatten();
        check(rtc_shape_init(kind, m.m.data(), &fm, &s.flat), "Shape::new_with_transform_and_material");
        return s;
    }
    Material &get_material_mut() { return material; }
    const Material &get_material() const { return material; }
    // Sphere::set_transform (shape.rs:319-322). Plane's and Cube's transpose their OLD transpose instead of the new inverse
    // (shape.rs:446-449, 535-538): kept.
    void set_transform(const Matrix &m) {
        check(rtc_matrix_inverse(m.m.data(), flat.inv), "Shape::set_transform");
        transform = m;
        double t[16];
        rtc_matrix_transpose(flat.kind == RTC_SPHERE ? flat.inv : flat.inv_t, t);
        std::memcpy(flat.inv_t, t, sizeof t);
    }
};
struct Sphere {
    static Shape new_() { return Shape::make(RTC_SPHERE, Matrix::identity(), Material::default_()); }
    static Shape new_with_transform(const Matrix &m) { return Shape::make(RTC_SPHERE, m, Material::default_()); }
    static Shape new_with_transform_and_material(const Matrix &m, const Material &mat) { return Shape::make(RTC_SPHERE, m, mat); }
    static Shape glass_sphere() { Material m = Material::default_(); m.transparency = 1.0; m.refractive_index = 1.5; return Shape::make(RTC_SPHERE, Matrix::identity(), m); }
};
struct Plane {
    static Shape new_() { return Shape::make(RTC_PLANE, Matrix::identity(), Material::default_()); }
    static Shape new_with_transform(const Matrix &m) { return Shape::make(RTC_PLANE, m, Material::default_()); }
    static Shape new_with_transform_and_material(const Matrix &m, const Material &mat) { return Shape::make(RTC_PLANE, m, mat); }
};
struct Cube {
    static Shape new_() { return Shape::make(RTC_CUBE, Matrix::identity(), Material::default_()); }
    static Shape new_with_transform(const Matrix &m) { return Shape::make(RTC_CUBE, m, Material::default_()); }
    static Shape new_with_transform_and_material(const Matrix &m, const Material &mat) { return Shape::make(RTC_CUBE, m, mat); }
};

class Canvas { // canvas.rs:16-109
  public:
    uint32_t width, height;
    std::vector<double> pixels; // [y][x][rgb], idx = y*width + x (canvas.rs:44)
    // A Canvas returned by Camera::render_rgb8 / render_async_rgb8 holds ONLY what the reference's file writers read from a
    // Canvas — Color::scale(c, 255) of every component (canvas.rs:98-104, color.rs:100-114), evaluated on the device: 3 bytes
    // per pixel crossed PCIe instead of 24 and `pixels` is empty. write_to_file_simple writes the same file either way.
    // Blind spot: those bytes are gamma 1's, so write_to_file of such a Canvas ignores `gamma` — a caller that sets a gamma
    // renders with Camera::render_rgba8 instead.
    std::vector<uint8_t> rgb8;
    // A Canvas returned by Camera::render_rgba8 / render_async_rgba8 holds to_imgbuf's RGBA (canvas.rs:61-79) at the gamma
    // it was rendered with (`rgba8_gamma`, also set as `gamma`), quantised on the device: 4 bytes per pixel crossed PCIe,
    // `pixels` and `rgb8` are empty. write_to_file writes it as it is and throws if `gamma` was changed after the render.
    std::vector<uint8_t> rgba8;
    float rgba8_gamma = 1.0f;
    Canvas(uint32_t w, uint32_t h) : width(w), height(h), pixels(static_cast<size_t>(w) * h * 3, 0.0) {} // BLACK canvas.rs:37-41
    static Canvas quantised(uint32_t w, uint32_t h) { Canvas c(0, 0); c.width = w; c.height = h; c.rgb8.assign(static_cast<size_t>(w) * h * 3, 0); return c; }
    static Canvas imgbuf(uint32_t w, uint32_t h, float g) {
        Canvas c(0, 0);
        c.width = w; c.height = h;
        c.rgba8.assign(static_cast<size_t>(w) * h * 4, 0);
        c.gamma = c.rgba8_gamma = g;
        return c;
    }
    bool is_quantised() const { return pixels.empty() && !rgb8.empty(); }
    bool is_imgbuf() const { return pixels.empty() && !rgba8.empty(); }
    void write_pixel(uint32_t x, uint32_t y, Color c) { double *p = at(x, y); p[0] = c.red; p[1] = c.green; p[2] = c.blue; }
    Color get_pixel(uint32_t x, uint32_t y) const { const double *p = const_cast<Canvas *>(this)->at(x, y); return {p[0], p[1], p[2]}; }
    // Ambient occlusion composited in place (rtc_canvas_apply_ao, include/rtc.h): every component of pixel i times
    // 1 - strength * ao[i] / n_samples. `ao` is Camera::render_ao's `shadow` plane and n_samples its n_lights. f64 canvases only.
    void apply_ao(const std::vector<uint16_t> &ao, uint32_t n_samples, double strength = 1.0) {
        if (pixels.size() != static_cast<size_t>(width) * height * 3 || ao.size() != static_cast<size_t>(width) * height)
            throw Panic(RTC_ERR_ARG, "Canvas::apply_ao: an f64 Canvas and a plane of its size are needed");
        check(rtc_canvas_apply_ao(pixels.data(), ao.data(), n_samples, strength, width, height), "Canvas::apply_ao");
    }
    // An occlusion FRACTION composited in place (rtc_canvas_apply_occlusion, include/rtc.h): every component of pixel i times
    // 1 - strength * occ[i]; apply_ao's bytes when occ is Aov::occlusion, and what takes a filtered plane. f64 canvases only.
    void apply_occlusion(const std::vector<double> &occ, double strength = 1.0) {
        if (pixels.size() != static_cast<size_t>(width) * height * 3 || occ.size() != static_cast<size_t>(width) * height)
            throw Panic(RTC_ERR_ARG, "Canvas::apply_occlusion: an f64 Canvas and a plane of its size are needed");
        check(rtc_canvas_apply_occlusion(pixels.data(), occ.data(), strength, width, height), "Canvas::apply_occlusion");
    }
    // A plane added in place (rtc_canvas_add_scaled, include/rtc.h): every component c becomes c + strength * plane's. `plane`
    // is three doubles per pixel, Camera::render_gather's `bounce` for one. f64 canvases only.
    void add_scaled(const std::vector<double> &plane, double strength = 1.0) {
        if (pixels.size() != static_cast<size_t>(width) * height * 3 || plane.size() != pixels.size())
            throw Panic(RTC_ERR_ARG, "Canvas::add_scaled: an f64 Canvas and a plane of its size are needed");
        check(rtc_canvas_add_scaled(pixels.data(), plane.data(), strength, width, height), "Canvas::add_scaled");
    }
    // The glare of highlights added in place (rtc_canvas_bloom, include/rtc.h): luminance above spec.threshold, blurred by a
    // separable Gaussian, times spec.strength. f64 canvases only. Not part of the reference's Canvas.
    void bloom(const rtc_bloom &spec) {
        if (pixels.size() != static_cast<size_t>(width) * height * 3) throw Panic(RTC_ERR_ARG, "Canvas::bloom: an f64 Canvas is needed");
        check(rtc_canvas_bloom(pixels.data(), width, height, &spec, pixels.data()), "Canvas::bloom");
    }
    // Exposure and a tone curve in place (rtc_canvas_tonemap): what comes before to_rgba8 or a file writer when the frame is
    // brighter than 1.0. With an AUTO flag in `spec` the Canvas takes its own statistics first (rtc_canvas_luminance).
    void tonemap(const rtc_tonemap &spec) {
        if (pixels.size() != static_cast<size_t>(width) * height * 3) throw Panic(RTC_ERR_ARG, "Canvas::tonemap: an f64 Canvas is needed");
        rtc_luminance stats{};
        if (spec.flags != 0u) check(rtc_canvas_luminance(pixels.data(), width, height, &stats), "Canvas::tonemap");
        check(rtc_canvas_tonemap(pixels.data(), width, height, &spec, spec.flags != 0u ? &stats : nullptr, pixels.data()), "Canvas::tonemap");
    }
    rtc_luminance luminance() const { // the frame statistics (rtc_canvas_luminance)
        if (pixels.size() != static_cast<size_t>(width) * height * 3) throw Panic(RTC_ERR_ARG, "Canvas::luminance: an f64 Canvas is needed");
        rtc_luminance stats{};
        check(rtc_canvas_luminance(pixels.data(), width, height, &stats), "Canvas::luminance");
        return stats;
    }
    // A copy of this Canvas filtered to w x h (rtc_canvas_resize, include/rtc.h): the horizontal pass first, an axis whose size
    // does not change copied. What turns a frame traced at 2x or 3x into an anti-aliased one, and a small plane into one that
    // can be composited over a full-size frame. f64 canvases only. Not part of the reference's Canvas.
    Canvas resized(uint32_t w, uint32_t h, const rtc_resize &spec) const {
        if (pixels.empty() || pixels.size() != static_cast<size_t>(width) * height * 3) throw Panic(RTC_ERR_ARG, "Canvas::resized: an f64 Canvas is needed");
        Canvas out(w, h);
        out.gamma = gamma;
        check(rtc_canvas_resize(pixels.data(), width, height, &spec, out.pixels.data(), w, h), "Canvas::resized");
        return out;
    }
    void write_to_file_simple(const std::string &file_name) const { // canvas.rs:86-109
        if (is_imgbuf()) { // the PPM is Color::scale's (gamma 1): only an RGBA frame of gamma 1 holds those bytes
            if (rgba8_gamma != 1.0f) throw Panic(RTC_ERR_ARG, "Canvas::write_to_file_simple: the Canvas holds RGBA at gamma != 1 (Camera::render_rgba8)");
            std::vector<uint8_t> rgb(static_cast<size_t>(width) * height * 3);
            for (size_t i = 0; i < static_cast<size_t>(width) * height; ++i)
                for (int k = 0; k < 3; ++k) rgb[i * 3 + k] = rgba8[i * 4 + k];
            check(rtc_canvas_write_ppm_rgb8(file_name.c_str(), rgb.data(), width, height), "Canvas::write_to_file_simple");
            return;
        }
        if (is_quantised()) check(rtc_canvas_write_ppm_rgb8(file_name.c_str(), rgb8.data(), width, height), "Canvas::write_to_file_simple");
        else check(rtc_canvas_write_ppm(file_name.c_str(), pixels.data(), width, height), "Canvas::write_to_file_simple");
    }
    // Canvas::write_to_file (canvas.rs:80-84): to_imgbuf().save(path), the codec chosen by the extension. PNG is written
    // (lossless: the same pixels after decoding as the reference's file); the `image` crate's other codecs are not rebuilt.
    void write_to_file(const std::string &file_name) const {
        const size_t dot = file_name.find_last_of('.');
        std::string ext = dot == std::string::npos ? std::string() : file_name.substr(dot + 1);
        for (char &c : ext) c = static_cast<char>(std::tolower(static_cast<unsigned char>(c)));
        if (ext != "png") throw Panic(RTC_ERR_ARG, "Canvas::write_to_file(" + file_name + "): only .png is written here (write_to_file_simple: PPM)");
        if (is_imgbuf()) {
            if (gamma != rgba8_gamma)
                throw Panic(RTC_ERR_ARG, "Canvas::write_to_file(" + file_name + "): gamma was changed after Camera::render_rgba8 made this frame");
            check(rtc_canvas_write_png8(file_name.c_str(), rgba8.data(), width, height, 4), "Canvas::write_to_file");
            return;
        }
        if (is_quantised()) { check(rtc_canvas_write_png8(file_name.c_str(), rgb8.data(), width, height, 3), "Canvas::write_to_file"); return; }
        std::vector<uint8_t> rgba(static_cast<size_t>(width) * height * 4);
        rtc_canvas_to_rgba8(pixels.data(), width, height, gamma, rgba.data());
        check(rtc_canvas_write_png8(file_name.c_str(), rgba.data(), width, height, 4), "Canvas::write_to_file");
    }
    // Canvas::write_to_file for a ".jpg" / ".jpeg" name, as its own call (write_to_file itself keeps panicking on them):
    // the same frame and gamma rules as write_to_file, encoded by the host JPEG writer (rtc_canvas_write_jpeg, include/rtc.h)
    // at `quality` — the reference's `save` uses 75. The name's extension is not looked at.
    void write_to_file_jpeg(const std::string &file_name, int32_t quality = 75) const {
        const char *where = "Canvas::write_to_file_jpeg";
        if (is_imgbuf()) {
            if (gamma != rgba8_gamma)
                throw Panic(RTC_ERR_ARG, "Canvas::write_to_file_jpeg(" + file_name + "): gamma was changed after Camera::render_rgba8 made this frame");
            check(rtc_canvas_write_jpeg(file_name.c_str(), rgba8.data(), width, height, 4, quality), where);
            return;
        }
        if (is_quantised()) { check(rtc_canvas_write_jpeg(file_name.c_str(), rgb8.data(), width, height, 3, quality), where); return; }
        std::vector<uint8_t> rgba(static_cast<size_t>(width) * height * 4);
        rtc_canvas_to_rgba8(pixels.data(), width, height, gamma, rgba.data());
        check(rtc_canvas_write_jpeg(file_name.c_str(), rgba.data(), width, height, 4, quality), where);
    }
    // Canvas::write_to_file with every codec of the save table (include/rtc.h, rtc_canvas_save): png, jpg / jpeg (quality
    // 75), gif, ppm, bmp, tga, tif / tiff, ico, ff, pam by the name's last extension, any case; anything else panics with
    // RTC_ERR_UNSUPPORTED and writes nothing. The same frame and gamma rules as write_to_file. An f64 Canvas under a name
    // of the float table (hdr, pfm, exr; rtc_canvas_save_f64) is saved as data: the pixels themselves, unclipped and
    // without gamma (EXR as HALF). A quantised Canvas has no such numbers left and goes through the 8-bit table.
    void save(const std::string &file_name) const {
        const char *where = "Canvas::save";
        uint32_t float_format = 0;
        if (!is_imgbuf() && !is_quantised() && rtc_float_format_for_name(file_name.c_str(), &float_format) == RTC_OK) {
            check(rtc_canvas_save_f64(file_name.c_str(), pixels.data(), width, height), where);
            return;
        }
        if (is_imgbuf()) {
            if (gamma != rgba8_gamma)
                throw Panic(RTC_ERR_ARG, "Canvas::save(" + file_name + "): gamma was changed after Camera::render_rgba8 made this frame");
            check(rtc_canvas_save(file_name.c_str(), rgba8.data(), width, height, 4), where);
            return;
        }
        if (is_quantised()) { check(rtc_canvas_save(file_name.c_str(), rgb8.data(), width, height, 3), where); return; }
        std::vector<uint8_t> rgba(static_cast<size_t>(width) * height * 4);
        rtc_canvas_to_rgba8(pixels.data(), width, height, gamma, rgba.data());
        check(rtc_canvas_save(file_name.c_str(), rgba.data(), width, height, 4), where);
    }
    float gamma = 1.0f; // canvas.rs:30
  private:
    double *at(uint32_t x, uint32_t y) {
        if (is_quantised() || is_imgbuf()) throw std::logic_error("Canvas holds the 8-bit frame only (Camera::render_rgb8 / render_rgba8): render() for f64 pixels");
        if (x >= width || y >= height) throw std::out_of_range("Canvas index out of bounds");
        return pixels.data() + (static_cast<size_t>(y) * width + x) * 3;
    }
};

// Process-wide device context (the Rust API has no explicit device handle).
class Device {
  public:
    static rtc_context *get() {
        static Device d;
        return d.ctx_;
    }
  private:
    Device() { check(rtc_context_create(0, nullptr, &ctx_), "rtc_context_create (MI355X required; no CPU fallback)"); }
    ~Device() { rtc_context_destroy(ctx_); }
    rtc_context *ctx_ = nullptr;
};

class World { // shape.rs:633-795
  public:
    explicit World(Light l) : light(l) {}
    static World new_(Light l) { return World(l); }
    static World default_() { // impl Default for World shape.rs:784-795
        World w(Light::default_());
        Material m = Material::solid_with_defaults(Color::new_(0.8, 1.0, 0.6));
        m.diffuse = 0.7; m.specular = 0.2;
        w.add_shape(Sphere::new_with_transform_and_material(Matrix::identity(), m));
        w.add_shape(Sphere::new_with_transform(Matrix::identity().scaling(0.5, 0.5, 0.5)));
        return w;
    }
    World &add_shape(Shape s) { // shape.rs:661-667
        s.flat.world_id = ++last_world_id;
        shapes.push_back(std::move(s));
        return *this;
    }
    // Further lights (the reference's World holds a list and shades with the first, shape.rs:636,686; here every light
    // contributes: rtc_world_create_lights). `light` stays the first; at most RTC_MAX_LIGHTS in all.
    World &add_light(Light l) {
        if (more_lights.size() + 2 > RTC_MAX_LIGHTS) check(RTC_ERR_ARG, "World::add_light");
        more_lights.push_back(l);
        return *this;
    }
    // The book's area light (rtc_area_light, include/rtc.h): the rectangle corner + s*uvec + t*vvec, sampled at the centres
    // of usteps x vsteps cells, each sample a point light of intensity / (usteps*vsteps). Area lights follow the point
    // lights in the World's sample list; at most RTC_MAX_LIGHT_SAMPLES samples in all (checked when the World is rendered).
    // The World keeps its point `light` (the reference's World::new takes one), so it is sample 0 and an area light always
    // shines beside it — give it Color::BLACK() for a World lit by area lights alone (its shadow rays are still cast).
    // lights() lists the point lights only; the area lights are `area_lights`.
    World &add_area_light(Point corner, Vector uvec, Vector vvec, uint32_t usteps, uint32_t vsteps, Color intensity) {
        if (usteps == 0 || vsteps == 0) check(RTC_ERR_ARG, "World::add_area_light");
        rtc_area_light a{};
        a.intensity[0] = intensity.red; a.intensity[1] = intensity.green; a.intensity[2] = intensity.blue;
        a.corner[0] = corner.x; a.corner[1] = corner.y; a.corner[2] = corner.z;
        a.uvec[0] = uvec.x; a.uvec[1] = uvec.y; a.uvec[2] = uvec.z;
        a.vvec[0] = vvec.x; a.vvec[1] = vvec.y; a.vvec[2] = vvec.z;
        a.usteps = usteps; a.vsteps = vsteps;
        area_lights.push_back(a);
        return *this;
    }
    std::vector<Light> lights() const {
        std::vector<Light> all{light};
        all.insert(all.end(), more_lights.begin(), more_lights.end());
        return all;
    }
    // Motion blur (rtc_motion, include/rtc.h): shape i moves from its own transform, when the shutter opens, to
    // `transform_at_close`, when it closes; a Camera with set_shutter renders the World averaged over that move, any other
    // Camera renders it as the shutter opens. Setting it again replaces the move; clear_shape_motions stops every shape.
    World &set_shape_motion(size_t i, const Matrix &transform_at_close) {
        if (i >= shapes.size()) check(RTC_ERR_ARG, "World::set_shape_motion");
        for (auto &mv : motions)
            if (mv.first == i) { mv.second = transform_at_close; return *this; }
        motions.emplace_back(i, transform_at_close);
        return *this;
    }
    void clear_shape_motions() { motions.clear(); }
    Shape &get_shape_mut(size_t i) { dirty_ = true; return shapes.at(i); }
    const Shape &get_shape(size_t i) const { return shapes.at(i); }

    // World::color_at(ray, remaining) shape.rs:702-710 — on the GPU
    Color color_at(Point origin, Vector direction, uint8_t remaining) const {
        const double ray[6] = {origin.x, origin.y, origin.z, direction.x, direction.y, direction.z};
        double rgb[3];
        Uploaded up(*this);
        check(rtc_color_at(Device::get(), up.w, ray, 1, remaining, 0, rgb, nullptr), "World::color_at");
        return {rgb[0], rgb[1], rgb[2]};
    }

    Light light;
    std::vector<Light> more_lights; // lights()[1..]
    std::vector<rtc_area_light> area_lights; // add_area_light: behind the point lights
    std::vector<Shape> shapes;
    std::vector<std::pair<size_t, Matrix>> motions; // set_shape_motion: (shape, its transform as the shutter closes)
    uint32_t last_world_id = 0;

    // The flattened World resident in HBM. Camera::render(&World) takes the World by reference on every call
    // (camera.rs:116,144); an animation loop calls it with the same World and a moving camera (lua.rs:34-41), so the
    // upload is cached process-wide: re-flatten (materials may have been edited via get_material_mut), compare with what
    // is resident, upload only when something changed.
    struct Uploaded {
        rtc_world *w = nullptr;
        explicit Uploaded(const World &world) {
            std::vector<rtc_shape> flat;
            flat.reserve(world.shapes.size());
            for (const Shape &s : world.shapes) {
                rtc_shape f = s.flat;
                f.material = s.material.flatten();
                flat.push_back(f);
            }
            std::vector<rtc_light> ls;
            for (const Light &wl : world.lights()) {
                rtc_light l;
                l.intensity[0] = wl.intensity.red; l.intensity[1] = wl.intensity.green; l.intensity[2] = wl.intensity.blue;
                l.position[0] = wl.position.x; l.position[1] = wl.position.y; l.position[2] = wl.position.z;
                ls.push_back(l);
            }
            w = Resident::instance().get(std::move(flat), ls, world.area_lights);
        }
        Uploaded(const Uploaded &) = delete;
        Uploaded &operator=(const Uploaded &) = delete;
    };
    class Resident { // the one World kept on the device between calls
      public:
        static Resident &instance() {
            static Resident r;
            return r;
        }
        rtc_world *get(std::vector<rtc_shape> &&flat, const rtc_light &l) { return get(std::move(flat), std::vector<rtc_light>{l}); }
        // `area`: the World's area lights, behind its point lights `ls` (none: the rtc_world_*_lights entries, as ever)
        rtc_world *get(std::vector<rtc_shape> &&flat, const std::vector<rtc_light> &ls, const std::vector<rtc_area_light> &area = {}) {
            const uint32_t nl = static_cast<uint32_t>(ls.size());
            std::vector<rtc_area_light> all; // every light as an area light, when the World has one
            if (!area.empty()) {
                all.resize(ls.size());
                for (size_t i = 0; i < ls.size(); ++i) check(rtc_area_light_from_point(&ls[i], &all[i]), "World lights");
                all.insert(all.end(), area.begin(), area.end());
            }
            const uint32_t na = static_cast<uint32_t>(all.size());
            const bool same = w_ != nullptr && flat.size() == flat_.size() && ls.size() == lights_.size() &&
                              std::memcmp(ls.data(), lights_.data(), ls.size() * sizeof(rtc_light)) == 0 && area.size() == area_.size() &&
                              (area.empty() || std::memcmp(area.data(), area_.data(), area.size() * sizeof(rtc_area_light)) == 0) &&
                              (flat.empty() || std::memcmp(flat.data(), flat_.data(), flat.size() * sizeof(rtc_shape)) == 0);
            if (!same) {
                // other contents for the World that is resident already (rtc_world_update: no destroy, no allocation while
                // it does not grow); a rejected update leaves it as it was, and so does this cache
                if (w_) {
                    const rtc_status st = na ? rtc_world_update_area_lights(Device::get(), w_, flat.data(), static_cast<uint32_t>(flat.size()), all.data(), na)
                                             : rtc_world_update_lights(Device::get(), w_, flat.data(), static_cast<uint32_t>(flat.size()), ls.data(), nl);
                    if (st == RTC_ERR_NOMEM || st == RTC_ERR_DEVICE) flat_.clear(), lights_.clear(), area_.clear(); // a failed growing update: nothing is resident
                    check(st, "World update");
                } else if (na) check(rtc_world_create_area_lights(Device::get(), flat.data(), static_cast<uint32_t>(flat.size()), all.data(), na, &w_), "World upload");
                else check(rtc_world_create_lights(Device::get(), flat.data(), static_cast<uint32_t>(flat.size()), ls.data(), nl, &w_), "World upload");
                flat_ = std::move(flat);
                lights_ = ls;
                area_ = area;
            }
            return w_;
        }
        rtc_world *resident() const { return w_; } // (tests: the handle stays the same across updates)
      private:
        Resident() { (void)Device::get(); } // the context outlives this cache (constructed first, destroyed last)
        ~Resident() { if (w_) rtc_world_destroy(w_); }
        rtc_world *w_ = nullptr;
        std::vector<rtc_shape> flat_;
        std::vector<rtc_light> lights_;
        std::vector<rtc_area_light> area_;
    };
  private:
    bool dirty_ = false;
};

// What each pixel's centre ray saw (rtc_render_aov, include/rtc.h): the planes of Camera::render_aov, row-major, idx =
// y*width + x. Not part of the reference: its renderer keeps the hit record to itself.
struct Aov {
    uint32_t width = 0, height = 0;
    uint32_t n_lights = 1;            // light samples of the World it was rendered from: the largest `shadow` count
    std::vector<int32_t> index;       // World.shapes position of the hit, -1 for a miss
    std::vector<double> depth;        // t, +infinity for a miss
    std::vector<double> point;        // [3] per pixel
    std::vector<double> normal;       // [3] per pixel, after the `inside` flip
    std::vector<uint8_t> flags;       // 1 = hit, | 2 = inside
    std::vector<uint16_t> shadow;     // light samples hidden from the hit's over_point
    enum View : uint32_t { DEPTH = RTC_AOV_VIEW_DEPTH, NORMAL = RTC_AOV_VIEW_NORMAL, INDEX = RTC_AOV_VIEW_INDEX, SHADOW = RTC_AOV_VIEW_SHADOW };
    bool hit(uint32_t x, uint32_t y) const { return (flags[static_cast<size_t>(y) * width + x] & 1u) != 0; }
    bool inside(uint32_t x, uint32_t y) const { return (flags[static_cast<size_t>(y) * width + x] & 2u) != 0; }
    rtc_aov_buffers buffers() {
        return rtc_aov_buffers{index.data(), depth.data(), point.data(), normal.data(), flags.data(), shadow.data()};
    }
    // A plane as a quantised Canvas (rtc_aov_view_rgb8) that every file writer takes; near / far are read by DEPTH only.
    Canvas view(View v, double near = 0.0, double far = 1.0) const {
        Canvas c = Canvas::quantised(width, height);
        const rtc_aov_buffers b = const_cast<Aov *>(this)->buffers();
        check(rtc_aov_view_rgb8(v, &b, width, height, near, far, n_lights, c.rgb8.data()), "Aov::view");
        return c;
    }
    // The `shadow` plane as the fraction count / n_lights (rtc_counts_to_fraction): what filter and Canvas::apply_occlusion take.
    std::vector<double> occlusion() const {
        if (shadow.size() != static_cast<size_t>(width) * height) throw Panic(RTC_ERR_ARG, "Aov::occlusion: the Aov has no shadow plane");
        std::vector<double> out(shadow.size());
        check(rtc_counts_to_fraction(shadow.data(), n_lights, width, height, out.data()), "Aov::occlusion");
        return out;
    }
    // A plane of `channels` (1 or 3) doubles per pixel — an occlusion fraction, a Gather's radiance or bounce — smoothed under
    // this Aov's index, point and normal planes by the edge-aware filter (rtc_plane_filter, include/rtc.h).
    std::vector<double> filter(const std::vector<double> &plane, uint32_t channels, const rtc_filter &spec) const {
        const size_t px = static_cast<size_t>(width) * height;
        if (index.size() != px || point.size() != 3 * px || normal.size() != 3 * px || plane.size() != px * channels)
            throw Panic(RTC_ERR_ARG, "Aov::filter: the index, point and normal planes and a plane of their size are needed");
        std::vector<double> out(plane.size());
        const rtc_aov_buffers b = const_cast<Aov *>(this)->buffers();
        check(rtc_plane_filter(plane.data(), channels, &b, width, height, &spec, out.data()), "Aov::filter");
        return out;
    }
    // rtc.h's default filter: RTC_FILTER_DEFAULT_*, taps of the same object only
    static rtc_filter default_filter() {
        return rtc_filter{RTC_FILTER_DEFAULT_PLANE_SIGMA, RTC_FILTER_DEFAULT_PASSES, RTC_FILTER_DEFAULT_NORMAL_SQUARINGS, RTC_FILTER_SAME_OBJECT, 0u};
    }
    // The planes as data: one multi-channel OpenEXR file (rtc_float_format, include/rtc.h) — Z, N.*, P.*, id, shadow and,
    // with an f64 `colour` Canvas of the same size, its R, G, B as HALF (FLOAT with `colour_as_float`).
    void save_exr(const std::string &file_name, const Canvas *colour = nullptr, bool colour_as_float = false) const {
        const char *where = "Aov::save_exr";
        if (colour && (colour->width != width || colour->height != height || colour->pixels.size() != static_cast<size_t>(width) * height * 3))
            throw Panic(RTC_ERR_ARG, std::string(where) + "(" + file_name + "): the colour Canvas must be an f64 Canvas of the planes' size");
        rtc_float_planes p{colour ? colour->pixels.data() : nullptr, const_cast<Aov *>(this)->buffers(), colour_as_float ? RTC_EXR_FLOAT : RTC_EXR_HALF, 0u};
        std::vector<uint8_t> file(rtc_float_format(RTC_FLOAT_EXR, &p, width, height, nullptr, 0));
        if (file.empty()) check(RTC_ERR_ARG, where);
        rtc_float_format(RTC_FLOAT_EXR, &p, width, height, file.data(), file.size());
        std::FILE *f = std::fopen(file_name.c_str(), "wb");
        if (!f) check(RTC_ERR_IO, where);
        const bool ok = std::fwrite(file.data(), 1, file.size(), f) == file.size();
        if (std::fclose(f) != 0 || !ok) check(RTC_ERR_IO, where);
    }
};

// One bounce of indirect light per pixel (rtc_render_gather, include/rtc.h "colour bleeding"): the planes of
// Camera::render_gather, row-major, three doubles per pixel. Not part of the reference.
struct Gather {
    uint32_t width = 0, height = 0;
    std::vector<double> radiance;     // the mean colour the fan sees from the centre ray's hit, within its radius
    std::vector<double> bounce;       // radiance times the hit's base colour and diffuse coefficient: Canvas::add_scaled takes it
};

class Camera { // camera.rs:17-160
  public:
    static constexpr uint8_t MAX_REFLECTIONS = RTC_MAX_REFLECTIONS;
    uint32_t hsize, vsize;
    double fov, half_height, half_width, pixel_size;
    uint8_t antialiasing_samples = 1;

    static Camera new_(uint32_t hsize, uint32_t vsize, double fov) { return new_with_transform(hsize, vsize, fov, Matrix::identity()); }
    static Camera new_with_transform(uint32_t hsize, uint32_t vsize, double fov, const Matrix &m) { // camera.rs:33-37
        Camera c;
        check(rtc_camera_init(hsize, vsize, fov, m.m.data(), &c.flat_), "Camera::new_with_transform");
        c.hsize = hsize; c.vsize = vsize; c.fov = fov;
        c.half_height = c.flat_.half_height; c.half_width = c.flat_.half_width; c.pixel_size = c.flat_.pixel_size;
        return c;
    }
    void set_samples(uint8_t n) { antialiasing_samples = n; }
    // Thin lens, depth of field (rtc_lens, include/rtc.h): a square lens of half-width `aperture`, sampled at the centres of
    // usteps x vsteps cells, in focus `focal_distance` in front of the camera. With a lens set, render / render_async and
    // their rgb8 forms go through rtc_render_lens / rtc_render_lens_rgb8 (antialiasing_samples must be 1; the rgba8 forms
    // have no lens entry and throw). Not part of the reference's Camera.
    void set_lens(double aperture, double focal_distance, uint32_t usteps = 1, uint32_t vsteps = 1) {
        const rtc_lens l{aperture, focal_distance, usteps, vsteps};
        check(rtc_lens_validate(&l), "Camera::set_lens");
        if (has_projection_) check(RTC_ERR_UNSUPPORTED, "Camera::set_lens on a camera with a projection");
        lens_ = l;
        has_lens_ = true;
    }
    void clear_lens() { has_lens_ = false; }
    bool has_lens() const { return has_lens_; }
    // Orthographic and panorama cameras (rtc_projection, include/rtc.h). With a projection set, render / render_async and
    // their rgb8 forms go through rtc_render_projection / rtc_render_projection_rgb8: this camera's size and view, the
    // projection's rays (antialiasing_samples must be 1). A lens and a projection exclude each other (whichever is set second
    // throws); the rgba8 forms and a shutter have no projection entry and throw. The passes — render_aov, render_ao,
    // render_gather — do not read the camera's projection and throw while one is set: a caller who wants the planes of a
    // projection's rays says so, with the overloads below that take the rtc_projection explicitly (projection() hands the
    // camera's own back). Not part of the reference's Camera.
    void set_projection(const rtc_projection &p) {
        check(rtc_projection_validate(&p), "Camera::set_projection");
        if (has_lens_) check(RTC_ERR_UNSUPPORTED, "Camera::set_projection on a camera with a lens");
        proj_ = p;
        has_projection_ = true;
    }
    void set_orthographic(double width) { set_projection(rtc_projection{RTC_PROJ_ORTHOGRAPHIC, width, 0., 0.}); }
    void set_panorama(double h_span = 6.283185307179586 /* 2 pi */, double v_span = 3.141592653589793 /* pi */) { set_projection(rtc_projection{RTC_PROJ_PANORAMA, 0., h_span, v_span}); }
    void clear_projection() { has_projection_ = false; }
    bool has_projection() const { return has_projection_; }
    const rtc_projection &projection() const { // the projection set_projection stored; throws when none is set
        if (!has_projection_) check(RTC_ERR_ARG, "Camera::projection without a projection set");
        return proj_;
    }
    // Motion blur (rtc_shutter, include/rtc.h): with a shutter set, every render form — the lens and render_rgba8 with a
    // lens included — is the mean of `samples` frames (1..RTC_MAX_SHUTTER_SAMPLES) of the World at the cell centres of the
    // shutter interval, its shapes moved as World::set_shape_motion says, rendered and averaged on the device by one
    // process-wide rtc_shutter. Not part of the reference's Camera.
    void set_shutter(uint32_t samples) {
        if (samples == 0 || samples > RTC_MAX_SHUTTER_SAMPLES) check(RTC_ERR_ARG, "Camera::set_shutter");
        shutter_ = samples;
    }
    void clear_shutter() { shutter_ = 0; }
    uint32_t shutter() const { return shutter_; } // 0: none
    // Edge-adaptive anti-aliasing (rtc_adaptive, include/rtc.h): with it set, render / render_async / render_async1 give the
    // one-sample frame with every pixel whose 4-neighbourhood has contrast replaced by the mean of usteps x vsteps sub-samples
    // (rtc_render_adaptive); adaptive_info() says what the last such render refined. antialiasing_samples must be 1. A lens, a
    // shutter or a projection has no adaptive form, and neither have the 8-bit renders: they throw RTC_ERR_UNSUPPORTED, as
    // render_ao does. Not part of the reference's Camera.
    void set_adaptive(double threshold = RTC_AA_DEFAULT_THRESHOLD, uint32_t usteps = RTC_AA_DEFAULT_STEPS, uint32_t vsteps = RTC_AA_DEFAULT_STEPS,
                      uint32_t max_rays = 0) {
        const rtc_adaptive a{threshold, usteps, vsteps, max_rays, 0u};
        check(rtc_adaptive_validate(&a), "Camera::set_adaptive");
        adaptive_ = a;
        has_adaptive_ = true;
    }
    void clear_adaptive() { has_adaptive_ = false; }
    bool has_adaptive() const { return has_adaptive_; }
    const rtc_adaptive_info &adaptive_info() const { return adaptive_info_; }
    std::pair<Point, Vector> ray_for_pixel(uint32_t x, uint32_t y) const { // camera.rs:78-82
        double r[6];
        rtc_camera_ray_for_pixel(&flat_, x, 0.5, y, 0.5, r);
        return {Point{r[0], r[1], r[2]}, Vector{r[3], r[4], r[5]}};
    }
    Canvas render(const World &w) const { return run(w, RTC_MODE_RENDER); }             // camera.rs:116-126
    Canvas render_async(const World &w) const { return run(w, RTC_MODE_RENDER_ASYNC); } // camera.rs:144-160
    Canvas render_async1(const World &w) const { return run(w, RTC_MODE_RENDER_ASYNC); } // camera.rs:128-142
    // The same renders for a caller that only writes the image (jamis.rs / main.rs: render, then write_to_file*): the Canvas
    // comes back quantised (Canvas::rgb8), see Canvas.
    Canvas render_rgb8(const World &w) const { return run8(w, RTC_MODE_RENDER); }
    Canvas render_async_rgb8(const World &w) const { return run8(w, RTC_MODE_RENDER_ASYNC); }
    // render + canvas.set_gamma(gamma) for a caller that then calls write_to_file (main.rs, lua.rs:67): the Canvas holds
    // to_imgbuf's RGBA at that gamma (Canvas::rgba8), made on the device byte for byte as the host conversion makes it.
    Canvas render_rgba8(const World &w, float gamma) const { return run_rgba8(w, RTC_MODE_RENDER, gamma); }
    Canvas render_async_rgba8(const World &w, float gamma) const { return run_rgba8(w, RTC_MODE_RENDER_ASYNC, gamma); }
    // The AOV planes of the same frame (struct Aov): the pixel-centre ray's hit record, whatever antialiasing_samples says;
    // a lens or a shutter has no AOV form (RTC_ERR_UNSUPPORTED).
    Aov render_aov(const World &w) const { return run_aov(w, RTC_MODE_RENDER); }
    Aov render_async_aov(const World &w) const { return run_aov(w, RTC_MODE_RENDER_ASYNC); }
    // The ambient-occlusion plane of the same frame (rtc_render_ao, include/rtc.h): an Aov whose `shadow` plane holds, per
    // pixel, how many of ao.usteps x ao.vsteps hemisphere rays from the centre ray's hit meet something within ao.radius,
    // and whose n_lights is that sample count — so Aov::view(Aov::SHADOW) is the AO picture and save_exr stores the counts.
    // The other planes are empty. A lens, a shutter or a projection has no AO form (RTC_ERR_UNSUPPORTED).
    Aov render_ao(const World &w, const rtc_ao &ao) const { return run_ao(w, ao, RTC_MODE_RENDER); }
    Aov render_async_ao(const World &w, const rtc_ao &ao) const { return run_ao(w, ao, RTC_MODE_RENDER_ASYNC); }
    // The one-bounce gather pass of the same frame (rtc_render_gather): what the fan `ao` sees from every centre ray's hit,
    // shaded under the World's lights. A lens, a shutter or a projection has no gather form (RTC_ERR_UNSUPPORTED).
    Gather render_gather(const World &w, const rtc_ao &ao) const { return run_gather(w, ao, RTC_MODE_RENDER); }
    Gather render_async_gather(const World &w, const rtc_ao &ao) const { return run_gather(w, ao, RTC_MODE_RENDER_ASYNC); }
    // The same passes under an orthographic or panorama camera (rtc_render_aov_projection, rtc_render_ao_projection,
    // rtc_render_gather_projection): this camera's size and view, the rays of `p`, whether or not the camera has a
    // projection of its own set (antialiasing_samples must be 1). The planes are the C-ABI's; the Aov filters, views and
    // saves to EXR as any other. A lens or a shutter is refused, as by the forms above.
    Aov render_aov(const World &w, const rtc_projection &p) const { return run_aov(w, RTC_MODE_RENDER, &p); }
    Aov render_async_aov(const World &w, const rtc_projection &p) const { return run_aov(w, RTC_MODE_RENDER_ASYNC, &p); }
    Aov render_ao(const World &w, const rtc_ao &ao, const rtc_projection &p) const { return run_ao(w, ao, RTC_MODE_RENDER, &p); }
    Gather render_gather(const World &w, const rtc_ao &ao, const rtc_projection &p) const { return run_gather(w, ao, RTC_MODE_RENDER, &p); }

  private:
    // (`p`: the explicit projection of the overloads above; NULL: the pinhole forms, which refuse a camera with one set)
    Aov run_aov(const World &w, uint32_t mode, const rtc_projection *p = nullptr) const {
        if (has_lens_ || shutter_) check(RTC_ERR_UNSUPPORTED, "Camera::render_aov with a lens or a shutter");
        if (!p && has_projection_) check(RTC_ERR_UNSUPPORTED, "Camera::render_aov with a projection");
        rtc_camera c = flat_;
        c.samples = antialiasing_samples;
        Aov a;
        a.width = hsize; a.height = vsize;
        const size_t px = static_cast<size_t>(hsize) * vsize;
        a.index.assign(px, -1); a.depth.assign(px, 0.0); a.point.assign(px * 3, 0.0); a.normal.assign(px * 3, 0.0);
        a.flags.assign(px, 0); a.shadow.assign(px, 0);
        World::Uploaded up(w);
        a.n_lights = rtc_world_light_count(up.w);
        const rtc_aov_buffers b = a.buffers();
        if (p) check(rtc_render_aov_projection(Device::get(), up.w, &c, p, mode, RTC_FLAG_NONE, &b), "Camera::render_aov");
        else check(rtc_render_aov(Device::get(), up.w, &c, mode, RTC_FLAG_NONE, &b), "Camera::render_aov");
        return a;
    }
    Aov run_ao(const World &w, const rtc_ao &ao, uint32_t mode, const rtc_projection *p = nullptr) const {
        if (has_lens_ || shutter_ || (!p && has_projection_)) check(RTC_ERR_UNSUPPORTED, "Camera::render_ao with a lens, a shutter or a projection");
        check(rtc_ao_validate(&ao), "Camera::render_ao");
        rtc_camera c = flat_;
        c.samples = antialiasing_samples;
        Aov a;
        a.width = hsize; a.height = vsize;
        a.n_lights = ao.usteps * ao.vsteps;
        a.shadow.assign(static_cast<size_t>(hsize) * vsize, 0);
        World::Uploaded up(w);
        if (p) check(rtc_render_ao_projection(Device::get(), up.w, &c, p, &ao, mode, RTC_FLAG_NONE, a.shadow.data()), "Camera::render_ao");
        else check(rtc_render_ao(Device::get(), up.w, &c, &ao, mode, RTC_FLAG_NONE, a.shadow.data()), "Camera::render_ao");
        return a;
    }
    Gather run_gather(const World &w, const rtc_ao &ao, uint32_t mode, const rtc_projection *p = nullptr) const {
        if (has_lens_ || shutter_ || (!p && has_projection_)) check(RTC_ERR_UNSUPPORTED, "Camera::render_gather with a lens, a shutter or a projection");
        check(rtc_ao_validate(&ao), "Camera::render_gather");
        rtc_camera c = flat_;
        c.samples = antialiasing_samples;
        Gather g;
        g.width = hsize; g.height = vsize;
        g.radiance.assign(static_cast<size_t>(hsize) * vsize * 3, 0.0);
        g.bounce.assign(static_cast<size_t>(hsize) * vsize * 3, 0.0);
        const rtc_gather_buffers b{g.radiance.data(), g.bounce.data()};
        World::Uploaded up(w);
        if (p) check(rtc_render_gather_projection(Device::get(), up.w, &c, p, &ao, mode, RTC_FLAG_NONE, &b), "Camera::render_gather");
        else check(rtc_render_gather(Device::get(), up.w, &c, &ao, mode, RTC_FLAG_NONE, &b), "Camera::render_gather");
        return g;
    }
    Canvas run(const World &w, uint32_t mode) const {
        rtc_camera c = flat_;
        c.samples = antialiasing_samples;
        Canvas canvas(hsize, vsize);
        if (has_adaptive_) {
            if (has_lens_ || shutter_ || has_projection_) check(RTC_ERR_UNSUPPORTED, "Camera::render with adaptive anti-aliasing and a lens, a shutter or a projection");
            World::Uploaded up(w);
            check(rtc_render_adaptive(Device::get(), up.w, &c, &adaptive_, mode, RTC_FLAG_NONE, canvas.pixels.data(), nullptr, &adaptive_info_, nullptr),
                  "Camera::render");
            return canvas;
        }
        if (has_projection_) {
            if (shutter_) check(RTC_ERR_UNSUPPORTED, "Camera::render with a projection and a shutter");
            World::Uploaded up(w);
            check(rtc_render_projection(Device::get(), up.w, &c, &proj_, mode, RTC_FLAG_NONE, canvas.pixels.data(), nullptr), "Camera::render");
            return canvas;
        }
        if (shutter_) {
            Exposure e(w, c, has_lens_ ? &lens_ : nullptr, shutter_);
            check(rtc_shutter_render(Exposure::shutter(), &e.scene, mode, RTC_FLAG_NONE, canvas.pixels.data(), nullptr), "Camera::render");
            return canvas;
        }
        World::Uploaded up(w);
        if (has_lens_) check(rtc_render_lens(Device::get(), up.w, &c, &lens_, mode, RTC_FLAG_NONE, canvas.pixels.data(), nullptr), "Camera::render");
        else check(rtc_render(Device::get(), up.w, &c, mode, RTC_FLAG_NONE, canvas.pixels.data(), nullptr), "Camera::render");
        return canvas;
    }
    Canvas run8(const World &w, uint32_t mode) const {
        if (has_adaptive_) check(RTC_ERR_UNSUPPORTED, "Camera::render_rgb8 with adaptive anti-aliasing");
        rtc_camera c = flat_;
        c.samples = antialiasing_samples;
        Canvas canvas = Canvas::quantised(hsize, vsize);
        if (has_projection_) {
            if (shutter_) check(RTC_ERR_UNSUPPORTED, "Camera::render with a projection and a shutter");
            World::Uploaded up(w);
            check(rtc_render_projection_rgb8(Device::get(), up.w, &c, &proj_, mode, RTC_FLAG_NONE, canvas.rgb8.data(), nullptr), "Camera::render");
            return canvas;
        }
        if (shutter_) {
            Exposure e(w, c, has_lens_ ? &lens_ : nullptr, shutter_);
            check(rtc_shutter_render_rgb8(Exposure::shutter(), &e.scene, mode, RTC_FLAG_NONE, canvas.rgb8.data(), nullptr), "Camera::render");
            return canvas;
        }
        World::Uploaded up(w);
        if (has_lens_) check(rtc_render_lens_rgb8(Device::get(), up.w, &c, &lens_, mode, RTC_FLAG_NONE, canvas.rgb8.data(), nullptr), "Camera::render");
        else check(rtc_render_rgb8(Device::get(), up.w, &c, mode, RTC_FLAG_NONE, canvas.rgb8.data(), nullptr), "Camera::render");
        return canvas;
    }
    Canvas run_rgba8(const World &w, uint32_t mode, float gamma) const {
        if (has_adaptive_) check(RTC_ERR_UNSUPPORTED, "Camera::render_rgba8 with adaptive anti-aliasing");
        rtc_camera c = flat_;
        c.samples = antialiasing_samples;
        if (has_projection_) check(RTC_ERR_UNSUPPORTED, "Camera::render_rgba8 with a projection");
        if (shutter_) { // (this path has a lens entry: the mean's RGBA is made by the averaging kernel)
            Canvas canvas = Canvas::imgbuf(hsize, vsize, gamma);
            Exposure e(w, c, has_lens_ ? &lens_ : nullptr, shutter_);
            check(rtc_shutter_render_rgba8(Exposure::shutter(), &e.scene, mode, RTC_FLAG_NONE, gamma, canvas.rgba8.data(), nullptr), "Camera::render_rgba8");
            return canvas;
        }
        if (has_lens_) check(RTC_ERR_UNSUPPORTED, "Camera::render_rgba8 with a lens");
        Canvas canvas = Canvas::imgbuf(hsize, vsize, gamma);
        World::Uploaded up(w);
        check(rtc_render_rgba8(Device::get(), up.w, &c, mode, RTC_FLAG_NONE, gamma, canvas.rgba8.data(), nullptr), "Camera::render_rgba8");
        return canvas;
    }
    // One motion-blurred frame's scene (rtc_shutter_scene) with the arrays it points into, and the process-wide shutter.
    struct Exposure {
        std::vector<rtc_shape> flat;
        std::vector<rtc_motion> moves;
        std::vector<rtc_area_light> lights;
        rtc_camera cam;
        rtc_shutter_scene scene{};
        Exposure(const World &w, const rtc_camera &c, const rtc_lens *lens, uint32_t samples) : cam(c) {
            for (const Shape &s : w.shapes) {
                rtc_shape f = s.flat;
                f.material = s.material.flatten();
                flat.push_back(f);
            }
            for (const auto &mv : w.motions) {
                rtc_motion m{};
                m.shape = static_cast<uint32_t>(mv.first);
                std::memcpy(m.transform_open, w.shapes.at(mv.first).transform.m.data(), sizeof m.transform_open);
                std::memcpy(m.transform_close, mv.second.m.data(), sizeof m.transform_close);
                moves.push_back(m);
            }
            for (const Light &wl : w.lights()) { // the World's sample list: its point lights, then its area lights
                rtc_light l;
                l.intensity[0] = wl.intensity.red; l.intensity[1] = wl.intensity.green; l.intensity[2] = wl.intensity.blue;
                l.position[0] = wl.position.x; l.position[1] = wl.position.y; l.position[2] = wl.position.z;
                rtc_area_light a;
                check(rtc_area_light_from_point(&l, &a), "World lights");
                lights.push_back(a);
            }
            lights.insert(lights.end(), w.area_lights.begin(), w.area_lights.end());
            scene.shapes = flat.data(); scene.n_shapes = static_cast<uint32_t>(flat.size());
            scene.motions = moves.data(); scene.n_motions = static_cast<uint32_t>(moves.size());
            scene.lights = lights.data(); scene.n_lights = static_cast<uint32_t>(lights.size());
            scene.cam_open = &cam; scene.cam_close = nullptr;
            scene.lens = lens;
            scene.samples = samples;
        }
        Exposure(const Exposure &) = delete;
        Exposure &operator=(const Exposure &) = delete;
        static rtc_shutter *shutter() {
            struct Holder {
                rtc_shutter *s = nullptr;
                Holder() { check(rtc_shutter_create(Device::get(), &s), "rtc_shutter_create"); } // (the context is constructed first, destroyed last)
                ~Holder() { rtc_shutter_destroy(s); }
            };
            static Holder h;
            return h.s;
        }
    };
    rtc_camera flat_{};
    rtc_lens lens_{0., 1., 1u, 1u};
    bool has_lens_ = false;
    rtc_projection proj_{};
    bool has_projection_ = false;
    uint32_t shutter_ = 0;
    rtc_adaptive adaptive_{};
    bool has_adaptive_ = false;
    mutable rtc_adaptive_info adaptive_info_{};
};

namespace detail {
struct LuaProgramGuard {
    rtc_lua_program *p;
    ~LuaProgramGuard() { rtc_lua_program_free(p); }
};
template <class Sink>
struct LuaSink {
    Sink *sink;
    std::exception_ptr thrown;
    static int frame(void *user, const rtc_lua_job *job, uint32_t, const uint8_t *rgb8) {
        LuaSink *c = static_cast<LuaSink *>(user);
        try {
            Canvas canvas = Canvas::quantised(job->camera.hsize, job->camera.vsize);
            canvas.rgb8.assign(rgb8, rgb8 + canvas.rgb8.size());
            (*c->sink)(canvas, std::string(job->outfile), job->kind == RTC_LUA_JOB_ADD_FRAME ? static_cast<int>(job->frame) : -1);
            return 0;
        } catch (...) { // never unwind through the C library
            c->thrown = std::current_exception();
            return 1;
        }
    }
};
} // namespace detail

// render_lua (lua.rs:50-91): run a scene script and render what it asks for. The reference writes each Render's Canvas
// with `image` (PNG / JPEG by extension) and each animation as a GIF; here the frames are handed to `sink` instead —
// (Canvas holding the 8-bit frame, the file name the script gave, frame number inside its animation or -1 for Render) — in
// the order the script made the calls, for write_to_file (PNG) or write_to_file_jpeg. Returns what the script print()ed.
template <class Sink>
inline std::string render_lua(const std::string &script, Sink &&sink) {
    char err[512] = "";
    rtc_lua_program *prog = nullptr;
    const rtc_status st = rtc_lua_run_file(script.c_str(), 0, &prog, err, sizeof err);
    if (st != RTC_OK) throw Panic(st, std::string("render_lua: ") + err); // lua.rs unwrap()s
    detail::LuaProgramGuard guard{prog};
    typedef typename std::remove_reference<Sink>::type SinkT;
    detail::LuaSink<SinkT> ctx{&sink, nullptr};
    const rtc_status rs = rtc_lua_program_render(Device::get(), prog, RTC_MODE_RENDER_ASYNC, RTC_FLAG_NONE, &detail::LuaSink<SinkT>::frame, &ctx, nullptr);
    if (ctx.thrown) std::rethrow_exception(ctx.thrown);
    check(rs, "render_lua");
    return rtc_lua_program_output(prog);
}

} // namespace ch1
#endif
