// test_facade_float.cpp — the C++ mirror's float files (raytracer-challenge_amd/host/ch1.hpp): Canvas::save of an f64
// Canvas under the names of the float table (hdr, pfm, exr), through a lens too, and Aov::save_exr with and without a colour
// Canvas. Writes the files and the raw canvases and planes into the directory argv[1]; tests/test_gpu_float_formats.py
// (marked gpu) compares them with the Python layer's bytes. Built by build.py's build_facade_float_test; exits non-zero on
// failure.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "ch1.hpp"

using namespace ch1;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

template <class T> static void dump(const std::string &path, const std::vector<T> &v) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::printf("FAIL cannot write %s\n", path.c_str()); ++failures; }
    if (f) std::fclose(f);
}

static bool exists(const std::string &path) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (f) std::fclose(f);
    return f != nullptr;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::puts("usage: test_facade_float DIR"); return 2; }
    const std::string dir = argv[1];
    try {
        World world = World::new_(Light::new_(Color::new_(1.8, 1.6, 1.4), Point::new_(-6., 8., -8.))); // bright: components above 1.0
        world.add_shape(Plane::new_());
        world.add_shape(Sphere::new_with_transform_and_material(Matrix::identity().scaling(0.8, 0.8, 0.8).translation(-0.6, 0.8, -1.),
                                                                Material::solid_with_defaults(Color::new_(0.9, 0.5, 0.2))));
        Camera camera = Camera::new_with_transform(61, 37, M_PI / 3.0,
            Matrix::make_view_transform(Point::new_(0., 1.5, -5.), Point::new_(0., 0.5, 0.), Vector::new_(0., 1., 0.)));
        const Canvas f64 = camera.render_async(world);
        dump(dir + "/f64.bin", f64.pixels);
        for (const char *n : {"a.hdr", "b.PFM", "c.exr"}) f64.save(dir + "/" + n);
        // a quantised Canvas holds no numbers to keep: the 8-bit table, which has no such name
        const Canvas rgb8 = camera.render_rgb8(world);
        bool refused = false;
        try { rgb8.save(dir + "/q.hdr"); } catch (const Panic &p) { refused = p.status == RTC_ERR_UNSUPPORTED; }
        EXPECT(refused && !exists(dir + "/q.hdr"));
        refused = false;
        try { f64.save(dir + "/x.xyz"); } catch (const Panic &p) { refused = p.status == RTC_ERR_UNSUPPORTED; }
        EXPECT(refused && !exists(dir + "/x.xyz"));
        f64.save(dir + "/still.png"); // the 8-bit table as before
        EXPECT(exists(dir + "/still.png"));
        // the planes, with and without the colour
        const Aov aov = camera.render_async_aov(world);
        dump(dir + "/index.bin", aov.index);
        dump(dir + "/depth.bin", aov.depth);
        dump(dir + "/point.bin", aov.point);
        dump(dir + "/normal.bin", aov.normal);
        dump(dir + "/flags.bin", aov.flags);
        dump(dir + "/shadow.bin", aov.shadow);
        aov.save_exr(dir + "/aov_colour.exr", &f64);
        aov.save_exr(dir + "/aov_colour_float.exr", &f64, true);
        aov.save_exr(dir + "/aov_planes.exr");
        refused = false;
        try { aov.save_exr(dir + "/bad.exr", &rgb8); } catch (const Panic &p) { refused = p.status == RTC_ERR_ARG; }
        EXPECT(refused && !exists(dir + "/bad.exr"));
        // through a lens
        camera.set_lens(0.1, 5., 2, 2);
        const Canvas lens = camera.render_async(world);
        dump(dir + "/lens.bin", lens.pixels);
        lens.save(dir + "/lens.hdr");
        EXPECT(lens.pixels != f64.pixels);
    } catch (const Panic &p) {
        std::printf("FAIL panic: %s\n", p.what());
        ++failures;
    }
    if (failures == 0) std::printf("facade float: ok\n");
    return failures ? 1 : 0;
}
