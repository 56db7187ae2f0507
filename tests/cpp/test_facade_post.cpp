// test_facade_post.cpp — the C++ mirror's post-processing (raytracer-challenge_amd/host/ch1.hpp): Canvas::bloom is
// rtc_canvas_bloom, Canvas::luminance is rtc_canvas_luminance and Canvas::tonemap is rtc_canvas_tonemap, which takes the
// statistics itself when a flag asks for them. The facade's bytes equal the C-ABI's on a frame rendered on the device under
// three lights; a bad record or an 8-bit Canvas is refused.
// Built by build.py's build_facade_post_test and run by tests/test_gpu_facade_post.py (marked gpu); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ch1.hpp"

using namespace ch1;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

static World scene() { // a shiny sphere on a pale floor under three lights: the floor and the highlight are brighter than 1.0
    World w = World::new_(Light::new_(Color::new_(1.6, 1.5, 1.4), Point::new_(-6., 9., -8.)));
    w.add_light(Light::new_(Color::new_(1.2, 1.3, 1.5), Point::new_(5., 7., -6.)));
    w.add_light(Light::new_(Color::new_(1.4, 1.4, 1.4), Point::new_(0., 10., 3.)));
    w.add_shape(Plane::new_with_transform_and_material(Matrix::identity(), Material::solid_with_defaults(Color::new_(0.9, 0.88, 0.82))));
    w.add_shape(Sphere::new_with_transform_and_material(Matrix::identity().translation(0., 1., 0.), Material::solid_with_defaults(Color::new_(0.9, 0.9, 0.95))));
    return w;
}

int main() {
    try {
        const uint32_t W = 70, H = 37; // more than one tile across, partial tiles on both edges
        const Matrix view = Matrix::make_view_transform(Point::new_(0., 2.4, -7.5), Point::new_(0., 0.8, 0.), Vector::new_(0., 1., 0.));
        const Camera camera = Camera::new_with_transform(W, H, 0.9, view);
        const Canvas frame = camera.render_async(scene());
        EXPECT(frame.pixels.size() == (size_t)W * H * 3);

        // the statistics
        const rtc_luminance st = frame.luminance();
        rtc_luminance want_st{};
        check(rtc_canvas_luminance(frame.pixels.data(), W, H, &want_st), "rtc_canvas_luminance");
        EXPECT(std::memcmp(&st, &want_st, sizeof st) == 0 && st.max > 1.5 && st.count > 0);

        // bloom
        const rtc_bloom glare{1.0, 0.6, 3.0, 9u, 0u};
        Canvas bloomed = frame;
        bloomed.bloom(glare);
        std::vector<double> want(frame.pixels.size());
        check(rtc_canvas_bloom(frame.pixels.data(), W, H, &glare, want.data()), "rtc_canvas_bloom");
        EXPECT(same(bloomed.pixels, want) && !same(bloomed.pixels, frame.pixels));

        // the tone map: fixed exposure, and with both AUTO flags, where the Canvas takes its own statistics
        const rtc_tonemap fixed{0.5, 4.0, RTC_TONEMAP_ACES, 0u};
        Canvas mapped = bloomed;
        mapped.tonemap(fixed);
        check(rtc_canvas_tonemap(bloomed.pixels.data(), W, H, &fixed, nullptr, want.data()), "rtc_canvas_tonemap");
        EXPECT(same(mapped.pixels, want));
        const rtc_tonemap automatic{0.18, 1.0, RTC_TONEMAP_REINHARD, RTC_TONEMAP_AUTO_EXPOSURE | RTC_TONEMAP_AUTO_WHITE};
        Canvas auto_mapped = bloomed;
        auto_mapped.tonemap(automatic);
        rtc_luminance bst{};
        check(rtc_canvas_luminance(bloomed.pixels.data(), W, H, &bst), "rtc_canvas_luminance");
        check(rtc_canvas_tonemap(bloomed.pixels.data(), W, H, &automatic, &bst, want.data()), "rtc_canvas_tonemap");
        EXPECT(same(auto_mapped.pixels, want) && !same(auto_mapped.pixels, bloomed.pixels));
        EXPECT(bst.max > 1.5);

        // what is refused
        bool refused = false;
        try { bloomed.bloom(rtc_bloom{1.0, 0.6, 3.0, 33u, 0u}); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
        refused = false;
        try { bloomed.tonemap(rtc_tonemap{0.0, 1.0, RTC_TONEMAP_LINEAR, 0u}); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
        refused = false;
        try { Canvas q = Canvas::quantised(4, 4); q.tonemap(fixed); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
        refused = false;
        try { Canvas q = Canvas::quantised(4, 4); q.bloom(glare); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
    } catch (const Panic &p) {
        std::printf("FAIL panic: %s\n", p.what());
        ++failures;
    }
    if (failures == 0) std::printf("facade post: ok\n");
    return failures ? 1 : 0;
}
