// test_facade_filter.cpp — the C++ mirror's edge-aware filter (raytracer-challenge_amd/host/ch1.hpp): Aov::occlusion is
// rtc_counts_to_fraction of the Aov's shadow plane, Aov::filter is rtc_plane_filter under the Aov's own guides — for the
// one-channel occlusion plane and for a Gather's three-channel bounce plane — Canvas::apply_occlusion is
// rtc_canvas_apply_occlusion (and, unfiltered, Canvas::apply_ao), and planes of the wrong size or a bad filter are refused.
// Built by build.py's build_facade_filter_test and run by tests/test_gpu_filter.py (marked gpu); exits non-zero on failure.
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

static World scene() { // a sphere and a cube resting on a floor
    World w = World::new_(Light::new_(Color::new_(1., 0.95, 0.9), Point::new_(-6., 8., -8.)));
    w.add_shape(Plane::new_());
    w.add_shape(Sphere::new_with_transform_and_material(Matrix::identity().scaling(0.8, 0.8, 0.8).translation(-1.1, 0.8, -1.5),
                                                        Material::solid_with_defaults(Color::new_(0.9, 0.3, 0.2))));
    w.add_shape(Cube::new_with_transform_and_material(Matrix::identity().scaling(0.7, 0.7, 0.7).rotation_y(0.5).translation(0.9, 0.7, 0.),
                                                      Material::solid_with_defaults(Color::new_(0.25, 0.7, 0.35))));
    return w;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

int main() {
    try {
        const uint32_t W = 37, H = 21; // partial tiles on both edges
        const Matrix view = Matrix::make_view_transform(Point::new_(0., 2.5, -7.), Point::new_(0., 0.5, 0.), Vector::new_(0., 1., 0.));
        const Camera camera = Camera::new_with_transform(W, H, 0.8, view);
        const World w = scene();
        const rtc_ao fan{1.5, 4u, 4u};
        Aov guides = camera.render_async_aov(w);
        const Aov ao = camera.render_async_ao(w, fan);
        const Gather gather = camera.render_async_gather(w, fan);
        EXPECT(guides.index.size() == (size_t)W * H && ao.n_lights == 16u && gather.bounce.size() == (size_t)W * H * 3);

        // the fraction
        const std::vector<double> occ = ao.occlusion();
        std::vector<double> want_occ((size_t)W * H);
        check(rtc_counts_to_fraction(ao.shadow.data(), 16u, W, H, want_occ.data()), "rtc_counts_to_fraction");
        EXPECT(same(occ, want_occ));
        bool some = false;
        for (size_t i = 0; i < occ.size(); ++i) {
            EXPECT(occ[i] == (double)ao.shadow[i] / 16.0);
            some = some || (occ[i] > 0. && occ[i] < 1.);
        }
        EXPECT(some);

        // the filter, one channel and three, is the host statement under the Aov's guides
        const rtc_filter spec = Aov::default_filter();
        EXPECT(rtc_filter_validate(&spec) == RTC_OK && spec.passes == RTC_FILTER_DEFAULT_PASSES && spec.flags == RTC_FILTER_SAME_OBJECT);
        const rtc_aov_buffers b = guides.buffers();
        const std::vector<double> smooth = guides.filter(occ, 1, spec);
        std::vector<double> want(occ.size());
        check(rtc_plane_filter(occ.data(), 1, &b, W, H, &spec, want.data()), "rtc_plane_filter");
        EXPECT(same(smooth, want) && !same(smooth, occ));
        const rtc_filter wide{std::numeric_limits<double>::infinity(), 4u, 0u, 0u, 0u};
        const std::vector<double> bounce = guides.filter(gather.bounce, 3, wide);
        std::vector<double> want3(gather.bounce.size());
        check(rtc_plane_filter(gather.bounce.data(), 3, &b, W, H, &wide, want3.data()), "rtc_plane_filter");
        EXPECT(same(bounce, want3) && !same(bounce, gather.bounce));
        for (size_t i = 0; i < (size_t)W * H; ++i)
            if (guides.index[i] < 0) EXPECT(smooth[i] == occ[i] && bounce[3 * i] == gather.bounce[3 * i]); // a miss is copied

        // compositing: the fraction as it is gives apply_ao's bytes; the filtered one is the host statement
        Canvas beauty = camera.render_async(w);
        Canvas by_counts = beauty, by_fraction = beauty;
        by_counts.apply_ao(ao.shadow, ao.n_lights, 0.75);
        by_fraction.apply_occlusion(occ, 0.75);
        EXPECT(same(by_counts.pixels, by_fraction.pixels));
        std::vector<double> expected = beauty.pixels;
        check(rtc_canvas_apply_occlusion(expected.data(), smooth.data(), 0.75, W, H), "rtc_canvas_apply_occlusion");
        check(rtc_canvas_add_scaled(expected.data(), bounce.data(), 1.0, W, H), "rtc_canvas_add_scaled");
        beauty.apply_occlusion(smooth, 0.75);
        beauty.add_scaled(bounce);
        EXPECT(same(beauty.pixels, expected) && !same(beauty.pixels, by_fraction.pixels));

        // what is refused
        bool refused = false;
        try { beauty.apply_occlusion(smooth, 1.5); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
        refused = false;
        try { beauty.apply_occlusion(bounce, 0.5); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
        refused = false;
        try { (void)guides.filter(occ, 3, spec); } catch (const Panic &) { refused = true; } // a one-channel plane called three
        EXPECT(refused);
        refused = false;
        try { (void)guides.filter(occ, 1, rtc_filter{0.05, 6u, 1u, 0u, 0u}); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
        refused = false;
        try { (void)ao.filter(occ, 1, spec); } catch (const Panic &) { refused = true; } // an Aov without guides
        EXPECT(refused);
    } catch (const Panic &p) {
        std::printf("FAIL panic: %s\n", p.what());
        ++failures;
    }
    if (failures == 0) std::printf("facade filter: ok\n");
    return failures ? 1 : 0;
}
