// test_facade_lens.cpp — the C++ mirror's Camera::set_lens (raytracer-challenge_amd/host/ch1.hpp): with a lens set,
// render / render_async give the canvas rtc_render_lens gives for the same World, camera and lens; clear_lens brings the
// pinhole frame back, and the degenerate lens IS the pinhole frame. Built by build.py's build_facade_lens_test and run by
// tests/test_gpu_lens.py (marked gpu); exits non-zero on failure.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ch1.hpp"

using namespace ch1;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static World scene() {
    World w = World::new_(Light::new_(Color::new_(1., 0.95, 0.9), Point::new_(-6., 8., -8.)));
    w.add_shape(Plane::new_());
    w.add_shape(Sphere::new_with_transform_and_material(Matrix::identity().scaling(0.6, 0.6, 0.6).translation(-1.1, 0.6, -3.5),
                                                        Material::solid_with_defaults(Color::new_(0.9, 0.3, 0.2))));
    w.add_shape(Sphere::new_with_transform_and_material(Matrix::identity().translation(0.2, 1., 0.),
                                                        Material::solid_with_defaults(Color::new_(0.25, 0.7, 0.35))));
    return w;
}

static bool same_pixels(const Canvas &a, const Canvas &b) {
    return a.pixels.size() == b.pixels.size() && std::memcmp(a.pixels.data(), b.pixels.data(), a.pixels.size() * sizeof(double)) == 0;
}

// the same World through the C-ABI
static Canvas through_abi(const World &w, const rtc_camera &cam, const rtc_lens &lens, uint32_t mode) {
    std::vector<rtc_shape> flat;
    for (const Shape &s : w.shapes) { rtc_shape f = s.flat; f.material = s.material.flatten(); flat.push_back(f); }
    rtc_light l;
    l.intensity[0] = 1.; l.intensity[1] = 0.95; l.intensity[2] = 0.9;
    l.position[0] = -6.; l.position[1] = 8.; l.position[2] = -8.;
    rtc_world *fresh = nullptr;
    check(rtc_world_create(Device::get(), flat.data(), (uint32_t)flat.size(), &l, &fresh), "fresh world");
    Canvas c(64, 48);
    check(rtc_render_lens(Device::get(), fresh, &cam, &lens, mode, 0, c.pixels.data(), nullptr), "fresh lens render");
    rtc_world_destroy(fresh);
    return c;
}

int main() {
    try {
        const Matrix view = Matrix::make_view_transform(Point::new_(0., 1.5, -7.), Point::new_(0., 1., 0.), Vector::new_(0., 1., 0.));
        Camera camera = Camera::new_with_transform(64, 48, 0.8, view);
        rtc_camera flat_camera;
        check(rtc_camera_init(64, 48, 0.8, view.m.data(), &flat_camera), "rtc_camera_init");
        const World w = scene();
        const Canvas pinhole = camera.render_async(w);
        EXPECT(!camera.has_lens());
        camera.set_lens(0.15, 7., 3, 2);
        EXPECT(camera.has_lens());
        const rtc_lens lens{0.15, 7., 3u, 2u};
        const Canvas blurred = camera.render_async(w);
        EXPECT(!same_pixels(blurred, pinhole));
        EXPECT(same_pixels(blurred, through_abi(w, flat_camera, lens, RTC_MODE_RENDER_ASYNC)));
        EXPECT(same_pixels(camera.render(w), through_abi(w, flat_camera, lens, RTC_MODE_RENDER)));
        rtc_launch_info info;
        check(rtc_context_last_launch_info(Device::get(), &info), "launch info");
        EXPECT(info.lens_samples == 6u && info.binned == 0u);
        // the 8-bit form goes through rtc_render_lens_rgb8: Color::scale of the f64 frame
        const Canvas q = camera.render_async_rgb8(w);
        std::vector<uint8_t> want(blurred.pixels.size());
        rtc_color_scale255(blurred.pixels.data(), blurred.pixels.size(), want.data());
        EXPECT(q.rgb8.size() == want.size() && std::memcmp(q.rgb8.data(), want.data(), want.size()) == 0);
        // the degenerate lens is the pinhole camera; so is no lens
        camera.set_lens(0., 1.);
        EXPECT(same_pixels(camera.render_async(w), pinhole));
        camera.set_lens(0.15, 7., 3, 2);
        camera.clear_lens();
        EXPECT(!camera.has_lens() && same_pixels(camera.render_async(w), pinhole));
        check(rtc_context_last_launch_info(Device::get(), &info), "launch info");
        EXPECT(info.lens_samples == 0u);
        // refused lenses leave the camera as it was; anti-aliasing and the lens do not compose
        bool refused = false;
        try { camera.set_lens(0.1, 0., 2, 2); } catch (const Panic &) { refused = true; }
        EXPECT(refused && !camera.has_lens());
        refused = false;
        try { camera.set_lens(0.1, 5., 17, 16); } catch (const Panic &) { refused = true; }
        EXPECT(refused && !camera.has_lens());
        camera.set_lens(0.15, 7., 2, 2);
        camera.set_samples(4);
        refused = false;
        try { (void)camera.render_async(w); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
    } catch (const Panic &p) {
        std::printf("FAIL panic: %s\n", p.what());
        ++failures;
    }
    if (failures == 0) std::printf("facade lens: ok\n");
    return failures ? 1 : 0;
}
