// test_facade_aov.cpp — the C++ mirror's AOV planes (raytracer-challenge_amd/host/ch1.hpp): Camera::render_aov /
// render_async_aov give the planes rtc_aov_from_hits packs from rtc_color_at's hit records of the same pixel-centre rays
// (k_trace's own records: every byte must agree), Aov::view gives rtc_aov_view_rgb8's picture, and a lens or a shutter is
// refused. Built by build.py's build_facade_aov_test and run by tests/test_gpu_facade_aov.py (marked gpu); exits non-zero
// on failure.
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
    w.add_shape(Cube::new_with_transform_and_material(Matrix::identity().scaling(0.7, 0.7, 0.7).rotation_y(0.5).translation(0.9, 0.7, 0.),
                                                      Material::solid_with_defaults(Color::new_(0.25, 0.7, 0.35))));
    return w;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0;
}

// the planes from the probe kernel's hit records of the same World and rays, packed by the host statement
static Aov through_color_at(const World &w, const Camera &camera, const rtc_camera &cam, uint32_t mode) {
    std::vector<rtc_shape> flat;
    for (const Shape &s : w.shapes) { rtc_shape f = s.flat; f.material = s.material.flatten(); flat.push_back(f); }
    rtc_light l;
    l.intensity[0] = 1.; l.intensity[1] = 0.95; l.intensity[2] = 0.9;
    l.position[0] = -6.; l.position[1] = 8.; l.position[2] = -8.;
    rtc_world *fresh = nullptr;
    check(rtc_world_create(Device::get(), flat.data(), (uint32_t)flat.size(), &l, &fresh), "fresh world");
    const size_t px = (size_t)cam.hsize * cam.vsize;
    std::vector<double> rays(px * 6), rgb(px * 3);
    for (uint32_t y = 0; y < cam.vsize; ++y)
        for (uint32_t x = 0; x < cam.hsize; ++x) rtc_camera_ray_for_pixel(&cam, x, 0.5, y, 0.5, &rays[((size_t)y * cam.hsize + x) * 6]);
    std::vector<rtc_hit> hits(px);
    check(rtc_color_at(Device::get(), fresh, rays.data(), (uint32_t)px, RTC_MAX_REFLECTIONS, 0, rgb.data(), hits.data()), "rtc_color_at");
    rtc_world_destroy(fresh);
    Aov a;
    a.width = camera.hsize; a.height = camera.vsize;
    a.index.assign(px, 7); a.depth.assign(px, 7.); a.point.assign(px * 3, 7.); a.normal.assign(px * 3, 7.); a.flags.assign(px, 7); a.shadow.assign(px, 7);
    const rtc_aov_buffers b = a.buffers();
    check(rtc_aov_from_hits(hits.data(), nullptr, cam.hsize, cam.vsize, mode, &b), "rtc_aov_from_hits");
    return a;
}

static bool same_planes(const Aov &a, const Aov &b) {
    return same(a.index, b.index) && same(a.depth, b.depth) && same(a.point, b.point) && same(a.normal, b.normal) && same(a.flags, b.flags) &&
           same(a.shadow, b.shadow);
}

int main() {
    try {
        const Matrix view = Matrix::make_view_transform(Point::new_(0., 1.5, -7.), Point::new_(0., 1., 0.), Vector::new_(0., 1., 0.));
        Camera camera = Camera::new_with_transform(37, 21, 0.8, view); // partial tiles on both edges
        rtc_camera flat_camera;
        check(rtc_camera_init(37, 21, 0.8, view.m.data(), &flat_camera), "rtc_camera_init");
        const World w = scene();
        const Aov a = camera.render_async_aov(w);
        EXPECT(a.width == 37u && a.height == 21u && a.n_lights == 1u && a.index.size() == 37u * 21u && a.point.size() == 37u * 21u * 3u);
        EXPECT(same_planes(a, through_color_at(w, camera, flat_camera, RTC_MODE_RENDER_ASYNC)));
        const Aov serial = camera.render_aov(w);
        EXPECT(same_planes(serial, through_color_at(w, camera, flat_camera, RTC_MODE_RENDER)));
        EXPECT(serial.index[37u * 21u - 1u] == -1 && !serial.hit(36, 20) && std::isinf(serial.depth[36]));
        // the frame holds hits, misses and shadowed pixels, and every kind of shape
        size_t hits = 0, misses = 0, shadowed = 0;
        bool kinds[3] = {false, false, false};
        for (size_t i = 0; i < a.index.size(); ++i) {
            if (a.index[i] < 0) { ++misses; continue; }
            ++hits;
            kinds[a.index[i]] = true;
            shadowed += a.shadow[i];
        }
        EXPECT(hits > 0 && misses > 0 && shadowed > 0 && kinds[0] && kinds[1] && kinds[2]);
        // anti-aliasing does not move the AOV ray: the centre sample
        camera.set_samples(4);
        EXPECT(same_planes(camera.render_async_aov(w), a));
        camera.set_samples(1);
        // views: the host statement's bytes, as a quantised Canvas
        double near = INFINITY, far = 0.;
        for (double t : a.depth)
            if (std::isfinite(t)) { near = std::fmin(near, t); far = std::fmax(far, t); }
        const rtc_aov_buffers b = const_cast<Aov &>(a).buffers();
        for (Aov::View v : {Aov::DEPTH, Aov::NORMAL, Aov::INDEX, Aov::SHADOW}) {
            const Canvas c = a.view(v, near, far);
            std::vector<uint8_t> want(37u * 21u * 3u);
            check(rtc_aov_view_rgb8(v, &b, 37, 21, near, far, 1, want.data()), "rtc_aov_view_rgb8");
            EXPECT(c.is_quantised() && same(c.rgb8, want));
        }
        // a lens or a shutter has no AOV form
        bool refused = false;
        camera.set_lens(0.15, 7., 2, 2);
        try { (void)camera.render_async_aov(w); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
        camera.clear_lens();
        camera.set_shutter(4);
        refused = false;
        try { (void)camera.render_aov(w); } catch (const Panic &) { refused = true; }
        EXPECT(refused);
        camera.clear_shutter();
        EXPECT(same_planes(camera.render_async_aov(w), a));
    } catch (const Panic &p) {
        std::printf("FAIL panic: %s\n", p.what());
        ++failures;
    }
    if (failures == 0) std::printf("facade aov: ok\n");
    return failures ? 1 : 0;
}
