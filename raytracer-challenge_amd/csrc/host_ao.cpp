// host_ao.cpp — [host] the normative statements of the ambient-occlusion pass (include/rtc.h, "ambient occlusion"): the sample
// table k_ao reads (rtc_ao_expand), the ray of a sample (rtc_ao_ray), the packing of per-pixel counts into the plane
// (rtc_ao_from_hits) and the compositing k_apply_ao does (rtc_canvas_apply_ao); rtc_ao_validate sits in host_math.cpp beside the other records the scene loader checks. Plain f64, compiled with -ffp-contract=off
// like every file of the library.
#include "rtc.h"
#include "rtc_ao.h"

#include <cmath>

extern "C" {

rtc_status rtc_ao_expand(const rtc_ao *ao, double *dirs, uint32_t *n) {
    if (!dirs || !n || rtc_ao_validate(ao) != RTC_OK) return RTC_ERR_ARG;
    for (uint32_t v = 0; v < ao->vsteps; ++v)
        for (uint32_t u = 0; u < ao->usteps; ++u) {
            const double r = std::sqrt(((double)u + 0.5) / (double)ao->usteps);
            const double phi = ((2.0 * M_PI) * ((double)v + 0.5)) / (double)ao->vsteps;
            double *d = dirs + 3u * ((size_t)v * ao->usteps + u);
            d[0] = r * std::cos(phi);
            d[1] = r * std::sin(phi);
            d[2] = std::sqrt(1.0 - r * r);
        }
    *n = ao->usteps * ao->vsteps;
    return RTC_OK;
}

rtc_status rtc_ao_ray(const double normal[3], const double over_point[3], const double local[3], double ray[6]) {
    if (!normal || !over_point || !local || !ray) return RTC_ERR_ARG;
    double t[3], s[3];
    rtc_ao_frame(normal, t, s);
    for (int c = 0; c < 3; ++c) {
        ray[c] = over_point[c];
        ray[3 + c] = rtc_ao_dir(t[c], s[c], normal[c], local[0], local[1], local[2]);
    }
    return RTC_OK;
}

rtc_status rtc_ao_from_hits(const rtc_hit *hits, const uint16_t *counts, uint32_t width, uint32_t height, uint32_t mode, uint16_t *out) {
    if (!hits || !counts || !out || mode > RTC_MODE_RENDER_ASYNC) return RTC_ERR_ARG;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            // Camera::render leaves the last row and column untouched (camera.rs:120-121): the miss value
            const bool skipped = mode == RTC_MODE_RENDER && (x + 1u >= width || y + 1u >= height);
            out[i] = (!skipped && hits[i].hit_index >= 0) ? counts[i] : (uint16_t)0;
        }
    return RTC_OK;
}

rtc_status rtc_ao_apply_check(uint32_t n_samples, double strength) {
    return (n_samples >= 1u && strength >= 0.0 && strength <= 1.0) ? RTC_OK : RTC_ERR_ARG; // (NaN fails both tests)
}

rtc_status rtc_canvas_apply_ao(double *rgb, const uint16_t *ao, uint32_t n_samples, double strength, uint32_t width, uint32_t height) {
    if (!rgb || !ao || rtc_ao_apply_check(n_samples, strength) != RTC_OK) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i) {
        const double f = rtc_ao_factor(ao[i], n_samples, strength);
        for (int c = 0; c < 3; ++c) rgb[3u * i + c] = rgb[3u * i + c] * f;
    }
    return RTC_OK;
}

} // extern "C"
