// host_gather.cpp — [host] the normative statements of the one-bounce gather pass (include/rtc.h, "colour bleeding"): the
// packing of per-sample records and colours into the radiance and bounce planes (rtc_gather_from_hits) and the compositing
// k_add_scaled does (rtc_canvas_add_scaled). The fan itself is the ambient-occlusion pass's (host_ao.cpp). Plain f64, compiled
// with -ffp-contract=off like every file of the library.
#include "rtc.h"
#include "rtc_gather.h"

#include <cmath>

extern "C" {

rtc_status rtc_gather_from_hits(const rtc_hit *hits, const rtc_hit *sample_hits, const double *sample_rgb, const double *albedo,
                                uint32_t n_samples, double radius, uint32_t width, uint32_t height, uint32_t mode,
                                const rtc_gather_buffers *out) {
    if (!hits || !sample_hits || !sample_rgb || !out || (!out->radiance && !out->bounce) || mode > RTC_MODE_RENDER_ASYNC) return RTC_ERR_ARG;
    if (out->bounce && !albedo) return RTC_ERR_ARG;
    if (n_samples == 0u || n_samples > RTC_MAX_AO_SAMPLES || !(radius > 0.)) return RTC_ERR_ARG; // (a NaN radius fails the test)
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            // Camera::render leaves the last row and column untouched (camera.rs:120-121): the miss value
            const bool skipped = mode == RTC_MODE_RENDER && (x + 1u >= width || y + 1u >= height);
            double rad[3] = {0.0, 0.0, 0.0};
            const bool hit = !skipped && hits[i].hit_index >= 0;
            if (hit) {
                double sum[3] = {0.0, 0.0, 0.0};
                for (uint32_t k = 0; k < n_samples; ++k) {
                    const size_t s = i * n_samples + k;
                    const bool counted = sample_hits[s].hit_index >= 0 && sample_hits[s].t < radius;
                    for (int c = 0; c < 3; ++c) sum[c] = sum[c] + (counted ? sample_rgb[3u * s + c] : 0.0);
                }
                for (int c = 0; c < 3; ++c) rad[c] = rtc_gather_mean(sum[c], n_samples);
            }
            for (int c = 0; c < 3; ++c) {
                if (out->radiance) out->radiance[3u * i + c] = rad[c];
                if (out->bounce) out->bounce[3u * i + c] = hit ? rtc_gather_bounce(albedo[3u * i + c], rad[c]) : 0.0;
            }
        }
    return RTC_OK;
}

rtc_status rtc_gather_strength_check(double strength) {
    return (strength >= 0.0 && strength < INFINITY) ? RTC_OK : RTC_ERR_ARG; // (NaN fails both tests)
}

rtc_status rtc_canvas_add_scaled(double *rgb, const double *plane, double strength, uint32_t width, uint32_t height) {
    if (!rgb || !plane || rtc_gather_strength_check(strength) != RTC_OK) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height * 3u;
    for (size_t i = 0; i < n; ++i) rgb[i] = rtc_gather_add_scaled(rgb[i], plane[i], strength);
    return RTC_OK;
}

} // extern "C"
