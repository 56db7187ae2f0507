// host_aov.cpp — [host] the normative statements of the AOV planes (include/rtc.h, "arbitrary output variables"):
// rtc_aov_from_hits packs per-pixel hit records into the image planes k_aov writes, rtc_aov_view_rgb8 turns one plane into
// the 8-bit picture k_aov_view writes. Plain f64, compiled with -ffp-contract=off like every file of the library.
#include "rtc.h"
#include "rtc_aov.h"

#include <cmath>
#include <limits>

extern "C" {

rtc_status rtc_aov_from_hits(const rtc_hit *hits, const uint16_t *shadow_counts, uint32_t width, uint32_t height, uint32_t mode,
                             const rtc_aov_buffers *out) {
    if (!hits || !out || mode > RTC_MODE_RENDER_ASYNC) return RTC_ERR_ARG;
    if (!out->index && !out->depth && !out->point && !out->normal && !out->flags && !out->shadow) return RTC_ERR_ARG;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const rtc_hit &h = hits[i];
            // Camera::render leaves the last row and column untouched (camera.rs:120-121): the miss values
            const bool skipped = mode == RTC_MODE_RENDER && (x + 1u >= width || y + 1u >= height);
            const bool hit = !skipped && h.hit_index >= 0;
            if (out->index) out->index[i] = hit ? h.hit_index : -1;
            if (out->depth) out->depth[i] = hit ? h.t : std::numeric_limits<double>::infinity();
            for (int k = 0; k < 3; ++k) {
                if (out->point) out->point[3u * i + k] = hit ? h.point[k] : 0.0;
                if (out->normal) out->normal[3u * i + k] = hit ? h.normal[k] : 0.0;
            }
            if (out->flags) out->flags[i] = hit ? (uint8_t)(1u | ((h.inside ? 1u : 0u) << 1)) : (uint8_t)0;
            if (out->shadow) out->shadow[i] = hit ? (shadow_counts ? shadow_counts[i] : (uint16_t)h.shadowed) : (uint16_t)0;
        }
    return RTC_OK;
}

rtc_status rtc_aov_view_check(uint32_t view, const rtc_aov_buffers *b, double near, double far, uint32_t n_lights) {
    if (!b) return RTC_ERR_ARG;
    switch (view) {
    case RTC_AOV_VIEW_DEPTH:
        return (b->depth && std::isfinite(near) && std::isfinite(far) && far > near) ? RTC_OK : RTC_ERR_ARG;
    case RTC_AOV_VIEW_NORMAL: return b->normal ? RTC_OK : RTC_ERR_ARG;
    case RTC_AOV_VIEW_INDEX: return b->index ? RTC_OK : RTC_ERR_ARG;
    case RTC_AOV_VIEW_SHADOW: return (b->shadow && n_lights != 0u) ? RTC_OK : RTC_ERR_ARG;
    default: return RTC_ERR_ARG;
    }
}

rtc_status rtc_aov_view_rgb8(uint32_t view, const rtc_aov_buffers *b, uint32_t width, uint32_t height, double near, double far,
                             uint32_t n_lights, uint8_t *rgb8) {
    const rtc_status st = rtc_aov_view_check(view, b, near, far, n_lights);
    if (st != RTC_OK) return st;
    if (!rgb8) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    for (size_t i = 0; i < n; ++i) {
        double c[3];
        uint8_t *o = rgb8 + 3u * i;
        if (view == RTC_AOV_VIEW_INDEX) {
            rtc_aov_index_rgb(b->index[i], o);
            continue;
        }
        if (view == RTC_AOV_VIEW_DEPTH) c[0] = c[1] = c[2] = rtc_aov_depth_value(b->depth[i], near, far);
        else if (view == RTC_AOV_VIEW_SHADOW) c[0] = c[1] = c[2] = rtc_aov_shadow_value(b->shadow[i], n_lights);
        else
            for (int k = 0; k < 3; ++k) c[k] = rtc_aov_normal_value(b->normal[3u * i + k]);
        rtc_color_scale255(c, 3, o);
    }
    return RTC_OK;
}

} // extern "C"
