// host_adaptive.cpp — [host] the normative statements of edge-adaptive anti-aliasing (include/rtc.h, "edge-adaptive
// anti-aliasing"): the record's ranges (rtc_adaptive_validate), a sample's offsets (rtc_adaptive_offset) and the mask k_aa_mask
// computes (rtc_adaptive_mask). Plain f64, compiled with -ffp-contract=off like every file of the library.
#include "rtc.h"
#include "rtc_adaptive.h"

#include <cstring>

extern "C" {

rtc_status rtc_adaptive_validate(const rtc_adaptive *spec) {
    if (!spec) return RTC_ERR_ARG;
    if (spec->threshold != spec->threshold) return RTC_ERR_ARG; // NaN
    if (spec->usteps == 0u || spec->vsteps == 0u) return RTC_ERR_ARG;
    const uint64_t n = (uint64_t)spec->usteps * spec->vsteps;
    if (n > RTC_MAX_AA_SAMPLES) return RTC_ERR_ARG;
    if (spec->max_rays != 0u && spec->max_rays < n) return RTC_ERR_ARG;
    if (spec->_pad != 0u) return RTC_ERR_ARG;
    return RTC_OK;
}

rtc_status rtc_adaptive_offset(const rtc_adaptive *spec, uint32_t k, double *x_offset, double *y_offset) {
    if (!x_offset || !y_offset || rtc_adaptive_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    if (k >= spec->usteps * spec->vsteps) return RTC_ERR_ARG;
    *x_offset = rtc_aa_offset(k % spec->usteps, spec->usteps);
    *y_offset = rtc_aa_offset(k / spec->usteps, spec->vsteps);
    return RTC_OK;
}

rtc_status rtc_adaptive_mask(const double *rgb, uint32_t width, uint32_t height, uint32_t mode, double threshold, uint8_t *mask,
                             uint64_t *n_flagged) {
    if (!rgb || !mask || mode > RTC_MODE_RENDER_ASYNC || threshold != threshold) return RTC_ERR_ARG;
    if (n_flagged) *n_flagged = 0;
    const size_t px = (size_t)width * height;
    if (px == 0) return RTC_OK;
    std::memset(mask, 0, px);
    // the rendered area R: [0, rw) x [0, rh)
    const uint32_t rw = mode == RTC_MODE_RENDER ? width - 1u : width, rh = mode == RTC_MODE_RENDER ? height - 1u : height;
    uint64_t flagged = 0;
    for (uint32_t y = 0; y < rh; ++y)
        for (uint32_t x = 0; x < rw; ++x) {
            const size_t p = (size_t)y * width + x;
            const double *c = rgb + 3u * p;
            auto far = [&](size_t q) { return rtc_aa_distance(c[0], c[1], c[2], rgb[3u * q], rgb[3u * q + 1u], rgb[3u * q + 2u]) > threshold; };
            const bool flag = (x > 0u && far(p - 1u)) || (x + 1u < rw && far(p + 1u)) || (y > 0u && far(p - width)) || (y + 1u < rh && far(p + width));
            mask[p] = flag ? 1u : 0u;
            flagged += flag ? 1u : 0u;
        }
    if (n_flagged) *n_flagged = flagged;
    return RTC_OK;
}

} // extern "C"
