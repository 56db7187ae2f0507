// host_filter.cpp — [host] the normative statements of the edge-aware filter (include/rtc.h, "edge-aware filter"): the record's
// ranges (rtc_filter_validate), the à-trous passes k_atrous runs (rtc_plane_filter), the fraction of a count plane
// (rtc_counts_to_fraction) and the compositing k_apply_occlusion does (rtc_canvas_apply_occlusion). Plain f64, compiled with
// -ffp-contract=off like every file of the library.
#include "rtc.h"
#include "rtc_filter.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace {

// One pass: A_i = `src` to A_{i+1} = `dst` with taps `s` pixels apart.
template <uint32_t CH>
void pass(const double *src, double *dst, const int32_t *index, const double *point, const double *normal, uint32_t width, uint32_t height,
          uint32_t s, double inv, uint32_t squarings, bool same) {
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            const int32_t ip = index[p];
            double acc[CH], wsum = 0.0;
            for (uint32_t c = 0; c < CH; ++c) acc[c] = 0.0;
            if (ip >= 0) {
                const double *np = normal + 3u * p, *pp = point + 3u * p;
                for (int j = 0; j < 5; ++j) {
                    const int64_t qy = (int64_t)y + (int64_t)(j - 2) * (int64_t)s;
                    if (qy < 0 || qy >= (int64_t)height) continue;
                    for (int i = 0; i < 5; ++i) {
                        const int64_t qx = (int64_t)x + (int64_t)(i - 2) * (int64_t)s;
                        if (qx < 0 || qx >= (int64_t)width) continue;
                        const size_t q = (size_t)qy * width + (size_t)qx;
                        const int32_t iq = index[q];
                        if (iq < 0 || (same && iq != ip)) continue;
                        const double *nq = normal + 3u * q, *pq = point + 3u * q;
                        const double w = rtc_filter_weight(rtc_filter_h(j) * rtc_filter_h(i), inv, squarings, np[0], np[1], np[2], pp[0], pp[1], pp[2],
                                                           nq[0], nq[1], nq[2], pq[0], pq[1], pq[2]);
                        if (!(w > 0.0)) continue;
                        for (uint32_t c = 0; c < CH; ++c) acc[c] = acc[c] + w * src[CH * q + c];
                        wsum = wsum + w;
                    }
                }
            }
            if (wsum > 0.0)
                for (uint32_t c = 0; c < CH; ++c) dst[CH * p + c] = rtc_filter_quotient(acc[c], wsum);
            else
                std::memcpy(dst + CH * p, src + CH * p, sizeof(double) * CH); // a miss, or no tap survived: bit for bit
        }
}

} // namespace

extern "C" {

rtc_status rtc_filter_validate(const rtc_filter *flt) {
    if (!flt) return RTC_ERR_ARG;
    if (!(flt->plane_sigma > 0.0)) return RTC_ERR_ARG; // (NaN fails the test)
    if (flt->passes < 1u || flt->passes > RTC_MAX_FILTER_PASSES || flt->normal_squarings > 8u) return RTC_ERR_ARG;
    if ((flt->flags & ~(uint32_t)RTC_FILTER_SAME_OBJECT) != 0u || flt->_pad != 0u) return RTC_ERR_ARG;
    return RTC_OK;
}

rtc_status rtc_plane_filter(const double *in, uint32_t channels, const rtc_aov_buffers *guides, uint32_t width, uint32_t height,
                            const rtc_filter *flt, double *out) {
    if (!in || !out || in == out || !guides || (channels != 1u && channels != 3u) || rtc_filter_validate(flt) != RTC_OK) return RTC_ERR_ARG;
    if (!guides->index || !guides->point || !guides->normal) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    if (n == 0) return RTC_OK;
    std::vector<double> scratch;
    if (flt->passes > 1u) {
        try {
            scratch.resize(n * channels);
        } catch (const std::bad_alloc &) {
            return RTC_ERR_NOMEM;
        }
    }
    const double inv = 1.0 / flt->plane_sigma;
    const bool same = (flt->flags & RTC_FILTER_SAME_OBJECT) != 0u;
    // the last pass writes `out`, the one before it the scratch plane, the one before that `out` again, ...
    const double *src = in;
    for (uint32_t i = 0; i < flt->passes; ++i) {
        double *dst = ((flt->passes - 1u - i) % 2u == 0u) ? out : scratch.data();
        if (channels == 1u) pass<1>(src, dst, guides->index, guides->point, guides->normal, width, height, 1u << i, inv, flt->normal_squarings, same);
        else pass<3>(src, dst, guides->index, guides->point, guides->normal, width, height, 1u << i, inv, flt->normal_squarings, same);
        src = dst;
    }
    return RTC_OK;
}

rtc_status rtc_counts_to_fraction(const uint16_t *counts, uint32_t n, uint32_t width, uint32_t height, double *out) {
    if (!counts || !out || n == 0u) return RTC_ERR_ARG;
    const size_t px = (size_t)width * height;
    for (size_t i = 0; i < px; ++i) out[i] = rtc_filter_fraction(counts[i], n);
    return RTC_OK;
}

rtc_status rtc_filter_strength_check(double strength) {
    return (strength >= 0.0 && strength <= 1.0) ? RTC_OK : RTC_ERR_ARG; // (NaN fails both tests)
}

rtc_status rtc_canvas_apply_occlusion(double *rgb, const double *occ, double strength, uint32_t width, uint32_t height) {
    if (!rgb || !occ || rtc_filter_strength_check(strength) != RTC_OK) return RTC_ERR_ARG;
    const size_t px = (size_t)width * height;
    for (size_t i = 0; i < px; ++i) {
        const double o = occ[i];
        for (int c = 0; c < 3; ++c) rgb[3u * i + c] = rtc_filter_occlude(rgb[3u * i + c], o, strength);
    }
    return RTC_OK;
}

} // extern "C"
