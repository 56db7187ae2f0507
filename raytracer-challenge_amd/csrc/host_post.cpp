// host_post.cpp — [host] the normative statements of the post-processing passes (include/rtc.h, "exposure, tone mapping and
// bloom"): the frame statistics with their fixed tree order (rtc_canvas_luminance), the records' ranges, the multiplier and
// white term (rtc_tonemap_resolve), the tone map, the bloom's weight table (the only place exp is called) and the bloom
// itself. Plain f64, compiled with -ffp-contract=off like every file of the library; the per-pixel rules are rtc_post.h's,
// which the kernels of rtc_post.hip evaluate too.
#include "rtc.h"
#include "rtc_post.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace {

// v[0 .. 256) -> v[0], the header's tree
double tree(double *v) {
    for (uint32_t s = RTC_POST_BLOCK / 2u; s >= 1u; s /= 2u)
        for (uint32_t i = 0; i < s; ++i) v[i] = v[i] + v[i + s];
    return v[0];
}

bool finite_ge0(double v) { return v >= 0.0 && v < rtc_post_inf(); } // (NaN fails the first test)

} // namespace

extern "C" {

rtc_status rtc_canvas_luminance(const double *rgb, uint32_t width, uint32_t height, rtc_luminance *out) {
    if (!rgb || !out) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    const size_t blocks = n == 0 ? 1u : (n + RTC_POST_BLOCK - 1u) / RTC_POST_BLOCK;
    std::vector<double> level;
    try {
        level.resize(blocks);
    } catch (const std::bad_alloc &) {
        return RTC_ERR_NOMEM;
    }
    double v[RTC_POST_BLOCK], mx = 0.0;
    uint64_t count = 0;
    for (size_t b = 0; b < blocks; ++b) {
        for (uint32_t i = 0; i < RTC_POST_BLOCK; ++i) {
            const size_t p = b * RTC_POST_BLOCK + i;
            v[i] = 0.0;
            if (p >= n) continue;
            const double y = rtc_post_luminance(rgb[3u * p], rgb[3u * p + 1u], rgb[3u * p + 2u]);
            if (!rtc_post_contributes(y)) continue;
            v[i] = y;
            ++count;
            if (y > mx) mx = y;
        }
        level[b] = tree(v);
    }
    size_t len = blocks;
    while (len > 1u) { // the block results, reduced the same way (in place: block b is read before level[b] is written)
        const size_t next = (len + RTC_POST_BLOCK - 1u) / RTC_POST_BLOCK;
        for (size_t b = 0; b < next; ++b) {
            for (uint32_t i = 0; i < RTC_POST_BLOCK; ++i) {
                const size_t p = b * RTC_POST_BLOCK + i;
                v[i] = p < len ? level[p] : 0.0;
            }
            level[b] = tree(v);
        }
        len = next;
    }
    out->max = mx;
    out->sum = level[0];
    out->count = count;
    return RTC_OK;
}

rtc_status rtc_tonemap_validate(const rtc_tonemap *spec) {
    if (!spec) return RTC_ERR_ARG;
    if (!(spec->exposure > 0.0 && spec->exposure < rtc_post_inf())) return RTC_ERR_ARG; // (NaN fails the test)
    if (!(spec->white > 0.0)) return RTC_ERR_ARG;
    if (spec->curve > RTC_TONEMAP_ACES) return RTC_ERR_ARG;
    if ((spec->flags & ~(uint32_t)(RTC_TONEMAP_AUTO_EXPOSURE | RTC_TONEMAP_AUTO_WHITE)) != 0u) return RTC_ERR_ARG;
    return RTC_OK;
}

rtc_status rtc_tonemap_resolve(const rtc_tonemap *spec, const rtc_luminance *stats, double *m, double *inv_w2) {
    if (!m || !inv_w2 || rtc_tonemap_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    if (spec->flags != 0u && !stats) return RTC_ERR_ARG;
    rtc_post_resolve(spec->exposure, spec->white, spec->flags, stats, m, inv_w2);
    return RTC_OK;
}

rtc_status rtc_canvas_tonemap(const double *in, uint32_t width, uint32_t height, const rtc_tonemap *spec, const rtc_luminance *stats,
                              double *out) {
    if (!in || !out) return RTC_ERR_ARG;
    double m = 0.0, inv_w2 = 0.0;
    const rtc_status st = rtc_tonemap_resolve(spec, stats, &m, &inv_w2);
    if (st != RTC_OK) return st;
    const size_t n = (size_t)width * height;
    for (size_t p = 0; p < n; ++p) {
        double c[3] = {in[3u * p], in[3u * p + 1u], in[3u * p + 2u]};
        rtc_post_tonemap_pixel(c, spec->curve, m, inv_w2);
        out[3u * p] = c[0];
        out[3u * p + 1u] = c[1];
        out[3u * p + 2u] = c[2];
    }
    return RTC_OK;
}

rtc_status rtc_bloom_validate(const rtc_bloom *spec) {
    if (!spec) return RTC_ERR_ARG;
    if (!finite_ge0(spec->threshold) || !finite_ge0(spec->strength)) return RTC_ERR_ARG;
    if (!(spec->sigma > 0.0 && spec->sigma < rtc_post_inf()) || !((2.0 * spec->sigma) * spec->sigma > 0.0)) return RTC_ERR_ARG;
    if (spec->radius < 1u || spec->radius > RTC_MAX_BLOOM_RADIUS || spec->_pad != 0u) return RTC_ERR_ARG;
    return RTC_OK;
}

rtc_status rtc_bloom_weights(const rtc_bloom *spec, double *w) {
    if (!w || rtc_bloom_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    const int r = (int)spec->radius;
    const double sigma = spec->sigma;
    double sum = 0.0;
    for (int k = -r; k <= r; ++k) {
        w[k + r] = std::exp(-((double)(k * k)) / ((2.0 * sigma) * sigma));
        sum = sum + w[k + r];
    }
    for (int k = 0; k <= 2 * r; ++k) w[k] = w[k] / sum;
    return RTC_OK;
}

rtc_status rtc_canvas_bloom(const double *in, uint32_t width, uint32_t height, const rtc_bloom *spec, double *out) {
    if (!in || !out || rtc_bloom_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    if (n == 0) return RTC_OK;
    double w[2u * RTC_MAX_BLOOM_RADIUS + 1u];
    (void)rtc_bloom_weights(spec, w);
    std::vector<double> bright, hor;
    try {
        bright.resize(3u * n);
        hor.resize(3u * n);
    } catch (const std::bad_alloc &) {
        return RTC_ERR_NOMEM;
    }
    for (size_t p = 0; p < n; ++p) rtc_post_bright(in + 3u * p, spec->threshold, bright.data() + 3u * p);
    const int64_t r = spec->radius;
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int64_t k = -r; k <= r; ++k) {
                const int64_t qx = (int64_t)x + k;
                if (qx < 0 || qx >= (int64_t)width) continue; // a tap of +0.0
                const double *b = bright.data() + 3u * ((size_t)y * width + (size_t)qx);
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (w[k + r] * b[c]);
            }
            std::memcpy(hor.data() + 3u * ((size_t)y * width + x), acc, sizeof acc);
        }
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int64_t k = -r; k <= r; ++k) {
                const int64_t qy = (int64_t)y + k;
                if (qy < 0 || qy >= (int64_t)height) continue;
                const double *h = hor.data() + 3u * ((size_t)qy * width + x);
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (w[k + r] * h[c]);
            }
            const size_t p = (size_t)y * width + x;
            for (int c = 0; c < 3; ++c) out[3u * p + c] = rtc_post_composite(in[3u * p + c], spec->strength, acc[c]);
        }
    return RTC_OK;
}

} // extern "C"
