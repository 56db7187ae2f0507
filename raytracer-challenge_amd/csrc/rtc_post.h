// rtc_post.h — the rules of the post-processing passes (include/rtc.h, "exposure, tone mapping and bloom") that the host
// statement (host_post.cpp) and the device kernels (rtc_post.hip) share: the luminance, a pixel's contribution to the frame
// statistics, the multiplier and white term of a frame, the three curves, the bright pass and the composite. Both files are
// compiled with -ffp-contract=off; every rule is written in the header's order. Nothing here calls exp, log or pow. Not part
// of the ABI.
#ifndef RTC_POST_H
#define RTC_POST_H

#include <stdint.h>

#include "rtc.h"

#if defined(__HIPCC__)
#define RTC_POST_FN __host__ __device__ inline
#else
#define RTC_POST_FN inline
#endif

enum { RTC_POST_BLOCK = 256 }; // values per block of the statistics' tree
// Every kernel of rtc_post.hip runs workgroups of 256 threads, and a launch holds fewer than 2^32 threads in all: at most this
// many workgroups (the entries refuse larger frames with RTC_ERR_ARG before anything is launched).
enum { RTC_POST_MAX_BLOCKS = 0xffffff };

RTC_POST_FN double rtc_post_inf() { return __builtin_inf(); }
// a NaN as the one quiet NaN 0x7FF8000000000000 (rtc_canvas_average's rule)
RTC_POST_FN double rtc_post_canon(double v) { return (v != v) ? __builtin_nan("") : v; }
RTC_POST_FN double rtc_post_luminance(double r, double g, double b) { return ((0.2126 * r) + (0.7152 * g)) + (0.0722 * b); }
// whether a luminance contributes to the statistics (NaN fails both tests)
RTC_POST_FN bool rtc_post_contributes(double y) { return y > 0.0 && y < rtc_post_inf(); }

// rtc_tonemap_resolve's arithmetic; `st` is read only with an AUTO flag
RTC_POST_FN void rtc_post_resolve(double exposure, double white, uint32_t flags, const rtc_luminance *st, double *m_out, double *inv_w2_out) {
    double m = exposure;
    if (flags & RTC_TONEMAP_AUTO_EXPOSURE) {
        const uint64_t count = st->count;
        const double mean = st->sum / (double)count;
        m = (count > 0u && mean > 0.0) ? exposure / mean : 1.0;
    }
    double lw = white;
    if (flags & RTC_TONEMAP_AUTO_WHITE) lw = st->max * m;
    *m_out = m;
    *inv_w2_out = (lw > 0.0 && lw < rtc_post_inf()) ? 1.0 / (lw * lw) : 0.0;
}

RTC_POST_FN double rtc_post_aces(double x) {
    if (!(x > 0.0)) return 0.0;
    const double a = (2.51 * x) + 0.03, b = (2.43 * x) + 0.59;
    const double o = (x * a) / ((x * b) + 0.14);
    return o > 1.0 ? 1.0 : o;
}

// one pixel of rtc_canvas_tonemap: c[] in, c[] out
RTC_POST_FN void rtc_post_tonemap_pixel(double *c, uint32_t curve, double m, double inv_w2) {
    double r = c[0] * m, g = c[1] * m, b = c[2] * m;
    if (curve == RTC_TONEMAP_REINHARD) {
        const double l = rtc_post_luminance(r, g, b);
        if (l > 0.0) {
            const double s = (1.0 + (l * inv_w2)) / (1.0 + l);
            r = r * s;
            g = g * s;
            b = b * s;
        }
    } else if (curve == RTC_TONEMAP_ACES) {
        r = rtc_post_aces(r);
        g = rtc_post_aces(g);
        b = rtc_post_aces(b);
    }
    c[0] = rtc_post_canon(r);
    c[1] = rtc_post_canon(g);
    c[2] = rtc_post_canon(b);
}

// the bright pass of one pixel: b[] = B[p] from c[] = C[p]
RTC_POST_FN void rtc_post_bright(const double *c, double threshold, double *b) {
    const double l = rtc_post_luminance(c[0], c[1], c[2]);
    if (!(l > threshold) || !(l < rtc_post_inf())) {
        b[0] = b[1] = b[2] = 0.0;
        return;
    }
    const double k = (l - threshold) / l;
    b[0] = c[0] * k;
    b[1] = c[1] * k;
    b[2] = c[2] * k;
}

RTC_POST_FN double rtc_post_composite(double c, double strength, double v) { return rtc_post_canon(c + (strength * v)); }

#endif
