// rtc_filter.h — the rules of the edge-aware filter (include/rtc.h, "edge-aware filter") that the host statement
// (host_filter.cpp) and the device kernels (k_atrous, k_counts_to_fraction, k_apply_occlusion, rtc_filter.hip) share: a tap's
// weight, the quotient's NaN rule, the fraction of a count and the compositing product. Both files are compiled with
// -ffp-contract=off; every rule is written in the header's order. Not part of the ABI.
#ifndef RTC_FILTER_H
#define RTC_FILTER_H

#include <stdint.h>

#include "rtc.h"

#if defined(__HIPCC__)
#define RTC_FILTER_FN __host__ __device__ inline
#else
#define RTC_FILTER_FN inline
#endif

// h[k] of the B3-spline row {1, 4, 6, 4, 1} / 16, as arithmetic so that an unrolled tap loop holds a literal
RTC_FILTER_FN double rtc_filter_h(int k) { return k == 2 ? 0.375 : (k == 1 || k == 3) ? 0.25 : 0.0625; }

// The weight of tap q for pixel p, both of which hit (index >= 0) and lie in the image; `hh` = h[j]*h[i]. A result that is
// not > 0.0 (zero, negative, NaN) means: the tap is skipped.
RTC_FILTER_FN double rtc_filter_weight(double hh, double inv, uint32_t squarings, double npx, double npy, double npz, double ppx, double ppy,
                                       double ppz, double nqx, double nqy, double nqz, double pqx, double pqy, double pqz) {
    const double ex = pqx - ppx, ey = pqy - ppy, ez = pqz - ppz;
    const double d = __builtin_fabs(((npx * ex) + (npy * ey)) + (npz * ez));
    const double wz = 1.0 - d * inv;
    if (!(wz > 0.0)) return 0.0;
    double m = ((npx * nqx) + (npy * nqy)) + (npz * nqz);
    if (!(m > 0.0)) return 0.0;
    for (uint32_t k = 0; k < squarings; ++k) m = m * m;
    return (hh * wz) * m;
}

// acc / wsum; a NaN as the one quiet NaN 0x7FF8000000000000 (rtc_canvas_average's rule)
RTC_FILTER_FN double rtc_filter_quotient(double acc, double wsum) {
    const double v = acc / wsum;
    return (v != v) ? __builtin_nan("") : v;
}

RTC_FILTER_FN double rtc_filter_fraction(uint16_t count, uint32_t n) { return (double)count / (double)n; }
RTC_FILTER_FN double rtc_filter_occlude(double c, double occ, double strength) { return c * (1.0 - strength * occ); }

// RTC_OK when the compositing strength is valid: 0 <= strength <= 1 (host_filter.cpp; shared with the device entry)
extern "C" rtc_status rtc_filter_strength_check(double strength);

#endif
