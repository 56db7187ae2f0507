// rtc_gather.h — the rules of include/rtc.h "colour bleeding" that the host statement (host_gather.cpp) and the device
// kernels (k_gather, k_add_scaled, rtc_kernels.hip) share: the mean of a pixel's samples, the bounce product and the
// compositing sum. Both files are compiled with -ffp-contract=off; every rule is written in the header's order. Not part of
// the ABI.
#ifndef RTC_GATHER_H
#define RTC_GATHER_H

#include <stdint.h>

#include "rtc.h"

#if defined(__HIPCC__)
#define RTC_GATHER_FN __host__ __device__ inline
#else
#define RTC_GATHER_FN inline
#endif

// A NaN as the one quiet NaN 0x7FF8000000000000 host and device agree on (rtc_canvas_average's rule)
RTC_GATHER_FN double rtc_gather_one_nan(double v) {
    return (v != v) ? __builtin_bit_cast(double, (uint64_t)0x7FF8000000000000ull) : v;
}
// radiance: the sum of a pixel's samples (from 0.0, in sample order) over their number
RTC_GATHER_FN double rtc_gather_mean(double sum, uint32_t n_samples) { return rtc_gather_one_nan(sum / (double)n_samples); }
// bounce: (base * diffuse) * radiance, with albedo = base * diffuse
RTC_GATHER_FN double rtc_gather_bounce(double albedo, double radiance) { return rtc_gather_one_nan(albedo * radiance); }
// Compositing: c + strength * p
RTC_GATHER_FN double rtc_gather_add_scaled(double c, double p, double strength) { return c + strength * p; }

// RTC_OK when the compositing strength is valid (host_gather.cpp; shared with the device entry)
extern "C" rtc_status rtc_gather_strength_check(double strength);

#endif
