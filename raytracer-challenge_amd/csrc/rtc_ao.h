// rtc_ao.h — the ambient-occlusion rules of include/rtc.h that the host statement (host_ao.cpp) and the device kernels
// (k_ao, k_apply_ao, rtc_kernels.hip) share: the sample's direction about a normal and the compositing factor. Both files
// are compiled with -ffp-contract=off; every rule is written in the header's order. Not part of the ABI.
#ifndef RTC_AO_H
#define RTC_AO_H

#include <stdint.h>

#include "rtc.h"

#if defined(__HIPCC__)
#define RTC_AO_FN __host__ __device__ inline
#else
#define RTC_AO_FN inline
#endif

// The tangent frame (t, s) of the unit normal n: Duff et al.'s branch-free basis, in the header's order.
RTC_AO_FN void rtc_ao_frame(const double n[3], double t[3], double s[3]) {
    const double sign = __builtin_copysign(1.0, n[2]);
    const double a = -1.0 / (sign + n[2]);
    const double b = (n[0] * n[1]) * a;
    t[0] = 1.0 + ((sign * n[0]) * n[0]) * a;
    t[1] = sign * b;
    t[2] = -(sign * n[0]);
    s[0] = b;
    s[1] = sign + ((n[1] * n[1]) * a);
    s[2] = -n[1];
}
// One component of the sample's direction: ((t*l.x) + (s*l.y)) + (n*l.z)
RTC_AO_FN double rtc_ao_dir(double t, double s, double n, double lx, double ly, double lz) { return ((t * lx) + (s * ly)) + (n * lz); }
// Compositing: the factor every component of a pixel is multiplied by
RTC_AO_FN double rtc_ao_factor(uint16_t count, uint32_t n_samples, double strength) {
    return 1.0 - strength * ((double)count / (double)n_samples);
}

// RTC_OK when the compositing parameters are valid (host_ao.cpp; shared with the device entry)
extern "C" rtc_status rtc_ao_apply_check(uint32_t n_samples, double strength);

#endif
