// rtc_aov.h — the AOV view rules of include/rtc.h, written once for the host statement (host_aov.cpp) and the device
// kernel (k_aov_view, rtc_kernels.hip): what goes INTO Color::scale(c, 255), and the index palette. Both files are compiled
// with -ffp-contract=off; every rule is one or two f64 operations in the header's order. Not part of the ABI.
#ifndef RTC_AOV_H
#define RTC_AOV_H

#include <stdint.h>

#include "rtc.h"

#if defined(__HIPCC__)
#define RTC_AOV_FN __host__ __device__ inline
#else
#define RTC_AOV_FN inline
#endif

// DEPTH: (far - t) / (far - near); t = +inf gives -inf (scale: 0), t <= near gives >= 1 (scale: 255), NaN stays NaN (0)
RTC_AOV_FN double rtc_aov_depth_value(double t, double near, double far) { return (far - t) / (far - near); }
// NORMAL: (n_c + 1.0) * 0.5; a miss (0.0) is 0.5 -> 127
RTC_AOV_FN double rtc_aov_normal_value(double n) { return (n + 1.0) * 0.5; }
// SHADOW: 1.0 - (double)count / (double)n_lights (n_lights != 0)
RTC_AOV_FN double rtc_aov_shadow_value(uint16_t count, uint32_t n_lights) { return 1.0 - (double)count / (double)n_lights; }
// INDEX: black for a miss, else the low three bytes of splitmix64(index) (the function written out at rtc_camera.samples),
// each with bit 6 set so that no object is as dark as the background
RTC_AOV_FN void rtc_aov_index_rgb(int32_t index, uint8_t rgb[3]) {
    if (index < 0) {
        rgb[0] = rgb[1] = rgb[2] = 0u;
        return;
    }
    unsigned long long z = (unsigned long long)index + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    rgb[0] = (uint8_t)((z & 255u) | 0x40u);
    rgb[1] = (uint8_t)(((z >> 8) & 255u) | 0x40u);
    rgb[2] = (uint8_t)(((z >> 16) & 255u) | 0x40u);
}

// RTC_OK when `view` exists, its plane is there and its parameters are valid (host_aov.cpp; shared with the device entry)
extern "C" rtc_status rtc_aov_view_check(uint32_t view, const rtc_aov_buffers *b, double near, double far, uint32_t n_lights);

#endif
