// rtc_adaptive.h — the rules of edge-adaptive anti-aliasing (include/rtc.h, "edge-adaptive anti-aliasing") that the host
// statement (host_adaptive.cpp) and the device kernels (k_aa_mask, k_aa_rays, k_aa_resolve, rtc_adaptive.hip) share: the
// distance of two colours, a sample's offset, and Camera::ray_for_pixel_offset's direction restated for the device. Both
// files are compiled with -ffp-contract=off; every rule is written in the header's order. Not part of the ABI.
#ifndef RTC_ADAPTIVE_H
#define RTC_ADAPTIVE_H

#include <stdint.h>

#include "rtc.h"

#if defined(__HIPCC__)
#define RTC_AA_FN __host__ __device__ inline
#else
#define RTC_AA_FN inline
#endif

// Color::distance_from (color.rs:122-126): the differences, their squares summed left to right, an IEEE sqrt
RTC_AA_FN double rtc_aa_distance(double pr, double pg, double pb, double qr, double qg, double qb) {
    const double dr = pr - qr, dg = pg - qg, db = pb - qb;
    return __builtin_sqrt(((dr * dr) + (dg * dg)) + (db * db));
}

// the offset of cell `i` of `steps` along one axis
RTC_AA_FN double rtc_aa_offset(uint32_t i, uint32_t steps) { return ((double)i + 0.5) / (double)steps; }

// The direction of rtc_camera_ray_for_pixel(cam, x, xo, y, yo) (host_math.cpp; camera.rs:64-76), operation for operation:
// `vinv` the first three rows of cam->view_inv, `origin` that function's origin, transform_point(view_inv, (0, 0, 0)).
RTC_AA_FN void rtc_aa_direction(double half_width, double half_height, double pixel_size, const double *vinv, const double *origin,
                                uint32_t x, double xo, uint32_t y, double yo, double dir[3]) {
    const double xoffset = ((double)x + xo) * pixel_size;
    const double yoffset = ((double)y + yo) * pixel_size;
    const double world_x = half_width - xoffset;
    const double world_y = half_height - yoffset;
    double d[3];
    for (int r = 0; r < 3; ++r) {
        const double pixel = vinv[4 * r] * world_x + vinv[4 * r + 1] * world_y + vinv[4 * r + 2] * -1. + vinv[4 * r + 3];
        d[r] = pixel - origin[r];
    }
    const double mag = __builtin_sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); // vec.rs:65-76: sqrt of the sum, then three divisions
    dir[0] = d[0] / mag;
    dir[1] = d[1] / mag;
    dir[2] = d[2] / mag;
}

// the launchers of rtc_adaptive.hip and what they take: rtc_internal.h

#endif
