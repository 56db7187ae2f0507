// rtc_filter.cpp — [device] the entries of the edge-aware filter (include/rtc.h, "edge-aware filter"): rtc_plane_filter_device,
// rtc_counts_to_fraction_device and rtc_canvas_apply_occlusion_device. Each checks its arguments as the host statement does
// (host_filter.cpp), plus the alignment of the device pointers, and only then enqueues on the context's stream: a refused call
// launches nothing. The kernels are rtc_filter.hip's.
#include <hip/hip_runtime.h>

#include "rtc.h"
#include "rtc_filter.h"
#include "rtc_internal.h"

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

extern "C" {

rtc_status rtc_plane_filter_device(rtc_context *ctx, const void *d_in, uint32_t channels, const rtc_aov_buffers *d_guides, uint32_t width,
                                   uint32_t height, const rtc_filter *flt, void *d_out) {
    if (!ctx || !d_in || !d_out || d_in == d_out || !d_guides || (channels != 1u && channels != 3u) || rtc_filter_validate(flt) != RTC_OK)
        return RTC_ERR_ARG;
    if (!d_guides->index || !d_guides->point || !d_guides->normal) return RTC_ERR_ARG;
    if (((size_t)d_in | (size_t)d_out | (size_t)d_guides->point | (size_t)d_guides->normal) % sizeof(double) != 0 || (size_t)d_guides->index % 4u != 0)
        return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    if (n == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (flt->passes > 1u) {
        const rtc_status st = ctx->d_filter.reserve(n * channels, &ctx->render_allocs);
        if (st != RTC_OK) return st;
    }
    AtrousArgs a{};
    a.index = d_guides->index;
    a.point = d_guides->point;
    a.normal = d_guides->normal;
    a.inv = 1.0 / flt->plane_sigma;
    a.width = width;
    a.height = height;
    a.squarings = flt->normal_squarings;
    a.src = static_cast<const double *>(d_in);
    // the last pass writes d_out, the one before it the context's plane, the one before that d_out again, ... (host_filter.cpp)
    for (uint32_t i = 0; i < flt->passes; ++i) {
        a.dst = ((flt->passes - 1u - i) % 2u == 0u) ? static_cast<double *>(d_out) : ctx->d_filter.get();
        a.step = 1u << i;
        if (rtc_launch_atrous(&a, channels, (flt->flags & RTC_FILTER_SAME_OBJECT) != 0u, ctx->stream) != hipSuccess) return RTC_ERR_DEVICE;
        a.src = a.dst;
    }
    return RTC_OK;
}

rtc_status rtc_counts_to_fraction_device(rtc_context *ctx, const void *d_counts, uint32_t n, uint32_t width, uint32_t height, void *d_out) {
    if (!ctx || !d_counts || !d_out || n == 0u) return RTC_ERR_ARG;
    if (((size_t)d_counts % 2u) != 0 || ((size_t)d_out % sizeof(double)) != 0) return RTC_ERR_ARG;
    const size_t px = (size_t)width * height;
    if (px == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(rtc_launch_counts_to_fraction(static_cast<const uint16_t *>(d_counts), px, n, static_cast<double *>(d_out), ctx->stream));
    return RTC_OK;
}

rtc_status rtc_canvas_apply_occlusion_device(rtc_context *ctx, void *d_rgb, const void *d_occ, double strength, uint32_t width, uint32_t height) {
    if (!ctx || !d_rgb || !d_occ || rtc_filter_strength_check(strength) != RTC_OK) return RTC_ERR_ARG;
    if (((size_t)d_rgb | (size_t)d_occ) % sizeof(double) != 0) return RTC_ERR_ARG;
    const size_t px = (size_t)width * height;
    if (px == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(rtc_launch_apply_occlusion(static_cast<double *>(d_rgb), static_cast<const double *>(d_occ), px, strength, ctx->stream));
    return RTC_OK;
}

} // extern "C"
