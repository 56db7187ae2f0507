// rtc_post.cpp — [device] the entries of the post-processing passes (include/rtc.h, "exposure, tone mapping and bloom"):
// rtc_canvas_luminance_device, rtc_canvas_tonemap_device and rtc_canvas_bloom_device. Each checks its arguments as the host
// statement does (host_post.cpp), plus the alignment of the device pointers, and only then enqueues on the context's stream: a
// refused call launches nothing, and none waits for the stream. The kernels are rtc_post.hip's; the scratch (the statistics'
// block results, the bloom's horizontal plane) is grow-only buffers of the context.
#include <hip/hip_runtime.h>

#include "rtc.h"
#include "rtc_internal.h"
#include "rtc_post.h"

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

extern "C" {

rtc_status rtc_canvas_luminance_device(rtc_context *ctx, const void *d_rgb, uint32_t width, uint32_t height, void *d_out) {
    if (!ctx || !d_rgb || !d_out) return RTC_ERR_ARG;
    if (((size_t)d_rgb | (size_t)d_out) % sizeof(double) != 0) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    const size_t blocks = n == 0 ? 1u : (n + RTC_POST_BLOCK - 1u) / RTC_POST_BLOCK;
    if (blocks > RTC_POST_MAX_BLOCKS) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (blocks > 1u) { // level 0's results, and level 1's behind them (rtc_launch_luminance)
        const rtc_status st = ctx->d_post_lum.reserve(blocks + (blocks + RTC_POST_BLOCK - 1u) / RTC_POST_BLOCK, &ctx->render_allocs);
        if (st != RTC_OK) return st;
    }
    HIP_TRY(rtc_launch_luminance(static_cast<const double *>(d_rgb), n, ctx->d_post_lum.get(), static_cast<rtc_luminance *>(d_out), ctx->stream));
    return RTC_OK;
}

rtc_status rtc_canvas_tonemap_device(rtc_context *ctx, const void *d_in, uint32_t width, uint32_t height, const rtc_tonemap *spec,
                                     const void *d_stats, void *d_out) {
    if (!ctx || !d_in || !d_out || rtc_tonemap_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    if (spec->flags != 0u && !d_stats) return RTC_ERR_ARG;
    if (((size_t)d_in | (size_t)d_out | (size_t)d_stats) % sizeof(double) != 0) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    if (n == 0) return RTC_OK;
    if ((n + 255u) / 256u > RTC_POST_MAX_BLOCKS) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(rtc_launch_tonemap(static_cast<const double *>(d_in), static_cast<double *>(d_out), n, spec, static_cast<const rtc_luminance *>(d_stats),
                               ctx->stream));
    return RTC_OK;
}

rtc_status rtc_canvas_bloom_device(rtc_context *ctx, const void *d_in, uint32_t width, uint32_t height, const rtc_bloom *spec, void *d_out) {
    if (!ctx || !d_in || !d_out || rtc_bloom_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    if (((size_t)d_in | (size_t)d_out) % sizeof(double) != 0) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    if (n == 0) return RTC_OK;
    // k_bloom_h: one workgroup per 256-pixel segment of a row; k_bloom_v: one per 32 x 64 tile (rtc_post.hip)
    const uint64_t h_blocks = (((uint64_t)width + 255u) / 256u) * height, v_blocks = (((uint64_t)width + 31u) / 32u) * (((uint64_t)height + 63u) / 64u);
    if (h_blocks > RTC_POST_MAX_BLOCKS || v_blocks > RTC_POST_MAX_BLOCKS) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const rtc_status st = ctx->d_post_hor.reserve(3u * n, &ctx->render_allocs);
    if (st != RTC_OK) return st;
    BloomArgs a{};
    a.in = static_cast<const double *>(d_in);
    a.out = static_cast<double *>(d_out);
    a.hor = ctx->d_post_hor.get();
    a.threshold = spec->threshold;
    a.strength = spec->strength;
    (void)rtc_bloom_weights(spec, a.w); // the host's table: the device never evaluates exp
    a.width = width;
    a.height = height;
    a.radius = spec->radius;
    HIP_TRY(rtc_launch_bloom(&a, ctx->stream));
    return RTC_OK;
}

} // extern "C"
