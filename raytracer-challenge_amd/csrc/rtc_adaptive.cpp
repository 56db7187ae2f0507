// rtc_adaptive.cpp — [device] the entries of edge-adaptive anti-aliasing (include/rtc.h, "edge-adaptive anti-aliasing"):
// rtc_adaptive_mask_device, rtc_render_adaptive_device and rtc_render_adaptive. Each checks its arguments as the host
// statement does (host_adaptive.cpp), plus the alignment of the device canvas, and only then enqueues on the context's stream:
// a refused call launches nothing. The kernels are rtc_adaptive.hip's; the base frame is rtc_render_rows' launch and the
// refinement rays are traced by rtc_color_at's (rtc_color_at_device, rtc_api.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rtc.h"
#include "rtc_adaptive.h"
#include "rtc_internal.h"

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

namespace {

uint32_t tile_count(uint32_t width, uint32_t height) {
    return ((width + RTC_AA_TILE_W - 1u) / RTC_AA_TILE_W) * ((height + RTC_AA_TILE_H - 1u) / RTC_AA_TILE_H);
}

// The mask of d_rgb into d_mask and the tile counts into the context's buffer (counts, offsets, total: 2*tiles + 1 words).
rtc_status mask_pass(rtc_context *ctx, const void *d_rgb, uint32_t width, uint32_t height, uint32_t mode, double threshold, void *d_mask) {
    const rtc_status st = ctx->d_aa_tiles.reserve(2u * (size_t)tile_count(width, height) + 1u, &ctx->render_allocs);
    if (st != RTC_OK) return st;
    HIP_TRY(rtc_launch_aa_mask(static_cast<const double *>(d_rgb), width, height, mode, threshold, static_cast<unsigned char *>(d_mask),
                               ctx->d_aa_tiles.get(), ctx->stream));
    return RTC_OK;
}

} // namespace

extern "C" {

rtc_status rtc_adaptive_mask_device(rtc_context *ctx, const void *d_rgb, uint32_t width, uint32_t height, uint32_t mode, double threshold,
                                    void *d_mask) {
    if (!ctx || !d_rgb || !d_mask || mode > RTC_MODE_RENDER_ASYNC || threshold != threshold) return RTC_ERR_ARG;
    if ((size_t)d_rgb % sizeof(double) != 0 || (uint64_t)width * height > 0x7fffffffull) return RTC_ERR_ARG;
    if (width == 0u || height == 0u) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return mask_pass(ctx, d_rgb, width, height, mode, threshold, d_mask);
}

rtc_status rtc_render_adaptive_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_adaptive *spec, uint32_t mode,
                                      uint32_t flags, void *d_rgb, void *d_mask, rtc_adaptive_info *info) {
    if (!ctx || !w || !cam || !d_rgb || rtc_adaptive_validate(spec) != RTC_OK || mode > RTC_MODE_RENDER_ASYNC) return RTC_ERR_ARG;
    if (cam->hsize == 0u || cam->vsize == 0u || cam->samples != 1u) return RTC_ERR_ARG; // the base frame is the centre-sample frame
    if ((size_t)d_rgb % sizeof(double) != 0 || (uint64_t)cam->hsize * cam->vsize > 0x7fffffffull) return RTC_ERR_ARG;
    if (flags & RTC_FLAG_LDS_TABLE) return RTC_ERR_UNSUPPORTED;
    if (info) *info = rtc_adaptive_info{};
    const uint32_t W = cam->hsize, H = cam->vsize, n = spec->usteps * spec->vsteps;
    const size_t px = (size_t)W * H;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!d_mask) {
        const rtc_status ms = ctx->d_aa_mask.reserve(px, &ctx->render_allocs);
        if (ms != RTC_OK) return ms;
        d_mask = ctx->d_aa_mask.get();
    }
    rtc_status st = ctx->aa_total.ready();
    if (st != RTC_OK) return st;
    // 1. the centre-sample frame (a World of another context is refused here)
    st = rtc_render_rows(ctx, w, cam, mode, 0u, H, d_rgb, nullptr, flags);
    if (st != RTC_OK) return st;
    if (ctx->lanes > 1u) { // a pipelined context dealt the launch to a lane: the context's stream waits for it
        st = rtc_context_fence(ctx);
        if (st != RTC_OK) return st;
    }
    // 2., 3. the mask, the tile counts, their prefix sum; the total is the one thing the host has to know
    st = mask_pass(ctx, d_rgb, W, H, mode, spec->threshold, d_mask);
    if (st != RTC_OK) return st;
    const uint32_t tiles = tile_count(W, H);
    uint32_t *counts = ctx->d_aa_tiles.get(), *offsets = counts + tiles, *d_total = offsets + tiles;
    HIP_TRY(rtc_launch_aa_scan(counts, tiles, offsets, d_total, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->aa_total.get(), d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t flagged = *ctx->aa_total.get();
    if (flagged > px) return RTC_ERR_DEVICE; // (cannot happen: every tile counts its own pixels)
    const uint32_t max_rays = spec->max_rays ? spec->max_rays : RTC_AA_DEFAULT_MAX_RAYS;
    const uint32_t per_chunk = max_rays / n; // >= 1: rtc_adaptive_validate, and RTC_AA_DEFAULT_MAX_RAYS >= RTC_MAX_AA_SAMPLES
    if (info) {
        info->pixels_refined = flagged;
        info->rays_refined = (uint64_t)flagged * n;
        info->launches = (flagged + per_chunk - 1u) / per_chunk;
    }
    if (flagged == 0u) return RTC_OK;
    // 4. the list
    const size_t chunk_rays = (size_t)std::min(flagged, per_chunk) * n;
    st = ctx->d_aa_list.reserve(flagged, &ctx->render_allocs);
    if (st == RTC_OK) st = ctx->d_aa_rays.reserve(6u * chunk_rays, &ctx->render_allocs);
    if (st == RTC_OK) st = ctx->d_aa_colors.reserve(3u * chunk_rays, &ctx->render_allocs);
    if (st != RTC_OK) return st;
    HIP_TRY(rtc_launch_aa_list(static_cast<const unsigned char *>(d_mask), W, H, counts, offsets, ctx->d_aa_list.get(), ctx->stream));
    // 5. the chunks, one after the other through the same two buffers (stream order)
    AaRayArgs a{};
    a.half_width = cam->half_width;
    a.half_height = cam->half_height;
    a.pixel_size = cam->pixel_size;
    std::memcpy(a.vinv, cam->view_inv, sizeof a.vinv);
    double centre[6];
    rtc_camera_ray_for_pixel(cam, 0u, 0.5, 0u, 0.5, centre); // its origin is every ray's
    std::memcpy(a.origin, centre, sizeof a.origin);
    a.rays = ctx->d_aa_rays.get();
    a.width = W;
    a.usteps = spec->usteps;
    a.vsteps = spec->vsteps;
    for (uint32_t first = 0u; first < flagged; first += per_chunk) {
        a.list = ctx->d_aa_list.get() + first;
        a.pixels = std::min(per_chunk, flagged - first);
        HIP_TRY(rtc_launch_aa_rays(&a, ctx->stream));
        st = rtc_color_at_device(ctx, w, a.rays, a.pixels * n, RTC_MAX_REFLECTIONS, flags & RTC_FLAG_NO_CULL, ctx->d_aa_colors.get(), nullptr, true);
        if (st != RTC_OK) return st;
        HIP_TRY(rtc_launch_aa_resolve(a.list, ctx->d_aa_colors.get(), a.pixels, n, static_cast<double *>(d_rgb), ctx->stream));
    }
    return RTC_OK;
}

rtc_status rtc_render_adaptive(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_adaptive *spec, uint32_t mode, uint32_t flags,
                               double *rgb, uint8_t *mask, rtc_adaptive_info *info, rtc_stats *stats) {
    if (!ctx || !cam || !rgb || cam->hsize == 0u || cam->vsize == 0u) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)cam->hsize * cam->vsize;
    rtc_status st = ctx->d_aa_canvas.reserve(3u * px, &ctx->render_allocs);
    if (st == RTC_OK && mask) st = ctx->d_aa_mask.reserve(px, &ctx->render_allocs);
    if (st != RTC_OK) return st;
    if (stats) {
        st = rtc_stats_reset(ctx);
        if (st != RTC_OK) return st;
    }
    st = rtc_render_adaptive_device(ctx, w, cam, spec, mode, flags, ctx->d_aa_canvas.get(), mask ? ctx->d_aa_mask.get() : nullptr, info);
    if (st != RTC_OK) return st;
    if (hipMemcpyAsync(rgb, ctx->d_aa_canvas.get(), sizeof(double) * 3u * px, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = RTC_ERR_DEVICE;
    if (st == RTC_OK && mask && hipMemcpyAsync(mask, ctx->d_aa_mask.get(), px, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = RTC_ERR_DEVICE;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) st = RTC_ERR_DEVICE;
    if (st == RTC_OK && stats) st = rtc_stats_read(ctx, stats);
    return st;
}

} // extern "C"
