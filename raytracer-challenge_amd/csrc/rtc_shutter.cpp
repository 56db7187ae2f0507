// rtc_shutter.cpp — [device] motion blur (include/rtc.h "Motion blur"): rtc_canvas_average_device and the rtc_shutter
// object. Everything here launches through entries the library already has — rtc_world_create_area_lights /
// rtc_world_update_area_lights for the shutter's own World, rtc_render_rows / rtc_render_lens_rows for the sub-frames —
// plus k_average_over (rtc_shutter.hip). The render kernels, the binning kernel and the world build are untouched.
//
// Ordering. Sub-frame k renders into ring canvas k % RTC_SHUTTER_RING; on a pipelined context (depth <= 4) consecutive
// sub-frames go to different lanes and, the ring being twice as long, to different canvases. When the ring is full, and
// behind the last sub-frame, one averaging pass runs on the context's stream:
//     rtc_context_fence            the stream waits for every lane's renders (no host wait);
//     k_average_over               reads the ring in sample order, carries the sum;
//     an event behind the kernel   every lane waits for it before the renders that REFILL the ring are enqueued (the next
//                                  frame's included: render_device does not wait for the host).
// On an in-order context all of it is one stream and the fence and the event are no-ops. The World updates between the
// sub-frames order themselves (rtc_world_update: ordered like a launch); their one host wait, for the build header, stays.
// The render kernels write every pixel of the rows they are given — pixels they prove black (RTC_MODE_RENDER's last row and
// column, the sky tile rows) are stored as zeros, which is what lets rtc_render reuse its canvas — so a ring canvas
// needs no clearing before it is reused.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "rtc.h"
#include "rtc_internal.h"

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

constexpr uint32_t RING = RTC_SHUTTER_RING;
static_assert(RING >= 2u * rtc_context::MAX_LANES, "consecutive sub-frames of a pipelined context need distinct ring canvases");

// Color::average_over of n frames `stride` doubles apart, RING per pass, the sum carried in d_out.
rtc_status average_passes(rtc_context *ctx, const double *d_frames, uint32_t n, size_t stride, size_t count, double *d_out) {
    for (uint32_t done = 0; done < n; done += RING) {
        AverageArgs a{};
        a.frames = d_frames + (size_t)done * stride;
        a.nf = n - done < RING ? n - done : RING;
        a.sum_in = done ? d_out : nullptr;
        a.f64_out = d_out;
        a.stride = stride;
        a.count = count;
        a.divisor = done + a.nf == n ? static_cast<double>(n) : 0.0;
        HIP_TRY(rtc_launch_average_over(&a, ctx->stream));
    }
    return RTC_OK;
}

} // namespace

struct rtc_shutter {
    rtc_context *ctx = nullptr;
    rtc_world *world = nullptr;      // the shutter's own: created by the first frame, updated ever after
    DevBuf<double> ring, sum;        // min(samples, RING) canvases `stride` doubles apart; the carried sum and the host entries' mean
    DevBuf<unsigned char> bytes;     // the host entries' 8-bit frame
    hipEvent_t averaged = nullptr;   // behind the latest averaging pass: the lanes wait for it before they refill the ring
    std::vector<rtc_shape> shapes;   // sub-frame k's shapes
};

extern "C" {

rtc_status rtc_canvas_average_device(rtc_context *ctx, const void *d_frames, uint32_t n, size_t count, void *d_out) {
    if (!ctx || !d_frames || !d_out || n == 0u || n > RTC_MAX_SHUTTER_SAMPLES) return RTC_ERR_ARG;
    if (((size_t)d_frames % sizeof(double)) != 0u || ((size_t)d_out % sizeof(double)) != 0u) return RTC_ERR_ARG;
    if (count == 0u) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return average_passes(ctx, static_cast<const double *>(d_frames), n, count, count, static_cast<double *>(d_out));
}

rtc_status rtc_shutter_create(rtc_context *ctx, rtc_shutter **out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    *out = nullptr;
    rtc_shutter *s = new (std::nothrow) rtc_shutter;
    if (!s) return RTC_ERR_NOMEM;
    s->ctx = ctx;
    *out = s;
    return RTC_OK;
}

void rtc_shutter_destroy(rtc_shutter *s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)rtc_context_synchronize(s->ctx); // nothing may still read the scratch
    if (s->world) rtc_world_destroy(s->world);
    if (s->averaged) (void)hipEventDestroy(s->averaged);
    delete s;
}

} // extern "C"

namespace {

// The ring's averaging pass over sub-frames [first, first + nf) of `n`, ordered behind their renders; `fin` (the last
// pass): where the outputs go.
struct Outputs {
    double *f64 = nullptr;
    unsigned char *rgb8 = nullptr, *rgba8 = nullptr;
    const DevGamma *g = nullptr;
};

rtc_status ring_pass(rtc_shutter *s, uint32_t first, uint32_t nf, uint32_t n, size_t stride, size_t count, const Outputs *fin) {
    rtc_context *ctx = s->ctx;
    const rtc_status fs = rtc_context_fence(ctx);
    if (fs != RTC_OK) return fs;
    AverageArgs a{};
    a.frames = s->ring.get();
    a.nf = nf;
    a.sum_in = first ? s->sum.get() : nullptr;
    a.stride = stride;
    a.count = count;
    if (fin) {
        a.divisor = static_cast<double>(n);
        a.f64_out = fin->f64;
        a.rgb8 = fin->rgb8;
        a.rgba8 = fin->rgba8;
        a.g = fin->g;
    } else {
        a.f64_out = s->sum.get();
    }
    HIP_TRY(rtc_launch_average_over(&a, ctx->stream));
    if (ctx->lanes > 1u) { // the renders that refill the ring — this frame's or the next one's — run on the lanes: behind this pass
        if (!s->averaged) HIP_TRY(hipEventCreateWithFlags(&s->averaged, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s->averaged, ctx->stream));
        for (uint32_t l = 0; l < rtc_context::MAX_LANES; ++l)
            if (ctx->lane[l]) HIP_TRY(hipStreamWaitEvent(ctx->lane[l], s->averaged, 0));
    }
    return RTC_OK;
}

// Everything the four entries share. Host outputs (h_*) go through the shutter's scratch and are copied out; device
// outputs are written by the last pass directly.
rtc_status shutter_frame(rtc_shutter *s, const rtc_shutter_scene *sc, uint32_t mode, uint32_t flags, float gamma, void *d_rgb, void *d_rgb8,
                         void *d_rgba8, double *h_rgb, uint8_t *h_rgb8, uint8_t *h_rgba8, rtc_stats *stats) {
    if (!s || !sc || !sc->cam_open || !sc->lights || (sc->n_shapes && !sc->shapes)) return RTC_ERR_ARG;
    if (!d_rgb && !d_rgb8 && !d_rgba8 && !h_rgb && !h_rgb8 && !h_rgba8) return RTC_ERR_ARG;
    rtc_context *ctx = s->ctx;
    const uint32_t n = sc->samples;
    const rtc_camera &c0 = *sc->cam_open;
    const bool want_rgba = d_rgba8 || h_rgba8;
    // ---- the whole frame is validated before anything is launched
    if (n == 0u || n > RTC_MAX_SHUTTER_SAMPLES || mode > RTC_MODE_RENDER_ASYNC) return RTC_ERR_ARG;
    if (c0.hsize == 0u || c0.vsize == 0u || c0.samples > 255u) return RTC_ERR_ARG;
    if (want_rgba && !(gamma > 0.f && gamma <= 3.402823466e+38f)) return RTC_ERR_ARG; // positive and finite
    if (d_rgb && ((size_t)d_rgb % sizeof(double)) != 0u) return RTC_ERR_ARG;
    if (sc->lens && (rtc_lens_validate(sc->lens) != RTC_OK || c0.samples != 1u)) return RTC_ERR_ARG;
    rtc_camera cam;
    rtc_status st = rtc_shutter_camera(sc->cam_open, sc->cam_close, n, 0u, &cam);
    if (st != RTC_OK) return st;
    st = rtc_shutter_check_motions(sc->motions, sc->n_motions, sc->n_shapes, n);
    if (st != RTC_OK) return st;
    HIP_TRY(hipSetDevice(ctx->device));
    // ---- scratch: grow-only, bounded by RING canvases + the sum + the bytes
    const size_t px = (size_t)c0.hsize * c0.vsize, count = 3u * px, stride = count + (count & 1u); // every ring canvas on 16 bytes
    const bool host_out = h_rgb || h_rgb8 || h_rgba8;
    const size_t ring_need = stride * (n < RING ? n : RING), sum_need = (n > RING || h_rgb) ? count : 0u;
    const size_t bytes_need = h_rgba8 ? px * 4u : h_rgb8 ? px * 3u : 0u;
    if (ring_need > s->ring.capacity() || sum_need > s->sum.capacity() || bytes_need > s->bytes.capacity())
        HIP_TRY(hipDeviceSynchronize()); // growing frees what an earlier frame's work (render_device does not wait) may still use
    st = s->ring.reserve(ring_need);
    if (st == RTC_OK) st = s->sum.reserve(sum_need);
    if (st == RTC_OK) st = s->bytes.reserve(bytes_need);
    if (st != RTC_OK) return st;
    Outputs fin;
    fin.f64 = h_rgb ? s->sum.get() : static_cast<double *>(d_rgb);
    fin.rgb8 = h_rgb8 ? s->bytes.get() : static_cast<unsigned char *>(d_rgb8);
    fin.rgba8 = h_rgba8 ? s->bytes.get() : static_cast<unsigned char *>(d_rgba8);
    if (want_rgba) {
        st = rtc_gamma_table_on_stream(ctx, gamma, &fin.g);
        if (st != RTC_OK) return st;
    }
    if (stats) {
        st = rtc_stats_reset(ctx);
        if (st != RTC_OK) return st;
    }
    // ---- the sub-frames, back to back
    s->shapes.resize(sc->n_shapes ? sc->n_shapes : 1u);
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t slot = k % RING;
        if (k && slot == 0u) { // the ring is full: fold it into the sum before it is refilled
            st = ring_pass(s, k - RING, RING, n, stride, count, nullptr);
            if (st != RTC_OK) return st;
        }
        if (k == 0u || sc->n_motions) { // a World without moving shapes is the same in every sub-frame
            st = rtc_shutter_shapes(sc->shapes, sc->n_shapes, sc->motions, sc->n_motions, n, k, s->shapes.data());
            if (st != RTC_OK) return st;
            if (!s->world) st = rtc_world_create_area_lights(ctx, s->shapes.data(), sc->n_shapes, sc->lights, sc->n_lights, &s->world);
            else st = rtc_world_update_area_lights(ctx, s->world, s->shapes.data(), sc->n_shapes, sc->lights, sc->n_lights);
            if (st != RTC_OK) return st;
        }
        st = rtc_shutter_camera(sc->cam_open, sc->cam_close, n, k, &cam);
        if (st != RTC_OK) return st;
        double *canvas = s->ring.get() + (size_t)slot * stride;
        st = sc->lens ? rtc_render_lens_rows(ctx, s->world, &cam, sc->lens, mode, 0u, cam.vsize, canvas, nullptr, flags)
                      : rtc_render_rows(ctx, s->world, &cam, mode, 0u, cam.vsize, canvas, nullptr, flags);
        if (st != RTC_OK) return st;
    }
    const uint32_t first = ((n - 1u) / RING) * RING;
    st = ring_pass(s, first, n - first, n, stride, count, &fin);
    if (st != RTC_OK) return st;
    if (!host_out) return RTC_OK;
    if (h_rgb) HIP_TRY(hipMemcpyAsync(h_rgb, s->sum.get(), count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (h_rgb8) HIP_TRY(hipMemcpyAsync(h_rgb8, s->bytes.get(), px * 3u, hipMemcpyDeviceToHost, ctx->stream));
    if (h_rgba8) HIP_TRY(hipMemcpyAsync(h_rgba8, s->bytes.get(), px * 4u, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return stats ? rtc_stats_read(ctx, stats) : RTC_OK;
}

} // namespace

extern "C" {

rtc_status rtc_shutter_render(rtc_shutter *s, const rtc_shutter_scene *scene, uint32_t mode, uint32_t flags, double *rgb, rtc_stats *stats) {
    if (!rgb) return RTC_ERR_ARG;
    return shutter_frame(s, scene, mode, flags, 0.f, nullptr, nullptr, nullptr, rgb, nullptr, nullptr, stats);
}

rtc_status rtc_shutter_render_rgb8(rtc_shutter *s, const rtc_shutter_scene *scene, uint32_t mode, uint32_t flags, uint8_t *rgb8,
                                   rtc_stats *stats) {
    if (!rgb8) return RTC_ERR_ARG;
    return shutter_frame(s, scene, mode, flags, 0.f, nullptr, nullptr, nullptr, nullptr, rgb8, nullptr, stats);
}

rtc_status rtc_shutter_render_rgba8(rtc_shutter *s, const rtc_shutter_scene *scene, uint32_t mode, uint32_t flags, float gamma,
                                    uint8_t *rgba8, rtc_stats *stats) {
    if (!rgba8) return RTC_ERR_ARG;
    return shutter_frame(s, scene, mode, flags, gamma, nullptr, nullptr, nullptr, nullptr, nullptr, rgba8, stats);
}

rtc_status rtc_shutter_render_device(rtc_shutter *s, const rtc_shutter_scene *scene, uint32_t mode, uint32_t flags, float gamma, void *d_rgb,
                                     void *d_rgb8, void *d_rgba8) {
    if (!d_rgb && !d_rgb8 && !d_rgba8) return RTC_ERR_ARG;
    return shutter_frame(s, scene, mode, flags, gamma, d_rgb, d_rgb8, d_rgba8, nullptr, nullptr, nullptr, nullptr);
}

} // extern "C"
