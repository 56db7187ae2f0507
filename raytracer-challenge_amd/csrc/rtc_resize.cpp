// rtc_resize.cpp — [device] rtc_canvas_resize_device (include/rtc.h, "resizing f64 canvases"). It checks its arguments as the
// host statement does (host_resize.cpp), plus the alignment of the device pointers, plans the launch (rtc_resize_plan, a pure
// function), finds or uploads the tables of the axes that change, and only then enqueues on the context's stream: a refused
// call launches nothing. The tables are built by rtc_resize_build_axis, the function behind rtc_resize_weights, and kept in
// the context for the last RESIZE_SLOTS (n_in, n_out, filter) triples. A hit uploads nothing and does not wait; a miss waits
// for the stream before it replaces the least recently used slot, since a kernel in flight may still read it, and again
// behind its own upload, whose source is a local vector. The kernels are rtc_resize.hip's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "rtc.h"
#include "rtc_internal.h"
#include "rtc_resize.h"

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

namespace {

// The slot that holds the table of (n_in, n_out, filter), uploaded if need be. `stamp` marks the slots of this call: a
// call's second axis never replaces its first.
rtc_status axis_table(rtc_context *ctx, uint32_t n_in, uint32_t n_out, uint32_t filter, unsigned long long stamp, rtc_context::ResizeSlot **out) {
    rtc_context::ResizeSlot *lru = nullptr;
    for (auto &s : ctx->resize_slot) {
        if (s.valid && s.n_in == n_in && s.n_out == n_out && s.filter == filter) {
            s.used = stamp;
            *out = &s;
            return RTC_OK;
        }
        if (s.used != stamp && (!lru || s.used < lru->used)) lru = &s;
    }
    ResizeAxis ax;
    const rtc_status bs = rtc_resize_build_axis(n_in, n_out, filter, &ax);
    if (bs != RTC_OK) return bs;
    std::vector<double> packed;
    try {
        packed.resize((size_t)n_out * (ax.taps + 1u));
    } catch (const std::bad_alloc &) {
        return RTC_ERR_NOMEM;
    }
    for (uint32_t o = 0; o < n_out; ++o) {
        const uint32_t fc[2] = {ax.first[o], ax.count[o]};
        std::memcpy(&packed[o], fc, sizeof fc);
    }
    std::memcpy(packed.data() + n_out, ax.w.data(), sizeof(double) * ax.w.size());
    HIP_TRY(hipStreamSynchronize(ctx->stream)); // an earlier resize may still read the slot
    lru->valid = false;
    const rtc_status rs = lru->table.reserve(packed.size(), &ctx->render_allocs);
    if (rs != RTC_OK) return rs;
    HIP_TRY(hipMemcpyAsync(lru->table.get(), packed.data(), sizeof(double) * packed.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); // `packed` goes out of scope
    lru->n_in = n_in;
    lru->n_out = n_out;
    lru->filter = filter;
    lru->taps = ax.taps;
    lru->used = stamp;
    lru->valid = true;
    ++ctx->resize_uploads;
    *out = lru;
    return RTC_OK;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

} // namespace

extern "C" {

// Test hook (not in include/rtc.h): how many axis tables this context has uploaded
rtc_status rtc_debug_resize_uploads(rtc_context *ctx, unsigned long long *out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    *out = ctx->resize_uploads;
    return RTC_OK;
}

rtc_status rtc_canvas_resize_device(rtc_context *ctx, const void *d_in, uint32_t w_in, uint32_t h_in, const rtc_resize *spec, void *d_out,
                                    uint32_t w_out, uint32_t h_out) {
    if (!ctx || !d_in || !d_out || rtc_resize_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    if (((size_t)d_in | (size_t)d_out) % sizeof(double) != 0) return RTC_ERR_ARG;
    if (w_in == 0u || h_in == 0u || w_out == 0u || h_out == 0u) return RTC_ERR_ARG;
    const size_t n_in = 3u * (size_t)w_in * h_in, n_out = 3u * (size_t)w_out * h_out;
    if (overlap(d_in, n_in * sizeof(double), d_out, n_out * sizeof(double))) return RTC_ERR_ARG;
    const ResizePlanInputs pin{w_in, h_in, w_out, h_out, spec->filter};
    ResizePlan plan;
    rtc_resize_plan(&pin, &plan);
    if (plan.status != RTC_OK) return (rtc_status)plan.status;
    HIP_TRY(hipSetDevice(ctx->device));
    const double *in = static_cast<const double *>(d_in);
    double *out = static_cast<double *>(d_out);
    if (plan.copy) {
        HIP_TRY(rtc_launch_resize_copy(in, out, n_in, ctx->stream));
        return RTC_OK;
    }
    const unsigned long long stamp = ++ctx->resize_clock;
    rtc_context::ResizeSlot *th = nullptr, *tv = nullptr;
    if (plan.h.run) {
        const rtc_status st = axis_table(ctx, w_in, w_out, spec->filter, stamp, &th);
        if (st != RTC_OK) return st;
    }
    if (plan.v.run) {
        const rtc_status st = axis_table(ctx, h_in, h_out, spec->filter, stamp, &tv);
        if (st != RTC_OK) return st;
    }
    double *mid = nullptr;
    if (plan.h.run && plan.v.run) { // (growing frees the old plane, which waits for the device)
        const rtc_status st = ctx->d_resize_mid.reserve(3u * (size_t)w_out * h_in, &ctx->render_allocs);
        if (st != RTC_OK) return st;
        mid = ctx->d_resize_mid.get();
    }
    ResizeArgs a{};
    a.w_in = w_in;
    a.h_in = h_in;
    a.w_out = w_out;
    a.h_out = h_out;
    if (plan.h.run) {
        a.in = in;
        a.out = plan.v.run ? mid : out;
        a.fc = reinterpret_cast<const uint2 *>(th->table.get());
        a.w = th->table.get() + w_out;
        HIP_TRY(rtc_launch_resize_h(&a, &plan.h, ctx->stream));
    }
    if (plan.v.run) {
        a.in = plan.h.run ? mid : in;
        a.out = out;
        a.fc = reinterpret_cast<const uint2 *>(tv->table.get());
        a.w = tv->table.get() + h_out;
        HIP_TRY(rtc_launch_resize_v(&a, &plan.v, ctx->stream));
    }
    return RTC_OK;
}

} // extern "C"
