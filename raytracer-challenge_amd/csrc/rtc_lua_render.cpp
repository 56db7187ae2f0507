// rtc_lua_render.cpp — [device] render_lua (lua.rs:50-91) for a program rtc_lua_run has interpreted: the one lane loop
// behind rtc_lua_program_render and its encoded variants (_gif, _files, _png, _saved).
//
// Every job is one render launch. The launches go through the context's lanes (pipeline depth 3 unless the caller chose
// one) — the shape of the reference's AddFrame loop, one camera per call — and each is followed on its own lane by what
// its output needs: the copy of its rows into a page-locked host buffer, or a file's chain (rtc_encode.h) and the copy of
// the body's 8-byte length. Outputs are handed to the callback in job order while later frames are still being rendered;
// an encoded body crosses PCIe at delivery, exactly its length, on a copy stream of the call.
#include <hip/hip_runtime.h>

#include <cctype>
#include <cstring>
#include <vector>

#include "rtc.h"
#include "rtc_encode.h"
#include "rtc_float.h"
#include "rtc_image.h"
#include "rtc_internal.h"

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

enum class Entry { ROWS, GIF, FILES, PNG, SAVED };

bool ends_with(const char *name, const char *ext) { // any case, as the `image` crate matches extensions
    if (!name) return false;
    const size_t n = std::strlen(name), k = std::strlen(ext);
    if (n < k) return false;
    for (size_t i = 0; i < k; ++i)
        if (std::tolower((unsigned char)name[n - k + i]) != ext[i]) return false;
    return true;
}

// What a job delivers: `format` (RTC_LUA_OUT_*) and either an encoded file (`job`) or the rows, copied behind the render
// (a saved PPM's rows are printed at delivery). `f64`: the job renders its f64 canvas, not 8-bit rows (a float file).
struct Output {
    uint32_t format = RTC_LUA_OUT_RGB8;
    bool encoded = false;
    RtcEncodeJob job;
    bool f64 = false;
};

rtc_status choose(Entry entry, const rtc_lua_job &job, int32_t quality, Output *out) {
    const bool add_frame = job.kind == RTC_LUA_JOB_ADD_FRAME;
    *out = Output{};
    switch (entry) {
    case Entry::ROWS: break;
    case Entry::GIF:
    case Entry::FILES:
        if (add_frame) *out = {RTC_LUA_OUT_GIF_RECORD, true, {RtcEncodeJob::GIF_RECORD}};
        else if (entry == Entry::FILES && (ends_with(job.outfile, ".jpg") || ends_with(job.outfile, ".jpeg")))
            *out = {RTC_LUA_OUT_JPEG, true, {RtcEncodeJob::JPEG, quality}};
        break;
    case Entry::PNG: // render_to_files' files: a PNG for everything but a .ppm name
        if (add_frame || !ends_with(job.outfile, ".ppm")) *out = {RTC_LUA_OUT_PNG, true, {RtcEncodeJob::PNG}};
        break;
    case Entry::SAVED: {
        if (add_frame) {
            *out = {RTC_LUA_OUT_GIF_RECORD, true, {RtcEncodeJob::GIF_RECORD}};
            break;
        }
        uint32_t f = 0;
        if (rtc_float_format_for_name(job.outfile, &f) == RTC_OK) { // the float table first
            *out = {RTC_LUA_OUT_FILE, true, {RtcEncodeJob::FLOAT, 0, f}, true};
            break;
        }
        const rtc_status st = rtc_image_format_for_name(job.outfile, &f);
        if (st != RTC_OK) return st;
        *out = {RTC_LUA_OUT_FILE, f != RTC_IMAGE_PPM, {RtcEncodeJob::SAVED, 0, f}};
        break;
    }
    }
    return RTC_OK;
}

// The saved entry's check of every name and size before the first launch: an unsupported one renders nothing.
rtc_status check_saved(const rtc_lua_program *prog) {
    for (uint32_t i = 0, n = rtc_lua_program_jobs(prog); i < n; ++i) {
        rtc_lua_job job;
        const rtc_status js = rtc_lua_program_job(prog, i, &job);
        if (js != RTC_OK) return js;
        uint32_t f = 0;
        if (job.kind == RTC_LUA_JOB_ADD_FRAME) {
            if (job.camera.hsize == 0 || job.camera.vsize == 0 || job.camera.hsize > 65535u || job.camera.vsize > 65535u) return RTC_ERR_ARG;
            continue;
        }
        if (rtc_float_format_for_name(job.outfile, &f) == RTC_OK) {
            if (!rtc_float_size_ok(f, job.camera.hsize, job.camera.vsize)) return RTC_ERR_ARG;
            continue;
        }
        const rtc_status fs = rtc_image_format_for_name(job.outfile, &f);
        if (fs != RTC_OK) return fs == RTC_ERR_ARG ? RTC_ERR_UNSUPPORTED : fs;
        if (!rtc_image_size_ok(f, job.camera.hsize, job.camera.vsize) || job.camera.hsize > 65535u || job.camera.vsize > 65535u)
            return RTC_ERR_ARG;
    }
    return RTC_OK;
}

rtc_status render_lua(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags, Entry entry, int32_t quality,
                      rtc_lua_file_fn fn, void *user, rtc_stats *stats) {
    if (!ctx || !prog || mode > RTC_MODE_RENDER_ASYNC) return RTC_ERR_ARG;
    if (entry == Entry::SAVED) {
        const rtc_status cs = check_saved(prog);
        if (cs != RTC_OK) return cs;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    constexpr uint32_t RING = rtc_context::MAX_LANES + 1u; // a frame's buffers are reused only after `depth` later launches
    struct Slot {
        DevBuf<uint8_t> d;     // the frame's rows (a float file's job: its f64 canvas)
        uint8_t *h = nullptr;  // the delivered bytes (page-locked)
        size_t hcap = 0;
        RtcEncoder enc;
        unsigned long long *h_len = nullptr; // page-locked: an encoded body's length lands here
        hipEvent_t done = nullptr;
        bool pending = false;
        Output out;
        RtcEncoded e;
        uint32_t job = 0;
    } ring[RING];
    hipStream_t copy = nullptr; // created by the first encoded job
    const uint32_t njobs = rtc_lua_program_jobs(prog);
    const uint32_t lanes_before = ctx->lanes;
    rtc_world *world = nullptr;
    rtc_status st = RTC_OK;
    bool stop = false;
    auto host_buf = [&](Slot &sl, size_t bytes) -> rtc_status {
        if (sl.hcap >= bytes) return RTC_OK;
        if (sl.h) (void)hipHostFree(sl.h);
        sl.h = nullptr;
        sl.hcap = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&sl.h), bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return RTC_ERR_NOMEM; }
        sl.hcap = bytes;
        return RTC_OK;
    };
    auto deliver = [&](Slot &sl) -> rtc_status { // wait for the slot's output and hand it over
        if (!sl.pending) return RTC_OK;
        sl.pending = false;
        if (hipEventSynchronize(sl.done) != hipSuccess) return RTC_ERR_DEVICE;
        rtc_lua_job job;
        const rtc_status js = rtc_lua_program_job(prog, sl.job, &job);
        if (js != RTC_OK) return js;
        unsigned long long len = (unsigned long long)3 * job.camera.hsize * job.camera.vsize; // the rows
        if (sl.out.encoded) {
            len = *sl.h_len;
            const size_t n = sl.e.file_bytes(len);
            if (n == 0) return RTC_ERR_DEVICE;
            const rtc_status hb = host_buf(sl, n);
            if (hb != RTC_OK) return hb;
            if (hipMemcpyAsync(sl.h + sl.e.prefix(), sl.e.d_body, (size_t)len, hipMemcpyDeviceToHost, copy) != hipSuccess ||
                hipStreamSynchronize(copy) != hipSuccess)
                return RTC_ERR_DEVICE;
        } else if (sl.out.format == RTC_LUA_OUT_FILE) { // a saved PPM
            sl.e = RtcEncoded{};
            sl.e.host = RtcEncoded::PPM_ROWS;
            sl.e.width = job.camera.hsize;
            sl.e.height = job.camera.vsize;
        } else {
            if (fn && !stop && fn(user, &job, sl.job, sl.out.format, sl.h, (size_t)len) != 0) stop = true;
            return RTC_OK;
        }
        std::vector<uint8_t> text;
        size_t nbytes = 0;
        const uint8_t *file = rtc_encode_finish(sl.e, len, sl.h, text, &nbytes);
        if (!file) return RTC_ERR_ARG;
        if (fn && !stop && fn(user, &job, sl.job, sl.out.format, file, nbytes) != 0) stop = true;
        return RTC_OK;
    };
    auto drain = [&](uint32_t next_job) -> rtc_status { // every output in flight, oldest first
        rtc_status r = RTC_OK;
        for (uint32_t k = 0; k < RING; ++k) {
            const rtc_status d = deliver(ring[(next_job + k) % RING]);
            if (r == RTC_OK) r = d;
        }
        return r;
    };
    if (stats) st = rtc_stats_reset(ctx);
    if (st == RTC_OK && lanes_before == 1u && njobs > 1u) st = rtc_context_set_pipeline(ctx, 3u);
    uint32_t i = 0;
    std::vector<rtc_area_light> light_buf(RTC_MAX_LIGHT_SAMPLES); // one buffer for every job's lights (26 KB: not on the stack)
    rtc_area_light *const lights = light_buf.data();
    for (; st == RTC_OK && !stop && i < njobs; ++i) {
        rtc_lua_job job;
        st = rtc_lua_program_job(prog, i, &job);
        if (st != RTC_OK) break;
        // every light of the job's world, point lights as 1x1 area lights (a World of at most RTC_MAX_LIGHTS samples IS the
        // rtc_world_create_lights World of those samples)
        uint32_t n_lights = 0;
        if ((st = rtc_lua_program_job_area_lights(prog, i, lights, RTC_MAX_LIGHT_SAMPLES, &n_lights)) != RTC_OK) break;
        const size_t bytes = (size_t)3 * job.camera.hsize * job.camera.vsize;
        Output out;
        if ((st = choose(entry, job, quality, &out)) != RTC_OK) break;
        if (bytes == 0 || (out.encoded && (job.camera.hsize > 65535u || job.camera.vsize > 65535u))) { st = RTC_ERR_ARG; break; }
        Slot &sl = ring[i % RING];
        st = deliver(sl);
        if (st != RTC_OK || stop) break;
        if (!world) { // the program's first job
            st = rtc_world_create_area_lights(ctx, job.shapes, job.n_shapes, lights, n_lights, &world);
            if (st != RTC_OK) break;
        } else if (!job.same_world_as_previous && ctx->world_update) {
            // other contents for the resident World, ordered like a launch: the frames in flight keep theirs, and the
            // outputs' ring is safe as it is (a slot is reused only after `depth` later launches)
            st = rtc_world_update_area_lights(ctx, world, job.shapes, job.n_shapes, lights, n_lights);
            if (st != RTC_OK) break;
        } else if (!job.same_world_as_previous) { // RTC_WORLD_UPDATE=0, a new World: nothing may still read the old one
            st = drain(i);
            if (st == RTC_OK) st = rtc_context_synchronize(ctx);
            if (st != RTC_OK || stop) break;
            rtc_world_destroy(world);
            world = nullptr;
            st = rtc_world_create_area_lights(ctx, job.shapes, job.n_shapes, lights, n_lights, &world);
            if (st != RTC_OK) break;
        }
        if ((st = sl.d.reserve(out.f64 ? bytes * sizeof(double) : bytes)) != RTC_OK) break;
        if (!out.encoded && (st = host_buf(sl, bytes)) != RTC_OK) break;
        if (out.encoded) {
            if (!sl.h_len && hipHostMalloc(reinterpret_cast<void **>(&sl.h_len), sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { st = RTC_ERR_NOMEM; break; }
            if (!copy && hipStreamCreateWithFlags(&copy, hipStreamNonBlocking) != hipSuccess) { copy = nullptr; st = RTC_ERR_DEVICE; break; }
        }
        if (!sl.done && hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) != hipSuccess) { st = RTC_ERR_DEVICE; break; }
        st = rtc_render_rows(ctx, world, &job.camera, mode, 0, job.camera.vsize, out.f64 ? sl.d.get() : nullptr, out.f64 ? nullptr : sl.d.get(), flags);
        if (st != RTC_OK) break;
        hipStream_t s = ctx->lanes > 1u ? ctx->lane[ctx->last.lane] : ctx->stream; // the stream that launch went to
        if (out.encoded) {
            st = sl.enc.enqueue(out.job, sl.d.get(), job.camera.hsize, job.camera.vsize, 3, s, &sl.e);
            if (st != RTC_OK) break;
            if (hipMemcpyAsync(sl.h_len, sl.e.d_len, sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess) { st = RTC_ERR_DEVICE; break; }
        } else if (hipMemcpyAsync(sl.h, sl.d.get(), bytes, hipMemcpyDeviceToHost, s) != hipSuccess) {
            st = RTC_ERR_DEVICE;
            break;
        }
        if (hipEventRecord(sl.done, s) != hipSuccess) { st = RTC_ERR_DEVICE; break; }
        sl.pending = true;
        sl.out = out;
        sl.job = i;
    }
    {
        const rtc_status d = drain(i);
        if (st == RTC_OK) st = d;
    }
    const rtc_status sy = rtc_context_synchronize(ctx);
    if (st == RTC_OK) st = sy;
    for (hipStream_t lane : ctx->lane) // whatever failed above, nothing may still use the slots' buffers
        if (lane) (void)hipStreamSynchronize(lane);
    if (world) rtc_world_destroy(world);
    for (Slot &sl : ring) { // (the slots' device buffers are freed when the ring goes out of scope, after these syncs)
        if (sl.h) (void)hipHostFree(sl.h);
        if (sl.h_len) (void)hipHostFree(sl.h_len);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (copy) (void)hipStreamDestroy(copy);
    if (ctx->lanes != lanes_before) {
        const rtc_status r = rtc_context_set_pipeline(ctx, lanes_before);
        if (st == RTC_OK) st = r;
    }
    if (st == RTC_OK && stats) st = rtc_stats_read(ctx, stats);
    return st;
}

struct FrameFnAdapter {
    rtc_lua_frame_fn fn;
    void *user;
};

int frame_fn_adapter(void *user, const rtc_lua_job *job, uint32_t job_index, uint32_t, const uint8_t *bytes, size_t) {
    const FrameFnAdapter *a = static_cast<const FrameFnAdapter *>(user);
    return a->fn ? a->fn(a->user, job, job_index, bytes) : 0;
}

struct GifFnAdapter {
    rtc_lua_gif_fn fn;
    void *user;
};

int gif_fn_adapter(void *user, const rtc_lua_job *job, uint32_t job_index, uint32_t, const uint8_t *bytes, size_t nbytes) {
    const GifFnAdapter *a = static_cast<const GifFnAdapter *>(user);
    return a->fn ? a->fn(a->user, job, job_index, bytes, nbytes) : 0;
}

} // namespace

rtc_status rtc_lua_program_render(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags, rtc_lua_frame_fn fn,
                                  void *user, rtc_stats *stats) {
    FrameFnAdapter a{fn, user};
    return render_lua(ctx, prog, mode, flags, Entry::ROWS, 0, frame_fn_adapter, &a, stats);
}

rtc_status rtc_lua_program_render_gif(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags, rtc_lua_gif_fn fn,
                                      void *user, rtc_stats *stats) {
    GifFnAdapter a{fn, user};
    return render_lua(ctx, prog, mode, flags, Entry::GIF, 0, gif_fn_adapter, &a, stats);
}

rtc_status rtc_lua_program_render_files(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags, int32_t quality,
                                        rtc_lua_file_fn fn, void *user, rtc_stats *stats) {
    if (quality < 1 || quality > 100) return RTC_ERR_ARG;
    return render_lua(ctx, prog, mode, flags, Entry::FILES, quality, fn, user, stats);
}

rtc_status rtc_lua_program_render_png(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags, rtc_lua_file_fn fn,
                                      void *user, rtc_stats *stats) {
    return render_lua(ctx, prog, mode, flags, Entry::PNG, 0, fn, user, stats);
}

rtc_status rtc_lua_program_render_saved(rtc_context *ctx, const rtc_lua_program *prog, uint32_t mode, uint32_t flags, rtc_lua_file_fn fn,
                                        void *user, rtc_stats *stats) {
    return render_lua(ctx, prog, mode, flags, Entry::SAVED, 0, fn, user, stats);
}
