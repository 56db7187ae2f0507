// rtc_encode.cpp — [device] the device file writers' shared host side (rtc_encode.h): which chains make each file, the
// host's part of the file, and the encoder objects of include/rtc.h (rtc_gif_writer, rtc_jpeg_encoder, rtc_png_encoder,
// rtc_image_encoder, rtc_float_encoder) on one core.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "rtc.h"
#include "rtc_encode.h"
#include "rtc_float.h"
#include "rtc_gif.h"
#include "rtc_image.h"
#include "rtc_internal.h"
#include "rtc_jpeg.h"

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

uint32_t RtcEncoded::prefix() const {
    switch (host) {
    case JPEG_FILE: return RTC_JPEG_HEADER_BYTES;
    case GIF_FILE: return RTC_GIF_FILE_HEADER;
    case ICO_FILE: return RTC_ICO_HEADER_BYTES;
    default: return 0;
    }
}

const uint8_t *rtc_encode_finish(const RtcEncoded &e, unsigned long long len, uint8_t *file, std::vector<uint8_t> &text,
                                 size_t *nbytes) {
    switch (e.host) {
    case RtcEncoded::BODY: break;
    case RtcEncoded::JPEG_FILE: rtc_jpeg_header(e.width, e.height, e.quality, file); break;
    case RtcEncoded::GIF_FILE:
        rtc_gif_file_header(file, e.width, e.height);
        file[RTC_GIF_FILE_HEADER + len] = 0x3B;
        break;
    case RtcEncoded::ICO_FILE: rtc_image_ico_header(e.width, e.height, (uint32_t)len, file); break;
    case RtcEncoded::PPM_ROWS: // 3 bytes per pixel crossed PCIe: the P3 text is printed here
        text.resize(rtc_image_format(RTC_IMAGE_PPM, file, e.width, e.height, 3, nullptr, 0));
        if (text.empty()) return nullptr;
        rtc_image_format(RTC_IMAGE_PPM, file, e.width, e.height, 3, text.data(), text.size());
        *nbytes = text.size();
        return text.data();
    }
    *nbytes = e.prefix() + (size_t)len + e.suffix();
    return file;
}

rtc_status RtcEncoder::enqueue(const RtcEncodeJob &job, const void *d_pixels, uint32_t w, uint32_t h, uint32_t channels, hipStream_t s,
                               RtcEncoded *e) {
    const uint8_t *px = static_cast<const uint8_t *>(d_pixels);
    *e = RtcEncoded{};
    e->width = w;
    e->height = h;
    if (job.kind == RtcEncodeJob::FLOAT) {
        const rtc_float_planes d{static_cast<const double *>(d_pixels), job.aov, job.rgb_type, 0u};
        return rtc_float_enqueue(flt, job.format, &d, w, h, s, e);
    }
    if (job.kind == RtcEncodeJob::GIF_RECORD) return rtc_gif_enqueue(gif, px, w, h, s, e);
    if (job.kind == RtcEncodeJob::PNG) return rtc_png_enqueue(png, px, w, h, channels, s, e);
    if (job.kind == RtcEncodeJob::JPEG || job.format == RTC_IMAGE_JPEG) {
        e->host = RtcEncoded::JPEG_FILE;
        e->quality = job.kind == RtcEncodeJob::JPEG ? job.quality : RTC_IMAGE_JPEG_QUALITY;
        return rtc_jpeg_enqueue(jpeg, px, w, h, channels, e->quality, s, e);
    }
    switch (job.format) { // the save table
    case RTC_IMAGE_PNG:
    case RTC_IMAGE_GIF:
    case RTC_IMAGE_ICO: {
        // the chain's input: R,G,B for PNG and GIF, R,G,B,255 for ICO's PNG (always repacked: the input's alpha is not read)
        const uint32_t want = job.format == RTC_IMAGE_ICO ? 4u : 3u;
        if (channels != want || want == 4u) {
            RtcEncoded raw;
            const rtc_status st = rtc_image_pack_enqueue(pack, want == 3u ? RTC_IMAGE_RAW_RGB : RTC_IMAGE_RAW_RGBA, px, w, h, channels, s, &raw);
            if (st != RTC_OK) return st;
            px = raw.d_body;
        }
        if (job.format == RTC_IMAGE_GIF) {
            e->host = RtcEncoded::GIF_FILE;
            return rtc_gif_enqueue(gif, px, w, h, s, e);
        }
        if (job.format == RTC_IMAGE_ICO) e->host = RtcEncoded::ICO_FILE;
        return rtc_png_enqueue(png, px, w, h, want, s, e);
    }
    case RTC_IMAGE_PPM: e->host = RtcEncoded::PPM_ROWS; return rtc_image_pack_enqueue(pack, RTC_IMAGE_RAW_RGB, px, w, h, channels, s, e);
    default: return rtc_image_pack_enqueue(pack, job.format, px, w, h, channels, s, e);
    }
}

// ---- the encoder objects --------------------------------------------------------------------------------------------

// What every encoder object is: bound to a context, its encoder's scratch, the render target of its render entry
// (grow-only) and the file on the host.
struct RtcEncoderObject {
    rtc_context *ctx = nullptr;
    RtcEncoder enc;
    DevBuf<uint8_t> d_frame;
    std::vector<uint8_t> file;
};
struct rtc_gif_writer : RtcEncoderObject {
    uint32_t width = 0, height = 0; // file: header + records, without the trailer
};
struct rtc_jpeg_encoder : RtcEncoderObject {};
struct rtc_png_encoder : RtcEncoderObject {};
struct rtc_image_encoder : RtcEncoderObject {};
struct rtc_float_encoder : RtcEncoderObject {};

namespace {

template <typename T>
rtc_status create(rtc_context *ctx, T **out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    *out = new (std::nothrow) T;
    if (!*out) return RTC_ERR_NOMEM;
    (*out)->ctx = ctx;
    return RTC_OK;
}

template <typename T>
void destroy(T *o) {
    if (!o) return;
    if (hipSetDevice(o->ctx->device) == hipSuccess) (void)hipStreamSynchronize(o->ctx->stream);
    delete o; // its device buffers too, after the stream that used them
}

// `job` for the frame at d_pixels on the context's stream; blocks until the file is on the host at file[at..] (file is
// then at + its size long).
rtc_status encode(RtcEncoderObject *o, const RtcEncodeJob &job, const void *d_pixels, uint32_t w, uint32_t h, uint32_t channels,
                  size_t at) {
    rtc_context *ctx = o->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    RtcEncoded e;
    const rtc_status st = o->enc.enqueue(job, d_pixels, w, h, channels, ctx->stream, &e);
    if (st != RTC_OK) return st;
    unsigned long long len = 0;
    HIP_TRY(hipMemcpyAsync(&len, e.d_len, sizeof len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t n = e.file_bytes(len);
    if (n == 0) return RTC_ERR_DEVICE;
    o->file.resize(at + n);
    HIP_TRY(hipMemcpy(o->file.data() + at + e.prefix(), e.d_body, (size_t)len, hipMemcpyDeviceToHost));
    std::vector<uint8_t> text;
    size_t nbytes = 0;
    const uint8_t *f = rtc_encode_finish(e, len, o->file.data() + at, text, &nbytes);
    if (!f) return RTC_ERR_ARG;
    if (f == text.data()) o->file.swap(text); // PPM (at is 0)
    return RTC_OK;
}

// Camera::render + set_gamma(gamma) into the object's frame: at gamma 1 through the rows path (3 channels), at any other
// gamma through rtc_render_views_rgba8 (4 channels); the context's stream waits for it.
rtc_status render(RtcEncoderObject *o, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags, float gamma,
                  uint32_t *channels) {
    rtc_context *ctx = o->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    *channels = gamma == 1.0f ? 3u : 4u;
    const uint32_t rows = *channels == 3u ? cam->vsize : (cam->vsize + 7u) / 8u * 8u; // a view holds whole 8-row bands
    const size_t bytes = (size_t)*channels * cam->hsize * rows;
    if (bytes == 0) return RTC_ERR_ARG;
    rtc_status st = o->d_frame.reserve(bytes);
    if (st != RTC_OK) return st;
    st = *channels == 3u ? rtc_render_rows(ctx, w, cam, mode, 0, cam->vsize, nullptr, o->d_frame.get(), flags)
                         : rtc_render_views_rgba8(ctx, w, cam, 1, mode, 0, 1, gamma, o->d_frame.get(), rows, flags);
    if (st == RTC_OK) st = rtc_context_fence(ctx); // a pipelined context rendered on a lane: the stream waits for it
    return st;
}

// the file, followed by `trailer` when it is not 0 (the GIF writer's 0x3B)
size_t bytes_of(const RtcEncoderObject *o, uint8_t *buf, size_t cap, uint8_t trailer) {
    if (!o || o->file.empty()) return 0;
    const size_t need = o->file.size() + (trailer ? 1 : 0);
    if (buf) {
        std::memcpy(buf, o->file.data(), std::min(cap, o->file.size()));
        if (trailer && cap >= need) buf[need - 1] = trailer;
    }
    return need;
}

rtc_status write_file(const RtcEncoderObject *o, const char *path, uint8_t trailer) {
    if (!o || !path || o->file.empty()) return RTC_ERR_ARG;
    FILE *f = std::fopen(path, "wb");
    if (!f) return RTC_ERR_IO;
    const bool ok = std::fwrite(o->file.data(), 1, o->file.size(), f) == o->file.size() && (!trailer || std::fwrite(&trailer, 1, 1, f) == 1);
    return (std::fclose(f) == 0 && ok) ? RTC_OK : RTC_ERR_IO;
}

// Camera::render's f64 canvas into the object's frame through the rows path (the lens entry with a lens); the context's
// stream waits for it.
rtc_status render_f64(RtcEncoderObject *o, const rtc_world *w, const rtc_camera *cam, const rtc_lens *lens, uint32_t mode, uint32_t flags) {
    rtc_context *ctx = o->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    rtc_status st = o->d_frame.reserve((size_t)3 * sizeof(double) * cam->hsize * cam->vsize);
    if (st != RTC_OK) return st;
    st = lens ? rtc_render_lens_rows(ctx, w, cam, lens, mode, 0, cam->vsize, o->d_frame.get(), nullptr, flags)
              : rtc_render_rows(ctx, w, cam, mode, 0, cam->vsize, o->d_frame.get(), nullptr, flags);
    if (st == RTC_OK) st = rtc_context_fence(ctx);
    return st;
}

bool gamma_ok(float gamma) { return gamma > 0.0f && gamma <= 3.4028235e38f; }

bool jpeg_args_ok(const void *d, uint32_t w, uint32_t h, uint32_t channels, int32_t quality) {
    return d && w >= 1 && w <= 65535u && h >= 1 && h <= 65535u && (channels == 3 || channels == 4) && quality >= 1 && quality <= 100;
}

bool png_args_ok(const void *d, uint32_t w, uint32_t h, uint32_t channels) {
    return d && w >= 1 && w <= 65535u && h >= 1 && h <= 65535u && (channels == 3 || channels == 4);
}

bool image_args_ok(uint32_t format, const void *d, uint32_t w, uint32_t h, uint32_t channels) {
    return d && format <= RTC_IMAGE_PAM && (channels == 3 || channels == 4) && rtc_image_size_ok(format, w, h);
}

} // namespace

rtc_status rtc_gif_writer_create(rtc_context *ctx, rtc_gif_writer **out) { return create(ctx, out); }
void rtc_gif_writer_destroy(rtc_gif_writer *g) { destroy(g); }

rtc_status rtc_gif_writer_append_device(rtc_gif_writer *g, const void *d_rgb8, uint32_t width, uint32_t height) {
    if (!g || !d_rgb8 || width == 0 || height == 0 || width > 65535u || height > 65535u) return RTC_ERR_ARG;
    if (!g->file.empty() && (width != g->width || height != g->height)) return RTC_ERR_ARG;
    const bool first = g->file.empty();
    const rtc_status st = encode(g, {RtcEncodeJob::GIF_RECORD}, d_rgb8, width, height, 3, first ? RTC_GIF_FILE_HEADER : g->file.size());
    if (st != RTC_OK) {
        if (first) g->file.clear();
        return st;
    }
    if (first) {
        rtc_gif_file_header(g->file.data(), width, height);
        g->width = width;
        g->height = height;
    }
    return RTC_OK;
}

rtc_status rtc_gif_writer_render(rtc_gif_writer *g, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags) {
    if (!g || !w || !cam || w->ctx != g->ctx) return RTC_ERR_ARG;
    if (cam->hsize > 65535u || cam->vsize > 65535u) return RTC_ERR_ARG;
    if (!g->file.empty() && (cam->hsize != g->width || cam->vsize != g->height)) return RTC_ERR_ARG;
    uint32_t channels = 0;
    const rtc_status st = render(g, w, cam, mode, flags, 1.0f, &channels);
    return st == RTC_OK ? rtc_gif_writer_append_device(g, g->d_frame.get(), cam->hsize, cam->vsize) : st;
}

size_t rtc_gif_writer_bytes(const rtc_gif_writer *g, uint8_t *buf, size_t cap) { return bytes_of(g, buf, cap, 0x3B); }
rtc_status rtc_gif_writer_write(const rtc_gif_writer *g, const char *path) { return write_file(g, path, 0x3B); }

rtc_status rtc_jpeg_encoder_create(rtc_context *ctx, rtc_jpeg_encoder **out) { return create(ctx, out); }
void rtc_jpeg_encoder_destroy(rtc_jpeg_encoder *e) { destroy(e); }

rtc_status rtc_jpeg_encoder_encode_device(rtc_jpeg_encoder *e, const void *d_pixels, uint32_t width, uint32_t height, uint32_t channels,
                                          int32_t quality) {
    if (!e || !jpeg_args_ok(d_pixels, width, height, channels, quality)) return RTC_ERR_ARG;
    return encode(e, {RtcEncodeJob::JPEG, quality}, d_pixels, width, height, channels, 0);
}

rtc_status rtc_jpeg_encoder_render(rtc_jpeg_encoder *e, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                                   float gamma, int32_t quality) {
    if (!e || !w || !cam || w->ctx != e->ctx) return RTC_ERR_ARG;
    if (cam->hsize == 0 || cam->vsize == 0 || cam->hsize > 65535u || cam->vsize > 65535u || quality < 1 || quality > 100) return RTC_ERR_ARG;
    if (!gamma_ok(gamma)) return RTC_ERR_ARG;
    uint32_t channels = 0;
    const rtc_status st = render(e, w, cam, mode, flags, gamma, &channels);
    return st == RTC_OK ? rtc_jpeg_encoder_encode_device(e, e->d_frame.get(), cam->hsize, cam->vsize, channels, quality) : st;
}

size_t rtc_jpeg_encoder_bytes(const rtc_jpeg_encoder *e, uint8_t *buf, size_t cap) { return bytes_of(e, buf, cap, 0); }
rtc_status rtc_jpeg_encoder_write(const rtc_jpeg_encoder *e, const char *path) { return write_file(e, path, 0); }

rtc_status rtc_png_encoder_create(rtc_context *ctx, rtc_png_encoder **out) { return create(ctx, out); }
void rtc_png_encoder_destroy(rtc_png_encoder *e) { destroy(e); }

rtc_status rtc_png_encoder_encode_device(rtc_png_encoder *e, const void *d_pixels, uint32_t width, uint32_t height, uint32_t channels) {
    if (!e || !png_args_ok(d_pixels, width, height, channels)) return RTC_ERR_ARG;
    return encode(e, {RtcEncodeJob::PNG}, d_pixels, width, height, channels, 0);
}

rtc_status rtc_png_encoder_render(rtc_png_encoder *e, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags, float gamma) {
    if (!e || !w || !cam || w->ctx != e->ctx) return RTC_ERR_ARG;
    if (cam->hsize == 0 || cam->vsize == 0 || cam->hsize > 65535u || cam->vsize > 65535u) return RTC_ERR_ARG;
    if (!gamma_ok(gamma)) return RTC_ERR_ARG;
    uint32_t channels = 0;
    const rtc_status st = render(e, w, cam, mode, flags, gamma, &channels);
    return st == RTC_OK ? rtc_png_encoder_encode_device(e, e->d_frame.get(), cam->hsize, cam->vsize, channels) : st;
}

size_t rtc_png_encoder_bytes(const rtc_png_encoder *e, uint8_t *buf, size_t cap) { return bytes_of(e, buf, cap, 0); }
rtc_status rtc_png_encoder_write(const rtc_png_encoder *e, const char *path) { return write_file(e, path, 0); }

rtc_status rtc_image_encoder_create(rtc_context *ctx, rtc_image_encoder **out) { return create(ctx, out); }
void rtc_image_encoder_destroy(rtc_image_encoder *e) { destroy(e); }

rtc_status rtc_image_encoder_encode_device(rtc_image_encoder *e, uint32_t format, const void *d_pixels, uint32_t width, uint32_t height,
                                           uint32_t channels) {
    if (!e || !image_args_ok(format, d_pixels, width, height, channels)) return RTC_ERR_ARG;
    return encode(e, {RtcEncodeJob::SAVED, 0, format}, d_pixels, width, height, channels, 0);
}

rtc_status rtc_image_encoder_render(rtc_image_encoder *e, uint32_t format, const rtc_world *w, const rtc_camera *cam, uint32_t mode,
                                    uint32_t flags, float gamma) {
    if (!e || !w || !cam || w->ctx != e->ctx || format > RTC_IMAGE_PAM) return RTC_ERR_ARG;
    if (!rtc_image_size_ok(format, cam->hsize, cam->vsize) || cam->hsize > 65535u || cam->vsize > 65535u) return RTC_ERR_ARG;
    if (!gamma_ok(gamma)) return RTC_ERR_ARG;
    uint32_t channels = 0;
    const rtc_status st = render(e, w, cam, mode, flags, gamma, &channels);
    return st == RTC_OK ? rtc_image_encoder_encode_device(e, format, e->d_frame.get(), cam->hsize, cam->vsize, channels) : st;
}

size_t rtc_image_encoder_bytes(const rtc_image_encoder *e, uint8_t *buf, size_t cap) { return bytes_of(e, buf, cap, 0); }
rtc_status rtc_image_encoder_write(const rtc_image_encoder *e, const char *path) { return write_file(e, path, 0); }

rtc_status rtc_float_encoder_create(rtc_context *ctx, rtc_float_encoder **out) { return create(ctx, out); }
void rtc_float_encoder_destroy(rtc_float_encoder *e) { destroy(e); }

rtc_status rtc_float_encoder_encode_device(rtc_float_encoder *e, uint32_t format, const rtc_float_planes *d, uint32_t width, uint32_t height) {
    RtcFloatLayout L;
    if (!e || !rtc_float_layout(format, d, width, height, &L, nullptr)) return RTC_ERR_ARG;
    RtcEncodeJob job{RtcEncodeJob::FLOAT, 0, format};
    job.rgb_type = d->rgb_type;
    job.aov = d->aov;
    return encode(e, job, d->rgb, width, height, 3, 0);
}

rtc_status rtc_float_encoder_render_lens(rtc_float_encoder *e, uint32_t format, const rtc_world *w, const rtc_camera *cam, const rtc_lens *lens,
                                         uint32_t mode, uint32_t flags, uint32_t rgb_type) {
    if (!e || !w || !cam || w->ctx != e->ctx) return RTC_ERR_ARG;
    if (!rtc_float_size_ok(format, cam->hsize, cam->vsize) || (format == RTC_FLOAT_EXR && rgb_type != RTC_EXR_HALF && rgb_type != RTC_EXR_FLOAT))
        return RTC_ERR_ARG;
    const rtc_status st = render_f64(e, w, cam, lens, mode, flags);
    if (st != RTC_OK) return st;
    rtc_float_planes d{};
    d.rgb = reinterpret_cast<const double *>(e->d_frame.get());
    d.rgb_type = rgb_type;
    return rtc_float_encoder_encode_device(e, format, &d, cam->hsize, cam->vsize);
}

rtc_status rtc_float_encoder_render(rtc_float_encoder *e, uint32_t format, const rtc_world *w, const rtc_camera *cam, uint32_t mode,
                                    uint32_t flags, uint32_t rgb_type) {
    return rtc_float_encoder_render_lens(e, format, w, cam, nullptr, mode, flags, rgb_type);
}

size_t rtc_float_encoder_bytes(const rtc_float_encoder *e, uint8_t *buf, size_t cap) { return bytes_of(e, buf, cap, 0); }
rtc_status rtc_float_encoder_write(const rtc_float_encoder *e, const char *path) { return write_file(e, path, 0); }
