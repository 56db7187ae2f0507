// rtc_image.hip — [device] the save-by-name writer of include/rtc.h on gfx950 for a frame already in device memory, and the
// encoder object that uses it. host_image.cpp states the same bytes on the host; the layouts of both are rtc_image_layout.
//
// Kernels, by format:
//   k_image_pack   BMP, TGA, TIFF, farbfeld, PAM (and the raw R,G,B / R,G,B,255 inputs of the chains below): one thread per
//                  16 bytes of the FILE, so every store is one aligned 16-byte store and a wave writes 1 KiB contiguously;
//                  a thread takes its bytes from the header (computed on the host, uploaded in front of the launch) or
//                  from the frame (row flipped for BMP, B and R swapped for BMP / TGA, each sample twice for farbfeld),
//                  walking pixel, row and channel from one division at its first byte
//   k_image_wrap   PNG, JPEG, GIF, ICO: the chain's output (PNG file, JPEG entropy-coded data, GIF record, ICO's PNG) behind
//                  the host's header bytes (ICO: the PNG's length patched in from the device) and in front of the suffix
//                  (GIF: 0x3B), 16 bytes per thread as above; its length is known only on the device
// PPM is printed on the host from the R,G,B rows (k_image_pack's raw packing): 3 bytes per pixel cross PCIe instead of ~12.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "rtc.h"
#include "rtc_gif.h"
#include "rtc_image.h"
#include "rtc_internal.h"
#include "rtc_jpeg.h"
#include "rtc_png.h"

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

constexpr uint32_t PACK_THREADS = 256;
constexpr uint32_t NO_PATCH = 0xffffffffu;

struct PackArgs {
    const uint8_t *src;
    const uint8_t *hdr;
    uint8_t *out;
    unsigned long long *len;
    unsigned long long file_bytes;
    uint32_t w, h, channels, header, bpp, bgr, flip;
};

__global__ __launch_bounds__(PACK_THREADS) void k_image_pack(PackArgs a) {
    const unsigned long long p0 = 16ull * (blockIdx.x * (unsigned long long)PACK_THREADS + threadIdx.x);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.len = a.file_bytes;
    if (p0 >= a.file_bytes) return;
    uint32_t v[4] = {0, 0, 0, 0}; // the 16 bytes, little-endian in 4 words
    const unsigned long long b0 = p0 > a.header ? p0 - a.header : 0ull;
    unsigned long long pix = b0 / a.bpp;
    uint32_t c = (uint32_t)(b0 - pix * a.bpp);
    uint32_t y = (uint32_t)(pix / a.w), x = (uint32_t)(pix - (unsigned long long)y * a.w);
    const uint8_t *row = a.src + (size_t)(a.flip ? a.h - 1u - y : y) * a.w * a.channels;
    for (uint32_t k = 0; k < 16; ++k) {
        const unsigned long long p = p0 + k;
        uint32_t byte = 0;
        if (p < a.header) {
            byte = a.hdr[p];
        } else if (p < a.file_bytes) {
            const uint32_t comp = a.bpp == 8 ? c >> 1 : c; // farbfeld: v * 257 is the byte v twice
            const uint32_t ch = (a.bgr && comp != 1u && comp != 3u) ? 2u - comp : comp;
            byte = ch == 3u ? 255u : row[(size_t)x * a.channels + ch];
            if (++c == a.bpp) {
                c = 0;
                if (++x == a.w) {
                    x = 0;
                    ++y;
                    if (y < a.h) row = a.src + (size_t)(a.flip ? a.h - 1u - y : y) * a.w * a.channels;
                }
            }
        }
        v[k >> 2] |= byte << (8u * (k & 3u));
    }
    *reinterpret_cast<uint4 *>(a.out + p0) = make_uint4(v[0], v[1], v[2], v[3]);
}

struct WrapArgs {
    const uint8_t *hdr;           // `header` bytes (device)
    const uint8_t *src;           // the chain's output
    const unsigned long long *src_len;
    unsigned long long src_cap;   // bytes readable at src
    uint8_t *out;
    unsigned long long *len;
    unsigned long long cap;       // bytes of `out` (a multiple of 16)
    uint32_t header, patch_at;    // ICO: the PNG's length goes to hdr bytes patch_at .. +3
    uint32_t suffix_len, suffix;
};

__global__ __launch_bounds__(PACK_THREADS) void k_image_wrap(WrapArgs a) {
    const unsigned long long L = *a.src_len;
    const unsigned long long total = a.header + L + a.suffix_len;
    const bool fits = L <= a.src_cap && total <= a.cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.len = fits ? total : 0ull;
    if (!fits) return;
    for (unsigned long long p0 = 16ull * (blockIdx.x * (unsigned long long)PACK_THREADS + threadIdx.x); p0 < total;
         p0 += 16ull * gridDim.x * PACK_THREADS) {
        uint32_t v[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < 16; ++k) {
            const unsigned long long p = p0 + k;
            uint32_t byte = 0;
            if (p < a.header) {
                byte = (a.patch_at != NO_PATCH && p >= a.patch_at && p < a.patch_at + 4ull) ? (uint32_t)(L >> (8 * (p - a.patch_at))) & 255u
                                                                                           : a.hdr[p];
            } else if (p < a.header + L) {
                byte = a.src[p - a.header];
            } else if (p < total) {
                byte = a.suffix;
            }
            v[k >> 2] |= byte << (8u * (k & 3u));
        }
        *reinterpret_cast<uint4 *>(a.out + p0) = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

} // namespace

// ---- host side ------------------------------------------------------------------------------------------------------

struct ImageScratch {
    uint8_t *out = nullptr, *tmp = nullptr, *d_hdr = nullptr, *h_hdr = nullptr;
    size_t out_cap = 0, tmp_cap = 0, hdr_cap = 0;
    unsigned long long *d_len = nullptr;
    PngScratch *png = nullptr;
    JpegScratch *jpeg = nullptr;
    GifFrameScratch *gif = nullptr;

    static rtc_status dev(uint8_t *&p, size_t &cap, size_t bytes) {
        if (bytes <= cap) return RTC_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e == hipErrorOutOfMemory ? RTC_ERR_NOMEM : RTC_ERR_DEVICE; }
        cap = bytes;
        return RTC_OK;
    }
    // the header's device copy and its page-locked source (the upload is asynchronous; the source stays until the next file)
    rtc_status header(size_t bytes) {
        if (bytes <= hdr_cap) return RTC_OK;
        if (h_hdr) (void)hipHostFree(h_hdr);
        if (d_hdr) (void)hipFree(d_hdr);
        h_hdr = d_hdr = nullptr;
        hdr_cap = 0;
        const size_t b = std::max<size_t>(bytes, 4096);
        size_t dcap = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&h_hdr), b, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h_hdr = nullptr; return RTC_ERR_NOMEM; }
        const rtc_status st = dev(d_hdr, dcap, b);
        if (st != RTC_OK) return st;
        hdr_cap = b;
        return RTC_OK;
    }
    void release() {
        if (out) (void)hipFree(out);
        if (tmp) (void)hipFree(tmp);
        if (d_hdr) (void)hipFree(d_hdr);
        if (h_hdr) (void)hipHostFree(h_hdr);
        if (d_len) (void)hipFree(d_len);
        out = tmp = d_hdr = h_hdr = nullptr;
        d_len = nullptr;
        out_cap = tmp_cap = hdr_cap = 0;
        rtc_png_scratch_free(png);
        rtc_jpeg_scratch_free(jpeg);
        rtc_gif_scratch_free(gif);
        png = nullptr;
        jpeg = nullptr;
        gif = nullptr;
    }
};

namespace {

bool encode_args_ok(uint32_t format, const void *d, uint32_t w, uint32_t h, uint32_t channels) {
    return d && format <= RTC_IMAGE_PAM && (channels == 3 || channels == 4) && rtc_image_size_ok(format, w, h);
}

// k_image_pack of `format` (a packed file or a raw packing) from `src` into `dst` (at least up16(file_bytes) bytes)
rtc_status pack(ImageScratch &sc, uint32_t format, const uint8_t *src, uint32_t w, uint32_t h, uint32_t channels, uint8_t *dst,
                hipStream_t s) {
    RtcImageLayout L;
    if (!rtc_image_layout(format, w, h, &L, nullptr)) return RTC_ERR_ARG;
    rtc_status st = sc.header(L.header);
    if (st != RTC_OK) return st;
    if (L.header) {
        rtc_image_layout(format, w, h, &L, sc.h_hdr);
        HIP_TRY(hipMemcpyAsync(sc.d_hdr, sc.h_hdr, L.header, hipMemcpyHostToDevice, s));
    }
    const unsigned long long threads = (L.file_bytes + 15) / 16;
    const PackArgs a{src, sc.d_hdr, dst, sc.d_len, L.file_bytes, w, h, channels, L.header, L.bytes_per_pixel, L.bgr, L.flip};
    hipLaunchKernelGGL(k_image_pack, dim3((uint32_t)((threads + PACK_THREADS - 1) / PACK_THREADS)), dim3(PACK_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return RTC_OK;
}

// k_image_wrap: `header` host bytes + the chain's src_len bytes at src + the suffix, into sc.out
rtc_status wrap(ImageScratch &sc, const uint8_t *hdr, uint32_t header, uint32_t patch_at, const uint8_t *src,
                const unsigned long long *src_len, size_t src_cap, uint32_t suffix_len, uint32_t suffix, hipStream_t s) {
    rtc_status st = sc.header(header);
    if (st == RTC_OK) st = ImageScratch::dev(sc.out, sc.out_cap, up16(header + src_cap + suffix_len));
    if (st != RTC_OK) return st;
    if (header) {
        std::memcpy(sc.h_hdr, hdr, header);
        HIP_TRY(hipMemcpyAsync(sc.d_hdr, sc.h_hdr, header, hipMemcpyHostToDevice, s));
    }
    const WrapArgs a{sc.d_hdr, src, src_len, (unsigned long long)src_cap, sc.out, sc.d_len, (unsigned long long)sc.out_cap, header, patch_at, suffix_len, suffix};
    const uint32_t grid = (uint32_t)std::min<size_t>(1024, (sc.out_cap / 16 + PACK_THREADS - 1) / PACK_THREADS);
    hipLaunchKernelGGL(k_image_wrap, dim3(grid), dim3(PACK_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return RTC_OK;
}

// Enqueue the whole chain on `s`; the file (PPM: the R,G,B rows) is then at sc.out, its length at sc.d_len.
rtc_status encode_frame(ImageScratch &sc, uint32_t format, const uint8_t *d_pixels, uint32_t w, uint32_t h, uint32_t channels,
                        hipStream_t s) {
    if (!sc.d_len) {
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&sc.d_len), sizeof(unsigned long long));
        if (e != hipSuccess) { (void)hipGetLastError(); sc.d_len = nullptr; return RTC_ERR_DEVICE; }
    }
    const size_t px = (size_t)w * h;
    rtc_status st = RTC_OK;
    switch (format) {
    case RTC_IMAGE_PPM: {
        st = ImageScratch::dev(sc.out, sc.out_cap, up16(3 * px));
        return st == RTC_OK ? pack(sc, RTC_IMAGE_RAW_RGB, d_pixels, w, h, channels, sc.out, s) : st;
    }
    case RTC_IMAGE_PNG:
    case RTC_IMAGE_GIF:
    case RTC_IMAGE_ICO: {
        // the chain's input: R,G,B for PNG and GIF, R,G,B,255 for ICO's PNG (always repacked: the input's alpha is not read)
        const uint32_t want = format == RTC_IMAGE_ICO ? 4u : 3u;
        const uint8_t *in = d_pixels;
        if (channels != want || want == 4u) {
            st = ImageScratch::dev(sc.tmp, sc.tmp_cap, up16(want * px));
            if (st == RTC_OK) st = pack(sc, want == 3u ? RTC_IMAGE_RAW_RGB : RTC_IMAGE_RAW_RGBA, d_pixels, w, h, channels, sc.tmp, s);
            if (st != RTC_OK) return st;
            in = sc.tmp;
        }
        if (format == RTC_IMAGE_GIF) {
            if (!sc.gif && !(sc.gif = rtc_gif_scratch_new())) return RTC_ERR_NOMEM;
            st = (rtc_status)rtc_gif_scratch_encode(sc.gif, in, w, h, s);
            if (st != RTC_OK) return st;
            uint8_t hdr[RTC_GIF_FILE_HEADER];
            rtc_gif_file_header(hdr, w, h);
            return wrap(sc, hdr, sizeof hdr, NO_PATCH, rtc_gif_scratch_record(sc.gif), rtc_gif_scratch_length(sc.gif),
                        rtc_gif_scratch_record_cap(sc.gif), 1, 0x3B, s);
        }
        if (!sc.png && !(sc.png = rtc_png_scratch_new())) return RTC_ERR_NOMEM;
        st = (rtc_status)rtc_png_scratch_encode(sc.png, in, w, h, want, s);
        if (st != RTC_OK) return st;
        uint8_t hdr[RTC_ICO_HEADER_BYTES];
        if (format == RTC_IMAGE_ICO) rtc_image_ico_header(w, h, 0, hdr); // the length is patched in on the device
        return wrap(sc, hdr, format == RTC_IMAGE_ICO ? RTC_ICO_HEADER_BYTES : 0u, format == RTC_IMAGE_ICO ? 14u : NO_PATCH,
                    rtc_png_scratch_data(sc.png), rtc_png_scratch_length(sc.png), rtc_png_scratch_out_cap(sc.png), 0, 0, s);
    }
    case RTC_IMAGE_JPEG: {
        if (!sc.jpeg && !(sc.jpeg = rtc_jpeg_scratch_new())) return RTC_ERR_NOMEM;
        st = (rtc_status)rtc_jpeg_scratch_encode(sc.jpeg, d_pixels, w, h, channels, RTC_IMAGE_JPEG_QUALITY, s);
        if (st != RTC_OK) return st;
        uint8_t hdr[RTC_JPEG_HEADER_BYTES];
        rtc_jpeg_header(w, h, RTC_IMAGE_JPEG_QUALITY, hdr);
        return wrap(sc, hdr, RTC_JPEG_HEADER_BYTES, NO_PATCH, rtc_jpeg_scratch_data(sc.jpeg), rtc_jpeg_scratch_length(sc.jpeg),
                    rtc_jpeg_scratch_out_cap(sc.jpeg), 0, 0, s);
    }
    default: {
        RtcImageLayout L;
        if (!rtc_image_layout(format, w, h, &L, nullptr)) return RTC_ERR_ARG;
        st = ImageScratch::dev(sc.out, sc.out_cap, up16((size_t)L.file_bytes));
        return st == RTC_OK ? pack(sc, format, d_pixels, w, h, channels, sc.out, s) : st;
    }
    }
}

// the host's part: the file from the bytes that crossed PCIe (PPM: printed from the rows)
void finish(uint32_t format, uint32_t w, uint32_t h, std::vector<uint8_t> &file) {
    if (format != RTC_IMAGE_PPM) return;
    const std::vector<uint8_t> rows = std::move(file);
    file.assign(rtc_image_format(RTC_IMAGE_PPM, rows.data(), w, h, 3, nullptr, 0), 0);
    rtc_image_format(RTC_IMAGE_PPM, rows.data(), w, h, 3, file.data(), file.size());
}

} // namespace

ImageScratch *rtc_image_scratch_new() { return new (std::nothrow) ImageScratch; }
void rtc_image_scratch_free(ImageScratch *sc) {
    if (!sc) return;
    sc->release();
    delete sc;
}
int rtc_image_scratch_encode(ImageScratch *sc, uint32_t format, const void *d_pixels, uint32_t width, uint32_t height, uint32_t channels,
                             void *stream) {
    if (!sc || !encode_args_ok(format, d_pixels, width, height, channels)) return RTC_ERR_ARG;
    return encode_frame(*sc, format, static_cast<const uint8_t *>(d_pixels), width, height, channels, static_cast<hipStream_t>(stream));
}
const uint8_t *rtc_image_scratch_data(const ImageScratch *sc) { return sc->out; }
size_t rtc_image_scratch_out_cap(const ImageScratch *sc) { return sc->out_cap; }
const unsigned long long *rtc_image_scratch_length(const ImageScratch *sc) { return sc->d_len; }

struct rtc_image_encoder {
    rtc_context *ctx = nullptr;
    ImageScratch sc;
    uint8_t *d_frame = nullptr; // render target of rtc_image_encoder_render
    size_t frame_cap = 0;
    std::vector<uint8_t> file;
};

rtc_status rtc_image_encoder_create(rtc_context *ctx, rtc_image_encoder **out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    *out = new (std::nothrow) rtc_image_encoder;
    if (!*out) return RTC_ERR_NOMEM;
    (*out)->ctx = ctx;
    return RTC_OK;
}

void rtc_image_encoder_destroy(rtc_image_encoder *e) {
    if (!e) return;
    if (hipSetDevice(e->ctx->device) == hipSuccess) {
        (void)hipStreamSynchronize(e->ctx->stream);
        e->sc.release();
        if (e->d_frame) (void)hipFree(e->d_frame);
    }
    delete e;
}

rtc_status rtc_image_encoder_encode_device(rtc_image_encoder *e, uint32_t format, const void *d_pixels, uint32_t width, uint32_t height,
                                           uint32_t channels) {
    if (!e || !encode_args_ok(format, d_pixels, width, height, channels)) return RTC_ERR_ARG;
    rtc_context *ctx = e->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const rtc_status st = encode_frame(e->sc, format, static_cast<const uint8_t *>(d_pixels), width, height, channels, ctx->stream);
    if (st != RTC_OK) return st;
    unsigned long long len = 0;
    HIP_TRY(hipMemcpyAsync(&len, e->sc.d_len, sizeof len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (len == 0 || len > e->sc.out_cap) return RTC_ERR_DEVICE;
    e->file.resize((size_t)len);
    HIP_TRY(hipMemcpy(e->file.data(), e->sc.out, (size_t)len, hipMemcpyDeviceToHost));
    finish(format, width, height, e->file);
    return RTC_OK;
}

rtc_status rtc_image_encoder_render(rtc_image_encoder *e, uint32_t format, const rtc_world *w, const rtc_camera *cam, uint32_t mode,
                                    uint32_t flags, float gamma) {
    if (!e || !w || !cam || w->ctx != e->ctx || format > RTC_IMAGE_PAM) return RTC_ERR_ARG;
    if (!rtc_image_size_ok(format, cam->hsize, cam->vsize) || cam->hsize > 65535u || cam->vsize > 65535u) return RTC_ERR_ARG;
    if (!(gamma > 0.0f) || !(gamma <= 3.4028235e38f)) return RTC_ERR_ARG;
    rtc_context *ctx = e->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t channels = gamma == 1.0f ? 3u : 4u;
    const uint32_t rows = channels == 3u ? cam->vsize : (cam->vsize + 7u) / 8u * 8u; // a view holds whole 8-row bands
    const size_t bytes = (size_t)channels * cam->hsize * rows;
    if (e->frame_cap < bytes) {
        if (e->d_frame) (void)hipFree(e->d_frame);
        e->d_frame = nullptr;
        e->frame_cap = 0;
        const hipError_t he = hipMalloc(reinterpret_cast<void **>(&e->d_frame), bytes);
        if (he != hipSuccess) { (void)hipGetLastError(); return he == hipErrorOutOfMemory ? RTC_ERR_NOMEM : RTC_ERR_DEVICE; }
        e->frame_cap = bytes;
    }
    rtc_status st = channels == 3u ? rtc_render_rows(ctx, w, cam, mode, 0, cam->vsize, nullptr, e->d_frame, flags)
                                   : rtc_render_views_rgba8(ctx, w, cam, 1, mode, 0, 1, gamma, e->d_frame, rows, flags);
    if (st == RTC_OK) st = rtc_context_fence(ctx); // a pipelined context rendered on a lane: the stream waits for it
    if (st == RTC_OK) st = rtc_image_encoder_encode_device(e, format, e->d_frame, cam->hsize, cam->vsize, channels);
    return st;
}

size_t rtc_image_encoder_bytes(const rtc_image_encoder *e, uint8_t *buf, size_t cap) {
    if (!e || e->file.empty()) return 0;
    if (buf) std::memcpy(buf, e->file.data(), std::min(cap, e->file.size()));
    return e->file.size();
}

rtc_status rtc_image_encoder_write(const rtc_image_encoder *e, const char *path) {
    if (!e || !path || e->file.empty()) return RTC_ERR_ARG;
    FILE *f = std::fopen(path, "wb");
    if (!f) return RTC_ERR_IO;
    const bool ok = std::fwrite(e->file.data(), 1, e->file.size(), f) == e->file.size();
    return (std::fclose(f) == 0 && ok) ? RTC_OK : RTC_ERR_IO;
}
