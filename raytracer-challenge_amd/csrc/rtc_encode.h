// rtc_encode.h — the one internal interface of the device file writers (rtc_gif.hip, rtc_jpeg.hip, rtc_png.hip,
// rtc_image.hip), used by the encoder objects (rtc_encode.cpp) and the Lua lane loop (rtc_lua_render.cpp). Not part of the
// ABI.
//
// A chain is enqueued behind the frame on a stream and leaves a body in device memory whose length is known only on the
// device. The file is a host prefix, that body and a host suffix: the caller copies the length, then exactly that many
// bytes, and rtc_encode_finish writes the host's part around them.
#ifndef RTC_ENCODE_H
#define RTC_ENCODE_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "rtc.h"

// What to produce from a frame in device memory.
struct RtcEncodeJob {
    enum Kind : uint32_t { GIF_RECORD, JPEG, PNG, SAVED } kind = GIF_RECORD;
    int32_t quality = 0; // JPEG
    uint32_t format = 0; // SAVED: the save table's RTC_IMAGE_* format
};

// What an enqueued chain leaves behind.
struct RtcEncoded {
    const uint8_t *d_body = nullptr;           // the body, [0, *d_len) (device)
    const unsigned long long *d_len = nullptr; // its length (device)
    unsigned long long cap = 0;                // bytes readable at d_body
    unsigned long long min_len = 1;            // the chain's own check: min_len <= *d_len <= cap
    // the host's part: nothing, the JPEG header (at `quality`), the GIF file header and trailer, the ICO header (its length
    // field patched), or — for PPM — the body is the R,G,B rows the host prints
    enum Host : uint32_t { BODY, JPEG_FILE, GIF_FILE, ICO_FILE, PPM_ROWS } host = BODY;
    uint32_t width = 0, height = 0;
    int32_t quality = 0;

    uint32_t prefix() const;
    uint32_t suffix() const { return host == GIF_FILE ? 1u : 0u; }
    // the bytes of the file around a body of `len` bytes (prefix + len + suffix; PPM: the rows), 0 when `len` fails the check
    size_t file_bytes(unsigned long long len) const {
        return (len < min_len || len > cap) ? 0 : prefix() + (size_t)len + suffix();
    }
};

// The file of a finished chain: `file` holds file_bytes(len) bytes, the body copied to file + prefix(). Writes the prefix
// and suffix in place, or prints a PPM's rows into `text`. Returns the file (`file` or text's data), *nbytes of it; null
// when the rows cannot be printed.
const uint8_t *rtc_encode_finish(const RtcEncoded &e, unsigned long long len, uint8_t *file, std::vector<uint8_t> &text,
                                 size_t *nbytes);

// Each file's chain: its scratch is created by the first enqueue (into `sc`) and grow-only; the arguments are checked by
// the callers. The input is height*width*channels bytes (GIF: channels 3).
struct GifScratch;
struct JpegScratch;
struct PngScratch;
struct PackScratch;
rtc_status rtc_gif_enqueue(GifScratch *&sc, const uint8_t *d_rgb8, uint32_t width, uint32_t height, hipStream_t s, RtcEncoded *e);
void rtc_gif_release(GifScratch *sc);
rtc_status rtc_jpeg_enqueue(JpegScratch *&sc, const uint8_t *d_pixels, uint32_t width, uint32_t height, uint32_t channels,
                            int32_t quality, hipStream_t s, RtcEncoded *e);
void rtc_jpeg_release(JpegScratch *sc);
rtc_status rtc_png_enqueue(PngScratch *&sc, const uint8_t *d_pixels, uint32_t width, uint32_t height, uint32_t channels,
                           hipStream_t s, RtcEncoded *e);
void rtc_png_release(PngScratch *sc);
// k_image_pack: a packed file of the save table, or a raw R,G,B / R,G,B,255 packing (RTC_IMAGE_RAW_*)
rtc_status rtc_image_pack_enqueue(PackScratch *&sc, uint32_t format, const uint8_t *d_pixels, uint32_t width, uint32_t height,
                                  uint32_t channels, hipStream_t s, RtcEncoded *e);
void rtc_image_pack_release(PackScratch *sc);

// The scratch of every chain, each created on first use, all released together (rtc_encode.cpp).
struct RtcEncoder {
    GifScratch *gif = nullptr;
    JpegScratch *jpeg = nullptr;
    PngScratch *png = nullptr;
    PackScratch *pack = nullptr;

    // enqueue `job` for the frame at d_pixels on `s`
    rtc_status enqueue(const RtcEncodeJob &job, const void *d_pixels, uint32_t width, uint32_t height, uint32_t channels, hipStream_t s,
                       RtcEncoded *e);
    void release();
};

#endif
