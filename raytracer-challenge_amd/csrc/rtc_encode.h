// rtc_encode.h — the one internal interface of the device file writers (rtc_gif.hip, rtc_jpeg.hip, rtc_png.hip,
// rtc_image.hip, rtc_float.hip), used by the encoder objects (rtc_encode.cpp) and the Lua lane loop (rtc_lua_render.cpp). Not part of the
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
#include "rtc_devmem.h"

// What to produce from a frame in device memory.
struct RtcEncodeJob {
    enum Kind : uint32_t { GIF_RECORD, JPEG, PNG, SAVED, FLOAT } kind = GIF_RECORD;
    int32_t quality = 0; // JPEG
    uint32_t format = 0; // SAVED: the save table's RTC_IMAGE_* format; FLOAT: the float table's RTC_FLOAT_*
    // FLOAT: the frame is the f64 canvas (height*width*3 doubles, or null for an EXR of planes only); EXR's type for its
    // R, G, B and the AOV planes to store beside them (device pointers, null = none)
    uint32_t rgb_type = RTC_EXR_HALF;
    rtc_aov_buffers aov = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
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

// Each chain's grow-only scratch: one device block, carved by its reserve() (in the chain's file) when an enqueue needs
// more. The info records are of the chain's own types.
struct GifScratch {
    size_t px_cap = 0;      // pixels the buffers below are sized for
    DevBuf<uint8_t> block;  // the parts cleared per frame first
    uint32_t *bitmap = nullptr, *cnt = nullptr, *pal32 = nullptr;
    unsigned long long *boxsum = nullptr;
    size_t clear_bytes = 0;
    uint32_t *blockcnt = nullptr;
    void *info = nullptr; // GifInfo
    uint8_t *lut = nullptr, *idx = nullptr, *seg = nullptr, *record = nullptr;
    uint32_t *seglen = nullptr;
    unsigned long long *segoff = nullptr;
    size_t record_cap = 0;
    rtc_status reserve(size_t n);
};
struct JpegScratch {
    size_t mcu_cap = 0;
    DevBuf<uint8_t> block;
    int16_t *coef = nullptr;
    uint32_t *acbits = nullptr, *mcu_off = nullptr, *ffcnt = nullptr;
    int32_t *dc = nullptr;
    unsigned long long *group = nullptr, *words = nullptr, *chunk_off = nullptr;
    void *info = nullptr; // JpegInfo
    uint8_t *out = nullptr;
    size_t nwords = 0, data_max = 0; // the packed stream's buffer: words, and its worst case in bytes
    rtc_status reserve(size_t nmcu);
};
struct PngScratch {
    size_t n_cap = 0;
    DevBuf<uint8_t> block;
    uint8_t *filt = nullptr, *out = nullptr;
    uint16_t *prev = nullptr; // then T, the token flags
    uint32_t *M = nullptr;
    unsigned long long *words = nullptr, *chunk_off = nullptr;
    void *info = nullptr, *pinfo = nullptr; // SegInfo[], PngInfo
    size_t out_cap = 0;
    rtc_status reserve(size_t n);
};
struct PackScratch {
    DevBuf<uint8_t> out, d_hdr;
    uint8_t *h_hdr = nullptr; // d_hdr's page-locked source (the upload is asynchronous; the source stays until the next file)
    size_t hdr_cap = 0;
    DevBuf<unsigned long long> d_len;
    rtc_status header(size_t bytes);
    ~PackScratch();
};

struct FloatScratch {
    PackScratch pack;                // the file, the header (with EXR's channel table behind it) and the length
    DevBuf<uint8_t> planes;          // RLE HDR: the R, G, B, E byte planes of every row
    DevBuf<uint32_t> sizes;          // ... the coded size of each of the 4h row-planes
    DevBuf<unsigned long long> offs; // ... and where each starts in the file
};

// The chains, their arguments checked by the callers. The input is height*width*channels bytes (GIF: channels 3).
rtc_status rtc_gif_enqueue(GifScratch &sc, const uint8_t *d_rgb8, uint32_t width, uint32_t height, hipStream_t s, RtcEncoded *e);
rtc_status rtc_jpeg_enqueue(JpegScratch &sc, const uint8_t *d_pixels, uint32_t width, uint32_t height, uint32_t channels,
                            int32_t quality, hipStream_t s, RtcEncoded *e);
rtc_status rtc_png_enqueue(PngScratch &sc, const uint8_t *d_pixels, uint32_t width, uint32_t height, uint32_t channels,
                           hipStream_t s, RtcEncoded *e);
// k_image_pack: a packed file of the save table, or a raw R,G,B / R,G,B,255 packing (RTC_IMAGE_RAW_*)
rtc_status rtc_image_pack_enqueue(PackScratch &sc, uint32_t format, const uint8_t *d_pixels, uint32_t width, uint32_t height,
                                  uint32_t channels, hipStream_t s, RtcEncoded *e);

// rtc_float.hip: a float file (RTC_FLOAT_*) of the planes at d (device pointers)
rtc_status rtc_float_enqueue(FloatScratch &sc, uint32_t format, const rtc_float_planes *d, uint32_t width, uint32_t height, hipStream_t s,
                             RtcEncoded *e);

// The scratch of every chain. Its owner makes its device current and waits for its streams before letting it go.
struct RtcEncoder {
    GifScratch gif;
    JpegScratch jpeg;
    PngScratch png;
    PackScratch pack;
    FloatScratch flt;

    // enqueue `job` for the frame at d_pixels on `s`
    rtc_status enqueue(const RtcEncodeJob &job, const void *d_pixels, uint32_t width, uint32_t height, uint32_t channels, hipStream_t s,
                       RtcEncoded *e);
};

#endif
