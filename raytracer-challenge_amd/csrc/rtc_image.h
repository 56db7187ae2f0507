// rtc_image.h — the save-by-name writer's layouts, shared by its host statement (host_image.cpp) and the device pipeline
// (rtc_image.hip). Not part of the ABI; the rules themselves are in include/rtc.h.
#ifndef RTC_IMAGE_H
#define RTC_IMAGE_H

#include <cstddef>
#include <cstdint>

#include "rtc.h"

enum {
    // internal packings of the device pipeline, beside the RTC_IMAGE_* files: the frame's R,G,B or R,G,B,255 bytes with no
    // header (the input of the GIF / PNG / PPM chains, and of ICO's PNG)
    RTC_IMAGE_RAW_RGB = 100,
    RTC_IMAGE_RAW_RGBA = 101,
    RTC_ICO_HEADER_BYTES = 22,
    RTC_TIFF_HEADER_FIXED = 206, // header, IFD, BitsPerSample, X/YResolution
};

// One packed file (BMP, TGA, TIFF, farbfeld, PAM, or a raw packing): `header` bytes, then the pixels — rows top to bottom
// (bottom to top when `flip`), per pixel `bytes_per_pixel` bytes: R,G,B (3), R,G,B,255 (4; B,G,R,255 when `bgr`) or
// those four each written twice (8: farbfeld's big-endian v * 257).
struct RtcImageLayout {
    uint32_t header;
    uint32_t bytes_per_pixel;
    uint32_t bgr, flip;
    unsigned long long file_bytes;
};

// The layout of `format` for a width x height frame; false when `format` is not packed or the size is outside its limits.
// `hdr` (may be null) receives the header's L->header bytes.
bool rtc_image_layout(uint32_t format, uint32_t width, uint32_t height, RtcImageLayout *L, uint8_t *hdr);
// true when a width x height frame can be saved as `format` (the limits of include/rtc.h's table)
bool rtc_image_size_ok(uint32_t format, uint32_t width, uint32_t height);
// ICONDIR + ICONDIRENTRY for a PNG of png_bytes bytes
void rtc_image_ico_header(uint32_t width, uint32_t height, uint32_t png_bytes, uint8_t hdr[RTC_ICO_HEADER_BYTES]);

// The device pipeline (rtc_image.hip) as a scratch object for the Lua lane loop (rtc_gif.hip): encode enqueues the chain
// of one file on `stream`; the file (for PPM: the R,G,B rows the host prints) is then at data(), its length at the device
// address length().
struct ImageScratch;
ImageScratch *rtc_image_scratch_new();
void rtc_image_scratch_free(ImageScratch *sc);
int rtc_image_scratch_encode(ImageScratch *sc, uint32_t format, const void *d_pixels, uint32_t width, uint32_t height,
                             uint32_t channels, void *stream);
const uint8_t *rtc_image_scratch_data(const ImageScratch *sc);
size_t rtc_image_scratch_out_cap(const ImageScratch *sc);
const unsigned long long *rtc_image_scratch_length(const ImageScratch *sc);

// The GIF chain of rtc_gif.hip for one frame, as a scratch object (rtc_image.hip's GIF files): the record (not the file)
// is at record(), its length at the device address length().
struct GifFrameScratch;
GifFrameScratch *rtc_gif_scratch_new();
void rtc_gif_scratch_free(GifFrameScratch *sc);
int rtc_gif_scratch_encode(GifFrameScratch *sc, const void *d_rgb8, uint32_t width, uint32_t height, void *stream);
const uint8_t *rtc_gif_scratch_record(const GifFrameScratch *sc);
size_t rtc_gif_scratch_record_cap(const GifFrameScratch *sc);
const unsigned long long *rtc_gif_scratch_length(const GifFrameScratch *sc);

#endif
