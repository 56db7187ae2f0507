// rtc_image.h — the save-by-name writer's layouts, shared by its host statement (host_image.cpp) and the device pipeline
// (rtc_image.hip). Not part of the ABI; the rules themselves are in include/rtc.h.
#ifndef RTC_IMAGE_H
#define RTC_IMAGE_H

#include <cstddef>
#include <cstdint>

#include "rtc.h"

enum {
    // internal packings of the device pipeline, beside the RTC_IMAGE_* files: the frame's R,G,B or R,G,B,255 bytes with no
    // header (the input of the GIF and PNG chains, of ICO's PNG, and the rows of a PPM)
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

#endif
