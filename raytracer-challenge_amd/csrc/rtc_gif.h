// rtc_gif.h — constants of the GIF writer shared by its host statement (host_gif.cpp) and the device pipeline
// (rtc_gif.hip). Not part of the ABI; the rules themselves are in include/rtc.h.
#ifndef RTC_GIF_H
#define RTC_GIF_H

#include <cstddef>
#include <cstdint>
#include <vector>

enum {
    RTC_GIF_BINS = 32768,      // (r>>3, g>>3, b>>3)
    RTC_GIF_CLEAR = 256,
    RTC_GIF_EOI = 257,
    RTC_GIF_FIRST_CODE = 258,
    RTC_GIF_FILE_HEADER = 13,  // "GIF89a" + logical screen descriptor
    RTC_GIF_RECORD_HEADER = 8 + 10 + 768 + 1, // graphic control extension, image descriptor, local table, min code size
    RTC_GIF_LCT_OFFSET = 18,
    // worst-case bytes of one segment's codes: at most S + 3 codes (the leading clear, one clear when the dictionary
    // fills — it takes 3838 codes, so once per segment — and the terminator) of at most 12 bits, rounded up to words
    RTC_GIF_SEG_BYTES = ((4096 + 3) * 12 / 8 + 3) / 4 * 4 + 8,
};

// the 13 bytes in front of the first frame / the 787 bytes in front of a frame's sub-blocks (table left for the caller)
extern "C" void rtc_gif_file_header(uint8_t *hdr, uint32_t width, uint32_t height);
extern "C" void rtc_gif_record_header(uint8_t *hdr, uint32_t width, uint32_t height);
// one frame's record (extension + descriptor + table + sub-blocks + terminator) appended to `out`; 0 on bad arguments
size_t rtc_gif_format_record(const uint8_t *rgb8, uint32_t width, uint32_t height, std::vector<uint8_t> &out);

#endif
