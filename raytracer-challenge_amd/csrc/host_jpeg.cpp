// host_jpeg.cpp — [host] the JPEG writer of include/rtc.h (Canvas::write_to_file for ".jpg" names, canvas.rs:80-84):
// baseline, 4:4:4, the Annex K tables at a libjpeg quality, the integer DCT and quantiser of rtc_jpeg.h, entropy coding
// written serially. This file is the statement: rtc_jpeg.hip produces the same bytes on the device.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtc.h"
#include "rtc_jpeg.h"

namespace {

bool args_ok(const uint8_t *pixels, uint32_t w, uint32_t h, uint32_t channels, int32_t quality) {
    return pixels && w >= 1 && w <= 65535u && h >= 1 && h <= 65535u && (channels == 3 || channels == 4) && quality >= 1 &&
           quality <= 100;
}

// The quantised blocks of MCU (mx, my): Y, Cb, Cr, natural order; edge pixels replicated.
void mcu_coefficients(const uint8_t *pixels, uint32_t w, uint32_t h, uint32_t channels, const uint32_t q[128], uint32_t mx,
                      uint32_t my, int16_t out[192]) {
    uint32_t s[3][64];
    for (uint32_t i = 0; i < 64; ++i) {
        const uint32_t x = std::min(mx * 8 + (i & 7u), w - 1), y = std::min(my * 8 + (i >> 3), h - 1);
        const uint8_t *p = pixels + ((size_t)y * w + x) * channels;
        uint32_t ycc[3];
        rtc_jpeg_ycc(p[0], p[1], p[2], ycc);
        for (int c = 0; c < 3; ++c) s[c][i] = ycc[c];
    }
    for (int c = 0; c < 3; ++c) {
        int32_t d[64];
        rtc_jpeg_fdct_block(s[c], d);
        for (int i = 0; i < 64; ++i) out[64 * c + i] = (int16_t)rtc_jpeg_quantise(d[i], (int32_t)q[64 * (c ? 1 : 0) + i]);
    }
}

struct BitWriter { // MSB-first, 0xFF followed by 0x00
    std::vector<uint8_t> &out;
    uint64_t acc = 0;
    int bits = 0;
    void byte(uint8_t b) {
        out.push_back(b);
        if (b == 0xFF) out.push_back(0);
    }
    void put(uint64_t code, uint32_t len) { // len <= 59
        for (uint32_t k = len; k > 0;) {
            const uint32_t take = std::min<uint32_t>(k, 32u);
            k -= take;
            acc = (acc << take) | ((code >> k) & ((1ull << take) - 1));
            bits += (int)take;
            while (bits >= 8) { bits -= 8; byte((uint8_t)(acc >> bits)); }
        }
    }
    void flush() { // pad with 1-bits
        if (bits > 0) put((1ull << (8 - bits)) - 1, (uint32_t)(8 - bits));
    }
};

void put16(std::vector<uint8_t> &o, uint32_t v) { o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v); }

} // namespace

// SOI .. SOS: RTC_JPEG_HEADER_BYTES bytes, fixed for a size and quality
extern "C" void rtc_jpeg_header(uint32_t w, uint32_t h, int32_t quality, uint8_t *hdr) {
    std::vector<uint8_t> o;
    o.reserve(RTC_JPEG_HEADER_BYTES);
    const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 2, 0, 0, 1, 0, 1, 0, 0};
    o.insert(o.end(), app0, app0 + sizeof app0);
    for (int t = 0; t < 2; ++t) {
        const uint8_t dqt[] = {0xFF, 0xDB, 0x00, 67, (uint8_t)t};
        o.insert(o.end(), dqt, dqt + sizeof dqt);
        for (int k = 0; k < 64; ++k) o.push_back((uint8_t)rtc_jpeg_quant_entry(quality, t, kJpegZigzag[k]));
    }
    const uint8_t sof[] = {0xFF, 0xC0, 0x00, 17, 8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, 3,
                           1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1};
    o.insert(o.end(), sof, sof + sizeof sof);
    for (int t = 0; t < 4; ++t) { // DC0, AC0, DC1, AC1
        const int c = t >> 1, ac = t & 1;
        const uint8_t *bits = ac ? kJpegAcBits[c] : kJpegDcBits[c];
        const uint8_t *vals = ac ? kJpegAcVals[c] : kJpegDcVals;
        uint32_t n = 0;
        for (int i = 0; i < 16; ++i) n += bits[i];
        o.push_back(0xFF); o.push_back(0xC4);
        put16(o, 2 + 1 + 16 + n);
        o.push_back((uint8_t)((ac << 4) | c));
        o.insert(o.end(), bits, bits + 16);
        o.insert(o.end(), vals, vals + n);
    }
    const uint8_t sos[] = {0xFF, 0xDA, 0x00, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    o.insert(o.end(), sos, sos + sizeof sos);
    std::memcpy(hdr, o.data(), RTC_JPEG_HEADER_BYTES);
}

rtc_status rtc_jpeg_quant_tables(int32_t quality, uint16_t *out) {
    if (!out || quality < 1 || quality > 100) return RTC_ERR_ARG;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) out[64 * t + i] = (uint16_t)rtc_jpeg_quant_entry(quality, t, i);
    return RTC_OK;
}

rtc_status rtc_jpeg_fdct(const uint8_t *samples, int32_t *out) {
    if (!samples || !out) return RTC_ERR_ARG;
    uint32_t s[64];
    for (int i = 0; i < 64; ++i) s[i] = samples[i];
    rtc_jpeg_fdct_block(s, out);
    return RTC_OK;
}

rtc_status rtc_jpeg_coefficients(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, int32_t quality,
                                 int16_t *out) {
    if (!args_ok(pixels, width, height, channels, quality) || !out) return RTC_ERR_ARG;
    uint32_t q[128];
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) q[64 * t + i] = rtc_jpeg_quant_entry(quality, t, i);
    const uint32_t mw = (width + 7) / 8, mh = (height + 7) / 8;
    for (uint32_t my = 0; my < mh; ++my)
        for (uint32_t mx = 0; mx < mw; ++mx) mcu_coefficients(pixels, width, height, channels, q, mx, my, out + ((size_t)my * mw + mx) * 192);
    return RTC_OK;
}

size_t rtc_jpeg_format(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, int32_t quality, uint8_t *buf,
                       size_t cap) {
    if (!args_ok(pixels, width, height, channels, quality)) return 0;
    std::vector<uint8_t> out(RTC_JPEG_HEADER_BYTES);
    rtc_jpeg_header(width, height, quality, out.data());
    uint32_t q[128];
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) q[64 * t + i] = rtc_jpeg_quant_entry(quality, t, i);
    BitWriter bw{out};
    int32_t pred[3] = {0, 0, 0};
    const uint32_t mw = (width + 7) / 8, mh = (height + 7) / 8;
    int16_t co[192];
    for (uint32_t my = 0; my < mh; ++my)
        for (uint32_t mx = 0; mx < mw; ++mx) {
            mcu_coefficients(pixels, width, height, channels, q, mx, my, co);
            for (int c = 0; c < 3; ++c) {
                const int chroma = c ? 1 : 0;
                const int16_t *b = co + 64 * c;
                uint64_t code;
                uint32_t len = rtc_jpeg_dc_code(chroma, b[0] - pred[c], &code);
                bw.put(code, len);
                pred[c] = b[0];
                uint32_t run = 0;
                for (int k = 1; k < 64; ++k) {
                    const int32_t v = b[kJpegZigzag[k]];
                    if (v == 0) { ++run; continue; }
                    len = rtc_jpeg_ac_code(chroma, run, v, &code);
                    bw.put(code, len);
                    run = 0;
                }
                if (run) {
                    len = rtc_jpeg_eob_code(chroma, &code);
                    bw.put(code, len);
                }
            }
        }
    bw.flush();
    out.push_back(0xFF);
    out.push_back(0xD9);
    if (buf) std::memcpy(buf, out.data(), std::min(cap, out.size()));
    return out.size();
}

rtc_status rtc_canvas_write_jpeg(const char *path, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                                 int32_t quality) {
    if (!path) return RTC_ERR_ARG;
    const size_t need = rtc_jpeg_format(pixels, width, height, channels, quality, nullptr, 0);
    if (need == 0) return RTC_ERR_ARG;
    std::vector<uint8_t> b(need);
    rtc_jpeg_format(pixels, width, height, channels, quality, b.data(), need);
    FILE *f = std::fopen(path, "wb");
    if (!f) return RTC_ERR_IO;
    const bool ok = std::fwrite(b.data(), 1, need, f) == need;
    return (std::fclose(f) == 0 && ok) ? RTC_OK : RTC_ERR_IO;
}
