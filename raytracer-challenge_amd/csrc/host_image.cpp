// host_image.cpp — [host] the save-by-name writer of include/rtc.h: the extension table, the packed layouts (BMP, TGA, TIFF,
// ICO's header, farbfeld, PAM) and rtc_image_format, which delegates PNG, JPEG, GIF and PPM to their own writers. This is
// the serial statement rtc_image.hip matches byte for byte; rtc_image_layout is shared by both.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rtc.h"
#include "rtc_image.h"

namespace {

void le16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
void le32(uint8_t *p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k)); }
void be32(uint8_t *p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (24 - 8 * k)); }

// TIFF's strips: rows per strip and strip count
void tiff_strips(uint32_t w, uint32_t h, uint32_t *rows, uint32_t *strips) {
    const unsigned long long per = std::max<unsigned long long>(1, RTC_TIFF_STRIP_BYTES / (4ull * w));
    *rows = (uint32_t)std::min<unsigned long long>(per, h);
    *strips = (uint32_t)((h + (unsigned long long)*rows - 1) / *rows);
}

std::string pam_header(uint32_t w, uint32_t h) {
    return "P7\nWIDTH " + std::to_string(w) + "\nHEIGHT " + std::to_string(h) + "\nDEPTH 4\nMAXVAL 255\nTUPLTYPE RGB_ALPHA\nENDHDR\n";
}

bool input_ok(const uint8_t *pixels, uint32_t w, uint32_t h, uint32_t channels) {
    return pixels && w >= 1 && h >= 1 && (channels == 3 || channels == 4) && (unsigned long long)w * h <= (1ull << 60);
}

// the frame's R,G,B (channels = 3) or R,G,B,255 (4) bytes
std::vector<uint8_t> repack(const uint8_t *pixels, uint32_t w, uint32_t h, uint32_t channels, uint32_t out_channels) {
    const size_t n = (size_t)w * h;
    std::vector<uint8_t> v(n * out_channels);
    for (size_t i = 0; i < n; ++i) {
        for (uint32_t k = 0; k < 3; ++k) v[i * out_channels + k] = pixels[i * channels + k];
        if (out_channels == 4) v[i * 4 + 3] = 255;
    }
    return v;
}

// the whole file of `format`; empty on bad arguments
std::vector<uint8_t> image_file(uint32_t format, const uint8_t *pixels, uint32_t w, uint32_t h, uint32_t channels) {
    std::vector<uint8_t> f;
    if (format > RTC_IMAGE_PAM || !input_ok(pixels, w, h, channels) || !rtc_image_size_ok(format, w, h)) return f;
    const uint8_t *rgb = pixels;
    std::vector<uint8_t> tmp;
    if (channels == 4 && (format == RTC_IMAGE_PNG || format == RTC_IMAGE_GIF || format == RTC_IMAGE_PPM)) {
        tmp = repack(pixels, w, h, 4, 3);
        rgb = tmp.data();
    }
    switch (format) {
    case RTC_IMAGE_PNG: {
        f.resize(rtc_png_format(rgb, w, h, 3, nullptr, 0));
        rtc_png_format(rgb, w, h, 3, f.data(), f.size());
        return f;
    }
    case RTC_IMAGE_JPEG: {
        f.resize(rtc_jpeg_format(pixels, w, h, channels, RTC_IMAGE_JPEG_QUALITY, nullptr, 0));
        rtc_jpeg_format(pixels, w, h, channels, RTC_IMAGE_JPEG_QUALITY, f.data(), f.size());
        return f;
    }
    case RTC_IMAGE_GIF: {
        f.resize(rtc_gif_format(rgb, 1, w, h, nullptr, 0));
        rtc_gif_format(rgb, 1, w, h, f.data(), f.size());
        return f;
    }
    case RTC_IMAGE_PPM: {
        f.resize(rtc_canvas_format_ppm_rgb8(rgb, w, h, nullptr, 0) + 1); // the formatter writes a NUL behind the text
        f.resize(rtc_canvas_format_ppm_rgb8(rgb, w, h, reinterpret_cast<char *>(f.data()), f.size()));
        return f;
    }
    case RTC_IMAGE_ICO: {
        const std::vector<uint8_t> rgba = channels == 4 ? repack(pixels, w, h, 4, 4) : repack(pixels, w, h, 3, 4);
        const size_t png = rtc_png_format(rgba.data(), w, h, 4, nullptr, 0);
        if (png == 0 || png > 0xffffffffull - RTC_ICO_HEADER_BYTES) return f;
        f.resize(RTC_ICO_HEADER_BYTES + png);
        rtc_image_ico_header(w, h, (uint32_t)png, f.data());
        rtc_png_format(rgba.data(), w, h, 4, f.data() + RTC_ICO_HEADER_BYTES, png);
        return f;
    }
    default: break;
    }
    RtcImageLayout L;
    if (!rtc_image_layout(format, w, h, &L, nullptr)) return f;
    f.resize((size_t)L.file_bytes);
    rtc_image_layout(format, w, h, &L, f.data());
    uint8_t *o = f.data() + L.header;
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t *row = pixels + (size_t)(L.flip ? h - 1 - y : y) * w * channels;
        for (uint32_t x = 0; x < w; ++x) {
            const uint8_t *p = row + (size_t)x * channels;
            const uint8_t px[4] = {L.bgr ? p[2] : p[0], p[1], L.bgr ? p[0] : p[2], 255};
            for (uint32_t k = 0; k < (L.bytes_per_pixel == 3 ? 3u : 4u); ++k) {
                *o++ = px[k];
                if (L.bytes_per_pixel == 8) *o++ = px[k];
            }
        }
    }
    return f;
}

} // namespace

bool rtc_image_size_ok(uint32_t format, uint32_t w, uint32_t h) {
    if (w == 0 || h == 0) return false;
    switch (format) {
    case RTC_IMAGE_PNG: case RTC_IMAGE_JPEG: case RTC_IMAGE_GIF: return w <= 65535u && h <= 65535u;
    case RTC_IMAGE_ICO: return w <= 256u && h <= 256u;
    case RTC_IMAGE_PPM: return (unsigned long long)w * h <= (1ull << 60);
    default: {
        RtcImageLayout L;
        return rtc_image_layout(format, w, h, &L, nullptr);
    }
    }
}

void rtc_image_ico_header(uint32_t w, uint32_t h, uint32_t png_bytes, uint8_t hdr[RTC_ICO_HEADER_BYTES]) {
    std::memset(hdr, 0, RTC_ICO_HEADER_BYTES);
    le16(hdr + 2, 1);
    le16(hdr + 4, 1);
    hdr[6] = (uint8_t)(w & 255u); // 256 -> 0
    hdr[7] = (uint8_t)(h & 255u);
    le16(hdr + 10, 1);
    le16(hdr + 12, 32);
    le32(hdr + 14, png_bytes);
    le32(hdr + 18, RTC_ICO_HEADER_BYTES);
}

bool rtc_image_layout(uint32_t format, uint32_t w, uint32_t h, RtcImageLayout *L, uint8_t *hdr) {
    if (!L || w == 0 || h == 0) return false;
    const unsigned long long px = (unsigned long long)w * h;
    if (px > (1ull << 60)) return false;
    *L = RtcImageLayout{0, 4, 0, 0, 0};
    switch (format) {
    case RTC_IMAGE_RAW_RGB:
        L->bytes_per_pixel = 3;
        break;
    case RTC_IMAGE_RAW_RGBA:
        break;
    case RTC_IMAGE_BMP: {
        if (w > 0x7fffffffu || h > 0x7fffffffu || 122ull + 4 * px > 0xffffffffull) return false;
        L->header = 122;
        L->bgr = L->flip = 1;
        if (hdr) {
            std::memset(hdr, 0, 122);
            hdr[0] = 'B';
            hdr[1] = 'M';
            le32(hdr + 2, (uint32_t)(122 + 4 * px));
            le32(hdr + 10, 122);
            le32(hdr + 14, 108);
            le32(hdr + 18, w);
            le32(hdr + 22, h);
            le16(hdr + 26, 1);
            le16(hdr + 28, 32);
            le32(hdr + 30, 3);
            le32(hdr + 34, (uint32_t)(4 * px));
            le32(hdr + 54, 0x00ff0000u);
            le32(hdr + 58, 0x0000ff00u);
            le32(hdr + 62, 0x000000ffu);
            le32(hdr + 66, 0xff000000u);
            le32(hdr + 70, 0x73524742u);
        }
        break;
    }
    case RTC_IMAGE_TGA: {
        if (w > 65535u || h > 65535u) return false;
        L->header = 18;
        L->bgr = 1;
        if (hdr) {
            std::memset(hdr, 0, 18);
            hdr[2] = 2;
            le16(hdr + 12, w);
            le16(hdr + 14, h);
            hdr[16] = 32;
            hdr[17] = 0x28;
        }
        break;
    }
    case RTC_IMAGE_TIFF: {
        uint32_t rows, strips;
        tiff_strips(w, h, &rows, &strips);
        const unsigned long long head = RTC_TIFF_HEADER_FIXED + (strips > 1 ? 8ull * strips : 0ull);
        if (head + 4 * px > 0xffffffffull) return false;
        L->header = (uint32_t)head;
        if (hdr) {
            std::memset(hdr, 0, (size_t)head);
            hdr[0] = hdr[1] = 'I';
            le16(hdr + 2, 42);
            le32(hdr + 4, 8);
            le16(hdr + 8, 14);
            uint8_t *e = hdr + 10;
            auto entry = [&](uint32_t tag, uint32_t type, uint32_t count, uint32_t value) {
                le16(e, tag);
                le16(e + 2, type);
                le32(e + 4, count);
                if (type == 3 && count == 1) le16(e + 8, value);
                else le32(e + 8, value);
                e += 12;
            };
            const uint32_t row_bytes = 4 * w;
            const uint32_t offs = strips > 1 ? RTC_TIFF_HEADER_FIXED : (uint32_t)head;
            const uint32_t cnts = strips > 1 ? RTC_TIFF_HEADER_FIXED + 4 * strips : row_bytes * h;
            entry(256, 4, 1, w);
            entry(257, 4, 1, h);
            entry(258, 3, 4, 182);
            entry(259, 3, 1, 1);
            entry(262, 3, 1, 2);
            entry(273, 4, strips, offs);
            entry(277, 3, 1, 4);
            entry(278, 4, 1, rows);
            entry(279, 4, strips, cnts);
            entry(282, 5, 1, 190);
            entry(283, 5, 1, 198);
            entry(284, 3, 1, 1);
            entry(296, 3, 1, 1);
            entry(338, 3, 1, 2);
            // next-IFD offset 0 at 178..181
            for (int k = 0; k < 4; ++k) le16(hdr + 182 + 2 * k, 8);
            le32(hdr + 190, 1);
            le32(hdr + 194, 1);
            le32(hdr + 198, 1);
            le32(hdr + 202, 1);
            if (strips > 1)
                for (uint32_t s = 0; s < strips; ++s) {
                    const uint32_t r = std::min(rows, h - s * rows);
                    le32(hdr + RTC_TIFF_HEADER_FIXED + 4 * s, (uint32_t)head + s * rows * row_bytes);
                    le32(hdr + RTC_TIFF_HEADER_FIXED + 4 * strips + 4 * s, r * row_bytes);
                }
        }
        break;
    }
    case RTC_IMAGE_FARBFELD: {
        L->header = 16;
        L->bytes_per_pixel = 8;
        if (hdr) {
            std::memcpy(hdr, "farbfeld", 8);
            be32(hdr + 8, w);
            be32(hdr + 12, h);
        }
        break;
    }
    case RTC_IMAGE_PAM: {
        const std::string s = pam_header(w, h);
        L->header = (uint32_t)s.size();
        if (hdr) std::memcpy(hdr, s.data(), s.size());
        break;
    }
    default: return false;
    }
    L->file_bytes = L->header + px * L->bytes_per_pixel;
    return true;
}

extern "C" {

rtc_status rtc_image_format_for_name(const char *name, uint32_t *format) {
    if (!name || !format) return RTC_ERR_ARG;
    const char *base = std::strrchr(name, '/');
    base = base ? base + 1 : name;
    const char *dot = std::strrchr(base, '.');
    if (!dot || dot == base) return RTC_ERR_UNSUPPORTED; // no '.', or a leading one only (Path::extension)
    std::string ext(dot + 1);
    for (char &c : ext) c = (char)std::tolower((unsigned char)c);
    static const struct { const char *ext; uint32_t format; } table[] = {
        {"png", RTC_IMAGE_PNG}, {"jpg", RTC_IMAGE_JPEG}, {"jpeg", RTC_IMAGE_JPEG}, {"gif", RTC_IMAGE_GIF}, {"ppm", RTC_IMAGE_PPM},
        {"bmp", RTC_IMAGE_BMP}, {"tga", RTC_IMAGE_TGA}, {"tif", RTC_IMAGE_TIFF}, {"tiff", RTC_IMAGE_TIFF}, {"ico", RTC_IMAGE_ICO},
        {"ff", RTC_IMAGE_FARBFELD}, {"pam", RTC_IMAGE_PAM}};
    for (const auto &t : table)
        if (ext == t.ext) {
            *format = t.format;
            return RTC_OK;
        }
    return RTC_ERR_UNSUPPORTED;
}

size_t rtc_image_format(uint32_t format, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint8_t *buf,
                        size_t cap) {
    const std::vector<uint8_t> f = image_file(format, pixels, width, height, channels);
    if (buf && !f.empty()) std::memcpy(buf, f.data(), std::min(cap, f.size()));
    return f.size();
}

rtc_status rtc_canvas_save(const char *path, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels) {
    uint32_t format = 0;
    const rtc_status st = rtc_image_format_for_name(path, &format);
    if (st != RTC_OK) return st;
    const std::vector<uint8_t> f = image_file(format, pixels, width, height, channels);
    if (f.empty()) return RTC_ERR_ARG;
    std::FILE *fp = std::fopen(path, "wb");
    if (!fp) return RTC_ERR_IO;
    const bool ok = std::fwrite(f.data(), 1, f.size(), fp) == f.size();
    return (std::fclose(fp) == 0 && ok) ? RTC_OK : RTC_ERR_IO;
}

} // extern "C"
