// host_float.cpp — [host] the float file writers of include/rtc.h: Radiance HDR, PFM and OpenEXR from an f64 canvas and the
// AOV planes. The float extension table, the layouts (rtc_float_layout, shared with the device chain) and the serial
// statement of every byte, which rtc_float.hip matches. The conversions are rtc_float.h's, the same code on both sides.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rtc.h"
#include "rtc_float.h"

namespace {

void le32(uint8_t *p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k)); }
void le64(uint8_t *p, unsigned long long v) { for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k)); }

std::string text_header(uint32_t format, uint32_t w, uint32_t h) {
    if (format == RTC_FLOAT_PFM) return "PF\n" + std::to_string(w) + " " + std::to_string(h) + "\n-1.0\n";
    return "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y " + std::to_string(h) + " +X " + std::to_string(w) + "\n";
}

// EXR: magic, version, the attributes and their terminator (the offset table follows)
std::vector<uint8_t> exr_attributes(const RtcFloatLayout &L, const char *const *names, uint32_t w, uint32_t h) {
    std::vector<uint8_t> v = {0x76, 0x2F, 0x31, 0x01, 2, 0, 0, 0};
    auto str = [&](const char *s) { v.insert(v.end(), s, s + std::strlen(s) + 1); };
    auto i32 = [&](uint32_t x) { for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k))); };
    auto attr = [&](const char *name, const char *type, uint32_t size) { str(name); str(type); i32(size); };
    uint32_t chlist = 1;
    for (uint32_t c = 0; c < L.n_channels; ++c) chlist += (uint32_t)std::strlen(names[c]) + 1 + 16;
    attr("channels", "chlist", chlist);
    for (uint32_t c = 0; c < L.n_channels; ++c) {
        str(names[c]);
        i32(L.ch[c].type);
        i32(0); // pLinear and three reserved bytes
        i32(1);
        i32(1);
    }
    v.push_back(0);
    attr("compression", "compression", 1);
    v.push_back(0);
    for (const char *name : {"dataWindow", "displayWindow"}) {
        attr(name, "box2i", 16);
        i32(0); i32(0); i32(w - 1); i32(h - 1);
    }
    attr("lineOrder", "lineOrder", 1);
    v.push_back(0);
    attr("pixelAspectRatio", "float", 4);
    i32(0x3F800000u);
    attr("screenWindowCenter", "v2f", 8);
    i32(0); i32(0);
    attr("screenWindowWidth", "float", 4);
    i32(0x3F800000u);
    v.push_back(0);
    return v;
}

// One plane of one row, by the maximal-run rule; returns the bytes needed and writes at most cap.
size_t rle_plane(const uint8_t *b, uint32_t w, uint8_t *out, size_t cap) {
    size_t n = 0;
    auto put = [&](uint8_t v) { if (out && n < cap) out[n] = v; ++n; };
    uint32_t lit = 0; // where the pending literal stretch starts
    auto flush = [&](uint32_t end) {
        for (uint32_t s = lit; s < end; s += 128) {
            const uint32_t cnt = std::min<uint32_t>(128, end - s);
            put((uint8_t)cnt);
            for (uint32_t j = 0; j < cnt; ++j) put(b[s + j]);
        }
    };
    for (uint32_t i = 0; i < w;) {
        uint32_t j = i + 1;
        while (j < w && b[j] == b[i]) ++j;
        if (j - i >= 4) {
            flush(i);
            for (uint32_t rest = j - i; rest > 0;) {
                const uint32_t cnt = std::min<uint32_t>(127, rest);
                put((uint8_t)(128 + cnt));
                put(b[i]);
                rest -= cnt;
            }
            lit = j;
        }
        i = j;
    }
    flush(w);
    return n;
}

// the whole file; empty on bad arguments
std::vector<uint8_t> float_file(uint32_t format, const rtc_float_planes *p, uint32_t w, uint32_t h) {
    std::vector<uint8_t> f;
    RtcFloatLayout L;
    if (!rtc_float_layout(format, p, w, h, &L, nullptr)) return f;
    f.resize((size_t)L.file_bytes);
    rtc_float_layout(format, p, w, h, &L, f.data());
    uint8_t *o = f.data() + L.header;
    if (format == RTC_FLOAT_PFM) {
        for (uint32_t y = 0; y < h; ++y) {
            const double *row = p->rgb + (size_t)(h - 1 - y) * w * 3;
            for (size_t k = 0; k < (size_t)w * 3; ++k, o += 4) le32(o, rtc_f64_to_f32_bits(row[k]));
        }
    } else if (format == RTC_FLOAT_HDR) {
        std::vector<uint8_t> planes((size_t)w * 4);
        for (uint32_t y = 0; y < h; ++y) {
            const double *row = p->rgb + (size_t)y * w * 3;
            if (!rtc_hdr_is_rle(w)) {
                for (uint32_t x = 0; x < w; ++x, o += 4) le32(o, rtc_rgbe_bits(row[3 * x], row[3 * x + 1], row[3 * x + 2]));
                continue;
            }
            for (uint32_t x = 0; x < w; ++x) {
                const uint32_t v = rtc_rgbe_bits(row[3 * x], row[3 * x + 1], row[3 * x + 2]);
                for (uint32_t c = 0; c < 4; ++c) planes[(size_t)c * w + x] = (uint8_t)(v >> (8 * c));
            }
            *o++ = 2;
            *o++ = 2;
            *o++ = (uint8_t)(w >> 8);
            *o++ = (uint8_t)w;
            for (uint32_t c = 0; c < 4; ++c) o += rle_plane(planes.data() + (size_t)c * w, w, o, (size_t)(f.data() + f.size() - o));
        }
        f.resize((size_t)(o - f.data())); // file_bytes was the worst case
    } else {
        for (uint32_t y = 0; y < h; ++y) {
            le32(o, y);
            le32(o + 4, L.pixel_bytes * w);
            o += 8;
            for (uint32_t c = 0; c < L.n_channels; ++c)
                for (uint32_t x = 0; x < w; ++x) {
                    const uint32_t v = rtc_exr_value(L.ch[c], (size_t)y * w + x);
                    *o++ = (uint8_t)v;
                    *o++ = (uint8_t)(v >> 8);
                    if (L.ch[c].type != 1u) {
                        *o++ = (uint8_t)(v >> 16);
                        *o++ = (uint8_t)(v >> 24);
                    }
                }
        }
    }
    return f;
}

} // namespace

bool rtc_float_size_ok(uint32_t format, uint32_t w, uint32_t h) {
    return format <= RTC_FLOAT_EXR && w >= 1 && h >= 1 && w <= 65535u && h <= 65535u;
}

bool rtc_float_layout(uint32_t format, const rtc_float_planes *p, uint32_t w, uint32_t h, RtcFloatLayout *L, uint8_t *hdr) {
    if (!L || !p || !rtc_float_size_ok(format, w, h)) return false;
    *L = RtcFloatLayout{};
    const unsigned long long px = (unsigned long long)w * h;
    if (format != RTC_FLOAT_EXR) {
        if (!p->rgb) return false;
        const std::string s = text_header(format, w, h);
        L->header = (uint32_t)s.size();
        if (hdr) std::memcpy(hdr, s.data(), s.size());
        L->pixel_bytes = format == RTC_FLOAT_PFM ? 12u : 4u;
        L->file_bytes = L->header + (format == RTC_FLOAT_HDR && rtc_hdr_is_rle(w) ? (4ull + 4ull * rtc_hdr_plane_max(w)) * h : px * L->pixel_bytes);
        return true;
    }
    if (p->rgb && p->rgb_type != RTC_EXR_HALF && p->rgb_type != RTC_EXR_FLOAT) return false;
    // byte-wise alphabetical: B G N.X N.Y N.Z P.X P.Y P.Z R Z id shadow
    const char *names[RTC_EXR_MAX_CHANNELS];
    uint32_t n = 0;
    auto add = [&](const char *name, const void *src, uint32_t stride, uint32_t comp, uint32_t source, uint32_t type) {
        names[n] = name;
        L->ch[n++] = RtcExrChannel{src, stride, comp, source, type};
    };
    static const char *const N[3] = {"N.X", "N.Y", "N.Z"}, *const P[3] = {"P.X", "P.Y", "P.Z"};
    if (p->rgb) add("B", p->rgb, 3, 2, RTC_EXR_SRC_F64, p->rgb_type);
    if (p->rgb) add("G", p->rgb, 3, 1, RTC_EXR_SRC_F64, p->rgb_type);
    for (uint32_t k = 0; k < 3 && p->aov.normal; ++k) add(N[k], p->aov.normal, 3, k, RTC_EXR_SRC_F64, 2);
    for (uint32_t k = 0; k < 3 && p->aov.point; ++k) add(P[k], p->aov.point, 3, k, RTC_EXR_SRC_F64, 2);
    if (p->rgb) add("R", p->rgb, 3, 0, RTC_EXR_SRC_F64, p->rgb_type);
    if (p->aov.depth) add("Z", p->aov.depth, 1, 0, RTC_EXR_SRC_F64, 2);
    if (p->aov.index) add("id", p->aov.index, 1, 0, RTC_EXR_SRC_INDEX, 0);
    if (p->aov.shadow) add("shadow", p->aov.shadow, 1, 0, RTC_EXR_SRC_SHADOW, 0);
    if (n == 0) return false;
    L->n_channels = n;
    for (uint32_t c = 0; c < n; ++c) {
        L->ch_off[c] = L->pixel_bytes;
        L->pixel_bytes += L->ch[c].type == 1u ? 2u : 4u;
    }
    for (uint32_t c = n; c <= RTC_EXR_MAX_CHANNELS; ++c) L->ch_off[c] = L->pixel_bytes;
    const std::vector<uint8_t> a = exr_attributes(*L, names, w, h);
    L->header = (uint32_t)(a.size() + 8ull * h);
    const unsigned long long line = 8ull + (unsigned long long)L->pixel_bytes * w;
    L->file_bytes = L->header + line * h;
    if (hdr) {
        std::memcpy(hdr, a.data(), a.size());
        for (uint32_t y = 0; y < h; ++y) le64(hdr + a.size() + 8ull * y, L->header + line * y);
    }
    return true;
}

extern "C" {

rtc_status rtc_float_format_for_name(const char *name, uint32_t *format) {
    if (!name || !format) return RTC_ERR_ARG;
    const char *base = std::strrchr(name, '/');
    base = base ? base + 1 : name;
    const char *dot = std::strrchr(base, '.');
    if (!dot || dot == base) return RTC_ERR_UNSUPPORTED; // rtc_image_format_for_name's rule
    std::string ext(dot + 1);
    for (char &c : ext) c = (char)std::tolower((unsigned char)c);
    static const struct { const char *ext; uint32_t format; } table[] = {{"hdr", RTC_FLOAT_HDR}, {"pfm", RTC_FLOAT_PFM}, {"exr", RTC_FLOAT_EXR}};
    for (const auto &t : table)
        if (ext == t.ext) {
            *format = t.format;
            return RTC_OK;
        }
    return RTC_ERR_UNSUPPORTED;
}

size_t rtc_float_format(uint32_t format, const rtc_float_planes *p, uint32_t width, uint32_t height, uint8_t *buf, size_t cap) {
    const std::vector<uint8_t> f = float_file(format, p, width, height);
    if (buf && !f.empty()) std::memcpy(buf, f.data(), std::min(cap, f.size()));
    return f.size();
}

rtc_status rtc_canvas_save_f64(const char *path, const double *rgb, uint32_t width, uint32_t height) {
    uint32_t format = 0;
    const rtc_status st = rtc_float_format_for_name(path, &format);
    if (st != RTC_OK) return st;
    rtc_float_planes p{};
    p.rgb = rgb;
    p.rgb_type = RTC_EXR_HALF;
    const std::vector<uint8_t> f = float_file(format, &p, width, height);
    if (f.empty()) return RTC_ERR_ARG;
    std::FILE *fp = std::fopen(path, "wb");
    if (!fp) return RTC_ERR_IO;
    const bool ok = std::fwrite(f.data(), 1, f.size(), fp) == f.size();
    return (std::fclose(fp) == 0 && ok) ? RTC_OK : RTC_ERR_IO;
}

rtc_status rtc_hdr_rle_row(const uint8_t *plane, uint32_t width, uint8_t *out, size_t cap, size_t *n) {
    if (!plane || !n || width == 0) return RTC_ERR_ARG;
    *n = rle_plane(plane, width, out, cap);
    return RTC_OK;
}

} // extern "C"
