// host_gif.cpp — [host] the animated-GIF writer behind StartAnimation / AddFrame (lua.rs:17-45,75-79,
// Canvas::frame_to_file canvas.rs:53-59): the project's own deterministic quantiser (exact palette or median cut,
// include/rtc.h) and the segmented LZW stream rtc_gif.hip produces on the device. This file is the statement of both:
// the device output is compared with it byte for byte.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rtc.h"
#include "rtc_gif.h"

namespace {

inline uint32_t bin_of(const uint8_t *p) { return ((uint32_t)(p[0] >> 3) << 10) | ((uint32_t)(p[1] >> 3) << 5) | (uint32_t)(p[2] >> 3); }
inline int bin_coord(uint32_t bin, int axis) { return (int)((bin >> (10 - 5 * axis)) & 31u); }

struct Box {
    int lo[3], hi[3];
    uint64_t n;
};

// Shrink box `b` to the bounding box of its occupied bins and count its pixels.
void box_bounds(Box &box, uint32_t b, const std::vector<uint32_t> &occ, const std::vector<uint8_t> &owner, const std::vector<uint32_t> &cnt) {
    for (int a = 0; a < 3; ++a) { box.lo[a] = 31; box.hi[a] = 0; }
    box.n = 0;
    for (size_t e = 0; e < occ.size(); ++e) {
        if (owner[e] != b) continue;
        for (int a = 0; a < 3; ++a) {
            const int c = bin_coord(occ[e], a);
            box.lo[a] = std::min(box.lo[a], c);
            box.hi[a] = std::max(box.hi[a], c);
        }
        box.n += cnt[occ[e]];
    }
}

// Median cut over the 32768 bins (include/rtc.h); palette entries in box-creation order; returns the number of boxes.
uint32_t median_cut(const uint8_t *rgb8, size_t n, uint8_t *pal) {
    std::vector<uint32_t> cnt(RTC_GIF_BINS, 0);
    std::vector<uint64_t> sum((size_t)3 * RTC_GIF_BINS, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *p = rgb8 + 3 * i;
        const uint32_t b = bin_of(p);
        ++cnt[b];
        for (int c = 0; c < 3; ++c) sum[(size_t)3 * b + c] += p[c];
    }
    std::vector<uint32_t> occ;
    for (uint32_t b = 0; b < RTC_GIF_BINS; ++b)
        if (cnt[b]) occ.push_back(b);
    std::vector<uint8_t> owner(occ.size(), 0);
    std::vector<Box> boxes(1);
    box_bounds(boxes[0], 0, occ, owner, cnt);
    while (boxes.size() < 256) {
        int best = -1;
        for (size_t i = 0; i < boxes.size(); ++i) {
            const Box &x = boxes[i];
            const bool splittable = x.hi[0] > x.lo[0] || x.hi[1] > x.lo[1] || x.hi[2] > x.lo[2];
            if (splittable && (best < 0 || x.n > boxes[best].n)) best = (int)i;
        }
        if (best < 0) break;
        const Box x = boxes[best];
        int axis = 0;
        for (int a = 1; a < 3; ++a)
            if (x.hi[a] - x.lo[a] > x.hi[axis] - x.lo[axis]) axis = a;
        uint64_t plane[32] = {0};
        for (size_t e = 0; e < occ.size(); ++e)
            if (owner[e] == (uint32_t)best) plane[bin_coord(occ[e], axis) - x.lo[axis]] += cnt[occ[e]];
        int cut = x.hi[axis] - 1;
        uint64_t cum = 0;
        for (int q = x.lo[axis]; q < x.hi[axis]; ++q) {
            cum += plane[q - x.lo[axis]];
            if (2 * cum >= x.n) { cut = q; break; }
        }
        const uint8_t nb = (uint8_t)boxes.size();
        for (size_t e = 0; e < occ.size(); ++e)
            if (owner[e] == (uint32_t)best && bin_coord(occ[e], axis) > cut) owner[e] = nb;
        boxes.emplace_back();
        box_bounds(boxes[best], (uint32_t)best, occ, owner, cnt);
        box_bounds(boxes.back(), nb, occ, owner, cnt);
    }
    std::vector<uint64_t> bs((size_t)3 * boxes.size(), 0);
    for (size_t e = 0; e < occ.size(); ++e)
        for (int c = 0; c < 3; ++c) bs[(size_t)3 * owner[e] + c] += sum[(size_t)3 * occ[e] + c];
    for (size_t i = 0; i < boxes.size(); ++i)
        for (int c = 0; c < 3; ++c) pal[3 * i + c] = (uint8_t)((2 * bs[3 * i + c] + boxes[i].n) / (2 * boxes[i].n));
    return (uint32_t)boxes.size();
}

// Segmented LZW (include/rtc.h): appends the codes of indices [0, n) LSB-first to `out`.
struct BitWriter {
    std::vector<uint8_t> &out;
    uint64_t acc = 0;
    int bits = 0;
    void put(uint32_t code, int width) {
        acc |= (uint64_t)code << bits;
        bits += width;
        while (bits >= 8) { out.push_back((uint8_t)acc); acc >>= 8; bits -= 8; }
    }
    void flush() { if (bits > 0) out.push_back((uint8_t)acc); acc = 0; bits = 0; }
};

void lzw_segment(const uint8_t *idx, size_t n, bool first, bool last, BitWriter &bw, std::vector<int16_t> &dict) {
    std::fill(dict.begin(), dict.end(), (int16_t)-1);
    int width = 9;
    uint32_t next = RTC_GIF_FIRST_CODE;
    if (first) bw.put(RTC_GIF_CLEAR, width);
    uint32_t prefix = idx[0];
    auto added = [&]() { // a code was emitted: the dictionary grows by one entry, or is full
        ++next;
        if (next > (1u << width) && width < 12) ++width;
    };
    for (size_t i = 1; i < n; ++i) {
        const uint32_t k = idx[i];
        const int16_t c = dict[(size_t)prefix * 256 + k];
        if (c >= 0) { prefix = (uint32_t)c; continue; }
        bw.put(prefix, width);
        if (next < 4096) {
            dict[(size_t)prefix * 256 + k] = (int16_t)next;
            added();
        } else {
            bw.put(RTC_GIF_CLEAR, width);
            std::fill(dict.begin(), dict.end(), (int16_t)-1);
            width = 9;
            next = RTC_GIF_FIRST_CODE;
        }
        prefix = k;
    }
    bw.put(prefix, width);
    if (next < 4096) added();
    bw.put(last ? RTC_GIF_EOI : RTC_GIF_CLEAR, width);
}

} // namespace

extern "C" void rtc_gif_record_header(uint8_t *hdr, uint32_t width, uint32_t height) {
    const uint8_t gce[8] = {0x21, 0xF9, 0x04, 0x00, (uint8_t)RTC_GIF_DELAY_CS, 0x00, 0x00, 0x00};
    std::memcpy(hdr, gce, 8);
    uint8_t *d = hdr + 8;
    d[0] = 0x2C;
    d[1] = d[2] = d[3] = d[4] = 0;
    d[5] = (uint8_t)width; d[6] = (uint8_t)(width >> 8);
    d[7] = (uint8_t)height; d[8] = (uint8_t)(height >> 8);
    d[9] = 0x87; // local colour table of 2^(7+1) entries, not interlaced
    hdr[RTC_GIF_RECORD_HEADER - 1] = 8; // LZW minimum code size (after the 768-byte table the caller fills)
}

extern "C" void rtc_gif_file_header(uint8_t *hdr, uint32_t width, uint32_t height) {
    const uint8_t sig[6] = {'G', 'I', 'F', '8', '9', 'a'};
    std::memcpy(hdr, sig, 6);
    hdr[6] = (uint8_t)width; hdr[7] = (uint8_t)(width >> 8);
    hdr[8] = (uint8_t)height; hdr[9] = (uint8_t)(height >> 8);
    hdr[10] = hdr[11] = hdr[12] = 0; // no global colour table, background 0, no aspect ratio
}

rtc_status rtc_gif_quantize(const uint8_t *rgb8, uint32_t width, uint32_t height, uint8_t *palette, uint8_t *indices, uint32_t *used) {
    if (!rgb8 || !palette || !indices || width == 0 || height == 0) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    std::memset(palette, 0, 768);
    std::vector<uint64_t> present((size_t)1 << 18, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t *p = rgb8 + 3 * i;
        const uint32_t c = ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
        present[c >> 6] |= 1ull << (c & 63);
    }
    uint64_t distinct = 0;
    for (uint64_t w : present) distinct += (uint64_t)__builtin_popcountll(w);
    uint32_t k = 0;
    if (distinct <= 256) { // exact: the colours in ascending order
        for (size_t w = 0; w < present.size(); ++w)
            for (uint64_t m = present[w]; m; m &= m - 1) {
                const uint32_t c = (uint32_t)(w * 64 + (size_t)__builtin_ctzll(m));
                palette[3 * k] = (uint8_t)(c >> 16); palette[3 * k + 1] = (uint8_t)(c >> 8); palette[3 * k + 2] = (uint8_t)c;
                ++k;
            }
    } else {
        k = median_cut(rgb8, n, palette);
    }
    if (used) *used = k;
    for (size_t i = 0; i < n; ++i) { // nearest entry of all 256, ties to the lowest index (the rank in the exact case)
        const uint8_t *p = rgb8 + 3 * i;
        int best = 0, bd = 1 << 30;
        for (int e = 0; e < 256; ++e) {
            const int dr = p[0] - palette[3 * e], dg = p[1] - palette[3 * e + 1], db = p[2] - palette[3 * e + 2];
            const int d = dr * dr + dg * dg + db * db;
            if (d < bd) { bd = d; best = e; }
        }
        indices[i] = (uint8_t)best;
    }
    return RTC_OK;
}

size_t rtc_gif_lzw(const uint8_t *indices, size_t n, uint8_t *buf, size_t cap) {
    if (!indices || n == 0) return 0;
    std::vector<uint8_t> bytes;
    BitWriter bw{bytes};
    std::vector<int16_t> dict((size_t)4096 * 256);
    for (size_t s = 0; s < n; s += RTC_GIF_SEGMENT) {
        const size_t m = std::min<size_t>(RTC_GIF_SEGMENT, n - s);
        lzw_segment(indices + s, m, s == 0, s + m == n, bw, dict);
    }
    bw.flush();
    if (buf) std::memcpy(buf, bytes.data(), std::min(cap, bytes.size()));
    return bytes.size();
}

size_t rtc_gif_format_record(const uint8_t *rgb8, uint32_t width, uint32_t height, std::vector<uint8_t> &out) {
    std::vector<uint8_t> idx((size_t)width * height);
    uint8_t hdr[RTC_GIF_RECORD_HEADER];
    rtc_gif_record_header(hdr, width, height);
    if (rtc_gif_quantize(rgb8, width, height, hdr + 18, idx.data(), nullptr) != RTC_OK) return 0;
    const size_t d = rtc_gif_lzw(idx.data(), idx.size(), nullptr, 0);
    std::vector<uint8_t> data(d);
    rtc_gif_lzw(idx.data(), idx.size(), data.data(), d);
    out.insert(out.end(), hdr, hdr + RTC_GIF_RECORD_HEADER);
    for (size_t j = 0; j < d; j += 255) {
        const size_t len = std::min<size_t>(255, d - j);
        out.push_back((uint8_t)len);
        out.insert(out.end(), data.begin() + (ptrdiff_t)j, data.begin() + (ptrdiff_t)(j + len));
    }
    out.push_back(0);
    return out.size();
}

size_t rtc_gif_format(const uint8_t *frames, uint32_t nframes, uint32_t width, uint32_t height, uint8_t *buf, size_t cap) {
    if (!frames || nframes == 0 || width == 0 || height == 0 || width > 65535u || height > 65535u) return 0;
    std::vector<uint8_t> out(RTC_GIF_FILE_HEADER);
    rtc_gif_file_header(out.data(), width, height);
    const size_t frame_bytes = (size_t)3 * width * height;
    for (uint32_t f = 0; f < nframes; ++f)
        if (rtc_gif_format_record(frames + f * frame_bytes, width, height, out) == 0) return 0;
    out.push_back(0x3B);
    if (buf) std::memcpy(buf, out.data(), std::min(cap, out.size()));
    return out.size();
}
