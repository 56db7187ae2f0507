// host_png.cpp — [host] the compressed PNG writer of include/rtc.h: row filters by the minimum sum of absolute
// differences, hash chains, the lazy parse, one deflate block per segment (stored, fixed or dynamic Huffman), one IDAT
// chunk per segment. This file is the statement, written serially: rtc_png.hip produces the same bytes on the device; the
// arithmetic both use is rtc_png.h.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "rtc.h"
#include "rtc_png.h"

namespace {

bool args_ok(const uint8_t *pixels, uint32_t w, uint32_t h, uint32_t channels) {
    return pixels && w >= 1 && w <= 65535u && h >= 1 && h <= 65535u && (channels == 3 || channels == 4);
}

void filter_rows(const uint8_t *px, uint32_t w, uint32_t h, uint32_t bpp, uint8_t *types, uint8_t *out) {
    const size_t row = (size_t)w * bpp;
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t *cur = px + (size_t)y * row, *up = y ? cur - row : nullptr;
        auto at = [&](uint32_t t, size_t x) {
            const uint32_t a = x >= bpp ? cur[x - bpp] : 0u, b = up ? up[x] : 0u, c = (up && x >= bpp) ? up[x - bpp] : 0u;
            return rtc_png_filter_byte(t, cur[x], a, b, c);
        };
        uint32_t best = 0;
        uint64_t best_sum = ~0ull;
        for (uint32_t t = 0; t < 5; ++t) {
            uint64_t sum = 0;
            for (size_t x = 0; x < row; ++x) sum += rtc_png_filter_cost(at(t, x));
            if (sum < best_sum) { best_sum = sum; best = t; }
        }
        if (types) types[y] = (uint8_t)best;
        if (out) {
            uint8_t *o = out + (size_t)y * (row + 1);
            o[0] = (uint8_t)best;
            for (size_t x = 0; x < row; ++x) o[1 + x] = (uint8_t)at(best, x);
        }
    }
}

struct BitWriter { // LSB first
    std::vector<uint8_t> &out;
    uint64_t acc = 0;
    uint32_t bits = 0;
    void operator()(uint64_t v, uint32_t n) { // n <= 48
        acc |= v << bits;
        bits += n;
        while (bits >= 8) { out.push_back((uint8_t)acc); acc >>= 8; bits -= 8; }
    }
    void align() { if (bits) (*this)(0, 8 - bits); }
};

struct Crc {
    uint32_t t[256];
    Crc() { for (uint32_t i = 0; i < 256; ++i) t[i] = rtc_png_crc_table(i); }
    uint32_t operator()(const uint8_t *p, size_t n) const {
        uint32_t c = 0xffffffffu;
        for (size_t i = 0; i < n; ++i) c = t[(c ^ p[i]) & 255u] ^ (c >> 8);
        return c ^ 0xffffffffu;
    }
};

void chunk(std::vector<uint8_t> &f, const char *type, const uint8_t *data, size_t n) {
    static const Crc crc;
    const size_t at = f.size();
    f.resize(at + 8);
    rtc_png_be32(&f[at], (uint32_t)n);
    std::memcpy(&f[at + 4], type, 4);
    f.insert(f.end(), data, data + n);
    f.resize(f.size() + 4);
    rtc_png_be32(&f[f.size() - 4], crc(&f[at + 4], n + 4));
}

// The whole file of a filtered stream s[0, n).
std::vector<uint8_t> encode(const uint8_t *s, size_t n, uint32_t w, uint32_t h, uint32_t channels) {
    // prev[p] = p - the nearest earlier position of p's hash (0 if none within the window)
    std::vector<uint16_t> prev(n, 0);
    std::vector<int64_t> head(RTC_PNG_HASH_SIZE, -1);
    for (size_t p = 0; p + 3 <= n; ++p) {
        const uint32_t hh = rtc_png_hash(s[p], s[p + 1], s[p + 2]);
        if (head[hh] >= 0 && p - (size_t)head[hh] <= RTC_PNG_WINDOW) prev[p] = (uint16_t)(p - (size_t)head[hh]);
        head[hh] = (int64_t)p;
    }
    std::vector<uint8_t> file(33);
    rtc_png_head(w, h, channels, file.data());
    file.resize(29);
    {
        std::vector<uint8_t> ihdr(file.begin() + 16, file.begin() + 29);
        file.resize(8);
        chunk(file, "IHDR", ihdr.data(), ihdr.size());
    }
    std::unique_ptr<PngPlan> plan(new PngPlan);
    std::unique_ptr<PngHuffWork> work(new PngHuffWork);
    std::vector<uint32_t> L(RTC_PNG_SEGMENT + 1), D(RTC_PNG_SEGMENT + 1);
    std::vector<uint8_t> data;
    const size_t nseg = (n + RTC_PNG_SEGMENT - 1) / RTC_PNG_SEGMENT;
    for (size_t g = 0; g < nseg; ++g) {
        const size_t s0 = g * RTC_PNG_SEGMENT, end = std::min(n, s0 + RTC_PNG_SEGMENT), m = end - s0;
        const bool last = g + 1 == nseg;
        for (size_t p = s0; p < end; ++p) L[p - s0] = rtc_png_match(s, n, prev.data(), p, end, &D[p - s0]);
        L[m] = 0;
        uint32_t lit[RTC_PNG_NLIT] = {0}, dist[RTC_PNG_NDIST] = {0};
        uint64_t extra = 0;
        std::vector<uint32_t> starts; // token start offsets
        for (size_t p = 0; p < m;) {
            starts.push_back((uint32_t)p);
            if (rtc_png_takes_match(L[p], L[p + 1])) {
                const uint32_t lc = rtc_png_len_code(L[p]), dc = rtc_png_dist_code(D[p]);
                ++lit[257 + lc];
                ++dist[dc];
                extra += rtc_png_len_extra(lc) + rtc_png_dist_extra(dc);
                p += L[p];
            } else {
                ++lit[s[s0 + p]];
                ++p;
            }
        }
        lit[256] = 1;
        rtc_png_plan(lit, dist, extra, (uint32_t)m, plan.get(), work.get());
        data.clear();
        if (g == 0) { data.push_back(0x78); data.push_back(0x9c); }
        BitWriter bw{data};
        rtc_png_block_header(*plan, last, (uint32_t)m, bw);
        if (plan->type == RTC_PNG_STORED) {
            for (size_t p = 0; p < m; ++p) bw(s[s0 + p], 8);
        } else {
            for (uint32_t p : starts) {
                uint32_t nb;
                const bool mt = rtc_png_takes_match(L[p], L[p + 1]);
                const uint64_t v = rtc_png_token_code(*plan, s[s0 + p], mt ? L[p] : 0u, mt ? D[p] : 0u, &nb);
                bw(v, nb);
            }
            bw(plan->lit_code[256], plan->lit_len[256]);
        }
        if (!last) {
            bw(0, 3);
            bw.align();
            bw(0xffff0000u, 32);
        }
        bw.align();
        if (last) {
            uint32_t a = 1, b = 0;
            for (size_t i = 0; i < n;) {
                const size_t k = std::min<size_t>(n - i, 5552);
                for (size_t j = 0; j < k; ++j) { a += s[i + j]; b += a; }
                a %= 65521u;
                b %= 65521u;
                i += k;
            }
            data.resize(data.size() + 4);
            rtc_png_be32(&data[data.size() - 4], (b << 16) | a);
        }
        chunk(file, "IDAT", data.data(), data.size());
    }
    chunk(file, "IEND", nullptr, 0);
    return file;
}

std::vector<uint8_t> png_file(const uint8_t *pixels, uint32_t w, uint32_t h, uint32_t channels) {
    const size_t n = ((size_t)w * channels + 1) * h;
    std::vector<uint8_t> s(n);
    filter_rows(pixels, w, h, channels, nullptr, s.data());
    return encode(s.data(), n, w, h, channels);
}

} // namespace

extern "C" {

rtc_status rtc_png_filter(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint8_t *types, uint8_t *filtered) {
    if (!args_ok(pixels, width, height, channels)) return RTC_ERR_ARG;
    filter_rows(pixels, width, height, channels, types, filtered);
    return RTC_OK;
}

size_t rtc_png_format(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint8_t *buf, size_t cap) {
    if (!args_ok(pixels, width, height, channels)) return 0;
    const std::vector<uint8_t> f = png_file(pixels, width, height, channels);
    if (buf) std::memcpy(buf, f.data(), std::min(cap, f.size()));
    return f.size();
}

rtc_status rtc_canvas_write_png(const char *path, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels) {
    if (!path || !args_ok(pixels, width, height, channels)) return RTC_ERR_ARG;
    const std::vector<uint8_t> f = png_file(pixels, width, height, channels);
    std::FILE *fp = std::fopen(path, "wb");
    if (!fp) return RTC_ERR_IO;
    const bool ok = std::fwrite(f.data(), 1, f.size(), fp) == f.size();
    return (std::fclose(fp) == 0 && ok) ? RTC_OK : RTC_ERR_IO;
}

} // extern "C"
