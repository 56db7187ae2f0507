// test_float_formats_asan.cpp — the float file writers' host code (csrc/host_float.cpp) under -fsanitize=address,undefined:
// rtc_hdr_rle_row and rtc_float_format over byte planes that sit on every decision of the run-length rule, each call with a
// heap buffer of exactly `cap` bytes and cap one byte short of the file, so a write past cap is a heap overflow the
// sanitizer reports. Host code only: no GPU, no Python.
//
// usage: test_float_formats_asan PLANES   — PLANES: records of u32 width (little-endian) + width bytes
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rtc.h"

static int fail(const char *what, size_t k) {
    std::printf("FAIL %s (plane %zu)\n", what, k);
    return 1;
}

// rtc_float_format with cap = need - 1 into a buffer of exactly that size, then whole; both must agree on what they share
static bool file_short_and_whole(uint32_t format, const rtc_float_planes *p, uint32_t w, uint32_t h, std::vector<uint8_t> *whole) {
    const size_t need = rtc_float_format(format, p, w, h, nullptr, 0);
    if (need == 0) return false;
    uint8_t *tight = static_cast<uint8_t *>(std::malloc(need - 1 ? need - 1 : 1));
    if (rtc_float_format(format, p, w, h, tight, need - 1) != need) return false;
    whole->assign(need, 0);
    if (rtc_float_format(format, p, w, h, whole->data(), need) != need) return false;
    const bool same = std::memcmp(tight, whole->data(), need - 1) == 0;
    std::free(tight);
    return same;
}

int main(int argc, char **argv) {
    if (argc < 2) return fail("usage", 0);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return fail("open", 0);
    std::vector<std::vector<uint8_t>> planes;
    for (uint8_t head[4]; std::fread(head, 1, 4, f) == 4;) {
        const uint32_t w = head[0] | head[1] << 8 | head[2] << 16 | (uint32_t)head[3] << 24;
        std::vector<uint8_t> p(w);
        if (std::fread(p.data(), 1, w, f) != w) return fail("read", planes.size());
        planes.push_back(p);
    }
    std::fclose(f);
    size_t files = 0;
    for (size_t k = 0; k < planes.size(); ++k) {
        const std::vector<uint8_t> &p = planes[k];
        const uint32_t w = (uint32_t)p.size();
        size_t need = 0, again = 0;
        if (rtc_hdr_rle_row(p.data(), w, nullptr, 0, &need) != RTC_OK || need == 0) return fail("rtc_hdr_rle_row size", k);
        if (need > (size_t)w + (w + 127) / 128) return fail("the w + ceil(w / 128) bound", k);
        uint8_t *tight = static_cast<uint8_t *>(std::malloc(need - 1 ? need - 1 : 1));
        if (rtc_hdr_rle_row(p.data(), w, tight, need - 1, &again) != RTC_OK || again != need) return fail("rtc_hdr_rle_row short", k);
        std::vector<uint8_t> whole(need);
        if (rtc_hdr_rle_row(p.data(), w, whole.data(), need, &again) != RTC_OK || again != need) return fail("rtc_hdr_rle_row", k);
        if (std::memcmp(tight, whole.data(), need - 1) != 0) return fail("short and whole differ", k);
        std::free(tight);
        // the plane as the R, G and B bytes of a canvas (byte * 2^(130 - 136), the other mantissas 255), and planes from it
        const uint32_t h = 3;
        std::vector<double> rgb((size_t)w * h * 3), depth((size_t)w * h), vec((size_t)w * h * 3);
        std::vector<int32_t> index((size_t)w * h);
        std::vector<uint16_t> shadow((size_t)w * h);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                const size_t i = (size_t)y * w + x;
                for (uint32_t c = 0; c < 3; ++c) rgb[i * 3 + c] = std::ldexp(c == y ? (double)p[x] : 255.0, -6);
                depth[i] = p[x] ? (double)p[x] : INFINITY;
                vec[i * 3] = p[x] * 1e38;
                vec[i * 3 + 1] = -1e-46 * p[x];
                vec[i * 3 + 2] = p[x] ? 1.0 / p[x] : NAN;
                index[i] = (int32_t)p[x] - 1;
                shadow[i] = (uint16_t)(p[x] * 257u);
            }
        rtc_float_planes fp;
        std::memset(&fp, 0, sizeof fp);
        fp.rgb = rgb.data();
        fp.rgb_type = RTC_EXR_HALF;
        std::vector<uint8_t> file;
        for (uint32_t format : {RTC_FLOAT_HDR, RTC_FLOAT_PFM, RTC_FLOAT_EXR}) {
            if (!file_short_and_whole(format, &fp, w, h, &file)) return fail("rtc_float_format", k);
            ++files;
        }
        fp.aov.depth = depth.data();
        fp.aov.point = vec.data();
        fp.aov.normal = vec.data();
        fp.aov.index = index.data();
        fp.aov.shadow = shadow.data();
        fp.rgb_type = RTC_EXR_FLOAT;
        if (!file_short_and_whole(RTC_FLOAT_EXR, &fp, w, h, &file)) return fail("rtc_float_format, all channels", k);
        fp.rgb = nullptr;
        if (!file_short_and_whole(RTC_FLOAT_EXR, &fp, w, h, &file)) return fail("rtc_float_format, planes only", k);
        files += 2;
        // the flat branch (width 7) and one pixel
        if (w >= 7) {
            fp.rgb = rgb.data();
            if (!file_short_and_whole(RTC_FLOAT_HDR, &fp, 7, 2, &file) || !file_short_and_whole(RTC_FLOAT_PFM, &fp, 1, 1, &file)) return fail("small files", k);
            files += 2;
        }
    }
    // bad arguments write nothing
    uint8_t one = 0;
    size_t n = 0;
    rtc_float_planes none;
    std::memset(&none, 0, sizeof none);
    if (rtc_float_format(RTC_FLOAT_EXR, &none, 4, 4, &one, 1) != 0 || rtc_float_format(RTC_FLOAT_HDR, &none, 4, 4, &one, 1) != 0 ||
        rtc_float_format(3, &none, 4, 4, &one, 1) != 0 || rtc_hdr_rle_row(nullptr, 4, &one, 1, &n) != RTC_ERR_ARG ||
        rtc_hdr_rle_row(&one, 0, &one, 1, &n) != RTC_ERR_ARG)
        return fail("bad arguments", 0);
    std::printf("no crash: %zu planes, %zu files\n", planes.size(), files);
    return 0;
}
