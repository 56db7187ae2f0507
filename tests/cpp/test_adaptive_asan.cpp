// The host statements of edge-adaptive anti-aliasing (csrc/host_adaptive.cpp) under AddressSanitizer and UBSan: the canvas and
// the mask in heap buffers of exactly their sizes, over the sizes at which an index can go wrong — one pixel, one pixel wide or
// high, smaller than a neighbourhood, no multiple of anything (37 x 29) — in both modes, at every kind of threshold, with NaN
// and infinities in the canvas. Compiled and run by tests/test_host_adaptive.py; links nothing but host_adaptive.cpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "rtc.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static double rnd() { // xorshift64*, in [0, 1)
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (double)((state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            return 1;                                                        \
        }                                                                    \
    } while (0)

int main() {
    const uint32_t sizes[][2] = {{1, 1}, {5, 3}, {64, 1}, {1, 64}, {16, 16}, {17, 17}, {37, 29}, {70, 40}};
    const double inf = std::numeric_limits<double>::infinity();
    int runs = 0;
    for (const auto &sz : sizes) {
        const uint32_t w = sz[0], h = sz[1];
        const size_t n = (size_t)w * h;
        std::vector<double> rgb(3 * n);
        for (double &v : rgb) v = std::floor(rnd() * 4.0) * 0.25 + rnd() * 0.008;
        if (n > 2) {
            rgb[3] = std::numeric_limits<double>::quiet_NaN();
            rgb[7] = inf;
            rgb[3 * n - 1] = -inf;
        }
        for (uint32_t mode : {(uint32_t)RTC_MODE_RENDER, (uint32_t)RTC_MODE_RENDER_ASYNC})
            for (double threshold : {-1.0, 0.0, 0.01, 0.25, inf}) {
                std::vector<uint8_t> mask(n, 0x5A);
                uint64_t flagged = ~0ull, ones = 0;
                REQUIRE(rtc_adaptive_mask(rgb.data(), w, h, mode, threshold, mask.data(), &flagged) == RTC_OK);
                for (size_t i = 0; i < n; ++i) {
                    REQUIRE(mask[i] <= 1u);
                    ones += mask[i];
                    const uint32_t x = (uint32_t)(i % w), y = (uint32_t)(i / w);
                    if (mode == RTC_MODE_RENDER && (x + 1u == w || y + 1u == h)) REQUIRE(mask[i] == 0u); // outside the rendered area
                }
                REQUIRE(ones == flagged);
                if (threshold == inf) REQUIRE(flagged == 0);
                REQUIRE(rtc_adaptive_mask(rgb.data(), w, h, mode, threshold, mask.data(), nullptr) == RTC_OK);
                ++runs;
            }
        std::vector<uint8_t> mask(n);
        REQUIRE(rtc_adaptive_mask(rgb.data(), w, h, 2u, 0.01, mask.data(), nullptr) == RTC_ERR_ARG);
        REQUIRE(rtc_adaptive_mask(rgb.data(), w, h, RTC_MODE_RENDER, std::numeric_limits<double>::quiet_NaN(), mask.data(), nullptr) == RTC_ERR_ARG);
        REQUIRE(rtc_adaptive_mask(nullptr, w, h, RTC_MODE_RENDER, 0.01, mask.data(), nullptr) == RTC_ERR_ARG);
    }
    for (uint32_t us : {1u, 2u, 3u, 16u, 256u})
        for (uint32_t vs : {1u, 5u, 16u}) {
            const rtc_adaptive spec{0.01, us, vs, 0u, 0u};
            if ((uint64_t)us * vs > RTC_MAX_AA_SAMPLES) {
                REQUIRE(rtc_adaptive_validate(&spec) == RTC_ERR_ARG);
                continue;
            }
            REQUIRE(rtc_adaptive_validate(&spec) == RTC_OK);
            double xo = -1.0, yo = -1.0;
            for (uint32_t k = 0; k < us * vs; ++k) {
                REQUIRE(rtc_adaptive_offset(&spec, k, &xo, &yo) == RTC_OK);
                REQUIRE(xo > 0.0 && xo < 1.0 && yo > 0.0 && yo < 1.0);
            }
            REQUIRE(rtc_adaptive_offset(&spec, us * vs, &xo, &yo) == RTC_ERR_ARG);
            ++runs;
        }
    std::printf("no crash: %d runs\n", runs);
    return 0;
}
