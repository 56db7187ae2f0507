// The host statement of the edge-aware filter (csrc/host_filter.cpp) under AddressSanitizer and UBSan: every plane in a heap
// buffer of exactly its size, over the sizes at which an index can go wrong — smaller than the two-tap halo, one pixel wide or
// high, steps as large as the image (16 x 16 and 17 x 17 at five passes), no multiple of anything (37 x 29) — with every pass
// count, both channel counts and both flag values, about a fifth of the pixels missing. Compiled and run by
// tests/test_host_filter.py; links nothing but host_filter.cpp.
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
    int runs = 0;
    for (const auto &sz : sizes) {
        const uint32_t w = sz[0], h = sz[1];
        const size_t n = (size_t)w * h;
        std::vector<int32_t> index(n);
        std::vector<double> point(3 * n), normal(3 * n);
        for (size_t i = 0; i < n; ++i) {
            index[i] = rnd() < 0.2 ? -1 : (int32_t)(rnd() * 4.0);
            double len = 0.0;
            for (int c = 0; c < 3; ++c) {
                point[3 * i + c] = rnd();
                normal[3 * i + c] = rnd() - 0.3;
                len += normal[3 * i + c] * normal[3 * i + c];
            }
            for (int c = 0; c < 3; ++c) normal[3 * i + c] /= std::sqrt(len);
        }
        if (n > 2) {
            normal[3] = std::numeric_limits<double>::quiet_NaN();
            point[6] = std::numeric_limits<double>::quiet_NaN();
        }
        rtc_aov_buffers g{};
        g.index = index.data();
        g.point = point.data();
        g.normal = normal.data();
        for (uint32_t ch : {1u, 3u}) {
            std::vector<double> in(n * ch), out(n * ch);
            for (double &v : in) v = rnd();
            for (uint32_t passes = 1; passes <= RTC_MAX_FILTER_PASSES; ++passes)
                for (uint32_t flags : {0u, (uint32_t)RTC_FILTER_SAME_OBJECT})
                    for (double sigma : {0.05, std::numeric_limits<double>::infinity()}) {
                        const rtc_filter f{sigma, passes, passes % 3u == 0u ? 8u : passes % 3u - 1u, flags, 0u};
                        REQUIRE(rtc_plane_filter(in.data(), ch, &g, w, h, &f, out.data()) == RTC_OK);
                        for (size_t i = 0; i < n; ++i)
                            if (index[i] < 0)
                                for (uint32_t c = 0; c < ch; ++c) REQUIRE(out[ch * i + c] == in[ch * i + c]); // a miss is copied
                        ++runs;
                    }
            const rtc_filter f{0.05, 1u, 1u, 0u, 0u};
            REQUIRE(rtc_plane_filter(in.data(), ch, &g, w, h, &f, in.data()) == RTC_ERR_ARG);
            REQUIRE(rtc_plane_filter(in.data(), 2u, &g, w, h, &f, out.data()) == RTC_ERR_ARG);
        }
        std::vector<uint16_t> counts(n);
        std::vector<double> occ(n), rgb(3 * n, 0.5);
        for (uint16_t &c : counts) c = (uint16_t)(rnd() * 17.0);
        REQUIRE(rtc_counts_to_fraction(counts.data(), 16u, w, h, occ.data()) == RTC_OK);
        REQUIRE(rtc_canvas_apply_occlusion(rgb.data(), occ.data(), 0.75, w, h) == RTC_OK);
        REQUIRE(rgb[0] == 0.5 * (1.0 - 0.75 * ((double)counts[0] / 16.0)));
        ++runs;
    }
    std::printf("no crash: %d runs\n", runs);
    return 0;
}
