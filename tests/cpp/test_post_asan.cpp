// The host statements of the post-processing passes (csrc/host_post.cpp) under AddressSanitizer and UBSan: every canvas in a
// heap buffer of exactly its size, over the sizes at which an index can go wrong — one pixel, an image narrower and lower than
// the widest halo (5 x 3 at radius 32), a row of one 256-value block and one pixel more (257 x 3) — with every curve and flag,
// radii 1, 2 and 32, in place and out of place, and a NaN, a +inf and a negative component planted. Compiled and run by
// tests/test_host_post.py; links nothing but host_post.cpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
    const uint32_t sizes[][2] = {{1, 1}, {5, 3}, {257, 3}};
    int runs = 0;
    for (const auto &sz : sizes) {
        const uint32_t w = sz[0], h = sz[1];
        const size_t n = (size_t)w * h;
        std::vector<double> in(3 * n), out(3 * n), again(3 * n);
        for (double &v : in) v = rnd() * 8.0;
        if (n > 8) {
            in[4] = std::numeric_limits<double>::quiet_NaN();
            in[6] = std::numeric_limits<double>::infinity();
            in[9] = -0.5;
        }
        rtc_luminance st{};
        REQUIRE(rtc_canvas_luminance(in.data(), w, h, &st) == RTC_OK);
        REQUIRE(st.count <= n && st.max >= 0.0 && st.sum >= st.max);
        ++runs;
        for (uint32_t curve : {RTC_TONEMAP_LINEAR, RTC_TONEMAP_REINHARD, RTC_TONEMAP_ACES})
            for (uint32_t flags = 0; flags < 4u; ++flags) {
                const rtc_tonemap t{0.18, 4.0, curve, flags};
                REQUIRE(rtc_canvas_tonemap(in.data(), w, h, &t, &st, out.data()) == RTC_OK);
                again = in;
                REQUIRE(rtc_canvas_tonemap(again.data(), w, h, &t, &st, again.data()) == RTC_OK);
                REQUIRE(std::memcmp(again.data(), out.data(), sizeof(double) * 3 * n) == 0);
                REQUIRE(rtc_canvas_tonemap(in.data(), w, h, &t, nullptr, out.data()) == (flags ? RTC_ERR_ARG : RTC_OK));
                ++runs;
            }
        for (uint32_t radius : {1u, 2u, 32u}) {
            const rtc_bloom b{1.0, 0.7, radius == 32u ? 9.0 : 0.8, radius, 0u};
            std::vector<double> wts(2 * radius + 1);
            REQUIRE(rtc_bloom_weights(&b, wts.data()) == RTC_OK);
            REQUIRE(wts[0] == wts[2 * radius] && wts[radius] >= wts[0]);
            REQUIRE(rtc_canvas_bloom(in.data(), w, h, &b, out.data()) == RTC_OK);
            again = in;
            REQUIRE(rtc_canvas_bloom(again.data(), w, h, &b, again.data()) == RTC_OK);
            REQUIRE(std::memcmp(again.data(), out.data(), sizeof(double) * 3 * n) == 0);
            const rtc_bloom bad{1.0, 0.7, 2.0, radius + 32u, 0u};
            REQUIRE(rtc_canvas_bloom(in.data(), w, h, &bad, out.data()) == RTC_ERR_ARG);
            ++runs;
        }
    }
    std::printf("no crash: %d runs\n", runs);
    return 0;
}
