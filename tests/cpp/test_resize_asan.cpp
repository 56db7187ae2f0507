// The host statement of the resize (csrc/host_resize.cpp) under AddressSanitizer and UBSan: every canvas and every table in a
// heap buffer of exactly its size, over the shapes at which an index can go wrong — one pixel to one pixel (a copy), one
// pixel enlarged (every tap window clipped on both sides), a frame reduced to one pixel (one output covers the whole axis), an
// axis alone, 1000 x 1 -> 1 x 1 (LANCZOS3's 1000 taps) — with every filter, a NaN and an infinity planted, the launch plan of
// each shape, and the refused calls. Compiled and run by tests/test_host_resize.py; links nothing but host_resize.cpp.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "rtc.h"
#include "rtc_resize.h"

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
    const uint32_t shapes[][4] = {{1, 1, 1, 1}, {1, 1, 3, 2}, {7, 5, 1, 1}, {17, 13, 7, 5}, {7, 5, 17, 13}, {31, 9, 8, 9}, {9, 31, 9, 8}, {1000, 1, 1, 1}};
    int runs = 0;
    for (const auto &s : shapes) {
        const uint32_t w_in = s[0], h_in = s[1], w_out = s[2], h_out = s[3];
        std::vector<double> in(3 * (size_t)w_in * h_in), out(3 * (size_t)w_out * h_out);
        for (double &v : in) v = rnd() * 4.0 - 1.0;
        if (in.size() > 12) {
            in[4] = std::numeric_limits<double>::quiet_NaN();
            in[11] = std::numeric_limits<double>::infinity();
        }
        for (uint32_t f = RTC_RESIZE_BOX; f <= RTC_RESIZE_LANCZOS3; ++f) {
            const rtc_resize spec{f, 0u};
            REQUIRE(rtc_resize_validate(&spec) == RTC_OK);
            const uint32_t axes[2][2] = {{w_in, w_out}, {h_in, h_out}};
            for (const auto &ax : axes) {
                const uint32_t taps = rtc_resize_taps(ax[0], ax[1], f);
                REQUIRE(taps >= 1u && taps <= RTC_MAX_RESIZE_TAPS);
                std::vector<uint32_t> first(ax[1]), count(ax[1]);
                std::vector<double> w((size_t)ax[1] * taps);
                REQUIRE(rtc_resize_weights(ax[0], ax[1], &spec, first.data(), count.data(), w.data()) == RTC_OK);
                for (uint32_t o = 0; o < ax[1]; ++o) REQUIRE(count[o] >= 1u && count[o] <= taps && first[o] + count[o] <= ax[0]);
            }
            REQUIRE(rtc_canvas_resize(in.data(), w_in, h_in, &spec, out.data(), w_out, h_out) == RTC_OK);
            if (w_in == w_out && h_in == h_out) REQUIRE(std::memcmp(in.data(), out.data(), sizeof(double) * in.size()) == 0);
            if (w_in == 1 && h_in == 1)
                for (size_t p = 0; p < out.size(); ++p) REQUIRE(std::memcmp(&out[p], &in[p % 3], sizeof(double)) == 0);
            const ResizePlanInputs pin{w_in, h_in, w_out, h_out, f};
            ResizePlan plan;
            REQUIRE(rtc_debug_plan_resize(&pin, &plan) == RTC_OK && plan.status == RTC_OK);
            REQUIRE(plan.h.lds_bytes <= RTC_RESIZE_LDS_BUDGET && (!plan.h.run || plan.h.seg >= 1u));
            ++runs;
        }
    }
    // what is refused, with `out` untouched
    {
        std::vector<double> in(3 * 3100), out(3 * 6, 123.25);
        for (double &v : in) v = rnd();
        const rtc_resize good{RTC_RESIZE_LANCZOS3, 0u}, bad_filter{5u, 0u}, bad_pad{RTC_RESIZE_BOX, 1u};
        REQUIRE(rtc_canvas_resize(nullptr, 7, 5, &good, out.data(), 3, 2) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 7, 5, &good, nullptr, 3, 2) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 7, 5, nullptr, out.data(), 3, 2) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 7, 5, &bad_filter, out.data(), 3, 2) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 7, 5, &bad_pad, out.data(), 3, 2) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 0, 5, &good, out.data(), 3, 2) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 7, 0, &good, out.data(), 3, 2) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 7, 5, &good, out.data(), 0, 2) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 7, 5, &good, out.data(), 3, 0) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 3100, 1, &good, out.data(), 1, 1) == RTC_ERR_ARG); // more than 1024 taps
        REQUIRE(rtc_canvas_resize(in.data(), 1, 3100, &good, out.data(), 1, 1) == RTC_ERR_ARG);
        REQUIRE(rtc_canvas_resize(in.data(), 7, 5, &good, in.data() + 3, 3, 2) == RTC_ERR_ARG);  // overlapping
        REQUIRE(rtc_resize_taps(0, 3, 0) == 0u && rtc_resize_taps(3, 0, 0) == 0u && rtc_resize_taps(3, 5, 9) == 0u);
        REQUIRE(rtc_resize_taps(3100, 1, RTC_RESIZE_LANCZOS3) > RTC_MAX_RESIZE_TAPS);
        uint32_t first[1], count[1];
        double w[1];
        REQUIRE(rtc_resize_weights(3100, 1, &good, first, count, w) == RTC_ERR_ARG);
        for (double v : out) REQUIRE(v == 123.25);
        const ResizePlanInputs pin{3100, 1, 1, 1, RTC_RESIZE_LANCZOS3};
        ResizePlan plan;
        REQUIRE(rtc_debug_plan_resize(&pin, &plan) == RTC_OK && plan.status == RTC_ERR_ARG);
        ++runs;
    }
    std::printf("no crash: %d runs\n", runs);
    return 0;
}
