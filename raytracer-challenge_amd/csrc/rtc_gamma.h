// rtc_gamma.h — the ONE definition of how a gamma-corrected channel is quantised without `pow`: Canvas::to_imgbuf
// (canvas.rs:61-79) stores Color::scale(c.powf(1/gamma), 255) per channel (color.rs:55-65, the reciprocal taken in f32).
// Device `pow` is a few ulp off glibc's, so bytes computed with it would differ wherever a value lands on a quantisation
// step. Instead the host builds, per gamma, the table of thresholds
//     T[k] = the smallest double c >= +0 with scale255(pow(c, e)) >= k,  k = 1..255,  e = (double)(1.0f / gamma)
// (bisection on the bit patterns of doubles, calling the host's own pow: host_ppm.cpp rtc_gamma_thresholds), and
//     byte(c) = #{k : T[k] <= c}            for c >= +0 (the byte is monotone in c),
// with the rest of pow's C99 Annex F cases restated below for inputs whose sign bit is set (and NaN). Used by
//   * host_ppm.cpp     — builds the table, and pins this lookup against rtc_canvas_to_rgba8 in the CPU tests,
//   * rtc_kernels.hip  — k_trace's RGBA epilogue and k_canvas_to_rgba8 (the f32 estimate below is a guess only: every
//                        byte is decided by comparisons with the table),
//   * rtc_shutter.hip  — k_average_over's RGBA output (the mean of a motion-blurred frame),
//   * rtc_api.cpp      — the context's per-gamma cache of tables in device memory.
#ifndef RTC_GAMMA_H
#define RTC_GAMMA_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RTC_GHD __host__ __device__ inline
#else
#define RTC_GHD inline
#endif

// What pow(c, e) does for c with the sign bit set (e > 0 always: gamma is positive and finite)
enum {
    RTC_GAMMA_NEG_ABS = 0,  // e an even integer, or +inf (1/gamma overflowed f32): pow(c, e) = pow(|c|, e)
    RTC_GAMMA_NEG_ZERO = 1, // e an odd integer: pow(c, e) = -pow(|c|, e) <= -0 -> byte 0
    RTC_GAMMA_NEG_NAN = 2   // e not an integer: NaN for finite c < 0 -> byte 0; pow(-0, e) = +0; pow(-inf, e) = +inf -> 255
};

struct DevGamma {
    double t[256];  // t[0] = 0 (never compared against), t[k] = T[k]; non-decreasing, +inf where no double reaches k
    float e;        // 1.0f / gamma: the f32 estimate's exponent
    uint32_t neg;   // RTC_GAMMA_NEG_*
    uint32_t _pad[2];
};

// #{k in 1..255 : t[k] <= c} for c >= +0, given a guess: exact whenever t[guess] <= c < t[guess + 1] holds, an 8-step
// binary search otherwise. The guess only decides how fast the answer is found, never what it is.
RTC_GHD uint32_t rtc_gamma_count(const double *t, double c, uint32_t guess) {
    if (guess <= 255u && (guess == 0u || t[guess] <= c) && (guess == 255u || c < t[guess + 1u])) return guess;
    uint32_t k = 0;
    for (uint32_t step = 128u; step; step >>= 1) // k + step <= 255 throughout: the steps sum to 255
        if (t[k + step] <= c) k += step;
    return k;
}

// scale255(pow(c, e)) exactly as the host computes it, from the table. `guess` as for rtc_gamma_count (any value).
RTC_GHD uint32_t rtc_gamma_byte_with(const DevGamma *g, double c, uint32_t guess) {
    if (c != c) return 0u; // pow(NaN, e > 0) = NaN; Color::scale: NaN -> 0
    if (__builtin_signbit(c)) {
        if (g->neg == RTC_GAMMA_NEG_ZERO) return 0u;
        if (g->neg == RTC_GAMMA_NEG_NAN) return c == -__builtin_inf() ? 255u : 0u;
        c = -c;
    }
    return rtc_gamma_count(g->t, c, guess);
}

#if defined(__HIPCC__)
// The two 8-bit channels of the device: k_trace's epilogues, k_canvas_to_rgba8 (rtc_kernels.hip), k_average_over (rtc_shutter.hip).

// Color::scale(component, 255) color.rs:100-114: `(c * 255.0) as i32` (truncating, saturating,
// NaN -> 0) then clamp to [0, 255].
__device__ inline __attribute__((always_inline)) unsigned char scale255(double c) {
    const double v = c * 255.0;
    if (!(v >= 0.0)) return 0;   // negative (truncates to <= 0, clamps to 0) or NaN
    if (v >= 255.0) return 255;  // saturates / clamps
    return (unsigned char)(int)v; // v_cvt_i32_f64 truncates toward zero
}

// Canvas::to_imgbuf's channel, scale255(c.powf(1/gamma)) (canvas.rs:61-79, color.rs:55-65), from the launch's threshold
// table. The f32 estimate only picks which table entries to compare first; the byte is decided by the
// comparisons (an 8-step binary search when the estimate missed), so it equals the host's bit for bit.
__device__ inline __attribute__((always_inline)) unsigned char gamma_byte(const DevGamma *g, double c) {
    const float cf = (float)__builtin_fabs(c);
    const float v = __builtin_amdgcn_exp2f(g->e * __builtin_amdgcn_logf(cf)) * 255.0f; // v_log_f32 / v_exp_f32
    const uint32_t guess = v >= 1.0f ? (v < 255.0f ? (uint32_t)v : 255u) : 0u;          // NaN -> 0
    return (unsigned char)rtc_gamma_byte_with(g, c, guess);
}
#endif

#endif
