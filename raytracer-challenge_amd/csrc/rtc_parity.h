// rtc_parity.h — the ONE definition of the patterns' even test: `x % 2.0 == 0.0` of the stripe, ring and checker
// pattern_at bodies (material.rs), i.e. fmod(x, 2.0) == 0.0, without fmod. Device fmod is a remainder loop (v_rndne_f64,
// v_ldexp_f64 and v_cndmask around three branches, 71 instructions for the checker's test); the form below is 24 straight
// instructions and decides the same thing for EVERY double. Used by
//   * rtc_kernels.hip — pattern_color (stripe, ring, checker) and k_arith op 7 (rtc_device_arith),
//   * rtc_api.cpp     — rtc_debug_even_f64, through which the CPU tests pin it against fmod.
#ifndef RTC_PARITY_H
#define RTC_PARITY_H

#if defined(__HIPCC__)
#define RTC_PHD __host__ __device__ inline
#else
#define RTC_PHD inline
#endif

// fmod(x, 2.0) == 0.0, exactly. fmod is exact in IEEE arithmetic: it is 0 precisely when x is a finite even integer (+-0
// included), and NaN for x = +-inf or NaN. With h = x * 0.5 and t = trunc(h):
//   * x * 0.5 only lowers the exponent, so h is exact unless x is below 2^-1021 in magnitude; then |h| < 1, t = +-0 and
//     the result is x == 0 — right, because the only even integer down there is 0.
//   * t is an integer of magnitude <= |h| <= 2^1023, so 2.0 * t is exact and finite, and it is an even integer.
//   * x - 2t is exact: 2t lies between 0 and x (t between 0 and h), and x and 2t are both multiples of ulp(x) (2t is an
//     integer; ulp(x) <= 1 below 2^53, and from 2^53 on h is itself an integer, t = h and 2t = x). So the difference is a
//     multiple of ulp(x) of magnitude <= |x|, which a double holds. (A fused x - 2t, should a compiler contract it, rounds
//     the same exact value.)
//   So the difference is 0 exactly when x = 2t, i.e. when x is an even integer.
//   * x = +-inf: h = t = 2t = +-inf, inf - inf = NaN, and NaN == 0.0 is false; x = NaN: NaN throughout, false. As fmod.
RTC_PHD bool rtc_even_f64(double x) { return (x - 2.0 * __builtin_trunc(x * 0.5)) == 0.0; }

#endif
