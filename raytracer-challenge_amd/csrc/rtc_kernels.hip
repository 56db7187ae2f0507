// rtc_kernels.hip — hand-written CDNA4 (gfx950, wave64) kernels for the hot path
//   Camera::render -> World::color_at -> World::intersect -> shade_hit
// of joedane/raytracer-challenge (ch1/src/camera.rs:94-160, shape.rs:677-781,
// material.rs:319-361).
//
// Design:
//  * one thread per pixel; a wave owns an 8x8 pixel tile (coherent hit / miss / shadow
//    decisions), a workgroup 2 such tiles side by side (1 for the frame-stack kernels, rtc_device.h);
//    tile = workgroup id, which the hardware
//    deals round-robin over the 8 XCDs (an even share of the image for each; see k_trace's tile loop).
//  * every value is IEEE f64 evaluated in the reference's operation order; the file is
//    compiled with -ffp-contract=off, so results are bit-identical to the CPU path apart
//    from pow() (material.rs:355).
//  * the object loop is wave-uniform. Default (SRC_CULL, SRC_CULL2 above 256 objects): a
//    conservative per-wave cull — 64 objects (or groups of 64) at a time, one bounding sphere per
//    lane against the wave's ray bundle, __ballot, exact tests only for the survivors, their
//    records fetched by uniform index through the scalar cache into SGPRs. Brute-force variants
//    kept for A/B (RTC_FLAG_NO_CULL): records through the scalar cache (SRC_SMEM) or from LDS
//    tiles shared by the workgroup (SRC_LDS1 one tile, SRC_LDSN many tiles with a barrier each).
//  * the sorted Intersections list of the reference (shape.rs:167-237) is replaced by its
//    streaming equivalent: running minimum over t >= 0 with first-inserted-wins ties
//    (closest hit), any-hit with early exit (shadow), and an "open set" pass for n1/n2
//    (compute_refractive, shape.rs:115-141) taken only when the hit material is transparent.
//  * recursion (reflected_color / refracted_color, depth <= 5) is an explicit per-thread
//    frame stack; colours are folded back in the reference's nesting order.
//  * no MFMA anywhere: there is no dense contraction on this path.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "rtc.h"
#include "rtc_ao.h"
#include "rtc_aov.h"
#include "rtc_bands.h"
#include "rtc_device.h"
#include "rtc_gather.h"
#include "rtc_gamma.h"
#include "rtc_parity.h"
#include "rtc_world_build.h"

// Depth of the reflection / refraction frame stack. A frame is pushed only by a color_at call whose
// `remaining` is not 0, and each level passes remaining - 1 on (shape.rs:730,735,752,765): a chain started with
// remaining = 5 (Camera::MAX_REFLECTIONS, camera.rs:31) suspends at most 5 shade_hit calls.
#define RTC_MAX_STACK 5
// 2nd argument of __launch_bounds__ = minimum waves per SIMD (caps VGPRs: 5 -> 96, 4 -> 128,
// 3 -> 168, 2 -> 256, 6 -> 80). Measured on the north-star scene (culled flat kernel, 90 VGPRs):
// 4 -> 0.0784 ms, 5 -> 0.0736 ms, 6 -> 0.0882 ms with 256-thread workgroups and one frame per launch; with
// 128-thread workgroups and 8 frames per launch 4, 5 and 6 measure the same (0.5365 ms per launch). Every one of these
// six-wave figures was taken on a kernel that SPILLED at 80 VGPRs (56 - 84 B of scratch per lane): they
// say what the spills cost, not what a sixth wave is worth.
// Kernels that carry the reflection/refraction frame stack: see RTC_WAVES_PER_SIMD_STACK.
// The bound is a constant of the instantiation (trace_waves_per_simd): the flat one-level one-sample whole-tile kernel
// takes RTC_WAVES_PER_SIMD_WHOLE, every other k_trace RTC_WAVES_PER_SIMD or RTC_WAVES_PER_SIMD_STACK.
#ifdef RTC_WAVES_PER_SIMD
#ifndef RTC_WAVES_PER_SIMD_WHOLE
#define RTC_WAVES_PER_SIMD_WHOLE RTC_WAVES_PER_SIMD // a sweep of RTC_WAVES_PER_SIMD moves the flagship kernel too
#endif
#else
#define RTC_WAVES_PER_SIMD 5
#endif
// k_trace<SRC_CULL, flat, ONE, WHOLE>, the north star's kernel: the only one that fits six waves (80 VGPRs) without a
// private segment (78 VGPRs, 0 B; tools/kernel_resources.py -DRTC_WAVES_PER_SIMD_WHOLE=6; its one-sample twin gets 12 B of
// scratch at 6). Measured that way, without spills, for the first time (profiles/sorted_lists_ab.log): the
// kernel alone is 5.5 % faster at 6, the pipelined frame — three launches and their binning kernels sharing the chip — is
// not (-0.05 % +- 0.8 %), and on top of the scalar tile-list walk 6 is slower than 5. So it stays 5.
#ifndef RTC_WAVES_PER_SIMD_WHOLE
#define RTC_WAVES_PER_SIMD_WHOLE 5
#endif
// Frame-stack kernels (124 VGPRs) on a reflective 2048x2048 / 100-sphere scene: 4 -> 0.871 ms,
// 5 -> 0.870, 6 -> 0.862 (forcing more waves trades spills for occupancy: a wash).
#ifndef RTC_WAVES_PER_SIMD_STACK
#define RTC_WAVES_PER_SIMD_STACK 4
#endif

#define IS_CULL(S) ((S) == SRC_CULL || (S) == SRC_CULL2) // (SRC_* and CULL_LEVEL: rtc_device.h)

struct V3 {
    double x, y, z;
};

#define DEVI __device__ __forceinline__

DEVI V3 mk(double x, double y, double z) { V3 v; v.x = x; v.y = y; v.z = z; return v; }
DEVI V3 vadd(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
DEVI V3 vsub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
DEVI V3 vmul(V3 a, double m) { return mk(a.x * m, a.y * m, a.z * m); }
DEVI V3 vmulv(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
DEVI V3 vneg(V3 a) { return mk(-a.x, -a.y, -a.z); }
// Vector::dot vec.rs:78-82: (x*x' + y*y') + z*z'
DEVI double vdot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// Vector::normalize vec.rs:65-76: magnitude, then three divisions
DEVI V3 vnormalize_plain(V3 a) {
    const double mag = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    return mk(a.x / mag, a.y / mag, a.z / mag);
}
// sqrt(x) (f64) without the part of hipcc's expansion that an ordinary operand does not need. The expansion is 21 VALU
// instructions: a compare of x against 2^-767 and v_ldexp_f64 of x by 256 where it is below (so that v_rsq_f64 never sees a
// denormal); the root itself — v_rsq_f64, two multiplies, seven fmas, the sequence of sqrt_bare below —; v_ldexp_f64 of the
// root by -128 where x was scaled; and a v_cmp_class_f64 select that hands x itself back where it is +-0 or +inf. With the
// selects and the constants' moves that is eleven instructions around a ten-instruction core.
// The guard, on x's upper word: sign clear and biased exponent in [256, 2047), one subtraction and one unsigned compare. x is
// then finite, positive, normal and at least 2^-767 (field 256 = 1023 - 767); +-0 and denormals (field 0), negative numbers
// and -0 (sign bit: the difference wraps far above the bound), +inf and NaN (field 2047) fail. For such an x
//   * the compare against 2^-767 is false, so both v_ldexp_f64 shift by 0: the identity on any finite number;
//   * x is neither +-0 nor +inf, so the class select keeps the root;
// and the core alone gives the expansion's bits. sqrt_wave chooses per WAVE, as vnormalize_wave below does: the guard is
// evaluated per lane and balloted over the active lanes; the wave runs the bare core when no active lane fails it and plain
// sqrt(x), in one cold block, otherwise. Both give the same bits in every lane that passes, so which one a wave takes cannot
// change a result and nothing is blended (tests/test_gpu_bare_sqrt.py: rtc_device_arith op 9 vs op 0 vs the host).
constexpr bool sqrt_bare_ok(uint32_t hi) { return hi - (256u << 20) < ((2047u - 256u) << 20); }
constexpr uint32_t f64_hi(double x) { return (uint32_t)(__builtin_bit_cast(unsigned long long, x) >> 32); }
static_assert(sqrt_bare_ok(f64_hi(0x1p-767)), "2^-767 passes");
static_assert(!sqrt_bare_ok(f64_hi(0x1.fffffffffffffp-768)), "the double below 2^-767 fails");
static_assert(sqrt_bare_ok(f64_hi(0x1.fffffffffffffp1023)), "DBL_MAX passes");
static_assert(!sqrt_bare_ok(f64_hi(__builtin_inf())) && !sqrt_bare_ok(f64_hi(__builtin_nan(""))), "+inf and NaN fail");
static_assert(!sqrt_bare_ok(f64_hi(0.0)) && !sqrt_bare_ok(f64_hi(-0.0)) && !sqrt_bare_ok(f64_hi(-1.0)), "+0, -0 and -1.0 fail");
static_assert(!sqrt_bare_ok(f64_hi(0x1p-1022 / 2)), "DBL_MIN / 2 (a denormal) fails");
DEVI double sqrt_bare(double x) { // the expansion's core, for an x that passes sqrt_bare_ok
    const double y = __builtin_amdgcn_rsq(x);
    const double g0 = x * y;
    const double h0 = 0.5 * y;
    const double r0 = __builtin_fma(-h0, g0, 0.5);
    const double g1 = __builtin_fma(g0, r0, g0);
    const double h1 = __builtin_fma(h0, r0, h0);
    const double d0 = __builtin_fma(-g1, g1, x);
    const double g2 = __builtin_fma(d0, h1, g1);
    const double d1 = __builtin_fma(-g2, g2, x);
    return __builtin_fma(d1, h1, g2);
}
DEVI double sqrt_wave(double x) {
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!sqrt_bare_ok(f64_hi(x))) == 0ull, 1)) return sqrt_bare(x); // (wave-uniform)
    return sqrt(x);
}
// Where the flat k_trace kernels and the binning kernel take it: a mask of sites, 0 = plain sqrt everywhere, the code as it
// was (kept for the A/B).
//   1  the square root inside vnormalize_wave (ray generation, shadow_ray, shape_normal[_of]): one guard for the function
//   2  the sphere's discriminant root of the primary pass (closest_update)
//   4  the sphere's discriminant root of the shadow pass (occludes)
//   8  the ring pattern's root (pattern_color)
//  16  vnormalize_shared as the binning kernel calls it (primary_dir): per lane, joined to that function's own condition;
//      not in the default: alone it measured no gain on the north star (profiles/bare_sqrt_ab.log)
// trace_bare_sqrt: the instantiations that take sites 1 to 8 — trace_wave_normalize's family, the render flavour of SRC_CULL
// and SRC_CULL2 without a frame stack, one light, pinhole camera (with ONE and WHOLE and without). Every other kernel is the
// parent's code (tools/isa_compare.py; profiles/bare_sqrt_*).
#ifndef RTC_BARE_SQRT
#define RTC_BARE_SQRT 15
#endif
enum { BS_NORMALIZE = 1, BS_PRIMARY = 2, BS_SHADOW = 4, BS_RING = 8, BS_BIN = 16 };
constexpr bool trace_bare_sqrt(int site, int src, bool refl, bool probe, bool alt, bool multi) {
    return (RTC_BARE_SQRT & site) != 0 && IS_CULL(src) && !refl && !probe && !alt && !multi;
}
// The shared-divisor form of a / mag (vnormalize_shared's and vnormalize_wave's, see there) for a caller that has checked
// their guard: the callers that take the magnitude's root through sqrt_bare.
DEVI V3 vdivide_shared(V3 a, double mag) {
    const double r0 = __builtin_amdgcn_rcp(mag);
    const double e0 = __builtin_fma(-mag, r0, 1.0);
    const double r1 = __builtin_fma(r0, e0, r0);
    const double e1 = __builtin_fma(-mag, r1, 1.0);
    const double r = __builtin_fma(r1, e1, r1);
    auto quot = [&](double x) {
        const double q = x * r;
        const double rem = __builtin_fma(-mag, q, x);
        return __builtin_amdgcn_div_fixup(__builtin_fma(rem, r, q), mag, x);
    };
    return mk(quot(a.x), quot(a.y), quot(a.z));
}
// The three IEEE divisions share their divisor. hipcc expands x / y (f64) into v_div_scale x2, v_rcp, four v_fma refining
// 1/y, v_mul, v_fma, v_div_fmas, v_div_fixup (11 instructions); everything up to the refined reciprocal depends on y alone
// as long as v_div_scale leaves y unscaled, which it does unless y, 1/y or x/y leave the normal range or x is tiny
// (ISA: V_DIV_SCALE_F64). vnormalize_shared evaluates that part once when |mag| is in [2^-400, 2^400] and every
// component is +-0 or at least 2^-500 in magnitude (then no scaling happens, VCC is clear and v_div_fmas is a plain fma):
// 5 + 3 x 4 instructions + the guards instead of 33, bit-identical (tests/test_gpu_round3.py: rtc_device_arith op 5 vs op 6
// vs the host, 2 M triples). The binning kernel uses it (primary_dir). In k_trace this per-lane form measured no gain (north
// star equal, C4 +1 %, profiles/r03_exp_shared_normalize.log: both paths compiled in line and blended per lane); the flat
// k_trace kernels take vnormalize_wave below, every other kernel keeps vnormalize_plain.
// BARE (RTC_BARE_SQRT's site 16): the magnitude's root through sqrt_bare under the same per-lane condition, whose term on
// `mag` becomes vnormalize_wave's term on the sum of squares — in [2^-767, 2^799), which implies it (see there).
template <bool BARE = false> DEVI V3 vnormalize_shared(V3 a) {
    if constexpr (BARE) {
        const double s = a.x * a.x + a.y * a.y + a.z * a.z;
        auto in_range = [](double v) { return __builtin_amdgcn_class(v, 0x060 /* +-0 */) || fabs(v) >= 0x1p-500; };
        if (f64_hi(s) - (256u << 20) < ((1023u + 799u - 256u) << 20) && in_range(a.x) && in_range(a.y) && in_range(a.z)) {
            return vdivide_shared(a, sqrt_bare(s));
        }
        const double mag = sqrt(s);
        return mk(a.x / mag, a.y / mag, a.z / mag);
    }
    const double mag = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    auto in_range = [](double v) { return __builtin_amdgcn_class(v, 0x060 /* +-0 */) || fabs(v) >= 0x1p-500; };
    if (fabs(mag) >= 0x1p-400 && fabs(mag) <= 0x1p400 && in_range(a.x) && in_range(a.y) && in_range(a.z)) {
        const double r0 = __builtin_amdgcn_rcp(mag);
        const double e0 = __builtin_fma(-mag, r0, 1.0);
        const double r1 = __builtin_fma(r0, e0, r0);
        const double e1 = __builtin_fma(-mag, r1, 1.0);
        const double r = __builtin_fma(r1, e1, r1);
        auto quot = [&](double x) {
            const double q = x * r;
            const double rem = __builtin_fma(-mag, q, x);
            return __builtin_amdgcn_div_fixup(__builtin_fma(rem, r, q), mag, x);
        };
        return mk(quot(a.x), quot(a.y), quot(a.z));
    }
    return mk(a.x / mag, a.y / mag, a.z / mag);
}
// The same two forms, chosen per WAVE: the guard is evaluated per lane and balloted over the active lanes, and the wave takes
// the shared form when no active lane fails it, the three plain divisions (one cold block) otherwise. Both forms give the
// same bits in every lane that passes the guard, so which one a wave takes cannot change a result and nothing is blended.
// Also returns `mag`, the correctly rounded square root (the shadow ray's distance).
// The guard, exact and stricter than vnormalize_shared's condition:
//   * v_frexp_exp_i32_f64 of each component (0 for +-0; the true exponent of a denormal), an integer minimum and one
//     compare: every component is +-0 or at least 2^-500 in magnitude (2^-500 = 0.5 * 2^-499: exponent >= -499);
//   * mag's biased exponent field in [1023 - 400, 1023 + 399], read off its upper word with one subtraction and one unsigned
//     compare: mag in [2^-400, 2^400). mag is a square root: +0, positive, +inf or NaN, so zero, infinite and NaN magnitudes
//     (fields 0 and 2047, and a NaN's sign bit only makes the difference larger) all fail and take the plain divisions.
// Inf and NaN COMPONENTS need no term of their own (frexp_exp gives 0 for them, which passes): they make mag inf or NaN,
// which fails. And even without that, v_div_fixup — the last instruction of both forms, with the same numerator and
// denominator — decides every quotient with a NaN, an infinity or a zero among the two from those two operands alone,
// whatever the refined quotient it is handed. tests/test_gpu_shared_normalize_flat.py (rtc_device_arith op 8 vs op 6 vs
// the host) pins all of it, waves with lanes on both sides of the guard included.
// RTC_BARE_SQRT's site 1: the root through sqrt_bare in the same wave-level choice, under ONE guard. The term on mag is
// replaced by one on the sum of squares s, read off ITS upper word: biased exponent field in [256, 1023 + 799), that is s in
// [2^-767, 2^799), sign clear. It is sqrt_bare_ok with a lower upper bound, so the bare root is the root; and it implies the
// term on mag it replaces: sqrt is monotone and correctly rounded, so mag >= sqrt(2^-767) > 2^-400, and s < 2^799 gives
// sqrt(s) < 2^399.5, which rounds to at most the double nearest 2^399.5, below 2^400. (s < 2^800 would not do: the root of the
// double just below 2^800 rounds UP to 2^400.) Waves with a magnitude in [2^-400, 2^-383.5) or [2^399.5, 2^400) now take the
// plain form, where they took the shared one: the same bits. The term on the components' exponents stays as it is.
DEVI V3 vnormalize_wave(V3 a, double &mag_out) {
    if constexpr ((RTC_BARE_SQRT & BS_NORMALIZE) != 0) {
        const double s = a.x * a.x + a.y * a.y + a.z * a.z;
        const int emin = min(min(__builtin_amdgcn_frexp_exp(a.x), __builtin_amdgcn_frexp_exp(a.y)), __builtin_amdgcn_frexp_exp(a.z));
        const bool fits = emin >= -499 && f64_hi(s) - (256u << 20) < ((1023u + 799u - 256u) << 20);
        static_assert(1023u + 799u < 2047u, "the guard on s is sqrt_bare_ok's with a lower upper bound");
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(!fits) == 0ull, 1)) { // (wave-uniform)
            mag_out = sqrt_bare(s);
            return vdivide_shared(a, mag_out);
        }
        const double mag = sqrt(s);
        mag_out = mag;
        return mk(a.x / mag, a.y / mag, a.z / mag);
    }
    const double mag = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
    mag_out = mag;
    const int emin = min(min(__builtin_amdgcn_frexp_exp(a.x), __builtin_amdgcn_frexp_exp(a.y)), __builtin_amdgcn_frexp_exp(a.z));
    const uint32_t mag_hi = (uint32_t)(__builtin_bit_cast(unsigned long long, mag) >> 32);
    const bool fits = emin >= -499 && mag_hi - ((1023u - 400u) << 20) < (800u << 20);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!fits) == 0ull, 1)) { // (wave-uniform)
        const double r0 = __builtin_amdgcn_rcp(mag);
        const double e0 = __builtin_fma(-mag, r0, 1.0);
        const double r1 = __builtin_fma(r0, e0, r0);
        const double e1 = __builtin_fma(-mag, r1, 1.0);
        const double r = __builtin_fma(r1, e1, r1);
        auto quot = [&](double x) {
            const double q = x * r;
            const double rem = __builtin_fma(-mag, q, x);
            return __builtin_amdgcn_div_fixup(__builtin_fma(rem, r, q), mag, x);
        };
        return mk(quot(a.x), quot(a.y), quot(a.z));
    }
    return mk(a.x / mag, a.y / mag, a.z / mag);
}
// Vector::reflect vec.rs:106-108: self - n*(2*(self.n))
DEVI V3 vreflect(V3 v, V3 n) { return vsub(v, vmul(n, 2. * vdot(v, n))); }

// Matrix::transform_point transform.rs:122-128 (rows of 4, row 3 never read)
template <class P> DEVI V3 xpoint(P m, V3 p) {
    return mk(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
              m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}
// Matrix::transform_vector transform.rs:107-120
template <class P> DEVI V3 xvector(P m, V3 v) {
    return mk(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z,
              m[8] * v.x + m[9] * v.y + m[10] * v.z);
}
// transform_vector with a packed 3x3
template <class P> DEVI V3 xvector3(P m, V3 v) {
    return mk(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z,
              m[6] * v.x + m[7] * v.y + m[8] * v.z);
}

DEVI unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
DEVI uint32_t popc64(unsigned long long m) { return (uint32_t)__popcll(m); }

// Cube::check_axis shape.rs:540-564
DEVI void check_axis(double origin, double direction, double &tmin, double &tmax) {
    const double tmin_numerator = -1.0 - origin;
    const double tmax_numerator = 1. - origin;
    if (fabs(direction) >= RTC_EPSILON) {
        tmin = tmin_numerator / direction;
        tmax = tmax_numerator / direction;
    } else {
        tmin = (tmin_numerator >= 0.0) ? __builtin_inf() : -__builtin_inf();
        tmax = (tmax_numerator >= 0.0) ? __builtin_inf() : -__builtin_inf();
    }
    if (tmin > tmax) {
        const double s = tmin;
        tmin = tmax;
        tmax = s;
    }
}

// Entries of one shape for a ray already in object space, in the order the reference's
// per-shape list holds them (shape.rs:361-375, 462-471, 577-591). Returns their count.
// `c_pre`: the sphere's `c` when the caller already has it (primary rays).
template <bool HAVE_C> DEVI int shape_entries(uint32_t kind, V3 o, V3 d, double c_pre, double &t0, double &t1) {
    if (kind == RTC_SPHERE) {
        const double a = vdot(d, d);
        const double b = 2. * vdot(d, o);
        const double c = HAVE_C ? c_pre : (vdot(o, o) - 1.);
        const double disc = (b * b) - 4. * a * c;
        if (disc < 0.) return 0;
        const double sq = sqrt(disc);
        const double den = 2. * a;
        t0 = (-b - sq) / den;
        t1 = (-b + sq) / den;
        return 2;
    } else if (kind == RTC_PLANE) {
        if (fabs(d.y) < RTC_EPSILON) return 0;
        t0 = -o.y / d.y;
        return 1;
    } else {
        double xmin, xmax, ymin, ymax, zmin, zmax;
        check_axis(o.x, d.x, xmin, xmax);
        check_axis(o.y, d.y, ymin, ymax);
        check_axis(o.z, d.z, zmin, zmax);
        const double tmin = fmax(xmin, fmax(ymin, zmin));
        const double tmax = fmin(xmax, fmin(ymax, zmax));
        if (tmin < tmax) {
            t0 = tmin;
            t1 = tmax;
            return 2;
        }
        return 0;
    }
}

// Does entry (t, object j) come before the current best entry (best, hidx) in the reference's
// merged sorted list? Smaller t first; at equal t the shape inserted first (lower index); an
// object's own second root never precedes its first (t1 <= t2 and j == hidx fails the test).
// Visiting objects in insertion order makes the index comparison redundant but harmless; the
// culled path visits them in Morton order and needs it.
DEVI bool closer(double t, int j, double best, int hidx) { return t < best || (t == best && j < hidx); }

// Closest-hit update for one object: Intersections::get_hit (shape.rs:220-232) over the merged
// sorted list == smallest t >= 0.0, ties to the entry inserted first (lower object index, then
// first root). For a sphere t1 <= t2, so the second root is only needed when the first is not
// a candidate (t1 < 0 or NaN).
// Object-space y row only: all a plane needs (transform.rs:116,125 for the y component).
template <class P> DEVI double xpoint_y(P m, V3 p) { return m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7]; }
template <class P> DEVI double xvector_y(P m, V3 v) { return m[4] * v.x + m[5] * v.y + m[6] * v.z; }

// Plane::intersect_local computes t = -o.y / d.y (shape.rs:467) and every caller then asks whether
// t >= 0.0. When o.y and d.y are both positive or both negative the quotient is strictly negative —
// provided it cannot underflow to -0.0 (which WOULD satisfy t >= 0.0): with |o.y| >= 2^-500 and
// |d.y| <= 2^500 its magnitude is >= 2^-1000. In that case the division (~12 instructions, several
// of them quarter-rate) can be skipped without changing any result.
DEVI bool plane_t_certainly_negative(double oy, double dy) {
    const double lo = 0x1p-500, hi = 0x1p500;
    return ((oy >= lo && dy > 0. && dy <= hi) || (oy <= -lo && dy < 0. && dy >= -hi));
}

// World-space ray in, per-kind transform inside (a plane only needs the y row of the inverse).
template <bool BARE = false, class P> DEVI void closest_world(uint32_t kind, P m, V3 ro, V3 rd, int j, double &best, int &hidx, int &hroot);
template <bool BARE = false, class P> DEVI bool occludes_world(uint32_t kind, P m, V3 ro, V3 rd, double dist);

// BARE (here, in occludes and in pattern_color): the root through sqrt_wave — RTC_BARE_SQRT's sites 2, 4 and 8.
template <bool HAVE_C, bool BARE = false>
DEVI void closest_update(uint32_t kind, V3 o, V3 d, double c_pre, int j, double &best, int &hidx, int &hroot) {
    if (kind == RTC_SPHERE) {
        const double a = vdot(d, d);
        const double b = 2. * vdot(d, o);
        const double c = HAVE_C ? c_pre : (vdot(o, o) - 1.);
        const double disc = (b * b) - 4. * a * c;
        if (!(disc < 0.)) {
            const double sq = BARE ? sqrt_wave(disc) : sqrt(disc);
            const double den = 2. * a;
            const double t1 = (-b - sq) / den;
            if (t1 >= 0.0) {
                if (closer(t1, j, best, hidx)) { best = t1; hidx = j; hroot = 0; }
            } else {
                const double t2 = (-b + sq) / den;
                if (t2 >= 0.0 && closer(t2, j, best, hidx)) { best = t2; hidx = j; hroot = 1; }
            }
        }
    } else {
        double t0 = 0., t1 = 0.;
        const int cnt = shape_entries<false>(kind, o, d, 0., t0, t1);
        if (cnt >= 1 && t0 >= 0.0 && closer(t0, j, best, hidx)) { best = t0; hidx = j; hroot = 0; }
        if (cnt == 2 && t1 >= 0.0 && closer(t1, j, best, hidx)) { best = t1; hidx = j; hroot = 1; }
    }
}

// is_shadowed_by_light (shape.rs:716-727): hit.t < distance  <=>  some entry has 0 <= t < distance.
template <bool BARE = false> DEVI bool occludes(uint32_t kind, V3 o, V3 d, double dist) {
    if (kind == RTC_SPHERE) {
        const double a = vdot(d, d);
        const double b = 2. * vdot(d, o);
        const double c = vdot(o, o) - 1.;
        const double disc = (b * b) - 4. * a * c;
        if (disc < 0.) return false;
        const double sq = BARE ? sqrt_wave(disc) : sqrt(disc);
        const double den = 2. * a;
        const double t1 = (-b - sq) / den;
        if (t1 >= 0.0) return t1 < dist;
        const double t2 = (-b + sq) / den;
        return t2 >= 0.0 && t2 < dist;
    }
    double t0 = 0., t1 = 0.;
    const int cnt = shape_entries<false>(kind, o, d, 0., t0, t1);
    if (cnt >= 1 && t0 >= 0.0 && t0 < dist) return true;
    if (cnt == 2 && t1 >= 0.0 && t1 < dist) return true;
    return false;
}

template <bool BARE, class P> DEVI void closest_world(uint32_t kind, P m, V3 ro, V3 rd, int j, double &best, int &hidx, int &hroot) {
    if (kind == RTC_PLANE) { // shape.rs:462-471
        const double oy = xpoint_y(m, ro), dy = xvector_y(m, rd);
        if (!(fabs(dy) < RTC_EPSILON) && !plane_t_certainly_negative(oy, dy)) {
            const double t = -oy / dy;
            if (t >= 0.0 && closer(t, j, best, hidx)) { best = t; hidx = j; hroot = 0; }
        }
    } else {
        closest_update<false, BARE>(kind, xpoint(m, ro), xvector(m, rd), 0., j, best, hidx, hroot);
    }
}
template <bool BARE, class P> DEVI bool occludes_world(uint32_t kind, P m, V3 ro, V3 rd, double dist) {
    if (kind == RTC_PLANE) {
        const double oy = xpoint_y(m, ro), dy = xvector_y(m, rd);
        if (fabs(dy) < RTC_EPSILON || plane_t_certainly_negative(oy, dy)) return false;
        const double t = -oy / dy;
        return t >= 0.0 && t < dist;
    }
    return occludes<BARE>(kind, xpoint(m, ro), xvector(m, rd), dist);
}

// Primary rays: the object-space origin `po` (= transform_point(inv, camera origin)) and the sphere's
// c = po.po - 1 are the same for every pixel; they come from the per-render table `prim`
// (k_prep_primary, same arithmetic), so only the direction is transformed here.
template <bool BARE = false, class P, class Q> DEVI void closest_prim(uint32_t kind, P m, Q pr, V3 rd, int j, double &best, int &hidx, int &hroot) {
    if (kind == RTC_PLANE) {
        const double oy = pr[1], dy = xvector_y(m, rd);
        if (!(fabs(dy) < RTC_EPSILON) && !plane_t_certainly_negative(oy, dy)) {
            const double t = -oy / dy;
            if (t >= 0.0 && closer(t, j, best, hidx)) { best = t; hidx = j; hroot = 0; }
        }
    } else {
        closest_update<true, BARE>(kind, mk(pr[0], pr[1], pr[2]), xvector(m, rd), pr[3], j, best, hidx, hroot);
    }
}

// ---- wave64 reduction (DPP): inclusive scan inside each row of 16 lanes, then two row
// broadcasts; the result lands in lane 63. All 64 lanes must execute it (converged code);
// lanes that do not take part pass the identity.
// Maximum of NON-NEGATIVE floats (NaN-free): their bit patterns order like unsigned integers, and
// v_max_u32 with identity 0 folds into the DPP instruction (one instruction per step).
template <int CTRL, int ROW_MASK> DEVI unsigned dpp_u32(unsigned src) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)src, CTRL, ROW_MASK, 0xf, false);
}
DEVI unsigned wave_max_u32(unsigned v) {
    v = max(v, dpp_u32<0x111, 0xf>(v));
    v = max(v, dpp_u32<0x112, 0xf>(v));
    v = max(v, dpp_u32<0x114, 0xf>(v));
    v = max(v, dpp_u32<0x118, 0xf>(v));
    v = max(v, dpp_u32<0x142, 0xa>(v));
    v = max(v, dpp_u32<0x143, 0xc>(v));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
DEVI float wave_max_nonneg(float f) { return __builtin_bit_cast(float, wave_max_u32(__builtin_bit_cast(unsigned, f))); }

// ---- conservative per-wave cull ------------------------------------------------------------
// The rays a wave is about to trace form a bundle: a cone (apex, unit axis, half-angle theta)
// that contains every active lane's ray, optionally fattened by the spread `rho` of the ray
// origins around the apex and cut at distance `tmax`. An object whose world-space bounding
// sphere (centre C, radius R, DevBound) cannot touch the bundle cannot produce an intersection
// with t >= 0 for any lane, so skipping it leaves the closest hit / shadow bit unchanged — the
// objects that survive are visited in insertion order and tested with the exact f64 arithmetic.
// The bundle is built in f32 (cheap DPP reductions) and widened by far more than the f32 error;
// the per-object test is f64 and square-root free.
struct Bundle {
    double px, py, pz;   // apex
    double ax, ay, az;   // axis (unit to ~1e-6)
    double cosT, sinT;   // half-angle, already widened
    double rho;          // origin spread around the apex
    double tmax;         // reach along the rays (inf: unbounded)
    double spread;       // upper bound of the distance apex -> the ORIGIN the exact test uses (0 for
                         // primary rays, rho for secondary rays, tmax for shadow segments, whose
                         // exact rays start at the far end)
    bool off;            // bundle could not be bounded: every object is a candidate
};

// A wave-uniform double that the compiler would otherwise keep in two VGPRs: move it to SGPRs.
DEVI double uniform_f64(double x) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

DEVI double lane_f64(double x, uint32_t l) { // lane l's value in every lane (l wave-uniform)
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, (int)l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), (int)l);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

DEVI bool finite3(V3 v) { return fabs(v.x) < __builtin_inf() && fabs(v.y) < __builtin_inf() && fabs(v.z) < __builtin_inf(); }

// SHARED: every active lane's ray starts at `apex` (the camera origin, or the light for shadow
// segments walked backwards); otherwise the apex is the origin of the axis lane and `rho` the
// spread of the lanes' origins around it. REACH: the rays end after `reach` (shadow segments). The axis is the direction of
// one active lane near the tile centre (no reduction needed); the half-angle is the largest
// deviation from it.
template <bool SHARED, bool REACH>
DEVI Bundle make_bundle(bool active, V3 apex, V3 o, V3 d, double reach) {
#pragma clang fp contract(fast) // cull arithmetic (see bundle_touches)
    Bundle B;
    float fx = 0.f, fy = 0.f, fz = 0.f;
    bool good = active && finite3(o) && finite3(d);
    if (good) {
        const float x = (float)d.x, y = (float)d.y, z = (float)d.z;
        const float l2 = x * x + y * y + z * z;
        good = l2 > 1e-30f && l2 < 1e30f;
        const float il = __builtin_amdgcn_rsqf(l2);
        fx = x * il; fy = y * il; fz = z * il;
    }
    const unsigned long long gmask = ballot(good);
    bool off = ballot(active && !good) != 0ull || gmask == 0ull;
    // axis = direction of a lane near the middle of the 8x8 tile (lane 27 = pixel (3,3)) when it is
    // active, else the nearest active lane: a centred axis halves the cone's half-angle compared
    // with a corner lane, i.e. ~4x fewer objects survive the cull
    const unsigned long long ghi = gmask & ~((1ull << 27) - 1ull);
    const int lane0 = ghi ? __builtin_ctzll(ghi) : (gmask ? 63 - __builtin_clzll(gmask) : 0);
    const float ax = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fx), lane0));
    const float ay = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fy), lane0));
    const float az = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, fz), lane0));
    float dotv = 1.f, q2 = 0.f; // cos and sin^2 of the angle to the axis
    if (good) {
        dotv = ax * fx + ay * fy + az * fz;
        const float cx = ay * fz - az * fy, cy = az * fx - ax * fz, cz = ax * fy - ay * fx;
        q2 = cx * cx + cy * cy + cz * cz;
    }
    const float q2max = wave_max_nonneg(q2);
    // narrow bundle (every lane within ~45 degrees of the axis): the common case needs only the
    // sin^2 reduction; the cosine minimum is reduced only for wide bundles
    const bool narrow = ballot(good && !(dotv > 0.7f)) == 0ull;
    float cmin = 1.f;
    if (!narrow) cmin = 1.f - wave_max_nonneg(good ? fmaxf(0.f, 1.f - dotv) : 0.f);
    float rho = 0.f;
    if constexpr (!SHARED) {
        // apex = the origin of the axis lane (three readlanes), not the centroid of the origins (four wave sums): C4 -1.4 %,
        // reflective 1080p -1 % (profiles/r03_exp_small_steps.log). Either is conservative: rho is measured from the apex.
        const float mx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, (float)o.x), lane0));
        const float my = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, (float)o.y), lane0));
        const float mz = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, (float)o.z), lane0));
        apex = mk((double)mx, (double)my, (double)mz);
        float e2 = 0.f;
        if (good) {
            const double ex = o.x - apex.x, ey = o.y - apex.y, ez = o.z - apex.z;
            e2 = (float)(ex * ex + ey * ey + ez * ez) * 1.0001f;
        }
        const float e2max = wave_max_nonneg(e2);
        rho = __builtin_sqrtf(e2max) * 1.0001f + 1e-30f;
        if (!(e2max < 1e30f) || !(fabsf(mx) < 1e30f && fabsf(my) < 1e30f && fabsf(mz) < 1e30f)) off = true;
    }
    float tmax = __builtin_inff();
    if constexpr (REACH) {
        float tm = 0.f;
        if (good) tm = (reach < 1e30) ? fmaxf(0.f, (float)reach) * 1.0001f + 1e-30f : __builtin_inff();
        tmax = wave_max_nonneg(tm);
    }
    if (!(cmin > 0.2f)) off = true;
    float sinT, cosT;
    if (narrow) { // the cross product resolves small angles, the dot does not
        sinT = __builtin_sqrtf(q2max) * 1.001f + 4e-6f;
        cosT = __builtin_sqrtf(fmaxf(0.f, 1.f - sinT * sinT));
    } else {
        // widen through the cosine only and derive the sine from it: (cosT, sinT) must stay a unit
        // pair. (Inflating the sine on its own SHRINKS the computed distance budget for centres
        // behind the apex plane, wa < 0 — found by the stress campaign, 1 world in ~25 000.)
        cosT = cmin - 1e-3f;
        sinT = __builtin_sqrtf(fmaxf(0.f, 1.f - cosT * cosT));
    }
    if (!(sinT < 0.98f)) off = true;
    B.off = off;
    B.px = uniform_f64(apex.x); B.py = uniform_f64(apex.y); B.pz = uniform_f64(apex.z);
    B.ax = uniform_f64((double)ax); B.ay = uniform_f64((double)ay); B.az = uniform_f64((double)az);
    B.cosT = uniform_f64((double)cosT); B.sinT = uniform_f64((double)sinT);
    B.rho = uniform_f64((double)rho);
    B.tmax = uniform_f64((double)tmax);
    B.spread = REACH ? B.tmax : B.rho;
    if (!(B.spread < 1e300)) off = true; // shadow segment of unbounded length: do not cull
    B.off = off;
    return B;
}

// Can the bounding sphere touch the bundle? (false => provably no intersection with t >= 0.)
// Let (wa, perp) be the centre's axial / radial coordinates about the axis. The distance from the
// centre to the cone's side is perp*cos(theta) - wa*sin(theta); the sphere (fattened by rho) can
// touch the solid cone only if that is <= Re, it is not wholly behind the apex plane, and it
// is within reach. Squares instead of square roots.
// `key` (KEYED only): a lower bound of the distance from the apex to any point of the (inflated)
// sphere, 0 when there is none to give. For rays that START at the apex with a unit direction
// (primary rays) every intersection of the object has t >= key, which is what lets the ordered walk
// of the two-level cull stop early (for_each_object, Skip).
template <bool KEYED = false> DEVI bool bundle_touches(const Bundle &B, const DevBound &b, float *key = nullptr) {
#pragma clang fp contract(fast) // cull arithmetic, not reference arithmetic: the file is compiled with
                                // -ffp-contract=off for the exact tests; here FMA halves the dot products and only
                                // tightens the rounding that the slacks below already cover
    if constexpr (KEYED) *key = 0.f;
    if (B.off) return true;
    if (!(b.r < __builtin_inf())) return true;
    const double wx = b.cx - B.px, wy = b.cy - B.py, wz = b.cz - B.pz;
    // rounding inflation of the radius (rtc_device.h, DevBound): D <= |C - apex|_1 + spread
    const double l1 = fabs(wx) + fabs(wy) + fabs(wz);
    const double Dub = l1 + B.spread;
    const double r_eff = b.r + b.r * (b.k * Dub * (b.cn + Dub));
    // slack: 1e-5 relative on the radius, plus 1e-6 of the centre's L1 distance (>= its Euclidean
    // distance) for the f32 origin of (axis, cosT, sinT): axis length and cos^2+sin^2 are 1 to ~2e-6
    const double Re = (r_eff + B.rho) * 1.00001 + 1e-6 * l1 + 1e-12;
    const double d2 = wx * wx + wy * wy + wz * wz;
    if (d2 <= Re * Re) return true;
    if constexpr (KEYED) { // |C - apex| - Re, rounded down with 1e-6 margins (f32 conversions and sqrt err ~1e-7)
        const float dist = __builtin_sqrtf((float)d2) * 0.999999f, rad = (float)Re * 1.000001f;
        *key = fmaxf(0.f, (dist - rad) * 0.999999f); // NaN / inf - inf -> 0: no bound
    }
    const double wa = wx * B.ax + wy * B.ay + wz * B.az;
    if (wa < -Re) return false;                       // wholly behind the apex plane (theta < 90 deg)
    const double far = B.tmax + Re;
    if (d2 > far * far) return false;                  // beyond the reach of every ray (inf*inf = inf: never)
    // the axis is unit only to ~2e-6: take an upper bound of the axial coordinate on the right-hand
    // side and a lower bound of perp^2 on the left, so the inequality can only err towards "keep"
    const double rhs = Re + (wa + fabs(wa) * 1e-5) * B.sinT;
    if (rhs < 0.) return false;
    const double perp2 = d2 - wa * wa * 1.00001;
    return !(perp2 * (B.cosT * B.cosT) > rhs * rhs);   // NaN-safe: keep the object unless provably far
}

// The KEY of bundle_touches<true> on its own: a lower bound of the distance from `apex` to the bound's inflated sphere
// (0 when the apex may be inside or nothing can be said). Rays that start at the apex with unit directions meet the object
// only at t >= key.
DEVI float bound_key(V3 apex, const DevBound &b) {
#pragma clang fp contract(fast)
    if (!(b.r < __builtin_inf())) return 0.f;
    const double wx = b.cx - apex.x, wy = b.cy - apex.y, wz = b.cz - apex.z;
    const double l1 = fabs(wx) + fabs(wy) + fabs(wz);
    const double r_eff = b.r + b.r * (b.k * l1 * (b.cn + l1));
    const double Re = r_eff * 1.00001 + 1e-6 * l1 + 1e-12;
    const double d2 = wx * wx + wy * wy + wz * wz;
    if (d2 <= Re * Re) return 0.f;
    const float dist = __builtin_sqrtf((float)d2) * 0.999999f, rad = (float)Re * 1.000001f;
    return fmaxf(0.f, (dist - rad) * 0.999999f); // NaN / inf - inf -> 0: no bound
}

// Direction (from the light) -> cube-map cell. Face = the axis of the largest component (ties: x before y before z) and
// its sign; (u, v) = the other two components over it, each in [-1, 1]; cell = floor((u + 1) * R / 2), clamped.
// Evaluated in f32 (a third of the f64 form's instructions, one of them a division): the direction is unit, so u/m and v/m carry
// an absolute error below 3e-7 — 2e-5 of a cell — which k_light_cells' cones cover fifty times over (their half-angles are
// widened by 1e-5 rad for exactly this: a direction on a cell border may land in either cell); a tie between two components
// resolved differently than in f64 is a direction on a face border, covered by both faces' border cells the same way.
DEVI uint32_t light_cell(V3 d) {
    const float x = (float)d.x, y = (float)d.y, z = (float)d.z;
    const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    uint32_t a;
    float m, u, v;
    if (ax >= ay && ax >= az) { a = 0u; m = x; u = y; v = z; }
    else if (ay >= az) { a = 1u; m = y; u = z; v = x; }
    else { a = 2u; m = z; u = x; v = y; }
    const float im = __builtin_amdgcn_rcpf(fabsf(m));
    const float fu = (u * im + 1.0f) * (0.5f * RTC_LIGHT_R), fv = (v * im + 1.0f) * (0.5f * RTC_LIGHT_R);
    const int iu = (int)fminf(fmaxf(fu, 0.0f), (float)(RTC_LIGHT_R - 1u)), iv = (int)fminf(fmaxf(fv, 0.0f), (float)(RTC_LIGHT_R - 1u)); // NaN -> 0
    return ((a * 2u + (m < 0.f ? 1u : 0u)) * RTC_LIGHT_R + (uint32_t)iv) * RTC_LIGHT_R + (uint32_t)iu;
}
// Per-lane prefilter for INCOHERENT rays (reflection / refraction): can THIS lane's ray, for some
// t >= 0, touch the object's bounding sphere? false => the exact test would find no entry with
// t >= 0 for this lane. ~22 f64 instructions against 54+ for the exact test; the exact test is
// then issued only if some lane of the wave passes. (For coherent primary / shadow bundles the
// wave-level cull already leaves 1-2 candidates per pass and this filter would only add work.)
DEVI bool ray_touches(V3 o, V3 d, const DevBound &b) {
#pragma clang fp contract(fast) // cull arithmetic, not reference arithmetic: FMA only tightens the rounding the slacks cover
    if (!(b.r < __builtin_inf())) return true;
    const double wx = b.cx - o.x, wy = b.cy - o.y, wz = b.cz - o.z;
    const double Dub = fabs(wx) + fabs(wy) + fabs(wz); // >= |C - o|
    const double R = (b.r + b.r * (b.k * Dub * (b.cn + Dub))) * 1.000001 + 1e-12; // rounding inflation, see DevBound
    const double ww = wx * wx + wy * wy + wz * wz;
    const double R2 = R * R;
    if (ww <= R2) return true;                       // origin inside the sphere
    const double proj = wx * d.x + wy * d.y + wz * d.z;
    if (proj < 0.) return false;                      // sphere wholly behind the origin (ww > R^2)
    const double dd = d.x * d.x + d.y * d.y + d.z * d.z;
    // perp^2 * dd = ww*dd - proj^2 <= R^2 * dd ; the slack covers the cancellation error
    return !(ww * dd - proj * proj > R2 * dd + 1e-11 * ww * dd); // NaN-safe: keep unless provably far
}

// The same question against a pre-inflated record (DevPre, rtc_device.h) — valid for origins with |o|_1 <= pre_limit, which the
// caller checks once per pass. One inequality: with pm = max(proj, 0) the squared distance from the centre to the RAY (t >= 0)
// is ww - pm^2 / dd, so the sphere can be touched only if ww*dd - pm^2 <= R2*dd (+ the cancellation slack); proj < 0 turns it
// into ww <= R2 (origin inside), as the general test has it. `dd` = d.d, computed once per pass.
DEVI bool ray_touches_pre(V3 o, V3 d, double dd, const DevPre &b) {
#pragma clang fp contract(fast) // cull arithmetic
    const double wx = b.cx - o.x, wy = b.cy - o.y, wz = b.cz - o.z;
    const double ww = wx * wx + wy * wy + wz * wz;
    const double pm = fmax(wx * d.x + wy * d.y + wz * d.z, 0.);
    return !(ww * dd - pm * pm > (b.R2 + 1e-11 * ww) * dd); // NaN-safe: keep unless provably far; R2 = inf: never culled
}
// The same test as the MASK of the active lanes it keeps: the compare writes the wave's mask directly (v_cmp -> SGPR pair), where
// ballot(bool) of a value that lives across blocks costs a v_cndmask 0/1 and a second compare. Used in the batched walk of the
// one-level kernels (C4 -1.1 %, reflective 1080p -1.4 %); the same form in the two-level kernels' walks and in the binned walk's
// early-out measured 3 % SLOWER on C3 / C5 (profiles/r03_exp_small_steps.log) and is not used there.
DEVI unsigned long long ray_touches_pre_mask(V3 o, V3 d, double dd, const DevPre &b) {
#pragma clang fp contract(fast) // cull arithmetic
    const double wx = b.cx - o.x, wy = b.cy - o.y, wz = b.cz - o.z;
    const double ww = wx * wx + wy * wy + wz * wz;
    const double pm = fmax(wx * d.x + wy * d.y + wz * d.z, 0.);
    return __builtin_amdgcn_fcmp(ww * dd - pm * pm, (b.R2 + 1e-11 * ww) * dd, 13 /* ULE: !(lhs > rhs) */);
}
// Candidates of a per-lane-filtered walk are taken PRE_BATCH at a time: their records are requested together and their
// prefilters evaluated back to back before any exact test, so that a pass over many candidates — a secondary pass whose bundle
// cannot be bounded visits all 101 objects of the reflective north star — is not one scalar-load round trip per object
// (profiles/r03_exp_unbounded_walks.log: those walks, 0.27 passes per wave, were a third of C4's kernel time).
constexpr uint32_t PRE_BATCH = 2;
// The one-level listed shadow pass (k_trace) takes this many entries of a lane's own cell list per step, their prefilter records
// requested together. Measured 1 / 2 / 4 (profiles/r03_exp_lane_lists.log): 2 and 4 keep 16 / 32 more VGPRs of records live and
// spill in the flat kernel (12 / 24 B per lane) — rejected for that alone — and are 2 % / 5 % slower on the north star, whose cells
// list 0-2 objects; on C4 and the reflective 1080p frame 1 and 2 measure the same.
#ifndef RTC_LANE_LIST_BATCH
#define RTC_LANE_LIST_BATCH 1
#endif
constexpr uint32_t LANE_LIST_BATCH = RTC_LANE_LIST_BATCH;

// ---- wave-uniform object loop ------------------------------------------------------------
// f(j, m, kind, prim) is called for objects j = 0..n-1 in insertion order (World::intersect,
// shape.rs:679-681) and returns true while some lane of the wave still needs objects.
// SRC_SMEM : uniform global loads (scalar cache -> SGPR operands); no barriers.
// SRC_LDS1 : the whole table was staged into LDS once by stage_all(); no barriers.
// SRC_LDSN : tiles of P.tile_cap objects staged by the whole workgroup; EVERY thread of the
//            workgroup must call this the same number of times (barriers inside).
// The World tables are passed as separate `const T *__restrict__` kernel arguments (not inside the
// parameter struct): only then may the compiler treat them as read-only for the whole launch and
// fetch wave-uniform records with scalar loads (s_load through the scalar cache into SGPRs)
// instead of 64 identical vector loads.
struct Tables {
    const DevIsect *__restrict__ isect;
    const uint32_t *__restrict__ kind;
    const DevShade *__restrict__ shade;
    const DevPrim *__restrict__ prim;
    const DevBound *__restrict__ bound;
    // two-level cull tables (Morton order, groups of 64)
    const DevIsect *__restrict__ isect_s;
    const uint32_t *__restrict__ kind_s;
    const DevBound *__restrict__ bound_s;
    const uint32_t *__restrict__ orig_s;
    const DevBound *__restrict__ gbound;
    const DevIdEntry *__restrict__ idtab; // shapes in stable order of world_id (n1/n2 pass)
    const DevPre *__restrict__ pre;       // per-lane prefilter records, insertion order / sorted order
    const DevPre *__restrict__ pre_s;
};

struct LdsView {
    double *m;      // [cap][12]
    double *prim;   // [cap][4]
    uint32_t *kind; // [cap]
};

DEVI LdsView lds_view(double *base, uint32_t cap) {
    LdsView v;
    v.m = base;
    v.prim = base + (size_t)cap * 12;
    v.kind = reinterpret_cast<uint32_t *>(base + (size_t)cap * 16);
    return v;
}

DEVI void stage_tile(const Tables &T, const LdsView &L, uint32_t base, uint32_t cnt) {
    const double *gm = reinterpret_cast<const double *>(T.isect + base);
    for (uint32_t e = threadIdx.x; e < cnt * 12; e += blockDim.x) L.m[e] = gm[e];
    const double *gp = reinterpret_cast<const double *>(T.prim + base);
    for (uint32_t e = threadIdx.x; e < cnt * 4; e += blockDim.x) L.prim[e] = gp[e];
    for (uint32_t e = threadIdx.x; e < cnt; e += blockDim.x) L.kind[e] = T.kind[base + e];
}

// Skip (two-level cull, closest-hit passes of rays that start at the bundle's apex with unit
// directions): skip(key) is wave-uniform and true when no lane can still be improved by an object
// whose intersections all have t >= key. With it the groups of a 64-group step, and the objects of a
// group, are visited in ascending key order and the walk stops at the first key that is out of
// reach for every lane. Results do not depend on the visiting order: closer() compares (t, index).
struct NoSkip {
    DEVI bool operator()(float) const { return false; }
};
// From the lanes flagged in `mask` take the one with the smallest key (ties: lowest lane).
DEVI int take_min_key(unsigned long long &mask, float key, float &kmin) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool in = (mask >> lane) & 1ull;
    const unsigned kb = in ? __builtin_bit_cast(unsigned, key) : 0xffffffffu; // keys are >= 0: bits order like the values
    const unsigned minbits = ~wave_max_u32(~kb);
    const int sel = (int)__builtin_ctzll(ballot(in && kb == minbits));
    mask &= ~(1ull << sel);
    kmin = __builtin_bit_cast(float, minbits);
    return sel;
}

// Shape of the cull walks: a round of the one-level cull tests OS x 64 object spheres, a round of the group level SLOTS x 64
// group spheres (ordered walks then take the nearest key across the whole round), and K surviving groups are expanded
// together. Measured on MI355X (ms per frame, 8 frames per launch): OS/SLOTS/K = 1/1/1: C3 0.234, C5 5.07, north star
// 0.0696; 2/4/2: 0.259 / 5.63 / 0.0724; 4/4/4: 0.274 / 5.99 / 0.0718. Batching the walks buys nothing: these kernels are
// bound by VALU issue slots, not by the length of the load -> test -> ballot dependency chains, so all three
// are fixed at 1. The walks keep their batched form: written for width 1 they compile differently (one-level reflective
// kernels +8..+29 instructions, C4 +0.65 % kernel time; ordered two-level kernels about +100 instructions).
template <int SRC, bool LANE_FILTER = false, class PP, class F, class SK = NoSkip>
DEVI void for_each_object(const PP &P, const Tables &T, const LdsView &L, bool lane_needs, const Bundle &B, F &&f,
                          V3 fro = V3{0., 0., 0.}, V3 frd = V3{0., 0., 0.}, SK skip = SK{}) {
    constexpr bool ORDERED = !__is_same(SK, NoSkip);
    // per-lane prefilter: the pre-inflated records hold while every origin of the pass is within their limit
    bool pre_ok = false;
    double fdd = 0.;
    if constexpr (LANE_FILTER) {
#pragma clang fp contract(fast)
        pre_ok = ballot(lane_needs && !(fabs(fro.x) + fabs(fro.y) + fabs(fro.z) <= P.pre_limit)) == 0ull;
        fdd = frd.x * frd.x + frd.y * frd.y + frd.z * frd.z;
    }
    if constexpr (SRC == SRC_CULL) {
        const unsigned long long needs_mask = ballot(lane_needs); // (lane_needs does not change during the walk)
        // One-level cull (small worlds): up to OS x 64 objects per round, each lane tests one object's sphere of
        // every slot against the wave's bundle (the slots' loads are in flight together: one load -> test -> ballot
        // dependency chain per round instead of one per 64 objects); the ballot masks are walked in ascending
        // (= insertion) order and the survivors get the exact test, their records fetched by uniform index (scalar cache).
        if (ballot(lane_needs) == 0ull) return;
        const uint32_t lane = threadIdx.x & 63u;
        constexpr uint32_t OS = 1; // (walk shape: see above)
        for (uint32_t base = 0; base < P.n; base += 64u * OS) {
            unsigned long long masks[OS];
#pragma unroll
            for (uint32_t sl = 0; sl < OS; ++sl) {
                const uint32_t j = base + sl * 64u + lane;
                bool cand = false;
                if (base + sl * 64u < P.n && j < P.n) cand = bundle_touches(B, T.bound[j]);
                masks[sl] = ballot(cand);
            }
#pragma unroll
            for (uint32_t sl = 0; sl < OS; ++sl) {
                unsigned long long mask = masks[sl];
                if constexpr (LANE_FILTER) {
                    if (pre_ok) { // PRE_BATCH candidates at a time (see ray_touches_pre)
                        while (mask) {
                            uint32_t jx[PRE_BATCH];
                            unsigned long long bx[PRE_BATCH];
                            uint32_t cnt = 0;
#pragma unroll
                            for (uint32_t k = 0; k < PRE_BATCH; ++k) {
                                jx[k] = k ? jx[0] : base + sl * 64u; // (slots past the last candidate repeat the first: a harmless second look)
                                if (mask) {
                                    jx[k] = base + sl * 64u + (uint32_t)__builtin_ctzll(mask);
                                    mask &= mask - 1ull;
                                    cnt = k + 1u;
                                }
                            }
                            DevPre q[PRE_BATCH]; // all requested before the first is used: one round trip for the batch
#pragma unroll
                            for (uint32_t k = 0; k < PRE_BATCH; ++k) q[k] = T.pre[jx[k]];
#pragma unroll
                            for (uint32_t k = 0; k < PRE_BATCH; ++k) {
                                bx[k] = ray_touches_pre_mask(fro, frd, fdd, q[k]) & needs_mask; // (evaluated by every lane: no branch around the loads)
                            }
#pragma unroll
                            for (uint32_t k = 0; k < PRE_BATCH; ++k) {
                                if (k >= cnt || bx[k] == 0ull) continue;
                                const DevIsect rec = T.isect[jx[k]]; // record and kind requested together, ahead of the callback's branches
                                const uint32_t kd = T.kind[jx[k]];
                                if (!f((int)jx[k], rec.m, kd, (const double *)nullptr)) return;
                            }
                        }
                        continue;
                    }
                }
                while (mask) {
                    const uint32_t jj = base + sl * 64u + (uint32_t)__builtin_ctzll(mask);
                    mask &= mask - 1ull;
                    if constexpr (LANE_FILTER) {
                        if (ballot(lane_needs && ray_touches(fro, frd, T.bound[jj])) == 0ull) continue;
                    }
                    const DevIsect *rec = T.isect + jj;
                    if (!f((int)jj, rec->m, T.kind[jj], (const double *)nullptr)) return;
                }
            }
        }
    } else if constexpr (SRC == SRC_CULL2) {
        // Two-level cull (large worlds) over the Morton-sorted tables. Level 1: group spheres against the wave's
        // bundle, one per lane and slot. Level 2: the 64 objects of surviving groups, one object sphere per lane —
        // K groups per round, their bounds loaded and tested together (one dependency chain per round).
        // Objects are not visited in insertion order here, so the callback receives the insertion index and the
        // tie-break compares it (closer()).
        if (ballot(lane_needs) == 0ull) return;
        const uint32_t lane = threadIdx.x & 63u;
        constexpr uint32_t SLOTS = 1, K = 1; // (walk shape: see above)
        // level 2 for the `cnt` (<= K) groups gidx[0..cnt); returns false when the walk is over (callback said so)
        auto expand = [&](const uint32_t (&gidx)[K], uint32_t cnt) -> bool {
            unsigned long long masks[K];
            float okey[K];
#pragma unroll
            for (uint32_t k = 0; k < K; ++k) {
                bool cand = false;
                okey[k] = 0.f;
                if (k < cnt) {
                    const uint32_t j = gidx[k] * 64u + lane;
                    if (j < P.n) cand = bundle_touches<ORDERED>(B, T.bound_s[j], &okey[k]);
                }
                masks[k] = ballot(cand);
            }
#pragma unroll
            for (uint32_t k = 0; k < K; ++k) {
                unsigned long long mask = masks[k];
                const uint32_t base = (k < cnt ? gidx[k] : 0u) * 64u;
                while (mask) {
                    uint32_t jj;
                    if constexpr (ORDERED) {
                        float kmin;
                        jj = base + (uint32_t)take_min_key(mask, okey[k], kmin);
                        if (skip(kmin)) break;
                    } else {
                        jj = base + (uint32_t)__builtin_ctzll(mask);
                        mask &= mask - 1ull;
                    }
                    if constexpr (LANE_FILTER) {
                        if (ballot(lane_needs && (pre_ok ? ray_touches_pre(fro, frd, fdd, T.pre_s[jj]) : ray_touches(fro, frd, T.bound_s[jj]))) == 0ull) continue;
                    }
                    const DevIsect *rec = T.isect_s + jj;
                    if (!f((int)T.orig_s[jj], rec->m, T.kind_s[jj], (const double *)nullptr)) return false;
                }
            }
            return true;
        };
        for (uint32_t gbase = 0; gbase < P.ngroups; gbase += 64u * SLOTS) {
            // one round of level 1: group (gbase + s*64 + lane) for s = 0..SLOTS-1, all loads in flight together
            unsigned kb[SLOTS];               // ordered: key bits (keys are >= 0: they order like unsigned); ~0u = no candidate
            unsigned long long gm[SLOTS];     // unordered: candidate masks
#pragma unroll
            for (uint32_t sl = 0; sl < SLOTS; ++sl) {
                const uint32_t g = gbase + sl * 64u + lane;
                bool gc = false;
                float gkey = 0.f;
                if (gbase + sl * 64u < P.ngroups && g < P.ngroups)
                    gc = bundle_touches<ORDERED>(B, T.gbound[g], &gkey);
                kb[sl] = gc ? __builtin_bit_cast(unsigned, gkey) : 0xffffffffu;
                gm[sl] = ballot(gc);
            }
            if constexpr (ORDERED) {
                // the round's queue: nearest key first over ALL its slots. Each lane keeps its own minimum; the wave
                // minimum picks the lane, that lane's slot is read back and struck out. K groups are taken per expansion.
                for (bool more = true; more;) {
                    uint32_t gidx[K];
                    uint32_t cnt = 0;
#pragma unroll
                    for (uint32_t k = 0; k < K; ++k) {
                        gidx[k] = 0u;
                        if (!more) continue;
                        unsigned mine = kb[0];
                        uint32_t msl = 0;
#pragma unroll
                        for (uint32_t sl = 1; sl < SLOTS; ++sl)
                            if (kb[sl] < mine) { mine = kb[sl]; msl = sl; }
                        const unsigned minbits = ~wave_max_u32(~mine);
                        // queue empty, or ascending keys: the rest is out of reach too
                        if (minbits == 0xffffffffu || skip(__builtin_bit_cast(float, minbits))) { more = false; continue; }
                        const int sel = (int)__builtin_ctzll(ballot(mine == minbits));
                        const uint32_t ssl = (uint32_t)__builtin_amdgcn_readlane((int)msl, sel);
#pragma unroll
                        for (uint32_t sl = 0; sl < SLOTS; ++sl)
                            if (sl == ssl && lane == (uint32_t)sel) kb[sl] = 0xffffffffu;
                        gidx[k] = gbase + ssl * 64u + (uint32_t)sel;
                        cnt = k + 1u;
                    }
                    if (cnt == 0u) break;
                    if (!expand(gidx, cnt)) return;
                }
            } else {
                uint32_t gidx[K];
                uint32_t cnt = 0;
#pragma unroll
                for (uint32_t sl = 0; sl < SLOTS; ++sl) {
                    unsigned long long gmask = gm[sl];
                    while (gmask) {
                        gidx[cnt++] = gbase + sl * 64u + (uint32_t)__builtin_ctzll(gmask);
                        gmask &= gmask - 1ull;
                        if (cnt == K) {
                            if (!expand(gidx, cnt)) return;
                            cnt = 0;
                        }
                    }
                }
                if (cnt != 0u && !expand(gidx, cnt)) return;
            }
        }
    } else if constexpr (SRC == SRC_SMEM) {
        if (ballot(lane_needs) == 0ull) return;
        for (uint32_t j = 0; j < P.n; ++j) {
            const DevIsect *rec = T.isect + j;
            if (!f((int)j, rec->m, T.kind[j], reinterpret_cast<const double *>(T.prim + j))) break;
        }
    } else if constexpr (SRC == SRC_LDS1) {
        if (ballot(lane_needs) == 0ull) return;
        for (uint32_t j = 0; j < P.n; ++j) {
            const uint32_t kind = __builtin_amdgcn_readfirstlane(L.kind[j]);
            if (!f((int)j, L.m + j * 12, kind, L.prim + j * 4)) break;
        }
    } else {
        bool wave_live = ballot(lane_needs) != 0ull;
        for (uint32_t base = 0; base < P.n; base += P.tile_cap) {
            const uint32_t cnt = (P.n - base < P.tile_cap) ? (P.n - base) : P.tile_cap;
            __syncthreads(); // previous tile fully consumed
            stage_tile(T, L, base, cnt);
            __syncthreads();
            if (wave_live) {
                for (uint32_t j = 0; j < cnt; ++j) {
                    const uint32_t kind = __builtin_amdgcn_readfirstlane(L.kind[j]);
                    if (!f((int)(base + j), L.m + j * 12, kind, L.prim + j * 4)) { wave_live = false; break; }
                }
            }
        }
    }
}

// ---- stages k_trace and k_aov share ------------------------------------------------------------------------------
// Shape::normal_at shape.rs:34-40: the world normal at `point`, before the inside flip. A plane's normal does not depend on
// the point: it was evaluated once per object at rtc_world_create (DevShade::plane_n).
// WAVE_NORM: the sphere's and the cube's normalisation through vnormalize_wave (the flat k_trace kernels), same bits.
template <bool WAVE_NORM = false> DEVI V3 shape_normal(const DevShade *S, const double *m_obj, V3 point) {
    V3 ln = mk(0., 1., 0.);
    const uint32_t kind = S->kind;
    if (kind == RTC_SPHERE) {
        const V3 lp = xpoint(m_obj, point);
        ln = mk(lp.x - 0., lp.y - 0., lp.z - 0.);
    } else if (kind == RTC_CUBE) { // Cube::normal_at_local shape.rs:601-610
        const V3 lp = xpoint(m_obj, point);
        const double ax = fabs(lp.x), ay = fabs(lp.y), az = fabs(lp.z);
        const double maxc = fmax(ax, fmax(ay, az));
        if (maxc == ax) ln = mk(lp.x, 0., 0.);
        else if (maxc == ay) ln = mk(0., lp.y, 0.);
        else ln = mk(0., 0., lp.z);
    }
    if (kind == RTC_PLANE) return mk(S->plane_n[0], S->plane_n[1], S->plane_n[2]);
    if constexpr (WAVE_NORM) {
        double mag;
        return vnormalize_wave(xvector3(S->nt, ln), mag);
    }
    return vnormalize_plain(xvector3(S->nt, ln));
}
// The same function for a caller that already holds the object's kind (trace_short_chains' SC_KIND: nothing waits for
// DevShade::kind's load) and, GROUPED, with the two records a sphere's or a cube's normal reads — rows 0..2 of the inverse and
// DevShade::nt, both at addresses the hit index alone decides — requested together, ahead of the arithmetic (SC_NORMAL). The
// operations and their operands are shape_normal's.
// SP, MP: the two records' pointer types — per-lane global pointers, or the constant address space's for a tile whose hit lanes
// all name one object (trace_uniform_shade): `kind` is then wave-uniform too, the switch is a scalar branch and the records
// arrive in SGPRs.
template <bool WAVE_NORM, bool GROUPED, class SP, class MP> DEVI V3 shape_normal_of(uint32_t kind, SP S, MP m_obj, V3 point) {
    if (kind == RTC_PLANE) return mk(S->plane_n[0], S->plane_n[1], S->plane_n[2]);
    double mi[12], nt[9];
    if constexpr (GROUPED) {
#pragma unroll
        for (int i = 0; i < 12; ++i) mi[i] = m_obj[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) nt[i] = S->nt[i];
    }
    V3 ln = mk(0., 1., 0.);
    if (kind == RTC_SPHERE) {
        const V3 lp = GROUPED ? xpoint(mi, point) : xpoint(m_obj, point);
        ln = mk(lp.x - 0., lp.y - 0., lp.z - 0.);
    } else if (kind == RTC_CUBE) {
        const V3 lp = GROUPED ? xpoint(mi, point) : xpoint(m_obj, point);
        const double ax = fabs(lp.x), ay = fabs(lp.y), az = fabs(lp.z);
        const double maxc = fmax(ax, fmax(ay, az));
        if (maxc == ax) ln = mk(lp.x, 0., 0.);
        else if (maxc == ay) ln = mk(0., lp.y, 0.);
        else ln = mk(0., 0., lp.z);
    }
    const V3 wn = GROUPED ? xvector3(nt, ln) : xvector3(S->nt, ln);
    if constexpr (WAVE_NORM) {
        double mag;
        return vnormalize_wave(wn, mag);
    }
    return vnormalize_plain(wn);
}

// The shadow ray of is_shadowed_by_light (shape.rs:717-719): v = light - over_point, its length, three divisions. Lanes
// without a hit keep the `dir` and `dist` they came with. WAVE_NORM: through vnormalize_wave (the flat k_trace kernels), same bits.
template <bool WAVE_NORM = false> DEVI void shadow_ray(V3 light_pos, V3 over, bool hit, V3 &dir, double &dist) {
    if (hit) {
        const V3 v = vsub(light_pos, over);
        if constexpr (WAVE_NORM) {
            dir = vnormalize_wave(v, dist);
            return;
        }
        dist = sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
        dir = mk(v.x / dist, v.y / dist, v.z / dist);
    }
}

// The closest-hit walk's body (World::intersect + get_hit, streaming form): the exact test of object j for the lanes still
// tracing, folded into (best, hidx, hroot). Never stops the walk. Holds references, as a [&] lambda would.
template <bool BARE> struct ClosestHitT {
    const bool &tracing;
    const V3 &ro, &rd;
    double &best;
    int &hidx, &hroot;
    template <class M, class Q> DEVI bool operator()(int j, M m, uint32_t kind, Q) const {
        if (tracing) closest_world<BARE>(kind, m, ro, rd, j, best, hidx, hroot);
        return true;
    }
};
using ClosestHit = ClosestHitT<false>;

// The any-hit walk's body (is_shadowed shape.rs:721-726): the exact test of one object for the lanes still pending — the
// first object in the way settles a lane — and the walk goes on while some lane is pending. Holds references, as a [&]
// lambda would.
template <bool BARE> struct AnyHitT {
    bool &pending;
    const V3 &over, &dir;
    const double &dist;
    bool &shadowed;
    template <class M, class Q> DEVI bool operator()(int, M m, uint32_t kind, Q) const {
        if (pending) {
            if (occludes_world<BARE>(kind, m, over, dir, dist)) { shadowed = true; pending = false; }
        }
        return ballot(pending) != 0ull; // stop as soon as no lane is pending
    }
};
using AnyHit = AnyHitT<false>;

// ---- patterns (material.rs:41-45 and the six pattern_at bodies) --------------------------
template <bool BARE = false, class SP, class MP> DEVI V3 pattern_color(SP S, MP m_obj, V3 world_point) {
    const V3 op = xpoint(m_obj, world_point);
    const V3 pp = xpoint(S->pat_inv, op);
    const V3 a = mk(S->pat_a[0], S->pat_a[1], S->pat_a[2]);
    const V3 b = mk(S->pat_b[0], S->pat_b[1], S->pat_b[2]);
    switch (S->pattern_kind) {
    case RTC_PATTERN_TEST: return pp;
    case RTC_PATTERN_STRIPE: return rtc_even_f64(floor(pp.x)) ? a : b; // (`% 2.0 == 0.0`: rtc_parity.h)
    case RTC_PATTERN_GRADIENT: {
        const V3 diff = vsub(b, a); // GradientPattern::new: _diff = b.sub(a)
        return vadd(a, vmul(diff, pp.x - floor(pp.x)));
    }
    case RTC_PATTERN_RING: return rtc_even_f64(floor(BARE ? sqrt_wave(pp.x * pp.x + pp.y * pp.y) : sqrt(pp.x * pp.x + pp.y * pp.y))) ? a : b;
    case RTC_PATTERN_CHECKER: return rtc_even_f64(floor(pp.x) + floor(pp.y) + floor(pp.z)) ? a : b;
    case RTC_PATTERN_GRID:
        return (fabs(pp.x - floor(pp.x)) < 0.01 || fabs(pp.z - floor(pp.z)) < 0.01) ? b : a;
    default: return mk(0., 0., 0.);
    }
}

// Material::lighting material.rs:319-361. lightv = (light.position - point).normalize() is
// the shadow ray's direction (same expression, shape.rs:717-719), passed in.
// SP, MP: as shape_normal_of's — with the constant address space's pointers the material's scalars and the pattern record are
// scalar operands and the pattern switch is a scalar branch.
template <bool BARE = false, class PP, class SP, class MP>
DEVI V3 lighting(const PP &P, SP S, MP m_obj, V3 point, V3 eyev, V3 normal,
                 V3 lightv, bool in_shadow) {
    // The reference's statement order is effective_color, lightv, ambient, [shadow?] light_dot_normal,
    // diffuse, reflectv, reflect_dot_eye, factor, specular. The values do not depend on that order
    // (no shared rounding), so the geometric scalars and the one expensive call (pow) are done FIRST,
    // while little else is live, and the colour arithmetic afterwards.
    double ldn = 0., kspec = 0.;
    bool lit = false, spec = false;
    if (!in_shadow) {
        ldn = vdot(lightv, normal);
        if (!(ldn < 0.)) {
            lit = true;
            const V3 reflectv = vreflect(vneg(lightv), normal);
            const double rde = vdot(reflectv, eyev);
            if (!(rde <= 0.)) {
                // factor = rde.powf(shininess) (material.rs:355). When specular == 0 and the power is
                // certainly finite and positive (0 < rde <= 1, 0 <= shininess < inf), specular*factor is
                // exactly specular (a signed zero) whatever the power is: skip the ~200-instruction pow.
                const double ks = S->specular, sh = S->shininess;
                const bool trivial = (ks == 0.0) && (rde <= 1.0) && (sh >= 0.0) && (sh < __builtin_inf());
                const double factor = trivial ? 1.0 : pow(rde, sh);
                kspec = ks * factor;
                spec = true;
            }
        }
    }
    asm volatile("" ::: "memory"); // the material colour / pattern loads start here, not above the pow
    const V3 I = mk(P.light_int[0], P.light_int[1], P.light_int[2]);
    const V3 base = (S->pattern_kind != RTC_PATTERN_NONE) ? pattern_color<BARE>(S, m_obj, point)
                                                          : mk(S->color[0], S->color[1], S->color[2]);
    const V3 eff = vmulv(base, I);
    const V3 ambient = vmul(eff, S->ambient);
    if (in_shadow) return ambient;
    V3 diffuse = mk(0., 0., 0.), specular = mk(0., 0., 0.);
    if (lit) {
        diffuse = vmul(eff, S->diffuse * ldn);
        if (spec) specular = vmul(I, kspec);
    }
    return vadd(vadd(ambient, diffuse), specular);
}

// lighting()'s view of a light that is not the parameter block's own (lights 1..n-1 of a multi-light World)
struct LightInt {
    double light_int[3];
};
template <class T, class... R> DEVI const T &first_of(const T &t, const R &...) { return t; }
template <class T> DEVI const T &last_of(const T &t) { return t; }
template <class T, class U, class... R> DEVI const auto &last_of(const T &, const U &u, const R &...r) { return last_of(u, r...); }
// Does k_trace's trailing argument pack end in a DevLens (a thin-lens launch)?
template <class... T> constexpr bool has_lens_v = (false || ... || __is_same(T, DevLens));
// ... or in a DevProjection (an orthographic or panorama launch)?
template <class... T> constexpr bool has_projection_v = (false || ... || __is_same(T, DevProjection));
// Lights 1..n-1 of the multi-light loop, from the kernel arguments (DevExtraLights) or from the World's table in HBM
// (DevLightTable, 6 doubles per light). `i` is wave-uniform: plain loads, which the compiler may issue as scalar ones.
DEVI uint32_t further_light_count(const DevExtraLights &X) { return X.n; }
DEVI V3 further_light_position(const DevExtraLights &X, uint32_t i) { return mk(X.pos[i][0], X.pos[i][1], X.pos[i][2]); }
DEVI LightInt further_light_intensity(const DevExtraLights &X, uint32_t i) { return LightInt{{X.inten[i][0], X.inten[i][1], X.inten[i][2]}}; }
DEVI uint32_t further_light_count(const DevLightTable &X) { return X.n; }
DEVI V3 further_light_position(const DevLightTable &X, uint32_t i) { return mk(X.rec[6u * i], X.rec[6u * i + 1u], X.rec[6u * i + 2u]); }
DEVI LightInt further_light_intensity(const DevLightTable &X, uint32_t i) { return LightInt{{X.rec[6u * i + 3u], X.rec[6u * i + 4u], X.rec[6u * i + 5u]}}; }

// World::reflectance (Schlick) shape.rs:768-781
DEVI double reflectance(V3 eyev, V3 normal, double n1, double n2) {
    double cosv = vdot(eyev, normal);
    if (n1 > n2) {
        const double n = n1 / n2;
        const double sin2_t = (n * n) * (1.0 - cosv * cosv);
        if (sin2_t > 1.0) return 1.0;
        cosv = sqrt(1.0 - sin2_t);
    }
    const double q = (n1 - n2) / (n1 + n2);
    const double r0 = q * q;
    const double x = 1.0 - cosv;
    const double x2 = x * x;
    return r0 + (1.0 - r0) * (x * (x2 * x2)); // powi(5)
}

// The parameter block lives in the kernarg segment. Its loads are invariant, so LLVM hoists every
// one of them to the kernel entry and then has to carry ~80 SGPRs through the whole kernel (they
// spill into VGPR lanes). KP(P_arg) hands out a fresh, opaque constant-address-space view of the
// same block; loads through it stay in the phase that asked for it.
// (RenderParams is the kernel's FIRST argument, i.e. offset 0 of the kernarg segment.)
typedef const __attribute__((address_space(4))) RenderParams *ParamPtr;
DEVI ParamPtr param_view() {
    unsigned long long a = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return (ParamPtr)a;
}
#define KP(arg) (*param_view())
// The tile lists and their counts through the same address space: k_trace never writes them (k_bin_tiles did, in an earlier
// dispatch), and a wave asks for its own tile's — a wave-uniform address — so the loads are scalar ones and the words arrive
// in SGPRs.
typedef const __attribute__((address_space(4))) uint32_t *ConstWords;
DEVI ConstWords const_words(const uint32_t *p) { return (ConstWords)(unsigned long long)p; }
// The packed tile lists' walk in k_trace: 1 = the scalar walk over k_bin_tiles' sorted lists, 0 = the wave-minimum extraction
// (which does not care about the lists' order), kept for the A/B. trace_scalar_walk: the instantiations that take it.
#ifndef RTC_SCALAR_TILE_WALK
#define RTC_SCALAR_TILE_WALK 1
#endif
// The flat one-level k_trace kernels (SRC_CULL, no frame stack) with the binned pass take the scalar walk for the sorted
// lists — the launches whose lists k_bin_tiles sorts (rtc_launch_binning's `sort`: the host asks for it for exactly these
// worlds). Not the two-level kernels: at 10 000 objects the binning kernel is as long as the render kernel and has no time
// to spare. Not the frame-stack kernels: the primary pass is a small part of their frames, and with both walks in it the
// reflective whole-tile kernel measured 0.6 % slower (C4). Not the anti-aliased kernels of Worlds with several lights, which
// came out of the compiler with 4 to 8 B per lane more scratch than they had. All of those keep the wave-minimum extraction
// alone, which walks lists in any order, and their code is the parent's (tools/kernel_resources.py, tools/isa_compare.py;
// profiles/sorted_lists_*). `lights`: 0 one light, 1 the further lights in the kernel arguments (DevExtraLights), 2 in the
// World's table (DevLightTable).
constexpr bool trace_scalar_walk(int src, bool refl, bool one, int lights) {
    if (RTC_SCALAR_TILE_WALK == 0 || src != SRC_CULL || refl) return false;
    if (!one && lights != 0) return false;
    return true;
}
// Vector::normalize through vnormalize_wave (one reciprocal per normalisation, chosen per wave) in the flat k_trace kernels:
// a mask of sites, 1 = the pinhole ray generation, 2 = shadow_ray, 4 = shape_normal; 0 = vnormalize_plain and the three
// divisions everywhere, the code as it was (kept for the A/B). trace_wave_normalize: the instantiations that take it — the
// render flavour of SRC_CULL and SRC_CULL2 without a frame stack, one light, pinhole camera (with ONE and WHOLE and without).
// The frame-stack kernels sit at their register limit (the per-lane form cost them 1.2 %,
// profiles/r03_exp_shared_normalize.log); they, the multi-light, lens, projection, brute-force and probe instantiations and
// k_aov, k_ao and k_gather are the parent's code (tools/isa_compare.py; profiles/shared_normalize_flat_*).
#ifndef RTC_SHARED_NORMALIZE_FLAT
#define RTC_SHARED_NORMALIZE_FLAT 7
#endif
constexpr bool trace_wave_normalize(int site, int src, bool refl, bool probe, bool alt, bool multi) {
    return (RTC_SHARED_NORMALIZE_FLAT & site) != 0 && IS_CULL(src) && !refl && !probe && !alt && !multi;
}
// Shorter chains of dependent loads per tile in the flat one-sample k_trace kernels: loads are moved, merged or requested
// together, no arithmetic changes. A mask of items, 0 = the code as it was in every kernel (kept for the A/B):
//   1  the tile header's two tile_rows words through scalar loads (const_words), not a per-lane load + readfirstlane
//   2  the tile lookup in the tile header: the kernel arguments it needs in one group, then tile_rows' words, the tile's
//      count and its list's first entry in one more
//   4  unbounded objects of the binned primary pass: orig_s[k], kind_s[k] and isect_s[k] requested together
//   8  the packed tile-list walks: kind[j], isect[j] and prim[j] requested together, ahead of the kind switch
//  16  the hit object's kind carried per lane beside hidx (binned pass) instead of DevShade::kind's load before the normal
//  32  sphere and cube normal: isect[hidx].m and DevShade::nt requested together
//  64  the shadow-list stage's kernel arguments in one group
// 128  a lane's own light cell: its counter and the first batch of its list requested together
// trace_short_chains: the instantiations that take an item — the one-sample render flavour of SRC_CULL without a frame stack,
// one light (with WHOLE and without). Every other kernel is the parent's code (tools/isa_compare.py; profiles/short_chains_*).
#ifndef RTC_SHORT_CHAINS
#define RTC_SHORT_CHAINS 255
#endif
enum { SC_ROWS = 1, SC_LOOKUP = 2, SC_UNBOUNDED = 4, SC_WALK = 8, SC_KIND = 16, SC_NORMAL = 32, SC_SHADOW_ARGS = 64, SC_CELL = 128 };
constexpr bool trace_short_chains(int item, int src, bool refl, bool one, bool multi) {
    return (RTC_SHORT_CHAINS & item) != 0 && src == SRC_CULL && !refl && one && !multi;
}
// One-object tiles shaded from scalar registers in the flat one-sample k_trace kernels. After the closest-hit pass a wave
// asks whether every lane that hit something hit the SAME object (one ballot, one lane read, one compare; lanes that hit
// nothing do not count). If so, the hit's DevShade and the rows of its inverse are read through the constant address space at
// that wave-uniform index — scalar loads into SGPRs, scalar operands of the VALU, scalar branches on the kind and the pattern —
// by the very functions the per-lane path calls (shape_normal_of, lighting, pattern_color, instantiated for the other pointer
// type): the operations, their order and their operands' values are the same, only where an operand comes from differs. Mixed
// tiles take the per-lane path as before. A mask, 0 = the code as it was in every kernel (kept for the A/B):
//   1  SRC_CULL's flat one-sample kernels, one light (trace_short_chains' family: whole-tile, one-sample, its RGBA form)
//   2  SRC_CULL2's flat one-sample kernel, one light
// The run-time switch RTC_UNIFORM_SHADE=0 sends a launch to an instantiation without the path (DevPerLaneShade), as
// RTC_ONE_SAMPLE=0 sends it to the generic kernel: the host's choice, no branch per tile.
#ifndef RTC_UNIFORM_SHADE
#define RTC_UNIFORM_SHADE 3
#endif
constexpr bool trace_uniform_shade(int src, bool refl, bool one, bool multi) {
    return (((RTC_UNIFORM_SHADE & 1) != 0 && src == SRC_CULL) || ((RTC_UNIFORM_SHADE & 2) != 0 && src == SRC_CULL2)) && !refl && one && !multi;
}
// k_trace's trailing argument of the instantiations RTC_UNIFORM_SHADE=0 selects: a tag, nothing is read from it.
struct DevPerLaneShade {
    uint32_t unused;
};
typedef const __attribute__((address_space(4))) DevShade *ConstShade;
typedef const __attribute__((address_space(4))) double *ConstDoubles;

// One suspended shade_hit call (shape.rs:685-700) on a lane's stack. The stack lives in scratch
// (dynamic index), so its size is HBM/L2 traffic: Worlds without transparent materials (REFR ==
// false) recurse along a single chain `surface + color_at(reflected ray) * kr` and need only
// (surface, kr) = 32 bytes per level instead of 152 (1080p reflective north star: 1.67 GB of
// scratch writes per frame with the full frame).
template <bool REFR> struct FrameT;
template <> struct FrameT<true> {
    V3 surface;
    V3 a;           // state 0: origin of the pending refraction ray; state 1: the reflected colour (the ray has left)
    V3 rd;          // state 0: direction of the pending refraction ray
    double kr, tr, R;
    uint8_t rem;    // `remaining` of the color_at call that owns the frame
    uint8_t state;  // 0 waiting for the reflected child, 1 waiting for the refracted child
    uint8_t schlick;
    uint8_t has_refr;
};
template <> struct FrameT<false> {
    V3 surface;
    double kr;
};

// scale255 (Color::scale(component, 255)) and gamma_byte (Canvas::to_imgbuf's channel): rtc_gamma.h, shared with rtc_shutter.hip

// The RGBA form of a tile's 8-bit store (Canvas::to_imgbuf: R, G, B, alpha 255 — canvas.rs:74): `rows` x `cols` pixels of
// the 3-byte staging (rows SRC_STRIDE bytes apart) to rows orow0.. / columns px0.. of `out8` (4 B/pixel, W pixels per row),
// NT threads, this one number t. Whole rows of FULL pixels on a 4-byte aligned buffer: one dword per pixel, consecutive
// threads on consecutive pixels; anything else byte by byte.
template <uint32_t FULL, uint32_t SRC_STRIDE, uint32_t NT>
DEVI void store_rgba(const unsigned char *src8, unsigned char *out8, uint32_t W, uint32_t orow0, uint32_t px0, uint32_t rows,
                     uint32_t cols, uint32_t t) {
    if (cols == FULL && ((size_t)out8 % 4u) == 0) {
        for (uint32_t c = t; c < rows * FULL; c += NT) {
            const uint32_t r = c / FULL, x = c % FULL;
            const unsigned char *q = src8 + r * SRC_STRIDE + x * 3u;
            const unsigned v = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | 0xff000000u;
            __builtin_nontemporal_store(v, reinterpret_cast<unsigned *>(out8 + ((size_t)(orow0 + r) * W + px0 + x) * 4u));
        }
    } else {
        for (uint32_t c = t; c < rows * cols; c += NT) {
            const uint32_t r = c / cols, x = c % cols;
            const unsigned char *q = src8 + r * SRC_STRIDE + x * 3u;
            unsigned char *d = out8 + ((size_t)(orow0 + r) * W + px0 + x) * 4u;
            d[0] = q[0];
            d[1] = q[1];
            d[2] = q[2];
            d[3] = 255u;
        }
    }
}

// Offsets of Camera::resample's extra rays (camera.rs:84-92). The reference draws them from
// thread_rng; the documented counter-based stand-in (include/rtc.h, rtc_camera.samples): SplitMix64 of
// ((y*hsize + x) << 16 | draw), top 53 bits -> [0, 1).
DEVI double resample_offset(uint32_t W, uint32_t x, uint32_t y, uint32_t draw) {
    unsigned long long z = ((((unsigned long long)y * W + x) << 16) | draw) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-53;
}

// shade_hit's final combination shape.rs:692-699
DEVI V3 combine(V3 surface, V3 reflected, V3 refracted, bool schlick, double R) {
    if (schlick) return vadd(surface, vadd(vmul(reflected, R), vmul(refracted, 1.0 - R)));
    return vadd(vadd(surface, reflected), refracted);
}

// ---- the kernel -------------------------------------------------------------------------
// PROBE = true is the rtc_color_at flavour (arbitrary rays in, colours + hit records out); the
// render flavour (PROBE = false) never carries the hit record's extra vectors in registers.
// RGBA = true (render flavour only) is the launch with a gamma table (RenderParams::gamma): the 8-bit output is
// Canvas::to_imgbuf's RGBA. Its own instantiation, so that the RGB kernels' code and resources stay exactly as they are.
// XL: empty for a World with one light — the kernels as they always were, argument list included. One DevExtraLights
// (rtc_device.h) for a World with several (MULTI): lights 1..n-1 ride behind the tables in the kernarg segment, and the
// shadow and lighting stages loop over them (shade_hit with the FIXME at shape.rs:686 filled in: the sum of every light's
// lighting(), each with its own is_shadowed_by_light, shape.rs:716). Instantiated only for the sources a multi-light launch
// takes (SRC_SMEM, SRC_CULL, SRC_CULL2). One DevLightTable instead: the same loop reading the lights from the World's table
// in HBM (more than RTC_MAX_LIGHTS samples: area lights) — same sources, same flavours, nothing new stored.
// A DevLens as the LAST element of XL (alone, or behind the lights' block): the thin-lens flavour (LENS, rtc_render_lens*).
// Every pixel is Color::average_over of usteps * vsteps rays whose origin moves over the lens; the origin of sample k is the
// same for every pixel, so it takes the camera origin's place as the wave-uniform shared apex of the primary bundle. What
// assumes the PINHOLE origin is compiled out: the tile lists, the per-view DevPrim table (closest_prim), the black tile-row
// proof. Same sources as the multi-light kernels, render flavour only (no PROBE, no RGBA); three running sums per lane.
// A DevProjection in the DevLens' place (never both): the projection flavour (PROJ, rtc_render_projection*), one for both kinds.
// Only the ray generation differs — a wave-uniform branch on the kind: an orthographic pixel's ray starts at its own point of
// the camera's z = 0 plane (per-lane origins: the primary bundle is make_bundle's general form, no ordered walk), a panorama
// pixel's direction is the product of two host-computed {sin, cos} table entries and starts at the camera origin (shared apex,
// ordered walk, as the pinhole kernels; a tile too wide to bound runs with B.off). It compiles out what LENS compiles out,
// and the lens' running sums as well: one ray per pixel. Same sources, render flavour only.
// ONE = true (render flavour of SRC_CULL and SRC_CULL2, never LENS or PROJ): the launch of a camera with samples == 1, the reference's
// default (Camera::render_async) and the only launch the benchmark makes. `aa` is the constant false, so the sample loop is one
// straight pass and the sub-sample store, the resample test and the averaging are not part of the code: nothing of them is
// carried — spilled — across the tile loop and the pass loop. The generic kernel takes exactly this path when P.samples == 1,
// so the results cannot differ; rtc_launch_trace sends a launch here only when P.samples == 1 (RTC_ONE_SAMPLE=0: never).
// WHOLE = true (on top of ONE; one light, f64 output only): a launch of ONE camera whose every tile is a whole 8-row tile of
// contiguous rows inside the canvas — whole_tile_launch below, the launcher's condition (RTC_WHOLE_TILES=0: never). Every lane
// is in range and traced, the view is views[0], band_stride is 1, and the output stage is the 16-byte form alone: the
// per-lane range state, the view and band terms and the narrow and 8-bit output forms are not part of the code. The ONE
// kernel evaluates each of them to exactly these constants for such a launch, so the results cannot differ.
// __launch_bounds__' waves per SIMD of a k_trace instantiation (the macros above).
constexpr int trace_waves_per_simd(int src, bool refl, bool one, bool whole) {
    if (refl) return RTC_WAVES_PER_SIMD_STACK;
    return (src == SRC_CULL && one && whole) ? RTC_WAVES_PER_SIMD_WHOLE : RTC_WAVES_PER_SIMD;
}
template <int SRC, bool REFL, bool REFR, bool PROBE, bool RGBA = false, bool ONE = false, bool WHOLE = false, class... XL>
__global__ void __launch_bounds__(RTC_BLOCK_FOR(CULL_LEVEL(SRC), REFL, REFR, PROBE), trace_waves_per_simd(SRC, REFL, ONE, WHOLE))
k_trace(const RenderParams P_arg, const DevIsect *__restrict__ t_isect, const uint32_t *__restrict__ t_kind,
        const DevShade *__restrict__ t_shade, const DevPrim *__restrict__ t_prim, const DevBound *__restrict__ t_bound,
        const DevIsect *__restrict__ t_isect_s, const uint32_t *__restrict__ t_kind_s, const DevBound *__restrict__ t_bound_s,
        const uint32_t *__restrict__ t_orig_s, const DevBound *__restrict__ t_gbound, const DevIdEntry *__restrict__ t_idtab,
        const DevPre *__restrict__ t_pre, const DevPre *__restrict__ t_pre_s, const XL... xl_arg) {
    constexpr bool LENS = has_lens_v<XL...>;
    constexpr bool PROJ = has_projection_v<XL...>;
    constexpr bool ALT = LENS || PROJ; // primary rays that are not the pinhole's: whatever assumes the camera origin is compiled out
    constexpr bool PER_LANE = (false || ... || __is_same(XL, DevPerLaneShade)); // RTC_UNIFORM_SHADE=0's instantiation: the tag alone
    constexpr bool MULTI = sizeof...(XL) - (ALT ? 1 : 0) - (PER_LANE ? 1 : 0) != 0;
    static_assert(!PER_LANE || (sizeof...(XL) == 1 && trace_uniform_shade(SRC, REFL, ONE, false)), "the per-lane twin of a kernel that has the uniform path");
    static_assert(!(LENS && PROJ), "a lens or a projection, never both");
    static_assert(sizeof...(XL) <= (ALT ? 2 : 1), "at most one block of further lights, then at most one lens or projection");
    static_assert(!ALT || ((SRC == SRC_SMEM || IS_CULL(SRC)) && !PROBE && !RGBA), "lens and projection launches take SRC_SMEM, SRC_CULL or SRC_CULL2, f64 / RGB output");
    static_assert(!ONE || (IS_CULL(SRC) && !PROBE && !ALT), "the one-sample flavour: pinhole render launches of SRC_CULL and SRC_CULL2");
    static_assert(!WHOLE || (ONE && !RGBA && !MULTI), "the whole-tile flavour: one-sample launches of one light, f64 output");
    constexpr uint32_t BLOCK = RTC_BLOCK_FOR(CULL_LEVEL(SRC), REFL, REFR, PROBE), TILE_W = RTC_TILE_W_FOR(CULL_LEVEL(SRC), REFL, REFR, PROBE);
    extern __shared__ double lds_raw[];
    // Reflection-only Worlds keep their 32-byte frames (surface, kr) in LDS instead of scratch memory: 5 levels x 4 doubles x
    // 64 lanes = 10 KB per wave, SoA ([level][component][lane]: lane-consecutive 8-byte accesses, no bank conflicts). The
    // scratch stack was HBM traffic: C4 wrote 941 MB and fetched 236 MB per frame against 453 MB algorithmic
    // (profiles/r02_a_c4_pmc.json). The output tile is staged in the same LDS (the stack is dead by then), so a one-wave
    // workgroup still fits 16 times in a CU's 160 KB.
    constexpr bool LDS_STACK = REFL && !REFR;
    // Tile output: each wave stores its own 8x8 part as soon as it is done (frame-stack kernels, whose waves finish far apart:
    // 0.662 vs 0.690 ms), or a workgroup barrier + cooperative store of the whole tile in full 128-byte lines (flat kernels:
    // 0.0738 vs 0.0784 ms, the per-wave 192-byte row pieces straddle lines).
    constexpr bool WAVE_OUTPUT = REFL;
    // Per-lane prefilter (ray_touches) in front of the shadow pass's exact tests (secondary closest passes always take it).
    // Two-level cull: a dense world's shadow bundle keeps ~17 candidates per pass, of which each lane's own segment touches
    // few: 1000 spheres 0.535 -> 0.423 ms, 10 000 spheres 0.560 -> 0.462 ms. Frame-stack kernels: shadow segments from
    // scattered secondary hits (6.7 exact tests per pass without it), reflective 1080p 0.551 -> 0.536 ms. Not for the flat
    // one-level cull: at 100 objects (~2 candidates per pass) it costs more than it saves (0.0754 -> 0.0767 ms).
    constexpr bool SHADOW_LANE_FILTER = SRC == SRC_CULL2 || REFL;
    static_assert(!LDS_STACK || BLOCK == 64, "the tile is staged over the LDS frame stack: one wave per workgroup");
    __shared__ __attribute__((aligned(16))) double stack_lds[LDS_STACK ? RTC_MAX_STACK * 4 * BLOCK : 2];
    __shared__ __attribute__((aligned(16))) double stage_own[(PROBE || LDS_STACK) ? 2 : 8 * TILE_W * 3];     // the tile, canvas layout
    __shared__ __attribute__((aligned(16))) unsigned char stage_own8[(PROBE || LDS_STACK) ? 16 : 8 * TILE_W * 3];
    // with the LDS stack the tile is staged over it (every lane's stack is empty when its sample is done)
    double *const stage_f64 = LDS_STACK ? stack_lds : stage_own;
    unsigned char *const stage_u8 = LDS_STACK ? reinterpret_cast<unsigned char *>(stack_lds + 8 * TILE_W * 3) : stage_own8;
    const auto &P = KP(P_arg); // set-up view: grid, sizes, mode
    const LdsView L = lds_view(lds_raw, P.tile_cap);
    Tables T;
    T.isect = t_isect; T.kind = t_kind; T.shade = t_shade; T.prim = t_prim; T.bound = t_bound;
    T.isect_s = t_isect_s; T.kind_s = t_kind_s; T.bound_s = t_bound_s; T.orig_s = t_orig_s; T.gbound = t_gbound;
    T.idtab = t_idtab;
    T.pre = t_pre; T.pre_s = t_pre_s;

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr bool probe = PROBE;

    if constexpr (SRC == SRC_LDS1) { // the whole object table, once per workgroup
        stage_tile(T, L, 0, P.n);
        __syncthreads();
    }
    uint32_t c_primary = 0, c_shadow = 0, c_reflect = 0, c_refract = 0; // wave-uniform
    uint32_t c_resample = 0;            // wave-uniform: pixels that tripped the resample test
    uint32_t c_sky = 0;                 // wave-uniform: primary rays of tiles proven black (sky_tile)
    // A workgroup renders `reps` tiles, one after the other: tile ids blockIdx.x, blockIdx.x + gridDim.x, ... (consecutive
    // workgroups still land on consecutive XCDs). The canvas stores of tile k then drain while tile k+1 is traced (a wave cannot
    // retire before its stores are acknowledged), and the per-wave set-up and the counter atomics are paid once per `reps` tiles.
    uint32_t wg_reps = PROBE ? 1u : P.reps, wg_base = blockIdx.x, wg_stride = gridDim.x;
    if (!PROBE && (P.chunk_wgs[0] | P.chunk_wgs[1] | P.chunk_wgs[2] | P.chunk_wgs[3])) { // guided chunks (RenderParams::chunk_wgs)
        const uint32_t n8 = P.chunk_wgs[0], n4 = P.chunk_wgs[1], n3 = P.chunk_wgs[2], n2 = P.chunk_wgs[3];
        uint32_t b = blockIdx.x;
        if (b < n8) { wg_reps = 8u; wg_base = b; wg_stride = n8; }
        else if ((b -= n8) < n4) { wg_reps = 4u; wg_base = 8u * n8 + b; wg_stride = n4; }
        else if ((b -= n4) < n3) { wg_reps = 3u; wg_base = 8u * n8 + 4u * n4 + b; wg_stride = n3; }
        else if ((b -= n3) < n2) { wg_reps = 2u; wg_base = 8u * n8 + 4u * n4 + 3u * n3 + b; wg_stride = n2; }
        else { wg_reps = 1u; wg_base = 8u * n8 + 4u * n4 + 3u * n3 + 2u * n2 + (b - n2); wg_stride = 0u; }
    }
    const uint32_t reps = wg_reps;
    for (uint32_t rep = 0; rep < reps; ++rep) {
    // tile = workgroup id: the hardware deals consecutive ids round-robin over the 8 XCDs, so each XCD gets every 8th tile, an
    // even share of sky, floor and spheres. Contiguous XCD bands (for L2 locality, of which there is none to gain: a 50 KB scene,
    // a write-once canvas) measured 0.099 vs 0.073 ms on the north star, 1.07 vs 0.69 ms reflective.
    const uint32_t bid = wg_base + rep * wg_stride;
    if (!PROBE && bid >= P.total_blocks) break; // (workgroup-uniform)
    uint32_t px = 0, py = 0, ray_index = 0;
    uint32_t view = 0, tbid = bid; // which camera of the launch, and the tile's index inside that view
    // The tile's column and row in the view's grid: decomposed ONCE per tile (one unsigned division; two with several views),
    // wave-uniform, and used by the ray set-up, the black-row test, the tile-list lookup and the output stage alike.
    uint32_t bx = 0, by = 0;
    bool in_range, traced;
    if (probe) {
        ray_index = bid * BLOCK + threadIdx.x;
        in_range = ray_index < P.nrays;
        traced = in_range;
    } else {
        const uint32_t tiles = P.grid_x * P.grid_y;
        if (!WHOLE && P.nviews > 1u) { view = bid / tiles; tbid = bid % tiles; }
        by = tbid / P.grid_x;
        bx = tbid - by * P.grid_x;
        px = bx * TILE_W + wave * 8u + (lane & 7u);
        py = P.y0 + by * (WHOLE ? 1u : P.band_stride) * 8u + (lane >> 3);
        in_range = WHOLE || (px < P.W && py < P.y1);
        // Camera::render leaves the last row and column untouched (camera.rs:120-121)
        traced = WHOLE || (in_range && !(P.mode == RTC_MODE_RENDER && (px + 1u >= P.W || py + 1u >= P.H)));
    }

    // Tile rows the binning kernel PROVED black for this view (k_bin_tiles, `rows`): no ray is generated, no pass is run, the
    // tile is stored as Canvas::new left it; the primary rays the reference would have cast are still counted (and reported
    // separately, rtc_stats::rays_primary_proven_miss). One-sample renders only. Such a tile goes from here to the output
    // stage: it skips the sample loop with its camera loads, and stores its zeros through the same code as every other tile.
    bool sky_tile = false;
    // trace_short_chains' SC_LOOKUP: the proof's words come with the tile's list, further down (tile_header)
    constexpr bool HEADER_LOOKUP = trace_short_chains(SC_LOOKUP, SRC, REFL, ONE, MULTI);
    // SC_KIND: the binned pass keeps the kind of each lane's closest object beside hidx — it holds every tested object's kind
    // in an SGPR — and the normal starts from that instead of waiting for DevShade::kind, which the host fills from the same
    // rtc_shape::kind as kind[] and kind_s[] (flatten_shapes, for rtc_world_create and rtc_world_update alike). The walks
    // that are not the binned pass (no lists, an overflowing list) read DevShade::kind as before.
    constexpr bool CARRY_KIND = trace_short_chains(SC_KIND, SRC, REFL, ONE, MULTI);
    // RTC_BARE_SQRT's sites in this kernel (vnormalize_wave has site 1 in itself)
    constexpr bool BARE_PRIMARY = trace_bare_sqrt(BS_PRIMARY, SRC, REFL, PROBE, ALT, MULTI), BARE_SHADOW = trace_bare_sqrt(BS_SHADOW, SRC, REFL, PROBE, ALT, MULTI),
                   BARE_RING = trace_bare_sqrt(BS_RING, SRC, REFL, PROBE, ALT, MULTI);
    if constexpr (IS_CULL(SRC) && !PROBE && !ALT && !HEADER_LOOKUP) { // (the proof is for rays from the camera origin)
        const auto &Pt = KP(P_arg);
        if (Pt.tile_rows != nullptr && (ONE || Pt.samples == 1u)) {
            const uint32_t ity = (Pt.y0 >> 3) + by * (WHOLE ? 1u : Pt.band_stride);
            uint32_t first, lastinv;
            if constexpr (trace_short_chains(SC_ROWS, SRC, REFL, ONE, MULTI)) { // k_bin_tiles wrote them, the view is wave-uniform: scalar loads
                first = const_words(Pt.tile_rows)[2u * view], lastinv = const_words(Pt.tile_rows)[2u * view + 1u];
            } else {
                first = Pt.tile_rows[2u * view], lastinv = Pt.tile_rows[2u * view + 1u];
            }
            sky_tile = ity < first || ity > ~lastinv; // (no tile of the view is non-empty: first = 0xffffffff)
        }
        if (sky_tile) { // counted as cast (the reference casts them), answered by the proof
            const uint32_t cast = WHOLE ? 64u : popc64(ballot(traced)); // (WHOLE: every lane of the wave is traced)
            c_primary += cast;
            c_sky += cast;
        }
    }

    // Binned primary pass: this wave's 8x8 tile has a list of the objects its primary rays can touch (k_bin_tiles): lane e
    // holds entry e. Requested where the pass needs it: a request at kernel entry, ahead of the ray generation, measured
    // slower (north star +3 %, C5 +4 %; profiles/r02_exp_packed_tile_lists.log).
    // SCALAR_WALK: the count and the list's first entry come through scalar loads, issued together, into SGPRs (a sorted
    // list's entry k IS the k-th smallest, k_bin_tiles) — no per-lane list state; the lists that are not sorted (longer than
    // RTC_TILE_SORT_CAP, or a launch that did not sort) are read per lane where their walk starts.
    constexpr int LIGHTS = (false || ... || __is_same(XL, DevExtraLights)) ? 1 : (false || ... || __is_same(XL, DevLightTable)) ? 2 : 0;
    constexpr bool SCALAR_WALK = IS_CULL(SRC) && !PROBE && !ALT && trace_scalar_walk(SRC, REFL, ONE, LIGHTS);
    bool binned = false;
    uint32_t bin_cnt = 0, bin_ent = 0xffffffffu;
    ConstWords bin_list = nullptr; // SCALAR_WALK: the tile's list (wave-uniform)
    uint32_t bin_head = 0;         // SCALAR_WALK: its entry 0 (an empty list's: whatever the slot holds, never used)
    auto tile_lookup = [&]() {
        const auto &Pt = KP(P_arg);
        if (Pt.tile_cnt != nullptr) {
            const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave); // wave-uniform by construction
            const uint32_t itx = bx * (TILE_W / 8u) + wv, ity = (Pt.y0 >> 3) + by * (WHOLE ? 1u : Pt.band_stride);
            if (WHOLE || (itx < Pt.tiles_x && ity < Pt.tiles_y)) { // (WHOLE: every tile of the launch is a tile of the image)
                const size_t tile = (size_t)((WHOLE ? 0u : view * Pt.tiles_y) + ity) * Pt.tiles_x + itx;
                if constexpr (SCALAR_WALK) {
                    bin_list = const_words(Pt.tile_list) + tile * RTC_TILE_LIST_CAP;
                    bin_cnt = const_words(Pt.tile_cnt)[tile];
                    bin_head = bin_list[0];
                } else {
                    bin_cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)Pt.tile_cnt[tile]);
                    if (lane < bin_cnt) bin_ent = Pt.tile_list[tile * RTC_TILE_LIST_CAP + lane];
                }
                binned = bin_cnt <= RTC_TILE_LIST_CAP; // an overflowing list is incomplete: walk instead
            }
        }
    };
    // HEADER_LOOKUP: the black-row test and tile_lookup in one place, two scalar round trips per tile. First the kernel
    // arguments both read, one group; then — both addresses are known from those — the view's two tile_rows words and
    // the tile's count and first list entry, one more. Every pointer is tested before anything is read through it, as above;
    // a one-sample pinhole launch looks its tile up in its only pass, so nothing is asked for that the pass would not ask
    // for, except by the tiles proven black (their tile is a tile of the same tables: in bounds).
    if constexpr (HEADER_LOOKUP) {
        static_assert(SCALAR_WALK, "the header lookup is the scalar walk's");
        const auto &Pt = KP(P_arg);
        unsigned long long q_cnt = (unsigned long long)Pt.tile_cnt, q_list = (unsigned long long)Pt.tile_list, q_rows = (unsigned long long)Pt.tile_rows;
        uint32_t a_tiles_x = Pt.tiles_x, a_tiles_y = WHOLE ? 0u : Pt.tiles_y;
        const uint32_t a_y0 = P.y0; // (the set-up view's, with its grid_x: the tile's decomposition above reads both)
        // (the empty statement takes and returns its operands in SGPRs: every load above has been asked for, and is waited
        // for once, before one of the values is looked at; left to itself the compiler asks for each where it is first used)
        asm volatile("" : "+s"(q_cnt), "+s"(q_list), "+s"(q_rows), "+s"(a_tiles_x), "+s"(a_tiles_y) : "s"(a_y0), "s"(P.grid_x));
        const ConstWords a_cnt = (ConstWords)q_cnt, a_list = (ConstWords)q_list, a_rows = (ConstWords)q_rows;
        const uint32_t ity = (a_y0 >> 3) + by * (WHOLE ? 1u : Pt.band_stride);
        uint32_t first = 0u, lastinv = 0u; // (no proof: no row is below 0 or above 0xffffffff)
        bool looked_up = false;
        if (a_rows != nullptr) first = a_rows[2u * view], lastinv = a_rows[2u * view + 1u];
        if (a_cnt != nullptr) {
            const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave); // wave-uniform by construction
            const uint32_t itx = bx * (TILE_W / 8u) + wv;
            if (WHOLE || (itx < a_tiles_x && ity < a_tiles_y)) { // (WHOLE: every tile of the launch is a tile of the image)
                const size_t tile = (size_t)((WHOLE ? 0u : view * a_tiles_y) + ity) * a_tiles_x + itx;
                bin_list = a_list + tile * RTC_TILE_LIST_CAP;
                bin_cnt = a_cnt[tile];
                bin_head = bin_list[0];
                looked_up = true;
            }
        }
        asm volatile("" : "+s"(first), "+s"(lastinv), "+s"(bin_cnt), "+s"(bin_head)); // the four words: one wait
        binned = looked_up && bin_cnt <= RTC_TILE_LIST_CAP; // an overflowing list is incomplete: walk instead
        sky_tile = ity < first || ity > ~lastinv; // (no tile of the view is non-empty: first = 0xffffffff)
        if (sky_tile) { // counted as cast (the reference casts them), answered by the proof
            const uint32_t cast = WHOLE ? 64u : popc64(ballot(traced));
            c_primary += cast;
            c_sky += cast;
        }
    }

    // render_pixel (camera.rs:94-114): one ray, or the 4 fixed sub-samples followed — for the pixels whose
    // samples differ by more than 0.01 from their mean — by `resample_n` more rays (Camera::resample)
    const bool aa = !ONE && !ALT && !probe && P.samples != 1u; // (ONE: P.samples == 1, the launcher's condition)
    uint32_t nsamples = aa ? 4u : 1u;   // grows to 4 + resample_n after sample 3 when some lane resamples
    // thin lens: sample s = lens_v * usteps + lens_u (v outer, u inner), Color::average_over's running sums in registers
    uint32_t lens_u = 0u, lens_v = 0u;
    V3 lens_sum = mk(0., 0., 0.);
    if constexpr (LENS) {
        const DevLens &LZ = last_of(xl_arg...);
        nsamples = LZ.usteps * LZ.vsteps;
    }
    bool lane_resample = false;         // this lane's pixel tripped the test AND the resample is enabled
    // per thread: the four sub-samples (12 doubles) and Color::average_over's running sums (3 doubles)
    double *aa_store = reinterpret_cast<double *>(reinterpret_cast<char *>(lds_raw) + P.aa_lds_off) + threadIdx.x * 15u;
    V3 result = mk(0., 0., 0.);

    typedef FrameT<REFR> Frame;
    Frame stack[(REFL && !LDS_STACK) ? RTC_MAX_STACK : 1];
    // LDS stack: level l, component c of this thread's ray at stack_lds[(l*4 + c) * BLOCK + threadIdx.x] (a ray never leaves
    // its lane)
    double *lstk = stack_lds + threadIdx.x;

    for (uint32_t s = sky_tile ? nsamples : 0u; s < nsamples; ++s) { // (a tile proven black: no sample at all)
        V3 ro, rd;
        bool shared_origin;
        const auto &Pr = KP(P_arg).views[WHOLE ? 0u : view]; // ray-generation view: this workgroup's camera block
        // ray origin of every primary ray: transform_point(view_inv, (0,0,0)) camera.rs:72 — as the host evaluated it when
        // every element of view_inv is finite (DevCamera::origin: the same operations on the same operands, the same bits),
        // evaluated here otherwise (NaN signs and payloads are the device's own)
        V3 cam_origin;
        if (!LENS && Pr.origin_ok != 0u) { // (the lens flavour replaces the origin below)
            cam_origin = mk(Pr.origin[0], Pr.origin[1], Pr.origin[2]);
        } else {
            cam_origin = xpoint(Pr.vinv, mk(0., 0., 0.));
            cam_origin = mk(uniform_f64(cam_origin.x), uniform_f64(cam_origin.y), uniform_f64(cam_origin.z)); // same in every lane
        }
        V3 lens_origin_v = cam_origin; // (lens flavour: the sample's origin as computed, in VGPRs)
        if constexpr (LENS) {
            // the lens sample's origin (include/rtc.h): a point of the lens in camera space, the same for every pixel of the
            // launch — it takes the camera origin's place as ray origin and, moved to SGPRs, as the primary bundle's shared apex
            // (RTC_LENS_UNIFORM_ORIGIN, rtc_device.h)
            const DevLens &LZ = last_of(xl_arg...);
            const double lu = -LZ.aperture + LZ.ucell * ((double)lens_u + 0.5);
            const double lv = -LZ.aperture + LZ.vcell * ((double)lens_v + 0.5);
            cam_origin = xpoint(Pr.vinv, mk(lu, lv, 0.0));
            lens_origin_v = cam_origin;
            if constexpr (RTC_LENS_UNIFORM_ORIGIN != 0)
                cam_origin = mk(uniform_f64(cam_origin.x), uniform_f64(cam_origin.y), uniform_f64(cam_origin.z));
            if (++lens_u == LZ.usteps) { lens_u = 0u; ++lens_v; }
        }
        if (probe) {
            const double *rp = P.rays + (size_t)(in_range ? ray_index : 0u) * 6;
            ro = mk(rp[0], rp[1], rp[2]);
            rd = mk(rp[3], rp[4], rp[5]);
            shared_origin = false;
        } else {
            // Camera::ray_for_pixel_offset camera.rs:64-76; sub-sample offsets camera.rs:98,102-105
            double xo = 0.5, yo = 0.5;
            if (aa) {
                if (s < 4u) { xo = (s & 1u) ? 0.75 : 0.25; yo = (s & 2u) ? 0.75 : 0.25; }
                else { xo = resample_offset(P.W, px, py, 2u * (s - 4u)); yo = resample_offset(P.W, px, py, 2u * (s - 4u) + 1u); }
            }
            const double xoffset = ((double)px + xo) * Pr.pixel_size;
            const double yoffset = ((double)py + yo) * Pr.pixel_size;
            const double world_x = Pr.half_width - xoffset;
            const double world_y = Pr.half_height - yoffset;
            if constexpr (PROJ) { // include/rtc.h's projection rays, in its order (the pinhole's world_x / world_y above are dead code here)
                const DevProjection &PJ = last_of(xl_arg...);
                if (PJ.kind == RTC_PROJ_ORTHOGRAPHIC) { // (wave-uniform) parallel rays from the camera's z = 0 plane
                    const double ox = PJ.half_w - ((double)px + 0.5) * PJ.pixel;
                    const double oy = PJ.half_h - ((double)py + 0.5) * PJ.pixel;
                    ro = xpoint(Pr.vinv, mk(ox, oy, 0.));
                    rd = vnormalize_plain(vsub(xpoint(Pr.vinv, mk(ox, oy, -1.)), ro));
                    shared_origin = false;
                } else { // panorama: {sin, cos} of the pixel's longitude and latitude from the host's tables, one 16-byte load each
                    typedef double SinCos __attribute__((ext_vector_type(2)));
                    const SinCos c = *reinterpret_cast<const SinCos *>(PJ.col + 2u * (size_t)(in_range ? px : 0u)); // (lanes outside the canvas: entry 0)
                    const SinCos r = *reinterpret_cast<const SinCos *>(PJ.row + 2u * (size_t)(in_range ? py : 0u));
                    const V3 target = xpoint(Pr.vinv, mk(r.y * c.x, r.x, -(r.y * c.y)));
                    ro = cam_origin;
                    rd = vnormalize_plain(vsub(target, cam_origin));
                    shared_origin = true;
                }
            } else if constexpr (LENS) { // the pixel's point on the plane in focus
                const DevLens &LZ = last_of(xl_arg...);
                const V3 target = xpoint(Pr.vinv, mk(world_x * LZ.focal_distance, world_y * LZ.focal_distance, -LZ.focal_distance));
                // (RTC_LENS_UNIFORM_ORIGIN == 2: the exact tests read the origin from VGPRs — same bits — and only the bundle's apex from SGPRs)
                ro = RTC_LENS_UNIFORM_ORIGIN == 2 ? lens_origin_v : cam_origin;
                rd = vnormalize_plain(vsub(target, ro));
                shared_origin = RTC_LENS_UNIFORM_ORIGIN != 0;
            } else {
            const V3 pixel = xpoint(Pr.vinv, mk(world_x, world_y, -1.));
            ro = cam_origin;
            if constexpr (trace_wave_normalize(1, SRC, REFL, PROBE, ALT, MULTI)) {
                double mag;
                rd = vnormalize_wave(vsub(pixel, cam_origin), mag);
            } else {
                rd = vnormalize_plain(vsub(pixel, cam_origin));
            }
            shared_origin = true;
            }
        }

        bool tracing = traced && (ALT || s < 4u || lane_resample);
        bool first = true; // this ray is the one color_at was called with (depth 0)
        int rem = (int)P.remaining;
        int sp = 0;
        c_primary += WHOLE ? 64u : popc64(ballot(tracing)); // (WHOLE: every lane of the wave starts out tracing)

        // Worlds without reflective / transparent materials (REFL == false) need exactly one pass per
        // primary ray; otherwise loop until every lane's frame stack has unwound.
        for (bool pass_again = true; pass_again;) {
            if constexpr (REFL) {
                bool any_tracing;
                if constexpr (SRC == SRC_LDSN) any_tracing = __syncthreads_or(tracing ? 1 : 0) != 0;
                else any_tracing = ballot(tracing) != 0ull;
                if (!any_tracing) break;
            } else {
                pass_again = false;
            }

            // ---- World::intersect + get_hit (shape.rs:677-683, 220-232), streaming form ----
            double best = __builtin_inf();
            int hidx = -1, hroot = 0;
            Bundle B{}; // every field defined: an undefined field turns into a value carried around the pass loop
            B.off = true;
            if constexpr (IS_CULL(SRC) && !PROBE && !ALT && !HEADER_LOOKUP) { // (HEADER_LOOKUP: looked up with the tile's header)
                if (shared_origin && first) tile_lookup();
            }
            const bool use_bins = !ALT && binned && shared_origin && first; // (binned is false in the probe and brute-force variants)
            if constexpr (IS_CULL(SRC)) {
                if (ballot(tracing) != 0ull && !use_bins) {
                    if (shared_origin && first) B = make_bundle<true, false>(tracing, cam_origin, ro, rd, 0.);
                    else B = make_bundle<false, false>(tracing, cam_origin, ro, rd, 0.);
                }
            }
            if (!IS_CULL(SRC) && !ALT && shared_origin && first) { // (DevPrim: the CAMERA origin in object space)
                for_each_object<SRC>(P, T, L, tracing, B, [&](int j, auto m, uint32_t kind, auto pr) {
                    if (tracing) closest_prim(kind, m, pr, rd, j, best, hidx, hroot);
                    return true;
                });
            } else if (IS_CULL(SRC) && REFL && !(shared_origin && first)) {
                // reflection / refraction rays: incoherent, per-lane prefilter before the exact test
                for_each_object<SRC, true>(P, T, L, tracing, B, ClosestHit{tracing, ro, rd, best, hidx, hroot}, ro, rd);
            } else if (IS_CULL(SRC) && !PROBE && use_bins) {
                // binned primary pass: the unbounded objects, then the tile's own list (k_bin_tiles) — together
                // every object this tile's rays can touch
                // (the view's primary-ray constants come from the binning kernel's table: only the direction is transformed)
                const auto &Pb = KP(P_arg);
                const DevPrim *__restrict__ vprim = WHOLE ? T.prim : T.prim + (size_t)view * Pb.n;
                // closest_prim: the camera origin in object space and the sphere's c from that table, 24 VALU instructions
                // fewer per sphere test than transforming the origin again (closest_world)
                auto binned_test = [&](uint32_t kind, const double *m, uint32_t j) {
                    closest_prim<BARE_PRIMARY>(kind, m, reinterpret_cast<const double *>(vprim + j), rd, (int)j, best, hidx, hroot);
                    // CARRY_KIND: object j is a lane's closest hit exactly when hidx names it after its test; its kind goes above
                    // the root bit of hroot (0 or 1, and read by the refractive kernels only): no further value beside hidx
                    if constexpr (CARRY_KIND) {
                        if (hidx == (int)j) hroot = (hroot & 1) | (int)(kind << 1);
                    }
                };
                // trace_short_chains' SC_WALK / SC_UNBOUNDED: the kind, the record and the DevPrim row of object j (record
                // and kind at `recs` / `kinds`) as values, requested together ahead of the kind switch — which otherwise
                // stands between the kind's load and the others'. A plane's test reads one row of them.
                // `j_loaded`: j itself comes from a load (orig_s[k]) that is still under way — then it, the kind and the record
                // are one group and the DevPrim row, whose address needs j, a second one.
                auto binned_test_grouped = [&](auto kinds, const DevIsect *recs, uint32_t at, uint32_t j, bool j_loaded) {
                    uint32_t kd = kinds[at];
                    DevIsect rec = recs[at];
                    // (all of it in SGPRs here: asked for together, one wait — see the tile header)
                    if (j_loaded)
                        asm volatile("" : "+s"(j), "+s"(kd), "+s"(rec.m[0]), "+s"(rec.m[1]), "+s"(rec.m[2]), "+s"(rec.m[4]), "+s"(rec.m[5]),
                                     "+s"(rec.m[6]), "+s"(rec.m[8]), "+s"(rec.m[9]), "+s"(rec.m[10]));
                    DevPrim pr = vprim[j];
                    if (j_loaded)
                        asm volatile("" : "+s"(pr.ox), "+s"(pr.oy), "+s"(pr.oz), "+s"(pr.c));
                    else
                        asm volatile("" : "+s"(kd), "+s"(rec.m[0]), "+s"(rec.m[1]), "+s"(rec.m[2]), "+s"(rec.m[4]), "+s"(rec.m[5]), "+s"(rec.m[6]),
                                     "+s"(rec.m[8]), "+s"(rec.m[9]), "+s"(rec.m[10]), "+s"(pr.ox), "+s"(pr.oy), "+s"(pr.oz), "+s"(pr.c));
                    const double prv[4] = {pr.ox, pr.oy, pr.oz, pr.c};
                    closest_prim<BARE_PRIMARY>(kd, rec.m, prv, rd, (int)j, best, hidx, hroot);
                    if constexpr (CARRY_KIND) {
                        if (hidx == (int)j) hroot = (hroot & 1) | (int)(kd << 1);
                    }
                };
                // ... and what the two loops below read of the kernel arguments — their bounds and the one table pointer that is
                // not in registers yet — asked for here, together (operands of an empty statement: in SGPRs at this point).
                // kind_s is then read through const_words' address space, as the tile lists are: written when the World was
                // built, never by k_trace (a pointer that has been such an operand reads through scalar loads only from there).
                if constexpr (trace_short_chains(SC_UNBOUNDED, SRC, REFL, ONE, MULTI)) {
                    unsigned long long q_kind_s = (unsigned long long)T.kind_s;
                    asm volatile("" : "+s"(q_kind_s) : "s"(Pb.n_unb), "s"(Pb.bin_packed));
                    for (uint32_t k = 0; k < Pb.n_unb; ++k) {
                        const uint32_t jo = T.orig_s[k];
                        if (tracing) binned_test_grouped((ConstWords)q_kind_s, T.isect_s, k, jo, true);
                    }
                } else {
                if constexpr (trace_short_chains(SC_WALK, SRC, REFL, ONE, MULTI))
                    asm volatile("" ::"s"(Pb.n_unb), "s"(Pb.bin_packed));
                for (uint32_t k = 0; k < Pb.n_unb; ++k) {
                    const uint32_t jo = T.orig_s[k];
                    if (tracing) binned_test(T.kind_s[k], T.isect_s[k].m, jo);
                }
                }
                // the tile's list, nearest first: lane e holds entry e and the lower bound of the distance from the camera to
                // its (inflated) bounding sphere — every intersection of that object has t >= key for these unit-direction
                // rays — and the walk stops at the first key no lane can use any more (as the ordered group walk does)
                if (SCALAR_WALK && Pb.bin_packed == 2u && bin_cnt <= RTC_TILE_SORT_CAP) {
                    // entry = key's upper 16 bits (truncated: still a lower bound) above the object index, and the list is
                    // sorted ascending by it (k_bin_tiles): entry k is the k-th nearest object and its key. A scalar loop
                    // over the count, entries in SGPRs — the sequence of exact tests and early-out decisions of the
                    // wave-minimum extraction below, without the reduction. Entry k + 1 is requested before entry k's test:
                    // one scalar load beside the test's own kind[j] load, answered under the same wait (slot k + 1 <= 16 is
                    // one of the tile's own 64 slots; used only when it is below the count). Eight entries per load, held in
                    // SGPRs, was compiled first: picking entry k mod 8 out of them is a chain of seven compare-and-select
                    // pairs per entry, 14 scalar instructions where this form has one load.
                    uint32_t e_next = bin_head;
                    for (uint32_t k = 0; k < bin_cnt; ++k) {
                        const uint32_t e = e_next;
                        e_next = bin_list[k + 1u];
                        const float kmin = __builtin_bit_cast(float, e & 0xffff0000u);
                        if (ballot(tracing && !(best < (double)kmin)) == 0ull) break;
                        const uint32_t j = e & 0xffffu;
                        if constexpr (trace_short_chains(SC_WALK, SRC, REFL, ONE, MULTI)) {
                            if (tracing) binned_test_grouped(T.kind, T.isect, j, j, false);
                        } else {
                            if (tracing) binned_test(T.kind[j], T.isect[j].m, j);
                        }
                    }
                } else if (Pb.bin_packed) {
                    // the same walk over lists in any order: lane e holds entry e, the wave's minimum IS the next object and
                    // its key
                    if constexpr (SCALAR_WALK) { // (the per-lane form of the list, which the scalar walk does not need)
                        if (lane < bin_cnt) bin_ent = ((const uint32_t *)(unsigned long long)bin_list)[lane];
                    }
                    uint32_t ent = lane < bin_cnt ? bin_ent : 0xffffffffu;
                    for (;;) {
                        const uint32_t e = ~wave_max_u32(~ent);
                        if (e == 0xffffffffu) break;
                        const float kmin = __builtin_bit_cast(float, e & 0xffff0000u);
                        if (ballot(tracing && !(best < (double)kmin)) == 0ull) break;
                        if (ent == e) ent = 0xffffffffu;
                        const uint32_t j = e & 0xffffu;
                        if constexpr (trace_short_chains(SC_WALK, SRC, REFL, ONE, MULTI)) {
                            if (tracing) binned_test_grouped(T.kind, T.isect, j, j, false);
                        } else {
                            if (tracing) binned_test(T.kind[j], T.isect[j].m, j);
                        }
                    }
                } else { // more than 65 536 objects: plain indices, keys from the bounds
                    uint32_t my_j = 0u;
                    float my_key = 0.f;
                    if constexpr (SCALAR_WALK) { // (the per-lane form of the list, which only this walk needs)
                        if (lane < bin_cnt) bin_ent = ((const uint32_t *)(unsigned long long)bin_list)[lane];
                    }
                    if (lane < bin_cnt) {
                        my_j = bin_ent;
                        my_key = bound_key(cam_origin, T.bound[my_j]);
                    }
                    unsigned long long lmask = bin_cnt >= 64u ? ~0ull : ((1ull << bin_cnt) - 1ull);
                    while (lmask) {
                        float kmin;
                        const int sel = take_min_key(lmask, my_key, kmin);
                        if (ballot(tracing && !(best < (double)kmin)) == 0ull) break;
                        const uint32_t j = (uint32_t)__builtin_amdgcn_readlane((int)my_j, sel);
                        if (tracing) binned_test(T.kind[j], T.isect[j].m, j);
                    }
                }
            } else if (SRC == SRC_CULL2 && !PROBE && shared_origin && first) {
                // primary rays of a large world: start at the apex, unit direction -> ordered walk with early stop
                for_each_object<SRC, false>(P, T, L, tracing, B, ClosestHitT<BARE_PRIMARY>{tracing, ro, rd, best, hidx, hroot}, ro, rd, [&](float key) { return ballot(tracing && !(best < (double)key)) == 0ull; });
            } else {
                for_each_object<SRC>(P, T, L, tracing, B, ClosestHitT<BARE_PRIMARY>{tracing, ro, rd, best, hidx, hroot}, ro, rd);
            }
            const bool hit = tracing && hidx >= 0;
            const auto &Ph = KP(P_arg); // shading view: light
            const V3 lightp = mk(Ph.light_pos[0], Ph.light_pos[1], Ph.light_pos[2]);

            // ---- Intersection::compute_vectors (shape.rs:144-152, 75-96) --------------------
            V3 point = mk(0, 0, 0), eyev = mk(0, 0, 0), normal = mk(0, 0, 0), over = mk(0, 0, 0), under = mk(0, 0, 0),
               reflectv = mk(0, 0, 0), sdir = mk(0, 0, 0);
            double sdist = 0., n1 = 1.0, n2 = 1.0, m_kr = 0., m_tr = 0.;
            bool inside = false;
            const DevShade *S = T.shade + (hit ? hidx : 0);
            const double *m_obj = T.isect[hit ? hidx : 0].m;
            // trace_uniform_shade's test, where `hit` and `hidx` are final: does every lane that hit something name the object
            // the lowest hit lane names? Then `u_obj` is that object, else — and for a tile without a hit, where nothing is
            // shaded — NOT_UNIFORM, which is no object's index (the tables hold fewer than 2^31 objects: hidx is an int).
            constexpr bool UNIFORM_SHADE = !PER_LANE && trace_uniform_shade(SRC, REFL, ONE, MULTI);
            constexpr uint32_t NOT_UNIFORM = 0xffffffffu;
            uint32_t u_obj = NOT_UNIFORM, u_lane = 0u; // wave-uniform
            if constexpr (UNIFORM_SHADE) {
                const unsigned long long hit_mask = ballot(hit);
                if (hit_mask != 0ull) {
                    u_lane = (uint32_t)__builtin_ctzll(hit_mask);
                    const uint32_t named = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane(hidx, (int)u_lane));
                    if (ballot(hit && hidx != (int)named) == 0ull) u_obj = named;
                }
            }
            if (hit) {
                point = vadd(ro, vmul(rd, best)); // Ray::position vec.rs:207-209
                eyev = vneg(rd);
                if (UNIFORM_SHADE && u_obj != NOT_UNIFORM) { // (wave-uniform) the kind, then plane_n or the inverse's rows and nt: scalar loads
                    const ConstShade Su = (ConstShade)(T.shade + u_obj);
                    const ConstDoubles mu = (ConstDoubles)T.isect[u_obj].m;
                    const uint32_t ukind = (CARRY_KIND && use_bins) ? (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_amdgcn_readlane(hroot, (int)u_lane)) >> 1 : Su->kind;
                    normal = shape_normal_of<trace_wave_normalize(4, SRC, REFL, PROBE, ALT, MULTI), trace_short_chains(SC_NORMAL, SRC, REFL, ONE, MULTI)>(ukind, Su, mu, point);
                } else // (a mixed tile, and every kernel without the path: per lane)
                if constexpr (CARRY_KIND || trace_short_chains(SC_NORMAL, SRC, REFL, ONE, MULTI)) {
                    const uint32_t nkind = (CARRY_KIND && use_bins) ? (uint32_t)hroot >> 1 : S->kind; // (use_bins is wave-uniform)
                    normal = shape_normal_of<trace_wave_normalize(4, SRC, REFL, PROBE, ALT, MULTI), trace_short_chains(SC_NORMAL, SRC, REFL, ONE, MULTI)>(nkind, S, m_obj, point);
                } else {
                    normal = shape_normal<trace_wave_normalize(4, SRC, REFL, PROBE, ALT, MULTI)>(S, m_obj, point);
                }
                inside = vdot(normal, eyev) < 0.0;
                if (inside) normal = vneg(normal);
                over = vadd(point, vmul(normal, RTC_EPSILON));
                under = vsub(point, vmul(normal, RTC_EPSILON));
                reflectv = vreflect(rd, normal);
                m_kr = S->reflective;
                m_tr = S->transparency;
                shadow_ray<trace_wave_normalize(2, SRC, REFL, PROBE, ALT, MULTI)>(lightp, over, hit, sdir, sdist);
            }

            // ---- compute_refractive (shape.rs:115-141), open-set form, transparent hits only ----
            if constexpr (REFR) {
                const bool need = hit && m_tr != 0.0;
                bool any_need;
                if constexpr (SRC == SRC_LDSN) any_need = __syncthreads_or(need ? 1 : 0) != 0;
                else any_need = ballot(need) != 0ull;
                if (any_need) {
                    // `containers` is keyed by world_id (shape.rs:127): every entry that precedes the hit
                    // entry in list order toggles its id. An id is present iff an odd number of its
                    // entries precede the hit; the element standing for it is the LAST of them (the one
                    // that pushed it back in); containers.last = the present id whose such entry is
                    // latest in list order (max (t, shape index)). Shapes are walked grouped by id
                    // (idtab: stable order of world_id, wave-uniform scalar loads), one class
                    // accumulator at a time. Unique ids (World::add_shape's own numbering up to 255
                    // shapes): a class is one shape and this is the open set of SURVEY.md App. A.6;
                    // shared ids (the reference's u8 counter wraps, shape.rs:287,661-667): still the
                    // literal walk. Never culled: entries with t < 0 count.
                    bool have_all = false, have_oth = false;
                    double key_all = 0., key_oth = 0.;
                    int idx_all = -1, idx_oth = -1;
                    const uint32_t hid = S->world_id;
                    uint32_t cnt_h = 0, cnt = 0;
                    double last_t = 0.;
                    int last_s = -1;
                    auto fold = [&](uint32_t id) { // class `id` is complete
                        if (id == hid) cnt_h = cnt;
                        if (cnt & 1u) {
                            if (!have_all || last_t > key_all || (last_t == key_all && last_s > idx_all)) { have_all = true; key_all = last_t; idx_all = last_s; }
                            if (id != hid && (!have_oth || last_t > key_oth || (last_t == key_oth && last_s > idx_oth))) { have_oth = true; key_oth = last_t; idx_oth = last_s; }
                        }
                        cnt = 0;
                        last_s = -1;
                    };
                    const uint32_t nobj = P.n;
                    uint32_t cur_id = 0;
                    for (uint32_t k = 0; k < nobj; ++k) {
                        const DevIdEntry e = T.idtab[k];
                        if (k > 0 && e.id != cur_id) fold(cur_id);
                        cur_id = e.id;
                        if (need) {
                            const int j = (int)e.index;
                            const double *m = T.isect[j].m;
                            const V3 o = xpoint(m, ro);
                            const V3 d = xvector(m, rd);
                            double t0 = 0., t1 = 0.;
                            const int cnt_e = shape_entries<false>(T.kind[j], o, d, 0., t0, t1);
                            bool p1, p2;
                            if (j == hidx) { p1 = (hroot == 1); p2 = false; }
                            else {
                                p1 = t0 < best || (t0 == best && j < hidx);
                                p2 = t1 < best || (t1 == best && j < hidx);
                            }
                            p1 = p1 && cnt_e >= 1;
                            p2 = p2 && cnt_e == 2;
                            if (p1 || p2) {
                                const double te = p2 ? t1 : t0; // this shape's last entry before the hit
                                cnt += (p1 ? 1u : 0u) + (p2 ? 1u : 0u);
                                if (last_s < 0 || te > last_t || (te == last_t && j >= last_s)) { last_t = te; last_s = j; }
                            }
                        }
                    }
                    if (nobj) fold(cur_id);
                    if (need) {
                        n1 = have_all ? T.shade[idx_all].refractive_index : 1.0;
                        if (cnt_h & 1u) n2 = have_oth ? T.shade[idx_oth].refractive_index : 1.0; // the hit entry removes its id
                        else n2 = S->refractive_index;                                            // the hit entry pushes its id
                    }
                }
            }

            // ---- is_shadowed (shape.rs:712-727): any-hit with early exit ----------------------
            bool sh_pending = hit, shadowed = false;
            c_shadow += popc64(ballot(hit));
            Bundle Bs{};
            Bs.off = true;
            // Light-space shadow lists, small worlds (one-level cull): the cells' lists are a handful of objects, so they
            // are the candidates themselves — no shadow bundle, no bound tests. Every lane walks the list of ITS OWN cell
            // (per-lane loads of the entries and of their prefilter records, LANE_LIST_BATCH at a time); only the exact
            // test of a survivor is wave-level, its record fetched by uniform index.
            bool listed = false;
            if constexpr (SRC == SRC_CULL) {
                // trace_short_chains' SC_SHADOW_ARGS: what this stage reads of the kernel arguments as one group of loads under
                // one wait, held in SGPRs, instead of one load and one wait per term of the condition below and per loop
                // bound (the pointers are still tested before anything is read through them)
                struct ShadowArgs {
                    const uint32_t *light_cnt, *light_list;
                    uint32_t light_cap, n_unb;
                    double light_reach, pre_limit;
                };
                auto shadow_args = [&]() -> decltype(auto) {
                    if constexpr (trace_short_chains(SC_SHADOW_ARGS, SRC, REFL, ONE, MULTI)) {
                        const auto &Pa = KP(P_arg);
                        unsigned long long p0 = (unsigned long long)Pa.light_cnt, p1 = (unsigned long long)Pa.light_list;
                        unsigned long long d0 = __builtin_bit_cast(unsigned long long, Pa.light_reach), d1 = __builtin_bit_cast(unsigned long long, Pa.pre_limit);
                        uint32_t u0 = Pa.light_cap, u1 = Pa.n_unb;
                        asm volatile("" : "+s"(p0), "+s"(p1), "+s"(u0), "+s"(u1), "+s"(d0), "+s"(d1)); // all of them, here
                        typedef const __attribute__((address_space(1))) uint32_t *GlobalWords; // (global memory, as every kernel argument's)
                        return ShadowArgs{(const uint32_t *)(GlobalWords)p0, (const uint32_t *)(GlobalWords)p1, u0, u1, __builtin_bit_cast(double, d0), __builtin_bit_cast(double, d1)};
                    } else {
                        return (KP(P_arg)); // the parameter block itself: each field loaded where it is read
                    }
                };
                const auto &Pl = shadow_args();
                constexpr bool CELL_TOGETHER = trace_short_chains(SC_CELL, SRC, REFL, ONE, MULTI);
                // (light_cap == RTC_LIGHT_LIST_CAP_SMALL: a one-level World's own lists; a larger World only gets here with the
                // one-level cull FORCED, RTC_SRC=3 — its 128-entry lists feed a filter step — and takes the bundle walk)
                if (Pl.light_cnt != nullptr && Pl.light_cap == RTC_LIGHT_LIST_CAP_SMALL && ballot(hit) != 0ull && ballot(hit && !(sdist <= Pl.light_reach)) == 0ull) {
                    constexpr uint32_t LB = LANE_LIST_BATCH;
                    static_assert((LB == 1u || LB == 2u || LB == 4u) && RTC_LIGHT_LIST_CAP_SMALL % LB == 0u, "a batch of entries is one aligned vector load");
                    const uint32_t cid = hit ? light_cell(vneg(sdir)) : 0u;
                    const uint32_t ccnt = hit ? Pl.light_cnt[cid] : 0u; // every lane its own cell's counter: one round trip
                    // SC_CELL: the first batch of the lane's own list with the counter — both addresses come from cid alone, and
                    // a cell's CAP slots exist whatever its count; the batch is masked by the count where it is used, as every batch
                    uint32_t ent0[LB] = {};
                    if constexpr (CELL_TOGETHER) {
                        const uint32_t *l0 = Pl.light_list + (size_t)cid * RTC_LIGHT_LIST_CAP_SMALL;
                        if (hit) {
                            if constexpr (LB == 4u) { const uint4 v = *reinterpret_cast<const uint4 *>(l0); ent0[0] = v.x; ent0[1] = v.y; ent0[2] = v.z; ent0[3] = v.w; }
                            else if constexpr (LB == 2u) { const uint2 v = *reinterpret_cast<const uint2 *>(l0); ent0[0] = v.x; ent0[1] = v.y; }
                            else ent0[0] = l0[0];
                        }
                    }
                    listed = ballot(ccnt > Pl.light_cap) == 0ull;      // a cell whose list overflowed is incomplete: fall back
                    if (listed) {
                        for (uint32_t k = 0; k < Pl.n_unb && ballot(sh_pending) != 0ull; ++k) { // unbounded objects: never listed
                            if (sh_pending && occludes_world<BARE_SHADOW>(T.kind_s[k], T.isect_s[k].m, over, sdir, sdist)) { shadowed = true; sh_pending = false; }
                        }
                        // pre-inflated prefilter records hold while every origin is within their limit (DevPre)
                        bool pre_ok;
                        double sdd;
                        {
#pragma clang fp contract(fast)
                            pre_ok = ballot(hit && !(fabs(over.x) + fabs(over.y) + fabs(over.z) <= Pl.pre_limit)) == 0ull;
                            sdd = sdir.x * sdir.x + sdir.y * sdir.y + sdir.z * sdir.z;
                        }
                        // Why the shadow bit is what the union walk over all the wave's cells gave: it is an any-hit; a cell's
                        // list is conservative for EVERY segment of that cell (k_light_cells' cones), so an object that is not on
                        // a lane's own list cannot occlude that lane, and the prefilter — the same conservative function on the
                        // same operands — only drops objects the exact test would miss. Restricting the unchanged exact test of
                        // object j to the lanes whose own list names j and whose prefilter keeps it therefore drops only tests
                        // that cannot hit. A lane's list holds each object once: no "done" set, no limit on the number of cells.
                        const uint32_t *mylist = Pl.light_list + (size_t)cid * RTC_LIGHT_LIST_CAP_SMALL;
                        for (uint32_t k0 = 0; ballot(sh_pending && k0 < ccnt) != 0ull; k0 += LB) {
                            uint32_t ent[LB]; // (all lanes load: k0 + LB <= the cap, no branch around the loads; entries past the counter are masked)
                            if (CELL_TOGETHER && k0 == 0u) { // (wave-uniform) the batch that came with the counter
#pragma unroll
                                for (uint32_t b = 0; b < LB; ++b) ent[b] = ent0[b];
                            } else
                            if constexpr (LB == 4u) { const uint4 v = *reinterpret_cast<const uint4 *>(mylist + k0); ent[0] = v.x; ent[1] = v.y; ent[2] = v.z; ent[3] = v.w; }
                            else if constexpr (LB == 2u) { const uint2 v = *reinterpret_cast<const uint2 *>(mylist + k0); ent[0] = v.x; ent[1] = v.y; }
                            else ent[0] = mylist[k0];
                            bool todo[LB];
#pragma unroll
                            for (uint32_t b = 0; b < LB; ++b) {
                                todo[b] = sh_pending && k0 + b < ccnt;
                                if (!todo[b]) ent[b] = 0u;
                            }
                            if (pre_ok) {
                                DevPre q[LB]; // the records of the batch are requested together, ahead of the tests
#pragma unroll
                                for (uint32_t b = 0; b < LB; ++b) q[b] = T.pre[ent[b]];
#pragma unroll
                                for (uint32_t b = 0; b < LB; ++b) todo[b] = todo[b] && ray_touches_pre(over, sdir, sdd, q[b]);
                            } else {
#pragma unroll
                                for (uint32_t b = 0; b < LB; ++b) todo[b] = todo[b] && ray_touches(over, sdir, T.bound[ent[b]]);
                            }
                            // survivors: one object at a time, for every lane of the batch that still has it to test
                            for (;;) {
                                bool any = false;
                                uint32_t mine = 0u;
#pragma unroll
                                for (uint32_t b = LB; b-- > 0u;) {
                                    if (todo[b]) { any = true; mine = ent[b]; }
                                }
                                const unsigned long long m = ballot(any && sh_pending);
                                if (m == 0ull) break;
                                const uint32_t j = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)__builtin_ctzll(m));
                                const DevIsect rec = T.isect[j]; // record and kind requested together
                                const uint32_t kd = T.kind[j];
                                bool sel = false;
#pragma unroll
                                for (uint32_t b = 0; b < LB; ++b) {
                                    if (todo[b] && ent[b] == j) { sel = true; todo[b] = false; }
                                }
                                if (sel && sh_pending && occludes_world<BARE_SHADOW>(kd, rec.m, over, sdir, sdist)) { shadowed = true; sh_pending = false; }
                            }
                        }
                    }
                }
            }
            if constexpr (IS_CULL(SRC)) {
                // the segment over_point -> light, walked from the light: apex = light (shared)
                if (ballot(hit) != 0ull && !listed) Bs = make_bundle<true, true>(hit, lightp, lightp, vneg(sdir), sdist);
            }
            // Light-space shadow lists (two-level worlds): instead of walking every group sphere, filter the lists of the
            // direction cells (around the light) this wave's segments fall in with the wave's own shadow bundle.
            if constexpr (SRC == SRC_CULL2) {
                const auto &Pl = KP(P_arg);
                if (Pl.light_cnt != nullptr && !Bs.off && Bs.tmax <= Pl.light_reach && ballot(hit) != 0ull) {
                    const uint32_t cid = hit ? light_cell(vneg(sdir)) : 0u;
                    const uint32_t ccnt = hit ? Pl.light_cnt[cid] : 0u;          // every lane its own cell's counter: one round trip
                    listed = ballot(hit && ccnt > Pl.light_cap) == 0ull;       // a cell whose list overflowed is incomplete: walk instead
                    if (listed) {
                        for (uint32_t k = 0; k < Pl.n_unb && ballot(sh_pending) != 0ull; ++k) { // unbounded objects: never listed
                            if (sh_pending && occludes_world<BARE_SHADOW>(T.kind_s[k], T.isect_s[k].m, over, sdir, sdist)) { shadowed = true; sh_pending = false; }
                        }
                        bool pre_ok; // pre-inflated prefilter records hold while every origin is within their limit (DevPre)
                        double sdd;
                        {
#pragma clang fp contract(fast)
                            pre_ok = ballot(hit && !(fabs(over.x) + fabs(over.y) + fabs(over.z) <= Pl.pre_limit)) == 0ull;
                            sdd = sdir.x * sdir.x + sdir.y * sdir.y + sdir.z * sdir.z;
                        }
                        for (unsigned long long todo = ballot(hit); todo && ballot(sh_pending) != 0ull;) {
                            const int cl = (int)__builtin_ctzll(todo);
                            const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cid, cl);
                            const uint32_t nl = (uint32_t)__builtin_amdgcn_readlane((int)ccnt, cl);
                            todo &= ~ballot(hit && cid == c);
                            const uint32_t *ll = Pl.light_list + (size_t)c * Pl.light_cap;
                            for (uint32_t base = 0; base < nl && ballot(sh_pending) != 0ull; base += 64u) {
                                const uint32_t e = base + lane;
                                uint32_t idx = 0u;
                                bool cand = false;
                                if (e < nl) { idx = ll[e]; cand = bundle_touches(Bs, T.bound[idx]); }
                                unsigned long long mask = ballot(cand);
                                while (mask && ballot(sh_pending) != 0ull) { // survivors two at a time (PRE_BATCH, as for_each_object)
                                    const uint32_t j0 = (uint32_t)__builtin_amdgcn_readlane((int)idx, (int)__builtin_ctzll(mask));
                                    mask &= mask - 1ull;
                                    uint32_t j1 = j0;
                                    const bool two = mask != 0ull;
                                    if (two) { j1 = (uint32_t)__builtin_amdgcn_readlane((int)idx, (int)__builtin_ctzll(mask)); mask &= mask - 1ull; }
                                    unsigned long long b0, b1;
                                    if (pre_ok) {
                                        const DevPre q0 = T.pre[j0], q1 = T.pre[j1];
                                        const bool t0 = ray_touches_pre(over, sdir, sdd, q0), t1 = ray_touches_pre(over, sdir, sdd, q1);
                                        b0 = ballot(sh_pending & t0);
                                        b1 = two ? ballot(sh_pending & t1) : 0ull;
                                    } else {
                                        b0 = ballot(sh_pending && ray_touches(over, sdir, T.bound[j0]));
                                        b1 = two ? ballot(sh_pending && ray_touches(over, sdir, T.bound[j1])) : 0ull;
                                    }
                                    if (b0 != 0ull) {
                                        const DevIsect rec = T.isect[j0];
                                        const uint32_t kd = T.kind[j0];
                                        if (sh_pending && occludes_world<BARE_SHADOW>(kd, rec.m, over, sdir, sdist)) { shadowed = true; sh_pending = false; }
                                    }
                                    if (b1 != 0ull && ballot(sh_pending) != 0ull) {
                                        const DevIsect rec = T.isect[j1];
                                        const uint32_t kd = T.kind[j1];
                                        if (sh_pending && occludes_world<BARE_SHADOW>(kd, rec.m, over, sdir, sdist)) { shadowed = true; sh_pending = false; }
                                    }
                                }
                            }
                        }
                    }
                }
            }
            if (!listed)
            for_each_object<SRC, SHADOW_LANE_FILTER>(P, T, L, sh_pending, Bs, AnyHitT<BARE_SHADOW>{sh_pending, over, sdir, sdist, shadowed}, over, sdir);

            // keep the material / pattern loads of the lighting stage BELOW the shadow loop: hoisted
            // above it they stay live through the loop and cost a wave per SIMD in occupancy
            asm volatile("" ::: "memory");
            if constexpr (PROBE) if (first && in_range && P.hits) {
                rtc_hit *H = reinterpret_cast<rtc_hit *>(P.hits) + ray_index;
                H->hit_index = hit ? hidx : -1;
                H->inside = inside ? 1u : 0u;
                H->shadowed = shadowed ? 1u : 0u;
                H->_pad = 0u;
                H->t = hit ? best : 0.;
                H->point[0] = point.x; H->point[1] = point.y; H->point[2] = point.z;
                H->over_point[0] = over.x; H->over_point[1] = over.y; H->over_point[2] = over.z;
                H->under_point[0] = under.x; H->under_point[1] = under.y; H->under_point[2] = under.z;
                H->eyev[0] = eyev.x; H->eyev[1] = eyev.y; H->eyev[2] = eyev.z;
                H->normal[0] = normal.x; H->normal[1] = normal.y; H->normal[2] = normal.z;
                H->reflectv[0] = reflectv.x; H->reflectv[1] = reflectv.y; H->reflectv[2] = reflectv.z;
                H->n1 = n1; H->n2 = n2;
            }

            // ---- several lights (MULTI): surface = lighting(L[0]) + lighting(L[1]) + ..., in light order ----
            // The first light's term (its shadow bit comes from the passes above, lists included), then per further light
            // the shadow ray's set-up (shape.rs:717-719), the any-hit pass and lighting(). The further lights have no
            // light-space lists: their segments take the bundle walk, apex = that light. Kept out of the divergent
            // branch below: the walks are wave-level code (ballots, DPP reductions).
            V3 surface_all = mk(0., 0., 0.);
            if constexpr (MULTI) {
                static_assert(SRC == SRC_SMEM || IS_CULL(SRC), "multi-light launches take SRC_SMEM, SRC_CULL or SRC_CULL2");
                const auto &X = first_of(xl_arg...); // DevExtraLights (kernel arguments) or DevLightTable (HBM): further_light_*
                if (hit) surface_all = lighting(KP(P_arg), S, m_obj, over, eyev, normal, sdir, shadowed);
                const uint32_t n_extra = further_light_count(X);
                for (uint32_t li = 0; li < n_extra; ++li) {
                    const V3 lp = further_light_position(X, li);
                    V3 ldir = mk(0, 0, 0);
                    double ldist = 0.;
                    shadow_ray(lp, over, hit, ldir, ldist);
                    bool l_pending = hit, l_shadowed = false;
                    c_shadow += popc64(ballot(hit));
                    Bundle Bl{};
                    Bl.off = true;
                    if constexpr (IS_CULL(SRC)) {
                        if (ballot(hit) != 0ull) Bl = make_bundle<true, true>(hit, lp, lp, vneg(ldir), ldist);
                    }
                    for_each_object<SRC, SHADOW_LANE_FILTER>(P, T, L, l_pending, Bl, AnyHit{l_pending, over, ldir, ldist, l_shadowed}, over, ldir);
                    asm volatile("" ::: "memory"); // as above: the material loads stay below the walk
                    if (hit) {
                        const LightInt I = further_light_intensity(X, li);
                        surface_all = vadd(surface_all, lighting(I, S, m_obj, over, eyev, normal, ldir, l_shadowed));
                    }
                }
            }

            // ---- shade_hit (shape.rs:685-700) ------------------------------------------------
            V3 val = mk(0., 0., 0.); // value returned by the color_at call that just finished
            bool have_val = false;
            bool l_refl = false, l_refr = false; // this lane launched a reflection / refraction ray
            if (tracing && !hit) { // background_color: BLACK shape.rs:652-653
                have_val = true;
            } else if (hit) {
                V3 surface;
                if constexpr (MULTI) surface = surface_all;
                else if (UNIFORM_SHADE && u_obj != NOT_UNIFORM) { // (wave-uniform) the material's scalars and the pattern record: scalar loads
                    // (the index as operand of an empty statement: the loads at the addresses made from it start here, below
                    // the shadow pass, as the fence above keeps the per-lane ones — nothing of the normal's records is held across it)
                    uint32_t u_here = u_obj;
                    asm volatile("" : "+s"(u_here));
                    const ConstShade Su = (ConstShade)(T.shade + u_here);
                    const ConstDoubles mu = (ConstDoubles)T.isect[u_here].m;
                    surface = lighting<BARE_RING>(KP(P_arg), Su, mu, over, eyev, normal, sdir, shadowed);
                } else surface = lighting<BARE_RING>(KP(P_arg), S, m_obj, over, eyev, normal, sdir, shadowed);
                bool want_refl = false, want_refr = false;
                V3 fr_o = mk(0, 0, 0), fr_d = mk(0, 0, 0);
                if constexpr (REFL) want_refl = (rem != 0) && !(m_kr <= 0.); // reflected_color shape.rs:730 (NaN: cast)
                if constexpr (REFR) {
                    if (rem != 0 && m_tr != 0.0) { // refracted_color shape.rs:751-766
                        const double n_ratio = n1 / n2;
                        const double cos_i = vdot(eyev, normal);
                        const double sin2_t = (n_ratio * n_ratio) * (1.0 - cos_i * cos_i);
                        if (!(sin2_t > 1.0)) {
                            const double cos_t = sqrt(1.0 - sin2_t);
                            fr_d = vsub(vmul(normal, n_ratio * cos_i - cos_t), vmul(eyev, n_ratio));
                            fr_o = under;
                            want_refr = true;
                        }
                    }
                }
                bool schlick = false;
                double R = 0.;
                if constexpr (REFR) {
                    if (m_kr > 0.0 && m_tr > 0.0) { schlick = true; R = reflectance(eyev, normal, n1, n2); }
                }
                if (!want_refl && !want_refr) {
                    val = combine(surface, mk(0., 0., 0.), mk(0., 0., 0.), schlick, R);
                    have_val = true;
                } else {
                    if constexpr (REFR) {
                        Frame &F = stack[sp];
                        F.surface = surface;
                        F.a = fr_o; F.rd = fr_d;
                        F.kr = m_kr; F.tr = m_tr; F.R = R;
                        F.rem = (uint8_t)rem;
                        F.state = want_refl ? 0 : 1;
                        F.schlick = schlick ? 1 : 0;
                        F.has_refr = want_refr ? (want_refl ? 1 : 2) : 0; // 2: refraction only, no reflected colour will arrive
                        ++sp;
                        if (want_refl) { ro = over; rd = reflectv; l_refl = true; } // Ray::new(over_point, reflectv) shape.rs:734
                        else { ro = fr_o; rd = fr_d; l_refr = true; }               // Ray::new(under_point, direction) shape.rs:764
                        rem = rem - 1;
                    } else if constexpr (REFL) { // reflection only: want_refl holds here
                        if constexpr (LDS_STACK) {
                            double *f = lstk + (uint32_t)sp * 4u * BLOCK;
                            f[0] = surface.x; f[BLOCK] = surface.y; f[2 * BLOCK] = surface.z; f[3 * BLOCK] = m_kr;
                        } else {
                            Frame &F = stack[sp];
                            F.surface = surface;
                            F.kr = m_kr;
                        }
                        ++sp;
                        ro = over; rd = reflectv; l_refl = true;                     // shape.rs:734
                        rem = rem - 1;
                    }
                }
            }
            first = false;

            // ---- return `val` to the callers (unwind) ------------------------------------------
            if (have_val) {
                bool relaunched = false;
                if constexpr (REFL && !REFR) {
                    while (sp > 0) { // surface + reflected + refracted(BLACK), innermost call first shape.rs:692-699
                        if constexpr (LDS_STACK) {
                            const double *f = lstk + (uint32_t)(sp - 1) * 4u * BLOCK;
                            val = combine(mk(f[0], f[BLOCK], f[2 * BLOCK]), vmul(val, f[3 * BLOCK]), mk(0., 0., 0.), false, 0.);
                        } else {
                            const Frame &F = stack[sp - 1];
                            val = combine(F.surface, vmul(val, F.kr), mk(0., 0., 0.), false, 0.);
                        }
                        --sp;
                    }
                }
                if constexpr (REFR) {
                    while (sp > 0) {
                        Frame &F = stack[sp - 1];
                        if (F.state == 0) {
                            const V3 reflected = vmul(val, F.kr); // c.mul_f64(reflectiveness) shape.rs:736
                            if (F.has_refr) { // now refracted_color's recursion shape.rs:764-765
                                F.state = 1;
                                ro = F.a; rd = F.rd;
                                F.a = reflected;     // the pending ray has left the frame: its slot keeps the reflected colour
                                rem = (int)F.rem - 1;
                                relaunched = true;
                                l_refr = true;
                                break;
                            }
                            val = combine(F.surface, reflected, mk(0., 0., 0.), F.schlick != 0, F.R);
                            --sp;
                        } else {
                            // a frame that never launched a reflection ray (state 1 from the start) holds the refraction
                            // ray's origin in `a`; its reflected colour is BLACK (reflected_color shape.rs:730-732)
                            const V3 reflected = F.has_refr == 2 ? mk(0., 0., 0.) : F.a;
                            const V3 refracted = vmul(val, F.tr); // shape.rs:765
                            val = combine(F.surface, reflected, refracted, F.schlick != 0, F.R);
                            --sp;
                        }
                    }
                }
                if constexpr (REFL) {
                    if (!relaunched) {
                        result = val;
                        tracing = false;
                    }
                }
            }
            if constexpr (REFL) {
                c_reflect += popc64(ballot(l_refl));
                c_refract += popc64(ballot(l_refr));
            } else {
                result = val; // BLACK for lanes that traced nothing or missed (val starts at 0)
            }
        }

        if constexpr (PROBE) {
            if (in_range) {
                double *o = KP(P_arg).out + (size_t)ray_index * 3;
                o[0] = result.x;
                o[1] = result.y;
                o[2] = result.z;
            }
        } else {
            // Between AA samples Color::average_over's running sums (color.rs:128-139: reds = ((0 + c0) + c1) + ...)
            // wait in the thread's part of the dynamic LDS block (the tile may be staged over the frame stack).
            if (!traced) result = mk(0., 0., 0.); // Canvas::new BLACK canvas.rs:37-41
            if constexpr (LENS) { // Color::average_over color.rs:128-139: sums from 0.0 in sample order, one division each
                lens_sum = vadd(lens_sum, result);
                if (s + 1u == nsamples) {
                    const double l = (double)nsamples;
                    result = mk(lens_sum.x / l, lens_sum.y / l, lens_sum.z / l);
                }
            }
            if (aa) {
                // aa_store[12..14] hold Color::average_over's running sums (reds = ((0 + c0) + c1) + ..., color.rs:128-139)
                // while a lane still collects samples, and the pixel's final colour afterwards
                const bool collecting = s < 4u || lane_resample;
                V3 acc = (s == 0u) ? mk(0., 0., 0.) : mk(aa_store[12], aa_store[13], aa_store[14]);
                if (collecting) acc = vadd(acc, result);
                if (s < 4u) { aa_store[s * 3u] = result.x; aa_store[s * 3u + 1u] = result.y; aa_store[s * 3u + 2u] = result.z; }
                if (s == 3u) {
                    // average = Color::average_over(&sample); resample if any |c - average| > 0.01 (camera.rs:106-111,
                    // Color::distance_from color.rs:122-126: sqrt of the sum of squares)
                    const V3 mean = mk(acc.x / 4., acc.y / 4., acc.z / 4.);
                    bool trip = false;
                    for (uint32_t i = 0; i < 4u; ++i) {
                        const double dr = aa_store[i * 3u] - mean.x, dg = aa_store[i * 3u + 1u] - mean.y, db = aa_store[i * 3u + 2u] - mean.z;
                        trip = trip || (sqrt(dr * dr + dg * dg + db * db) > 0.01);
                    }
                    trip = trip && traced;
                    c_resample += popc64(ballot(trip));
                    const auto &Pa = KP(P_arg);
                    lane_resample = trip && Pa.resample_n != 0u;
                    bool more;
                    if constexpr (SRC == SRC_LDSN) more = __syncthreads_or(lane_resample ? 1 : 0) != 0; // same pass count for every wave
                    else more = ballot(lane_resample) != 0ull;
                    if (more) nsamples = 4u + Pa.resample_n;
                    if (!lane_resample) acc = mean; // final: the mean of the four
                }
                if (s >= 4u && s + 1u == nsamples && lane_resample) { // Color::average_over(&samples) over 4 + n
                    const double l = (double)nsamples;
                    acc = mk(acc.x / l, acc.y / l, acc.z / l);
                }
                result = acc;
                aa_store[12] = acc.x; aa_store[13] = acc.y; aa_store[14] = acc.z;
            }
        }
    } // samples

    // ---- the output stage: once per tile, after its last sample; a tile proven black arrives with `result` still BLACK ----
    if constexpr (!PROBE) {
        // The workgroup's (TILE_W x 8)-pixel tile is staged in LDS (row-major, exactly the canvas layout of
        // the tile) and written out by the whole workgroup: with TILE_W = 16 each tile row is 384 contiguous
        // bytes of the f64 canvas (three full 128-byte lines) and 48 contiguous bytes of the 8-bit frame,
        // stored 16 bytes per lane. Direct per-pixel stores (3 x 8 B at a 24 B stride, 3 single
        // bytes) cost 1.6x the algorithmic bytes in HBM write traffic (rocprofv3 WRITE_SIZE).
        // (the lane number through an opaque copy: the slot arithmetic is done here, per tile, and not hoisted in front of the
        // tile loop, from where it would be carried — spilled — through the whole trace)
        uint32_t olane = lane;
        asm volatile("" : "+v"(olane));
        const uint32_t tx = wave * 8u + (olane & 7u), ty = olane >> 3; // position inside the tile
        double *slot = stage_f64 + (ty * TILE_W + tx) * 3u;
        slot[0] = result.x;
        slot[1] = result.y;
        slot[2] = result.z;
        const auto &Po = KP(P_arg); // output view
        const bool want8 = !WHOLE && Po.out8 != nullptr;
        if (want8) {
            unsigned char *q = stage_u8 + (ty * TILE_W + tx) * 3u;
            if constexpr (RGBA) { // Canvas::to_imgbuf's channels (rtc_gamma.h)
                const DevGamma *gt = Po.gamma;
                q[0] = gamma_byte(gt, result.x);
                q[1] = gamma_byte(gt, result.y);
                q[2] = gamma_byte(gt, result.z);
            } else {
                q[0] = scale255(result.x);
                q[1] = scale255(result.y);
                q[2] = scale255(result.z);
            }
        }
        // Canvas stores are non-temporal (written once, never read by the kernel): north star -2.3 %, C3 -4.2 %,
        // C5 -1.5 % (profiles/r02_exp_nt_stores.log).
        if constexpr (WAVE_OUTPUT) {
        // Each wave stores its own 8x8 part of the tile (no workgroup barrier: a wave that is
        // done retires without waiting for the slowest of its three neighbours). Its LDS
        // region is written and read by this wave only; LDS operations of one wave execute
        // in order, the fences only stop the compiler from reordering them.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t px0 = bx * TILE_W + wave * 8u, py0 = Po.y0 + by * (WHOLE ? 1u : Po.band_stride) * 8u,
                       orow0 = (WHOLE ? 0u : view * Po.view_rows) + by * 8u; // first image row / first output row of the tile
        // (WHOLE: eight whole rows of eight pixels, 16-byte aligned, and an f64 canvas to store them in)
        const uint32_t cols = WHOLE ? 8u : (px0 >= Po.W) ? 0u : ((Po.W - px0 < 8u) ? (Po.W - px0) : 8u); // valid pixels per row
        const uint32_t rows = WHOLE ? 8u : (Po.y1 - py0 < 8u) ? (Po.y1 - py0) : 8u;                       // valid tile rows
        const size_t row_bytes = (size_t)Po.W * 24u;
        const double *src = stage_f64 + wave * 24u;
        // a row of the wave's part is 192 contiguous bytes of the canvas: 12 pieces of 16 bytes
        const bool wide = WHOLE || (cols == 8u && (row_bytes % 16u) == 0 && ((size_t)Po.out % 16u) == 0);
        if (!WHOLE && Po.out == nullptr) { // 8-bit frame only (rtc_render_rgb8): nothing of the f64 canvas leaves the chip
        } else if (wide) {
            typedef double __attribute__((ext_vector_type(2))) d2;
            for (uint32_t c = lane; c < rows * 12u; c += 64u) {
                const uint32_t r = c / 12u, k = c % 12u;
                const d2 v = *reinterpret_cast<const d2 *>(src + r * (TILE_W * 3u) + k * 2u);
                char *dst = reinterpret_cast<char *>(Po.out) + (size_t)(orow0 + r) * row_bytes + (size_t)px0 * 24u + k * 16u;
                __builtin_nontemporal_store(v, reinterpret_cast<d2 *>(dst));
            }
        } else {
            for (uint32_t c = lane; c < rows * cols * 3u; c += 64u) {
                const uint32_t r = c / (cols * 3u), k = c % (cols * 3u);
                Po.out[((size_t)(orow0 + r) * Po.W + px0) * 3u + k] = src[r * (TILE_W * 3u) + k];
            }
        }
        if constexpr (RGBA) {
            if (want8) store_rgba<8u, TILE_W * 3u, 64u>(stage_u8 + wave * 24u, Po.out8, Po.W, orow0, px0, rows, cols, lane);
        } else if (want8) {
            const size_t row8 = (size_t)Po.W * 3u;
            const unsigned char *src8 = stage_u8 + wave * 24u;
            // 24 contiguous bytes per row: 3 pieces of 8 bytes
            const bool wide8 = cols == 8u && (row8 % 8u) == 0 && ((size_t)Po.out8 % 8u) == 0;
            if (wide8) {
                typedef unsigned __attribute__((ext_vector_type(2))) u2;
                for (uint32_t c = lane; c < rows * 3u; c += 64u) {
                    const uint32_t r = c / 3u, k = c % 3u;
                    const u2 v = *reinterpret_cast<const u2 *>(src8 + r * (TILE_W * 3u) + k * 8u);
                    __builtin_nontemporal_store(v, reinterpret_cast<u2 *>(Po.out8 + (size_t)(orow0 + r) * row8 + (size_t)px0 * 3u + k * 8u));
                }
            } else {
                for (uint32_t c = lane; c < rows * cols * 3u; c += 64u) {
                    const uint32_t r = c / (cols * 3u), k = c % (cols * 3u);
                    Po.out8[((size_t)(orow0 + r) * Po.W + px0) * 3u + k] = src8[r * (TILE_W * 3u) + k];
                }
            }
        }
        } else {
        __syncthreads();
        const uint32_t px0 = bx * TILE_W, py0 = Po.y0 + by * (WHOLE ? 1u : Po.band_stride) * 8u,
                       orow0 = (WHOLE ? 0u : view * Po.view_rows) + by * 8u; // first image row / first output row of the tile
        // (WHOLE: eight whole tile rows, 16-byte aligned, and an f64 canvas to store them in)
        const uint32_t cols = WHOLE ? TILE_W : (Po.W - px0 < TILE_W) ? (Po.W - px0) : TILE_W;      // valid pixels per tile row
        const uint32_t rows = WHOLE ? 8u : (Po.y1 - py0 < 8u) ? (Po.y1 - py0) : 8u;      // valid tile rows
        // f64 canvas: 16-byte pieces when every tile row is whole and 16-byte aligned
        const size_t row_bytes = (size_t)Po.W * 24u;
        const bool wide = WHOLE || (cols == TILE_W && (row_bytes % 16u) == 0 && ((size_t)Po.out % 16u) == 0);
        if (!WHOLE && Po.out == nullptr) { // 8-bit frame only (rtc_render_rgb8)
        } else if (wide) {
            typedef double __attribute__((ext_vector_type(2))) d2;
            for (uint32_t c = threadIdx.x; c < rows * (TILE_W * 3u / 2u); c += BLOCK) {
                const uint32_t r = c / (TILE_W * 3u / 2u), k = c % (TILE_W * 3u / 2u);
                const d2 v = *reinterpret_cast<const d2 *>(stage_f64 + r * (TILE_W * 3u) + k * 2u);
                char *dst = reinterpret_cast<char *>(Po.out) + (size_t)(orow0 + r) * row_bytes + (size_t)px0 * 24u + k * 16u;
                __builtin_nontemporal_store(v, reinterpret_cast<d2 *>(dst));
            }
        } else {
            for (uint32_t c = threadIdx.x; c < rows * cols * 3u; c += BLOCK) {
                const uint32_t r = c / (cols * 3u), k = c % (cols * 3u);
                Po.out[((size_t)(orow0 + r) * Po.W + px0) * 3u + k] = stage_f64[r * (TILE_W * 3u) + k];
            }
        }
        if constexpr (RGBA) {
            if (want8) store_rgba<TILE_W, TILE_W * 3u, BLOCK>(stage_u8, Po.out8, Po.W, orow0, px0, rows, cols, threadIdx.x);
        } else if (want8) {
            const size_t row8 = (size_t)Po.W * 3u;
            // a tile row is 24 bytes per wave: 16-byte pieces for an even number of waves, 8-byte pieces for one
            constexpr uint32_t PIECE = (TILE_W * 3u) % 16u == 0 ? 16u : 8u;
            const bool wide8 = cols == TILE_W && (row8 % PIECE) == 0 && ((size_t)Po.out8 % PIECE) == 0;
            if (wide8) {
                typedef unsigned __attribute__((ext_vector_type(PIECE / 4u))) piece_t;
                for (uint32_t c = threadIdx.x; c < rows * (TILE_W * 3u / PIECE); c += BLOCK) {
                    const uint32_t r = c / (TILE_W * 3u / PIECE), k = c % (TILE_W * 3u / PIECE);
                    const piece_t v = *reinterpret_cast<const piece_t *>(stage_u8 + r * (TILE_W * 3u) + k * PIECE);
                    __builtin_nontemporal_store(v, reinterpret_cast<piece_t *>(Po.out8 + (size_t)(orow0 + r) * row8 + (size_t)px0 * 3u + k * PIECE));
                }
            } else {
                for (uint32_t c = threadIdx.x; c < rows * cols * 3u; c += BLOCK) {
                    const uint32_t r = c / (cols * 3u), k = c % (cols * 3u);
                    Po.out8[((size_t)(orow0 + r) * Po.W + px0) * 3u + k] = stage_u8[r * (TILE_W * 3u) + k];
                }
            }
        }
        }
    }

    if (rep + 1u < reps) {
        // the next tile is staged over the same LDS: the workgroup's cooperative store must have read it (a wave's own LDS
        // operations are in order, so the per-wave output form needs nothing)
        if constexpr (!PROBE && !WAVE_OUTPUT) __syncthreads();
    }
    } // rep
    const auto &Pc = KP(P_arg);
    if (Pc.counters) {
        if (lane == 0) { // (rtc_stats::pixels is counted by the host, render_launch)
            unsigned long long *slot = Pc.counters + (size_t)((blockIdx.x * (BLOCK / 64u) + wave) % CNT_SLOTS) * CNT_N;
            if (c_primary) atomicAdd(slot + CNT_PRIMARY, (unsigned long long)c_primary);
            if (c_shadow) atomicAdd(slot + CNT_SHADOW, (unsigned long long)c_shadow);
            if (c_reflect) atomicAdd(slot + CNT_REFLECT, (unsigned long long)c_reflect);
            if (c_refract) atomicAdd(slot + CNT_REFRACT, (unsigned long long)c_refract);
            if (c_resample) atomicAdd(slot + CNT_RESAMPLE, (unsigned long long)c_resample);
            if (c_sky) atomicAdd(slot + CNT_SKY, (unsigned long long)c_sky);
        }
    }
}

// Per-render prologue: camera origin in each object's space and the sphere quadratic's `c`
// (shape.rs:363,366) — the part of every primary-ray test that does not depend on the pixel.
DEVI DevPrim prim_of(const double *m_obj, V3 origin) { // (file scope: never under a contraction pragma — parity arithmetic)
    const V3 o = xpoint(m_obj, origin);
    DevPrim r;
    r.ox = o.x;
    r.oy = o.y;
    r.oz = o.z;
    r.c = vdot(o, o) - 1.;
    return r;
}
__global__ void __launch_bounds__(256) k_prep_primary(const DevIsect *isect, DevPrim *prim, uint32_t n,
                                                            double v0, double v1, double v2, double v3, double v4,
                                                            double v5, double v6, double v7, double v8, double v9,
                                                            double v10, double v11) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const double vinv[12] = {v0, v1, v2, v3, v4, v5, v6, v7, v8, v9, v10, v11};
    prim[j] = prim_of(isect[j].m, xpoint(vinv, mk(0., 0., 0.)));
}

// Device arithmetic probe (rtc_device_arith).
__global__ void k_arith(uint32_t op, const double *a, const double *b, uint32_t n, double *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op == 5u || op == 6u) { // Vector::normalize of the triple (a[3t], a[3t+1], a[3t+2]): 5 = the shared-divisor form, 6 = three divisions
        if (i % 3u == 0u && i + 2u < n) {
            const V3 v = mk(a[i], a[i + 1], a[i + 2]);
            const V3 r3 = op == 5u ? vnormalize_shared<(RTC_BARE_SQRT & BS_BIN) != 0>(v) : vnormalize_plain(v); // (5: as primary_dir calls it)
            out[i] = r3.x; out[i + 1] = r3.y; out[i + 2] = r3.z;
        }
        return;
    }
    if (op == 8u) { // the same through vnormalize_wave, the flat k_trace kernels' form: thread t takes triple t, so a wave holds 64
        // consecutive triples and takes one form for all of them
        if (3ull * i + 2u < n) {
            double mag;
            const V3 r3 = vnormalize_wave(mk(a[3u * i], a[3u * i + 1u], a[3u * i + 2u]), mag);
            out[3u * i] = r3.x; out[3u * i + 1u] = r3.y; out[3u * i + 2u] = r3.z;
        }
        return;
    }
    double r;
    switch (op) {
    case 0: r = sqrt(a[i]); break;
    case 9: r = sqrt_wave(a[i]); break; // sqrt as the flat k_trace kernels call it: thread t takes element t, a wave holds 64 consecutive values
    case 1: r = a[i] / b[i]; break;
    case 2: r = pow(a[i], b[i]); break;
    case 3: r = floor(a[i]); break;
    case 7: r = rtc_even_f64(a[i]) ? 1.0 : 0.0; break; // the patterns' even test (rtc_parity.h)
    default: r = fmod(a[i], 2.0); break;
    }
    out[i] = r;
}

// ---- binned primary pass: per-view tile lists (DevTileBundle, rtc_device.h) ---------------------------------------
// Primary ray of pixel (px, py) of one camera: Camera::ray_for_pixel_offset(x, 0.5, y, 0.5) camera.rs:64-76, the
// expression k_trace evaluates.
template <bool BARE = false> DEVI V3 primary_dir(const DevCamera &C, V3 cam_origin, uint32_t px, uint32_t py, double xo = 0.5, double yo = 0.5) {
    const double xoffset = ((double)px + xo) * C.pixel_size;
    const double yoffset = ((double)py + yo) * C.pixel_size;
    const double world_x = C.half_width - xoffset;
    const double world_y = C.half_height - yoffset;
    const V3 pixel = xpoint(C.vinv, mk(world_x, world_y, -1.));
    // the shared-divisor form (bit-identical, and a cone does not even need that): the binning kernel's lanes normalise ten
    // corner rays each on one latency-bound chain — C3's pipelined frame -7 % (profiles/r03_exp_shared_normalize.log)
    return vnormalize_shared<BARE>(vsub(pixel, cam_origin)); // (BARE: RTC_BARE_SQRT's site 16, the binning kernel's cones only)
}

struct BinParams {
    DevCamera views[RTC_MAX_VIEWS];
    uint32_t nviews, W, H, n;
    uint32_t tiles_x, tiles_y, macros_x, macros_y; // tiles of 8x8 pixels, macro tiles of 8x8 tiles
    uint32_t packed;           // n <= 65 536: list entries carry the key (bin_entry)
    uint32_t row0, row_stride; // the launch renders tile rows row0, row0 + row_stride, ... only (one rank's bands): the others get no lists
};

DEVI Bundle bundle_of(const DevTileBundle &t, V3 apex) { // a stored cone as the Bundle bundle_touches takes (rho 0, no reach)
    Bundle B{};
    B.px = apex.x; B.py = apex.y; B.pz = apex.z;
    B.ax = (double)t.ax; B.ay = (double)t.ay; B.az = (double)t.az;
    B.cosT = (double)t.cosT; B.sinT = (double)t.sinT;
    B.rho = 0.; B.tmax = __builtin_inf(); B.spread = 0.;
    B.off = t.off != 0u;
    return B;
}

// f32 unit direction as make_bundle takes it from a lane's f64 direction
DEVI bool dir_f32(V3 d, float &fx, float &fy, float &fz) {
    const float x = (float)d.x, y = (float)d.y, z = (float)d.z;
    const float l2 = x * x + y * y + z * z;
    const float il = __builtin_amdgcn_rsqf(l2);
    fx = x * il; fy = y * il; fz = z * il;
    return finite3(d) && l2 > 1e-30f && l2 < 1e30f;
}

// The cone of the primary rays of the `cell` x `cell` pixel block at (x0, y0), clipped to the image, with make_bundle's
// arithmetic and margins but from five rays instead of all: the axis ray (a pixel near the block's centre) and the four
// corners. The angle between a ray through the image plane and a fixed axis is a quasi-convex function of the pixel
// position (its sub-level sets are the interiors of conic sections), so over the block's rectangle it peaks at a corner;
// the reference arithmetic's rounding (1e-16) and the f32 conversion (6e-8) sit far inside make_bundle's margins
// (sinT * 1.001 + 4e-6). All pixels inside the image count: a superset of the lanes Camera::render traces.
DEVI DevTileBundle cell_cone(const BinParams &Q, uint32_t view, uint32_t x0, uint32_t y0, uint32_t cell) {
#pragma clang fp contract(fast)
    const uint32_t x1 = min(x0 + cell - 1u, Q.W - 1u), y1 = min(y0 + cell - 1u, Q.H - 1u);
    const DevCamera &C = Q.views[view];
    const V3 o = xpoint(C.vinv, mk(0., 0., 0.));
    float ax, ay, az;
    bool good = finite3(o) && dir_f32(primary_dir<(RTC_BARE_SQRT & BS_BIN) != 0>(C, o, min(x0 + cell / 2u - 1u, x1), min(y0 + cell / 2u - 1u, y1)), ax, ay, az);
    float q2max = 0.f;
    bool narrow = true;
    // corners of the cell's pixel AREA (offsets 0 and 1, not the pixel centres): the cone then also holds every
    // anti-aliasing sub-sample and resample ray of its pixels (camera.rs:98-105: offsets in [0, 1))
    const uint32_t cx[4] = {x0, x1, x0, x1}, cy[4] = {y0, y0, y1, y1};
    for (int k = 0; k < 4; ++k) {
        float fx, fy, fz;
        good = dir_f32(primary_dir<(RTC_BARE_SQRT & BS_BIN) != 0>(C, o, cx[k], cy[k], (k & 1) ? 1.0 : 0.0, (k & 2) ? 1.0 : 0.0), fx, fy, fz) && good;
        const float dotv = ax * fx + ay * fy + az * fz;
        const float ux = ay * fz - az * fy, uy = az * fx - ax * fz, uz = ax * fy - ay * fx;
        q2max = fmaxf(q2max, ux * ux + uy * uy + uz * uz);
        narrow = narrow && dotv > 0.7f;
    }
    DevTileBundle r;
    r.ax = ax; r.ay = ay; r.az = az;
    r.sinT = __builtin_sqrtf(q2max) * 1.001f + 4e-6f;
    r.cosT = __builtin_sqrtf(fmaxf(0.f, 1.f - r.sinT * r.sinT));
    r.off = (good && narrow && r.sinT < 0.98f) ? 0u : 1u; // wide or odd cells: every object is a candidate
    return r;
}

// A tile-list entry: the object's index and, while the indices fit 16 bits (BinParams::packed), the upper half of its
// key above it — bound_key from the view's camera, truncated towards zero (keys are >= 0), so still a lower bound.
DEVI uint32_t bin_entry(const BinParams &Q, V3 o, const DevBound &b, uint32_t j) {
    if (!Q.packed) return j;
    return (__builtin_bit_cast(uint32_t, bound_key(o, b)) & 0xffff0000u) | j;
}

// The binning kernel: one wave per (view, macro tile of 64x64 pixels), lane = one of its 8x8 tiles of 8x8 pixels. Every
// object goes on the list of each tile whose cone (cell_cone) its bounding sphere can touch — bundle_touches, the wave-level
// cull's own conservative predicate. The wave first finds the objects its MACRO tile's cone can touch through the World's
// two-level tables (groups of 64 Morton-ordered objects, a sphere around each group: lane = group, then lane = member);
// every lane then tests those survivors — fetched by uniform index — against its own tile's cone and appends to its own
// list: no atomics, entries in table order, one launch per render. (Round 2 first PUSHED the objects into the tiles — one
// wave per (view, object), atomic appends, a second kernel for objects that cover many tiles, a third for the cones: the
// same lists at 3x the launches; C3 -2 %, C5 -3 %, one camera per launch C3 -11 % for this form,
// profiles/r02_exp_pull_binning.log.)
// Can NO ray of the cone `t` around apex `o` hit the plane whose stored inverse has the rows m[0..11]? Plane::intersect_local
// (shape.rs:462-471): none when |d'.y| < EPSILON, else t = -o'.y / d'.y, a hit iff t >= 0 — i.e. iff o'.y and d'.y differ in
// sign (or the quotient underflows to -0.0, which `t >= 0.0` accepts: |o'.y| >= 2^-500 and |r| <= 2^500 rule that out, as in
// plane_t_certainly_negative). o'.y is the same for every ray of the view (shared origin; evaluated as the kernel does); d'.y
// = r . d with r = (m4, m5, m6) and d a unit vector within theta of the axis a: s * (r . d) >= s*(r.a) cos(theta) - |r x a|
// sin(theta) when s*(r.a) > 0. Proven a miss when that lower bound clears 1e-4 |r| (the axis is unit to 2e-6, cos / sin carry
// cell_cone's margins, the reference's own roundings are 1e-16).
DEVI bool cone_misses_plane(const double *m, V3 o, const DevTileBundle &t) {
#pragma clang fp contract(fast) // cull arithmetic
    if (t.off != 0u) return false;
    const double oy = m[4] * o.x + m[5] * o.y + m[6] * o.z + m[7];
    if (!(fabs(oy) >= 0x1p-500) || !(fabs(oy) < __builtin_inf())) return false; // (0, NaN, inf: no proof)
    const double s = oy > 0. ? 1. : -1.;
    const double rx = m[4], ry = m[5], rz = m[6];
    const double rr = rx * rx + ry * ry + rz * rz;
    if (!(rr > 0x1p-900) || !(rr < 0x1p900)) return false;
    const double ra = s * (rx * (double)t.ax + ry * (double)t.ay + rz * (double)t.az);
    if (!(ra > 0.)) return false;
    const double perp = __builtin_sqrt(fmax(0., rr - ra * ra) * 1.00001 + 1e-10 * rr);
    const double lower = ra * (double)t.cosT * 0.99999 - perp * (double)t.sinT;
    return lower > 1e-4 * __builtin_sqrt(rr);
}

// SORT (its own instantiation; packed lists only: the launcher's condition): lists of at most RTC_TILE_SORT_CAP entries leave
// sorted ascending by entry, the order k_trace's scalar walk takes them in. A lane keeps a copy of its list's first entries
// in LDS (entry s of lane l at word l * (CAP + 1) + s: the odd stride keeps the lanes' accesses to one slot on different
// banks) and ranks them once the group walk is over. SORT = false is the kernel as it always was, LDS-free.
template <bool SORT>
__global__ void __launch_bounds__(64) k_bin_tiles(const BinParams Q, const DevBound *__restrict__ bound_s, const DevBound *__restrict__ gbound,
                                                   const uint32_t *__restrict__ orig_s, uint32_t ngroups, uint32_t *__restrict__ cnt,
                                                   uint32_t *__restrict__ list, const DevIsect *__restrict__ isect_s,
                                                   const uint32_t *__restrict__ kind_s, uint32_t n_unb, uint32_t *__restrict__ rows,
                                                   const DevIsect *__restrict__ isect, DevPrim *__restrict__ prim) {
    __shared__ uint32_t ents[SORT ? 64u * (RTC_TILE_SORT_CAP + 1u) : 1u];
    const uint32_t macros = Q.macros_x * Q.macros_y;
    const uint32_t view = blockIdx.x / macros, m = blockIdx.x % macros, lane = threadIdx.x;
    // The view's per-object primary-ray constants (camera origin in object space, the sphere's c: k_prep_primary's table,
    // same arithmetic) for the render kernel's binned pass, spread over all the view's binning threads.
    if (prim != nullptr) {
        const V3 cam = xpoint(Q.views[view].vinv, mk(0., 0., 0.));
        for (uint32_t j = m * 64u + lane; j < Q.n; j += macros * 64u) prim[(size_t)view * Q.n + j] = prim_of(isect[j].m, cam);
    }
    const uint32_t mx = m % Q.macros_x, my = m / Q.macros_x;
    const uint32_t tx = mx * 8u + (lane & 7u), ty = my * 8u + (lane >> 3);
    const bool mine = tx < Q.tiles_x && ty < Q.tiles_y && ty >= Q.row0 && (ty - Q.row0) % Q.row_stride == 0u;
    if (ballot(mine) == 0ull) return; // the launch renders none of this macro tile's rows
    const DevCamera &C = Q.views[view];
    V3 o = xpoint(C.vinv, mk(0., 0., 0.));
    o = mk(uniform_f64(o.x), uniform_f64(o.y), uniform_f64(o.z));
    const Bundle MB = bundle_of(cell_cone(Q, view, mx * 64u, my * 64u, 64u), o);
    const DevTileBundle tcone = cell_cone(Q, view, min(tx, Q.tiles_x - 1u) * 8u, min(ty, Q.tiles_y - 1u) * 8u, 8u);
    const Bundle TB = bundle_of(tcone, o);
    const size_t tile = (size_t)(view * Q.tiles_y + min(ty, Q.tiles_y - 1u)) * Q.tiles_x + min(tx, Q.tiles_x - 1u);
    uint32_t *my_list = list + tile * RTC_TILE_LIST_CAP;
    uint32_t my_cnt = 0;
    // is this tile's cone clear of every unbounded object? (uniform loop, scalar loads, ahead of the group walk so that their latency
    // is not on the kernel's tail; used below for the tile-row proof)
    bool clear_of_planes = n_unb <= 4u;
    for (uint32_t k = 0; k < n_unb && n_unb <= 4u; ++k)
        clear_of_planes = clear_of_planes && (kind_s[k] == RTC_PLANE) && cone_misses_plane(isect_s[k].m, o, tcone);
    for (uint32_t gbase = 0; gbase < ngroups; gbase += 64u) {
        const uint32_t g = gbase + lane;
        unsigned long long gmask = ballot(g < ngroups && bundle_touches(MB, gbound[g])); // (a group with an unbounded member: r = inf, kept)
        // the members' bounds of the NEXT touched group are requested before the current group's survivors are appended: the
        // expansions are a chain of dependent 48-byte-per-lane gathers otherwise (C3: 92 -> see profiles/r03_exp_small_steps.log)
        const DevBound none = DevBound{0., 0., 0., __builtin_inf(), 0., 0.};
        auto fetch = [&](uint32_t gs, DevBound &bb, uint32_t &oo) {
            const uint32_t kk = gs * 64u + lane;
            bb = none; oo = 0u;
            if (kk < Q.n) { bb = bound_s[kk]; oo = orig_s[kk]; }
        };
        DevBound b_next = none;
        uint32_t o_next = 0u;
        if (gmask) fetch(gbase + (uint32_t)__builtin_ctzll(gmask), b_next, o_next);
        while (gmask) {
            const uint32_t gsel = gbase + (uint32_t)__builtin_ctzll(gmask);
            gmask &= gmask - 1ull;
            const DevBound b = b_next;
            const uint32_t orig = o_next;
            if (gmask) fetch(gbase + (uint32_t)__builtin_ctzll(gmask), b_next, o_next);
            const uint32_t k = gsel * 64u + lane;
            bool to = false;
            uint32_t entry = 0u;
            if (k < Q.n) {
                to = b.r < __builtin_inf() && bundle_touches(MB, b); // unbounded objects are never listed: every tile tests them anyway
                if (to) entry = bin_entry(Q, o, b, orig);
            }
            unsigned long long omask = ballot(to);
            while (omask) { // the survivor's record comes from the lane that tested it (readlane: no second round trip to memory)
                const uint32_t l = (uint32_t)__builtin_ctzll(omask);
                omask &= omask - 1ull;
                const DevBound bj = DevBound{lane_f64(b.cx, l), lane_f64(b.cy, l), lane_f64(b.cz, l), lane_f64(b.r, l), lane_f64(b.k, l), lane_f64(b.cn, l)};
                const uint32_t ej = (uint32_t)__builtin_amdgcn_readlane((int)entry, (int)l);
                if (mine && bundle_touches(TB, bj)) {
                    if (my_cnt < RTC_TILE_LIST_CAP) my_list[my_cnt] = ej;
                    if constexpr (SORT) {
                        if (my_cnt < RTC_TILE_SORT_CAP) ents[lane * (RTC_TILE_SORT_CAP + 1u) + my_cnt] = ej;
                    }
                    ++my_cnt;
                }
            }
        }
    }
    if constexpr (SORT) {
        // Every lane ranks its own list, all 64 at once: an entry's rank is the number of the list's entries below it (entries
        // are unique: the object index is part of them), and the entry goes to that slot of the list — over the table-order
        // copy the appends left there. The lists' copies come out of LDS once, into registers (slots past a lane's count: the
        // largest word, below nothing); then at most c x 16 compares for the wave's longest short list c, and nothing at all
        // for a wave whose lists have at most one entry each.
        const uint32_t c = my_cnt <= RTC_TILE_SORT_CAP ? my_cnt : 0u; // (my_cnt != 0: the tile is `mine`)
        const uint32_t cmax = wave_max_u32(c);
        if (cmax >= 2u) {
            const uint32_t *const row = ents + lane * (RTC_TILE_SORT_CAP + 1u);
            uint32_t v[RTC_TILE_SORT_CAP];
#pragma unroll
            for (uint32_t k = 0; k < RTC_TILE_SORT_CAP; ++k) v[k] = k < c ? row[k] : 0xffffffffu;
#pragma unroll
            for (uint32_t e = 0; e < RTC_TILE_SORT_CAP; ++e) {
                if (e >= cmax) break; // (wave-uniform)
                uint32_t rank = 0u;
#pragma unroll
                for (uint32_t k = 0; k < RTC_TILE_SORT_CAP; ++k) rank += v[k] < v[e] ? 1u : 0u;
                if (e < c) my_list[rank] = v[e];
            }
        }
    }
    if (mine) cnt[tile] = my_cnt; // > RTC_TILE_LIST_CAP: the list is incomplete and the render wave walks instead
    // Tile rows that are PROVABLY BLACK for this view: a tile whose list is empty and whose cone misses every unbounded object
    // (planes: cone_misses_plane; anything else unbounded: no proof) has no primary hit at any pixel — Camera::render writes
    // background_color there (shape.rs:702-710, 652-653) whatever the rays' exact directions. rows[2v] = the smallest,
    // ~rows[2v + 1] the largest tile row with a tile that is NOT proven empty (both preset to 0xffffffff): the render kernel
    // skips ray generation and every pass for the tile rows outside that range (the sky of a floor scene: a third of the north star).
    const bool nonempty = mine && !(my_cnt == 0u && clear_of_planes);
    const uint32_t rmin = ~wave_max_u32(nonempty ? ~ty : 0u), rmaxinv = ~wave_max_u32(nonempty ? ty : 0u);
    const bool any_nonempty = ballot(nonempty) != 0ull; // (evaluated by the whole wave, not under the lane-0 branch)
    if (lane == 0u && any_nonempty) {
        // look before the atomic: the words only ever decrease, so a (possibly stale) value that is already small enough makes it
        // redundant — at 8192^2 sixteen thousand waves would otherwise queue on these two words (C5: the binning kernel 0.38 ms)
        volatile uint32_t *rw = rows + 2u * view;
        if (rmin < rw[0]) atomicMin(rows + 2u * view, rmin);
        if (rmaxinv < rw[1]) atomicMin(rows + 2u * view + 1u, rmaxinv);
    }
}

extern "C" hipError_t rtc_launch_binning(const DevCamera *views, uint32_t nviews, uint32_t W, uint32_t H, uint32_t n, const DevBound *bound_s,
                                         const DevBound *gbound, const uint32_t *orig_s, uint32_t ngroups, uint32_t *cnt, uint32_t *list,
                                         uint32_t row0, uint32_t row_stride, hipStream_t stream, hipEvent_t e0, hipEvent_t e1,
                                         const DevIsect *isect_s, const uint32_t *kind_s, uint32_t n_unb, uint32_t *rows,
                                         const DevIsect *isect, DevPrim *prim, uint32_t sort) {
    if (n == 0) return hipSuccess;
    if (hipMemsetAsync(rows, 0xff, sizeof(uint32_t) * 2u * RTC_MAX_VIEWS, stream) != hipSuccess) return hipGetLastError();
    BinParams Q;
    Q.row0 = row0; Q.row_stride = row_stride ? row_stride : 1u;
    for (uint32_t v = 0; v < nviews; ++v) Q.views[v] = views[v];
    for (uint32_t v = nviews; v < RTC_MAX_VIEWS; ++v) Q.views[v] = views[0];
    Q.nviews = nviews; Q.W = W; Q.H = H; Q.n = n;
    Q.packed = RTC_BIN_PACKED(n) ? 1u : 0u;
    Q.tiles_x = (W + 7u) / 8u; Q.tiles_y = (H + 7u) / 8u;
    Q.macros_x = (Q.tiles_x + 7u) / 8u; Q.macros_y = (Q.tiles_y + 7u) / 8u;
    // e0/e1 (may be NULL): the dispatch's own begin/end timestamps, as for k_trace
    const dim3 grid(nviews * Q.macros_x * Q.macros_y);
    if (sort != 0u && Q.packed != 0u)
        hipExtLaunchKernelGGL(k_bin_tiles<true>, grid, dim3(64), 0, stream, e0, e1, 0, Q, bound_s, gbound, orig_s, ngroups, cnt, list, isect_s, kind_s, n_unb,
                              rows, isect, prim);
    else
        hipExtLaunchKernelGGL(k_bin_tiles<false>, grid, dim3(64), 0, stream, e0, e1, 0, Q, bound_s, gbound, orig_s, ngroups, cnt, list, isect_s, kind_s, n_unb,
                              rows, isect, prim);
    return hipGetLastError();
}

// ---- light-space shadow lists (rtc_device.h) -------------------------------------------------------------------------
// Unit direction through cube-map coordinates (u, v) of face `face`.
DEVI void light_dir(uint32_t face, float u, float v, float &x, float &y, float &z) {
    const float s = (face & 1u) ? -1.f : 1.f;
    const uint32_t a = face >> 1;
    float c[3];
    c[a] = s; c[(a + 1u) % 3u] = u; c[(a + 2u) % 3u] = v;
    const float il = __builtin_amdgcn_rsqf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    x = c[0] * il; y = c[1] * il; z = c[2] * il;
}
// One thread per cell or per macro cell (8x8 cells): the cone of its directions (axis through the centre, half-angle to
// the farthest of the four corners — the angle to the axis is quasi-convex over the square — with make_bundle's margins).
__global__ void __launch_bounds__(256) k_light_cells(DevTileBundle *__restrict__ cells, DevTileBundle *__restrict__ macros, uint32_t *__restrict__ cnt) {
#pragma clang fp contract(fast)
    constexpr uint32_t R = RTC_LIGHT_R, M = RTC_LIGHT_R / 8u;
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t g, span;
    DevTileBundle *out;
    if (i < 6u * R * R) { g = R; span = 1u; out = cells; cnt[i] = 0u; }
    else if ((i -= 6u * R * R) < 6u * M * M) { g = M; span = 8u; out = macros; }
    else return;
    const uint32_t face = i / (g * g), ix = (i % g) * span, iy = ((i / g) % g) * span;
    const float u0 = (float)ix * (2.f / R) - 1.f, u1 = (float)(ix + span) * (2.f / R) - 1.f;
    const float v0 = (float)iy * (2.f / R) - 1.f, v1 = (float)(iy + span) * (2.f / R) - 1.f;
    float ax, ay, az;
    light_dir(face, 0.5f * (u0 + u1), 0.5f * (v0 + v1), ax, ay, az);
    const float cu[4] = {u0, u1, u0, u1}, cv[4] = {v0, v0, v1, v1};
    float q2max = 0.f;
    for (int k = 0; k < 4; ++k) {
        float fx, fy, fz;
        light_dir(face, cu[k], cv[k], fx, fy, fz);
        const float ux = ay * fz - az * fy, uy = az * fx - ax * fz, uz = ax * fy - ay * fx;
        q2max = fmaxf(q2max, ux * ux + uy * uy + uz * uz);
    }
    DevTileBundle r;
    r.ax = ax; r.ay = ay; r.az = az;
    r.sinT = __builtin_sqrtf(q2max) * 1.001f + 1e-5f; // + the f64 -> cell rounding of a direction on a cell border
    r.cosT = __builtin_sqrtf(fmaxf(0.f, 1.f - r.sinT * r.sinT));
    r.off = r.sinT < 0.7f ? 0u : 1u;
    out[i] = r;
}
DEVI Bundle light_bundle_of(const DevTileBundle &t, V3 apex, double reach) { // rays FROM the light, reach-limited (rho 0)
    Bundle B = bundle_of(t, apex);
    B.tmax = reach;
    B.spread = reach; // the exact rays start at the far end (DevBound rounding note)
    return B;
}
// One wave per object: macro cells (8x8 cells) 64 per step, then the cells of the touched macro cells.
DEVI void light_bin(uint32_t n, uint32_t cap, const DevBound *__restrict__ bound, double lx, double ly, double lz, double reach,
                    const DevTileBundle *__restrict__ cells, const DevTileBundle *__restrict__ macros,
                    uint32_t *__restrict__ cnt, uint32_t *__restrict__ list) {
    constexpr uint32_t R = RTC_LIGHT_R, M = RTC_LIGHT_R / 8u;
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    if (j >= n) return;
    const DevBound b = bound[j];
    if (!(b.r < __builtin_inf())) return; // unbounded: every shadow pass tests it anyway
    const V3 o = mk(lx, ly, lz);
    for (uint32_t mbase = 0; mbase < 6u * M * M; mbase += 64u) {
        const uint32_t m = mbase + lane;
        bool tm = false;
        if (m < 6u * M * M) tm = bundle_touches(light_bundle_of(macros[m], o, reach), b);
        unsigned long long mmask = ballot(tm);
        while (mmask) {
            const uint32_t msel = mbase + (uint32_t)__builtin_ctzll(mmask);
            mmask &= mmask - 1ull;
            const uint32_t face = msel / (M * M), mx = msel % M, my = (msel / M) % M;
            const uint32_t cell = (face * R + my * 8u + (lane >> 3)) * R + mx * 8u + (lane & 7u);
            if (bundle_touches(light_bundle_of(cells[cell], o, reach), b)) {
                const uint32_t slot = atomicAdd(cnt + cell, 1u);
                if (slot < cap) list[(size_t)cell * cap + slot] = j;
            }
        }
    }
}
__global__ void __launch_bounds__(64) k_light_bin(uint32_t n, uint32_t cap, const DevBound *__restrict__ bound, double lx, double ly, double lz, double reach,
                                                   const DevTileBundle *__restrict__ cells, const DevTileBundle *__restrict__ macros,
                                                   uint32_t *__restrict__ cnt, uint32_t *__restrict__ list) {
    light_bin(n, cap, bound, lx, ly, lz, reach, cells, macros, cnt, list);
}
// The same for a World built on the device (rtc_world_build.h): the reach is in the build's header, 0 when the World gets no lists.
__global__ void __launch_bounds__(64) k_light_bin_built(uint32_t n, uint32_t cap, const DevBound *__restrict__ bound, double lx, double ly, double lz,
                                                         const DevWorldHeader *__restrict__ hdr, const DevTileBundle *__restrict__ cells,
                                                         const DevTileBundle *__restrict__ macros, uint32_t *__restrict__ cnt, uint32_t *__restrict__ list) {
    const double reach = hdr->light_reach;
    if (reach > 0.) light_bin(n, cap, bound, lx, ly, lz, reach, cells, macros, cnt, list);
}

extern "C" hipError_t rtc_launch_light_lists(uint32_t n, uint32_t cap, const DevBound *bound, const double light[3], double reach, DevTileBundle *cells,
                                             DevTileBundle *macros, uint32_t *cnt, uint32_t *list, hipStream_t stream) {
    constexpr uint32_t R = RTC_LIGHT_R, M = RTC_LIGHT_R / 8u;
    hipLaunchKernelGGL(k_light_cells, dim3((6u * R * R + 6u * M * M + 255u) / 256u), dim3(256), 0, stream, cells, macros, cnt);
    if (n) hipLaunchKernelGGL(k_light_bin, dim3(n), dim3(64), 0, stream, n, cap, bound, light[0], light[1], light[2], reach, (const DevTileBundle *)cells,
                              (const DevTileBundle *)macros, cnt, list);
    return hipGetLastError();
}

// The lists of a World whose tables the device has just built on `stream`: clears the counters and bins with the header's
// reach. `cells` and `macros` are the World's cone tables as rtc_launch_light_lists left them (they do not depend on the World).
extern "C" hipError_t rtc_launch_light_lists_built(uint32_t n, uint32_t cap, const DevBound *bound, const double light[3], const DevWorldHeader *hdr,
                                                   const DevTileBundle *cells, const DevTileBundle *macros, uint32_t *cnt, uint32_t *list,
                                                   hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(cnt, 0, sizeof(uint32_t) * 6u * RTC_LIGHT_R * RTC_LIGHT_R, stream);
    if (e != hipSuccess) return e;
    if (n) hipLaunchKernelGGL(k_light_bin_built, dim3(n), dim3(64), 0, stream, n, cap, bound, light[0], light[1], light[2], hdr, cells, macros, cnt, list);
    return hipGetLastError();
}

// Un-deal (rtc_group_render, member 0): the gather leaves N chunks, chunk p = member p's packed bands of
// `nframes` frames ([nframes][rows_max][row_units] units each); this puts band k of member p at image rows
// (p + k*N)*8.. of its frame — the reference's row-major Canvas (canvas.rs:43-51). One unit = UNIT bytes
// (16 for the f64 canvas of an even-width image), one lane per unit, 256-B contiguous per wave-instruction.
template <class U>
__global__ void __launch_bounds__(256) k_undeal(const U *__restrict__ staging, U *__restrict__ canvas, uint32_t nranks,
                                                 uint32_t nframes, uint32_t H, uint32_t rows_max, uint32_t row_units) {
    const size_t total = (size_t)nframes * H * row_units;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (size_t)gridDim.x * 256u) {
        const uint32_t u = (uint32_t)(i % row_units);
        const size_t fy = i / row_units;
        const uint32_t y = (uint32_t)(fy % H), f = (uint32_t)(fy / H);
        canvas[i] = staging[rtc_staging_index(f, y, u, nranks, nframes, rows_max, row_units)]; // rtc_bands.h: THE mapping
    }
}

extern "C" hipError_t rtc_launch_undeal(const void *staging, void *canvas, uint32_t nranks, uint32_t nframes, uint32_t H,
                                        uint32_t rows_max, size_t row_bytes, hipStream_t stream) {
    if (nframes == 0 || H == 0 || row_bytes == 0) return hipSuccess;
    const bool a16 = row_bytes % 16u == 0 && ((size_t)staging % 16u) == 0 && ((size_t)canvas % 16u) == 0;
    const bool a8 = row_bytes % 8u == 0 && ((size_t)staging % 8u) == 0 && ((size_t)canvas % 8u) == 0;
    const uint32_t unit = a16 ? 16u : a8 ? 8u : 1u;
    const size_t total = (size_t)nframes * H * (row_bytes / unit);
    const uint32_t blocks = (uint32_t)((total + 255u) / 256u < 16384u ? (total + 255u) / 256u : 16384u);
    typedef unsigned __attribute__((ext_vector_type(4))) u4;
    if (unit == 16u)
        hipLaunchKernelGGL(k_undeal<u4>, dim3(blocks), dim3(256), 0, stream, (const u4 *)staging, (u4 *)canvas, nranks, nframes, H, rows_max, (uint32_t)(row_bytes / 16u));
    else if (unit == 8u)
        hipLaunchKernelGGL(k_undeal<unsigned long long>, dim3(blocks), dim3(256), 0, stream, (const unsigned long long *)staging, (unsigned long long *)canvas, nranks, nframes, H, rows_max, (uint32_t)(row_bytes / 8u));
    else
        hipLaunchKernelGGL(k_undeal<unsigned char>, dim3(blocks), dim3(256), 0, stream, (const unsigned char *)staging, (unsigned char *)canvas, nranks, nframes, H, rows_max, (uint32_t)row_bytes);
    return hipGetLastError();
}

// Canvas::to_imgbuf (canvas.rs:61-79) of an f64 canvas already in device memory: `n` pixels of 24 bytes in, 4 bytes out
// (alpha 255), every channel through the gamma's threshold table. One pixel per lane, grid-stride: consecutive lanes read
// consecutive 24-byte pixels and write consecutive dwords.
__global__ void __launch_bounds__(256) k_canvas_to_rgba8(const double *__restrict__ rgb, size_t n, const DevGamma *__restrict__ g,
                                                         unsigned char *__restrict__ out, uint32_t aligned4) {
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const double r = rgb[i * 3u], gr = rgb[i * 3u + 1u], b = rgb[i * 3u + 2u];
        const unsigned v = (unsigned)gamma_byte(g, r) | ((unsigned)gamma_byte(g, gr) << 8) | ((unsigned)gamma_byte(g, b) << 16) | 0xff000000u;
        if (aligned4) __builtin_nontemporal_store(v, reinterpret_cast<unsigned *>(out + i * 4u));
        else {
            out[i * 4u] = (unsigned char)v;
            out[i * 4u + 1u] = (unsigned char)(v >> 8);
            out[i * 4u + 2u] = (unsigned char)(v >> 16);
            out[i * 4u + 3u] = 255u;
        }
    }
}

extern "C" hipError_t rtc_launch_canvas_to_rgba8(const double *rgb, size_t n, const DevGamma *g, unsigned char *out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t want = (n + 255u) / 256u;
    const uint32_t blocks = (uint32_t)(want < 8192u ? want : 8192u); // at most 8192 workgroups (2M lanes); the loop strides over the rest
    hipLaunchKernelGGL(k_canvas_to_rgba8, dim3(blocks), dim3(256), 0, stream, rgb, n, g, out, ((size_t)out % 4u) == 0 ? 1u : 0u);
    return hipGetLastError();
}

// ---- stages the tile passes share (k_aov, k_ao, k_gather) -----------------------------------------------------------
// Each in the form that leaves the kernels' instruction streams as they were ("Shared stages of the tile
// passes"): results by value, the tables filled in place. The primary pass's closest-hit walk, the shadow test of one light, the
// sample direction and the whole hit frame as one function are not among them: as functions they compile to other code.

// The World's tables from a tile pass's eleven pointer arguments (k_trace's, less prim and idtab).
DEVI void tile_tables(Tables &T, const DevIsect *isect, const uint32_t *kind, const DevShade *shade, const DevBound *bound, const DevIsect *isect_s,
                      const uint32_t *kind_s, const DevBound *bound_s, const uint32_t *orig_s, const DevBound *gbound, const DevPre *pre,
                      const DevPre *pre_s) {
    T.isect = isect; T.kind = kind; T.shade = shade; T.bound = bound;
    T.isect_s = isect_s; T.kind_s = kind_s; T.bound_s = bound_s; T.orig_s = orig_s; T.gbound = gbound;
    T.pre = pre; T.pre_s = pre_s;
}

// The lane's pixel: one wave = one 8x8 tile = one workgroup, tile id = workgroup id, one pixel per lane. in_range: the pixel
// exists (partial tiles on the right and bottom edges mask their lanes) and is stored; traced: it also gets a ray —
// Camera::render leaves the last row and column untouched (camera.rs:120-121), they get the miss values.
struct TileLane { uint32_t px, py; bool in_range, traced; };
DEVI TileLane tile_lane(const TileParams &A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t px = (blockIdx.x % A.tiles_x) * 8u + (lane & 7u), py = (blockIdx.x / A.tiles_x) * 8u + (lane >> 3);
    const bool in_range = px < A.W && py < A.H;
    return TileLane{px, py, in_range, in_range && !(A.mode == RTC_MODE_RENDER && (px + 1u >= A.W || py + 1u >= A.H))};
}

// ray_for_pixel(x, 0.5, y, 0.5): camera.rs:64-76. The origin is the same in every lane (SGPRs): the primary bundle's shared apex.
struct PrimaryRay { V3 ro, rd; };
DEVI PrimaryRay primary_ray(const DevCamera &C, uint32_t px, uint32_t py) {
    V3 cam_origin = xpoint(C.vinv, mk(0., 0., 0.));
    cam_origin = mk(uniform_f64(cam_origin.x), uniform_f64(cam_origin.y), uniform_f64(cam_origin.z));
    return PrimaryRay{cam_origin, primary_dir(C, cam_origin, px, py)};
}

// The projection flavour of the tile passes (a trailing DevProjection, as k_trace's; rtc_render_aov_projection* and its
// kin): the two stages that differ from the pinhole's, chosen with `if constexpr` — a pinhole instantiation sees neither.
// rtc_projection_ray(x, y) (include/rtc.h) in k_trace's PROJ block's order, operation for operation. `kind` is wave-uniform
// and read here only; what follows asks `shared`: every ray leaves the camera origin (panorama) or each its own point of the
// camera's z = 0 plane (orthographic). The panorama's {sin, cos} come from the host's tables, one 16-byte load each; lanes
// outside the canvas read entry 0.
struct ProjectionRay { V3 ro, rd; bool shared; };
DEVI ProjectionRay projection_ray(const DevCamera &C, const DevProjection &PJ, uint32_t px, uint32_t py, bool in_range) {
    if (PJ.kind == RTC_PROJ_ORTHOGRAPHIC) {
        const double ox = PJ.half_w - ((double)px + 0.5) * PJ.pixel;
        const double oy = PJ.half_h - ((double)py + 0.5) * PJ.pixel;
        const V3 ro = xpoint(C.vinv, mk(ox, oy, 0.));
        return ProjectionRay{ro, vnormalize_plain(vsub(xpoint(C.vinv, mk(ox, oy, -1.)), ro)), false};
    }
    typedef double SinCos __attribute__((ext_vector_type(2)));
    V3 cam_origin = xpoint(C.vinv, mk(0., 0., 0.));
    cam_origin = mk(uniform_f64(cam_origin.x), uniform_f64(cam_origin.y), uniform_f64(cam_origin.z));
    const SinCos c = *reinterpret_cast<const SinCos *>(PJ.col + 2u * (size_t)(in_range ? px : 0u));
    const SinCos r = *reinterpret_cast<const SinCos *>(PJ.row + 2u * (size_t)(in_range ? py : 0u));
    const V3 target = xpoint(C.vinv, mk(r.y * c.x, r.x, -(r.y * c.y)));
    return ProjectionRay{cam_origin, vnormalize_plain(vsub(target, cam_origin)), true};
}
// World::intersect + get_hit of those rays, k_trace's PROJ flavour: a panorama's bundle has the camera origin as its shared
// apex, and a two-level World takes the ordered walk with early stop; an orthographic tile's bundle is the general form
// (apex = the axis lane's origin, rho the spread of the others), and without a shared origin there is no ordered walk: every
// candidate is visited, behind the per-lane prefilter in two-level Worlds.
template <int SRC, class PP>
DEVI void projection_closest_hit(const PP &A, const Tables &T, const LdsView &L, bool traced, bool shared, V3 ro, V3 rd, double &best, int &hidx,
                                 int &hroot) {
    Bundle B{};
    B.off = true;
    if constexpr (IS_CULL(SRC)) {
        if (ballot(traced) != 0ull) {
            if (shared) B = make_bundle<true, false>(traced, ro, ro, rd, 0.);
            else B = make_bundle<false, false>(traced, ro, ro, rd, 0.);
        }
    }
    if (SRC == SRC_CULL2 && shared)
        for_each_object<SRC, false>(A, T, L, traced, B, ClosestHit{traced, ro, rd, best, hidx, hroot}, ro, rd, [&](float key) { return ballot(traced && !(best < (double)key)) == 0ull; });
    else
        for_each_object<SRC, SRC == SRC_CULL2>(A, T, L, traced, B, ClosestHit{traced, ro, rd, best, hidx, hroot}, ro, rd);
}

// The hit frame of k_ao and k_gather, in two parts. Intersection::compute_vectors' normal (shape.rs:144-152, 75-96) of object
// `hidx` at `point`, flipped to face a ray of direction rd; and rtc_ao.h's tangent frame about it, built once per pixel, in
// front of the sample loop (its one division).
DEVI V3 facing_normal(const Tables &T, int hidx, V3 point, V3 rd) {
    V3 normal = shape_normal(T.shade + hidx, T.isect[hidx].m, point);
    if (vdot(normal, vneg(rd)) < 0.0) normal = vneg(normal);
    return normal;
}
struct Tangents { V3 tv, sv; };
DEVI Tangents tangent_frame(V3 normal) {
    const double nn[3] = {normal.x, normal.y, normal.z};
    double t3[3], s3[3];
    rtc_ao_frame(nn, t3, s3);
    return Tangents{mk(t3[0], t3[1], t3[2]), mk(s3[0], s3[1], s3[2])};
}

// The reach of a sample's bundle (k_ao, k_gather): per sample a bundle over the lanes' rays, origins per lane (apex = the axis
// lane's over_point, rho the spread of the others around it). It is make_bundle's unbounded per-lane-origin form with the reach
// put in afterwards, not its REACH form: that one is for segments the exact test walks from the far end (spread = reach) and
// gives up on an unbounded reach, where these passes start every exact ray at its lane's origin (spread = rho) and
// radius = +inf still has a cone to cull with. Rounded up as the REACH form rounds it (f32, 1e-4 relative: the direction is
// unit to a few ulp).
DEVI void limit_reach(Bundle &Bk, double radius) {
    if (radius < 1e30) Bk.tmax = uniform_f64((double)(fmaxf(0.f, (float)radius) * 1.0001f + 1e-30f));
}

// ---- AOV planes (rtc_render_aov*, include/rtc.h): what each pixel's centre ray saw ----------------------------------
// k_trace's primary pass, its compute_vectors and — SHADOW only — one any-hit pass per light sample, and nothing of the
// shading: no material, no pattern, no recursion, no counters. One wave = one 8x8 pixel tile (tile_lane), so the primary
// bundle's cone is tight; the cull walks are wave-level code (ballots, DPP) and stay in converged code, every lane reaching them.
// SRC: SRC_SMEM (RTC_FLAG_NO_CULL), SRC_CULL or SRC_CULL2 (the ordered walk with the skip functor, as k_trace's large-world
// primary pass). There is no binning kernel, no per-launch DevPrim table: closest_world transforms the origin itself, with
// the arithmetic k_prep_primary has. XL: empty for one light, or the World's further lights (DevExtraLights / DevLightTable),
// SHADOW instantiations only. Results do not depend on SRC: closer() orders by (t, insertion index), the cull is conservative.
// A DevProjection as the pack's last element (both SHADOW forms): the projection flavour, one for both kinds — projection_ray
// and projection_closest_hit in the place of primary_ray and the primary pass, everything behind the hit as it stands.
template <int SRC, bool SHADOW, class... XL>
__global__ void __launch_bounds__(64, RTC_WAVES_PER_SIMD)
k_aov(const AovParams A, const DevIsect *__restrict__ t_isect, const uint32_t *__restrict__ t_kind, const DevShade *__restrict__ t_shade,
      const DevBound *__restrict__ t_bound, const DevIsect *__restrict__ t_isect_s, const uint32_t *__restrict__ t_kind_s,
      const DevBound *__restrict__ t_bound_s, const uint32_t *__restrict__ t_orig_s, const DevBound *__restrict__ t_gbound,
      const DevPre *__restrict__ t_pre, const DevPre *__restrict__ t_pre_s, const XL... xl_arg) {
    static_assert(SRC == SRC_SMEM || IS_CULL(SRC), "AOV launches take SRC_SMEM, SRC_CULL or SRC_CULL2");
    constexpr bool PROJ = has_projection_v<XL...>; // (the pack's last element, behind the further lights)
    constexpr size_t LIGHT_BLOCKS = sizeof...(XL) - (PROJ ? 1 : 0);
    static_assert(LIGHT_BLOCKS <= (SHADOW ? 1 : 0), "further lights only where shadow rays are cast, one block at most");
    Tables T{};
    tile_tables(T, t_isect, t_kind, t_shade, t_bound, t_isect_s, t_kind_s, t_bound_s, t_orig_s, t_gbound, t_pre, t_pre_s);
    const LdsView L{};
    const TileLane lane = tile_lane(A);
    const uint32_t px = lane.px, py = lane.py;
    const bool in_range = lane.in_range, traced = lane.traced;
    PrimaryRay pr;
    bool shared_origin = true; // (a pinhole's rays; a projection's: projection_ray)
    if constexpr (PROJ) {
        const ProjectionRay q = projection_ray(A.cam, last_of(xl_arg...), px, py, in_range);
        pr = PrimaryRay{q.ro, q.rd};
        shared_origin = q.shared;
    } else {
        pr = primary_ray(A.cam, px, py);
    }
    const V3 ro = pr.ro, rd = pr.rd;

    // ---- World::intersect + get_hit, streaming form (k_trace's primary pass without the tile lists) ----
    double best = __builtin_inf();
    int hidx = -1, hroot = 0;
    if constexpr (PROJ) {
        projection_closest_hit<SRC>(A, T, L, traced, shared_origin, ro, rd, best, hidx, hroot);
    } else {
    Bundle B{};
    B.off = true;
    if constexpr (IS_CULL(SRC)) {
        if (ballot(traced) != 0ull) B = make_bundle<true, false>(traced, ro, ro, rd, 0.);
    }
    if constexpr (SRC == SRC_CULL2)
        for_each_object<SRC, false>(A, T, L, traced, B, ClosestHit{traced, ro, rd, best, hidx, hroot}, ro, rd, [&](float key) { return ballot(traced && !(best < (double)key)) == 0ull; });
    else
        for_each_object<SRC>(A, T, L, traced, B, ClosestHit{traced, ro, rd, best, hidx, hroot}, ro, rd);
    }
    const bool hit = traced && hidx >= 0;

    // ---- Intersection::compute_vectors (shape.rs:144-152, 75-96), the part the planes hold ----
    V3 point = mk(0., 0., 0.), normal = mk(0., 0., 0.), over = mk(0., 0., 0.);
    bool inside = false;
    if (hit) point = vadd(ro, vmul(rd, best)); // Ray::position vec.rs:207-209
    if (SHADOW || A.normal != nullptr || A.flags != nullptr) { // (wave-uniform)
        if (hit) {
            const DevShade *S = T.shade + hidx;
            const double *m_obj = T.isect[hidx].m;
            const V3 eyev = vneg(rd);
            normal = shape_normal(S, m_obj, point);
            inside = vdot(normal, eyev) < 0.0;
            if (inside) normal = vneg(normal);
            over = vadd(point, vmul(normal, RTC_EPSILON));
        }
    }

    // ---- is_shadowed_by_light (shape.rs:716-727) per light sample, in order: how many hide the point ----
    uint32_t count = 0u;
    if constexpr (SHADOW) {
        auto one_light = [&](V3 lp) {
            V3 ldir = mk(0., 0., 0.);
            double ldist = 0.;
            shadow_ray(lp, over, hit, ldir, ldist);
            bool pending = hit, shadowed = false;
            Bundle Bl{};
            Bl.off = true;
            if constexpr (IS_CULL(SRC)) { // the segment over_point -> light, walked from the light: apex = light (shared), reach-limited
                if (ballot(hit) != 0ull) Bl = make_bundle<true, true>(hit, lp, lp, vneg(ldir), ldist);
            }
            // (the per-lane prefilter in front of the exact tests where k_trace's flat kernels have it: two-level Worlds)
            for_each_object<SRC, SRC == SRC_CULL2>(A, T, L, pending, Bl, AnyHit{pending, over, ldir, ldist, shadowed}, over, ldir);
            if (shadowed) ++count;
        };
        one_light(mk(A.light_pos[0], A.light_pos[1], A.light_pos[2]));
        if constexpr (LIGHT_BLOCKS == 1) {
            const auto &X = first_of(xl_arg...); // DevExtraLights (kernel arguments) or DevLightTable (HBM)
            const uint32_t n_extra = further_light_count(X);
            for (uint32_t li = 0; li < n_extra; ++li) one_light(further_light_position(X, li));
        }
    }

    // ---- the planes asked for (wave-uniform choice), one pixel per lane: plain vector stores ----
    if (in_range) {
        const size_t idx = (size_t)py * A.W + px;
        if (A.index != nullptr) A.index[idx] = hit ? hidx : -1;
        if (A.depth != nullptr) A.depth[idx] = hit ? best : __builtin_inf();
        if (A.point != nullptr) { A.point[3u * idx] = point.x; A.point[3u * idx + 1u] = point.y; A.point[3u * idx + 2u] = point.z; }
        if (A.normal != nullptr) { A.normal[3u * idx] = normal.x; A.normal[3u * idx + 1u] = normal.y; A.normal[3u * idx + 2u] = normal.z; }
        if (A.flags != nullptr) A.flags[idx] = hit ? (uint8_t)(1u | (inside ? 2u : 0u)) : (uint8_t)0u;
        if constexpr (SHADOW) A.shadow[idx] = (uint16_t)count;
    }
}

// rtc_aov_view_rgb8 on the device: one thread per pixel, the rules of rtc_aov.h, Color::scale by scale255 (rtc_gamma.h)
__global__ void __launch_bounds__(256) k_aov_view(const AovViewParams V) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= V.n) return;
    uint8_t o[3];
    if (V.view == RTC_AOV_VIEW_DEPTH) {
        o[0] = o[1] = o[2] = scale255(rtc_aov_depth_value(V.depth[i], V.near, V.far));
    } else if (V.view == RTC_AOV_VIEW_NORMAL) {
        for (uint32_t k = 0; k < 3u; ++k) o[k] = scale255(rtc_aov_normal_value(V.normal[3u * i + k]));
    } else if (V.view == RTC_AOV_VIEW_INDEX) {
        rtc_aov_index_rgb(V.index[i], o);
    } else {
        o[0] = o[1] = o[2] = scale255(rtc_aov_shadow_value(V.shadow[i], V.n_lights));
    }
    V.out[3u * i] = o[0];
    V.out[3u * i + 1u] = o[1];
    V.out[3u * i + 2u] = o[2];
}

// ---- ambient occlusion (rtc_render_ao*, include/rtc.h) ---------------------------------------------------------------
// k_aov's shape — one wave = one 8x8 pixel tile = one workgroup, the same primary pass and compute_vectors, one pixel per
// lane stored — with, in place of the light loop, a wave-uniform loop over the samples of the host's table: sample k's local
// direction is read by a uniform address (scalar loads, SGPRs), each lane turns it about its own normal (rtc_ao.h: the
// header's arithmetic, no sin or cos here) and the bounded any-hit walk counts the lanes that meet something with t < radius.
// Lanes without a hit carry pending = false through every walk: the walks are wave-level code and stay converged.
// Cull sources: per sample a bundle over the lanes' rays (limit_reach). Where a tile's normals diverge the cone passes 0.98 /
// the axis dot falls under 0.2 and the bundle goes off: every object is a candidate, which is correct and slower. Results do
// not depend on SRC.
// The per-lane prefilter (ray_touches_pre: it takes d.d, so the direction need not be unit) stands in front of the exact tests
// in the one-level walks too, where k_aov's shadow passes have it for two-level Worlds only: a shadow bundle always holds, an AO
// bundle is off wherever a tile's normals diverge, and then the filter is the only cull there is. RTC_AO_LANE_FILTER_ONE_LEVEL=0
// takes it out (A/B: north star, 1080p, 0.35 -> 0.22 ms at 4 samples, 4.5 -> 2.6 ms at 64; profiles/ao_lane_filter_ab.log).
#ifndef RTC_AO_LANE_FILTER_ONE_LEVEL
#define RTC_AO_LANE_FILTER_ONE_LEVEL 1
#endif
template <int SRC> constexpr bool SAMPLE_LANE_FILTER = SRC == SRC_CULL2 || (SRC == SRC_CULL && RTC_AO_LANE_FILTER_ONE_LEVEL); // the sample walks of k_ao and k_gather
// XP: nothing, or a DevProjection (the projection flavour, as k_aov's; facing_normal then takes a direction per lane)
template <int SRC, class... XP>
__global__ void __launch_bounds__(64, RTC_WAVES_PER_SIMD)
k_ao(const AoParams A, const double *__restrict__ t_dirs, const DevIsect *__restrict__ t_isect, const uint32_t *__restrict__ t_kind,
     const DevShade *__restrict__ t_shade, const DevBound *__restrict__ t_bound, const DevIsect *__restrict__ t_isect_s,
     const uint32_t *__restrict__ t_kind_s, const DevBound *__restrict__ t_bound_s, const uint32_t *__restrict__ t_orig_s,
     const DevBound *__restrict__ t_gbound, const DevPre *__restrict__ t_pre, const DevPre *__restrict__ t_pre_s, const XP... xp_arg) {
    static_assert(SRC == SRC_SMEM || IS_CULL(SRC), "AO launches take SRC_SMEM, SRC_CULL or SRC_CULL2");
    constexpr bool PROJ = has_projection_v<XP...>;
    static_assert(sizeof...(XP) == (PROJ ? 1 : 0), "nothing, or the projection");
    Tables T{};
    tile_tables(T, t_isect, t_kind, t_shade, t_bound, t_isect_s, t_kind_s, t_bound_s, t_orig_s, t_gbound, t_pre, t_pre_s);
    const LdsView L{};
    const TileLane lane = tile_lane(A);
    const uint32_t px = lane.px, py = lane.py;
    const bool in_range = lane.in_range, traced = lane.traced;
    PrimaryRay pr;
    bool shared_origin = true; // (a pinhole's rays; a projection's: projection_ray)
    if constexpr (PROJ) {
        const ProjectionRay q = projection_ray(A.cam, last_of(xp_arg...), px, py, in_range);
        pr = PrimaryRay{q.ro, q.rd};
        shared_origin = q.shared;
    } else {
        pr = primary_ray(A.cam, px, py);
    }
    const V3 ro = pr.ro, rd = pr.rd;

    // ---- World::intersect + get_hit, streaming form (k_aov's primary pass) ----
    double best = __builtin_inf();
    int hidx = -1, hroot = 0;
    if constexpr (PROJ) {
        projection_closest_hit<SRC>(A, T, L, traced, shared_origin, ro, rd, best, hidx, hroot);
    } else {
    Bundle B{};
    B.off = true;
    if constexpr (IS_CULL(SRC)) {
        if (ballot(traced) != 0ull) B = make_bundle<true, false>(traced, ro, ro, rd, 0.);
    }
    if constexpr (SRC == SRC_CULL2)
        for_each_object<SRC, false>(A, T, L, traced, B, ClosestHit{traced, ro, rd, best, hidx, hroot}, ro, rd, [&](float key) { return ballot(traced && !(best < (double)key)) == 0ull; });
    else
        for_each_object<SRC>(A, T, L, traced, B, ClosestHit{traced, ro, rd, best, hidx, hroot}, ro, rd);
    }
    const bool hit = traced && hidx >= 0;

    // ---- Intersection::compute_vectors (shape.rs:144-152, 75-96): normal and over_point; then the tangent frame ----
    V3 normal = mk(0., 0., 0.), over = mk(0., 0., 0.), tv = mk(0., 0., 0.), sv = mk(0., 0., 0.);
    if (hit) {
        const V3 point = vadd(ro, vmul(rd, best)); // Ray::position vec.rs:207-209
        normal = facing_normal(T, hidx, point, rd);
        over = vadd(point, vmul(normal, RTC_EPSILON));
        const Tangents tf = tangent_frame(normal);
        tv = tf.tv;
        sv = tf.sv;
    }

    // ---- one bounded any-hit pass per sample, in the table's order: how many meet something within the radius ----
    uint32_t count = 0u;
    const double radius = A.radius;
    const uint32_t ns = A.nsamples;
    for (uint32_t k = 0; k < ns; ++k) {
        const double lx = t_dirs[3u * k], ly = t_dirs[3u * k + 1u], lz = t_dirs[3u * k + 2u]; // (k is wave-uniform: scalar loads)
        const V3 dir = mk(rtc_ao_dir(tv.x, sv.x, normal.x, lx, ly, lz), rtc_ao_dir(tv.y, sv.y, normal.y, lx, ly, lz),
                          rtc_ao_dir(tv.z, sv.z, normal.z, lx, ly, lz));
        bool pending = hit, occluded = false;
        Bundle Bk{};
        Bk.off = true;
        if constexpr (IS_CULL(SRC)) {
            if (ballot(hit) != 0ull) {
                Bk = make_bundle<false, false>(hit, over, over, dir, 0.);
                limit_reach(Bk, radius);
            }
        }
        for_each_object<SRC, SAMPLE_LANE_FILTER<SRC>>(A, T, L, pending, Bk, AnyHit{pending, over, dir, radius, occluded}, over, dir);
        if (occluded) ++count;
    }

    if (in_range) A.out[(size_t)py * A.W + px] = (uint16_t)count; // one pixel per lane: plain vector stores
}

// rtc_canvas_apply_ao on the device: one thread per pixel, rtc_ao.h's factor
__global__ void __launch_bounds__(256) k_apply_ao(double *__restrict__ rgb, const uint16_t *__restrict__ ao, size_t n, uint32_t n_samples, double strength) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double f = rtc_ao_factor(ao[i], n_samples, strength);
    rgb[3u * i] = rgb[3u * i] * f;
    rgb[3u * i + 1u] = rgb[3u * i + 1u] * f;
    rgb[3u * i + 2u] = rgb[3u * i + 2u] * f;
}

// ---- colour bleeding: one bounce gathered over the AO fan (rtc_render_gather*, include/rtc.h) ------------------------
// k_ao's shape, primary pass, compute_vectors and tangent frame, and its wave-uniform sample loop with the directions by
// scalar loads. Per sample, where k_ao asks "anything within the radius?":
//   1. a closest-hit walk (ClosestHit) for the lanes whose pixel hit, with k_ao's per-sample bundle (per-lane origins, the
//      reach in tmax when the radius is finite) and the per-lane prefilter. Both are culls: an object they drop cannot be
//      hit with 0 <= t < radius, and a hit at t >= radius is not counted whatever it is, so the bytes never depend on them.
//      The ordered walk's early exit (Skip) needs rays that start at the bundle's apex and is not available here: this walk
//      visits every candidate, where k_ao's any-hit walk stops at the first object in the way.
//   2. for the lanes with a counted hit (one with t < radius): the secondary normal, the inside flip against -dir, the
//      over-point, eyev = -dir — compute_vectors without compute_refractive and reflectv, which remaining == 0 never reads.
//   3. the light loop as k_aov<SRC, true, XL...> runs it (shadow_ray, the light's bundle, AnyHit), each light followed by
//      lighting() — the function k_trace shades with, so the terms are k_trace's arithmetic — summed in light order.
//   4. the sample's colour added to three doubles per lane (a lane without a counted hit adds 0.0).
// Lanes without work carry pending = false; every walk is reached by the whole wave. Whether `bounce` is wanted is a
// wave-uniform argument (A.bounce): one `base` evaluation per pixel behind the loop, from the primary hit's index and
// over-point, which are live through the loop anyway. XL: as k_aov's (nothing, DevExtraLights or DevLightTable, and behind them
// a DevProjection for the projection flavour).
// Registers: the loop carries the primary hit's frame (normal, over, t, s: 24 VGPRs), the accumulator (6) and, across the
// light loop, the secondary hit (normal, over, direction: 18) on top of what a walk needs, which is more than k_ao's 90; the
// bound is four waves per SIMD (128 VGPRs), the step at which no instantiation spills (profiles/gather_kernel_resources.txt).
#ifndef RTC_GATHER_WAVES_PER_SIMD
#define RTC_GATHER_WAVES_PER_SIMD 4
#endif
template <int SRC, class... XL>
__global__ void __launch_bounds__(64, RTC_GATHER_WAVES_PER_SIMD)
k_gather(const GatherParams A, const double *__restrict__ t_dirs, const DevIsect *__restrict__ t_isect, const uint32_t *__restrict__ t_kind,
         const DevShade *__restrict__ t_shade, const DevBound *__restrict__ t_bound, const DevIsect *__restrict__ t_isect_s,
         const uint32_t *__restrict__ t_kind_s, const DevBound *__restrict__ t_bound_s, const uint32_t *__restrict__ t_orig_s,
         const DevBound *__restrict__ t_gbound, const DevPre *__restrict__ t_pre, const DevPre *__restrict__ t_pre_s, const XL... xl_arg) {
    static_assert(SRC == SRC_SMEM || IS_CULL(SRC), "gather launches take SRC_SMEM, SRC_CULL or SRC_CULL2");
    constexpr bool PROJ = has_projection_v<XL...>; // (the pack's last element, behind the further lights)
    constexpr size_t LIGHT_BLOCKS = sizeof...(XL) - (PROJ ? 1 : 0);
    static_assert(LIGHT_BLOCKS <= 1, "the further lights: one block at most");
    Tables T{};
    tile_tables(T, t_isect, t_kind, t_shade, t_bound, t_isect_s, t_kind_s, t_bound_s, t_orig_s, t_gbound, t_pre, t_pre_s);
    const LdsView L{};
    const TileLane lane = tile_lane(A);
    const uint32_t px = lane.px, py = lane.py;
    const bool in_range = lane.in_range, traced = lane.traced;
    PrimaryRay pr;
    bool shared_origin = true; // (a pinhole's rays; a projection's: projection_ray)
    if constexpr (PROJ) {
        const ProjectionRay q = projection_ray(A.cam, last_of(xl_arg...), px, py, in_range);
        pr = PrimaryRay{q.ro, q.rd};
        shared_origin = q.shared;
    } else {
        pr = primary_ray(A.cam, px, py);
    }
    const V3 ro = pr.ro, rd = pr.rd;

    // ---- World::intersect + get_hit, streaming form (k_aov's primary pass) ----
    double best = __builtin_inf();
    int hidx = -1, hroot = 0;
    if constexpr (PROJ) {
        projection_closest_hit<SRC>(A, T, L, traced, shared_origin, ro, rd, best, hidx, hroot);
    } else {
    Bundle B{};
    B.off = true;
    if constexpr (IS_CULL(SRC)) {
        if (ballot(traced) != 0ull) B = make_bundle<true, false>(traced, ro, ro, rd, 0.);
    }
    if constexpr (SRC == SRC_CULL2)
        for_each_object<SRC, false>(A, T, L, traced, B, ClosestHit{traced, ro, rd, best, hidx, hroot}, ro, rd, [&](float key) { return ballot(traced && !(best < (double)key)) == 0ull; });
    else
        for_each_object<SRC>(A, T, L, traced, B, ClosestHit{traced, ro, rd, best, hidx, hroot}, ro, rd);
    }
    const bool hit = traced && hidx >= 0;

    // ---- Intersection::compute_vectors (shape.rs:144-152, 75-96): normal and over_point; then the tangent frame ----
    V3 normal = mk(0., 0., 0.), over = mk(0., 0., 0.), tv = mk(0., 0., 0.), sv = mk(0., 0., 0.);
    if (hit) {
        const V3 point = vadd(ro, vmul(rd, best)); // Ray::position vec.rs:207-209
        normal = facing_normal(T, hidx, point, rd);
        over = vadd(point, vmul(normal, RTC_EPSILON));
        const Tangents tf = tangent_frame(normal);
        tv = tf.tv;
        sv = tf.sv;
    }

    // ---- per sample, in the table's order: the first hit within the radius, shaded under every light ----
    V3 acc = mk(0.0, 0.0, 0.0); // Color::average_over's sum: from 0.0, in sample order
    const double radius = A.radius;
    const uint32_t ns = A.nsamples;
    for (uint32_t k = 0; k < ns; ++k) {
        const double lx = t_dirs[3u * k], ly = t_dirs[3u * k + 1u], lz = t_dirs[3u * k + 2u]; // (k is wave-uniform: scalar loads)
        const V3 dir = mk(rtc_ao_dir(tv.x, sv.x, normal.x, lx, ly, lz), rtc_ao_dir(tv.y, sv.y, normal.y, lx, ly, lz),
                          rtc_ao_dir(tv.z, sv.z, normal.z, lx, ly, lz));
        // 1. World::intersect + get_hit of the sample's ray
        double sbest = __builtin_inf();
        int sidx = -1, sroot = 0;
        Bundle Bk{};
        Bk.off = true;
        if constexpr (IS_CULL(SRC)) {
            if (ballot(hit) != 0ull) {
                Bk = make_bundle<false, false>(hit, over, over, dir, 0.);
                limit_reach(Bk, radius);
            }
        }
        for_each_object<SRC, SAMPLE_LANE_FILTER<SRC>>(A, T, L, hit, Bk, ClosestHit{hit, over, dir, sbest, sidx, sroot}, over, dir);
        const bool counted = hit && sidx >= 0 && sbest < radius;

        // 2. compute_vectors of the counted hit: eyev = -dir, the normal with its inside flip, over_point
        const DevShade *S2 = T.shade + (counted ? sidx : 0);
        const double *m2 = T.isect[counted ? sidx : 0].m;
        const V3 seye = vneg(dir);
        V3 snormal = mk(0., 0., 0.), sover = mk(0., 0., 0.);
        if (counted) {
            const V3 spoint = vadd(over, vmul(dir, sbest)); // Ray::position vec.rs:207-209
            snormal = shape_normal(S2, m2, spoint);
            if (vdot(snormal, seye) < 0.0) snormal = vneg(snormal);
            sover = vadd(spoint, vmul(snormal, RTC_EPSILON));
        }

        // 3. surface = lighting(L[0]) + lighting(L[1]) + ..., in light order, each with its own is_shadowed_by_light
        auto one_light = [&](V3 lp, const auto &I) {
            V3 ldir = mk(0., 0., 0.);
            double ldist = 0.;
            shadow_ray(lp, sover, counted, ldir, ldist);
            bool pending = counted, shadowed = false;
            Bundle Bl{};
            Bl.off = true;
            if constexpr (IS_CULL(SRC)) { // the segment over_point -> light, walked from the light: apex = light (shared), reach-limited
                if (ballot(counted) != 0ull) Bl = make_bundle<true, true>(counted, lp, lp, vneg(ldir), ldist);
            }
            for_each_object<SRC, SRC == SRC_CULL2>(A, T, L, pending, Bl, AnyHit{pending, sover, ldir, ldist, shadowed}, sover, ldir);
            asm volatile("" ::: "memory"); // as k_trace's light loop: the material loads stay below the walk
            V3 term = mk(0., 0., 0.);
            if (counted) term = lighting(I, S2, m2, sover, seye, snormal, ldir, shadowed);
            return term;
        };
        V3 surface = one_light(mk(A.light_pos[0], A.light_pos[1], A.light_pos[2]), A);
        if constexpr (LIGHT_BLOCKS == 1) {
            const auto &X = first_of(xl_arg...); // DevExtraLights (kernel arguments) or DevLightTable (HBM)
            const uint32_t n_extra = further_light_count(X);
            for (uint32_t li = 0; li < n_extra; ++li) surface = vadd(surface, one_light(further_light_position(X, li), further_light_intensity(X, li)));
        }

        // 4. the sum, in sample order
        acc = vadd(acc, surface);
    }

    // ---- the planes asked for (wave-uniform choice), one pixel per lane: plain vector stores ----
    V3 rad = mk(0.0, 0.0, 0.0);
    if (hit) rad = mk(rtc_gather_mean(acc.x, ns), rtc_gather_mean(acc.y, ns), rtc_gather_mean(acc.z, ns));
    const size_t idx = (size_t)py * A.W + px;
    if (A.radiance != nullptr && in_range) {
        A.radiance[3u * idx] = rad.x; A.radiance[3u * idx + 1u] = rad.y; A.radiance[3u * idx + 2u] = rad.z;
    }
    if (A.bounce != nullptr) {
        V3 out = mk(0.0, 0.0, 0.0);
        if (hit) { // `base` as lighting() takes it for the primary hit: the pattern colour at over_point, or the material's colour
            const DevShade *S = T.shade + hidx;
            const V3 base = (S->pattern_kind != RTC_PATTERN_NONE) ? pattern_color(S, T.isect[hidx].m, over) : mk(S->color[0], S->color[1], S->color[2]);
            const double kd = S->diffuse;
            out = mk(rtc_gather_bounce(base.x * kd, rad.x), rtc_gather_bounce(base.y * kd, rad.y), rtc_gather_bounce(base.z * kd, rad.z));
        }
        if (in_range) { A.bounce[3u * idx] = out.x; A.bounce[3u * idx + 1u] = out.y; A.bounce[3u * idx + 2u] = out.z; }
    }
}

// rtc_canvas_add_scaled on the device: one thread per pixel, rtc_gather.h's sum
__global__ void __launch_bounds__(256) k_add_scaled(double *__restrict__ rgb, const double *__restrict__ plane, size_t n, double strength) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    rgb[3u * i] = rtc_gather_add_scaled(rgb[3u * i], plane[3u * i], strength);
    rgb[3u * i + 1u] = rtc_gather_add_scaled(rgb[3u * i + 1u], plane[3u * i + 1u], strength);
    rgb[3u * i + 2u] = rtc_gather_add_scaled(rgb[3u * i + 2u], plane[3u * i + 2u], strength);
}

// ---- launch dispatch (rtc_launch_aov, rtc_launch_trace) -----------------------------------------------------------
// The runtime `src` as a compile-time constant: f(std::integral_constant<int, SRC_x>) for the one of `ALLOWED` it equals.
template <int... ALLOWED, class F> static hipError_t with_src(int src, F &&f) {
    hipError_t e = hipErrorInvalidValue; // (a source the launch does not take)
    (void)(... || (src == ALLOWED && ((e = f(std::integral_constant<int, ALLOWED>{})), true)));
    return e;
}
// A World's further lights as the kernel's trailing argument: f() for one light, f(*xl) for the kernel-argument block,
// f(*lt) for the device table (never both).
template <class F> static hipError_t with_further_lights(const DevExtraLights *xl, const DevLightTable *lt, F &&f) {
    if (xl != nullptr && lt != nullptr) return hipErrorInvalidValue;
    if (xl != nullptr && (xl->n == 0u || xl->n > RTC_MAX_LIGHTS - 1u)) return hipErrorInvalidValue;
    if (lt != nullptr && (lt->rec == nullptr || lt->n == 0u || lt->n > RTC_MAX_LIGHT_SAMPLES - 1u)) return hipErrorInvalidValue;
    if (xl != nullptr) return f(*xl);
    if (lt != nullptr) return f(*lt);
    return f();
}

// A tile pass's workgroups, one per 8x8 tile; 0 for a block whose size and tiles_x do not hold together.
static uint32_t tile_count(const TileParams &A) {
    if (A.W == 0u || A.H == 0u || A.tiles_x != (A.W + 7u) / 8u) return 0u;
    const unsigned long long tiles64 = (unsigned long long)A.tiles_x * ((A.H + 7u) / 8u);
    return tiles64 > 0x7fffffffull ? 0u : (uint32_t)tiles64;
}
// The World's eleven tables as a tile pass's kernel arguments, in tile_tables' order: f(isect, kind, ..., pre_s).
template <class F> static hipError_t with_tables(const RenderParams &P, F &&f) {
    return f(P.isect, P.kind, P.shade, P.bound, P.isect_s, P.kind_s, P.bound_s, P.orig_s, P.gbound, P.pre, P.pre_s);
}

// A tile pass's projection as the kernel's last argument: f() for a pinhole launch (proj == NULL), f(*proj) for an
// orthographic or panorama one — rtc_launch_trace's checks: a known kind, and both tables for a panorama (they hold the
// pass's W and H entries: the host's pano_tables).
template <class F> static hipError_t with_projection(const DevProjection *proj, F &&f) {
    if (proj == nullptr) return f();
    if (proj->kind != RTC_PROJ_ORTHOGRAPHIC && (proj->kind != RTC_PROJ_PANORAMA || proj->col == nullptr || proj->row == nullptr))
        return hipErrorInvalidValue;
    return f(*proj);
}

// `P`: the World's tables only (fill_world). `xl` / `lt` (never both): the further lights of a World with several, read only when
// A->shadow is set. src: SRC_SMEM, SRC_CULL or SRC_CULL2. `proj`: NULL, or the projection whose rays the pass casts.
extern "C" hipError_t rtc_launch_aov(const AovParams *A, const RenderParams *P, int src, const DevExtraLights *xl, const DevLightTable *lt,
                                     const DevProjection *proj, hipStream_t stream) {
    const uint32_t tiles = tile_count(*A);
    if (tiles == 0u) return hipErrorInvalidValue;
    return with_projection(proj, [&](const auto &...pj) {
        return with_further_lights(xl, lt, [&](const auto &...x) {
            return with_src<SRC_SMEM, SRC_CULL, SRC_CULL2>(src, [&](auto S) {
                return with_tables(*P, [&](auto... t) {
                    if (A->shadow == nullptr) // no shadow rays: the further lights are not read
                        hipLaunchKernelGGL((k_aov<S(), false, std::decay_t<decltype(pj)>...>), dim3(tiles), dim3(64), 0, stream, *A, t..., pj...);
                    else
                        hipLaunchKernelGGL((k_aov<S(), true, std::decay_t<decltype(x)>..., std::decay_t<decltype(pj)>...>), dim3(tiles), dim3(64), 0, stream, *A, t..., x..., pj...);
                    return hipGetLastError();
                });
            });
        });
    });
}

extern "C" hipError_t rtc_launch_aov_view(const AovViewParams *V, hipStream_t stream) {
    if (V->n == 0) return hipSuccess;
    const size_t blocks = (V->n + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_aov_view, dim3((uint32_t)blocks), dim3(256), 0, stream, *V);
    return hipGetLastError();
}

// `P`: the World's tables only (fill_world). `dirs`: A->nsamples directions in device memory. src: SRC_SMEM, SRC_CULL or SRC_CULL2.
// `proj`: as rtc_launch_aov's.
extern "C" hipError_t rtc_launch_ao(const AoParams *A, const double *dirs, const RenderParams *P, int src, const DevProjection *proj,
                                    hipStream_t stream) {
    const uint32_t tiles = tile_count(*A);
    if (tiles == 0u || A->out == nullptr || dirs == nullptr) return hipErrorInvalidValue;
    if (A->nsamples == 0u || A->nsamples > RTC_MAX_AO_SAMPLES) return hipErrorInvalidValue;
    return with_projection(proj, [&](const auto &...pj) {
        return with_src<SRC_SMEM, SRC_CULL, SRC_CULL2>(src, [&](auto S) {
            return with_tables(*P, [&](auto... t) {
                hipLaunchKernelGGL((k_ao<S(), std::decay_t<decltype(pj)>...>), dim3(tiles), dim3(64), 0, stream, *A, dirs, t..., pj...);
                return hipGetLastError();
            });
        });
    });
}

extern "C" hipError_t rtc_launch_apply_ao(double *rgb, const uint16_t *ao, size_t n, uint32_t n_samples, double strength, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apply_ao, dim3((uint32_t)blocks), dim3(256), 0, stream, rgb, ao, n, n_samples, strength);
    return hipGetLastError();
}

// `P`: the World's tables only (fill_world). `dirs`: A->nsamples directions in device memory. `xl` / `lt` (never both): the
// further lights of a World with several. src: SRC_SMEM, SRC_CULL or SRC_CULL2. `proj`: as rtc_launch_aov's.
extern "C" hipError_t rtc_launch_gather(const GatherParams *A, const double *dirs, const RenderParams *P, int src, const DevExtraLights *xl,
                                        const DevLightTable *lt, const DevProjection *proj, hipStream_t stream) {
    const uint32_t tiles = tile_count(*A);
    if (tiles == 0u || (A->radiance == nullptr && A->bounce == nullptr) || dirs == nullptr) return hipErrorInvalidValue;
    if (A->nsamples == 0u || A->nsamples > RTC_MAX_AO_SAMPLES) return hipErrorInvalidValue;
    return with_projection(proj, [&](const auto &...pj) {
        return with_further_lights(xl, lt, [&](const auto &...x) {
            return with_src<SRC_SMEM, SRC_CULL, SRC_CULL2>(src, [&](auto S) {
                return with_tables(*P, [&](auto... t) {
                    hipLaunchKernelGGL((k_gather<S(), std::decay_t<decltype(x)>..., std::decay_t<decltype(pj)>...>), dim3(tiles), dim3(64), 0, stream, *A, dirs, t..., x..., pj...);
                    return hipGetLastError();
                });
            });
        });
    });
}

extern "C" hipError_t rtc_launch_add_scaled(double *rgb, const double *plane, size_t n, double strength, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_add_scaled, dim3((uint32_t)blocks), dim3(256), 0, stream, rgb, plane, n, strength);
    return hipGetLastError();
}

// ---- launchers (called from rtc_api.cpp) --------------------------------------------------
// XL: nothing (one light), or the World's further lights (k_trace's trailing argument)
template <int SRC, bool REFL, bool REFR, bool PROBE, bool RGBA, bool ONE, bool WHOLE = false, class... XL>
static hipError_t launch_kernel(const RenderParams &P, dim3 grid, size_t lds_bytes, hipStream_t stream, hipEvent_t e0,
                                hipEvent_t e1, const XL &...xl) {
    if (lds_bytes > 48 * 1024) { // more dynamic LDS than the default limit: opt in (up to 160 KiB per CU on gfx950)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_trace<SRC, REFL, REFR, PROBE, RGBA, ONE, WHOLE, XL...>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    // e0/e1 (may be NULL) receive the dispatch's own begin/end timestamps: no marker packets on the stream
    hipExtLaunchKernelGGL((k_trace<SRC, REFL, REFR, PROBE, RGBA, ONE, WHOLE, XL...>), grid, dim3(RTC_BLOCK_FOR(CULL_LEVEL(SRC), REFL, REFR, PROBE)), lds_bytes, stream, e0, e1, 0, P, P.isect,
                          P.kind, P.shade, P.prim, P.bound, P.isect_s, P.kind_s, P.bound_s, P.orig_s, P.gbound, P.idtab, P.pre, P.pre_s, xl...);
    return hipGetLastError();
}
// The kernels the whole-tile flavour (WHOLE) is instantiated for: the culled sources' flat, reflective and refractive kernels,
// one light, f64 output — without the flat two-level one, which comes out with 95 VGPRs against its one-sample twin's 94
//  and stays on that twin.
static constexpr bool whole_tile_kernel(int src, bool refl) { return IS_CULL(src) && !(src == SRC_CULL2 && !refl); }
// What the flavour assumes of a launch, in one place: launch_one asks here and nowhere else, with the very parameter block
// the kernel reads. `src`, `refl`, `refr`: the kernel that would run; `further_lights`: the World has more than one light (a
// DevExtraLights or DevLightTable rides behind the tables).
//   - the one-sample flavour's own conditions: a culled source, a render (not a probe) launch, one ray per pixel;
//   - one light, no gamma table, an f64 canvas (16-byte aligned) and no 8-bit output: the output stage is the 16-byte form;
//   - one view, contiguous rows (band_stride 1), RTC_MODE_RENDER_ASYNC (Camera::render leaves a row and a column untraced);
//   - whole tiles only: W a multiple of the tile's width, rows [y0, y1) on tile-row boundaries and inside the canvas, and a
//     grid that is exactly those tiles — every lane of every workgroup is in range and traced, every tile row is whole;
//   - tile lists, where the launch has them, laid out for exactly this image: every tile of the launch has a list.
static bool whole_tile_launch(const RenderParams &P, int src, bool refl, bool refr, bool further_lights) {
    if (!whole_tile_kernel(src, refl) || P.rays != nullptr || P.samples != 1u) return false;
    const uint32_t tile_w = RTC_TILE_W_FOR(CULL_LEVEL(src), refl, refr, false); // the pixels a workgroup's tile is wide
    if (further_lights || P.gamma != nullptr || P.out8 != nullptr) return false;
    if (P.out == nullptr || ((size_t)P.out % 16u) != 0) return false;
    if (P.nviews != 1u || P.band_stride != 1u || P.mode != RTC_MODE_RENDER_ASYNC) return false;
    if (P.W == 0u || P.W % tile_w != 0u || P.y1 <= P.y0 || P.y1 > P.H || P.y0 % 8u != 0u || (P.y1 - P.y0) % 8u != 0u) return false;
    if (P.tile_cnt != nullptr && (P.tiles_x != P.W / 8u || (unsigned long long)P.tiles_y * 8u < P.y1)) return false;
    return P.grid_x == P.W / tile_w && P.grid_y == (P.y1 - P.y0) / 8u;
}
// Test hook (not in include/rtc.h): whole_tile_launch of a parameter block with these fields, for the kernel a World with
// these flavours would run (tests/test_host_whole_tile.py). Pointers are given as addresses; none is dereferenced.
struct WholeTileQuery {
    uint64_t out, out8, gamma, rays, tile_cnt;
    uint32_t samples, nviews, band_stride, mode, W, H, y0, y1, grid_x, grid_y, tiles_x, tiles_y;
    int32_t src;
    uint32_t refl, refr, further_lights;
};
extern "C" int rtc_debug_whole_tile_launch(const WholeTileQuery *q) {
    if (q == nullptr) return -1;
    RenderParams P{};
    P.out = reinterpret_cast<double *>((uintptr_t)q->out);
    P.out8 = reinterpret_cast<unsigned char *>((uintptr_t)q->out8);
    P.gamma = reinterpret_cast<const DevGamma *>((uintptr_t)q->gamma);
    P.rays = reinterpret_cast<const double *>((uintptr_t)q->rays);
    P.tile_cnt = reinterpret_cast<const uint32_t *>((uintptr_t)q->tile_cnt);
    P.tiles_x = q->tiles_x; P.tiles_y = q->tiles_y;
    P.samples = q->samples; P.nviews = q->nviews; P.band_stride = q->band_stride; P.mode = q->mode;
    P.W = q->W; P.H = q->H; P.y0 = q->y0; P.y1 = q->y1; P.grid_x = q->grid_x; P.grid_y = q->grid_y;
    return whole_tile_launch(P, q->src, q->refl != 0u, q->refr != 0u, q->further_lights != 0u) ? 1 : 0;
}

// `one_sample`: a render launch of a camera with samples == 1 takes the one-sample instantiation (ONE), which exists for the
// product sources SRC_CULL and SRC_CULL2 only; the measurement-only sources keep the generic kernel.
// `whole_tiles`: such a launch of one light for which whole_tile_launch holds takes the whole-tile instantiation (WHOLE) on top.
// `uniform_shade`: false sends a launch whose kernel has the uniform shading path (trace_uniform_shade) to that kernel's
// per-lane twin, the same template with DevPerLaneShade as its trailing argument.
template <int SRC, bool REFL, bool REFR, class... XL>
static hipError_t launch_one(const RenderParams &P, bool one_sample, bool whole_tiles, bool uniform_shade, dim3 grid, size_t lds_bytes,
                             hipStream_t stream, hipEvent_t e0, hipEvent_t e1, const XL &...xl) {
    if (P.rays != nullptr) return launch_kernel<SRC, REFL, REFR, true, false, false>(P, grid, lds_bytes, stream, e0, e1, xl...);
    if constexpr (IS_CULL(SRC)) {
        if (one_sample && P.samples == 1u) {
            if constexpr (trace_uniform_shade(SRC, REFL, true, sizeof...(XL) != 0)) {
                if (!uniform_shade) {
                    const DevPerLaneShade tag{0u};
                    if constexpr (whole_tile_kernel(SRC, REFL)) {
                        if (whole_tiles && whole_tile_launch(P, SRC, REFL, REFR, false))
                            return launch_kernel<SRC, REFL, REFR, false, false, true, true>(P, grid, lds_bytes, stream, e0, e1, tag);
                    }
                    if (P.gamma != nullptr) return launch_kernel<SRC, REFL, REFR, false, true, true>(P, grid, lds_bytes, stream, e0, e1, tag);
                    return launch_kernel<SRC, REFL, REFR, false, false, true>(P, grid, lds_bytes, stream, e0, e1, tag);
                }
            }
            if constexpr (sizeof...(XL) == 0 && whole_tile_kernel(SRC, REFL)) {
                if (whole_tiles && whole_tile_launch(P, SRC, REFL, REFR, false))
                    return launch_kernel<SRC, REFL, REFR, false, false, true, true>(P, grid, lds_bytes, stream, e0, e1);
            }
            if (P.gamma != nullptr) return launch_kernel<SRC, REFL, REFR, false, true, true>(P, grid, lds_bytes, stream, e0, e1, xl...);
            return launch_kernel<SRC, REFL, REFR, false, false, true>(P, grid, lds_bytes, stream, e0, e1, xl...);
        }
    }
    if (P.gamma != nullptr) return launch_kernel<SRC, REFL, REFR, false, true, false>(P, grid, lds_bytes, stream, e0, e1, xl...);
    return launch_kernel<SRC, REFL, REFR, false, false, false>(P, grid, lds_bytes, stream, e0, e1, xl...);
}

// `xl`: NULL for a World with one light; else its lights 1..n-1 (xl->n >= 1), and src one of SRC_SMEM, SRC_CULL, SRC_CULL2.
// `lt` (instead of `xl`, never both): the same lights as a device table (lt->rec holds lt->n records, rtc_device.h).
// `lens`: non-NULL for a thin-lens launch (render flavour, src one of SRC_SMEM, SRC_CULL, SRC_CULL2, no gamma table).
// `proj`: non-NULL for a projection launch, under the same conditions; a panorama's tables hold P->W and P->H entries. Never both.
// `one_sample`: non-zero lets a pinhole render launch with P->samples == 1 take the one-sample instantiation (the context's
// RTC_ONE_SAMPLE switch); zero keeps every launch on the generic kernel.
// `whole_tiles`: non-zero lets such a launch take the whole-tile instantiation where it qualifies (whole_tile_launch; the
// context's RTC_WHOLE_TILES switch); zero, or one_sample zero, keeps every launch on the kernels it had without the flavour.
// `uniform_shade`: zero keeps every launch off the uniform shading path (the context's RTC_UNIFORM_SHADE switch).
extern "C" hipError_t rtc_launch_trace(const RenderParams *P, int src, int refl, int refr, uint32_t nblocks,
                                       size_t lds_bytes, hipStream_t stream, hipEvent_t e0, hipEvent_t e1, const DevExtraLights *xl,
                                       const DevLightTable *lt, const DevLens *lens, const DevProjection *proj, int one_sample,
                                       int whole_tiles, int uniform_shade) {
    const dim3 grid(nblocks);
    // the recursion flavour: refractive Worlds carry the full frame stack, reflective ones the LDS stack, the others none
    auto with_depth = [&](auto &&launch) {
        if (refr) return launch(std::true_type{}, std::true_type{});
        if (refl) return launch(std::true_type{}, std::false_type{});
        return launch(std::false_type{}, std::false_type{});
    };
    if (lens != nullptr && proj != nullptr) return hipErrorInvalidValue;
    return with_further_lights(xl, lt, [&](const auto &...x) {
        if (proj != nullptr) {
            if (P->rays != nullptr || P->gamma != nullptr || P->samples != 1u) return hipErrorInvalidValue;
            if (proj->kind != RTC_PROJ_ORTHOGRAPHIC && (proj->kind != RTC_PROJ_PANORAMA || proj->col == nullptr || proj->row == nullptr))
                return hipErrorInvalidValue;
            return with_src<SRC_SMEM, SRC_CULL, SRC_CULL2>(src, [&](auto S) {
                return with_depth([&](auto RL, auto RR) { return launch_kernel<S(), RL(), RR(), false, false, false>(*P, grid, lds_bytes, stream, e0, e1, x..., *proj); });
            });
        }
        if (lens != nullptr) {
            if (P->rays != nullptr || P->gamma != nullptr || P->samples != 1u || lens->usteps == 0u || lens->vsteps == 0u ||
                (unsigned long long)lens->usteps * lens->vsteps > RTC_MAX_LENS_SAMPLES)
                return hipErrorInvalidValue;
            return with_src<SRC_SMEM, SRC_CULL, SRC_CULL2>(src, [&](auto S) {
                return with_depth([&](auto RL, auto RR) { return launch_kernel<S(), RL(), RR(), false, false, false>(*P, grid, lds_bytes, stream, e0, e1, x..., *lens); });
            });
        }
        auto flavours = [&](auto S) {
            return with_depth([&](auto RL, auto RR) { return launch_one<S(), RL(), RR()>(*P, one_sample != 0, whole_tiles != 0, uniform_shade != 0, grid, lds_bytes, stream, e0, e1, x...); });
        };
        // the LDS-staged sources exist for one-light pinhole launches only
        if constexpr (sizeof...(x) == 0) return with_src<SRC_SMEM, SRC_LDS1, SRC_LDSN, SRC_CULL, SRC_CULL2>(src, flavours);
        else return with_src<SRC_SMEM, SRC_CULL, SRC_CULL2>(src, flavours);
    });
}

extern "C" hipError_t rtc_launch_prep(const DevIsect *isect, DevPrim *prim, uint32_t n, const double vinv[12],
                                      hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_prep_primary, dim3((n + 255u) / 256u), dim3(256), 0, stream, isect, prim,
                       n, vinv[0], vinv[1], vinv[2], vinv[3], vinv[4], vinv[5], vinv[6], vinv[7], vinv[8], vinv[9],
                       vinv[10], vinv[11]);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_arith(uint32_t op, const double *a, const double *b, uint32_t n, double *out,
                                       hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_arith, dim3((n + 255) / 256), dim3(256), 0, stream, op, a, b, n, out);
    return hipGetLastError();
}
