// rtc_float.h — the float file writers' conversions and layouts (Radiance HDR, PFM, OpenEXR; the rules are in
// include/rtc.h), shared by their host statement (host_float.cpp) and the device chain (rtc_float.hip). Not part of the ABI.
//
// The conversions are the ONE definition of both sides, in the manner of rtc_parity.h and rtc_gamma.h: integer arithmetic
// on the f64's bits and f64 comparisons only, so host and device give the same bits for every input. No hardware
// conversion is used: v_cvt_f32_f64 keeps a NaN's payload, and f64 -> f16 through f32 rounds twice.
#ifndef RTC_FLOAT_H
#define RTC_FLOAT_H

#include <cstddef>
#include <cstdint>

#include "rtc.h"

#if defined(__HIPCC__)
#define RTC_FHD __host__ __device__ inline
#else
#define RTC_FHD inline
#endif

RTC_FHD uint64_t rtc_f64_bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}

// x rounded to nearest, ties to even, into a binary format of `mant` stored mantissa bits and exponent bias `bias` whose
// all-ones exponent field is `emax` (f32: 23, 127, 255; f16: 10, 15, 31), returned as its bits. Subnormals are kept,
// overflow gives +-inf, any NaN gives `qnan`. x = sig * 2^(E - 52) with the 53-bit sig; the target keeps sig's top
// mant + 1 bits when it is normal there and fewer when it is subnormal (one bit less per exponent step below the smallest
// normal), the dropped bits decide the rounding, and a carry out of the mantissa runs into the exponent field, which is
// what IEEE asks for (all-ones mantissa + 1 = the next power of two; the largest normal + 1 = inf).
RTC_FHD uint32_t rtc_f64_round_bits(double x, int mant, int bias, int emax, uint32_t qnan) {
    const uint64_t u = rtc_f64_bits(x);
    const uint32_t sign = (uint32_t)(u >> 63) << (mant + (emax == 255 ? 8 : 5));
    const int e = (int)((u >> 52) & 0x7ffu);
    const uint64_t m = u & 0xfffffffffffffull;
    const uint32_t inf = (uint32_t)emax << mant;
    if (e == 0x7ff) return m ? qnan : (sign | inf);
    if (e == 0) return sign; // +-0 and the f64 subnormals: below half of either target's smallest subnormal
    const uint64_t sig = m | (1ull << 52);
    int te = e - 1023 + bias; // the target's exponent field if x is normal there
    if (te >= emax) return sign | inf;
    int shift = 52 - mant;
    if (te < 1) {
        shift += 1 - te;
        te = 0;
        if (shift > 63) shift = 63; // sig < 2^53: the quotient is 0 and the rest below half either way
    }
    uint64_t q = sig >> shift;
    const uint64_t rest = sig & ((1ull << shift) - 1ull), half = 1ull << (shift - 1);
    if (rest > half || (rest == half && (q & 1ull))) ++q;
    // normal: q carries the implicit bit (1 << mant), so (te - 1) << mant plus q is te's field over the mantissa
    return sign | ((te ? (uint32_t)(te - 1) << mant : 0u) + (uint32_t)q);
}

RTC_FHD uint32_t rtc_f64_to_f32_bits(double x) { return rtc_f64_round_bits(x, 23, 127, 255, 0x7FC00000u); }
RTC_FHD uint32_t rtc_f64_to_f16_bits(double x) { return rtc_f64_round_bits(x, 10, 15, 31, 0x7E00u); }

// Ward's float2rgbe, made exact: the pixel's R, G, B, E bytes as R | G << 8 | B << 16 | E << 24. A component is first
// mapped (NaN or < 0 -> 0, above 0x1.FEp+126 -> 0x1.FEp+126, the largest value RGBE holds); v is the largest mapped
// component; v < 1e-32 is 0,0,0,0; otherwise frexp(v) = (m, e), byte c = floor(ldexp(comp_c, 8 - e)), E = e + 128. v is a
// normal f64 here, so e is its exponent field - 1022, and floor(comp * 2^(8 - e)) is comp's 53-bit sig shifted right: no
// rounding anywhere. comp <= v < 2^e, so a byte is at most 255; a component whose shift leaves nothing is 0.
RTC_FHD uint32_t rtc_rgbe_bits(double r, double g, double b) {
    const double top = 0x1.FEp+126;
    const double c[3] = {r > 0.0 ? (r > top ? top : r) : 0.0, g > 0.0 ? (g > top ? top : g) : 0.0, b > 0.0 ? (b > top ? top : b) : 0.0};
    const double v = c[0] > c[1] ? (c[0] > c[2] ? c[0] : c[2]) : (c[1] > c[2] ? c[1] : c[2]);
    if (v < 1e-32) return 0u;
    const int e = (int)((rtc_f64_bits(v) >> 52) & 0x7ffu) - 1022;
    uint32_t out = (uint32_t)(e + 128) << 24;
    for (int k = 0; k < 3; ++k) {
        const uint64_t u = rtc_f64_bits(c[k]);
        const int ec = (int)((u >> 52) & 0x7ffu); // 0: zero or subnormal, nothing left beside v >= 1e-32
        const int shift = 44 + e - (ec - 1023);   // sig * 2^(ec - 1023 - 52) * 2^(8 - e), floored
        if (ec != 0 && shift <= 52) out |= (uint32_t)(((u & 0xfffffffffffffull) | (1ull << 52)) >> shift) << (8 * k);
    }
    return out;
}

// ---- the layouts ------------------------------------------------------------------------------------------------------

// A row-plane of the RLE form never exceeds w + ceil(w / 128) bytes: a literal token costs 1 byte per 128, and a run token
// (2 bytes) stands for at least 4.
inline unsigned long long rtc_hdr_plane_max(uint32_t w) { return (unsigned long long)w + (w + 127u) / 128u; }
inline bool rtc_hdr_is_rle(uint32_t w) { return w >= 8u && w <= 32767u; }

// One channel of an EXR file, in chlist order.
struct RtcExrChannel {
    const void *src;  // the plane (host or device)
    uint32_t stride;  // elements per pixel of the plane (1 or 3)
    uint32_t comp;    // which of them
    uint32_t source;  // RTC_EXR_SRC_*
    uint32_t type;    // the file's pixel type: 0 UINT, 1 HALF, 2 FLOAT
};
enum { RTC_EXR_SRC_F64 = 0, RTC_EXR_SRC_INDEX = 1, RTC_EXR_SRC_SHADOW = 2, RTC_EXR_MAX_CHANNELS = 12 };

// The value of channel c at pixel idx as the file stores it (HALF in the low 16 bits).
RTC_FHD uint32_t rtc_exr_value(const RtcExrChannel &c, size_t idx) {
    if (c.source == RTC_EXR_SRC_INDEX) return (uint32_t)static_cast<const int32_t *>(c.src)[idx] + 1u; // -1, a miss, is 0
    if (c.source == RTC_EXR_SRC_SHADOW) return static_cast<const uint16_t *>(c.src)[idx];
    const double v = static_cast<const double *>(c.src)[idx * c.stride + c.comp];
    return c.type == 1u ? rtc_f64_to_f16_bits(v) : rtc_f64_to_f32_bits(v);
}

// What host and device agree on about one file: `header` bytes computed on the host (PFM, HDR: the text; EXR: magic,
// attributes and the offset table), then the pixels.
struct RtcFloatLayout {
    uint32_t header = 0;
    uint32_t n_channels = 0;      // EXR
    uint32_t pixel_bytes = 0;     // EXR: bytes of one pixel over all channels; PFM 12; HDR 4
    unsigned long long file_bytes = 0; // PFM, EXR, flat HDR: the file; RLE HDR: its worst case (the exact `cap`)
    RtcExrChannel ch[RTC_EXR_MAX_CHANNELS];
    uint32_t ch_off[RTC_EXR_MAX_CHANNELS + 1]; // EXR: byte offset of channel c's values in a scanline of width 1
};

// The layout of `format` for these planes; false on arguments the format does not take. `hdr` (may be null) receives the
// L->header bytes.
bool rtc_float_layout(uint32_t format, const rtc_float_planes *p, uint32_t width, uint32_t height, RtcFloatLayout *L, uint8_t *hdr);
// true when `format` exists and takes a width x height frame
bool rtc_float_size_ok(uint32_t format, uint32_t width, uint32_t height);

#endif
