// rtc_jpeg.h — the per-block arithmetic of the JPEG writer (include/rtc.h), shared by its host statement (host_jpeg.cpp)
// and the device encoder (rtc_jpeg.hip) so the two cannot drift: the Annex K tables, the zigzag order, the colour
// conversion, the integer forward DCT, the quantiser, the magnitude category and the Huffman code of one coefficient.
// Only the assembly of the bitstream differs between them (serial on the host, scanned and scattered on the device).
// Not part of the ABI.
#ifndef RTC_JPEG_H
#define RTC_JPEG_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTC_JHD __host__ __device__ inline
#else
#define RTC_JHD inline
#endif

enum {
    RTC_JPEG_HEADER_BYTES = 623, // SOI .. SOS, fixed for every size and quality (host_jpeg.cpp rtc_jpeg_header)
    // worst-case entropy-coded bits of one 8x8 block: DC code <= 11 + magnitude <= 11, 63 AC codes of <= 16 + 10,
    // at most 3 ZRLs (the runs of a block sum to <= 62) of <= 11 bits, one EOB of <= 4 bits
    RTC_JPEG_BLOCK_BITS_MAX = 22 + 63 * 26 + 3 * 11 + 4,
};

// Annex K.1, natural (row-major) order
constexpr uint8_t kJpegStdQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// natural index of zigzag position k
constexpr uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3: code counts per length 1..16 and symbols, in the order DC0 (luma), AC0, DC1 (chroma), AC1
constexpr uint8_t kJpegDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kJpegDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kJpegAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kJpegAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// Canonical codes of the four tables: (code << 8) | length per symbol, 0 for a symbol the table lacks.
struct RtcJpegCodes {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr RtcJpegCodes rtc_jpeg_make_codes() {
    RtcJpegCodes t{};
    for (int c = 0; c < 2; ++c) {
        uint32_t code = 0, k = 0;
        for (int len = 1; len <= 16; ++len, code <<= 1)
            for (int i = 0; i < kJpegDcBits[c][len - 1]; ++i, ++code, ++k) t.dc[c][kJpegDcVals[k]] = (code << 8) | (uint32_t)len;
        code = 0;
        k = 0;
        for (int len = 1; len <= 16; ++len, code <<= 1)
            for (int i = 0; i < kJpegAcBits[c][len - 1]; ++i, ++code, ++k) t.ac[c][kJpegAcVals[c][k]] = (code << 8) | (uint32_t)len;
    }
    return t;
}
constexpr RtcJpegCodes kJpegCodes = rtc_jpeg_make_codes();

// libjpeg's quality scaling over the Annex K.1 tables; quality in 1..100
RTC_JHD uint32_t rtc_jpeg_quant_entry(int quality, int table, int i) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    int v = ((int)kJpegStdQuant[table][i] * s + 50) / 100;
    return (uint32_t)(v < 1 ? 1 : v > 255 ? 255 : v);
}

// Rust's `f as u8`: truncation toward zero, saturating (NaN -> 0)
RTC_JHD uint32_t rtc_jpeg_f32_to_u8(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 255.0f) return 255u;
    return (uint32_t)f;
}

// RGB -> YCbCr, f32: every coefficient is the f32 quotient below, products and sums in the order written (no contraction:
// the build passes -ffp-contract=off), then rtc_jpeg_f32_to_u8
RTC_JHD void rtc_jpeg_ycc(uint32_t r8, uint32_t g8, uint32_t b8, uint32_t ycc[3]) {
    const float r = (float)r8, g = (float)g8, b = (float)b8;
    const float yr = 76.245f / 255.0f, yg = 149.685f / 255.0f, yb = 29.07f / 255.0f;
    const float br = -43.0185f / 255.0f, bg = -84.4815f / 255.0f, bb = 127.5f / 255.0f;
    const float rr = 127.5f / 255.0f, rg = -106.7685f / 255.0f, rb = -20.7315f / 255.0f;
    ycc[0] = rtc_jpeg_f32_to_u8(yr * r + yg * g + yb * b);
    ycc[1] = rtc_jpeg_f32_to_u8(br * r + bg * g + bb * b + 128.0f);
    ycc[2] = rtc_jpeg_f32_to_u8(rr * r + rg * g + rb * b + 128.0f);
}

// One pass of the integer LLM forward DCT (libjpeg's ISLOW): CONST_BITS 13, PASS1_BITS 2, DESCALE(x, n) =
// (x + 2^(n-1)) >> n (arithmetic). `pass` 0 works on level-shifted samples and leaves its outputs scaled up by
// 2^PASS1_BITS; pass 1 removes that scaling. Eight values at d[0], d[stride], ..., d[7 * stride], in place.
RTC_JHD void rtc_jpeg_fdct_1d(int32_t *d, int stride, int pass) {
    constexpr int CB = 13, P1 = 2;
    const int sh = pass == 0 ? CB - P1 : CB + P1;
    auto descale = [](int32_t x, int n) -> int32_t { return (x + (1 << (n - 1))) >> n; };
    const int32_t x0 = d[0], x1 = d[stride], x2 = d[2 * stride], x3 = d[3 * stride], x4 = d[4 * stride], x5 = d[5 * stride],
                  x6 = d[6 * stride], x7 = d[7 * stride];
    const int32_t t0 = x0 + x7, t7 = x0 - x7, t1 = x1 + x6, t6 = x1 - x6, t2 = x2 + x5, t5 = x2 - x5, t3 = x3 + x4, t4 = x3 - x4;
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (pass == 0) {
        d[0] = (t10 + t11) * (1 << P1);
        d[4 * stride] = (t10 - t11) * (1 << P1);
    } else {
        d[0] = descale(t10 + t11, P1);
        d[4 * stride] = descale(t10 - t11, P1);
    }
    const int32_t z1 = (t12 + t13) * 4433;                // 0.541196100
    d[2 * stride] = descale(z1 + t13 * 6270, sh);         // 0.765366865
    d[6 * stride] = descale(z1 + t12 * -15137, sh);       // 1.847759065
    const int32_t z5 = (t4 + t6 + t5 + t7) * 9633;        // 1.175875602
    const int32_t z1o = (t4 + t7) * -7373;                // 0.899976223
    const int32_t z2o = (t5 + t6) * -20995;               // 2.562915447
    const int32_t z3o = (t4 + t6) * -16069 + z5;          // 1.961570560
    const int32_t z4o = (t5 + t7) * -3196 + z5;           // 0.390180644
    d[7 * stride] = descale(t4 * 2446 + z1o + z3o, sh);   // 0.298631336
    d[5 * stride] = descale(t5 * 16819 + z2o + z4o, sh);  // 2.053119869
    d[3 * stride] = descale(t6 * 25172 + z2o + z3o, sh);  // 3.072711026
    d[1 * stride] = descale(t7 * 12299 + z1o + z4o, sh);  // 1.501321110
}

// The whole 2-D DCT of 64 samples (natural order, 0..255): the rows, then the columns. Output scaled by 8.
RTC_JHD void rtc_jpeg_fdct_block(const uint32_t *samples, int32_t out[64]) {
    for (int i = 0; i < 64; ++i) out[i] = (int32_t)samples[i] - 128;
    for (int r = 0; r < 8; ++r) rtc_jpeg_fdct_1d(out + 8 * r, 1, 0);
    for (int c = 0; c < 8; ++c) rtc_jpeg_fdct_1d(out + c, 8, 1);
}

// round(trunc(d / 8) / q), half away from zero, in integers
RTC_JHD int32_t rtc_jpeg_quantise(int32_t d, int32_t q) {
    const int32_t t = d / 8, a = t < 0 ? -t : t;
    const int32_t m = (2 * a + q) / (2 * q);
    return t < 0 ? -m : m;
}

// bits of |v| (0 for v = 0)
RTC_JHD uint32_t rtc_jpeg_category(int32_t v) {
    uint32_t a = (uint32_t)(v < 0 ? -v : v), n = 0;
    while (a) { ++n; a >>= 1; }
    return n;
}

// the `n` magnitude bits of v: v itself when positive, v - 1 (one's complement) when negative
RTC_JHD uint32_t rtc_jpeg_magnitude(int32_t v, uint32_t n) {
    return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
}

// DC difference -> (code, length): Huffman code of its category, then the magnitude bits. At most 22 bits.
RTC_JHD uint32_t rtc_jpeg_dc_code(int chroma, int32_t diff, uint64_t *code) {
    const uint32_t n = rtc_jpeg_category(diff), h = kJpegCodes.dc[chroma][n], hl = h & 255u;
    *code = ((uint64_t)(h >> 8) << n) | rtc_jpeg_magnitude(diff, n);
    return hl + n;
}

// A non-zero AC coefficient v after `run` zeros -> (code, length): run / 16 ZRLs, the code of (run % 16, category), the
// magnitude bits. At most 3 * 11 + 16 + 10 = 59 bits.
RTC_JHD uint32_t rtc_jpeg_ac_code(int chroma, uint32_t run, int32_t v, uint64_t *code) {
    const uint32_t zrl = kJpegCodes.ac[chroma][0xF0], zl = zrl & 255u;
    uint64_t c = 0;
    uint32_t len = 0;
    for (uint32_t k = 0; k < (run >> 4); ++k) { c = (c << zl) | (zrl >> 8); len += zl; }
    const uint32_t n = rtc_jpeg_category(v), h = kJpegCodes.ac[chroma][((run & 15u) << 4) | n], hl = h & 255u;
    c = (c << hl) | (h >> 8);
    c = (c << n) | rtc_jpeg_magnitude(v, n);
    *code = c;
    return len + hl + n;
}

// end of block -> (code, length)
RTC_JHD uint32_t rtc_jpeg_eob_code(int chroma, uint64_t *code) {
    const uint32_t h = kJpegCodes.ac[chroma][0];
    *code = h >> 8;
    return h & 255u;
}

// SOI .. SOS of a width x height file at `quality` (RTC_JPEG_HEADER_BYTES bytes): the part of the file the host writes
extern "C" void rtc_jpeg_header(uint32_t width, uint32_t height, int32_t quality, uint8_t *hdr);

#endif
