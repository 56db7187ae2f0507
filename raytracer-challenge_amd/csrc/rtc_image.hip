// rtc_image.hip — [device] the packed files of the save-by-name writer of include/rtc.h on gfx950 for a frame already in
// device memory (rtc_encode.h). host_image.cpp states the same bytes on the host; the layouts of both are rtc_image_layout.
//
//   k_image_pack   BMP, TGA, TIFF, farbfeld, PAM (and the raw R,G,B / R,G,B,255 inputs of the PNG and GIF chains and of
//                  PPM): one thread per 16 bytes of the FILE, so every store is one aligned 16-byte store and a wave writes
//                  1 KiB contiguously; a thread takes its bytes from the header (computed on the host, uploaded in front
//                  of the launch) or from the frame (row flipped for BMP, B and R swapped for BMP / TGA, each sample twice
//                  for farbfeld), walking pixel, row and channel from one division at its first byte
// PNG, JPEG, GIF and ICO are their chains with the header and trailer written on the host (rtc_encode.cpp); PPM is printed
// on the host from the R,G,B rows (k_image_pack's raw packing): 3 bytes per pixel cross PCIe instead of ~12.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rtc.h"
#include "rtc_encode.h"
#include "rtc_image.h"

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

constexpr uint32_t PACK_THREADS = 256;

struct PackArgs {
    const uint8_t *src;
    const uint8_t *hdr;
    uint8_t *out;
    unsigned long long *len;
    unsigned long long file_bytes;
    uint32_t w, h, channels, header, bpp, bgr, flip;
};

__global__ __launch_bounds__(PACK_THREADS) void k_image_pack(PackArgs a) {
    const unsigned long long p0 = 16ull * (blockIdx.x * (unsigned long long)PACK_THREADS + threadIdx.x);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.len = a.file_bytes;
    if (p0 >= a.file_bytes) return;
    uint32_t v[4] = {0, 0, 0, 0}; // the 16 bytes, little-endian in 4 words
    const unsigned long long b0 = p0 > a.header ? p0 - a.header : 0ull;
    unsigned long long pix = b0 / a.bpp;
    uint32_t c = (uint32_t)(b0 - pix * a.bpp);
    uint32_t y = (uint32_t)(pix / a.w), x = (uint32_t)(pix - (unsigned long long)y * a.w);
    const uint8_t *row = a.src + (size_t)(a.flip ? a.h - 1u - y : y) * a.w * a.channels;
    for (uint32_t k = 0; k < 16; ++k) {
        const unsigned long long p = p0 + k;
        uint32_t byte = 0;
        if (p < a.header) {
            byte = a.hdr[p];
        } else if (p < a.file_bytes) {
            const uint32_t comp = a.bpp == 8 ? c >> 1 : c; // farbfeld: v * 257 is the byte v twice
            const uint32_t ch = (a.bgr && comp != 1u && comp != 3u) ? 2u - comp : comp;
            byte = ch == 3u ? 255u : row[(size_t)x * a.channels + ch];
            if (++c == a.bpp) {
                c = 0;
                if (++x == a.w) {
                    x = 0;
                    ++y;
                    if (y < a.h) row = a.src + (size_t)(a.flip ? a.h - 1u - y : y) * a.w * a.channels;
                }
            }
        }
        v[k >> 2] |= byte << (8u * (k & 3u));
    }
    *reinterpret_cast<uint4 *>(a.out + p0) = make_uint4(v[0], v[1], v[2], v[3]);
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

} // namespace

// ---- host side ------------------------------------------------------------------------------------------------------

PackScratch::~PackScratch() {
    if (h_hdr) (void)hipHostFree(h_hdr);
}

// the header's device copy and its page-locked source
rtc_status PackScratch::header(size_t bytes) {
    if (bytes <= hdr_cap) return RTC_OK;
    if (h_hdr) (void)hipHostFree(h_hdr);
    h_hdr = nullptr;
    d_hdr.reset();
    hdr_cap = 0;
    const size_t b = std::max<size_t>(bytes, 4096);
    if (hipHostMalloc(reinterpret_cast<void **>(&h_hdr), b, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h_hdr = nullptr; return RTC_ERR_NOMEM; }
    const rtc_status st = d_hdr.reserve(b);
    if (st != RTC_OK) return st;
    hdr_cap = b;
    return RTC_OK;
}

// k_image_pack of `format` (a packed file or a raw packing) on `s`; the body is the file (RTC_IMAGE_RAW_*: the packed
// pixels), its length written by the kernel.
rtc_status rtc_image_pack_enqueue(PackScratch &sc, uint32_t format, const uint8_t *d_pixels, uint32_t w, uint32_t h, uint32_t channels,
                                  hipStream_t s, RtcEncoded *e) {
    rtc_status st = sc.d_len.reserve(1);
    if (st != RTC_OK) return st;
    RtcImageLayout L;
    if (!rtc_image_layout(format, w, h, &L, nullptr)) return RTC_ERR_ARG;
    st = sc.out.reserve(up16((size_t)L.file_bytes));
    if (st == RTC_OK) st = sc.header(L.header);
    if (st != RTC_OK) return st;
    if (L.header) {
        rtc_image_layout(format, w, h, &L, sc.h_hdr);
        HIP_TRY(hipMemcpyAsync(sc.d_hdr.get(), sc.h_hdr, L.header, hipMemcpyHostToDevice, s));
    }
    const unsigned long long threads = (L.file_bytes + 15) / 16;
    const PackArgs a{d_pixels, sc.d_hdr.get(), sc.out.get(), sc.d_len.get(), L.file_bytes, w, h, channels, L.header, L.bytes_per_pixel, L.bgr, L.flip};
    hipLaunchKernelGGL(k_image_pack, dim3((uint32_t)((threads + PACK_THREADS - 1) / PACK_THREADS)), dim3(PACK_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    e->d_body = sc.out.get();
    e->d_len = sc.d_len.get();
    e->cap = sc.out.capacity();
    e->min_len = 1;
    return RTC_OK;
}
