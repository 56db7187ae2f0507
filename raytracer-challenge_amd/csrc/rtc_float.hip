// rtc_float.hip — [device] the float file writers of include/rtc.h (Radiance HDR, PFM, OpenEXR) on gfx950 for an f64 canvas
// and AOV planes already in device memory (rtc_encode.h). host_float.cpp states the same bytes on the host; the
// conversions (rtc_float.h) are the same code on both sides, and rtc_float_layout gives both the same header.
//
//   k_float_pack   PFM, EXR and the flat form of HDR: one thread per 16 bytes of the FILE, as k_image_pack — every store one
//                  aligned 16-byte store; a thread takes its bytes from the header (text, or EXR's attributes and offset
//                  table; computed on the host, uploaded in front) or converts the elements they belong to, found by
//                  address arithmetic (PFM's row flip, EXR's planar scanlines): divisions for its first, a walk after. The file's length is known on the host.
//   RLE HDR (8 <= w <= 32767), a chain whose length exists only on the device:
//   k_hdr_planes   one thread per pixel: f64 -> R,G,B,E, stored as four byte planes per row (and the text header copied)
//   k_hdr_rle<0>   one wave per row-plane (4h independent problems of w bytes): the plane's coded size. The rule of
//                  include/rtc.h is defined on maximal runs, so everything a byte must know is local: it is in a run of
//                  four or more exactly when one of the four windows b[j..j+3] that cover it is constant (9 bytes around
//                  it), a segment (one long run, or one literal stretch) starts where that changes or a long run's byte
//                  changes, and the byte's place in its segment is its distance to the last start — a ballot and a count
//                  of leading zeros within the wave's 64 bytes, one carried index across them. Bytes of a run cost 2 at
//                  every 127th, literal bytes 1 and one more at every 128th; a wave scan of those is the byte's offset.
//   k_hdr_offsets  one workgroup: the scan over the 4h sizes (and the 4 marker bytes of every row), the markers, the length
//   k_hdr_rle<1>   the same walk again, now storing: a token's head is written by its LAST byte, which knows the count
// A row-plane never exceeds w + ceil(w / 128) bytes (rtc_hdr_plane_max), the buffer is sized from that, and every store of
// the chain is checked against it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rtc.h"
#include "rtc_encode.h"
#include "rtc_float.h"

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

constexpr uint32_t PACK_THREADS = 256;
constexpr uint32_t SCAN_THREADS = 1024;

struct FloatPackArgs {
    const uint8_t *hdr;
    uint8_t *out;
    unsigned long long *len;
    unsigned long long file_bytes;
    const double *rgb;
    const RtcExrChannel *ch; // EXR: the channels and ch_off, in device memory behind the header
    const uint32_t *ch_off;
    uint32_t format, w, h, header, pixel_bytes, n_channels;
};

// A walk over the body's elements (f32 / RGBE / i32 words, HALF values) in file order: one set of divisions finds the
// element that holds the thread's first body byte, every later one is the next in its row, channel or scanline.
struct Cursor {
    unsigned long long start; // the element's first byte in the body
    uint32_t size, value;
    unsigned long long y;     // PFM: row of the file; HDR: the pixel; EXR: scanline
    int c;                    // EXR: channel, -2 / -1 for the scanline's y and byte count
    uint32_t x;               // PFM: f32 within the row (0 .. 3w); EXR: pixel within the scanline
};

__device__ void load(const FloatPackArgs &a, Cursor &k) {
    k.size = 4;
    if (a.format == RTC_FLOAT_PFM) { // rows bottom to top
        k.value = rtc_f64_to_f32_bits(a.rgb[(a.h - 1ull - k.y) * 3ull * a.w + k.x]);
    } else if (a.format == RTC_FLOAT_HDR) { // flat R,G,B,E
        k.value = rtc_rgbe_bits(a.rgb[3 * k.y], a.rgb[3 * k.y + 1], a.rgb[3 * k.y + 2]);
    } else if (k.c < 0) { // i32 y, i32 bytes
        k.value = k.c == -2 ? (uint32_t)k.y : a.pixel_bytes * a.w;
    } else {
        const RtcExrChannel ch = a.ch[k.c];
        k.size = ch.type == 1u ? 2u : 4u;
        k.value = rtc_exr_value(ch, (size_t)(k.y * a.w + k.x));
    }
}

// the element that holds body byte b
__device__ void seek(const FloatPackArgs &a, Cursor &k, unsigned long long b) {
    k.c = 0;
    k.x = 0;
    if (a.format == RTC_FLOAT_PFM) {
        const unsigned long long e = b >> 2, per_row = 3ull * a.w;
        k.y = e / per_row;
        k.x = (uint32_t)(e - k.y * per_row);
        k.start = e << 2;
    } else if (a.format == RTC_FLOAT_HDR) {
        k.y = b >> 2;
        k.start = k.y << 2;
    } else {
        const unsigned long long line = 8ull + (unsigned long long)a.pixel_bytes * a.w;
        k.y = b / line;
        const unsigned long long r = b - k.y * line;
        if (r < 8) {
            k.c = r < 4 ? -2 : -1;
            k.start = b - (r & 3ull);
        } else {
            const unsigned long long d = r - 8;
            uint32_t c = 0;
            while (c + 1 < a.n_channels && d >= (unsigned long long)a.ch_off[c + 1] * a.w) ++c;
            const uint32_t sz = a.ch[c].type == 1u ? 2u : 4u;
            const unsigned long long in = d - (unsigned long long)a.ch_off[c] * a.w;
            k.c = (int)c;
            k.x = (uint32_t)(in / sz);
            k.start = b - (in - (unsigned long long)k.x * sz);
        }
    }
    load(a, k);
}

__device__ void next(const FloatPackArgs &a, Cursor &k) {
    k.start += k.size;
    if (a.format == RTC_FLOAT_PFM) {
        if (++k.x == 3u * a.w) {
            k.x = 0;
            ++k.y;
        }
    } else if (a.format == RTC_FLOAT_HDR) {
        ++k.y;
    } else if (k.c < 0) {
        ++k.c;
        k.x = 0;
    } else if (++k.x == a.w) {
        k.x = 0;
        if (++k.c == (int)a.n_channels) {
            k.c = -2;
            ++k.y;
        }
    }
    load(a, k);
}

__global__ __launch_bounds__(PACK_THREADS) void k_float_pack(FloatPackArgs a) {
    const unsigned long long p0 = 16ull * (blockIdx.x * (unsigned long long)PACK_THREADS + threadIdx.x);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.len = a.file_bytes;
    if (p0 >= a.file_bytes) return;
    uint32_t v[4] = {0, 0, 0, 0}; // the 16 bytes, little-endian in 4 words
    Cursor cur;
    cur.size = 0; // nothing yet
    for (uint32_t k = 0; k < 16; ++k) {
        const unsigned long long p = p0 + k;
        uint32_t byte = 0;
        if (p < a.header) {
            byte = a.hdr[p];
        } else if (p < a.file_bytes) { // (so an element is only ever loaded for a byte of the file: inside the planes)
            const unsigned long long b = p - a.header;
            if (cur.size == 0) seek(a, cur, b);
            else if (b - cur.start >= cur.size) next(a, cur);
            byte = (cur.value >> (8u * (uint32_t)(b - cur.start))) & 255u;
        }
        v[k >> 2] |= byte << (8u * (k & 3u));
    }
    *reinterpret_cast<uint4 *>(a.out + p0) = make_uint4(v[0], v[1], v[2], v[3]);
}

struct HdrArgs {
    const double *rgb;
    const uint8_t *hdr;
    uint8_t *planes;            // [h][4][w]
    uint32_t *sizes;            // [4h]
    unsigned long long *offs;   // [4h]: where each row-plane's tokens start in the file
    uint8_t *out;
    unsigned long long *len;
    unsigned long long cap;     // bytes of `out` the chain may write
    uint32_t w, h, header;
};

__global__ __launch_bounds__(PACK_THREADS) void k_hdr_planes(HdrArgs a) {
    const unsigned long long i = blockIdx.x * (unsigned long long)PACK_THREADS + threadIdx.x;
    if (i < a.header) a.out[i] = a.hdr[i];
    if (i >= (unsigned long long)a.w * a.h) return;
    const unsigned long long y = i / a.w, x = i - y * a.w;
    const uint32_t v = rtc_rgbe_bits(a.rgb[3 * i], a.rgb[3 * i + 1], a.rgb[3 * i + 2]);
    uint8_t *row = a.planes + y * 4ull * a.w + x;
    for (uint32_t c = 0; c < 4; ++c) row[(size_t)c * a.w] = (uint8_t)(v >> (8u * c));
}

__device__ inline uint32_t wave_scan_inclusive(uint32_t v, uint32_t lane) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

template <bool EMIT>
__global__ __launch_bounds__(PACK_THREADS) void k_hdr_rle(HdrArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long rp = blockIdx.x * (unsigned long long)(PACK_THREADS / 64u) + (threadIdx.x >> 6);
    if (rp >= 4ull * a.h) return; // the whole wave
    const uint8_t *b = a.planes + rp * a.w;
    const unsigned long long at = EMIT ? a.offs[rp] : 0ull;
    const int w = (int)a.w;
    int seg = 0;        // where the segment alive at this chunk's first byte started
    uint32_t total = 0; // coded bytes of the chunks before
    for (int base = 0; base < w; base += 64) {
        const int i = base + (int)lane;
        const bool active = i < w;
        // E bit t: b[j] == b[j + 1] for j = i - 4 + t, both inside the plane
        uint32_t E = 0, mine = 0;
        if (active) {
            uint32_t win[9];
            for (int t = 0; t < 9; ++t) {
                const int j = i - 4 + t;
                win[t] = (j >= 0 && j < w) ? b[j] : 256u + (uint32_t)t; // outside: equal to nothing
            }
            for (int t = 0; t < 8; ++t) E |= (uint32_t)(win[t] == win[t + 1]) << t;
            mine = win[4];
        }
        const uint32_t Q = E & (E >> 1) & (E >> 2); // bit t: b[j..j+3] constant for j = i - 4 + t
        const bool Lp = (Q & 0x0Fu) != 0, L = (Q & 0x1Eu) != 0, Ln = (Q & 0x3Cu) != 0; // in a run >= 4: bytes i-1, i, i+1
        const bool S = i == 0 || L != Lp || (L && !(E & 8u));                // a segment starts at i
        const bool Sn = i + 1 >= w || Ln != L || (Ln && !(E & 16u));         // ... at i + 1
        const unsigned long long starts = __ballot(active && S);
        const unsigned long long below = starts & (lane == 63u ? ~0ull : (2ull << lane) - 1ull);
        const int first = below ? base + 63 - __builtin_clzll(below) : seg;
        const uint32_t k = (uint32_t)(i - first); // the byte's place in its segment
        const uint32_t r = L ? k % 127u : k % 128u;
        const uint32_t cost = !active ? 0u : L ? (r == 0u ? 2u : 0u) : 1u + (r == 0u ? 1u : 0u);
        const uint32_t incl = wave_scan_inclusive(cost, lane);
        if (EMIT && active) {
            const unsigned long long P = at + total + incl - cost; // where this byte's cost starts
            if (L) {
                if (Sn || r == 126u) { // the token's last byte writes it
                    const unsigned long long pos = r == 0u ? P : P - 2ull;
                    if (pos + 1ull < a.cap) {
                        a.out[pos] = (uint8_t)(128u + r + 1u);
                        a.out[pos + 1] = (uint8_t)mine;
                    }
                }
            } else {
                const unsigned long long data = r == 0u ? P + 1ull : P;
                if (data < a.cap) a.out[data] = (uint8_t)mine;
                if (Sn || r == 127u) {
                    const unsigned long long pos = r == 0u ? P : P - 1ull - r;
                    if (pos < a.cap) a.out[pos] = (uint8_t)(r + 1u);
                }
            }
        }
        total += __shfl(incl, 63, 64);
        if (starts) seg = base + 63 - __builtin_clzll(starts);
    }
    if (!EMIT && lane == 0) a.sizes[rp] = total;
}

// offs[rp] = header + the markers and planes in front of it; the markers; the file's length
__global__ __launch_bounds__(SCAN_THREADS) void k_hdr_offsets(HdrArgs a) {
    __shared__ unsigned long long wave_total[SCAN_THREADS / 64];
    __shared__ unsigned long long running;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) running = a.header;
    __syncthreads();
    const unsigned long long n = 4ull * a.h;
    for (unsigned long long base = 0; base < n; base += SCAN_THREADS) {
        const unsigned long long rp = base + tid;
        const bool first = (rp & 3ull) == 0; // the row's marker stands in front of its R plane
        unsigned long long v = rp < n ? a.sizes[rp] + (first ? 4ull : 0ull) : 0ull;
        unsigned long long incl = v;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63u) wave_total[wave] = incl;
        __syncthreads();
        unsigned long long before = running;
        for (uint32_t k = 0; k < wave; ++k) before += wave_total[k];
        if (rp < n) {
            const unsigned long long pos = before + incl - v;
            if (first && pos + 3ull < a.cap) {
                a.out[pos] = 2;
                a.out[pos + 1] = 2;
                a.out[pos + 2] = (uint8_t)(a.w >> 8);
                a.out[pos + 3] = (uint8_t)a.w;
            }
            a.offs[rp] = pos + (first ? 4ull : 0ull);
        }
        __syncthreads();
        if (tid == SCAN_THREADS - 1) running = before + incl;
        __syncthreads();
    }
    if (tid == 0) *a.len = running;
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
size_t up8(size_t b) { return (b + 7) & ~(size_t)7; }

} // namespace

// ---- host side ------------------------------------------------------------------------------------------------------

// `format` of the planes at d (device pointers) on `s`. PFM, EXR and flat HDR: k_float_pack, the length known here. RLE
// HDR: the chain, the length on the device, cap the exact worst case.
rtc_status rtc_float_enqueue(FloatScratch &sc, uint32_t format, const rtc_float_planes *d, uint32_t w, uint32_t h, hipStream_t s,
                             RtcEncoded *e) {
    RtcFloatLayout L;
    if (!rtc_float_layout(format, d, w, h, &L, nullptr)) return RTC_ERR_ARG;
    rtc_status st = sc.pack.d_len.reserve(1);
    if (st == RTC_OK) st = sc.pack.out.reserve(up16((size_t)L.file_bytes));
    const size_t table = up8(L.header); // the channel table behind the header, 8-byte aligned
    if (st == RTC_OK) st = sc.pack.header(table + sizeof L.ch + sizeof L.ch_off);
    if (st != RTC_OK) return st;
    rtc_float_layout(format, d, w, h, &L, sc.pack.h_hdr);
    std::memcpy(sc.pack.h_hdr + table, L.ch, sizeof L.ch);
    std::memcpy(sc.pack.h_hdr + table + sizeof L.ch, L.ch_off, sizeof L.ch_off);
    HIP_TRY(hipMemcpyAsync(sc.pack.d_hdr.get(), sc.pack.h_hdr, table + sizeof L.ch + sizeof L.ch_off, hipMemcpyHostToDevice, s));
    e->d_body = sc.pack.out.get();
    e->d_len = sc.pack.d_len.get();
    e->cap = L.file_bytes;
    if (format == RTC_FLOAT_HDR && rtc_hdr_is_rle(w)) {
        const size_t planes = (size_t)4 * w * h;
        st = sc.planes.reserve(planes);
        if (st == RTC_OK) st = sc.sizes.reserve((size_t)4 * h);
        if (st == RTC_OK) st = sc.offs.reserve((size_t)4 * h);
        if (st != RTC_OK) return st;
        const HdrArgs a{d->rgb, sc.pack.d_hdr.get(), sc.planes.get(), sc.sizes.get(), sc.offs.get(), sc.pack.out.get(), sc.pack.d_len.get(),
                        L.file_bytes, w, h, L.header};
        const unsigned long long px = std::max<unsigned long long>((unsigned long long)w * h, L.header);
        const uint32_t waves = (4u * h + PACK_THREADS / 64u - 1u) / (PACK_THREADS / 64u);
        hipLaunchKernelGGL(k_hdr_planes, dim3((uint32_t)((px + PACK_THREADS - 1) / PACK_THREADS)), dim3(PACK_THREADS), 0, s, a);
        hipLaunchKernelGGL(k_hdr_rle<false>, dim3(waves), dim3(PACK_THREADS), 0, s, a);
        hipLaunchKernelGGL(k_hdr_offsets, dim3(1), dim3(SCAN_THREADS), 0, s, a);
        hipLaunchKernelGGL(k_hdr_rle<true>, dim3(waves), dim3(PACK_THREADS), 0, s, a);
        HIP_TRY(hipGetLastError());
        e->min_len = L.header + 12ull * h; // a marker and at least one run token per plane
        return RTC_OK;
    }
    const uint8_t *dh = sc.pack.d_hdr.get();
    const FloatPackArgs a{dh, sc.pack.out.get(), sc.pack.d_len.get(), L.file_bytes, d->rgb, reinterpret_cast<const RtcExrChannel *>(dh + table),
                          reinterpret_cast<const uint32_t *>(dh + table + sizeof L.ch), format, w, h, L.header, L.pixel_bytes, L.n_channels};
    const unsigned long long threads = (L.file_bytes + 15) / 16;
    hipLaunchKernelGGL(k_float_pack, dim3((uint32_t)((threads + PACK_THREADS - 1) / PACK_THREADS)), dim3(PACK_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    e->min_len = L.file_bytes;
    return RTC_OK;
}
