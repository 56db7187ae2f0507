// rtc_jpeg.hip — [device] the JPEG writer of include/rtc.h on gfx950 for a frame already in device memory (rtc_encode.h).
// host_jpeg.cpp states the same bytes on the host; the per-block arithmetic of both is rtc_jpeg.h. The host writes the 623 header bytes (fixed for a size and quality); the device produces the rest.
//
// Kernels of one frame, in stream order:
//   k_jpeg_blocks    one wave per MCU: colour (lane = pixel), the two DCT passes through LDS (one lane per row / column of
//                    each component), quantisation with lane = zigzag position; coefficients stored in zigzag order; a
//                    ballot of the non-zero mask gives each lane its run, and a wave sum the block's AC bits; DC kept apart
//   k_jpeg_mcu_scan  one thread per MCU: DC differences and their code lengths, the MCU's bits, a scan inside the workgroup
//   k_jpeg_group_scan one workgroup: scan of the workgroups' totals -> total bits, data bytes, 4 KB chunks
//   k_jpeg_clear     zero the words the packed stream will occupy
//   k_jpeg_pack      one wave per MCU: every lane rebuilds its code from the stored coefficient and ORs it into the
//                    big-endian 64-bit words at its offset (a code of <= 59 bits touches at most two words: two atomics);
//                    the padding 1-bits behind the last code
//   k_jpeg_ffcount   0xFF bytes per 4 KB chunk of the packed stream
//   k_jpeg_ffscan    one workgroup: scan of the chunk counts -> each chunk's output offset, file length
//   k_jpeg_scatter   the bytes of every chunk, a 0x00 behind each 0xFF, and EOI
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rtc.h"
#include "rtc_encode.h"
#include "rtc_jpeg.h"

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

constexpr uint32_t CHUNK = 4096;        // bytes of packed stream per workgroup of k_jpeg_ffcount / k_jpeg_scatter (16 per thread)
constexpr uint32_t MCU_PER_GROUP = 256; // k_jpeg_mcu_scan
constexpr uint32_t DATA_GRID_MAX = 1024;

struct JpegInfo {
    unsigned long long bits;       // entropy-coded bits, padding excluded
    unsigned long long data_bytes; // packed bytes, padding included
    unsigned long long out_bytes;  // stuffed data + EOI: what follows the header
    unsigned long long nchunks;
};

struct JpegQuant {
    uint16_t q[128]; // luma, chroma; natural order
};

template <typename T>
__device__ inline T wave_incl_scan(T v) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// inclusive scan over a workgroup of blockDim.x (a multiple of 64, at most 1024) threads
template <typename T>
__device__ inline T block_incl_scan(T v, T *s_tmp) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    v = wave_incl_scan(v);
    if (lane == 63) s_tmp[wave] = v;
    __syncthreads();
    for (uint32_t k = 0; k < wave; ++k) v += s_tmp[k];
    __syncthreads();
    return v;
}

// Code of zigzag position `lane` of a block whose quantised coefficients (zigzag order) this wave holds, one per lane: the
// DC difference on lane 0 (`dc_diff`), a non-zero AC with the ZRLs and the run in front of it, or EOB on lane 63 when the
// block ends in zeros. Every lane must call it (ballot).
__device__ inline uint32_t lane_code(int chroma, uint32_t lane, int32_t v, int32_t dc_diff, uint64_t *code) {
    const unsigned long long nz = __ballot(v != 0) & ~1ull;
    *code = 0;
    if (lane == 0) return rtc_jpeg_dc_code(chroma, dc_diff, code);
    if (v != 0) {
        const unsigned long long below = nz & ((1ull << lane) - 1ull);
        const uint32_t prev = below ? 63u - (uint32_t)__clzll(below) : 0u;
        return rtc_jpeg_ac_code(chroma, lane - 1u - prev, v, code);
    }
    if (lane == 63) return rtc_jpeg_eob_code(chroma, code);
    return 0;
}

__global__ __launch_bounds__(256) void k_jpeg_blocks(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                                                     uint32_t mcu_w, uint32_t nmcu, JpegQuant quant, int16_t *coef, uint32_t *acbits,
                                                     int32_t *dc) {
    __shared__ int32_t s[4][3][64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t mcu = blockIdx.x * 4u + wave;
    const bool active = mcu < nmcu;
    if (active) {
        const uint32_t mx = mcu % mcu_w, my = mcu / mcu_w;
        const uint32_t x = min(mx * 8u + (lane & 7u), width - 1u), y = min(my * 8u + (lane >> 3), height - 1u);
        const uint8_t *p = pixels + ((size_t)y * width + x) * channels;
        uint32_t ycc[3];
        rtc_jpeg_ycc(p[0], p[1], p[2], ycc);
        for (int c = 0; c < 3; ++c) s[wave][c][lane] = (int32_t)ycc[c] - 128;
    }
    __syncthreads();
    if (active && lane < 24) rtc_jpeg_fdct_1d(&s[wave][lane >> 3][8u * (lane & 7u)], 1, 0);
    __syncthreads();
    if (active && lane < 24) rtc_jpeg_fdct_1d(&s[wave][lane >> 3][lane & 7u], 8, 1);
    __syncthreads();
    if (!active) return; // no workgroup barrier below
    const uint32_t nat = kJpegZigzag[lane];
    for (int c = 0; c < 3; ++c) {
        const int chroma = c ? 1 : 0;
        const int32_t v = rtc_jpeg_quantise(s[wave][c][nat], (int32_t)quant.q[64 * chroma + nat]);
        const size_t b = (size_t)mcu * 3u + (uint32_t)c;
        coef[b * 64u + lane] = (int16_t)v;
        uint64_t code;
        uint32_t len = lane_code(chroma, lane, v, 0, &code);
        if (lane == 0) { len = 0; dc[b] = v; } // the DC's code needs its predecessor: k_jpeg_mcu_scan
        for (uint32_t o = 32; o; o >>= 1) len += __shfl_xor(len, o, 64);
        if (lane == 0) acbits[b] = len;
    }
}

__device__ inline uint32_t dc_bits(const int32_t *dc, uint32_t mcu, int c) {
    const int32_t prev = mcu ? dc[(size_t)(mcu - 1u) * 3u + (uint32_t)c] : 0;
    uint64_t code;
    return rtc_jpeg_dc_code(c ? 1 : 0, dc[(size_t)mcu * 3u + (uint32_t)c] - prev, &code);
}

__global__ __launch_bounds__(256) void k_jpeg_mcu_scan(const uint32_t *acbits, const int32_t *dc, uint32_t nmcu, uint32_t *mcu_off,
                                                       unsigned long long *group_total) {
    __shared__ uint32_t s_tmp[4];
    const uint32_t m = blockIdx.x * MCU_PER_GROUP + threadIdx.x;
    uint32_t bits = 0; // <= 3 * RTC_JPEG_BLOCK_BITS_MAX per MCU: 256 of them fit 32 bits
    if (m < nmcu)
        for (int c = 0; c < 3; ++c) bits += acbits[(size_t)m * 3u + (uint32_t)c] + dc_bits(dc, m, c);
    const uint32_t incl = block_incl_scan(bits, s_tmp);
    if (m < nmcu) mcu_off[m] = incl - bits;
    if (threadIdx.x == MCU_PER_GROUP - 1) group_total[blockIdx.x] = incl;
}

__global__ __launch_bounds__(1024) void k_jpeg_group_scan(unsigned long long *group, uint32_t ngroups, JpegInfo *info) {
    __shared__ unsigned long long s_tmp[16];
    __shared__ unsigned long long s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < ngroups; base += 1024) {
        const uint32_t j = base + threadIdx.x;
        const unsigned long long v = j < ngroups ? group[j] : 0ull;
        const unsigned long long incl = block_incl_scan(v, s_tmp);
        const unsigned long long carry = s_carry;
        if (j < ngroups) group[j] = carry + incl - v; // in place: totals -> offsets
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long T = s_carry, D = (T + 7) / 8;
        info->bits = T;
        info->data_bytes = D;
        info->nchunks = (D + CHUNK - 1) / CHUNK;
    }
}

__global__ __launch_bounds__(256) void k_jpeg_clear(unsigned long long *words, const JpegInfo *info) {
    const unsigned long long nw = (info->data_bytes + 7) / 8 + 1;
    for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < nw; j += (unsigned long long)gridDim.x * blockDim.x)
        words[j] = 0;
}

// OR the `len` (<= 59) low bits of `code` into the MSB-first stream at bit `at`
// (`nwords`: the buffer's words; the worst-case bound of include/rtc.h keeps every code inside it, checked anyway)
__device__ inline void put_bits(unsigned long long *words, unsigned long long nwords, unsigned long long at, uint64_t code, uint32_t len) {
    const unsigned long long w = at >> 6;
    if (len == 0 || w + 1 >= nwords) return;
    const uint32_t s = (uint32_t)(at & 63u);
    if (s + len <= 64) {
        atomicOr(&words[w], (unsigned long long)(code << (64u - s - len)));
    } else {
        atomicOr(&words[w], (unsigned long long)(code >> (s + len - 64u)));
        atomicOr(&words[w + 1], (unsigned long long)(code << (128u - s - len)));
    }
}

__global__ __launch_bounds__(256) void k_jpeg_pack(const int16_t *coef, const int32_t *dc, uint32_t nmcu, const uint32_t *mcu_off,
                                                   const unsigned long long *group_off, const JpegInfo *info, unsigned long long *words,
                                                   unsigned long long nwords) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t mcu = blockIdx.x * 4u + wave;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long T = info->bits;
        const uint32_t pad = (uint32_t)((8u - (T & 7u)) & 7u);
        put_bits(words, nwords, T, (1ull << pad) - 1ull, pad);
    }
    if (mcu >= nmcu) return; // the whole wave
    unsigned long long at = group_off[mcu / MCU_PER_GROUP] + mcu_off[mcu];
    for (int c = 0; c < 3; ++c) {
        const size_t b = (size_t)mcu * 3u + (uint32_t)c;
        const int32_t v = coef[b * 64u + lane];
        const int32_t diff = lane == 0 ? v - (mcu ? dc[b - 3u] : 0) : 0;
        uint64_t code;
        const uint32_t len = lane_code(c ? 1 : 0, lane, v, diff, &code);
        const uint32_t incl = wave_incl_scan(len);
        put_bits(words, nwords, at + (incl - len), code, len);
        at += __shfl(incl, 63, 64);
    }
}

__device__ inline uint32_t stream_byte(const unsigned long long *words, unsigned long long i) {
    return (uint32_t)(words[i >> 3] >> (56u - 8u * (uint32_t)(i & 7u))) & 255u;
}

__global__ __launch_bounds__(256) void k_jpeg_ffcount(const unsigned long long *words, const JpegInfo *info, uint32_t *ffcnt) {
    __shared__ uint32_t s_tmp[4];
    const unsigned long long D = info->data_bytes, nchunks = info->nchunks;
    for (unsigned long long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const unsigned long long i0 = ch * CHUNK + 16ull * threadIdx.x;
        uint32_t n = 0;
        for (uint32_t k = 0; k < 16; ++k)
            if (i0 + k < D && stream_byte(words, i0 + k) == 0xFFu) ++n;
        const uint32_t incl = block_incl_scan(n, s_tmp);
        if (threadIdx.x == 255) ffcnt[ch] = incl;
    }
}

__global__ __launch_bounds__(1024) void k_jpeg_ffscan(const uint32_t *ffcnt, JpegInfo *info, unsigned long long *chunk_off) {
    __shared__ unsigned long long s_tmp[16];
    __shared__ unsigned long long s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const unsigned long long nchunks = info->nchunks;
    for (unsigned long long base = 0; base < nchunks; base += 1024) {
        const unsigned long long j = base + threadIdx.x;
        const unsigned long long v = j < nchunks ? ffcnt[j] : 0ull;
        const unsigned long long incl = block_incl_scan(v, s_tmp);
        const unsigned long long carry = s_carry;
        if (j < nchunks) chunk_off[j] = j * CHUNK + carry + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) info->out_bytes = info->data_bytes + s_carry + 2;
}

__global__ __launch_bounds__(256) void k_jpeg_scatter(const unsigned long long *words, const JpegInfo *info,
                                                      const unsigned long long *chunk_off, uint8_t *out, unsigned long long cap) {
    __shared__ uint32_t s_tmp[4];
    const unsigned long long D = info->data_bytes, nchunks = info->nchunks;
    for (unsigned long long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const unsigned long long i0 = ch * CHUNK + 16ull * threadIdx.x;
        uint32_t b[16], n = 0;
        for (uint32_t k = 0; k < 16; ++k) {
            b[k] = i0 + k < D ? stream_byte(words, i0 + k) : 0u;
            n += (i0 + k < D && b[k] == 0xFFu) ? 1u : 0u;
        }
        const uint32_t incl = block_incl_scan(n, s_tmp);
        unsigned long long pos = chunk_off[ch] + 16ull * threadIdx.x + (incl - n);
        for (uint32_t k = 0; k < 16 && i0 + k < D; ++k) {
            if (pos + 1 < cap) out[pos] = (uint8_t)b[k];
            ++pos;
            if (b[k] == 0xFFu) {
                if (pos + 1 < cap) out[pos] = 0;
                ++pos;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned long long L = info->out_bytes;
        if (L >= 2 && L <= cap) {
            out[L - 2] = 0xFF;
            out[L - 1] = 0xD9;
        }
    }
}

} // namespace

// ---- host side ------------------------------------------------------------------------------------------------------

rtc_status JpegScratch::reserve(size_t nmcu) {
    if (nmcu <= mcu_cap) return RTC_OK;
    mcu_cap = 0;
    const size_t ngroups = (nmcu + MCU_PER_GROUP - 1) / MCU_PER_GROUP;
    nwords = (nmcu * 3 * (size_t)RTC_JPEG_BLOCK_BITS_MAX + 63) / 64 + 2; // + the padding's and a spare word
    data_max = nwords * 8;
    const size_t nchunks = (data_max + CHUNK - 1) / CHUNK;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_coef = 0, o_ac = o_coef + up(nmcu * 192 * 2), o_dc = o_ac + up(nmcu * 3 * 4), o_off = o_dc + up(nmcu * 3 * 4),
                 o_grp = o_off + up(nmcu * 4), o_info = o_grp + up(ngroups * 8), o_words = o_info + up(sizeof(JpegInfo)),
                 o_ff = o_words + up(nwords * 8), o_co = o_ff + up(nchunks * 4), o_out = o_co + up(nchunks * 8),
                 total = o_out + up(2 * data_max + 2);
    const rtc_status st = this->block.reserve(total);
    if (st != RTC_OK) return st;
    uint8_t *block = this->block.get();
    coef = reinterpret_cast<int16_t *>(block + o_coef);
    acbits = reinterpret_cast<uint32_t *>(block + o_ac);
    dc = reinterpret_cast<int32_t *>(block + o_dc);
    mcu_off = reinterpret_cast<uint32_t *>(block + o_off);
    group = reinterpret_cast<unsigned long long *>(block + o_grp);
    info = block + o_info;
    words = reinterpret_cast<unsigned long long *>(block + o_words);
    ffcnt = reinterpret_cast<uint32_t *>(block + o_ff);
    chunk_off = reinterpret_cast<unsigned long long *>(block + o_co);
    out = block + o_out;
    mcu_cap = nmcu;
    return RTC_OK;
}

// The whole chain on `s`; the body is the stuffed data + EOI (what follows the header), its length info->out_bytes.
rtc_status rtc_jpeg_enqueue(JpegScratch &sc, const uint8_t *d_pixels, uint32_t w, uint32_t h, uint32_t channels, int32_t quality,
                            hipStream_t s, RtcEncoded *e) {
    const uint32_t mcu_w = (w + 7) / 8, mcu_h = (h + 7) / 8;
    const size_t nmcu = (size_t)mcu_w * mcu_h;
    const rtc_status r = sc.reserve(nmcu);
    if (r != RTC_OK) return r;
    JpegInfo *info = static_cast<JpegInfo *>(sc.info);
    JpegQuant q;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) q.q[64 * t + i] = (uint16_t)rtc_jpeg_quant_entry(quality, t, i);
    const uint32_t ngroups = (uint32_t)((nmcu + MCU_PER_GROUP - 1) / MCU_PER_GROUP);
    const uint32_t grid_mcu = (uint32_t)((nmcu + 3) / 4);
    const size_t nchunks_max = (sc.data_max + CHUNK - 1) / CHUNK;
    const uint32_t grid_data = (uint32_t)std::min<size_t>(DATA_GRID_MAX, nchunks_max);
    const unsigned long long out_cap = 2 * sc.data_max + 2;
    hipLaunchKernelGGL(k_jpeg_blocks, dim3(grid_mcu), dim3(256), 0, s, d_pixels, w, h, channels, mcu_w, (uint32_t)nmcu, q, sc.coef,
                       sc.acbits, sc.dc);
    hipLaunchKernelGGL(k_jpeg_mcu_scan, dim3(ngroups), dim3(MCU_PER_GROUP), 0, s, sc.acbits, sc.dc, (uint32_t)nmcu, sc.mcu_off, sc.group);
    hipLaunchKernelGGL(k_jpeg_group_scan, dim3(1), dim3(1024), 0, s, sc.group, ngroups, info);
    hipLaunchKernelGGL(k_jpeg_clear, dim3(grid_data), dim3(256), 0, s, sc.words, info);
    hipLaunchKernelGGL(k_jpeg_pack, dim3(grid_mcu), dim3(256), 0, s, sc.coef, sc.dc, (uint32_t)nmcu, sc.mcu_off, sc.group, info,
                       sc.words, (unsigned long long)sc.nwords);
    hipLaunchKernelGGL(k_jpeg_ffcount, dim3(grid_data), dim3(256), 0, s, sc.words, info, sc.ffcnt);
    hipLaunchKernelGGL(k_jpeg_ffscan, dim3(1), dim3(1024), 0, s, sc.ffcnt, info, sc.chunk_off);
    hipLaunchKernelGGL(k_jpeg_scatter, dim3(grid_data), dim3(256), 0, s, sc.words, info, sc.chunk_off, sc.out, out_cap);
    HIP_TRY(hipGetLastError());
    e->d_body = sc.out;
    e->d_len = &info->out_bytes;
    e->cap = out_cap;
    e->min_len = 2; // EOI
    return RTC_OK;
}
