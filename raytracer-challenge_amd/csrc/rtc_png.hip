// rtc_png.hip — [device] the compressed PNG writer of include/rtc.h on gfx950 for a frame already in device memory
// (rtc_encode.h). host_png.cpp states the same bytes on the host; the arithmetic of both is rtc_png.h.
//
// Kernels of one frame, in stream order (n = filtered bytes, one segment = RTC_PNG_SEGMENT of them):
//   k_png_filter   one wave per row: the five filters' sums (lane = byte, wave reduction), then the chosen filter's row
//   k_png_prev     one workgroup (one wave) per segment: the hash heads of the segment's window (the 32 KiB before it
//                  and itself) in LDS, walked in order 64 positions at a time; duplicates inside the 64 are resolved by
//                  comparing every lane's hash with every other lane's; prev[p] (distance to the nearest earlier position
//                  of p's hash, 0 past the window) for the segment's positions
//   k_png_match    one thread per position: rtc_png_match through prev[] -> L and distance
//   k_png_parse    one workgroup per segment: the L of the segment in LDS, one lane walks the lazy parse and flags the
//                  token starts (the only serial step: one LDS read pair per token)
//   k_png_segment  one workgroup per segment: symbol counts (LDS atomics: counts only), the Adler-32 parts, the block plan
//                  (package-merge, rtc_png_plan, one lane), the header bits, a scan of the tokens' bit lengths and the
//                  codes ORed into the segment's own 64-bit words; the sync flush; the segment's byte length
//   k_png_layout   one workgroup: scan of the chunk sizes -> offsets; signature, IHDR, chunk heads, zlib header, Adler-32, IEND
//   k_png_copy     one workgroup per segment: its bytes into the file
//   k_png_crc      one workgroup per chunk: CRC-32 of 256 slices, combined pairwise (x^(8n) mod P)
// The atomics (symbol counts, Adler parts, ORs of disjoint bit ranges) are order-free; nothing is floating point.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rtc.h"
#include "rtc_encode.h"
#include "rtc_png.h"

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

constexpr uint32_t SEG = RTC_PNG_SEGMENT;
constexpr uint32_t SEG_WORDS = (RTC_PNG_SEG_BYTES_MAX + 7) / 8 + 2; // a segment's packed bytes, as 64-bit words, + spare
constexpr uint32_t SEG_THREADS = 1024, PER_THREAD = SEG / SEG_THREADS;
constexpr uint32_t NONE = 0xffffffffu;

struct SegInfo {
    uint32_t nbytes;  // deflate bytes of the segment (block + sync flush)
    uint32_t adler_a; // sum of its filtered bytes, mod 65521
    uint32_t adler_b; // sum of (n - p) * s[p] over its positions, mod 65521
    uint32_t pad;
};

struct PngInfo {
    unsigned long long file_bytes;
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

__global__ __launch_bounds__(256) void k_png_filter(const uint8_t *px, uint32_t w, uint32_t h, uint32_t bpp, uint8_t *out) {
    const uint32_t lane = threadIdx.x & 63u, y = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (y >= h) return; // the whole wave; no workgroup barrier
    const size_t row = (size_t)w * bpp;
    const uint8_t *cur = px + (size_t)y * row, *up = y ? cur - row : nullptr;
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (size_t x = lane; x < row; x += 64) {
        const uint32_t a = x >= bpp ? cur[x - bpp] : 0u, b = up ? up[x] : 0u, c = (up && x >= bpp) ? up[x - bpp] : 0u, v = cur[x];
#pragma unroll
        for (uint32_t t = 0; t < 5; ++t) sum[t] += rtc_png_filter_cost(rtc_png_filter_byte(t, v, a, b, c));
    }
    uint32_t best = 0, best_sum = 0;
#pragma unroll
    for (uint32_t t = 0; t < 5; ++t) {
        uint32_t s = sum[t];
        for (uint32_t o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
        if (t == 0 || s < best_sum) { best_sum = s; best = t; }
    }
    uint8_t *o = out + (size_t)y * (row + 1);
    if (lane == 0) o[0] = (uint8_t)best;
    for (size_t x = lane; x < row; x += 64) {
        const uint32_t a = x >= bpp ? cur[x - bpp] : 0u, b = up ? up[x] : 0u, c = (up && x >= bpp) ? up[x - bpp] : 0u;
        o[1 + x] = (uint8_t)rtc_png_filter_byte(best, cur[x], a, b, c);
    }
}

__global__ __launch_bounds__(64) void k_png_prev(const uint8_t *s, unsigned long long n, uint16_t *prev) {
    __shared__ uint32_t s_head[RTC_PNG_HASH_SIZE]; // 128 KiB: positions relative to the window's start
    const uint32_t lane = threadIdx.x;
    const unsigned long long s0 = (unsigned long long)blockIdx.x * SEG;
    if (n < 3) return;
    const unsigned long long ws = s0 >= RTC_PNG_WINDOW ? s0 - RTC_PNG_WINDOW : 0ull;
    const unsigned long long we = min(s0 + SEG, n - 2); // positions p with p + 3 <= n
    for (uint32_t j = lane; j < RTC_PNG_HASH_SIZE; j += 64) s_head[j] = NONE;
    __syncthreads();
    for (unsigned long long base = ws; base < we; base += 64) {
        const unsigned long long p = base + lane;
        const bool valid = p < we;
        const uint32_t h = valid ? rtc_png_hash(s[p], s[p + 1], s[p + 2]) : NONE;
        int near = -1;
        bool later = false;
        for (int j = 0; j < 64; ++j) {
            const uint32_t hj = __shfl(h, j, 64);
            if (valid && hj == h) {
                if (j < (int)lane) near = j;
                if (j > (int)lane) later = true;
            }
        }
        const uint32_t q = !valid ? NONE : near >= 0 ? (uint32_t)(base - ws) + (uint32_t)near : s_head[h];
        __syncthreads();
        if (valid && !later) s_head[h] = (uint32_t)(p - ws);
        __syncthreads();
        if (valid && p >= s0) prev[p] = (q != NONE && p - (ws + q) <= RTC_PNG_WINDOW) ? (uint16_t)(p - (ws + q)) : (uint16_t)0;
    }
}

__global__ __launch_bounds__(256) void k_png_match(const uint8_t *s, unsigned long long n, const uint16_t *prev, uint32_t *M) {
    const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const unsigned long long end = min((p / SEG + 1) * SEG, n);
    uint32_t d;
    const uint32_t l = rtc_png_match(s, n, prev, p, end, &d);
    M[p] = l | (d << 16);
}

// T[p]: 0x8000 = a literal starts at p, 0xC000 = a match starts at p, 0 = inside a match
__global__ __launch_bounds__(256) void k_png_parse(const uint32_t *M, unsigned long long n, uint16_t *T) {
    __shared__ uint16_t s_l[SEG + 1];
    const unsigned long long s0 = (unsigned long long)blockIdx.x * SEG;
    const uint32_t m = (uint32_t)min((unsigned long long)SEG, n - s0);
    for (uint32_t i = threadIdx.x; i <= m; i += 256) s_l[i] = i < m ? (uint16_t)(M[s0 + i] & 0xffffu) : (uint16_t)0;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t p = 0; p < m;) {
            const uint32_t l = s_l[p];
            if (rtc_png_takes_match(l, s_l[p + 1])) {
                s_l[p] = 0xC000u;
                p += l;
            } else {
                s_l[p] = 0x8000u;
                ++p;
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < m; i += 256) T[s0 + i] = s_l[i] & 0xC000u;
}

// OR `n` (<= 48) bits of v into the LSB-first stream of 64-bit words at bit `at`
__device__ inline void or_bits(unsigned long long *words, unsigned long long at, unsigned long long v, uint32_t n) {
    if (n == 0) return;
    const uint32_t w = (uint32_t)(at >> 6), sh = (uint32_t)(at & 63u);
    if (w >= SEG_WORDS) return; // cannot happen: no block exceeds its stored form
    atomicOr(&words[w], v << sh);
    if (sh + n > 64 && w + 1 < SEG_WORDS) atomicOr(&words[w + 1], v >> (64u - sh));
}

struct PngPlanShared {
    PngPlan plan;
    PngHuffWork work;
    uint32_t lit[RTC_PNG_NLIT], dist[RTC_PNG_NDIST];
    uint32_t extra, adler_a, adler_b, header_bits;
    uint64_t scan_tmp[SEG_THREADS / 64];
};

__device__ inline uint32_t token_bits(const PngPlan &pl, const uint8_t *s, const uint32_t *M, const uint16_t *T, unsigned long long p,
                                      uint64_t *code) {
    const uint32_t t = T[p];
    if (!(t & 0x8000u)) { *code = 0; return 0; }
    uint32_t nb;
    const bool mt = (t & 0x4000u) != 0;
    const uint32_t mm = mt ? M[p] : 0u;
    *code = rtc_png_token_code(pl, s[p], mm & 0xffffu, mm >> 16, &nb);
    return nb;
}

__global__ __launch_bounds__(SEG_THREADS) void k_png_segment(const uint8_t *s, unsigned long long n, const uint32_t *M, const uint16_t *T,
                                                             unsigned long long *seg_words, SegInfo *info) {
    __shared__ PngPlanShared sh;
    const uint32_t tid = threadIdx.x, g = blockIdx.x;
    const unsigned long long s0 = (unsigned long long)g * SEG;
    const uint32_t m = (uint32_t)min((unsigned long long)SEG, n - s0);
    const bool last = s0 + m == n;
    unsigned long long *words = seg_words + (size_t)g * SEG_WORDS;
    for (uint32_t i = tid; i < RTC_PNG_NLIT; i += SEG_THREADS) sh.lit[i] = 0;
    if (tid < RTC_PNG_NDIST) sh.dist[tid] = 0;
    if (tid == 0) { sh.extra = 0; sh.adler_a = 0; sh.adler_b = 0; }
    for (uint32_t i = tid; i < SEG_WORDS; i += SEG_THREADS) words[i] = 0;
    __syncthreads();
    const uint32_t i0 = tid * PER_THREAD, i1 = min(i0 + PER_THREAD, m);
    unsigned long long aa = 0, ab = 0;
    uint32_t extra = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        const unsigned long long p = s0 + i;
        const uint32_t b = s[p];
        aa += b;
        ab += (n - p) * b;
        const uint32_t t = T[p];
        if (t & 0x4000u) {
            const uint32_t mm = M[p], lc = rtc_png_len_code(mm & 0xffffu), dc = rtc_png_dist_code(mm >> 16);
            atomicAdd(&sh.lit[257 + lc], 1u);
            atomicAdd(&sh.dist[dc], 1u);
            extra += rtc_png_len_extra(lc) + rtc_png_dist_extra(dc);
        } else if (t & 0x8000u) {
            atomicAdd(&sh.lit[b], 1u);
        }
    }
    if (extra) atomicAdd(&sh.extra, extra);
    atomicAdd(&sh.adler_a, (uint32_t)(aa % 65521u));
    atomicAdd(&sh.adler_b, (uint32_t)(ab % 65521u));
    __syncthreads();
    if (tid == 0) {
        sh.lit[256] = 1;
        rtc_png_plan(sh.lit, sh.dist, sh.extra, m, &sh.plan, &sh.work);
        unsigned long long at = 0;
        auto put = [&](unsigned long long v, uint32_t nb) {
            or_bits(words, at, v, nb);
            at += nb;
        };
        rtc_png_block_header(sh.plan, last, m, put);
        sh.header_bits = (uint32_t)at;
        info[g].adler_a = sh.adler_a % 65521u;
        info[g].adler_b = sh.adler_b % 65521u;
    }
    __syncthreads();
    const PngPlan &pl = sh.plan;
    const bool stored = pl.type == RTC_PNG_STORED;
    uint64_t mine = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        uint64_t code;
        mine += stored ? 8u : token_bits(pl, s, M, T, s0 + i, &code);
    }
    const uint64_t incl = block_incl_scan(mine, sh.scan_tmp);
    unsigned long long at = sh.header_bits + (incl - mine);
    for (uint32_t i = i0; i < i1; ++i) {
        uint64_t code;
        uint32_t nb;
        if (stored) {
            code = s[s0 + i];
            nb = 8;
        } else {
            nb = token_bits(pl, s, M, T, s0 + i, &code);
        }
        or_bits(words, at, code, nb);
        at += nb;
    }
    if (tid == SEG_THREADS - 1) {
        unsigned long long bits = sh.header_bits + incl;
        if (!stored) {
            or_bits(words, bits, pl.lit_code[256], pl.lit_len[256]);
            bits += pl.lit_len[256];
        }
        uint32_t nbytes;
        if (!last) {
            bits += 3;                        // the empty stored block's BFINAL = 0, BTYPE = 00
            nbytes = (uint32_t)((bits + 7) / 8) + 4; // LEN 00 00, NLEN FF FF
            or_bits(words, 8ull * (nbytes - 2), 0xffffu, 16);
        } else {
            nbytes = (uint32_t)((bits + 7) / 8);
        }
        info[g].nbytes = nbytes;
    }
}

__device__ inline uint32_t chunk_data_bytes(const SegInfo *info, uint32_t g, uint32_t nseg) {
    return info[g].nbytes + (g == 0 ? 2u : 0u) + (g + 1 == nseg ? 4u : 0u);
}

__device__ inline uint32_t crc_bytes(uint32_t c, const uint8_t *p, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) c = rtc_png_crc_table((c ^ p[i]) & 255u) ^ (c >> 8);
    return c;
}

__global__ __launch_bounds__(1024) void k_png_layout(const SegInfo *info, uint32_t nseg, unsigned long long n, uint32_t w, uint32_t h,
                                                     uint32_t channels, unsigned long long *chunk_off, uint8_t *out, unsigned long long cap,
                                                     PngInfo *pinfo) {
    __shared__ unsigned long long s_tmp[16];
    __shared__ unsigned long long s_carry, s_a, s_b;
    if (threadIdx.x == 0) { s_carry = 33; s_a = 0; s_b = 0; }
    __syncthreads();
    for (uint32_t base = 0; base < nseg; base += 1024) {
        const uint32_t g = base + threadIdx.x;
        const unsigned long long v = g < nseg ? RTC_PNG_CHUNK_OVERHEAD + chunk_data_bytes(info, g, nseg) : 0ull;
        if (g < nseg) { atomicAdd(&s_a, (unsigned long long)info[g].adler_a); atomicAdd(&s_b, (unsigned long long)info[g].adler_b); }
        const unsigned long long incl = block_incl_scan(v, s_tmp);
        const unsigned long long carry = s_carry;
        if (g < nseg) {
            const unsigned long long at = carry + incl - v;
            chunk_off[g] = at;
            if (at + 8 <= cap) {
                rtc_png_be32(out + at, chunk_data_bytes(info, g, nseg));
                out[at + 4] = 'I'; out[at + 5] = 'D'; out[at + 6] = 'A'; out[at + 7] = 'T';
            }
        }
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long total = s_carry + 12;
        pinfo->file_bytes = total;
        if (total > cap) return;
        rtc_png_head(w, h, channels, out);
        rtc_png_be32(out + 29, crc_bytes(0xffffffffu, out + 12, 17) ^ 0xffffffffu);
        const unsigned long long first = chunk_off[0] + 8;
        out[first] = 0x78;
        out[first + 1] = 0x9c;
        const uint32_t A = (uint32_t)((1ull + s_a) % 65521u), B = (uint32_t)((n % 65521u + s_b) % 65521u);
        rtc_png_be32(out + s_carry - 8, (B << 16) | A); // the last chunk's data ends with it, then its CRC
        uint8_t *e = out + total - 12;
        rtc_png_be32(e, 0);
        e[4] = 'I'; e[5] = 'E'; e[6] = 'N'; e[7] = 'D';
        rtc_png_be32(e + 8, 0xAE426082u);
    }
}

__device__ inline uint32_t seg_byte(const unsigned long long *words, uint32_t i) {
    return (uint32_t)(words[i >> 3] >> (8u * (i & 7u))) & 255u;
}

__global__ __launch_bounds__(256) void k_png_copy(const unsigned long long *seg_words, const SegInfo *info, const unsigned long long *chunk_off,
                                                  uint8_t *out, unsigned long long cap) {
    const uint32_t g = blockIdx.x, nb = info[g].nbytes;
    const unsigned long long at = chunk_off[g] + 8 + (g == 0 ? 2 : 0);
    const unsigned long long *words = seg_words + (size_t)g * SEG_WORDS;
    for (uint32_t i = threadIdx.x; i < nb; i += 256)
        if (at + i < cap) out[at + i] = (uint8_t)seg_byte(words, i);
}

__global__ __launch_bounds__(256) void k_png_crc(const SegInfo *info, uint32_t nseg, const unsigned long long *chunk_off, uint8_t *out,
                                                 unsigned long long cap) {
    __shared__ uint32_t s_tab[256], s_crc[256], s_len[256];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    s_tab[t] = rtc_png_crc_table(t);
    const unsigned long long at = chunk_off[g] + 4;
    const uint32_t len = chunk_data_bytes(info, g, nseg) + 4; // type + data
    if (at + len + 4 > cap) return; // the whole workgroup
    const uint32_t per = (len + 255) / 256, b0 = min(t * per, len), b1 = min(b0 + per, len);
    __syncthreads();
    uint32_t c = 0xffffffffu;
    for (uint32_t i = b0; i < b1; ++i) c = s_tab[(c ^ out[at + i]) & 255u] ^ (c >> 8);
    s_crc[t] = c ^ 0xffffffffu; // the CRC-32 of the slice (0 for an empty one)
    s_len[t] = b1 - b0;
    __syncthreads();
    for (uint32_t st = 1; st < 256; st <<= 1) {
        if ((t & (2 * st - 1)) == 0) {
            s_crc[t] = rtc_png_crc_combine(s_crc[t], s_crc[t + st], s_len[t + st]);
            s_len[t] += s_len[t + st];
        }
        __syncthreads();
    }
    if (t == 0) rtc_png_be32(out + at + len, s_crc[0]);
}

} // namespace

// ---- host side ------------------------------------------------------------------------------------------------------

rtc_status PngScratch::reserve(size_t n) {
    if (n <= n_cap) return RTC_OK;
    n_cap = 0;
    const size_t nseg = (n + SEG - 1) / SEG;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t ocap = n + RTC_PNG_CHUNK_OVERHEAD * 2 * nseg + RTC_PNG_FILE_FIXED; // the stored bound, with room to spare
    const size_t o_filt = 0, o_prev = o_filt + up(n + 8), o_m = o_prev + up(2 * n), o_words = o_m + up(4 * n),
                 o_info = o_words + up(nseg * SEG_WORDS * 8), o_off = o_info + up(nseg * sizeof(SegInfo)), o_p = o_off + up(nseg * 8),
                 o_out = o_p + up(sizeof(PngInfo)), total = o_out + up(ocap);
    const rtc_status st = this->block.reserve(total);
    if (st != RTC_OK) return st;
    uint8_t *block = this->block.get();
    filt = block + o_filt;
    prev = reinterpret_cast<uint16_t *>(block + o_prev);
    M = reinterpret_cast<uint32_t *>(block + o_m);
    words = reinterpret_cast<unsigned long long *>(block + o_words);
    info = block + o_info;
    chunk_off = reinterpret_cast<unsigned long long *>(block + o_off);
    pinfo = block + o_p;
    out = block + o_out;
    out_cap = ocap;
    n_cap = n;
    return RTC_OK;
}

// The whole chain on `s`; the body is the file, its length pinfo->file_bytes.
rtc_status rtc_png_enqueue(PngScratch &sc, const uint8_t *d_pixels, uint32_t w, uint32_t h, uint32_t channels, hipStream_t s,
                           RtcEncoded *e) {
    const size_t n = ((size_t)w * channels + 1) * h;
    const rtc_status r = sc.reserve(n);
    if (r != RTC_OK) return r;
    SegInfo *info = static_cast<SegInfo *>(sc.info);
    PngInfo *pinfo = static_cast<PngInfo *>(sc.pinfo);
    const uint32_t nseg = (uint32_t)((n + SEG - 1) / SEG);
    const unsigned long long nn = n, cap = sc.out_cap;
    hipLaunchKernelGGL(k_png_filter, dim3((h + 3) / 4), dim3(256), 0, s, d_pixels, w, h, channels, sc.filt);
    hipLaunchKernelGGL(k_png_prev, dim3(nseg), dim3(64), 0, s, sc.filt, nn, sc.prev);
    hipLaunchKernelGGL(k_png_match, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, sc.filt, nn, sc.prev, sc.M);
    hipLaunchKernelGGL(k_png_parse, dim3(nseg), dim3(256), 0, s, sc.M, nn, sc.prev);
    hipLaunchKernelGGL(k_png_segment, dim3(nseg), dim3(SEG_THREADS), 0, s, sc.filt, nn, sc.M, sc.prev, sc.words, info);
    hipLaunchKernelGGL(k_png_layout, dim3(1), dim3(1024), 0, s, info, nseg, nn, w, h, channels, sc.chunk_off, sc.out, cap, pinfo);
    hipLaunchKernelGGL(k_png_copy, dim3(nseg), dim3(256), 0, s, sc.words, info, sc.chunk_off, sc.out, cap);
    hipLaunchKernelGGL(k_png_crc, dim3(nseg), dim3(256), 0, s, info, nseg, sc.chunk_off, sc.out, cap);
    HIP_TRY(hipGetLastError());
    e->d_body = sc.out;
    e->d_len = &pinfo->file_bytes;
    e->cap = cap;
    e->min_len = RTC_PNG_FILE_FIXED + RTC_PNG_CHUNK_OVERHEAD;
    return RTC_OK;
}
