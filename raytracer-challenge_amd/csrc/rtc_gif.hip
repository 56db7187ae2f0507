// rtc_gif.hip — [device] the GIF writer of include/rtc.h on gfx950: distinct-colour bitmap, bin histogram, median cut,
// nearest-entry mapping and segmented LZW for a frame already in device memory: one frame's record (rtc_encode.h).
// host_gif.cpp states the same bytes on the host.
//
// Kernels of one frame, in stream order (all on the stream of the frame's render):
//   k_gif_scan_pixels   pixel pass: presence bit of each 24-bit colour (global, tested before the atomic) and the
//                       32768-bin pixel counts (one 128 KB LDS histogram per workgroup, runs of one bin per thread
//                       merged before the LDS atomic, non-zero bins flushed with one global atomic each)
//   k_gif_bitmap_count  popcount of each 1024-word block of the 2 MB bitmap
//   k_gif_exact         total distinct colours; at most 256: every block writes its colours at its prefix (ascending)
//   k_gif_median_cut    one workgroup: the median cut over the occupied bins (list and owners in LDS, counts in L2),
//                       then the bin -> box table
//   k_gif_box_sums      median-cut case only: pixel pass summing r, g, b and n per box (LDS, then one atomic per box).
//                       The per-bin sums of the statement are only ever added up per box, so summing per box directly
//                       gives the same means with 256 accumulators instead of 3 x 32768 64-bit ones.
//   k_gif_map           palette into LDS (means, or the exact colours), table into the record, argmin over 256 entries
//   k_gif_lzw           one wave per segment of RTC_GIF_SEGMENT indices, dictionary as an 8192-slot hash in LDS
//   k_gif_offsets       one workgroup: scan of the segments' bit lengths, record length, record header
//   k_gif_pack          one byte of the packed stream per thread, with the sub-block length bytes and terminator
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rtc.h"
#include "rtc_encode.h"
#include "rtc_gif.h"

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

constexpr uint32_t BITMAP_WORDS = 1u << 19;  // 2^24 bits
constexpr uint32_t BITMAP_BLOCKS = 512;      // k_gif_bitmap_count / k_gif_exact: 1024 words per block
constexpr uint32_t PX_PER_THREAD = 8;
constexpr uint32_t PX_BLOCKS = 256; // k_gif_scan_pixels: one 1024-thread workgroup per CU (128 KB of LDS each), grid-stride beyond
constexpr uint32_t HASH_SLOTS = 8192;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;

struct GifInfo {
    uint32_t ncolours; // distinct colours (saturates nowhere: at most 2^24)
    uint32_t nbox;     // median cut: boxes; 0 = exact palette
    unsigned long long data_bytes;   // packed LZW bytes
    unsigned long long record_bytes; // the whole record
};

__device__ inline uint32_t bin_of(uint32_t r, uint32_t g, uint32_t b) { return ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3); }
__device__ inline int bin_coord(uint32_t bin, int axis) { return (int)((bin >> (10 - 5 * axis)) & 31u); }

// pixels [8t, 8t+8) ∩ [0, n) of `rgb` as 24 bytes (u64 loads when the frame is 8-byte aligned)
__device__ inline uint32_t load_px8(const uint8_t *rgb, size_t n, size_t i0, uint8_t (&px)[24]) {
    const uint32_t m = (uint32_t)min((size_t)PX_PER_THREAD, n - i0);
    const uint8_t *p = rgb + 3 * i0;
    if (m == PX_PER_THREAD && ((uintptr_t)p & 7u) == 0) {
        const unsigned long long *q = reinterpret_cast<const unsigned long long *>(p);
        unsigned long long w[3] = {q[0], q[1], q[2]};
        memcpy(px, w, 24);
    } else {
        for (uint32_t k = 0; k < 3 * m; ++k) px[k] = p[k];
    }
    return m;
}

__global__ __launch_bounds__(1024) void k_gif_scan_pixels(const uint8_t *rgb, size_t n, uint32_t *bitmap, uint32_t *cnt) {
    __shared__ uint32_t s_cnt[RTC_GIF_BINS]; // 128 KB
    for (uint32_t b = threadIdx.x; b < RTC_GIF_BINS; b += blockDim.x) s_cnt[b] = 0;
    __syncthreads();
    const size_t nthreads = (n + PX_PER_THREAD - 1) / PX_PER_THREAD;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * blockDim.x) {
        uint8_t px[24];
        const uint32_t m = load_px8(rgb, n, t * PX_PER_THREAD, px);
        uint32_t run_bin = EMPTY, run_n = 0, last_c = EMPTY;
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t r = px[3 * k], g = px[3 * k + 1], b = px[3 * k + 2];
            const uint32_t c = (r << 16) | (g << 8) | b;
            if (c != last_c) {
                last_c = c;
                const uint32_t bit = 1u << (c & 31u);
                if (!(__atomic_load_n(&bitmap[c >> 5], __ATOMIC_RELAXED) & bit)) atomicOr(&bitmap[c >> 5], bit);
            }
            const uint32_t bin = bin_of(r, g, b);
            if (bin != run_bin) {
                if (run_n) atomicAdd(&s_cnt[run_bin], run_n);
                run_bin = bin;
                run_n = 0;
            }
            ++run_n;
        }
        if (run_n) atomicAdd(&s_cnt[run_bin], run_n);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RTC_GIF_BINS; b += blockDim.x)
        if (s_cnt[b]) atomicAdd(&cnt[b], s_cnt[b]);
}

template <typename T>
__device__ inline T block_sum_256(T v, T *s_red) { // blockDim.x == 256
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63u) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    const T r = s_red[0] + s_red[1] + s_red[2] + s_red[3];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void k_gif_bitmap_count(const uint32_t *bitmap, uint32_t *blockcnt) {
    __shared__ uint32_t s_red[4];
    const uint32_t *w = bitmap + (size_t)blockIdx.x * 1024;
    uint32_t c = 0;
    for (uint32_t k = threadIdx.x; k < 1024; k += 256) c += __popc(w[k]);
    c = block_sum_256(c, s_red);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = c;
}

// inclusive scan over the 256 threads of a block
__device__ inline uint32_t block_scan_256(uint32_t v, uint32_t *s_tmp) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) s_tmp[wave] = v;
    __syncthreads();
    for (uint32_t k = 0; k < wave; ++k) v += s_tmp[k];
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(256) void k_gif_exact(uint32_t *bitmap, const uint32_t *blockcnt, uint32_t *pal32, GifInfo *info) {
    __shared__ uint32_t s_red[4];
    const uint32_t a = blockcnt[threadIdx.x], b = blockcnt[threadIdx.x + 256];
    const uint32_t total = block_sum_256(a + b, s_red);
    const uint32_t before = block_sum_256((threadIdx.x < blockIdx.x ? a : 0u) + (threadIdx.x + 256 < blockIdx.x ? b : 0u), s_red);
    if (blockIdx.x == 0 && threadIdx.x == 0) info->ncolours = total;
    if (total > 256) return;
    const uint32_t *w = bitmap + (size_t)blockIdx.x * 1024 + threadIdx.x * 4; // 4 consecutive words per thread: ascending
    uint32_t words[4], c = 0;
    for (int k = 0; k < 4; ++k) { words[k] = w[k]; c += __popc(words[k]); }
    const uint32_t incl = block_scan_256(c, s_red);
    uint32_t pos = before + incl - c;
    for (int k = 0; k < 4; ++k)
        for (uint32_t m = words[k]; m; m &= m - 1) {
            const uint32_t colour = ((blockIdx.x * 1024u + threadIdx.x * 4u + (uint32_t)k) << 5) | (uint32_t)__ffs(m) - 1u;
            pal32[pos++] = colour;
        }
}

// The median cut of include/rtc.h in one workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void k_gif_median_cut(const uint32_t *cnt, GifInfo *info, uint8_t *lut) {
    __shared__ uint16_t s_occ[RTC_GIF_BINS];  // occupied bins (any order: every decision below is a sum, min or max)
    __shared__ uint8_t s_owner[RTC_GIF_BINS]; // ... and the box each belongs to
    __shared__ int s_lo[256][3], s_hi[256][3];
    __shared__ unsigned long long s_n[256];
    __shared__ unsigned long long s_plane[32];
    __shared__ unsigned long long s_key[16];
    __shared__ uint32_t s_m, s_best, s_axis;
    __shared__ int s_cut;
    if (info->ncolours <= 256) {
        if (threadIdx.x == 0) info->nbox = 0;
        return;
    }
    const uint32_t t = threadIdx.x;
    if (t == 0) { s_m = 0; s_n[0] = 0; for (int a = 0; a < 3; ++a) { s_lo[0][a] = 31; s_hi[0][a] = 0; } }
    __syncthreads();
    for (uint32_t b = t; b < RTC_GIF_BINS; b += 1024) {
        const uint32_t c = cnt[b];
        if (c) {
            const uint32_t e = atomicAdd(&s_m, 1u);
            s_occ[e] = (uint16_t)b;
            s_owner[e] = 0;
            atomicAdd(&s_n[0], (unsigned long long)c);
            for (int a = 0; a < 3; ++a) { atomicMin(&s_lo[0][a], bin_coord(b, a)); atomicMax(&s_hi[0][a], bin_coord(b, a)); }
        }
    }
    __syncthreads();
    const uint32_t m = s_m;
    uint32_t nbox = 1;
    while (nbox < 256) {
        // the splittable box with the most pixels, ties to the lowest number: max of (n << 8) | (255 - box)
        unsigned long long key = 0;
        if (t < nbox && (s_hi[t][0] > s_lo[t][0] || s_hi[t][1] > s_lo[t][1] || s_hi[t][2] > s_lo[t][2]))
            key = (s_n[t] << 8) | (255u - t);
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(key, o, 64); key = u > key ? u : key; }
        if ((t & 63u) == 0) s_key[t >> 6] = key;
        __syncthreads();
        key = 0;
        for (int w = 0; w < 16; ++w) key = s_key[w] > key ? s_key[w] : key;
        if (key == 0) break; // uniform
        const uint32_t best = 255u - (uint32_t)(key & 255u);
        if (t == 0) {
            int axis = 0;
            for (int a = 1; a < 3; ++a)
                if (s_hi[best][a] - s_lo[best][a] > s_hi[best][axis] - s_lo[best][axis]) axis = a;
            s_axis = (uint32_t)axis;
            s_best = best;
        }
        if (t < 32) s_plane[t] = 0;
        __syncthreads();
        const int axis = (int)s_axis, lo = s_lo[best][axis], hi = s_hi[best][axis];
        for (uint32_t e = t; e < m; e += 1024)
            if (s_owner[e] == best) atomicAdd(&s_plane[bin_coord(s_occ[e], axis) - lo], (unsigned long long)cnt[s_occ[e]]);
        __syncthreads();
        if (t == 0) {
            const unsigned long long n = s_n[best];
            unsigned long long cum = 0;
            int cut = hi - 1;
            for (int q = lo; q < hi; ++q) {
                cum += s_plane[q - lo];
                if (2 * cum >= n) { cut = q; break; }
            }
            s_cut = cut;
            s_n[best] = 0;
            s_n[nbox] = 0;
            for (int a = 0; a < 3; ++a) { s_lo[best][a] = s_lo[nbox][a] = 31; s_hi[best][a] = s_hi[nbox][a] = 0; }
        }
        __syncthreads();
        const int cut = s_cut;
        for (uint32_t e = t; e < m; e += 1024) {
            if (s_owner[e] != best) continue;
            const uint32_t bin = s_occ[e];
            const uint32_t o = bin_coord(bin, axis) > cut ? nbox : best;
            s_owner[e] = (uint8_t)o;
            atomicAdd(&s_n[o], (unsigned long long)cnt[bin]);
            for (int a = 0; a < 3; ++a) { atomicMin(&s_lo[o][a], bin_coord(bin, a)); atomicMax(&s_hi[o][a], bin_coord(bin, a)); }
        }
        __syncthreads();
        ++nbox;
    }
    for (uint32_t e = t; e < m; e += 1024) lut[s_occ[e]] = s_owner[e];
    if (t == 0) info->nbox = nbox;
}

__global__ __launch_bounds__(256) void k_gif_box_sums(const uint8_t *rgb, size_t n, const GifInfo *info, const uint8_t *lut,
                                                      unsigned long long *boxsum) {
    if (info->nbox == 0) return;
    __shared__ unsigned long long s_sum[256][4];
    for (uint32_t k = threadIdx.x; k < 256 * 4; k += blockDim.x) (&s_sum[0][0])[k] = 0;
    __syncthreads();
    const size_t nthreads = (n + PX_PER_THREAD - 1) / PX_PER_THREAD;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * blockDim.x) {
        uint8_t px[24];
        const uint32_t m = load_px8(rgb, n, t * PX_PER_THREAD, px);
        uint32_t run_box = EMPTY, rn = 0, rr = 0, rg = 0, rb = 0;
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t r = px[3 * k], g = px[3 * k + 1], b = px[3 * k + 2];
            const uint32_t box = lut[bin_of(r, g, b)];
            if (box != run_box) {
                if (rn) {
                    atomicAdd(&s_sum[run_box][0], (unsigned long long)rn); atomicAdd(&s_sum[run_box][1], (unsigned long long)rr);
                    atomicAdd(&s_sum[run_box][2], (unsigned long long)rg); atomicAdd(&s_sum[run_box][3], (unsigned long long)rb);
                }
                run_box = box;
                rn = rr = rg = rb = 0;
            }
            ++rn; rr += r; rg += g; rb += b;
        }
        if (rn) {
            atomicAdd(&s_sum[run_box][0], (unsigned long long)rn); atomicAdd(&s_sum[run_box][1], (unsigned long long)rr);
            atomicAdd(&s_sum[run_box][2], (unsigned long long)rg); atomicAdd(&s_sum[run_box][3], (unsigned long long)rb);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 256 * 4; k += blockDim.x) {
        const unsigned long long v = (&s_sum[0][0])[k];
        if (v) atomicAdd(&boxsum[k], v);
    }
}

__global__ __launch_bounds__(256) void k_gif_map(const uint8_t *rgb, size_t n, const GifInfo *info, const uint32_t *pal32,
                                                 const unsigned long long *boxsum, uint8_t *idx, uint8_t *record) {
    __shared__ uint32_t s_pal[256];
    {
        const uint32_t e = threadIdx.x, nbox = info->nbox;
        uint32_t p = 0;
        if (nbox == 0) {
            p = pal32[e]; // exact colours (zero past the last: black)
        } else if (e < nbox) {
            const unsigned long long c = boxsum[4 * e];
            uint32_t ch[3];
            for (int k = 0; k < 3; ++k) ch[k] = (uint32_t)((2 * boxsum[4 * e + 1 + k] + c) / (2 * c));
            p = (ch[0] << 16) | (ch[1] << 8) | ch[2];
        }
        s_pal[e] = p;
        if (blockIdx.x == 0) {
            uint8_t *lct = record + RTC_GIF_LCT_OFFSET + 3 * e;
            lct[0] = (uint8_t)(p >> 16); lct[1] = (uint8_t)(p >> 8); lct[2] = (uint8_t)p;
        }
    }
    __syncthreads();
    const size_t nq = (n + 3) / 4;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
        const size_t i0 = 4 * q;
        const uint32_t m = (uint32_t)min((size_t)4, n - i0);
        int r[4], g[4], b[4], bd[4];
        uint32_t best[4];
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t i = k < m ? (uint32_t)k : 0u;
            r[k] = rgb[3 * (i0 + i)]; g[k] = rgb[3 * (i0 + i) + 1]; b[k] = rgb[3 * (i0 + i) + 2];
            bd[k] = 1 << 30; best[k] = 0;
        }
        for (uint32_t e = 0; e < 256; ++e) {
            const uint32_t p = s_pal[e];
            const int pr = (int)(p >> 16), pg = (int)((p >> 8) & 255u), pb = (int)(p & 255u);
            for (int k = 0; k < 4; ++k) {
                const int dr = r[k] - pr, dg = g[k] - pg, db = b[k] - pb;
                const int d = dr * dr + dg * dg + db * db;
                if (d < bd[k]) { bd[k] = d; best[k] = e; }
            }
        }
        for (uint32_t k = 0; k < m; ++k) idx[i0 + k] = (uint8_t)best[k];
    }
}

// One wave per segment. Every lane runs the same serial encoder (wave-uniform control flow, LDS reads broadcast), so that
// clearing the dictionary is 64 lanes wide; lane 0 stores the code words.
__global__ __launch_bounds__(64) void k_gif_lzw(const uint8_t *idx, size_t n, uint8_t *seg, uint32_t *seglen) {
    __shared__ uint32_t s_tab[HASH_SLOTS]; // (prefix << 20 | symbol << 12 | code); EMPTY = free
    __shared__ uint8_t s_sym[RTC_GIF_SEGMENT];
    const uint32_t lane = threadIdx.x, s = blockIdx.x;
    const size_t start = (size_t)s * RTC_GIF_SEGMENT;
    const uint32_t m = (uint32_t)min((size_t)RTC_GIF_SEGMENT, n - start);
    const bool first = s == 0, last = start + m == n;
    for (uint32_t j = lane; j < HASH_SLOTS; j += 64) s_tab[j] = EMPTY;
    for (uint32_t j = lane; j < m; j += 64) s_sym[j] = idx[start + j];
    __syncthreads();
    uint32_t *out = reinterpret_cast<uint32_t *>(seg + (size_t)s * RTC_GIF_SEG_BYTES);
    unsigned long long acc = 0;
    uint32_t bits = 0, words = 0;
    auto put = [&](uint32_t code, uint32_t width) {
        acc |= (unsigned long long)code << bits;
        bits += width;
        if (bits >= 32) {
            if (lane == 0) out[words] = (uint32_t)acc;
            ++words;
            acc >>= 32;
            bits -= 32;
        }
    };
    uint32_t width = 9, next = RTC_GIF_FIRST_CODE;
    if (first) put(RTC_GIF_CLEAR, width);
    uint32_t prefix = s_sym[0];
    for (uint32_t i = 1; i < m; ++i) {
        const uint32_t k = s_sym[i];
        const uint32_t key = (prefix << 8) | k;
        uint32_t h = (key * 2654435761u) >> 19;
        uint32_t e;
        while ((e = s_tab[h]) != EMPTY && (e >> 12) != key) h = (h + 1u) & (HASH_SLOTS - 1u);
        if (e != EMPTY) { prefix = e & 4095u; continue; }
        put(prefix, width);
        if (next < 4096) {
            s_tab[h] = (key << 12) | next;
            ++next;
            if (next > (1u << width) && width < 12) ++width;
        } else {
            put(RTC_GIF_CLEAR, width);
            __syncthreads();
            for (uint32_t j = lane; j < HASH_SLOTS; j += 64) s_tab[j] = EMPTY;
            __syncthreads();
            width = 9;
            next = RTC_GIF_FIRST_CODE;
        }
        prefix = k;
    }
    put(prefix, width);
    if (next < 4096) { ++next; if (next > (1u << width) && width < 12) ++width; }
    put(last ? RTC_GIF_EOI : RTC_GIF_CLEAR, width);
    if (lane == 0) {
        if (bits) out[words] = (uint32_t)acc;
        seglen[s] = words * 32u + bits;
    }
}

__global__ __launch_bounds__(256) void k_gif_offsets(const uint32_t *seglen, uint32_t nseg, unsigned long long *segoff, GifInfo *info,
                                                     uint8_t *record, uint32_t width, uint32_t height) {
    __shared__ uint32_t s_tmp[4];
    __shared__ unsigned long long s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nseg; base += 256) {
        const uint32_t j = base + threadIdx.x;
        const uint32_t v = j < nseg ? seglen[j] : 0u; // < 2^16 bits each: a 256-wide scan fits 32 bits
        const uint32_t incl = block_scan_256(v, s_tmp);
        const unsigned long long carry = s_carry;
        if (j < nseg) segoff[j] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == 255) s_carry = carry + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const unsigned long long T = s_carry, D = (T + 7) / 8;
        segoff[nseg] = T;
        info->data_bytes = D;
        info->record_bytes = RTC_GIF_RECORD_HEADER + D + (D + 254) / 255 + 1;
        const uint8_t hdr[18] = {0x21, 0xF9, 0x04, 0x00, (uint8_t)RTC_GIF_DELAY_CS, 0x00, 0x00, 0x00,
                                 0x2C, 0, 0, 0, 0, (uint8_t)width, (uint8_t)(width >> 8), (uint8_t)height, (uint8_t)(height >> 8), 0x87};
        for (int k = 0; k < 18; ++k) record[k] = hdr[k];
        record[RTC_GIF_RECORD_HEADER - 1] = 8;
    }
}

__global__ __launch_bounds__(256) void k_gif_pack(const uint8_t *seg, const unsigned long long *segoff, uint32_t nseg, const GifInfo *info,
                                                  uint8_t *record) {
    const unsigned long long D = info->data_bytes;
    uint8_t *body = record + RTC_GIF_RECORD_HEADER;
    for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < D; j += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long p = 8 * j;
        uint32_t lo = 0, hi = nseg - 1; // last segment with segoff <= p
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) / 2;
            if (segoff[mid] <= p) lo = mid; else hi = mid - 1;
        }
        const uint32_t s = lo;
        const unsigned long long q = p - segoff[s], len = segoff[s + 1] - segoff[s];
        const uint8_t *src = seg + (size_t)s * RTC_GIF_SEG_BYTES;
        uint32_t v = (uint32_t)src[q >> 3] | ((uint32_t)src[(q >> 3) + 1] << 8);
        v >>= (q & 7);
        const unsigned long long avail = len - q;
        if (avail < 8) {
            v &= (1u << avail) - 1u;
            if (s + 1 < nseg) v |= (uint32_t)seg[(size_t)(s + 1) * RTC_GIF_SEG_BYTES] << avail; // every segment has >= 18 bits
        }
        const unsigned long long at = j + j / 255 + 1;
        body[at] = (uint8_t)v;
        if (j % 255 == 0) body[at - 1] = (uint8_t)min(255ull, D - j);
        if (j == 0) body[D + (D + 254) / 255] = 0;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------

uint32_t segments(size_t n) { return (uint32_t)((n + RTC_GIF_SEGMENT - 1) / RTC_GIF_SEGMENT); }

} // namespace

rtc_status GifScratch::reserve(size_t n) {
    if (n <= px_cap) return RTC_OK;
    px_cap = 0;
    const size_t nseg = segments(n);
    const size_t dmax = nseg * (size_t)RTC_GIF_SEG_BYTES;
    record_cap = RTC_GIF_RECORD_HEADER + dmax + (dmax + 254) / 255 + 1;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_bitmap = 0, o_cnt = o_bitmap + up(4 * (size_t)BITMAP_WORDS), o_pal = o_cnt + up(4 * (size_t)RTC_GIF_BINS),
                 o_box = o_pal + up(4 * 256), o_end_clear = o_box + up(8 * 256 * 4);
    const size_t o_bc = o_end_clear, o_info = o_bc + up(4 * BITMAP_BLOCKS), o_lut = o_info + up(sizeof(GifInfo)),
                 o_seglen = o_lut + up(RTC_GIF_BINS), o_segoff = o_seglen + up(4 * nseg), o_idx = o_segoff + up(8 * (nseg + 1)),
                 o_seg = o_idx + up(n), o_rec = o_seg + up(nseg * (size_t)RTC_GIF_SEG_BYTES), total = o_rec + up(record_cap);
    const rtc_status st = this->block.reserve(total);
    if (st != RTC_OK) return st;
    uint8_t *block = this->block.get();
    bitmap = reinterpret_cast<uint32_t *>(block + o_bitmap);
    cnt = reinterpret_cast<uint32_t *>(block + o_cnt);
    pal32 = reinterpret_cast<uint32_t *>(block + o_pal);
    boxsum = reinterpret_cast<unsigned long long *>(block + o_box);
    clear_bytes = o_end_clear;
    blockcnt = reinterpret_cast<uint32_t *>(block + o_bc);
    info = block + o_info;
    lut = block + o_lut;
    seglen = reinterpret_cast<uint32_t *>(block + o_seglen);
    segoff = reinterpret_cast<unsigned long long *>(block + o_segoff);
    idx = block + o_idx;
    seg = block + o_seg;
    record = block + o_rec;
    px_cap = n;
    return RTC_OK;
}

// The whole chain for a width x height frame at d_rgb8 on `s`; the body is the frame's record (not the file), its length
// info->record_bytes.
rtc_status rtc_gif_enqueue(GifScratch &sc, const uint8_t *d_rgb8, uint32_t width, uint32_t height, hipStream_t s, RtcEncoded *e) {
    const size_t n = (size_t)width * height;
    const rtc_status r = sc.reserve(n);
    if (r != RTC_OK) return r;
    GifInfo *info = static_cast<GifInfo *>(sc.info);
    const uint32_t nseg = segments(n);
    const size_t px_threads = (n + PX_PER_THREAD - 1) / PX_PER_THREAD;
    const uint32_t grid_px = (uint32_t)std::min<size_t>(PX_BLOCKS, (px_threads + 1023) / 1024);
    const uint32_t grid_sum = (uint32_t)std::min<size_t>(1024, (px_threads + 255) / 256);
    const uint32_t grid_map = (uint32_t)std::min<size_t>(2048, ((n + 3) / 4 + 255) / 256);
    const uint32_t grid_pack = (uint32_t)std::min<size_t>(2048, (nseg * (size_t)RTC_GIF_SEG_BYTES + 255) / 256);
    HIP_TRY(hipMemsetAsync(sc.block.get(), 0, sc.clear_bytes, s));
    hipLaunchKernelGGL(k_gif_scan_pixels, dim3(grid_px), dim3(1024), 0, s, d_rgb8, n, sc.bitmap, sc.cnt);
    hipLaunchKernelGGL(k_gif_bitmap_count, dim3(BITMAP_BLOCKS), dim3(256), 0, s, sc.bitmap, sc.blockcnt);
    hipLaunchKernelGGL(k_gif_exact, dim3(BITMAP_BLOCKS), dim3(256), 0, s, sc.bitmap, sc.blockcnt, sc.pal32, info);
    hipLaunchKernelGGL(k_gif_median_cut, dim3(1), dim3(1024), 0, s, sc.cnt, info, sc.lut);
    hipLaunchKernelGGL(k_gif_box_sums, dim3(grid_sum), dim3(256), 0, s, d_rgb8, n, info, sc.lut, sc.boxsum);
    hipLaunchKernelGGL(k_gif_map, dim3(grid_map), dim3(256), 0, s, d_rgb8, n, info, sc.pal32, sc.boxsum, sc.idx, sc.record);
    hipLaunchKernelGGL(k_gif_lzw, dim3(nseg), dim3(64), 0, s, sc.idx, n, sc.seg, sc.seglen);
    hipLaunchKernelGGL(k_gif_offsets, dim3(1), dim3(256), 0, s, sc.seglen, nseg, sc.segoff, info, sc.record, width, height);
    hipLaunchKernelGGL(k_gif_pack, dim3(grid_pack), dim3(256), 0, s, sc.seg, sc.segoff, nseg, info, sc.record);
    HIP_TRY(hipGetLastError());
    e->d_body = sc.record;
    e->d_len = &info->record_bytes;
    e->cap = sc.record_cap;
    e->min_len = RTC_GIF_RECORD_HEADER + 1; // at least the header and the block terminator
    return RTC_OK;
}
