// rtc_post.hip — [device] the post-processing passes of include/rtc.h ("exposure, tone mapping and bloom") on gfx950. The
// per-pixel arithmetic is rtc_post.h's, which host_post.cpp evaluates too: the bytes are the host statement's. No kernel calls
// exp, log or pow.
//
//   k_lum_pixels    level 0 of the statistics: a workgroup of 256 threads owns 256 consecutive pixels — one block of the
//   k_lum_records   host's tree — and reduces their contributions in LDS with the host's steps (s = 128 .. 1, v[i] + v[i+s]);
//                   k_lum_records does the same over 256 consecutive block results of the level before. One launch per
//                   level; the level that has one workgroup writes the record itself. Values past the end are the padding
//                   (+0.0, 0.0, 0) and lanes i >= s are never read again, so every sum is the host's.
//   k_tonemap       one thread per pixel. m and inv_w2 are derived per thread from the record in device memory (uniform
//                   scalar loads and two divisions): no one-thread launch in between and no host wait.
//   k_bloom_h       one workgroup per segment of 256 pixels of ONE row: the segment and its R-pixel halo are staged in LDS
//                   as three f64 planes with the bright pass applied once, at staging; a tap is then one ds_read_b64 per
//                   plane at [lane + k] (lds_f64 below keeps the compiler from pairing them). The 32 lanes of a half-wave — the group whose addresses can conflict — read 32
//                   consecutive doubles, all 64 banks once (rtc_filter.hip has the rule). Entries outside the image are
//                   written as +0.0, so the tap loop has no bounds test. H goes to the context's plane as three planes
//                   (SoA), which k_bloom_v stages with unit-stride loads.
//   k_bloom_v       a tile of 32 x 64 pixels, 256 threads, eight outputs per thread, with R halo rows of H above and below
//                   in LDS: (64 + 2R) rows of 32 doubles, 32 kB at R = 32, for ONE channel; the three channels are three
//                   sweeps through the same LDS. All three at once would be 96 kB, one workgroup of a CU's 160 kB (4 waves);
//                   one per sweep leaves room for five (20 waves) at the cost of two more barrier pairs per tile; the sweeps' results stay
//                   in registers (24 doubles per thread) and a pixel's three channels are stored together. A
//                   half-wave is the 32 doubles of one LDS row, whatever k: conflict-free again. Writes the composite; reads
//                   C only at its own pixel, so d_out may be d_in.
// The weights travel in the kernel arguments (65 doubles) and are read by uniform index: scalar loads.
#include <hip/hip_runtime.h>

#include "rtc.h"
#include "rtc_internal.h"
#include "rtc_post.h"

namespace {

constexpr uint32_t B = RTC_POST_BLOCK;

// the tree of one block: thread 0 stores the block's record
__device__ inline void lum_block(double y, double mx, unsigned long long cnt, rtc_luminance *out) {
    __shared__ double s_sum[B], s_max[B];
    __shared__ unsigned long long s_cnt[B];
    const uint32_t i = threadIdx.x;
    s_sum[i] = y;
    s_max[i] = mx;
    s_cnt[i] = cnt;
    __syncthreads();
    for (uint32_t s = B / 2u; s >= 1u; s /= 2u) {
        if (i < s) {
            s_sum[i] = s_sum[i] + s_sum[i + s];
            const double a = s_max[i], b = s_max[i + s];
            s_max[i] = b > a ? b : a;
            s_cnt[i] = s_cnt[i] + s_cnt[i + s];
        }
        __syncthreads();
    }
    if (i == 0u) {
        rtc_luminance r;
        r.max = s_max[0];
        r.sum = s_sum[0];
        r.count = s_cnt[0];
        out[blockIdx.x] = r;
    }
}

__global__ void __launch_bounds__(B) k_lum_pixels(const double *__restrict__ rgb, size_t n, rtc_luminance *__restrict__ out) {
    const size_t p = (size_t)blockIdx.x * B + threadIdx.x;
    double y = 0.0;
    unsigned long long cnt = 0ull;
    if (p < n) {
        const double l = rtc_post_luminance(rgb[3u * p], rgb[3u * p + 1u], rgb[3u * p + 2u]);
        if (rtc_post_contributes(l)) {
            y = l;
            cnt = 1ull;
        }
    }
    lum_block(y, y, cnt, out); // a contribution is its own maximum; 0.0 otherwise, where the maximum starts
}

__global__ void __launch_bounds__(B) k_lum_records(const rtc_luminance *__restrict__ in, size_t n, rtc_luminance *__restrict__ out) {
    const size_t p = (size_t)blockIdx.x * B + threadIdx.x;
    double y = 0.0, mx = 0.0;
    unsigned long long cnt = 0ull;
    if (p < n) {
        y = in[p].sum;
        mx = in[p].max;
        cnt = in[p].count;
    }
    lum_block(y, mx, cnt, out);
}

__global__ void __launch_bounds__(256) k_tonemap(const double *in, double *out, size_t n, double exposure, double white, uint32_t curve,
                                                 uint32_t flags, const rtc_luminance *__restrict__ stats) {
    const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    double m, inv_w2;
    rtc_post_resolve(exposure, white, flags, stats, &m, &inv_w2);
    double c[3] = {in[3u * p], in[3u * p + 1u], in[3u * p + 2u]};
    rtc_post_tonemap_pixel(c, curve, m, inv_w2);
    out[3u * p] = c[0];
    out[3u * p + 1u] = c[1];
    out[3u * p + 2u] = c[2];
}

// How the tap loops read LDS. A plain load of [e] and one of [e + 1] (k_bloom_h) or of rows k and k + 1 (k_bloom_v) are merged by
// the compiler into ds_read2_b64, which the LDS serves at half the rate of ds_read_b64 (8 against 2 cycles per wave instruction
// for twice the data, bank modulus 32). A volatile load is never merged: one ds_read_b64 per tap and plane, issued in order and
// still in flight together. The pointer names the LDS address space itself: the compiler does not infer it for a volatile
// access and would emit flat loads. -DRTC_POST_PAIRED_READS=1 gives the plain loads back (A/B, tools/post_cost.py).
#ifndef RTC_POST_PAIRED_READS
#define RTC_POST_PAIRED_READS 0
#endif
#if RTC_POST_PAIRED_READS
using lds_f64 = const double;
#else
using lds_f64 = const volatile __attribute__((address_space(3))) double;
#endif

constexpr uint32_t HSEG = 256, HLW = HSEG + 2u * RTC_MAX_BLOOM_RADIUS; // k_bloom_h: pixels per workgroup, LDS entries per plane
constexpr uint32_t VW = 32, VH = 64, VROWS = 8, VPER = VH / VROWS;     // k_bloom_v: the tile, rows per sweep of the threads, outputs per thread

__global__ void __launch_bounds__(HSEG) k_bloom_h(BloomArgs a) {
    __shared__ double s_b[3][HLW];
    const uint32_t r = a.radius, segs = a.grid_x;
    const uint32_t y = blockIdx.x / segs, x0 = (blockIdx.x % segs) * HSEG;
    const double *row = a.in + 3u * (size_t)y * a.width;
    for (uint32_t e = threadIdx.x; e < HSEG + 2u * r; e += HSEG) {
        const int64_t x = (int64_t)x0 + e - r;
        double b[3] = {0.0, 0.0, 0.0};
        if (x >= 0 && x < (int64_t)a.width) {
            const double c[3] = {row[3u * (size_t)x], row[3u * (size_t)x + 1u], row[3u * (size_t)x + 2u]};
            rtc_post_bright(c, a.threshold, b);
        }
        s_b[0][e] = b[0];
        s_b[1][e] = b[1];
        s_b[2][e] = b[2];
    }
    __syncthreads();
    const uint32_t x = x0 + threadIdx.x;
    if (x >= a.width) return;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    lds_f64 *b0 = (lds_f64 *)(s_b[0] + threadIdx.x), *b1 = (lds_f64 *)(s_b[1] + threadIdx.x), *b2 = (lds_f64 *)(s_b[2] + threadIdx.x); // [k]: pixel x + k - r
    for (uint32_t k = 0; k <= 2u * r; ++k) {
        const double w = a.w[k];
        acc0 = acc0 + (w * b0[k]);
        acc1 = acc1 + (w * b1[k]);
        acc2 = acc2 + (w * b2[k]);
    }
    const size_t n = (size_t)a.width * a.height, p = (size_t)y * a.width + x;
    a.hor[p] = acc0;
    a.hor[n + p] = acc1;
    a.hor[2u * n + p] = acc2;
}

__global__ void __launch_bounds__(VW * VROWS) k_bloom_v(BloomArgs a) {
    extern __shared__ double s_h[]; // (VH + 2r) rows of VW doubles
    const uint32_t r = a.radius, rows = VH + 2u * r;
    const uint32_t tx0 = (blockIdx.x % a.grid_x) * VW, ty0 = (blockIdx.x / a.grid_x) * VH;
    const uint32_t lx = threadIdx.x % VW, ly = threadIdx.x / VW;
    const uint32_t x = tx0 + lx;
    const size_t n = (size_t)a.width * a.height;
    // acc[j][c]: channel c of output row ly + 8j. Every thread of the tile computes all of them — the LDS rows exist for the
    // whole tile — and only the stores are bounded by the image. Both loops are unrolled, so the array lives in registers.
    double acc[VPER][3];
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
        const double *plane = a.hor + (size_t)c * n;
        for (uint32_t row = ly; row < rows; row += VROWS) {
            const int64_t y = (int64_t)ty0 + row - r;
            double v = 0.0;
            if (x < a.width && y >= 0 && y < (int64_t)a.height) v = plane[(size_t)y * a.width + x];
            s_h[row * VW + lx] = v;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < VPER; ++j) {
            lds_f64 *col = (lds_f64 *)(s_h + (ly + j * VROWS) * VW + lx); // output row oy = ly + 8j: the taps are LDS rows oy .. oy + 2r
            double t = 0.0;
            for (uint32_t k = 0; k <= 2u * r; ++k) t = t + (a.w[k] * col[k * VW]);
            acc[j][c] = t;
        }
        __syncthreads(); // the next sweep overwrites the plane
    }
    // the composite, a pixel's three channels together: 24 contiguous bytes per lane (one channel per sweep would write 8 of every 24)
    if (x >= a.width) return;
#pragma unroll
    for (uint32_t j = 0; j < VPER; ++j) {
        const uint32_t y = ty0 + ly + j * VROWS;
        if (y >= a.height) continue;
        const size_t q = 3u * ((size_t)y * a.width + x);
        const double c0 = a.in[q], c1 = a.in[q + 1u], c2 = a.in[q + 2u];
        a.out[q] = rtc_post_composite(c0, a.strength, acc[j][0]);
        a.out[q + 1u] = rtc_post_composite(c1, a.strength, acc[j][1]);
        a.out[q + 2u] = rtc_post_composite(c2, a.strength, acc[j][2]);
    }
}

} // namespace

extern "C" hipError_t rtc_launch_luminance(const double *rgb, size_t n, rtc_luminance *scratch, rtc_luminance *out, hipStream_t stream) {
    // level 0 has `blocks` results, level 1 ceil(blocks / 256), ...; level l writes scratch region l % 2 (region 0: `blocks`
    // records from scratch[0], region 1 behind it), except the last, which writes `out`
    size_t len = n == 0 ? 1u : (n + B - 1u) / B;
    if (len > RTC_POST_MAX_BLOCKS) return hipErrorInvalidValue;
    const size_t region1 = len;
    rtc_luminance *dst = len == 1u ? out : scratch;
    hipLaunchKernelGGL(k_lum_pixels, dim3((uint32_t)len), dim3(B), 0, stream, rgb, n, dst);
    for (uint32_t level = 1; len > 1u; ++level) {
        const size_t next = (len + B - 1u) / B;
        const rtc_luminance *src = dst;
        dst = next == 1u ? out : (level % 2u ? scratch + region1 : scratch);
        hipLaunchKernelGGL(k_lum_records, dim3((uint32_t)next), dim3(B), 0, stream, src, len, dst);
        len = next;
    }
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_tonemap(const double *in, double *out, size_t n, const rtc_tonemap *spec, const rtc_luminance *stats,
                                         hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255u) / 256u;
    if (blocks > RTC_POST_MAX_BLOCKS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tonemap, dim3((uint32_t)blocks), dim3(256), 0, stream, in, out, n, spec->exposure, spec->white, spec->curve, spec->flags,
                       stats);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_bloom(const BloomArgs *args, hipStream_t stream) {
    BloomArgs a = *args;
    if (a.width == 0u || a.height == 0u) return hipSuccess;
    if (a.radius < 1u || a.radius > RTC_MAX_BLOOM_RADIUS) return hipErrorInvalidValue;
    const uint64_t segs = ((uint64_t)a.width + HSEG - 1u) / HSEG;
    const uint64_t gx = ((uint64_t)a.width + VW - 1u) / VW, gy = ((uint64_t)a.height + VH - 1u) / VH;
    if (segs * a.height > RTC_POST_MAX_BLOCKS || gx * gy > RTC_POST_MAX_BLOCKS) return hipErrorInvalidValue; // before anything is launched
    a.grid_x = (uint32_t)segs;
    hipLaunchKernelGGL(k_bloom_h, dim3((uint32_t)(segs * a.height)), dim3(HSEG), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e; // no H plane: nothing may be composited from it
    a.grid_x = (uint32_t)gx;
    const size_t lds = (size_t)(VH + 2u * a.radius) * VW * sizeof(double);
    hipLaunchKernelGGL(k_bloom_v, dim3((uint32_t)(gx * gy)), dim3(VW * VROWS), lds, stream, a);
    return hipGetLastError();
}
