// rtc_adaptive.hip — [device] the kernels of edge-adaptive anti-aliasing (include/rtc.h, "edge-adaptive anti-aliasing") on
// gfx950, everything between the one-sample frame and the probe launch that traces the extra rays. The arithmetic is
// rtc_adaptive.h's, which host_adaptive.cpp evaluates too: the bytes are the host statement's.
//
//   k_aa_mask    the mask and, per tile, how many of its bytes are 1. One workgroup per 32 x 8 tile, one pixel per lane of 256
//                threads; the tile plus its one-pixel halo, 34 x 10 = 340 entries, is staged in LDS once as three f64 planes
//                (r, g, b: 8160 B), so each colour is loaded once and not five times.
//                  banks   a comparison reads one ds_read_b64 per plane at [row][lx + const]: the 32 lanes of a half-wave —
//                          the group whose addresses can conflict — are the 32 consecutive doubles of ONE tile row, 256
//                          contiguous bytes, all 64 banks once, whatever the row pitch (k_atrous's layout).
//                  halo    an entry outside the rendered area R (outside the image; RTC_MODE_RENDER's last row and column) is
//                          NaN: its distance to anything is NaN and compares false, so the four comparisons have no bounds
//                          test, and a lane whose own pixel is outside R flags nothing.
//                The count is the sum of the four waves' ballots.
//   k_aa_scan    the exclusive prefix sum of the tile counts, by ONE workgroup that walks the counts 256 at a time (8 100 tiles
//                at 1080p: 32 rounds). A pixel's place in the list is then a function of the mask alone — no atomic hands out
//                slots — so two runs trace the same rays in the same waves.
//   k_aa_list    one workgroup per tile again: the flagged pixels of the tile, row-major, at the tile's offset; a lane's slot
//                is the count of flagged lanes in front of it (ballot and popcount in its wave, the earlier waves' totals
//                through LDS). A tile without flagged pixels leaves at once.
//   k_aa_rays    one thread per ray of a chunk: rtc_camera_ray_for_pixel for the sample's offsets, {origin, direction}.
//   k_aa_resolve one thread per pixel of a chunk: the n colours summed in sample order, divided once, stored to the canvas.
#include <hip/hip_runtime.h>

#include "rtc.h"
#include "rtc_adaptive.h"
#include "rtc_internal.h"

namespace {

constexpr uint32_t TW = RTC_AA_TILE_W, TH = RTC_AA_TILE_H, LW = TW + 2, LH = TH + 2, LN = LW * LH, THREADS = TW * TH, WAVES = THREADS / 64;

__global__ void __launch_bounds__(THREADS) k_aa_mask(const double *__restrict__ rgb, uint32_t width, uint32_t height, uint32_t rw, uint32_t rh,
                                                      uint32_t tiles_x, double threshold, unsigned char *__restrict__ mask,
                                                      uint32_t *__restrict__ counts) {
    __shared__ double s_c[3][LN];
    __shared__ uint32_t s_n[WAVES];
    const uint32_t tx0 = (blockIdx.x % tiles_x) * TW, ty0 = (blockIdx.x / tiles_x) * TH;
    for (uint32_t e = threadIdx.x; e < LN; e += THREADS) {
        const uint32_t ex = e % LW, ey = e / LW;
        const int64_t sx = (int64_t)tx0 + ex - 1, sy = (int64_t)ty0 + ey - 1;
        double c0 = __builtin_nan(""), c1 = c0, c2 = c0;
        if (sx >= 0 && sy >= 0 && sx < (int64_t)rw && sy < (int64_t)rh) {
            const size_t q = 3u * ((size_t)sy * width + (size_t)sx);
            c0 = rgb[q];
            c1 = rgb[q + 1u];
            c2 = rgb[q + 2u];
        }
        s_c[0][e] = c0;
        s_c[1][e] = c1;
        s_c[2][e] = c2;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % TW, ly = threadIdx.x / TW;
    const uint32_t x = tx0 + lx, y = ty0 + ly;
    const uint32_t ctr = (ly + 1u) * LW + lx + 1u;
    const double pr = s_c[0][ctr], pg = s_c[1][ctr], pb = s_c[2][ctr];
    bool flag = false;
    const uint32_t nb[4] = {ctr - 1u, ctr + 1u, ctr - LW, ctr + LW}; // left, right, up, down
#pragma unroll
    for (int k = 0; k < 4; ++k) flag = flag || rtc_aa_distance(pr, pg, pb, s_c[0][nb[k]], s_c[1][nb[k]], s_c[2][nb[k]]) > threshold;
    const bool inside = x < width && y < height;
    if (inside) mask[(size_t)y * width + x] = flag ? 1u : 0u;
    const uint32_t n = (uint32_t)__popcll(__ballot(inside && flag));
    if (threadIdx.x % 64u == 0u) s_n[threadIdx.x / 64u] = n;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t sum = 0u;
#pragma unroll
        for (uint32_t k = 0; k < WAVES; ++k) sum += s_n[k];
        counts[blockIdx.x] = sum;
    }
}

__global__ void __launch_bounds__(THREADS) k_aa_scan(const uint32_t *__restrict__ counts, uint32_t tiles, uint32_t *__restrict__ offsets,
                                                      uint32_t *__restrict__ total) {
    __shared__ uint32_t s_w[WAVES];
    const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < tiles; base += THREADS) { // (uniform bounds: every thread takes every round)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < tiles ? counts[i] : 0u;
        uint32_t inc = v; // inclusive sum within the wave
#pragma unroll
        for (uint32_t d = 1u; d < 64u; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63u) s_w[wave] = inc;
        __syncthreads();
        uint32_t before = 0u, round = 0u;
#pragma unroll
        for (uint32_t k = 0; k < WAVES; ++k) {
            if (k < wave) before += s_w[k];
            round += s_w[k];
        }
        if (i < tiles) offsets[i] = carry + before + (inc - v);
        carry += round;
        __syncthreads(); // s_w is written again in the next round
    }
    if (threadIdx.x == 0u) *total = carry;
}

__global__ void __launch_bounds__(THREADS) k_aa_list(const unsigned char *__restrict__ mask, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                      const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                      uint32_t *__restrict__ list) {
    __shared__ uint32_t s_n[WAVES];
    if (counts[blockIdx.x] == 0u) return; // the whole workgroup
    const uint32_t x = (blockIdx.x % tiles_x) * TW + threadIdx.x % TW, y = (blockIdx.x / tiles_x) * TH + threadIdx.x / TW;
    const size_t p = (size_t)y * width + x;
    const bool flag = x < width && y < height && mask[p] != 0u;
    const unsigned long long votes = __ballot(flag);
    const uint32_t lane = threadIdx.x % 64u, wave = threadIdx.x / 64u;
    if (lane == 0u) s_n[wave] = (uint32_t)__popcll(votes);
    __syncthreads();
    if (!flag) return;
    uint32_t slot = offsets[blockIdx.x] + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
#pragma unroll
    for (uint32_t k = 0; k < WAVES; ++k)
        if (k < wave) slot += s_n[k];
    list[slot] = (uint32_t)p;
}

__global__ void __launch_bounds__(256) k_aa_rays(AaRayArgs a) {
    const uint32_t n = a.usteps * a.vsteps;
    const size_t r = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= (size_t)a.pixels * n) return;
    const uint32_t p = a.list[r / n], k = (uint32_t)(r % n);
    const uint32_t x = p % a.width, y = p / a.width;
    double dir[3];
    rtc_aa_direction(a.half_width, a.half_height, a.pixel_size, a.vinv, a.origin, x, rtc_aa_offset(k % a.usteps, a.usteps), y,
                     rtc_aa_offset(k / a.usteps, a.vsteps), dir);
    double *o = a.rays + 6u * r;
    o[0] = a.origin[0];
    o[1] = a.origin[1];
    o[2] = a.origin[2];
    o[3] = dir[0];
    o[4] = dir[1];
    o[5] = dir[2];
}

__global__ void __launch_bounds__(256) k_aa_resolve(const uint32_t *__restrict__ list, const double *__restrict__ colors, uint32_t pixels, uint32_t n,
                                                     double *__restrict__ rgb) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const double *c = colors + 3u * (size_t)i * n;
    double r = 0.0, g = 0.0, b = 0.0; // Color::average_over: three sums from 0.0 in sample order, one division each
    for (uint32_t k = 0; k < n; ++k) {
        r = r + c[3u * k];
        g = g + c[3u * k + 1u];
        b = b + c[3u * k + 2u];
    }
    double *o = rgb + 3u * (size_t)list[i];
    o[0] = r / (double)n;
    o[1] = g / (double)n;
    o[2] = b / (double)n;
}

uint32_t tiles_of(uint32_t width, uint32_t height, uint32_t *tiles_x) {
    *tiles_x = (width + TW - 1u) / TW;
    return *tiles_x * ((height + TH - 1u) / TH);
}

} // namespace

// (the callers keep width*height below 2^31: the tile count and every pixel index fit in 32 bits)
extern "C" hipError_t rtc_launch_aa_mask(const double *rgb, uint32_t width, uint32_t height, uint32_t mode, double threshold, unsigned char *mask,
                                         uint32_t *counts, hipStream_t stream) {
    if (width == 0u || height == 0u) return hipSuccess;
    if ((uint64_t)width * height > 0x7fffffffull) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t tiles = tiles_of(width, height, &tiles_x);
    const uint32_t rw = mode == RTC_MODE_RENDER ? width - 1u : width, rh = mode == RTC_MODE_RENDER ? height - 1u : height;
    hipLaunchKernelGGL(k_aa_mask, dim3(tiles), dim3(THREADS), 0, stream, rgb, width, height, rw, rh, tiles_x, threshold, mask, counts);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_aa_scan(const uint32_t *counts, uint32_t tiles, uint32_t *offsets, uint32_t *total, hipStream_t stream) {
    hipLaunchKernelGGL(k_aa_scan, dim3(1), dim3(THREADS), 0, stream, counts, tiles, offsets, total);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_aa_list(const unsigned char *mask, uint32_t width, uint32_t height, const uint32_t *counts, const uint32_t *offsets,
                                         uint32_t *list, hipStream_t stream) {
    if (width == 0u || height == 0u) return hipSuccess;
    if ((uint64_t)width * height > 0x7fffffffull) return hipErrorInvalidValue;
    uint32_t tiles_x;
    const uint32_t tiles = tiles_of(width, height, &tiles_x);
    hipLaunchKernelGGL(k_aa_list, dim3(tiles), dim3(THREADS), 0, stream, mask, width, height, tiles_x, counts, offsets, list);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_aa_rays(const AaRayArgs *args, hipStream_t stream) {
    const uint64_t rays = (uint64_t)args->pixels * args->usteps * args->vsteps;
    if (rays == 0u) return hipSuccess;
    const uint64_t blocks = (rays + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_aa_rays, dim3((uint32_t)blocks), dim3(256), 0, stream, *args);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_aa_resolve(const uint32_t *list, const double *colors, uint32_t pixels, uint32_t n, double *rgb, hipStream_t stream) {
    if (pixels == 0u || n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_aa_resolve, dim3((pixels + 255u) / 256u), dim3(256), 0, stream, list, colors, pixels, n, rgb);
    return hipGetLastError();
}
