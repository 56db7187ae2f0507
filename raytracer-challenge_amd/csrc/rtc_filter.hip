// rtc_filter.hip — [device] the edge-aware à-trous filter of include/rtc.h ("edge-aware filter") on gfx950, and the two
// per-pixel kernels beside it. The arithmetic is rtc_filter.h's, which host_filter.cpp evaluates too: the bytes are the host
// statement's.
//
//   k_atrous<CH, SAME>   one pass (step s) over a plane of CH values per pixel; one launch per pass. Per pixel a pass reads 25
//                        taps of 52 B of guides and 8*CH B of values, nearly all of them shared with the pixel's neighbours, so
//                        a workgroup stages its tile plus the two-tap halo in LDS once and every tap is an LDS read:
//                          tile     32 x 8 pixels, one per lane of 256 threads; with the halo 36 x 12 = 432 entries;
//                          layout   SoA: six f64 planes (point xyz, normal xyz), CH f64 value planes, one i32 index plane —
//                                   (6 + CH) * 3456 + 1728 B = 25.9 kB (CH = 1) or 32.8 kB (CH = 3): four workgroups of a
//                                   CU's 160 kB, 16 waves;
//                          banks    a tap is one ds_read_b64 per plane at [row][lx + const]: the 32 lanes of a half-wave — the
//                                   group whose addresses can conflict — are the 32 consecutive doubles of ONE tile row, 256
//                                   contiguous bytes, all 64 banks once, whatever the row pitch. (A 16 x 16 tile would put two
//                                   rows, 20 entries apart, in a half-wave: the second row's last four entries meet the first row's first
//                                   four banks, a 2-way conflict on every read.) The i32
//                                   plane is read 32 consecutive words at a time.
//                          halo     an entry outside the image gets index = -1: the image edge and a miss take the same path
//                                   and the tap loop, fully unrolled, has no bounds test.
//                          step     for s > 1 a workgroup owns pixels of ONE residue class (x mod s, y mod s): in that class
//                                   the taps are again neighbours, so the tile, the halo and all LDS code are those of s = 1
//                                   and only the global addresses carry the stride.
//                        A skipped tap adds nothing (the host's `continue`): its weight and value are computed from whatever
//                        the entry holds and dropped by the test, never added.
//   k_counts_to_fraction, k_apply_occlusion   one thread per pixel (k_apply_ao's shape).
#include <hip/hip_runtime.h>

#include "rtc.h"
#include "rtc_filter.h"
#include "rtc_internal.h"

namespace {

constexpr uint32_t TW = 32, TH = 8, HALO = 2, LW = TW + 2 * HALO, LH = TH + 2 * HALO, LN = LW * LH, THREADS = TW * TH;

template <uint32_t CH, bool SAME>
__global__ void __launch_bounds__(THREADS) k_atrous(AtrousArgs a) {
    __shared__ double s_g[6][LN]; // point x, y, z, normal x, y, z
    __shared__ double s_v[CH][LN];
    __shared__ int32_t s_i[LN];
    const uint32_t s = a.step;
    const uint32_t bx = blockIdx.x % a.grid_x, by = blockIdx.x / a.grid_x;
    const uint32_t rx = bx % s, ry = by % s;               // the residue class
    const uint32_t tx0 = (bx / s) * TW, ty0 = (by / s) * TH; // the tile's origin among the class's pixels
    // the class has ceil((W - rx) / s) columns; a tile past them (a narrow image, a late class) has nothing to do
    const uint32_t wsub = rx < a.width ? (a.width - rx + s - 1u) / s : 0u, hsub = ry < a.height ? (a.height - ry + s - 1u) / s : 0u;
    if (tx0 >= wsub || ty0 >= hsub) return; // the whole workgroup
    for (uint32_t e = threadIdx.x; e < LN; e += THREADS) {
        const uint32_t lx = e % LW, ly = e / LW;
        const int64_t sx = (int64_t)tx0 + lx - HALO, sy = (int64_t)ty0 + ly - HALO;
        const bool inside = sx >= 0 && sy >= 0 && sx < (int64_t)wsub && sy < (int64_t)hsub;
        int32_t idx = -1;
        double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, v[CH];
#pragma unroll
        for (uint32_t c = 0; c < CH; ++c) v[c] = 0.0;
        if (inside) {
            const size_t q = ((size_t)ry + (size_t)sy * s) * a.width + ((size_t)rx + (size_t)sx * s);
            idx = a.index[q];
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) {
                g[c] = a.point[3u * q + c];
                g[3u + c] = a.normal[3u * q + c];
            }
#pragma unroll
            for (uint32_t c = 0; c < CH; ++c) v[c] = a.src[CH * q + c];
        }
        s_i[e] = idx;
#pragma unroll
        for (uint32_t c = 0; c < 6u; ++c) s_g[c][e] = g[c];
#pragma unroll
        for (uint32_t c = 0; c < CH; ++c) s_v[c][e] = v[c];
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % TW, ly = threadIdx.x / TW;
    const uint32_t sx = tx0 + lx, sy = ty0 + ly;
    if (sx >= wsub || sy >= hsub) return;
    const uint32_t ctr = (ly + HALO) * LW + lx + HALO;
    const int32_t ip = s_i[ctr];
    double acc[CH], wsum = 0.0;
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) acc[c] = 0.0;
    if (ip >= 0) {
        const double ppx = s_g[0][ctr], ppy = s_g[1][ctr], ppz = s_g[2][ctr], npx = s_g[3][ctr], npy = s_g[4][ctr], npz = s_g[5][ctr];
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const uint32_t o = ctr + (uint32_t)((j - 2) * (int)LW + (i - 2));
                const int32_t iq = s_i[o];
                const bool ok = iq >= 0 && (!SAME || iq == ip);
                const double w = rtc_filter_weight(rtc_filter_h(j) * rtc_filter_h(i), a.inv, a.squarings, npx, npy, npz, ppx, ppy, ppz, s_g[3][o],
                                                   s_g[4][o], s_g[5][o], s_g[0][o], s_g[1][o], s_g[2][o]);
                if (ok && w > 0.0) {
#pragma unroll
                    for (uint32_t c = 0; c < CH; ++c) acc[c] = acc[c] + w * s_v[c][o];
                    wsum = wsum + w;
                }
            }
    }
    const size_t p = ((size_t)ry + (size_t)sy * s) * a.width + ((size_t)rx + (size_t)sx * s);
#pragma unroll
    for (uint32_t c = 0; c < CH; ++c) a.dst[CH * p + c] = wsum > 0.0 ? rtc_filter_quotient(acc[c], wsum) : s_v[c][ctr];
}

__global__ void __launch_bounds__(256) k_counts_to_fraction(const uint16_t *__restrict__ counts, size_t px, uint32_t n, double *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= px) return;
    out[i] = rtc_filter_fraction(counts[i], n);
}

__global__ void __launch_bounds__(256) k_apply_occlusion(double *__restrict__ rgb, const double *__restrict__ occ, size_t px, double strength) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= px) return;
    const double o = occ[i];
    rgb[3u * i] = rtc_filter_occlude(rgb[3u * i], o, strength);
    rgb[3u * i + 1u] = rtc_filter_occlude(rgb[3u * i + 1u], o, strength);
    rgb[3u * i + 2u] = rtc_filter_occlude(rgb[3u * i + 2u], o, strength);
}

} // namespace

extern "C" hipError_t rtc_launch_atrous(const AtrousArgs *args, uint32_t channels, bool same, hipStream_t stream) {
    AtrousArgs a = *args;
    if (a.width == 0u || a.height == 0u) return hipSuccess;
    if (a.step == 0u || (channels != 1u && channels != 3u)) return hipErrorInvalidValue;
    // per axis: `step` classes, each with the tiles of its ceil(size / step) pixels (the later classes may have one pixel fewer)
    const uint64_t gx = (uint64_t)a.step * (((a.width + a.step - 1u) / a.step + TW - 1u) / TW);
    const uint64_t gy = (uint64_t)a.step * (((a.height + a.step - 1u) / a.step + TH - 1u) / TH);
    if (gx > 0x7fffffffull || gy > 0x7fffffffull || gx * gy > 0x7fffffffull) return hipErrorInvalidValue;
    a.grid_x = (uint32_t)gx;
    const dim3 grid((uint32_t)(gx * gy)), block(THREADS);
    if (channels == 1u && same) hipLaunchKernelGGL((k_atrous<1, true>), grid, block, 0, stream, a);
    else if (channels == 1u) hipLaunchKernelGGL((k_atrous<1, false>), grid, block, 0, stream, a);
    else if (same) hipLaunchKernelGGL((k_atrous<3, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_atrous<3, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_counts_to_fraction(const uint16_t *counts, size_t px, uint32_t n, double *out, hipStream_t stream) {
    if (px == 0) return hipSuccess;
    const size_t blocks = (px + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_counts_to_fraction, dim3((uint32_t)blocks), dim3(256), 0, stream, counts, px, n, out);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_apply_occlusion(double *rgb, const double *occ, size_t px, double strength, hipStream_t stream) {
    if (px == 0) return hipSuccess;
    const size_t blocks = (px + 255u) / 256u;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apply_occlusion, dim3((uint32_t)blocks), dim3(256), 0, stream, rgb, occ, px, strength);
    return hipGetLastError();
}
