// rtc_resize.hip — [device] the two passes of the resize (include/rtc.h, "resizing f64 canvases") on gfx950. No kernel
// evaluates a filter: the tables are the host's (host_resize.cpp), one record {first, count} and one row of `taps` weights
// per output, and a kernel only multiplies and adds, in tap order, without contraction: the bytes are the host statement's.
//
//   k_resize_v     a thread owns one value (x, channel) of RTC_RESIZE_V_ROWS consecutive output rows; a workgroup 256
//                  consecutive values of them. The rows' records and weights have uniform addresses — they depend on
//                  blockIdx alone — so they come through scalar loads and every test on them is a scalar branch. The thread
//                  walks the source rows from the first tap of its first output row to the last tap of its last, loads
//                  each ONCE (256 consecutive doubles per workgroup: coalesced, no LDS) and adds its product to every
//                  output row whose taps cover it: each output still sums its own taps in tap order, from 0.0. Halving
//                  with LANCZOS3 reads 20 rows for four outputs where one output row per thread reads 52. A small output
//                  takes the one-row instantiation instead (rtc_resize_plan): four times the workgroups, each with a
//                  quarter of the walk.
//   k_resize_h     a workgroup owns `seg` output columns of `rows` rows (both chosen per launch by rtc_resize_plan, so that
//                  the source span fits the LDS budget: the segment narrows as the downscale ratio grows). The rows' source
//                  span — from the first tap of the segment's first column to the last tap of its last — is staged in LDS
//                  with unit-stride loads, eight per thread in flight before the first is written to LDS (one at a time
//                  left the kernel waiting for memory: a workgroup stages six values per thread and then ends), a row at a
//                  pitch of 3*span doubles. A thread then owns an output PIXEL: its
//                  record and its weights are per lane and come from the table through the vector cache, where every row
//                  of the frame finds them again, one load per tap for the three channels; the tap's three values are
//                  three ds_read_b64 at 3*(first - span0 + j) + channel (through lds_f64, never paired: rtc_post.hip has
//                  the measurement). Neighbouring lanes are 3*scale doubles apart when shrinking — at scale 2 a half-wave's
//                  32 lanes fall in 16 distinct banks, a two-way conflict — and read the same entry when enlarging (a
//                  broadcast). The pixel's 24 bytes are stored together, as k_bloom_v stores its pixels.
//   k_resize_copy  both axes unchanged: the values' bytes, as 64-bit integers.
#include <hip/hip_runtime.h>

#include "rtc.h"
#include "rtc_internal.h"
#include "rtc_resize.h"

namespace {

constexpr uint32_t B = RTC_RESIZE_BLOCK;
using lds_f64 = const volatile __attribute__((address_space(3))) double;

template <uint32_t VR>
__global__ void __launch_bounds__(B) k_resize_v(ResizeArgs a) {
    const uint32_t oy0 = (blockIdx.x / a.grid_x) * VR;
    const uint32_t line = 3u * a.w_out; // values per row, of the source and of the output alike
    const uint32_t e = (blockIdx.x % a.grid_x) * B + threadIdx.x;
    if (e >= line) return;
    if constexpr (VR == 1u) { // one output row: its taps and nothing else, four rows' loads in flight
        const uint2 fc = a.fc[oy0];
        const double *w = a.w + (size_t)oy0 * a.taps;
        const double *v = a.in + (size_t)fc.x * line + e;
        double acc = 0.0;
#pragma unroll 4
        for (uint32_t j = 0; j < fc.y; ++j) acc = acc + (w[j] * v[(size_t)j * line]);
        a.out[(size_t)oy0 * line + e] = rtc_resize_canon(acc);
        return;
    }
    uint32_t first[VR], count[VR]; // uniform: scalar registers. A row past the frame has no taps.
    const double *w[VR];
#pragma unroll
    for (uint32_t k = 0; k < VR; ++k) {
        const uint32_t oy = min(oy0 + k, a.h_out - 1u);
        const uint2 fc = a.fc[oy];
        first[k] = fc.x;
        count[k] = oy0 + k < a.h_out ? fc.y : 0u;
        w[k] = a.w + (size_t)oy * a.taps;
    }
    // first and end never decrease along the axis: the rows' taps lie in [first[0], end of the last row of the frame's)
    const uint32_t last = min(oy0 + VR, a.h_out) - 1u - oy0;
    const uint32_t r0 = first[0], r1 = first[last] + count[last];
    const double *v = a.in + e;
    double acc[VR];
#pragma unroll
    for (uint32_t k = 0; k < VR; ++k) acc[k] = 0.0;
#pragma unroll 2
    for (uint32_t r = r0; r < r1; ++r) {
        const double s = v[(size_t)r * line];
#pragma unroll
        for (uint32_t k = 0; k < VR; ++k) {
            const uint32_t j = r - first[k]; // (wraps below the row's first tap: fails the test)
            if (j < count[k]) acc[k] = acc[k] + (w[k][j] * s);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < VR; ++k)
        if (oy0 + k < a.h_out) a.out[(size_t)(oy0 + k) * line + e] = rtc_resize_canon(acc[k]);
}

__global__ void __launch_bounds__(B) k_resize_h(ResizeArgs a) {
    extern __shared__ double s_src[]; // a.rows rows of a.pitch doubles
    const uint32_t x0 = (blockIdx.x % a.grid_x) * a.seg, y0 = (blockIdx.x / a.grid_x) * a.rows;
    const uint32_t cols = min(a.seg, a.w_out - x0), rows = min(a.rows, a.h_in - y0);
    const uint2 fc0 = a.fc[x0], fc1 = a.fc[x0 + cols - 1u];
    const uint32_t span0 = fc0.x, len = 3u * (fc1.x + fc1.y - span0); // doubles of one row's span
    if (len > a.pitch) return; // (never: the plan's span is the longest of the axis)
    const size_t line_in = 3u * (size_t)a.w_in, line_out = 3u * (size_t)a.w_out;
    constexpr uint32_t U = 8; // loads in flight per thread
    for (uint32_t r = 0; r < rows; ++r) {
        const double *src = a.in + (size_t)(y0 + r) * line_in + 3u * (size_t)span0;
        double *dst = s_src + r * a.pitch;
        for (uint32_t k0 = threadIdx.x; k0 < len; k0 += U * B) {
            double t[U];
#pragma unroll
            for (uint32_t u = 0; u < U; ++u) t[u] = k0 + u * B < len ? src[k0 + u * B] : 0.0;
#pragma unroll
            for (uint32_t u = 0; u < U; ++u)
                if (k0 + u * B < len) dst[k0 + u * B] = t[u];
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < rows * cols; i += B) {
        const uint32_t r = i / cols, xl = i - r * cols;
        const uint2 fc = a.fc[x0 + xl];
        const double *w = a.w + (size_t)(x0 + xl) * a.taps;
        lds_f64 *v = (lds_f64 *)(s_src + r * a.pitch + 3u * (fc.x - span0));
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
        for (uint32_t j = 0; j < fc.y; ++j) {
            const double wj = w[j];
            acc0 = acc0 + (wj * v[3u * j]);
            acc1 = acc1 + (wj * v[3u * j + 1u]);
            acc2 = acc2 + (wj * v[3u * j + 2u]);
        }
        double *o = a.out + (size_t)(y0 + r) * line_out + 3u * (size_t)(x0 + xl);
        o[0] = rtc_resize_canon(acc0);
        o[1] = rtc_resize_canon(acc1);
        o[2] = rtc_resize_canon(acc2);
    }
}

__global__ void __launch_bounds__(B) k_resize_copy(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * B + threadIdx.x;
    if (i < n) out[i] = in[i];
}

} // namespace

extern "C" hipError_t rtc_launch_resize_h(const ResizeArgs *args, const ResizePassPlan *p, hipStream_t stream) {
    ResizeArgs a = *args;
    if (!p->run || p->blocks == 0u || p->blocks > RTC_RESIZE_MAX_BLOCKS || p->lds_bytes > RTC_RESIZE_LDS_BUDGET || p->seg == 0u || p->rows == 0u)
        return hipErrorInvalidValue; // before anything is launched
    a.taps = p->taps;
    a.seg = p->seg;
    a.rows = p->rows;
    a.pitch = 3u * p->span;
    a.grid_x = p->grid_x;
    hipLaunchKernelGGL(k_resize_h, dim3((uint32_t)p->blocks), dim3(B), p->lds_bytes, stream, a);
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_resize_v(const ResizeArgs *args, const ResizePassPlan *p, hipStream_t stream) {
    ResizeArgs a = *args;
    if (!p->run || p->blocks == 0u || p->blocks > RTC_RESIZE_MAX_BLOCKS) return hipErrorInvalidValue;
    a.taps = p->taps;
    a.grid_x = p->grid_x;
    if (p->rows == RTC_RESIZE_V_ROWS)
        hipLaunchKernelGGL(k_resize_v<RTC_RESIZE_V_ROWS>, dim3((uint32_t)p->blocks), dim3(B), 0, stream, a);
    else if (p->rows == 1u)
        hipLaunchKernelGGL(k_resize_v<1u>, dim3((uint32_t)p->blocks), dim3(B), 0, stream, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

extern "C" hipError_t rtc_launch_resize_copy(const double *in, double *out, size_t n, hipStream_t stream) {
    const size_t blocks = (n + B - 1u) / B;
    if (blocks == 0u || blocks > RTC_RESIZE_MAX_BLOCKS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_resize_copy, dim3((uint32_t)blocks), dim3(B), 0, stream, reinterpret_cast<const unsigned long long *>(in),
                       reinterpret_cast<unsigned long long *>(out), n);
    return hipGetLastError();
}
