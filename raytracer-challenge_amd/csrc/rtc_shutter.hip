// rtc_shutter.hip — [device] Color::average_over (color.rs:128-139) of whole canvases on gfx950: the averaging pass behind
// motion blur (include/rtc.h "Motion blur", csrc/rtc_shutter.cpp).
//
//   k_average_over   one pass over up to RTC_SHUTTER_RING sub-frame canvases: every lane owns its elements, loads them from
//                    all the pass's frames first (independent loads, all in flight together), adds them IN SAMPLE ORDER to
//                    the carried sum (0.0 in the first pass), and either stores the sum or — last pass — divides once by
//                    (double)n and writes the f64 mean, Color::scale's bytes and / or to_imgbuf's RGBA, whichever were
//                    asked for. Purely memory-bound: no atomics, no reduction across lanes, so the only order there is, the
//                    one per element, is the host statement's (rtc_canvas_average) and the bytes are its bytes.
//                    Against a per-sample `sum += frame` (3 x 24 B per pixel and sample) a pass of R frames moves
//                    (R + 2) / R x 24 B per pixel and sample.
//   Shape: 256 threads per workgroup, at most MAX_WGS workgroups with a grid-stride loop; 16-byte loads and stores (two
//   doubles per lane) where every base is 16-byte aligned and the frame stride is even, scalar otherwise and for the odd
//   last element; the 8-bit forms go pixel by pixel (three doubles in, 3 or 4 bytes out), two pixels per lane on the
//   16-byte path. Outputs nobody reads again on the device (the mean, the bytes) are stored non-temporally; the carried
//   sum is read back by the next pass and is stored normally.
#include <hip/hip_runtime.h>

#include "rtc.h"
#include "rtc_internal.h"

namespace {

constexpr uint32_t THREADS = 256, MAX_WGS = 2048, RING = RTC_SHUTTER_RING;
typedef double __attribute__((ext_vector_type(2))) d2;

// The mean of a sum; a NaN as the one quiet NaN 0x7FF8000000000000 host and device agree on (include/rtc.h rtc_canvas_average)
__device__ __forceinline__ double mean_of(double s, double divisor) {
    const double m = s / divisor;
    return (m != m) ? __builtin_nan("") : m;
}

// T = double or d2. Element i (in units of T) of the pass's NF frames — the loads first, none of them behind a branch, so
// that all are in flight together — then the sum in sample order.
template <class T, uint32_t NF>
__device__ __forceinline__ T sum_n(const AverageArgs &a, size_t i, bool carried) {
    constexpr size_t PER = sizeof(T) / sizeof(double);
    T v[NF];
#pragma unroll
    for (uint32_t f = 0; f < NF; ++f) v[f] = *reinterpret_cast<const T *>(a.frames + (size_t)f * a.stride + i * PER);
    T s = carried ? *reinterpret_cast<const T *>(a.sum_in + i * PER) : T(0.0);
#pragma unroll
    for (uint32_t f = 0; f < NF; ++f) s = s + v[f];
    return s;
}
// ... for the pass's frame count, which is the same for every lane (a scalar branch)
template <class T>
__device__ __forceinline__ T sum_frames(const AverageArgs &a, size_t i, bool carried) {
    switch (a.nf) {
    case 1: return sum_n<T, 1>(a, i, carried);
    case 2: return sum_n<T, 2>(a, i, carried);
    case 3: return sum_n<T, 3>(a, i, carried);
    case 4: return sum_n<T, 4>(a, i, carried);
    case 5: return sum_n<T, 5>(a, i, carried);
    case 6: return sum_n<T, 6>(a, i, carried);
    case 7: return sum_n<T, 7>(a, i, carried);
    default: return sum_n<T, RING>(a, i, carried);
    }
}
static_assert(RING == 8u, "sum_frames lists the frame counts of a pass");

// VEC: every base 16-byte aligned, stride even. BYTES: the last pass with an 8-bit output (count = 3 x pixels).
template <bool VEC, bool BYTES>
__global__ void __launch_bounds__(THREADS) k_average_over(AverageArgs a) {
    const bool carried = a.sum_in != nullptr, last = a.divisor != 0.0;
    const size_t tid = (size_t)blockIdx.x * THREADS + threadIdx.x, nthreads = (size_t)gridDim.x * THREADS;
    if constexpr (!BYTES) {
        const size_t nvec = VEC ? a.count / 2u : 0u;
        if constexpr (VEC)
            for (size_t i = tid; i < nvec; i += nthreads) {
                d2 s = sum_frames<d2>(a, i, carried);
                if (last) {
                    s.x = mean_of(s.x, a.divisor);
                    s.y = mean_of(s.y, a.divisor);
                    __builtin_nontemporal_store(s, reinterpret_cast<d2 *>(a.f64_out) + i);
                } else {
                    reinterpret_cast<d2 *>(a.f64_out)[i] = s;
                }
            }
        for (size_t i = nvec * 2u + tid; i < a.count; i += nthreads) { // everything on the scalar path, or the odd last element
            const double s = sum_frames<double>(a, i, carried);
            if (last) __builtin_nontemporal_store(mean_of(s, a.divisor), a.f64_out + i);
            else a.f64_out[i] = s;
        }
    } else {
        const size_t px = a.count / 3u, npair = VEC ? px / 2u : 0u;
        if constexpr (VEC)
            for (size_t p = tid; p < npair; p += nthreads) { // pixels 2p and 2p + 1: 48 contiguous bytes of every frame
                double c[6];
#pragma unroll
                for (uint32_t j = 0; j < 3u; ++j) {
                    const d2 s = sum_frames<d2>(a, p * 3u + j, carried);
                    c[2u * j] = mean_of(s.x, a.divisor);
                    c[2u * j + 1u] = mean_of(s.y, a.divisor);
                    if (a.f64_out) __builtin_nontemporal_store(d2{c[2u * j], c[2u * j + 1u]}, reinterpret_cast<d2 *>(a.f64_out) + p * 3u + j);
                }
                if (a.rgb8) {
                    unsigned short *o = reinterpret_cast<unsigned short *>(a.rgb8 + p * 6u); // 2-byte aligned on this path
#pragma unroll
                    for (uint32_t j = 0; j < 3u; ++j)
                        __builtin_nontemporal_store((unsigned short)(scale255(c[2u * j]) | ((unsigned)scale255(c[2u * j + 1u]) << 8)), o + j);
                }
                if (a.rgba8) {
                    typedef unsigned __attribute__((ext_vector_type(2))) u2;
                    const unsigned lo = (unsigned)gamma_byte(a.g, c[0]) | ((unsigned)gamma_byte(a.g, c[1]) << 8) | ((unsigned)gamma_byte(a.g, c[2]) << 16) | 0xff000000u;
                    const unsigned hi = (unsigned)gamma_byte(a.g, c[3]) | ((unsigned)gamma_byte(a.g, c[4]) << 8) | ((unsigned)gamma_byte(a.g, c[5]) << 16) | 0xff000000u;
                    __builtin_nontemporal_store(u2{lo, hi}, reinterpret_cast<u2 *>(a.rgba8) + p);
                }
            }
        for (size_t p = npair * 2u + tid; p < px; p += nthreads) { // one pixel per lane
            double c[3];
#pragma unroll
            for (uint32_t j = 0; j < 3u; ++j) {
                c[j] = mean_of(sum_frames<double>(a, p * 3u + j, carried), a.divisor);
                if (a.f64_out) __builtin_nontemporal_store(c[j], a.f64_out + p * 3u + j);
            }
            if (a.rgb8)
#pragma unroll
                for (uint32_t j = 0; j < 3u; ++j) a.rgb8[p * 3u + j] = scale255(c[j]);
            if (a.rgba8) {
#pragma unroll
                for (uint32_t j = 0; j < 3u; ++j) a.rgba8[p * 4u + j] = gamma_byte(a.g, c[j]);
                a.rgba8[p * 4u + 3u] = 255u;
            }
        }
    }
}

bool aligned(const void *p, size_t to) { return ((size_t)p % to) == 0u; }

} // namespace

extern "C" hipError_t rtc_launch_average_over(const AverageArgs *args, hipStream_t stream) {
    const AverageArgs &a = *args;
    if (a.count == 0u) return hipSuccess;
    if (a.nf == 0u || a.nf > RING || !a.frames) return hipErrorInvalidValue;
    const bool bytes = a.rgb8 || a.rgba8;
    if (bytes ? (a.divisor == 0.0 || a.count % 3u != 0u || (a.rgba8 && !a.g)) : !a.f64_out) return hipErrorInvalidValue;
    // the 16-byte path: every frame of the pass, the carried sum and the f64 output start on 16 bytes, and the packed byte
    // stores on their own width
    const bool vec = aligned(a.frames, 16) && (a.nf == 1u || a.stride % 2u == 0u) && aligned(a.sum_in, 16) && aligned(a.f64_out, 16) &&
                     aligned(a.rgb8, 2) && aligned(a.rgba8, 8);
    const size_t work = bytes ? (vec ? (a.count / 3u + 1u) / 2u : a.count / 3u) : (vec ? (a.count + 1u) / 2u : a.count);
    const size_t want = (work + THREADS - 1u) / THREADS;
    const dim3 grid((uint32_t)(want < MAX_WGS ? want : MAX_WGS)), block(THREADS);
    if (bytes && vec) hipLaunchKernelGGL((k_average_over<true, true>), grid, block, 0, stream, a);
    else if (bytes) hipLaunchKernelGGL((k_average_over<false, true>), grid, block, 0, stream, a);
    else if (vec) hipLaunchKernelGGL((k_average_over<true, false>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((k_average_over<false, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}
