// rtc_world_build.hip — [device] the table build of rtc_world_update for gfx950: what rtc_world_create derives on the
// host from the flattened shapes (rtc_api.cpp: bound_of, the Morton order, the group spheres, the prefilter records),
// derived on the device with the same f64 operations in the same order, so that an updated World and a freshly created
// one hold the same bits. Compiled with -ffp-contract=off like the host code; f64 sqrt and / are correctly rounded, and
// fmin / fmax of the values reduced here do not depend on the order of the reduction. Only the group centres are sums:
// they are added in index order, as the host adds them.
//
// The build is a handful of small kernels and is bound by launch latency, not by throughput: one wave per workgroup
// wherever a wave of 64 objects (one group of the two-level tables) is the natural unit, no atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include "rtc.h"
#include "rtc_world_build.h"

#define DEVI __device__ __forceinline__

namespace {

constexpr double kInf = __builtin_inf();

DEVI bool finite(double x) { return __builtin_isfinite(x); }
DEVI double dmax(double a, double b) { return __builtin_fmax(a, b); }
DEVI double dmin(double a, double b) { return __builtin_fmin(a, b); }
DEVI double dabs(double a) { return __builtin_fabs(a); }
DEVI double dsqrt(double a) { return __builtin_sqrt(a); }

DEVI DevBound unbounded() { return DevBound{0., 0., 0., kInf, 0., 0.}; }

// bound_of (rtc_api.cpp), operation for operation. m = rows 0..2 of the stored inverse, four columns each.
DEVI DevBound bound_of(const double *m, uint32_t kind) {
    DevBound b = unbounded();
    if (kind == RTC_PLANE) return b;
    const double a[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
    const double t[3] = {m[3], m[7], m[11]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (!finite(t[i])) return b;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (!finite(a[i][j])) return b;
    }
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (!(dabs(det) > 1e-300) || !finite(det)) return b;
    double f[3][3];
    f[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) / det;
    f[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det;
    f[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
    f[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) / det;
    f[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det;
    f[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
    f[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) / det;
    f[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
    f[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
    double resid = 0., fmaxabs = 0.;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v = (i == j) ? -1. : 0.;
#pragma unroll
            for (int k = 0; k < 3; ++k) v += a[i][k] * f[k][j];
            resid = dmax(resid, dabs(v));
            fmaxabs = dmax(fmaxabs, dabs(f[i][j]));
            if (!finite(f[i][j])) return b;
        }
    if (!(resid < 1e-9)) return b;
    double c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = -(f[i][0] * t[0] + f[i][1] * t[1] + f[i][2] * t[2]);
    double r2;
    if (kind == RTC_SPHERE) {
        double S[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) S[i][j] = f[i][0] * f[j][0] + f[i][1] * f[j][1] + f[i][2] * f[j][2];
        for (int sweep = 0; sweep < 30; ++sweep) {
            const double off = dabs(S[0][1]) + dabs(S[0][2]) + dabs(S[1][2]);
            if (off < 1e-300) break;
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int q = p + 1; q < 3; ++q) {
                    if (S[p][q] == 0.) continue;
                    const double th = (S[q][q] - S[p][p]) / (2. * S[p][q]);
                    const double tt = (th >= 0. ? 1. : -1.) / (dabs(th) + dsqrt(th * th + 1.));
                    const double cs = 1. / dsqrt(tt * tt + 1.), sn = tt * cs;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double skp = S[k][p], skq = S[k][q];
                        S[k][p] = cs * skp - sn * skq;
                        S[k][q] = sn * skp + cs * skq;
                    }
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double spk = S[p][k], sqk = S[q][k];
                        S[p][k] = cs * spk - sn * sqk;
                        S[q][k] = sn * spk + cs * sqk;
                    }
                }
        }
        const double g = dabs(S[0][1]) + dabs(S[0][2]) + dabs(S[1][2]);
        r2 = dmax(S[0][0], dmax(S[1][1], S[2][2])) + 2. * g;
    } else {
        r2 = 0.;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double px = (k & 1) ? 1. : -1., py = (k & 2) ? 1. : -1., pz = (k & 4) ? 1. : -1.;
            double q = 0.;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double v = f[i][0] * px + f[i][1] * py + f[i][2] * pz;
                q += v * v;
            }
            r2 = dmax(r2, q);
        }
    }
    if (!finite(r2) || !(r2 >= 0.)) return b;
    const double cn = dsqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const double r = dsqrt(r2) * (1. + 1e-6) + 1e-9 * (1. + cn) + 1e-7 * fmaxabs;
    if (!finite(r) || !finite(cn)) return b;
    double na2 = 0.;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) na2 += a[i][j] * a[i][j];
    const double k = 0.75e-14 * na2;
    if (!finite(k)) return b;
    b.cx = c[0]; b.cy = c[1]; b.cz = c[2]; b.r = r;
    b.k = k;
    b.cn = cn;
    return b;
}

DEVI unsigned long long spread21(unsigned long long v) {
    v &= 0x1fffffULL;
    v = (v | (v << 32)) & 0x1f00000000ffffULL;
    v = (v | (v << 16)) & 0x1f0000ff0000ffULL;
    v = (v | (v << 8)) & 0x100f00f00f00f00fULL;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ULL;
    v = (v | (v << 2)) & 0x1249249249249249ULL;
    return v;
}
DEVI unsigned long long morton_key(const DevBound &b, const double lo[3], const double hi[3]) {
    unsigned long long k = 0;
    const double c[3] = {b.cx, b.cy, b.cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double ext = hi[a] - lo[a];
        double u = ext > 0. ? (c[a] - lo[a]) / ext : 0.;
        if (!(u >= 0.)) u = 0.;
        if (u > 1.) u = 1.;
        k |= spread21((unsigned long long)(u * 2097151.0)) << a;
    }
    return k;
}

DEVI DevPre pre_of(const DevBound &b, double pre_limit) {
    DevPre q{b.cx, b.cy, b.cz, kInf};
    if (finite(b.r) && finite(pre_limit)) {
        const double Dw = (dabs(b.cx) + dabs(b.cy) + dabs(b.cz) + pre_limit) * (1. + 1e-12);
        const double R = ((b.r + b.r * (b.k * Dw * (b.cn + Dw))) * 1.000001 + 1e-12) * (1. + 1e-12);
        const double R2 = R * R * (1. + 1e-12);
        if (finite(R2)) q.R2 = R2;
    }
    return q;
}

// Butterfly over the wave's 64 lanes: every lane ends with the result.
template <class Op>
DEVI double wave_all(double v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}
struct MaxOp { DEVI double operator()(double a, double b) const { return dmax(a, b); } };
struct MinOp { DEVI double operator()(double a, double b) const { return dmin(a, b); } };
struct AddOp { DEVI double operator()(double a, double b) const { return a + b; } }; // whole numbers below 2^53 only

// What the reductions start from (the host's initial values; extent's 1 and far's 0 are also their floors).
struct Partials {
    double v[RTC_WB_PARTIALS];
    DEVI void init() {
        v[0] = v[1] = v[2] = kInf;
        v[3] = v[4] = v[5] = -kInf;
        v[6] = 1.;
        v[7] = 0.;
        v[8] = 0.;
    }
    DEVI void wave_reduce() {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = wave_all(v[k], MinOp());
#pragma unroll
        for (int k = 3; k < 8; ++k) v[k] = wave_all(v[k], MaxOp());
        v[8] = wave_all(v[8], AddOp());
    }
};

// Step 1, one lane per object: its bound, and the wave's share of the reductions. n == 0: the default records of a World
// without shapes (rtc_world_create sizes every table for one entry).
__global__ void __launch_bounds__(64) k_wb_bounds(WorldBuildArgs a) {
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    if (a.n == 0u) {
        if (i == 0u) {
            a.bound[0] = DevBound{0., 0., 0., 0., 0., 0.};
            a.bound_s[0] = unbounded();
            a.gbound[0] = unbounded();
            a.pre[0] = a.pre_s[0] = DevPre{0., 0., 0., kInf};
            a.kind_s[0] = 0u;
            a.orig_s[0] = 0u;
            DevIsect z;
            for (int k = 0; k < 12; ++k) z.m[k] = 0.;
            a.isect_s[0] = z;
            *a.hdr = DevWorldHeader{0u, 0u, 64., 0., 64.};
        }
        return;
    }
    Partials P;
    P.init();
    if (i < a.n) {
        const DevIsect is = a.isect[i];
        const DevBound b = bound_of(is.m, a.kind[i]);
        a.bound[i] = b;
        if (finite(b.r)) {
            P.v[0] = P.v[3] = b.cx;
            P.v[1] = P.v[4] = b.cy;
            P.v[2] = P.v[5] = b.cz;
            P.v[6] = dmax(1., dabs(b.cx) + dabs(b.cy) + dabs(b.cz) + b.r);
            const double dx = b.cx - a.light[0], dy = b.cy - a.light[1], dz = b.cz - a.light[2];
            P.v[7] = dmax(0., dsqrt(dx * dx + dy * dy + dz * dz) + b.r);
        } else {
            P.v[8] = 1.;
        }
    }
    P.wave_reduce();
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < RTC_WB_PARTIALS; ++k) a.partial[(size_t)blockIdx.x * RTC_WB_PARTIALS + k] = P.v[k];
    }
}

// The second, atomic-free step of the reductions: every wave folds all partials itself (n / 64 of them) instead of one
// more launch in a latency-bound chain. Sized for the Worlds this renderer holds — at C3's 10 001 objects 256 waves read
// 11 KB each from L2; the reads grow as n^2 / 4096, so from some 10^5 objects on a one-wave fold kernel that leaves
// lo / hi in the header is the better trade.
DEVI Partials fold_partials(const WorldBuildArgs &a, uint32_t lane) {
    Partials P;
    P.init();
    const uint32_t nb = (a.n + 63u) / 64u;
    for (uint32_t p = lane; p < nb; p += 64u) {
        const double *q = a.partial + (size_t)p * RTC_WB_PARTIALS;
#pragma unroll
        for (int k = 0; k < 3; ++k) P.v[k] = dmin(P.v[k], q[k]);
#pragma unroll
        for (int k = 3; k < 8; ++k) P.v[k] = dmax(P.v[k], q[k]);
        P.v[8] += q[8];
    }
    P.wave_reduce();
    return P;
}

// Step 2, one lane per sort slot: the header (first wave), the Morton key and the prefilter record of each object.
// Slots past n hold the largest pair, so they stay behind every object.
__global__ void __launch_bounds__(64) k_wb_keys(WorldBuildArgs a) {
    const uint32_t lane = threadIdx.x, i = blockIdx.x * 64u + lane;
    const Partials P = fold_partials(a, lane);
    const double pre_limit = 64. * P.v[6];
    if (i == 0u) {
        const double reach = 2. * P.v[7];
        const bool lists = a.light_on && finite(reach) && reach > 0. && reach < 1e30;
        *a.hdr = DevWorldHeader{(uint32_t)P.v[8], 0u, finite(pre_limit) ? pre_limit : 0., lists ? reach : 0., pre_limit};
    }
    unsigned long long key = ~0ull;
    uint32_t idx = ~0u;
    if (i < a.n) {
        const DevBound b = a.bound[i];
        const double lo[3] = {P.v[0], P.v[1], P.v[2]}, hi[3] = {P.v[3], P.v[4], P.v[5]};
        key = finite(b.r) ? (1ull << 63) | morton_key(b, lo, hi) : 0ull;
        idx = i;
        a.pre[i] = pre_of(b, pre_limit);
    }
    a.key[i] = key; // i < npad: the grid is npad / 64 waves
    a.idx[i] = idx;
}

// Bitonic network on (key, index) pairs — no two objects share a pair, so the order is the host's stable order by key.
DEVI bool pair_after(unsigned long long ka, uint32_t ia, unsigned long long kb, uint32_t ib) { return ka > kb || (ka == kb && ia > ib); }

// Stages k0 .. k1 of the network for the compare distances that stay inside one chunk of `chunk` pairs, held in LDS:
// the whole sort of a chunk (k0 = 2, k1 = chunk), or the tail of a later stage (k0 = k1 = k) after the global passes.
__global__ void __launch_bounds__(1024) k_wb_sort_lds(unsigned long long *__restrict__ key, uint32_t *__restrict__ idx, uint32_t chunk,
                                                       uint32_t k0, uint32_t k1) {
    extern __shared__ unsigned long long sk[];
    uint32_t *si = reinterpret_cast<uint32_t *>(sk + chunk);
    const uint32_t base = blockIdx.x * chunk;
    for (uint32_t t = threadIdx.x; t < chunk; t += 1024u) {
        sk[t] = key[base + t];
        si[t] = idx[base + t];
    }
    __syncthreads();
    for (uint32_t k = k0; k <= k1 && k != 0u; k <<= 1) {
        for (uint32_t j = (k >> 1) < (chunk >> 1) ? (k >> 1) : (chunk >> 1); j != 0u; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (chunk >> 1); t += 1024u) {
                const uint32_t lo = 2u * t - (t & (j - 1u)), hi = lo + j;
                const bool up = ((base + lo) & k) == 0u;
                const unsigned long long ka = sk[lo], kb = sk[hi];
                const uint32_t ia = si[lo], ib = si[hi];
                if (pair_after(ka, ia, kb, ib) == up) {
                    sk[lo] = kb; sk[hi] = ka;
                    si[lo] = ib; si[hi] = ia;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t t = threadIdx.x; t < chunk; t += 1024u) {
        key[base + t] = sk[t];
        idx[base + t] = si[t];
    }
}

// One compare distance j >= chunk of stage k, in global memory: one lane per pair of slots.
__global__ void __launch_bounds__(256) k_wb_sort_global(unsigned long long *__restrict__ key, uint32_t *__restrict__ idx, uint32_t npad,
                                                         uint32_t k, uint32_t j) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (npad >> 1)) return;
    const uint32_t lo = 2u * t - (t & (j - 1u)), hi = lo + j;
    const bool up = (lo & k) == 0u;
    const unsigned long long ka = key[lo], kb = key[hi];
    const uint32_t ia = idx[lo], ib = idx[hi];
    if (pair_after(ka, ia, kb, ib) == up) {
        key[lo] = kb; key[hi] = ka;
        idx[lo] = ib; idx[hi] = ia;
    }
}

// Step 4, one wave per group of 64 sorted objects: the sorted copies, their prefilter records and the group's sphere.
// Every lane adds the members' centres itself, in index order, so the sums are the host's and need no broadcast.
__global__ void __launch_bounds__(64) k_wb_gather(WorldBuildArgs a) {
    __shared__ double sc[3][64];
    const uint32_t lane = threadIdx.x, g = blockIdx.x, i = g * 64u + lane;
    const bool have = i < a.n;
    const uint32_t members = a.n - g * 64u < 64u ? a.n - g * 64u : 64u;
    DevBound b = unbounded();
    if (have) {
        const uint32_t o = a.idx[i];
        b = a.bound[o];
        a.isect_s[i] = a.isect[o];
        a.kind_s[i] = a.kind[o];
        a.bound_s[i] = b;
        a.orig_s[i] = o;
        a.pre_s[i] = pre_of(b, a.hdr->pre_limit_raw);
    }
    sc[0][lane] = b.cx; sc[1][lane] = b.cy; sc[2][lane] = b.cz;
    __syncthreads();
    DevBound gb = unbounded();
    if (__ballot(have && !finite(b.r)) == 0ull) { // wave-uniform
        double cx = 0., cy = 0., cz = 0.;
        for (uint32_t m = 0; m < members; ++m) { cx += sc[0][m]; cy += sc[1][m]; cz += sc[2][m]; }
        const double cnt = (double)members;
        cx /= cnt; cy /= cnt; cz /= cnt;
        double ri = 0.;
        if (have) {
            const double dx = b.cx - cx, dy = b.cy - cy, dz = b.cz - cz;
            ri = dsqrt(dx * dx + dy * dy + dz * dz) + b.r;
            if (!(ri >= 0.)) ri = 0.; // NaN: fmax leaves the running 0 alone
        }
        double r = wave_all(ri, MaxOp());
        const double kmax = wave_all(have ? b.k : 0., MaxOp()), cnmax = wave_all(have ? b.cn : 0., MaxOp());
        r = r * (1. + 1e-9) + 1e-12;
        if (finite(r) && finite(cx) && finite(cy) && finite(cz)) gb = DevBound{cx, cy, cz, r, kmax * 4., cnmax + 2. * r};
    }
    if (lane == 0u) a.gbound[g] = gb;
}

} // namespace

extern "C" hipError_t rtc_launch_world_build(const WorldBuildArgs *pa, hipStream_t stream) {
    const WorldBuildArgs a = *pa;
    if (a.n == 0u) {
        hipLaunchKernelGGL(k_wb_bounds, dim3(1), dim3(64), 0, stream, a);
        return hipGetLastError();
    }
    const uint32_t groups = (a.n + 63u) / 64u, npad = a.npad, chunk = npad < RTC_WB_SORT_CHUNK ? npad : (uint32_t)RTC_WB_SORT_CHUNK;
    const size_t lds = (size_t)chunk * (sizeof(unsigned long long) + sizeof(uint32_t));
    if (lds > 48u * 1024u) { // more dynamic LDS than the default limit: opt in (up to 160 KiB per CU on gfx950)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wb_sort_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_wb_bounds, dim3(groups), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(k_wb_keys, dim3(npad / 64u), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(k_wb_sort_lds, dim3(npad / chunk), dim3(1024), lds, stream, a.key, a.idx, chunk, 2u, chunk);
    for (uint32_t k = chunk << 1; k != 0u && k <= npad; k <<= 1) { // worlds above one chunk: the long distances in global memory
        for (uint32_t j = k >> 1; j >= chunk; j >>= 1)
            hipLaunchKernelGGL(k_wb_sort_global, dim3((npad / 2u + 255u) / 256u), dim3(256), 0, stream, a.key, a.idx, npad, k, j);
        hipLaunchKernelGGL(k_wb_sort_lds, dim3(npad / chunk), dim3(1024), lds, stream, a.key, a.idx, chunk, k, k);
    }
    hipLaunchKernelGGL(k_wb_gather, dim3(groups), dim3(64), 0, stream, a);
    return hipGetLastError();
}
