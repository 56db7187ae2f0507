// rtc_world_build.h — the device build behind rtc_world_update: what one generation of a World's tables is built from
// and into (rtc_world_build.hip). Not part of the ABI.
#ifndef RTC_WORLD_BUILD_H
#define RTC_WORLD_BUILD_H

#include <hip/hip_runtime.h>

#include "rtc_device.h"

// The scalars of a generation that only the device knows after a build. The render kernels take them by argument, so the
// header is copied into page-locked memory behind the build and read by the first launch that uses the generation.
struct DevWorldHeader {
    uint32_t n_unb, _pad;
    double pre_limit;     // RenderParams::pre_limit (0 when 64 x extent is not finite)
    double light_reach;   // 2 x far; 0: this generation has no light lists
    double pre_limit_raw; // 64 x extent as pre_of takes it
};
static_assert(sizeof(DevWorldHeader) == 32, "one pinned 32-byte slot per generation");

enum { RTC_WB_PARTIALS = 9 }; // per wave of 64 objects: lo[3], hi[3], extent, far, unbounded count
enum { RTC_WB_SORT_CHUNK = 8192 }; // (key, index) pairs one workgroup sorts in LDS: 96 KiB of the CU's 160

// Pairs the sort works on: the next power of two, at least one wave.
inline uint32_t rtc_world_build_npad(uint32_t n) {
    uint32_t p = 64u;
    while (p < n) p <<= 1;
    return p;
}

struct WorldBuildArgs {
    uint32_t n, npad;
    uint32_t light_on; // n >= 32, a finite light position and room for the lists: reach decides the rest
    double light[3];
    const DevIsect *isect; // [n] in: the flattened shapes, insertion order
    const uint32_t *kind;  // [n] in
    DevBound *bound;       // [n] out, as everything below
    DevIsect *isect_s;
    uint32_t *kind_s;
    DevBound *bound_s;
    uint32_t *orig_s;
    DevBound *gbound; // [ceil(n / 64)]
    DevPre *pre, *pre_s;
    DevWorldHeader *hdr;
    double *partial;         // scratch [ceil(n / 64)][RTC_WB_PARTIALS]
    unsigned long long *key; // scratch [npad]
    uint32_t *idx;           // scratch [npad]
};

// Enqueues the whole build on `stream`: bounds, reductions, Morton keys, sort, gather, group spheres, prefilter records
// and the header — every table of rtc_world_create's host build, bit for bit. n == 0 writes the one default record.
extern "C" hipError_t rtc_launch_world_build(const WorldBuildArgs *a, hipStream_t stream);

#endif
