// rtc_launch_plan.h — what a launch will be, decided from plain numbers before anything touches the device.
//
// rtc_plan_launch is the one place where the host chooses a kernel's object source, workgroup size, dynamic LDS, binning
// and its memory, the guided-chunk split and the pixel count of a launch. It is pure integer arithmetic: no HIP, no
// rtc_context, no rtc_world, so every threshold is pinned by a CPU test (tests/test_host_launch_plan.py, through
// rtc_debug_plan_launch). rtc_api.cpp carries a plan out and decides only what the device tells it at run time.
#ifndef RTC_LAUNCH_PLAN_H
#define RTC_LAUNCH_PLAN_H

#include <stdint.h>

#include "rtc.h"
#include "rtc_device.h"

enum {
    RTC_PLAN_FRAME = 0, // rows, bands or views of a frame (render_launch)
    RTC_PLAN_PROBE = 1, // rtc_color_at: `hsize` rays, one lane each; the other request fields are not read
    RTC_PLAN_AOV = 2    // rtc_render_aov_device: one wave per 8x8 tile of the whole frame
};

struct LaunchPlanInputs {
    // the context's knobs (rtc_context, rtc_internal.h)
    int32_t force_src; // < 0: none
    uint32_t tile_cap, tiles_per_wg, tiles_guided_tenths, tiles_slots, tiles_kmax;
    uint32_t binning, pipelined; // pipelined: the context deals its launches over lanes (lanes > 1)
    uint64_t bin_small_pixels, bin_small_pixels_pipelined;
    // the World generation's facts
    uint32_t n, n_lights, any_refl, any_refr;
    // the request
    uint32_t kind; // RTC_PLAN_*
    uint32_t hsize, vsize, samples, nviews;
    uint32_t y0, y1, band_stride, grid_y; // tile row k of grid_y renders image rows y0 + 8*k*band_stride .. (+8), below y1
    uint32_t mode, flags;
    uint32_t lens_samples; // usteps * vsteps of a thin-lens launch; 0: pinhole
};

struct LaunchPlan {
    uint32_t status; // RTC_OK, or RTC_ERR_UNSUPPORTED: no kernel renders this request from the source it selects
    int32_t src;     // SRC_*
    uint32_t refl, refr; // the kernel's recursion flavour (refl: any frame stack at all)
    uint32_t flags;      // RenderParams::flags
    uint32_t tile_cap, lds_bytes, aa_lds_off, resample_n;
    uint32_t block, tile_w, grid_x, total_blocks, reps, chunk_wgs[4];
    uint32_t grid_wgs; // workgroups to launch
    // binned primary pass: wanted (the launch still walks when there is no memory for the lists), and what to reserve
    uint32_t bin, tiles_x, tiles_y;
    uint64_t tiles, tiles_alloc, prims, prims_alloc;
    uint32_t lane_dealt; // a pipelined context may deal the launch to a lane (else it stays in order on lane 0)
    uint32_t needs_prep; // rtc_launch_prep first: the per-render table of ONE camera, so one view per launch
    uint64_t launch_pixels;  // the part of the frame(s) the launch covers: what the thresholds compare
    uint64_t counted_pixels; // rtc_stats::pixels of the launch
};

void rtc_plan_launch(const LaunchPlanInputs &in, LaunchPlan &out);

// Unlisted export (not in include/rtc.h; tests bind it by hand): rtc_plan_launch as it stands.
extern "C" rtc_status rtc_debug_plan_launch(const LaunchPlanInputs *in, LaunchPlan *out);

#endif
