// rtc_resize.h — what the host statement of the resize (host_resize.cpp), the device entry (rtc_resize.cpp) and the kernels
// (rtc_resize.hip) share (include/rtc.h, "resizing f64 canvases"): the tap range of an output, the constants the kernels are
// compiled for, the table of one axis as the device entry keeps it, and the launch plan, a pure host function that a CPU
// test pins through rtc_debug_plan_resize. All three files are compiled with -ffp-contract=off. Not part of the ABI.
#ifndef RTC_RESIZE_H
#define RTC_RESIZE_H

#include <stdint.h>

#include <vector>

#include "rtc.h"

// What the kernels of rtc_resize.hip are compiled for.
enum {
    RTC_RESIZE_BLOCK = 256,          // threads per workgroup, every kernel
    RTC_RESIZE_MAX_SEG = 256,        // k_resize_h: the most output columns of a workgroup (one output pixel per thread)
    RTC_RESIZE_V_ROWS = 4,           // k_resize_v: output rows per workgroup, whose source rows are loaded once, ...
    RTC_RESIZE_V_MIN_BLOCKS = 2048,  // ... when that still leaves this many workgroups (eight per CU); else one row per workgroup
    RTC_RESIZE_LDS_BUDGET = 49152,   // k_resize_h: the most LDS bytes of a workgroup (three workgroups of a CU's 160 KiB)
    RTC_RESIZE_MAX_BLOCKS = 0xffffff // a launch holds fewer than 2^32 threads: at most this many workgroups of 256
};

// a NaN as the one quiet NaN 0x7FF8000000000000 (rtc_post_canon's rule)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline double rtc_resize_canon(double v) { return (v != v) ? __builtin_nan("") : v; }

// The table of one axis, n_in -> n_out: rtc_resize_weights' output. `taps` is the row length of w.
struct ResizeAxis {
    uint32_t n_in = 0, n_out = 0, filter = 0, taps = 0;
    std::vector<uint32_t> first, count;
    std::vector<double> w;
};
// [host_resize.cpp] The function behind rtc_resize_weights, which the device entry calls too. RTC_ERR_ARG as the entry's;
// RTC_ERR_NOMEM when a vector cannot grow.
rtc_status rtc_resize_build_axis(uint32_t n_in, uint32_t n_out, uint32_t filter, ResizeAxis *out);
// [host_resize.cpp] first and end of output o (the header's rule; radius: the filter's R). n_in != n_out.
void rtc_resize_range(uint32_t n_in, uint32_t n_out, double radius, uint32_t o, uint32_t *first, uint32_t *end);
double rtc_resize_radius(uint32_t filter); // 0.0 for an unknown filter

// The launch plan of one resize: which passes run and with what geometry. Plain data, laid out for ctypes.
struct ResizePassPlan {
    uint32_t run;       // 1: the pass filters; 0: its axis is unchanged and nothing is launched for it
    uint32_t taps;      // the axis's rtc_resize_taps
    uint32_t seg;       // k_resize_h: output columns per workgroup (1 .. RTC_RESIZE_MAX_SEG); k_resize_v: output values per workgroup (256)
    uint32_t rows;      // rows per workgroup (k_resize_v: RTC_RESIZE_V_ROWS output rows, or 1)
    uint32_t span;      // k_resize_h: the longest source span, in pixels, of a segment (the LDS row pitch is 3*span doubles); else 0
    uint32_t lds_bytes; // rows * span * 24 (k_resize_v: 0)
    uint32_t grid_x;    // segments per row (k_resize_v: per output row)
    uint32_t grid_y;    // row blocks
    uint64_t blocks;    // grid_x * grid_y, at most RTC_RESIZE_MAX_BLOCKS
    uint64_t table_bytes; // the axis's device table: n_out * (taps + 1) * 8
};
struct ResizePlan {
    uint32_t status;       // RTC_OK, or RTC_ERR_ARG: a zero size, an unknown filter, too many taps, a grid of 2^32 threads or more
    uint32_t copy;         // 1: both axes unchanged, k_resize_copy alone
    ResizePassPlan h, v;
    uint64_t copy_blocks;  // k_resize_copy's workgroups when copy
    uint64_t mid_bytes;    // the intermediate w_out x h_in frame; 0 unless both passes run
};
struct ResizePlanInputs {
    uint32_t w_in, h_in, w_out, h_out, filter;
};
// [host_resize.cpp] pure: no device, no allocation beyond O(1).
void rtc_resize_plan(const ResizePlanInputs *in, ResizePlan *out);
extern "C" rtc_status rtc_debug_plan_resize(const ResizePlanInputs *in, ResizePlan *out);

#endif
