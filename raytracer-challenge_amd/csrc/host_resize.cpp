// host_resize.cpp — [host] the normative statement of the resize (include/rtc.h, "resizing f64 canvases"): the five filters
// (the only place sin is called), the table of one axis, the two passes, and the launch plan of the device form (a pure
// function: rtc_resize.h). Plain f64, compiled with -ffp-contract=off like every file of the library.
#include "rtc.h"
#include "rtc_resize.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace {

double kernel_of(uint32_t filter, double x) {
    const double a = std::fabs(x);
    switch (filter) {
    case RTC_RESIZE_BOX: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case RTC_RESIZE_TRIANGLE: return a < 1.0 ? 1.0 - a : 0.0;
    case RTC_RESIZE_CATMULL_ROM:
        if (a < 1.0) return ((((1.5 * a) - 2.5) * a) * a) + 1.0;
        if (a < 2.0) return (((((-0.5 * a) + 2.5) * a) - 4.0) * a) + 2.0;
        return 0.0;
    case RTC_RESIZE_MITCHELL:
        if (a < 1.0) return (((((7.0 * a) - 12.0) * a) * a) + (16.0 / 3.0)) / 6.0;
        if (a < 2.0) return (((((((-7.0 / 3.0) * a) + 12.0) * a) - 20.0) * a) + (32.0 / 3.0)) / 6.0;
        return 0.0;
    default: // RTC_RESIZE_LANCZOS3
        if (x == 0.0) return 1.0;
        if (a < 3.0) {
            const double p = 3.141592653589793 * x, q = p / 3.0;
            return (std::sin(p) / p) * (std::sin(q) / q);
        }
        return 0.0;
    }
}

double axis_scale(uint32_t n_in, uint32_t n_out) { return (double)n_in / (double)n_out; }

// the largest count of a filtered axis (n_in != n_out)
uint32_t axis_taps(uint32_t n_in, uint32_t n_out, double radius) {
    uint32_t taps = 0;
    for (uint32_t o = 0; o < n_out; ++o) {
        uint32_t first, end;
        rtc_resize_range(n_in, n_out, radius, o, &first, &end);
        if (end - first > taps) taps = end - first;
    }
    return taps;
}

// one filtered pass over `n_lines` lines: output o of a line is the taps' sum over v[(first + j) * stride] (host statement)
void pass(const double *in, double *out, const ResizeAxis &ax, size_t n_lines, size_t line_in, size_t line_out, size_t stride, size_t chans) {
    for (size_t l = 0; l < n_lines; ++l)
        for (uint32_t o = 0; o < ax.n_out; ++o) {
            const double *w = ax.w.data() + (size_t)o * ax.taps;
            const uint32_t first = ax.first[o], count = ax.count[o];
            for (size_t c = 0; c < chans; ++c) {
                const double *v = in + l * line_in + c;
                double acc = 0.0;
                for (uint32_t j = 0; j < count; ++j) acc = acc + (w[j] * v[(size_t)(first + j) * stride]);
                out[l * line_out + (size_t)o * stride + c] = rtc_resize_canon(acc);
            }
        }
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

} // namespace

double rtc_resize_radius(uint32_t filter) {
    switch (filter) {
    case RTC_RESIZE_BOX: return 0.5;
    case RTC_RESIZE_TRIANGLE: return 1.0;
    case RTC_RESIZE_CATMULL_ROM: return 2.0;
    case RTC_RESIZE_MITCHELL: return 2.0;
    case RTC_RESIZE_LANCZOS3: return 3.0;
    default: return 0.0;
    }
}

void rtc_resize_range(uint32_t n_in, uint32_t n_out, double radius, uint32_t o, uint32_t *first, uint32_t *end) {
    const double scale = axis_scale(n_in, n_out), fs = scale > 1.0 ? scale : 1.0, support = radius * fs;
    const double c = ((double)o + 0.5) * scale;
    const double lo = std::floor((c - support) + 0.5), hi = std::floor((c + support) + 0.5);
    *first = lo > 0.0 ? (uint32_t)lo : 0u;
    *end = hi < (double)n_in ? (hi > 0.0 ? (uint32_t)hi : 0u) : n_in;
    if (*end < *first) *end = *first; // (never, by the header's rule: every output has a tap)
}

rtc_status rtc_resize_build_axis(uint32_t n_in, uint32_t n_out, uint32_t filter, ResizeAxis *out) {
    const double radius = rtc_resize_radius(filter);
    if (!out || n_in == 0u || n_out == 0u || radius == 0.0) return RTC_ERR_ARG;
    const uint32_t taps = n_in == n_out ? 1u : axis_taps(n_in, n_out, radius);
    if (taps > RTC_MAX_RESIZE_TAPS) return RTC_ERR_ARG;
    try {
        out->first.assign(n_out, 0u);
        out->count.assign(n_out, 0u);
        out->w.assign((size_t)n_out * taps, 0.0);
    } catch (const std::bad_alloc &) {
        return RTC_ERR_NOMEM;
    }
    out->n_in = n_in;
    out->n_out = n_out;
    out->filter = filter;
    out->taps = taps;
    if (n_in == n_out) {
        for (uint32_t o = 0; o < n_out; ++o) {
            out->first[o] = o;
            out->count[o] = 1u;
            out->w[o] = 1.0;
        }
        return RTC_OK;
    }
    const double scale = axis_scale(n_in, n_out), fs = scale > 1.0 ? scale : 1.0;
    for (uint32_t o = 0; o < n_out; ++o) {
        uint32_t first, end;
        rtc_resize_range(n_in, n_out, radius, o, &first, &end);
        const double c = ((double)o + 0.5) * scale;
        double *w = out->w.data() + (size_t)o * taps;
        double sum = 0.0;
        for (uint32_t j = 0; j < end - first; ++j) {
            w[j] = kernel_of(filter, ((((double)(first + j)) + 0.5) - c) / fs);
            sum = sum + w[j];
        }
        for (uint32_t j = 0; j < end - first; ++j) w[j] = w[j] / sum;
        out->first[o] = first;
        out->count[o] = end - first;
    }
    return RTC_OK;
}

void rtc_resize_plan(const ResizePlanInputs *in, ResizePlan *out) {
    std::memset(out, 0, sizeof *out);
    out->status = RTC_ERR_ARG;
    const double radius = rtc_resize_radius(in->filter);
    if (in->w_in == 0u || in->h_in == 0u || in->w_out == 0u || in->h_out == 0u || radius == 0.0) return;
    const bool run_h = in->w_in != in->w_out, run_v = in->h_in != in->h_out;
    if (!run_h && !run_v) {
        const uint64_t values = 3u * (uint64_t)in->w_in * in->h_in;
        out->copy_blocks = (values + RTC_RESIZE_BLOCK - 1u) / RTC_RESIZE_BLOCK;
        if (out->copy_blocks > RTC_RESIZE_MAX_BLOCKS) return;
        out->copy = 1u;
        out->status = RTC_OK;
        return;
    }
    // the grids that need no table first: a frame that is refused for its size costs no walk over its outputs
    if (run_v) {
        ResizePassPlan &p = out->v;
        p.seg = RTC_RESIZE_BLOCK;
        const uint64_t gx = (3u * (uint64_t)in->w_out + RTC_RESIZE_BLOCK - 1u) / RTC_RESIZE_BLOCK;
        uint64_t gy = ((uint64_t)in->h_out + RTC_RESIZE_V_ROWS - 1u) / RTC_RESIZE_V_ROWS;
        p.rows = RTC_RESIZE_V_ROWS;
        if (gx * gy < RTC_RESIZE_V_MIN_BLOCKS) { // a small output: more workgroups, each walking fewer source rows
            p.rows = 1u;
            gy = in->h_out;
        }
        p.blocks = gx * gy;
        if (p.blocks > RTC_RESIZE_MAX_BLOCKS) return;
        p.grid_x = (uint32_t)gx;
        p.grid_y = (uint32_t)gy;
    }
    if (run_h && (uint64_t)in->h_in > (uint64_t)RTC_RESIZE_MAX_BLOCKS * RTC_RESIZE_MAX_SEG) return; // (rows <= 256: at least h_in / 256 workgroups)
    if (run_v) {
        ResizePassPlan &p = out->v;
        p.taps = axis_taps(in->h_in, in->h_out, radius);
        if (p.taps > RTC_MAX_RESIZE_TAPS) return;
        p.table_bytes = (uint64_t)in->h_out * (p.taps + 1u) * sizeof(double);
        p.run = 1u;
    }
    if (run_h) {
        ResizePassPlan &p = out->h;
        p.taps = axis_taps(in->w_in, in->w_out, radius);
        if (p.taps > RTC_MAX_RESIZE_TAPS) return;
        p.table_bytes = (uint64_t)in->w_out * (p.taps + 1u) * sizeof(double);
        // The segment: as wide as the LDS budget lets one row's source span be. first and end never decrease along the
        // axis, so a segment's span runs from its first output's first to its last output's end.
        uint32_t seg = RTC_RESIZE_MAX_SEG, span = 0;
        for (;; seg /= 2u) {
            span = 0;
            for (uint64_t o0 = 0; o0 < in->w_out; o0 += seg) {
                const uint32_t o1 = (uint32_t)((o0 + seg < in->w_out ? o0 + seg : (uint64_t)in->w_out) - 1u);
                uint32_t f0, e0, f1, e1;
                rtc_resize_range(in->w_in, in->w_out, radius, (uint32_t)o0, &f0, &e0);
                rtc_resize_range(in->w_in, in->w_out, radius, o1, &f1, &e1);
                if (e1 - f0 > span) span = e1 - f0;
            }
            if (seg == 1u || (uint64_t)span * 24u <= RTC_RESIZE_LDS_BUDGET) break;
        }
        // Rows: enough for about 256 output pixels per workgroup when the segment (or the frame) is narrow, as many as the budget holds
        uint32_t rows = RTC_RESIZE_MAX_SEG / (seg < in->w_out ? seg : in->w_out);
        const uint32_t fit = (uint32_t)(RTC_RESIZE_LDS_BUDGET / ((uint64_t)span * 24u));
        if (rows > fit) rows = fit;
        if (rows > in->h_in) rows = in->h_in;
        if (rows < 1u) rows = 1u;
        p.seg = seg;
        p.rows = rows;
        p.span = span;
        p.lds_bytes = rows * span * 24u;
        const uint64_t gx = ((uint64_t)in->w_out + seg - 1u) / seg, gy = ((uint64_t)in->h_in + rows - 1u) / rows;
        p.blocks = gx * gy;
        if (p.blocks > RTC_RESIZE_MAX_BLOCKS || p.lds_bytes > RTC_RESIZE_LDS_BUDGET) return;
        p.grid_x = (uint32_t)gx;
        p.grid_y = (uint32_t)gy;
        p.run = 1u;
    }
    if (run_h && run_v) out->mid_bytes = (uint64_t)in->w_out * in->h_in * 24u;
    out->status = RTC_OK;
}

extern "C" {

rtc_status rtc_debug_plan_resize(const ResizePlanInputs *in, ResizePlan *out) {
    if (!in || !out) return RTC_ERR_ARG;
    rtc_resize_plan(in, out);
    return RTC_OK;
}

rtc_status rtc_resize_validate(const rtc_resize *spec) {
    if (!spec || spec->filter > RTC_RESIZE_LANCZOS3 || spec->_pad != 0u) return RTC_ERR_ARG;
    return RTC_OK;
}

uint32_t rtc_resize_taps(uint32_t n_in, uint32_t n_out, uint32_t filter) {
    const double radius = rtc_resize_radius(filter);
    if (n_in == 0u || n_out == 0u || radius == 0.0) return 0u;
    return n_in == n_out ? 1u : axis_taps(n_in, n_out, radius);
}

rtc_status rtc_resize_weights(uint32_t n_in, uint32_t n_out, const rtc_resize *spec, uint32_t *first, uint32_t *count, double *w) {
    if (!first || !count || !w || rtc_resize_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    ResizeAxis ax;
    const rtc_status st = rtc_resize_build_axis(n_in, n_out, spec->filter, &ax);
    if (st != RTC_OK) return st;
    std::memcpy(first, ax.first.data(), sizeof(uint32_t) * n_out);
    std::memcpy(count, ax.count.data(), sizeof(uint32_t) * n_out);
    std::memcpy(w, ax.w.data(), sizeof(double) * ax.w.size());
    return RTC_OK;
}

rtc_status rtc_canvas_resize(const double *in, uint32_t w_in, uint32_t h_in, const rtc_resize *spec, double *out, uint32_t w_out,
                             uint32_t h_out) {
    if (!in || !out || rtc_resize_validate(spec) != RTC_OK) return RTC_ERR_ARG;
    if (w_in == 0u || h_in == 0u || w_out == 0u || h_out == 0u) return RTC_ERR_ARG;
    const size_t n_in = 3u * (size_t)w_in * h_in, n_out = 3u * (size_t)w_out * h_out;
    if (overlap(in, n_in * sizeof(double), out, n_out * sizeof(double))) return RTC_ERR_ARG;
    const bool run_h = w_in != w_out, run_v = h_in != h_out;
    ResizeAxis ax_h, ax_v;
    if (run_h) {
        const rtc_status st = rtc_resize_build_axis(w_in, w_out, spec->filter, &ax_h);
        if (st != RTC_OK) return st;
    }
    if (run_v) {
        const rtc_status st = rtc_resize_build_axis(h_in, h_out, spec->filter, &ax_v);
        if (st != RTC_OK) return st;
    }
    if (!run_h && !run_v) { // neither axis is filtered: the input's bytes
        std::memcpy(out, in, n_in * sizeof(double));
        return RTC_OK;
    }
    if (!run_v) { // the vertical pass copies: the horizontal pass writes the frame
        pass(in, out, ax_h, h_in, 3u * (size_t)w_in, 3u * (size_t)w_out, 3u, 3u);
        return RTC_OK;
    }
    if (!run_h) { // the horizontal pass copies: a column's taps are a row pitch apart
        pass(in, out, ax_v, 1u, 0u, 0u, 3u * (size_t)w_out, 3u * (size_t)w_out);
        return RTC_OK;
    }
    std::vector<double> mid;
    try {
        mid.resize(3u * (size_t)w_out * h_in);
    } catch (const std::bad_alloc &) {
        return RTC_ERR_NOMEM;
    }
    pass(in, mid.data(), ax_h, h_in, 3u * (size_t)w_in, 3u * (size_t)w_out, 3u, 3u);
    pass(mid.data(), out, ax_v, 1u, 0u, 0u, 3u * (size_t)w_out, 3u * (size_t)w_out);
    return RTC_OK;
}

} // extern "C"
