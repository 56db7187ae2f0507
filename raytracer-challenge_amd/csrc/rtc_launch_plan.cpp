// rtc_launch_plan.cpp — rtc_plan_launch (rtc_launch_plan.h): every decision of a launch, from plain numbers.
#include "rtc_launch_plan.h"

#include <algorithm>

namespace {

bool cull_src(int src) { return src == SRC_CULL || src == SRC_CULL2; }

// Where the kernel takes its object records from, and the LDS table that goes with it.
// `multi`: a launch whose kernels exist for SRC_SMEM, SRC_CULL and SRC_CULL2 only (several lights, a lens, AOV planes), so the
// brute-force choice is SRC_SMEM at every size; an LDS source can then only come out of RTC_FLAG_LDS_TABLE or an RTC_SRC
// override, which rtc_plan_launch refuses.
void choose_source(const LaunchPlanInputs &in, bool multi, LaunchPlan &out) {
    // per object in LDS: 96 B inverse rows + 32 B primary prologue + 4 B kind
    const uint32_t per_obj = 96 + 32 + 4;
    const uint32_t n = in.n;
    int s;
    if (in.force_src >= 0) s = in.force_src;
    else if (!(in.flags & RTC_FLAG_NO_CULL)) s = (n > 256) ? SRC_CULL2 : SRC_CULL; // default: per-wave conservative cull,
                                                                                 // two-level above 4 groups of 64
    else if (in.flags & RTC_FLAG_LDS_TABLE) s = SRC_LDS1; // brute force over the LDS-staged object table (LDS tiles when it does not fit)
    else if (n <= 128 || multi) s = SRC_SMEM;
    else if (n <= 448) s = SRC_LDS1;
    else s = SRC_LDSN;
    uint32_t cap = 0;
    if (s == SRC_LDS1) {
        if ((uint64_t)n * per_obj > 150 * 1024) s = SRC_LDSN;
        else cap = n ? n : 1;
    }
    if (s == SRC_LDSN) cap = in.tile_cap;
    out.src = s;
    out.tile_cap = cap;
    // kinds sit behind cap*16 doubles; round the block up to 16 bytes
    out.lds_bytes = cap ? (uint32_t)(((uint64_t)cap * per_obj + 15) & ~(uint64_t)15) : 0;
}

// Binned primary pass (tile rows aligned with the image's): one small kernel puts every object on the list of each 8x8 tile
// its bounding sphere can touch (same conservative predicate as the wave-level cull), so the render kernel's primary pass
// runs exact tests on a short list instead of walking the groups. Two-level worlds always; one-level worlds when the launch
// is long enough for the extra kernel (and, in order on one stream, its two cross-stream events) to pay: the thresholds
// count the pixels THIS launch renders — whole frames or one rank's bands (k_bin_tiles lists only the tile rows the launch
// renders). Never for a lens launch: tile lists, black tile rows and DevPrim all assume rays from the camera origin.
void plan_binning(const LaunchPlanInputs &in, bool lens, LaunchPlan &out) {
    const uint64_t threshold = in.pipelined ? in.bin_small_pixels_pipelined : in.bin_small_pixels;
    const bool pays = out.src == SRC_CULL2 || (out.src == SRC_CULL && out.launch_pixels >= threshold);
    out.bin = pays && in.binning && (in.y0 % 8u) == 0u && in.n != 0u && !lens;
    out.tiles_x = (in.hsize + 7u) / 8u;
    out.tiles_y = (in.vsize + 7u) / 8u;
    const uint64_t per_view = (uint64_t)out.tiles_x * out.tiles_y;
    out.tiles = per_view * in.nviews;
    out.prims = (uint64_t)in.n * in.nviews;
    // Capacity. A pipelined lane's lists are sized for the largest launch seen. In order, both sets are made ready by the
    // FIRST binned launch, and for RTC_MAX_VIEWS views while that stays within 128 MB per set (1080p: 67 MB; larger frames:
    // exactly the launch's views, growing once if a later launch has more): a launch sequence must not allocate after its
    // first launch — hipMalloc / hipFree wait for the device, 0.2-3 ms in the middle of a frame sequence (a 5-frame warm-up
    // launch followed by 8-frame launches did exactly that: 0.09-0.22 ms per frame instead of 0.07).
    const uint64_t per_view_bytes = per_view * sizeof(uint32_t) * (1u + RTC_TILE_LIST_CAP);
    const uint32_t alloc_views = (!in.pipelined && per_view_bytes * RTC_MAX_VIEWS <= ((uint64_t)128 << 20)) ? (uint32_t)RTC_MAX_VIEWS : in.nviews;
    out.tiles_alloc = per_view * alloc_views;
    out.prims_alloc = (uint64_t)in.n * std::max(alloc_views, in.nviews);
}

// Guided chunks (RenderParams::chunk_wgs): with `slots` workgroups resident at once, the launch's last f x slots tiles go one
// per workgroup, the f x slots before them two, then three, four, and everything earlier eight (f = RTC_TILES_GUIDED
// tenths, default 2.0; 0 = off; the largest chunk = RTC_TILES_KMAX). Launches of fewer than 3 rounds of workgroups are left alone.
void plan_chunks(const LaunchPlanInputs &in, bool lens, LaunchPlan &out) {
    static const uint32_t sizes[5] = {1u, 2u, 3u, 4u, 8u}; // chunk sizes from the END of the launch backwards
    out.chunk_wgs[0] = out.chunk_wgs[1] = out.chunk_wgs[2] = out.chunk_wgs[3] = 0u;
    out.grid_wgs = (out.total_blocks + out.reps - 1u) / out.reps;
    const uint32_t slots = in.tiles_slots ? in.tiles_slots : (1024u * (out.refl ? 4u : 5u) / std::max(1u, out.block / 64u));
    const uint64_t per_level = (uint64_t)slots * in.tiles_guided_tenths / 10u;
    uint32_t nlevels = 1;
    while (nlevels < 5u && sizes[nlevels] <= in.tiles_kmax) ++nlevels;
    // Not for a large world on a small frame (C3: 10 000 spheres at 1080p): there the NEXT launch's binning kernel is as long
    // as this render kernel, and its few waves wait for slots that long-lived workgroups free late — the solo kernel gains
    // 6 %, the pipelined frame loses 9 % (profiles/r03_exp_tiles_per_workgroup.log).
    const bool heavy_binning = in.n > 4096u && out.launch_pixels < 8000000ull;
    if (out.reps != 1u || per_level == 0u || nlevels == 1u || out.total_blocks < 3u * slots || heavy_binning || lens) return;
    uint64_t rest = out.total_blocks, tiles[5] = {0, 0, 0, 0, 0};
    for (uint32_t l = 0; l < nlevels && rest; ++l) {
        uint64_t tk = (l + 1u == nlevels) ? rest : std::min(rest, per_level);
        if (l) tk -= tk % sizes[l]; // whole workgroups; what does not divide joins the single-tile level
        tiles[l] = tk;
        rest -= tk;
    }
    tiles[0] += rest;
    out.chunk_wgs[0] = (uint32_t)(tiles[4] / 8u); out.chunk_wgs[1] = (uint32_t)(tiles[3] / 4u);
    out.chunk_wgs[2] = (uint32_t)(tiles[2] / 3u); out.chunk_wgs[3] = (uint32_t)(tiles[1] / 2u);
    out.grid_wgs = out.chunk_wgs[0] + out.chunk_wgs[1] + out.chunk_wgs[2] + out.chunk_wgs[3] + (uint32_t)tiles[0];
}

// rtc_stats::pixels of the launch (the kernel traces exactly the pixels of its rows; Camera::render leaves the last row and
// column alone, camera.rs:120-121): counted on the host, one atomic per wave less
uint64_t counted_pixels(const LaunchPlanInputs &in) {
    const bool serial = in.mode == RTC_MODE_RENDER;
    uint64_t rows = 0;
    for (uint32_t k = 0; k < in.grid_y; ++k) {
        const uint64_t py0 = (uint64_t)in.y0 + (uint64_t)k * in.band_stride * 8u;
        if (py0 >= in.y1) break;
        uint64_t r = in.y1 - py0 < 8u ? in.y1 - py0 : 8u;
        if (serial && py0 + r == in.vsize) --r; // the image's last row
        rows += r;
    }
    return rows * (in.hsize - (serial ? 1u : 0u)) * in.nviews;
}

} // namespace

void rtc_plan_launch(const LaunchPlanInputs &in, LaunchPlan &out) {
    out = LaunchPlan{};
    const bool lens = in.kind == RTC_PLAN_FRAME && in.lens_samples != 0u, probe = in.kind == RTC_PLAN_PROBE;
    const bool multi = in.n_lights > 1u || lens || in.kind == RTC_PLAN_AOV;
    choose_source(in, multi, out);
    out.status = RTC_OK;
    // there are no multi-light, lens or AOV kernels for the LDS sources (RTC_FLAG_LDS_TABLE, RTC_SRC=1|2)
    if (multi && (out.src == SRC_LDS1 || out.src == SRC_LDSN)) out.status = RTC_ERR_UNSUPPORTED;
    if (in.kind == RTC_PLAN_AOV && (in.flags & RTC_FLAG_LDS_TABLE)) out.status = RTC_ERR_UNSUPPORTED; // ... culled or not
    out.refl = (in.any_refl || in.any_refr) ? 1u : 0u;
    out.refr = in.any_refr ? 1u : 0u;
    out.flags = lens ? in.flags & ~(uint32_t)RTC_FLAG_AA_RESAMPLE : in.flags;
    out.reps = 1u;
    out.lane_dealt = cull_src(out.src); // the brute-force variants share one per-render table (rtc_world::d_prim)
    if (in.kind == RTC_PLAN_AOV) { // k_aov: one wave = one tile = one workgroup, no dynamic LDS
        out.block = 64u;
        out.tile_w = 8u;
        out.lds_bytes = out.tile_cap = 0u;
        out.grid_x = (in.hsize + 7u) / 8u;
        out.total_blocks = out.grid_wgs = out.grid_x * ((in.vsize + 7u) / 8u);
        return;
    }
    const int cull = CULL_LEVEL(out.src);
    out.block = RTC_BLOCK_FOR(cull, out.refl, out.refr, probe);
    out.tile_w = RTC_TILE_W_FOR(cull, out.refl, out.refr, probe);
    if (probe) {
        out.grid_x = (in.hsize + out.block - 1u) / out.block;
        out.total_blocks = out.grid_wgs = out.grid_x;
        return;
    }
    out.grid_x = (in.hsize + out.tile_w - 1u) / out.tile_w;
    out.total_blocks = out.grid_x * in.grid_y * in.nviews;
    if (in.samples != 1u) { // the 4 sub-samples of every pixel wait in LDS for the resample test (camera.rs:108)
        out.aa_lds_off = out.lds_bytes;
        out.lds_bytes += out.block * 15u * (uint32_t)sizeof(double); // + the running sums
        // Camera::resample traces `antialiasing_samples` more rays (camera.rs:87); u8 in the reference
        out.resample_n = (out.flags & RTC_FLAG_AA_RESAMPLE) ? (in.samples & 0xffu) : 0u;
    }
    // a lens launch runs no per-view table either, and launches one workgroup per tile, every tile row included
    out.needs_prep = !cull_src(out.src) && !lens;
    out.reps = lens ? 1u : in.tiles_per_wg;
    out.launch_pixels = (uint64_t)in.nviews * in.hsize * std::min<uint64_t>((uint64_t)in.grid_y * 8u, in.vsize);
    plan_binning(in, lens, out);
    plan_chunks(in, lens, out);
    out.counted_pixels = counted_pixels(in);
}

extern "C" rtc_status rtc_debug_plan_launch(const LaunchPlanInputs *in, LaunchPlan *out) {
    if (!in || !out || in->kind > RTC_PLAN_AOV) return RTC_ERR_ARG;
    rtc_plan_launch(*in, *out);
    return RTC_OK;
}
