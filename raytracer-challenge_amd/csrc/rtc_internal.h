// rtc_internal.h — host-side objects behind the opaque handles of include/rtc.h; shared by rtc_api.cpp
// (one GPU) and rtc_group.cpp (row tiles across GPUs). Not part of the ABI.
#ifndef RTC_INTERNAL_H
#define RTC_INTERNAL_H

#include <hip/hip_runtime.h>

#include <vector>

#include "rtc.h"
#include "rtc_devmem.h"
#include "rtc_device.h"
#include "rtc_gamma.h"
#include "rtc_world_build.h"

struct rtc_context {
    int device = -1;
    unsigned long long render_allocs = 0; // hipMalloc calls made by render entry points (rtc_debug_render_allocs)
    unsigned long long pixels = 0; // rtc_stats::pixels of the launches since the last reset (counted by the launch plan, rtc_launch_plan.h)
    hipStream_t stream = nullptr;
    DevBuf<unsigned long long> d_counters;
    // ring of (begin, end) event pairs, one per timed k_trace launch. Created on demand, EV_CHUNK pairs
    // at a time (a context that never renders creates none; creating all 2048 up front made
    // rtc_context_create the slowest call of a one-frame render)
    static constexpr uint32_t EV_RING = 1024, EV_CHUNK = 16;
    hipEvent_t ev[EV_RING][2] = {};
    hipEvent_t ev_bin[EV_RING][2] = {}; // the same for the launch's binning kernel (k_bin_tiles), when it has one
    bool bin_timed[EV_RING] = {};       // ... whether slot k's launch had one
    uint32_t ev_created = 0; // pairs [0, ev_created) exist
    uint64_t launches = 0; // render launches so far
    uint64_t timed = 0;    // ... of which carried an event pair (ring position)
    uint32_t time_every = 1; // rtc_context_set_timing
    // device canvas of rtc_render (host-canvas entry point): grow-only, reused between frames
    DevBuf<double> d_canvas;
    DevBuf<unsigned char> d_canvas8; // the same for rtc_render_rgb8 (3 B/pixel) and rtc_render_rgba8 (4 B/pixel)
    DevBuf<unsigned char> d_aov;     // the planes of rtc_render_aov (host-buffer entry point), carved in order of alignment
    // Ambient occlusion (rtc_render_ao*, include/rtc.h): the sample table of the most recent launch's grid, the host's
    // rtc_ao_expand, copied in stream order in front of the launch when the grid changes (one grid in a loop: one copy);
    // `ao_host` is the copy's source and is rewritten only behind a wait for the stream. The radius is a kernel argument.
    DevBuf<double> d_ao_dirs;        // room for RTC_MAX_AO_SAMPLES directions, allocated by the first AO launch
    double ao_host[3u * RTC_MAX_AO_SAMPLES] = {};
    uint32_t ao_usteps = 0, ao_vsteps = 0; // the grid d_ao_dirs holds; 0: none yet
    DevBuf<uint16_t> d_ao;           // the plane of rtc_render_ao (host-buffer entry point)
    DevBuf<double> d_gather;         // the planes of rtc_render_gather (host-buffer entry point): radiance, then bounce
    DevBuf<double> d_filter;         // the ping-pong plane of rtc_plane_filter_device: width*height*channels, when passes > 1
    // Edge-adaptive anti-aliasing (rtc_adaptive.cpp; include/rtc.h), all grow-only:
    DevBuf<uint32_t> d_aa_tiles;     // per 32x8 tile its count of flagged pixels, then its offset in the list, then the total
    DevBuf<uint32_t> d_aa_list;      // the flagged pixels' indices y*hsize + x, tile by tile
    DevBuf<unsigned char> d_aa_mask; // the mask of a call that was given none
    DevBuf<double> d_aa_rays;        // one chunk's rays, 6 doubles each, pixel-major with the samples innermost
    DevBuf<double> d_aa_colors;      // ... and their colours, 3 doubles each
    DevBuf<double> d_aa_canvas;      // the frame of rtc_render_adaptive (host-buffer entry point)
    PinnedWord aa_total;             // where the number of flagged pixels lands
    // Post-processing (rtc_post.cpp; include/rtc.h), grow-only:
    DevBuf<rtc_luminance> d_post_lum; // the block results of the statistics' levels 0 and 1 (frames of more than 256 pixels)
    DevBuf<double> d_post_hor;        // the bloom's horizontal pass H: three planes of width*height
    // Resizing (rtc_resize.cpp; include/rtc.h), grow-only. A slot holds the device table of one axis: n_out records {first,
    // count} (two uint32 in the room of a double), then n_out rows of `taps` weights. A slot is rewritten only on a miss,
    // behind a wait for the stream; `used` orders the slots for replacement (the smallest is the least recently used).
    static constexpr uint32_t RESIZE_SLOTS = 4;
    struct ResizeSlot {
        bool valid = false;
        uint32_t n_in = 0, n_out = 0, filter = 0, taps = 0;
        unsigned long long used = 0;
        DevBuf<double> table;
    };
    ResizeSlot resize_slot[RESIZE_SLOTS];
    unsigned long long resize_clock = 0;   // the `used` stamp of the most recent call
    unsigned long long resize_uploads = 0; // tables uploaded so far (rtc_debug_resize_uploads)
    DevBuf<double> d_resize_mid;           // the intermediate w_out x h_in frame of a resize that changes both axes
    int force_src = -1;   // RTC_SRC env override (experiments)
    uint32_t tiles_per_wg = 1; // tiles one workgroup renders in sequence (RTC_TILES_PER_WG)
    uint32_t tiles_guided_tenths = 20; // guided chunks: tiles per chunk level in tenths of the resident workgroups (RTC_TILES_GUIDED; 0 = off)
    uint32_t tiles_slots = 0;          // 0: from the kernel's occupancy; else the number of resident workgroups to assume (RTC_TILES_SLOTS, tests)
    uint32_t tiles_kmax = 8;           // ... largest chunk (RTC_TILES_KMAX: 1, 2, 3, 4 or 8)
    uint32_t tile_cap = 512;
    hipStream_t side_stream = nullptr; // created on demand: per-render binning kernels run here, beside the previous launch's render
    // Pipelined launches (rtc_context_set_pipeline, include/rtc.h): `lanes` > 1 deals consecutive render launches round-robin
    // over that many streams of the context's own, so launch i+1 fills the CUs launch i's last waves leave idle (Camera::
    // render_async returns a NEW Canvas per call, canvas.rs:26-41: consecutive frames never alias). A lane is in order:
    // [k_bin_tiles ->] k_trace, its own set of tile lists (rtc_world::bin[lane]), no cross-stream events at all.
    static constexpr uint32_t MAX_LANES = 4;
    hipStream_t lane[MAX_LANES] = {};
    uint32_t lanes = 1;       // 1 = every launch in order on `stream` (the default)
    uint64_t lane_next = 0;   // launches dealt so far
    // the source / lists the most recent render launch ran with (rtc_context_last_launch_info)
    rtc_launch_info last{};
    uint32_t last_projection = 0; // ... and its projection kind, 0: none (rtc_context_last_launch_projection)
    uint64_t launches_total = 0; // render launches since the context was created (never reset)
    // the tile lists the most recent render launch read, if it was binned (rtc_debug_tile_counts): the World's upload serial
    // (a World created later at the same address has another), which of its sets, and the launch's grid
    struct LastBin {
        uint64_t world_serial = 0; // 0: the last launch was not binned
        uint32_t set = 0, nviews = 0, tiles_x = 0, tiles_y = 0;
    } last_bin;
    hipEvent_t fence_ev = nullptr; // rtc_context_fence
    bool light_table = false; // RTC_LIGHT_TABLE=1: Worlds of 2..RTC_MAX_LIGHTS lights read them from the device table too (parity measurements)
    bool light_lists = true; // RTC_LIGHT_LISTS=0: shadow passes of two-level worlds walk the groups (A/B)
    bool world_update = true; // RTC_WORLD_UPDATE=0: render_lua destroys and recreates the World when a job's differs (A/B)
    bool binning = true;  // RTC_BINNING=0: primary rays take the wave-level cull / group walk too (A/B)
    bool sky_rows = true; // RTC_SKY_ROWS=0: tile rows the binning kernel proved black are traced like any other (A/B)
    // RTC_BIN_SORT=0: k_bin_tiles leaves every packed list in table order and the render kernels take the wave-minimum walk
    // (tests, A/B); otherwise the short lists of flat one-level worlds are sorted for the scalar walk (RTC_TILE_SORT_CAP).
    bool bin_sort = true;
    bool one_sample = true; // RTC_ONE_SAMPLE=0: launches of cameras with samples == 1 take the generic render kernel (A/B, parity tests)
    bool whole_tiles = true; // RTC_WHOLE_TILES=0: no launch takes the whole-tile render kernels (A/B, parity tests); RTC_ONE_SAMPLE=0 implies it
    bool uniform_shade = true; // RTC_UNIFORM_SHADE=0: the flat one-sample kernels shade every tile per lane, one-object tiles too (A/B, parity tests)
    // one-level worlds (<= 256 objects) are binned only in launches of at least this many views (RTC_BIN_SMALL_VIEWS): the
    // binning kernels run on the side stream beside the previous launch's render, which hides them when launches follow each
    // other (north star, 8 views per launch: 0.0745 -> 0.0685 ms per frame; 4 views: 0.0732 -> 0.0704; C4 1.48 -> 1.42;
    // C2 unchanged) but not in front of a lone one-view launch (0.0824 -> 0.0895). Before the side stream the same binning
    // gave the render kernel its 12 % and took it all back in launch latency (profiles/r02_exp_binned_small_worlds.log).
    // one-level worlds (n <= 256) are binned when the launch is long enough for the extra kernel and its two cross-stream
    // events to pay: views x pixels >= this (RTC_BIN_SMALL_PIXELS; 1080p: from 3 views per launch, 4096^2: always)
    unsigned long long bin_small_pixels = 6000000ull;
    // ... and in a pipelined context (lanes > 1), where the binning kernel of launch i+1 runs beside launch i's render on the
    // other lane without any event: from this many pixels (RTC_BIN_SMALL_PIXELS_PIPELINED)
    unsigned long long bin_small_pixels_pipelined = 1500000ull;
    // Gamma tables (rtc_gamma.h) of the RGBA entries: one slot of device memory per gamma, filled once — on the stream of
    // the first launch that needs it — and never written again while the slot holds that gamma, so launches with different
    // gammas may be in flight on different lanes at once. A stream that did not do the upload waits for it once (the
    // slot's `ready` event; `seen`: bit l = lane l, bit MAX_LANES = `stream`). When every slot is taken the context waits
    // for all its streams and starts the cache afresh.
    static constexpr uint32_t GAMMA_SLOTS = 16;
    struct GammaSlot {
        bool used = false;
        float gamma = 0.f;
        uint32_t seen = 0;
        hipEvent_t ready = nullptr;
        DevGamma host{}; // the upload's source: stays put as long as the slot holds this gamma
    };
    DevBuf<DevGamma> d_gamma; // GAMMA_SLOTS tables, allocated by the first RGBA call
    GammaSlot gamma_slot[GAMMA_SLOTS];
    // Panorama tables (rtc_render_projection*, include/rtc.h): {sin, cos} per column and per row of the frame, the host's
    // rtc_projection_tables, uploaded when the key changes — behind a wait for every stream of the context, since a launch
    // in flight may read the tables that are replaced (pano_tables, rtc_api.cpp). One panorama size in a loop: one upload.
    struct PanoKey {
        uint32_t hsize, vsize;
        double h_span, v_span;
    };
    DevBuf<double> d_pano_col, d_pano_row;
    PanoKey pano_key{};
    bool pano_valid = false;
    unsigned long long pano_uploads = 0; // uploads so far (rtc_debug_projection_uploads)
};

struct rtc_world {
    rtc_context *ctx = nullptr; // identity check only; never dereferenced at destroy time
    int device = -1;
    uint64_t serial = 0; // 1, 2, ... in order of rtc_world_create, process-wide: never reused
    // One generation of the World's contents: every table a launch is pointed at (fill_world) and the scalars that go with
    // them. rtc_world_create fills generation 0 from its host build; rtc_world_update builds the next one of the ring on the
    // device (rtc_world_build.h) while launches made earlier still read theirs. A generation is written again GENS updates
    // later, behind the `read` events of the launches that used it.
    struct Gen {
        unsigned char *slab = nullptr; // its share of rtc_world::slabs: the tables below and the build's scratch, laid out by carve_gen (rtc_api.cpp)
        uint32_t *lights = nullptr;    // its share of rtc_world::lights: the cells' counters, then light_cap_alloc entries per cell
        DevIsect *isect = nullptr;
        DevShade *shade = nullptr;
        DevIdEntry *idtab = nullptr;
        uint32_t *kind = nullptr; // isect .. kind: what the host flattens; the rest is derived from them
        DevBound *bound = nullptr;
        DevIsect *isect_s = nullptr; // Morton-sorted copies for the two-level cull
        uint32_t *kind_s = nullptr;
        DevBound *bound_s = nullptr;
        uint32_t *orig_s = nullptr;
        DevBound *gbound = nullptr;
        DevPre *pre = nullptr, *pre_s = nullptr; // per-lane prefilter records (insertion / sorted order)
        double *partial = nullptr;               // build scratch (WorldBuildArgs)
        unsigned long long *key = nullptr;
        uint32_t *idx = nullptr;
        DevWorldHeader *d_hdr = nullptr;
        uint32_t n = 0;
        uint32_t ngroups = 0;
        rtc_light light{};                     // L[0]: the light with the light-space lists
        uint32_t n_lights = 1;                 // 1 .. RTC_MAX_LIGHT_SAMPLES (an area light counts as its samples)
        rtc_light more[RTC_MAX_LIGHT_SAMPLES - 1]{}; // L[1 .. n_lights)
        double *ltab = nullptr;                // device table of L[1 ..): 6 doubles each, room for RTC_MAX_LIGHT_SAMPLES - 1 (carve_gen)
        bool light_table = false;              // launches read L[1 ..) from ltab (written with this generation) instead of their arguments
        bool any_refl = false, any_refr = false;
        uint32_t light_cap = 0;  // entries per cell of this generation's lists; 0: it has none
        // known to the host build at once; after a device build only once the header has arrived (hdr_pending)
        uint32_t n_unb = 0; // unbounded objects: the first n_unb entries of the Morton-sorted tables
        double pre_limit = 0.;
        double light_reach = 0.;
        // update bookkeeping
        bool hdr_pending = false;    // the first launch waits for `built` on the host and reads *h_hdr
        uint32_t light_cap_want = 0; // ... and light_cap becomes this if the header reports a reach
        hipEvent_t built = nullptr;  // recorded on the build stream behind the header copy
        bool device_built = false;   // written by an update (`built` has been recorded), not by rtc_world_create's host build
        uint32_t ordered = 0;        // device_built: the streams that are ordered behind `built` already (bit: stream_bit, rtc_api.cpp)
        hipEvent_t read[rtc_context::MAX_LANES + 1] = {}; // per render stream: behind its latest launch that used this generation
        uint32_t read_mask = 0;                           // ... which of them have been recorded since the generation was built
        unsigned char *stage = nullptr; // page-locked: the flattened shapes of the update that builds this generation
        DevWorldHeader *h_hdr = nullptr; // page-locked: where the header lands
    };
    static constexpr uint32_t GENS = rtc_context::MAX_LANES + 1u; // as many as output slots can be in flight (the idea of BinSet)
    mutable Gen gen[GENS]; // (rtc_render_* take the World as const)
    // ONE allocation each for every generation's tables and for every generation's light lists: rtc_world_create pays for two
    // hipMalloc calls however many generations there are (a World that is destroyed and created per frame must not pay per generation)
    DevBuf<unsigned char> slabs;
    DevBuf<uint32_t> lights;
    uint32_t cur = 0;      // the generation launches made now are given
    bool valid = true;     // false after a growing update that failed: gen[cur] points nowhere, renders are refused
    uint32_t cap_n = 0;           // objects every generation has room for
    uint32_t light_cap_alloc = 0; // entries per cell every generation's `lights` has room for (0: no lists)
    unsigned long long allocs = 0; // hipMalloc calls made for this World so far (rtc_debug_world_tables)
    mutable bool updated = false;   // since the first update every launch records a read event
    hipStream_t build_stream = nullptr; // created by the first update: uploads and build kernels, beside the renders
    unsigned char *pinned = nullptr;    // one page-locked block: every generation's stage and header slot
    DevBuf<DevPrim> d_prim; // per-render scratch of the brute-force variants
    // binned primary pass: per-render scratch, grow-only, TWO sets — the binning of launch k+1 runs on the context's side
    // stream while launch k's render kernel still reads set k (rtc_render_* take the World as const: mutable)
    struct BinSet {
        DevBuf<uint32_t> tile_cnt, tile_list; // per (view, tile): entries used, RTC_TILE_LIST_CAP entry slots (tile_cnt: RTC_BIN_ROW_WORDS row words first)
        DevBuf<DevPrim> prim;            // per (view, object): the primary rays' constants, written by the set's binning kernel
        hipEvent_t binned = nullptr;     // recorded on the side stream after the set's binning kernel
        hipEvent_t traced = nullptr;     // recorded on the render stream after the render kernel that read the set
    };
    mutable BinSet bin[rtc_context::MAX_LANES]; // in-order contexts alternate between [0] and [1]; a pipelined context's lane l owns [l]
    mutable uint32_t bin_next = 0;
    DevBuf<DevTileBundle> d_light_cells; // the lists' cone tables: the same for every World, written once
    bool light_cells_ready = false;
};


extern "C" hipError_t rtc_launch_binning(const DevCamera *views, uint32_t nviews, uint32_t W, uint32_t H, uint32_t n, const DevBound *bound_s,
                                         const DevBound *gbound, const uint32_t *orig_s, uint32_t ngroups, uint32_t *cnt, uint32_t *list,
                                         uint32_t row0, uint32_t row_stride, hipStream_t stream, hipEvent_t e0, hipEvent_t e1,
                                         const DevIsect *isect_s, const uint32_t *kind_s, uint32_t n_unb, uint32_t *rows,
                                         const DevIsect *isect, DevPrim *prim, uint32_t sort);
enum { RTC_BIN_ROW_WORDS = 2 * RTC_MAX_VIEWS }; // a BinSet's tile_cnt buffer starts with the views' row words (RenderParams::tile_rows)
extern "C" hipError_t rtc_launch_light_lists(uint32_t n, uint32_t cap, const DevBound *bound, const double light[3], double reach, DevTileBundle *cells,
                                             DevTileBundle *macros, uint32_t *cnt, uint32_t *list, hipStream_t stream);
extern "C" hipError_t rtc_launch_light_lists_built(uint32_t n, uint32_t cap, const DevBound *bound, const double light[3], const DevWorldHeader *hdr,
                                                   const DevTileBundle *cells, const DevTileBundle *macros, uint32_t *cnt, uint32_t *list,
                                                   hipStream_t stream);
extern "C" rtc_status rtc_gamma_build_table(float gamma, DevGamma *g); // host_ppm.cpp
extern "C" void rtc_projection_ortho_terms(uint32_t hsize, uint32_t vsize, double width, double out[3]); // host_math.cpp: half_w, half_h, pixel
// k_aov / k_aov_view (rtc_kernels.hip). `P`: the World's tables only (fill_world); xl / lt: lights_of, read with A->shadow;
// `proj`: NULL (the pinhole's centre rays) or the projection whose rays the pass casts (tile_pass fills it).
extern "C" hipError_t rtc_launch_aov(const AovParams *A, const RenderParams *P, int src, const DevExtraLights *xl, const DevLightTable *lt,
                                     const DevProjection *proj, hipStream_t stream);
extern "C" hipError_t rtc_launch_aov_view(const AovViewParams *V, hipStream_t stream);
// k_ao / k_apply_ao (rtc_kernels.hip). `P`: the World's tables only (fill_world); `dirs`: the sample table in device memory.
extern "C" hipError_t rtc_launch_ao(const AoParams *A, const double *dirs, const RenderParams *P, int src, const DevProjection *proj,
                                    hipStream_t stream);
extern "C" hipError_t rtc_launch_apply_ao(double *rgb, const uint16_t *ao, size_t n, uint32_t n_samples, double strength, hipStream_t stream);
// k_gather / k_add_scaled (rtc_kernels.hip). `P`, `dirs`: as rtc_launch_ao; `xl` / `lt` / `proj`: as rtc_launch_aov.
extern "C" hipError_t rtc_launch_gather(const GatherParams *A, const double *dirs, const RenderParams *P, int src, const DevExtraLights *xl,
                                        const DevLightTable *lt, const DevProjection *proj, hipStream_t stream);
extern "C" hipError_t rtc_launch_add_scaled(double *rgb, const double *plane, size_t n, double strength, hipStream_t stream);
extern "C" hipError_t rtc_launch_canvas_to_rgba8(const double *rgb, size_t n, const DevGamma *g, unsigned char *out, hipStream_t stream);
// k_average_over (rtc_shutter.hip): one pass of Color::average_over over whole canvases. Adds frames[f * stride + i], f = 0..nf-1
// in that order, to the carried sum (sum_in, NULL: 0.0) for i < count. divisor == 0: stores the sum to f64_out. Otherwise the
// last pass: divides by `divisor` and writes whichever of f64_out (the mean), rgb8 (Color::scale, 3 B/pixel) and rgba8
// (to_imgbuf through `g`, 4 B/pixel) are not NULL; the 8-bit outputs need count % 3 == 0. sum_in may equal f64_out.
struct AverageArgs {
    const double *frames;
    const double *sum_in;
    double *f64_out;
    unsigned char *rgb8, *rgba8;
    const DevGamma *g;
    size_t stride, count;
    double divisor;
    uint32_t nf; // 1..RTC_SHUTTER_RING
};
extern "C" hipError_t rtc_launch_average_over(const AverageArgs *a, hipStream_t stream);
// k_atrous (rtc_filter.hip): one pass of the edge-aware filter (include/rtc.h), src to dst (never the same plane), taps `step`
// pixels apart; `inv` = 1.0 / plane_sigma. grid_x is the launcher's own. k_counts_to_fraction / k_apply_occlusion beside it.
struct AtrousArgs {
    const double *src;
    double *dst;
    const int32_t *index;
    const double *point, *normal;
    double inv;
    uint32_t width, height, step, squarings, grid_x;
};
extern "C" hipError_t rtc_launch_atrous(const AtrousArgs *a, uint32_t channels, bool same, hipStream_t stream);
extern "C" hipError_t rtc_launch_counts_to_fraction(const uint16_t *counts, size_t px, uint32_t n, double *out, hipStream_t stream);
extern "C" hipError_t rtc_launch_apply_occlusion(double *rgb, const double *occ, size_t px, double strength, hipStream_t stream);
// Edge-adaptive anti-aliasing (rtc_adaptive.hip; include/rtc.h). Tiles are 32 x 8 pixels, numbered row-major.
enum { RTC_AA_TILE_W = 32, RTC_AA_TILE_H = 8 };
// k_aa_mask: the mask of the canvas `rgb` and, per tile, its number of 1 bytes in counts[tile]
extern "C" hipError_t rtc_launch_aa_mask(const double *rgb, uint32_t width, uint32_t height, uint32_t mode, double threshold, unsigned char *mask,
                                         uint32_t *counts, hipStream_t stream);
// k_aa_scan: offsets[t] = counts[0] + ... + counts[t-1] for the `tiles` tiles, *total = their sum; one workgroup
extern "C" hipError_t rtc_launch_aa_scan(const uint32_t *counts, uint32_t tiles, uint32_t *offsets, uint32_t *total, hipStream_t stream);
// k_aa_list: tile t's flagged pixels, row-major within the tile, as y*width + x in list[offsets[t] ...]
extern "C" hipError_t rtc_launch_aa_list(const unsigned char *mask, uint32_t width, uint32_t height, const uint32_t *counts, const uint32_t *offsets,
                                         uint32_t *list, hipStream_t stream);
// k_aa_rays / k_aa_resolve: the `pixels` list entries from `list` on, `usteps*vsteps` samples each
struct AaRayArgs {
    double half_width, half_height, pixel_size;
    double vinv[12];
    double origin[3]; // rtc_camera_ray_for_pixel's origin, evaluated by the host
    const uint32_t *list;
    double *rays;     // k_aa_rays: out, pixels * n * 6
    uint32_t width, usteps, vsteps, pixels;
};
extern "C" hipError_t rtc_launch_aa_rays(const AaRayArgs *a, hipStream_t stream);
extern "C" hipError_t rtc_launch_aa_resolve(const uint32_t *list, const double *colors, uint32_t pixels, uint32_t n, double *rgb, hipStream_t stream);
// The middle of rtc_color_at (rtc_api.cpp): World::color_at for n rays in DEVICE memory into d_rgb (n x 3 doubles) and, when
// not NULL, d_hits, enqueued on the context's stream behind a pending build of the World. `record`: the launch is not
// awaited by its caller, so a later rtc_world_update has to wait for it.
extern "C" rtc_status rtc_color_at_device(rtc_context *ctx, const rtc_world *w, const double *d_rays, uint32_t n, uint32_t remaining, uint32_t flags,
                                          double *d_rgb, rtc_hit *d_hits, bool record);
// Post-processing (rtc_post.hip; include/rtc.h). k_lum_pixels / k_lum_records: the statistics of the n pixels of `rgb` into *out
// (device memory), one launch per level of the tree; `scratch`: room for ceil(n/256) + ceil(ceil(n/256)/256) records when n > 256.
extern "C" hipError_t rtc_launch_luminance(const double *rgb, size_t n, rtc_luminance *scratch, rtc_luminance *out, hipStream_t stream);
// k_tonemap: `stats` (device memory) is read only with an AUTO flag; out may be in
extern "C" hipError_t rtc_launch_tonemap(const double *in, double *out, size_t n, const rtc_tonemap *spec, const rtc_luminance *stats,
                                         hipStream_t stream);
// k_bloom_h, then k_bloom_v: `hor` has room for three planes of width*height; w: rtc_bloom_weights; out may be in. grid_x is
// the launcher's own.
struct BloomArgs {
    const double *in;
    double *out;
    double *hor;
    double threshold, strength;
    double w[2u * RTC_MAX_BLOOM_RADIUS + 1u];
    uint32_t width, height, radius, grid_x;
};
extern "C" hipError_t rtc_launch_bloom(const BloomArgs *a, hipStream_t stream);
// Resizing (rtc_resize.hip; include/rtc.h). fc: n_out records {first, count}; w: n_out rows of `taps` weights; the geometry
// (taps .. grid_x) is filled by the launchers from the pass's plan (rtc_resize.h). k_resize_h: w_in x h_in -> w_out x h_in;
// k_resize_v: w_out x (the axis's n_in rows) -> w_out x h_out.
struct ResizeArgs {
    const double *in;
    double *out;
    const uint2 *fc;
    const double *w;
    uint32_t w_in, h_in, w_out, h_out;
    uint32_t taps, seg, rows, pitch, grid_x;
};
struct ResizePassPlan;
extern "C" hipError_t rtc_launch_resize_h(const ResizeArgs *a, const ResizePassPlan *p, hipStream_t stream);
extern "C" hipError_t rtc_launch_resize_v(const ResizeArgs *a, const ResizePassPlan *p, hipStream_t stream);
extern "C" hipError_t rtc_launch_resize_copy(const double *in, double *out, size_t n, hipStream_t stream); // n: values
extern "C" rtc_status rtc_shutter_check_motions(const rtc_motion *motions, uint32_t n_motions, uint32_t n_shapes, uint32_t samples); // host_math.cpp
// The device table of `gamma` for work enqueued next on the context's own stream (rtc_api.cpp keeps the per-gamma cache).
extern "C" rtc_status rtc_gamma_table_on_stream(rtc_context *ctx, float gamma, const DevGamma **out);
extern "C" hipError_t rtc_launch_undeal(const void *staging, void *canvas, uint32_t nranks, uint32_t nframes, uint32_t H,
                                        uint32_t rows_max, size_t row_bytes, hipStream_t stream);

#endif
