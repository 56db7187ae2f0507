// rtc_api.cpp — [device] half of the C-ABI in include/rtc.h: context, HBM-resident World,
// render / color_at launches. Compiled by hipcc together with rtc_kernels.hip.
//
// There is deliberately no CPU fallback here: without a usable gfx950 device every entry
// point returns RTC_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "rtc.h"
#include "rtc_ao.h"
#include "rtc_aov.h"
#include "rtc_device.h"
#include "rtc_gather.h"
#include "rtc_internal.h"
#include "rtc_launch_plan.h"
#include "rtc_parity.h"

extern "C" hipError_t rtc_launch_trace(const RenderParams *P, int src, int refl, int refr, uint32_t nblocks,
                                       size_t lds_bytes, hipStream_t stream, hipEvent_t e0, hipEvent_t e1, const DevExtraLights *xl,
                                       const DevLightTable *lt, const DevLens *lens, const DevProjection *proj, int one_sample,
                                       int whole_tiles, int uniform_shade);
extern "C" hipError_t rtc_launch_prep(const DevIsect *isect, DevPrim *prim, uint32_t n, const double vinv[12],
                                      hipStream_t stream);
extern "C" hipError_t rtc_launch_arith(uint32_t op, const double *a, const double *b, uint32_t n, double *out,
                                       hipStream_t stream);

namespace {

#define HIP_TRY(expr)                                   \
    do {                                                \
        if ((expr) != hipSuccess) return RTC_ERR_DEVICE; \
    } while (0)

struct DeviceGuard { // make ctx->device current for the calling thread
    explicit DeviceGuard(int dev) { ok = hipSetDevice(dev) == hipSuccess; }
    bool ok;
};

// Pipelined context: wait for every lane (in-order contexts have none).
hipError_t drain_lanes(rtc_context *ctx) {
    for (uint32_t l = 0; l < rtc_context::MAX_LANES; ++l)
        if (ctx->lane[l]) {
            const hipError_t e = hipStreamSynchronize(ctx->lane[l]);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// 63-bit Morton key of a point inside the box [lo, hi]^3 (21 bits per axis).
uint64_t spread21(uint64_t v) {
    v &= 0x1fffffULL;
    v = (v | (v << 32)) & 0x1f00000000ffffULL;
    v = (v | (v << 16)) & 0x1f0000ff0000ffULL;
    v = (v | (v << 8)) & 0x100f00f00f00f00fULL;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ULL;
    v = (v | (v << 2)) & 0x1249249249249249ULL;
    return v;
}
constexpr size_t LIGHT_CELLS = 6u * (size_t)RTC_LIGHT_R * RTC_LIGHT_R, LIGHT_MACROS = 6u * (size_t)(RTC_LIGHT_R / 8u) * (RTC_LIGHT_R / 8u);

uint64_t morton_key(const DevBound &b, const double lo[3], const double hi[3]) {
    uint64_t k = 0;
    const double c[3] = {b.cx, b.cy, b.cz};
    for (int a = 0; a < 3; ++a) {
        const double ext = hi[a] - lo[a];
        double u = ext > 0. ? (c[a] - lo[a]) / ext : 0.;
        if (!(u >= 0.)) u = 0.;
        if (u > 1.) u = 1.;
        k |= spread21((uint64_t)(u * 2097151.0)) << a;
    }
    return k;
}

// World-space bounding sphere of a shape, derived from the stored inverse transform only (that is
// what the kernels intersect with): the surface is { F p : p on the unit sphere / cube } with
// F = inv^-1 (affine part). Conservative: radius = largest singular value of F's 3x3 (spheres) or
// the farthest transformed corner (cubes), inflated by 1e-6; anything not clearly well-conditioned
// gets r = +inf and is simply never culled.
DevBound bound_of(const rtc_shape &s) {
    DevBound b{0., 0., 0., INFINITY, 0., 0.};
    if (s.kind == RTC_PLANE) return b;
    const double *m = s.inv;
    const double a[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
    const double t[3] = {m[3], m[7], m[11]};
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(t[i])) return b;
        for (int j = 0; j < 3; ++j)
            if (!std::isfinite(a[i][j])) return b;
    }
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    if (!(std::fabs(det) > 1e-300) || !std::isfinite(det)) return b;
    double f[3][3]; // F3 = a^-1 by cofactors
    f[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) / det;
    f[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det;
    f[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
    f[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) / det;
    f[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det;
    f[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
    f[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) / det;
    f[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
    f[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
    double resid = 0., fmaxabs = 0.; // || a F - I ||_max: refuse to trust an ill-conditioned inverse
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double v = (i == j) ? -1. : 0.;
            for (int k = 0; k < 3; ++k) v += a[i][k] * f[k][j];
            resid = std::fmax(resid, std::fabs(v));
            fmaxabs = std::fmax(fmaxabs, std::fabs(f[i][j]));
            if (!std::isfinite(f[i][j])) return b;
        }
    if (!(resid < 1e-9)) return b;
    double c[3];
    for (int i = 0; i < 3; ++i) c[i] = -(f[i][0] * t[0] + f[i][1] * t[1] + f[i][2] * t[2]);
    double r2;
    if (s.kind == RTC_SPHERE) {
        // lambda_max of S = F F^T by cyclic Jacobi
        double S[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) S[i][j] = f[i][0] * f[j][0] + f[i][1] * f[j][1] + f[i][2] * f[j][2];
        for (int sweep = 0; sweep < 30; ++sweep) {
            const double off = std::fabs(S[0][1]) + std::fabs(S[0][2]) + std::fabs(S[1][2]);
            if (off < 1e-300) break;
            for (int p = 0; p < 2; ++p)
                for (int q = p + 1; q < 3; ++q) {
                    if (S[p][q] == 0.) continue;
                    const double th = (S[q][q] - S[p][p]) / (2. * S[p][q]);
                    const double tt = (th >= 0. ? 1. : -1.) / (std::fabs(th) + std::sqrt(th * th + 1.));
                    const double cs = 1. / std::sqrt(tt * tt + 1.), sn = tt * cs;
                    for (int k = 0; k < 3; ++k) { // S <- S J
                        const double skp = S[k][p], skq = S[k][q];
                        S[k][p] = cs * skp - sn * skq;
                        S[k][q] = sn * skp + cs * skq;
                    }
                    for (int k = 0; k < 3; ++k) { // S <- J^T S
                        const double spk = S[p][k], sqk = S[q][k];
                        S[p][k] = cs * spk - sn * sqk;
                        S[q][k] = sn * spk + cs * sqk;
                    }
                }
        }
        // Gershgorin guard on whatever off-diagonal mass is left
        const double g = std::fabs(S[0][1]) + std::fabs(S[0][2]) + std::fabs(S[1][2]);
        r2 = std::fmax(S[0][0], std::fmax(S[1][1], S[2][2])) + 2. * g;
    } else { // cube: farthest of the 8 transformed corners
        r2 = 0.;
        for (int k = 0; k < 8; ++k) {
            const double px = (k & 1) ? 1. : -1., py = (k & 2) ? 1. : -1., pz = (k & 4) ? 1. : -1.;
            double q = 0.;
            for (int i = 0; i < 3; ++i) {
                const double v = f[i][0] * px + f[i][1] * py + f[i][2] * pz;
                q += v * v;
            }
            r2 = std::fmax(r2, q);
        }
    }
    if (!std::isfinite(r2) || !(r2 >= 0.)) return b;
    const double cn = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const double r = std::sqrt(r2) * (1. + 1e-6) + 1e-9 * (1. + cn) + 1e-7 * fmaxabs;
    if (!std::isfinite(r) || !std::isfinite(cn)) return b;
    double na2 = 0.; // ||A||_F^2 >= ||A||_2^2
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) na2 += a[i][j] * a[i][j];
    const double k = 0.75e-14 * na2;
    if (!std::isfinite(k)) return b;
    b.cx = c[0]; b.cy = c[1]; b.cz = c[2]; b.r = r;
    b.k = k;
    b.cn = cn;
    return b;
}

void fill_camera(RenderParams &P, const rtc_camera *cam, uint32_t view = 0) {
    if (view == 0) {
        P.W = cam->hsize;
        P.H = cam->vsize;
        // antialiasing_samples == 1 is the one-ray branch; every other value (0 included) the sub-sample
        // branch (camera.rs:96-99)
        P.samples = cam->samples == 1u ? 1u : 4u;
    }
    DevCamera &c = P.views[view];
    c.half_width = cam->half_width;
    c.half_height = cam->half_height;
    c.pixel_size = cam->pixel_size;
    std::memcpy(c.vinv, cam->view_inv, sizeof(double) * 12);
    // transform_point(vinv, (0,0,0)) in xpoint's operation order (rtc_kernels.hip; this file is compiled without
    // contraction, as the kernels are). Not a copy of the translation column: (+0) + (-0) has to come out as it does there.
    const double *m = c.vinv;
    const double zero = 0.;
    bool finite = true;
    for (int i = 0; i < 12; ++i) finite = finite && std::isfinite(m[i]);
    for (int r = 0; r < 3; ++r) c.origin[r] = m[4 * r] * zero + m[4 * r + 1] * zero + m[4 * r + 2] * zero + m[4 * r + 3];
    c.origin_ok = finite ? 1u : 0u;
    c._pad = 0u;
}

void fill_world(RenderParams &P, const rtc_world::Gen &G) {
    P.isect = G.isect;
    P.kind = G.kind;
    P.shade = G.shade;
    P.bound = G.bound;
    P.isect_s = G.isect_s;
    P.kind_s = G.kind_s;
    P.bound_s = G.bound_s;
    P.orig_s = G.orig_s;
    P.gbound = G.gbound;
    P.idtab = G.idtab;
    P.pre = G.pre;
    P.pre_s = G.pre_s;
    P.pre_limit = G.pre_limit;
    P.light_cnt = G.light_cap ? G.lights : nullptr;
    P.light_list = G.light_cap ? G.lights + LIGHT_CELLS : nullptr;
    P.light_reach = G.light_reach;
    P.light_cap = G.light_cap;
    P.n_unb = G.n_unb;
    P.ngroups = G.ngroups;
    P.n = G.n;
    for (int i = 0; i < 3; ++i) {
        P.light_pos[i] = G.light.position[i];
        P.light_int[i] = G.light.intensity[i];
    }
}

// The further lights of generation G as k_trace's trailing argument: *xl (the kernel-argument block) or *lt (the
// generation's device table, Gen::light_table); both nullptr for a one-light World (the kernels without that argument).
// (Whether the launch's source has multi-light kernels at all is the plan's business: rtc_launch_plan.h.)
struct LaunchLights {
    DevExtraLights extra;
    DevLightTable table;
    const DevExtraLights *xl = nullptr;
    const DevLightTable *lt = nullptr;
};
void lights_of(const rtc_world::Gen &G, LaunchLights &L) {
    L.xl = nullptr;
    L.lt = nullptr;
    if (G.n_lights <= 1u) return;
    if (G.light_table) {
        L.table.rec = G.ltab;
        L.table.n = G.n_lights - 1u;
        L.lt = &L.table;
        return;
    }
    DevExtraLights &X = L.extra;
    std::memset(&X, 0, sizeof X);
    X.n = G.n_lights - 1u;
    for (uint32_t i = 0; i < X.n; ++i)
        for (int k = 0; k < 3; ++k) {
            X.pos[i][k] = G.more[i].position[k];
            X.inten[i][k] = G.more[i].intensity[k];
        }
    L.xl = &X;
}

// L[0] and L[1..n) of a generation, from the caller's array. More than RTC_MAX_LIGHTS of them (or RTC_LIGHT_TABLE=1 and
// more than one) reach the kernels through the generation's device table, which the caller then writes (light_records).
void set_lights(const rtc_context *ctx, rtc_world::Gen &G, const rtc_light *lights, uint32_t n_lights) {
    G.light = lights[0];
    G.n_lights = n_lights;
    for (uint32_t i = 1; i < n_lights; ++i) G.more[i - 1u] = lights[i];
    G.light_table = n_lights > RTC_MAX_LIGHTS || (ctx->light_table && n_lights > 1u);
}
// The table's records of L[1..n): position, then intensity (DevLightTable)
constexpr size_t LIGHT_TABLE_DOUBLES = 6u * (RTC_MAX_LIGHT_SAMPLES - 1u);
void light_records(const rtc_world::Gen &G, double *rec) {
    for (uint32_t i = 0; i + 1u < G.n_lights; ++i)
        for (int k = 0; k < 3; ++k) {
            rec[6u * i + k] = G.more[i].position[k];
            rec[6u * i + 3u + k] = G.more[i].intensity[k];
        }
}
// A World's lights as its sample list (12 KB, on the caller's stack: the update path makes no heap allocation either):
// RTC_OK and 1 <= *n <= RTC_MAX_LIGHT_SAMPLES, or rtc_area_light_expand's RTC_ERR_ARG
struct LightSamples {
    rtc_light at[RTC_MAX_LIGHT_SAMPLES];
};
rtc_status expand_lights(const rtc_area_light *lights, uint32_t n_lights, LightSamples &out, uint32_t *n) {
    if (!lights) return RTC_ERR_ARG;
    return rtc_area_light_expand(lights, n_lights, out.at, RTC_MAX_LIGHT_SAMPLES, n);
}

// ---- generations (rtc_world::Gen)

// Which of a context's streams: lane l, the context's own stream, its side stream (bits of Gen::ordered; the first
// MAX_LANES + 1 index Gen::read).
constexpr uint32_t BIT_STREAM = rtc_context::MAX_LANES, BIT_SIDE = rtc_context::MAX_LANES + 1u;

// Entries per cell of the light lists of a World of n shapes (0: none) — the sizing half of rtc_world_create's rules; the
// other half, a usable reach, is known only once the bounds are.
uint32_t light_cap_for(uint32_t n) { return n >= 32u ? (n > 256u ? RTC_LIGHT_LIST_CAP : RTC_LIGHT_LIST_CAP_SMALL) : 0u; }

// Points G's tables into its slab for a World of n shapes and returns the bytes they take. isect, shade, idtab and kind —
// what the host flattens — come first, `*staged` bytes in all: an update stages them in the same layout and copies them at once.
// The light table is the last of them (always room for RTC_MAX_LIGHT_SAMPLES - 1 records): a generation that does not use
// it stages and copies only the bytes in front of it.
size_t carve_gen(rtc_world::Gen &G, uint32_t n, size_t *staged) {
    const size_t na = n ? n : 1u, ng = n ? (n + 63u) / 64u : 1u, npad = rtc_world_build_npad(n);
    unsigned char *base = G.slab;
    size_t off = 0;
    auto take = [&](auto *&p, size_t count) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
        off += (count * sizeof(*p) + 255u) & ~(size_t)255u;
    };
    take(G.isect, na);
    take(G.shade, na);
    take(G.idtab, na);
    take(G.kind, na);
    take(G.ltab, LIGHT_TABLE_DOUBLES);
    if (staged) *staged = off;
    take(G.bound, na);
    take(G.isect_s, na);
    take(G.kind_s, na);
    take(G.bound_s, na);
    take(G.orig_s, na);
    take(G.gbound, ng);
    take(G.pre, na);
    take(G.pre_s, na);
    take(G.partial, ng * RTC_WB_PARTIALS);
    take(G.key, npad);
    take(G.idx, npad);
    take(G.d_hdr, 1);
    return off;
}

// Room in every generation for `cap_n` shapes and light lists of `light_cap` entries per cell, and the brute-force
// variants' scratch. Grow-only; what grows is freed first, so nothing may be in flight. The lists are an optimisation (the
// shadow pass walks without them): when there is no memory for them the World has none.
rtc_status reserve_generations(rtc_world *w, uint32_t cap_n, uint32_t light_cap) {
    rtc_world::Gen sizing;
    const size_t bytes = carve_gen(sizing, std::max(cap_n, w->cap_n), nullptr);
    if (w->slabs.capacity() < bytes * rtc_world::GENS) {
        const rtc_status st = w->slabs.reserve(bytes * rtc_world::GENS, &w->allocs);
        for (uint32_t g = 0; g < rtc_world::GENS; ++g) w->gen[g].slab = st == RTC_OK ? w->slabs.get() + bytes * g : nullptr;
        if (st != RTC_OK) return st;
    }
    if (cap_n > w->cap_n) w->cap_n = cap_n;
    const size_t na = cap_n ? cap_n : 1u;
    if (w->d_prim.capacity() < na) {
        const rtc_status st = w->d_prim.reserve(na, &w->allocs);
        if (st != RTC_OK) return st;
        if (hipMemset(w->d_prim.get(), 0, sizeof(DevPrim) * na) != hipSuccess) return RTC_ERR_DEVICE;
    }
    if (light_cap > w->light_cap_alloc) {
        const size_t per = LIGHT_CELLS * (1u + (size_t)light_cap);
        const bool got = w->d_light_cells.reserve(LIGHT_CELLS + LIGHT_MACROS, &w->allocs) == RTC_OK &&
                         w->lights.reserve(per * rtc_world::GENS, &w->allocs) == RTC_OK;
        if (!got) w->lights.reset();
        for (uint32_t g = 0; g < rtc_world::GENS; ++g) w->gen[g].lights = got ? w->lights.get() + per * g : nullptr;
        w->light_cap_alloc = got ? light_cap : 0u;
    }
    return RTC_OK;
}

// rtc_world_create's and rtc_world_update's checks of the shapes.
rtc_status check_shapes(const rtc_shape *shapes, uint32_t n) {
    // Material::lighting panics when a material has neither colour nor pattern (material.rs:328-331)
    for (uint32_t i = 0; i < n; ++i) {
        if (shapes[i].kind > RTC_CUBE || shapes[i].material.pattern_kind > RTC_PATTERN_GRID) return RTC_ERR_ARG;
        if (shapes[i].material.pattern_kind == RTC_PATTERN_NONE && !shapes[i].material.has_color) return RTC_ERR_NO_COLOR;
    }
    return RTC_OK;
}

// The shapes as the kernels read them: max(n, 1) records each of isect, kind, shade and idtab (zero beyond n).
void flatten_shapes(const rtc_shape *shapes, uint32_t n, DevIsect *isect, uint32_t *kind, DevShade *shade, DevIdEntry *idtab, bool *refl,
                    bool *refr) {
    const uint32_t na = n ? n : 1;
    std::memset(isect, 0, sizeof(DevIsect) * na);
    std::memset(kind, 0, sizeof(uint32_t) * na);
    std::memset(shade, 0, sizeof(DevShade) * na);
    bool any_refl = false, any_refr = false;
    // World::add_shape numbers the shapes last_world_id + 1 (shape.rs:661-667). A caller that leaves every id
    // 0 (rtc_shape_init does) gets exactly that numbering; ids that were given are honoured as they are —
    // equal ids are ONE container to compute_refractive (shape.rs:127), which is also what the reference's
    // own u8 ids do beyond 255 shapes.
    bool all_zero = true;
    for (uint32_t i = 0; i < n; ++i) all_zero = all_zero && shapes[i].world_id == 0u;
    idtab[0] = DevIdEntry{0u, 0u};
    for (uint32_t i = 0; i < n; ++i) idtab[i] = DevIdEntry{i, all_zero ? i + 1u : shapes[i].world_id};
    std::stable_sort(idtab, idtab + n, [](const DevIdEntry &a, const DevIdEntry &b) { return a.id < b.id; });
    for (uint32_t i = 0; i < n; ++i) {
        const rtc_shape &s = shapes[i];
        const rtc_material &m = s.material;
        std::memcpy(isect[i].m, s.inv, sizeof(double) * 12);
        kind[i] = s.kind;
        DevShade &d = shade[i];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                // Shape::normal_at uses transform_transpose (shape.rs:38); Cube::normal_at
                // transposes its inverse on the fly (shape.rs:627)
                d.nt[r * 3 + c] = (s.kind == RTC_CUBE) ? s.inv[c * 4 + r] : s.inv_t[r * 4 + c];
        for (int c = 0; c < 3; ++c) {
            d.color[c] = m.color[c];
            d.pat_a[c] = m.pat_a[c];
            d.pat_b[c] = m.pat_b[c];
        }
        d.ambient = m.ambient;
        d.diffuse = m.diffuse;
        d.specular = m.specular;
        d.shininess = m.shininess;
        d.reflective = m.reflective;
        d.transparency = m.transparency;
        d.refractive_index = m.refractive_index;
        std::memcpy(d.pat_inv, m.pat_inv, sizeof(double) * 12);
        if (s.kind == RTC_PLANE) {
            // world_normal = local_normal.transform(inverse_transpose).normalize() with local_normal
            // (0,1,0) (shape.rs:37-39, 481-483; transform.rs:114-117; vec.rs:65-76): mul/add/sqrt/div
            // in the reference's order, correctly rounded on the host exactly as on the device
            // (this file is compiled with -ffp-contract=off)
            const double *t = d.nt;
            const double wx = t[0] * 0. + t[1] * 1. + t[2] * 0.;
            const double wy = t[3] * 0. + t[4] * 1. + t[5] * 0.;
            const double wz = t[6] * 0. + t[7] * 1. + t[8] * 0.;
            const double mag = std::sqrt(wx * wx + wy * wy + wz * wz);
            d.plane_n[0] = wx / mag;
            d.plane_n[1] = wy / mag;
            d.plane_n[2] = wz / mag;
        }
        d.kind = s.kind;
        d.pattern_kind = m.pattern_kind;
        d.world_id = all_zero ? i + 1u : s.world_id;
        if (!(m.reflective <= 0.)) any_refl = true; // reflected_color shape.rs:730: `<= 0.` returns BLACK, so a NaN casts the ray
        if (m.transparency != 0.0) any_refr = true; // refracted_color shape.rs:752
    }
    *refl = any_refl;
    *refr = any_refr;
}

// The generation a launch made now renders, its header read (Gen::hdr_pending): the one host wait of an update's
// consumer — for the build kernels only, which nothing but the previous update precedes on their stream.
rtc_status current_gen(const rtc_world *w, rtc_world::Gen **out) {
    if (!w->valid) return RTC_ERR_NOMEM; // a growing update failed half way: no contents until an update succeeds
    rtc_world::Gen &G = w->gen[w->cur];
    if (G.hdr_pending) {
        HIP_TRY(hipEventSynchronize(G.built));
        G.n_unb = G.h_hdr->n_unb;
        G.pre_limit = G.h_hdr->pre_limit;
        G.light_reach = G.h_hdr->light_reach;
        G.light_cap = G.light_reach > 0. ? G.light_cap_want : 0u;
        G.hdr_pending = false;
    }
    *out = &G;
    return RTC_OK;
}
// Orders work enqueued next on `stream` (stream `bit`) behind G's build, once per stream.
hipError_t order_behind_build(rtc_world::Gen &G, hipStream_t stream, uint32_t bit) {
    if (!G.device_built || (G.ordered & (1u << bit))) return hipSuccess; // (a host build was complete before rtc_world_create returned)
    G.ordered |= 1u << bit;
    return hipStreamWaitEvent(stream, G.built, 0);
}
// A launch on `stream` (lane l, or BIT_STREAM) has read G: the update that writes G next waits for it on its own stream.
hipError_t record_read(const rtc_world *w, rtc_world::Gen &G, hipStream_t stream, uint32_t bit) {
    if (!w->updated) return hipSuccess; // the first update records for everything launched before it
    G.read_mask |= 1u << bit;
    return hipEventRecord(G.read[bit], stream);
}

// The RGBA entries accept what Canvas::set_gamma can meaningfully hold: a positive, finite gamma.
bool gamma_ok(float gamma) { return gamma > 0.f && std::isfinite(gamma); }

// The device table of `gamma` (rtc_gamma.h), readable by work enqueued next on `stream` — stream bit `bit` of
// rtc_context::GammaSlot::seen (lane l: l, the context's own stream: MAX_LANES). See rtc_context::gamma_slot.
rtc_status gamma_table(rtc_context *ctx, float gamma, hipStream_t stream, uint32_t bit, const DevGamma **out) {
    constexpr uint32_t NS = rtc_context::GAMMA_SLOTS;
    const rtc_status as = ctx->d_gamma.reserve(NS);
    if (as != RTC_OK) return as;
    uint32_t s = 0;
    while (s < NS && !(ctx->gamma_slot[s].used && ctx->gamma_slot[s].gamma == gamma)) ++s;
    if (s == NS) { // a new gamma: a free slot, or — all taken — wait until nothing can read any table, then start afresh
        s = 0;
        while (s < NS && ctx->gamma_slot[s].used) ++s;
        if (s == NS) {
            HIP_TRY(drain_lanes(ctx));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            for (rtc_context::GammaSlot &sl : ctx->gamma_slot) { sl.used = false; sl.seen = 0; }
            s = 0;
        }
        rtc_context::GammaSlot &sl = ctx->gamma_slot[s];
        const rtc_status st = rtc_gamma_build_table(gamma, &sl.host);
        if (st != RTC_OK) return st;
        if (!sl.ready) HIP_TRY(hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming));
        HIP_TRY(hipMemcpyAsync(ctx->d_gamma.get() + s, &sl.host, sizeof(DevGamma), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(sl.ready, stream));
        sl.used = true;
        sl.gamma = gamma;
        sl.seen = 1u << bit;
    } else if (!(ctx->gamma_slot[s].seen & (1u << bit))) { // uploaded on another stream: wait for that copy once
        HIP_TRY(hipStreamWaitEvent(stream, ctx->gamma_slot[s].ready, 0));
        ctx->gamma_slot[s].seen |= 1u << bit;
    }
    *out = ctx->d_gamma.get() + s;
    return RTC_OK;
}

// The context's timing event pairs [ev_created, upto) (rtc_context::ev, ev_bin).
hipError_t create_events(rtc_context *ctx, uint32_t upto) {
    for (uint32_t k = ctx->ev_created; k < upto; ++k) {
        for (hipEvent_t *e : {&ctx->ev[k][0], &ctx->ev[k][1], &ctx->ev_bin[k][0], &ctx->ev_bin[k][1]}) {
            const hipError_t r = hipEventCreate(e);
            if (r != hipSuccess) return r;
        }
        ctx->ev_created = k + 1;
    }
    return hipSuccess;
}

} // namespace

extern "C" {

rtc_status rtc_context_create(int32_t device, void *stream, rtc_context **out) {
    if (!out) return RTC_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return RTC_ERR_DEVICE;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RTC_ERR_DEVICE; // kernels are gfx950-only
    rtc_context *ctx = new (std::nothrow) rtc_context;
    if (!ctx) return RTC_ERR_NOMEM;
    ctx->device = device;
    ctx->stream = static_cast<hipStream_t>(stream); // NULL = the device's default stream

    if (ctx->d_counters.reserve(CNT_N * CNT_SLOTS) != RTC_OK ||
        hipMemsetAsync(ctx->d_counters.get(), 0, sizeof(unsigned long long) * CNT_N * CNT_SLOTS, ctx->stream) != hipSuccess) {
        rtc_context_destroy(ctx);
        return RTC_ERR_DEVICE;
    }
    if (const char *e = std::getenv("RTC_SRC")) {
        const int v = std::atoi(e);
        if (v >= 0 && v <= 4) ctx->force_src = v;
    }
    if (const char *e = std::getenv("RTC_BINNING")) ctx->binning = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_LIGHT_LISTS")) ctx->light_lists = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_LIGHT_TABLE")) ctx->light_table = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_WORLD_UPDATE")) ctx->world_update = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_SKY_ROWS")) ctx->sky_rows = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_BIN_SORT")) ctx->bin_sort = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_ONE_SAMPLE")) ctx->one_sample = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_WHOLE_TILES")) ctx->whole_tiles = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_UNIFORM_SHADE")) ctx->uniform_shade = std::atoi(e) != 0;
    if (const char *e = std::getenv("RTC_BIN_SMALL_PIXELS")) ctx->bin_small_pixels = std::strtoull(e, nullptr, 10);
    if (const char *e = std::getenv("RTC_BIN_SMALL_PIXELS_PIPELINED")) ctx->bin_small_pixels_pipelined = std::strtoull(e, nullptr, 10);
    if (const char *e = std::getenv("RTC_TILES_PER_WG")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 16) ctx->tiles_per_wg = (uint32_t)v;
    }
    if (const char *e = std::getenv("RTC_TILES_GUIDED")) { // tenths of `slots` tiles per chunk level (RenderParams::chunk_wgs); 0 = off
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 0 && v <= 1000) ctx->tiles_guided_tenths = (uint32_t)v;
    }
    if (const char *e = std::getenv("RTC_TILES_SLOTS")) { // tests: pretend this many workgroups are resident, so that small launches get every chunk level
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 0 && v <= 1000000) ctx->tiles_slots = (uint32_t)v;
    }
    if (const char *e = std::getenv("RTC_TILES_KMAX")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 8) ctx->tiles_kmax = (uint32_t)v;
    }
    if (const char *e = std::getenv("RTC_TILE_CAP")) {
        const int v = std::atoi(e);
        if (v >= 16 && v <= 1024) ctx->tile_cap = (uint32_t)v;
    }
    *out = ctx;
    return RTC_OK;
}

void rtc_context_destroy(rtc_context *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)drain_lanes(ctx);
    for (hipStream_t &l : ctx->lane)
        if (l) { (void)hipStreamDestroy(l); l = nullptr; }
    for (rtc_context::GammaSlot &sl : ctx->gamma_slot)
        if (sl.ready) (void)hipEventDestroy(sl.ready);
    if (ctx->side_stream) { (void)hipStreamSynchronize(ctx->side_stream); (void)hipStreamDestroy(ctx->side_stream); }
    if (ctx->fence_ev) (void)hipEventDestroy(ctx->fence_ev);
    for (auto &pair : ctx->ev)
        for (hipEvent_t e : pair)
            if (e) (void)hipEventDestroy(e);
    for (auto &pair : ctx->ev_bin)
        for (hipEvent_t e : pair)
            if (e) (void)hipEventDestroy(e);
    delete ctx; // its device buffers too: the device is current and its streams are idle
}

rtc_status rtc_context_synchronize(rtc_context *ctx) {
    if (!ctx) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(drain_lanes(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RTC_OK;
}

rtc_status rtc_context_set_pipeline(rtc_context *ctx, uint32_t depth) {
    if (!ctx || depth == 0 || depth > rtc_context::MAX_LANES) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(drain_lanes(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    if (depth > 1)
        for (uint32_t l = 0; l < depth; ++l)
            if (!ctx->lane[l]) HIP_TRY(hipStreamCreateWithFlags(&ctx->lane[l], hipStreamNonBlocking));
    ctx->lanes = depth;
    ctx->lane_next = 0;
    return RTC_OK;
}

rtc_status rtc_context_fence(rtc_context *ctx) {
    if (!ctx) return RTC_ERR_ARG;
    if (ctx->lanes <= 1) return RTC_OK; // in order on the stream already
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->fence_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->fence_ev, hipEventDisableTiming));
    for (uint32_t l = 0; l < rtc_context::MAX_LANES; ++l)
        if (ctx->lane[l]) {
            HIP_TRY(hipEventRecord(ctx->fence_ev, ctx->lane[l]));
            HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->fence_ev, 0)); // (the wait captures the record made just above)
        }
    return RTC_OK;
}

rtc_status rtc_context_last_launch_info(rtc_context *ctx, rtc_launch_info *out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    if (ctx->launches_total == 0) return RTC_ERR_ARG; // nothing launched yet
    *out = ctx->last;
    return RTC_OK;
}

rtc_status rtc_context_last_launch_projection(rtc_context *ctx, uint32_t *out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    if (ctx->launches_total == 0) return RTC_ERR_ARG; // nothing launched yet
    *out = ctx->last_projection;
    return RTC_OK;
}

rtc_status rtc_context_device_info(rtc_context *ctx, char *name, size_t cap, int32_t *compute_units, int32_t *clock_mhz) {
    if (!ctx) return RTC_ERR_ARG;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ctx->device));
    if (name && cap) {
        std::strncpy(name, prop.name, cap - 1);
        name[cap - 1] = 0;
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (clock_mhz) *clock_mhz = prop.clockRate / 1000;
    return RTC_OK;
}

static_assert(RTC_DEV_MAX_LIGHTS == RTC_MAX_LIGHTS && RTC_DEV_MAX_LIGHT_SAMPLES == RTC_MAX_LIGHT_SAMPLES, "include/rtc.h and rtc_device.h disagree");

rtc_status rtc_world_create(rtc_context *ctx, const rtc_shape *shapes, uint32_t n, const rtc_light *light, rtc_world **out) {
    return rtc_world_create_lights(ctx, shapes, n, light, 1u, out);
}

static rtc_status world_create(rtc_context *ctx, const rtc_shape *shapes, uint32_t n, const rtc_light *lights, uint32_t n_lights,
                               rtc_world **out);
static rtc_status world_update(rtc_context *ctx, rtc_world *w, const rtc_shape *shapes, uint32_t n, const rtc_light *lights,
                               uint32_t n_lights);

rtc_status rtc_world_create_lights(rtc_context *ctx, const rtc_shape *shapes, uint32_t n, const rtc_light *lights, uint32_t n_lights,
                                   rtc_world **out) {
    if (!ctx || !out || !lights || (n && !shapes) || n_lights == 0u || n_lights > RTC_MAX_LIGHTS) return RTC_ERR_ARG;
    return world_create(ctx, shapes, n, lights, n_lights, out);
}

// A World of area lights is the World of their samples (include/rtc.h): up to RTC_MAX_LIGHTS of them take
// rtc_world_create_lights' path as they are, more go through the generation's device table (set_lights).
rtc_status rtc_world_create_area_lights(rtc_context *ctx, const rtc_shape *shapes, uint32_t n, const rtc_area_light *lights,
                                        uint32_t n_lights, rtc_world **out) {
    if (!ctx || !out || !lights || (n && !shapes)) return RTC_ERR_ARG;
    *out = nullptr;
    LightSamples samples;
    uint32_t n_samples = 0;
    const rtc_status es = expand_lights(lights, n_lights, samples, &n_samples);
    if (es != RTC_OK) return es;
    return world_create(ctx, shapes, n, samples.at, n_samples, out);
}

rtc_status rtc_world_update_area_lights(rtc_context *ctx, rtc_world *w, const rtc_shape *shapes, uint32_t n,
                                        const rtc_area_light *lights, uint32_t n_lights) {
    if (!ctx || !w || !lights || (n && !shapes) || w->ctx != ctx) return RTC_ERR_ARG;
    LightSamples samples;
    uint32_t n_samples = 0;
    const rtc_status es = expand_lights(lights, n_lights, samples, &n_samples);
    if (es != RTC_OK) return es;
    return world_update(ctx, w, shapes, n, samples.at, n_samples);
}

// (the light-space lists are L[0]'s: `light` below; 1 <= n_lights <= RTC_MAX_LIGHT_SAMPLES, checked by the callers)
static rtc_status world_create(rtc_context *ctx, const rtc_shape *shapes, uint32_t n, const rtc_light *lights, uint32_t n_lights,
                               rtc_world **out) {
    const rtc_light *light = lights;
    *out = nullptr;
    const rtc_status cs = check_shapes(shapes, n);
    if (cs != RTC_OK) return cs;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t na = n ? n : 1;
    std::vector<DevIsect> isect(na);
    std::vector<uint32_t> kind(na, 0);
    std::vector<DevShade> shade(na);
    std::vector<DevBound> bound(na);
    std::vector<DevIdEntry> idtab(na, DevIdEntry{0u, 0u});
    bool any_refl = false, any_refr = false;
    flatten_shapes(shapes, n, isect.data(), kind.data(), shade.data(), idtab.data(), &any_refl, &any_refr);
    for (uint32_t i = 0; i < n; ++i) bound[i] = bound_of(shapes[i]);
    // ---- two-level cull tables: unbounded objects first, the rest in Morton order of their centres;
    // groups of 64 consecutive entries get a sphere around their members (inf if any is unbounded)
    std::vector<uint32_t> order(na, 0);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t i = 0; i < n; ++i)
            if (std::isfinite(bound[i].r)) {
                const double c[3] = {bound[i].cx, bound[i].cy, bound[i].cz};
                for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], c[a]); hi[a] = std::fmax(hi[a], c[a]); }
            }
        std::vector<uint64_t> key(na, 0);
        for (uint32_t i = 0; i < n; ++i) key[i] = std::isfinite(bound[i].r) ? (1ULL << 63) | morton_key(bound[i], lo, hi) : 0ULL;
        std::stable_sort(order.begin(), order.begin() + n, [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    }
    const uint32_t ngroups = (n + 63u) / 64u;
    std::vector<DevIsect> isect_s(na);
    std::vector<uint32_t> kind_s(na, 0), orig_s(na, 0);
    std::vector<DevBound> bound_s(na), gbound(ngroups ? ngroups : 1);
    std::memset(isect_s.data(), 0, sizeof(DevIsect) * na);
    for (uint32_t i = 0; i < na; ++i) bound_s[i] = DevBound{0., 0., 0., INFINITY, 0., 0.};
    for (uint32_t i = 0; i < n; ++i) {
        isect_s[i] = isect[order[i]];
        kind_s[i] = kind[order[i]];
        bound_s[i] = bound[order[i]];
        orig_s[i] = order[i];
    }
    gbound[0] = DevBound{0., 0., 0., INFINITY, 0., 0.};
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t a = g * 64u, b = (a + 64u < n) ? a + 64u : n;
        DevBound gb{0., 0., 0., INFINITY, 0., 0.};
        bool finite = true;
        double cx = 0., cy = 0., cz = 0., kmax = 0., cnmax = 0.;
        for (uint32_t i = a; i < b; ++i) {
            if (!std::isfinite(bound_s[i].r)) { finite = false; break; }
            cx += bound_s[i].cx; cy += bound_s[i].cy; cz += bound_s[i].cz;
            kmax = std::fmax(kmax, bound_s[i].k);
            cnmax = std::fmax(cnmax, bound_s[i].cn);
        }
        if (finite && b > a) {
            const double cnt = (double)(b - a);
            cx /= cnt; cy /= cnt; cz /= cnt;
            double r = 0.;
            for (uint32_t i = a; i < b; ++i) {
                const double dx = bound_s[i].cx - cx, dy = bound_s[i].cy - cy, dz = bound_s[i].cz - cz;
                r = std::fmax(r, std::sqrt(dx * dx + dy * dy + dz * dz) + bound_s[i].r);
            }
            r = r * (1. + 1e-9) + 1e-12;
            // rounding inflation of the group: members' radii inflate by at most
            // r_i*k_i*D_i*(cn_i + D_i) with D_i <= D_group + r_group; folded into the group's k/cn
            // conservatively: k = max k_i, cn = max cn_i + r (so that D_group + cn covers D_i + cn_i)
            if (std::isfinite(r) && std::isfinite(cx) && std::isfinite(cy) && std::isfinite(cz))
                gb = DevBound{cx, cy, cz, r, kmax * 4., cnmax + 2. * r};
        }
        gbound[g] = gb;
    }

    // per-lane prefilter records (DevPre, rtc_device.h): pre-inflated for every ray origin within 64x the extent of the bounded
    // objects around the world origin (secondary rays start on surfaces; a floor hit near the horizon can be farther: such a pass
    // takes the general test). The inflation is relative ~k*D^2 (1e-13 * 1e4..1e8 for ordinary scenes): generous limits cost nothing.
    double extent = 1.;
    for (uint32_t i = 0; i < n; ++i)
        if (std::isfinite(bound[i].r)) extent = std::fmax(extent, std::fabs(bound[i].cx) + std::fabs(bound[i].cy) + std::fabs(bound[i].cz) + bound[i].r);
    const double pre_limit = 64. * extent;
    auto pre_of = [&](const DevBound &b) {
        DevPre q{b.cx, b.cy, b.cz, INFINITY};
        if (std::isfinite(b.r) && std::isfinite(pre_limit)) {
            const double Dw = (std::fabs(b.cx) + std::fabs(b.cy) + std::fabs(b.cz) + pre_limit) * (1. + 1e-12);
            const double R = ((b.r + b.r * (b.k * Dw * (b.cn + Dw))) * 1.000001 + 1e-12) * (1. + 1e-12);
            const double R2 = R * R * (1. + 1e-12);
            if (std::isfinite(R2)) q.R2 = R2;
        }
        return q;
    };
    std::vector<DevPre> pre(na), pre_s(na);
    for (uint32_t i = 0; i < na; ++i) pre[i] = pre_s[i] = DevPre{0., 0., 0., INFINITY};
    for (uint32_t i = 0; i < n; ++i) { pre[i] = pre_of(bound[i]); pre_s[i] = pre_of(bound_s[i]); }

    rtc_world *w = new (std::nothrow) rtc_world;
    if (!w) return RTC_ERR_NOMEM;
    w->ctx = ctx;
    static std::atomic<uint64_t> uploads{0};
    w->serial = ++uploads;
    w->device = ctx->device;
    rtc_world::Gen &G = w->gen[0]; // the host build fills generation 0; the others wait for updates
    G.pre_limit = std::isfinite(pre_limit) ? pre_limit : 0.;
    G.ngroups = ngroups;
    G.n = n;
    set_lights(ctx, G, lights, n_lights);
    G.any_refl = any_refl;
    G.any_refr = any_refr;
    for (uint32_t i = 0; i < n; ++i)
        if (!std::isfinite(bound_s[i].r)) G.n_unb = i + 1u; // unbounded objects sort first (key 0)
    rtc_status st = reserve_generations(w, n, light_cap_for(n));
    if (st == RTC_OK) carve_gen(G, n, nullptr);
    auto upload = [&st](auto *dst, const auto &host) {
        if (st == RTC_OK) st = rtc_status_of(hipMemcpy(dst, host.data(), host.size() * sizeof(*dst), hipMemcpyHostToDevice));
    };
    upload(G.isect, isect);
    upload(G.kind, kind);
    upload(G.shade, shade);
    upload(G.bound, bound);
    upload(G.isect_s, isect_s);
    upload(G.kind_s, kind_s);
    upload(G.bound_s, bound_s);
    upload(G.orig_s, orig_s);
    upload(G.gbound, gbound);
    upload(G.idtab, idtab);
    upload(G.pre, pre);
    upload(G.pre_s, pre_s);
    if (G.light_table) {
        std::vector<double> rec(LIGHT_TABLE_DOUBLES, 0.);
        light_records(G, rec.data());
        upload(G.ltab, rec);
    }
    // light-space shadow lists: every shadow segment ends at the light, so the objects a segment can meet
    // are listed per direction cell of a cube map around the light, once per World. Reach = twice the far side of the
    // farthest bounded object as seen from the light (longer segments fall back to the group walk).
    if (st == RTC_OK && w->light_cap_alloc) { // (a handful of objects, n < 32: one cull step is cheaper than finding the cells — Criterion scene 33.5 vs 37.8 us)
        double far = 0.;
        for (uint32_t i = 0; i < n; ++i)
            if (std::isfinite(bound[i].r)) {
                const double dx = bound[i].cx - light->position[0], dy = bound[i].cy - light->position[1], dz = bound[i].cz - light->position[2];
                far = std::fmax(far, std::sqrt(dx * dx + dy * dy + dz * dz) + bound[i].r);
            }
        const double reach = 2. * far;
        if (std::isfinite(reach) && reach > 0. && reach < 1e30 && std::isfinite(light->position[0]) && std::isfinite(light->position[1]) &&
            std::isfinite(light->position[2])) {
            G.light_cap = light_cap_for(n);
            DevTileBundle *cell = w->d_light_cells.get();
            st = rtc_status_of(rtc_launch_light_lists(n, G.light_cap, G.bound, light->position, reach, cell, cell + LIGHT_CELLS, G.lights,
                                                      G.lights + LIGHT_CELLS, ctx->stream));
            if (st == RTC_OK) st = rtc_status_of(hipStreamSynchronize(ctx->stream));
            G.light_reach = reach;
            w->light_cells_ready = true;
        }
    }
    if (st != RTC_OK) {
        (void)hipGetLastError();
        rtc_world_destroy(w);
        return st;
    }
    *out = w;
    return RTC_OK;
}

// The streams, events and page-locked memory updates need: the first update makes them, a growing one the memory again.
static rtc_status ready_update(rtc_world *w) {
    if (!w->build_stream) HIP_TRY(hipStreamCreateWithFlags(&w->build_stream, hipStreamNonBlocking));
    for (rtc_world::Gen &G : w->gen) {
        if (!G.built) HIP_TRY(hipEventCreateWithFlags(&G.built, hipEventDisableTiming));
        for (hipEvent_t &e : G.read)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    rtc_world::Gen sizing;
    size_t staged = 0;
    carve_gen(sizing, w->cap_n, &staged);
    const size_t slot = staged + 256u; // + the header
    if (w->pinned && w->gen[1].stage == w->pinned + slot) return RTC_OK; // laid out for this capacity already
    if (w->pinned) (void)hipHostFree(w->pinned);
    w->pinned = nullptr;
    if (hipHostMalloc(reinterpret_cast<void **>(&w->pinned), slot * rtc_world::GENS, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return RTC_ERR_NOMEM;
    }
    for (uint32_t g = 0; g < rtc_world::GENS; ++g) {
        w->gen[g].stage = w->pinned + slot * g;
        w->gen[g].h_hdr = reinterpret_cast<DevWorldHeader *>(w->gen[g].stage + staged);
    }
    return RTC_OK;
}

// Replaces the contents of a resident World, ordered like a launch. The host flattens the shapes into the page-locked
// stage of the next generation of the ring; the copy and the build kernels (rtc_world_build.h, then the light lists) go
// to the World's build stream, behind the read events of the launches that last used that generation — a wait on the
// stream, never on the host — and run beside the renders in flight, which read other generations. Launches made after
// the call are given the new generation and wait, on their stream, for its `built` event.
//
// k_trace and k_bin_tiles take n_unb, pre_limit and light_reach by argument, and only the build knows them: the first
// render launch after an update therefore waits ON THE HOST for the generation's header, which is copied into a pinned
// 32-byte slot right behind the build (current_gen). That wait is for the small build kernels alone, which run beside
// the previous frame's render; it never waits for a render kernel.
//
// No hipMalloc, hipFree or hipDeviceSynchronize while the World's capacity suffices: n <= the largest count it has held,
// and light lists no larger than it has (the n >= 32 / n > 256 rules). Otherwise the slow path: wait for everything the
// context has in flight, grow every generation, go on as above; a World whose growing fails (RTC_ERR_NOMEM) has lost its
// contents: until an update succeeds every render of it returns RTC_ERR_NOMEM (rtc_world::valid). (The first update also creates the build stream, the events and the
// page-locked block.)
rtc_status rtc_world_update(rtc_context *ctx, rtc_world *w, const rtc_shape *shapes, uint32_t n, const rtc_light *light) {
    return rtc_world_update_lights(ctx, w, shapes, n, light, 1u);
}

uint32_t rtc_world_light_count(const rtc_world *w) { return w ? w->gen[w->cur].n_lights : 0u; }

// (the lights are host-side state of the generation: they reach the device in each launch's arguments, so a changed count
// costs nothing here)
rtc_status rtc_world_update_lights(rtc_context *ctx, rtc_world *w, const rtc_shape *shapes, uint32_t n, const rtc_light *lights,
                                   uint32_t n_lights) {
    if (!ctx || !w || !lights || (n && !shapes) || w->ctx != ctx || n_lights == 0u || n_lights > RTC_MAX_LIGHTS) return RTC_ERR_ARG;
    return world_update(ctx, w, shapes, n, lights, n_lights);
}

// (a generation with a light table stages its records behind the flattened shapes: one copy, in stream order with them)
static rtc_status world_update(rtc_context *ctx, rtc_world *w, const rtc_shape *shapes, uint32_t n, const rtc_light *lights,
                               uint32_t n_lights) {
    const rtc_light *light = lights;
    const rtc_status cs = check_shapes(shapes, n);
    if (cs != RTC_OK) return cs;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t light_cap = light_cap_for(n);
    if (n > w->cap_n || light_cap > w->light_cap_alloc) { // (a World that could not get its lists tries again each time it is updated)
        HIP_TRY(drain_lanes(ctx));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
        if (w->build_stream) HIP_TRY(hipStreamSynchronize(w->build_stream));
        w->valid = false; // the slabs are freed and allocated again: until this call has succeeded the World has no contents
        const rtc_status rs = reserve_generations(w, std::max(n, w->cap_n), std::max(light_cap, w->light_cap_alloc));
        if (rs != RTC_OK) return rs;
        for (rtc_world::Gen &G : w->gen) G.read_mask = 0; // nothing is in flight any more
    }
    const rtc_status us = ready_update(w);
    if (us != RTC_OK) return us;
    hipStream_t bs = w->build_stream;
    if (!w->updated) { // launches so far recorded nothing: one event per stream stands for all of them
        rtc_world::Gen &C = w->gen[w->cur];
        for (uint32_t l = 0; l < rtc_context::MAX_LANES; ++l)
            if (ctx->lane[l]) { HIP_TRY(hipEventRecord(C.read[l], ctx->lane[l])); C.read_mask |= 1u << l; }
        HIP_TRY(hipEventRecord(C.read[BIT_STREAM], ctx->stream));
        C.read_mask |= 1u << BIT_STREAM;
        w->updated = true;
    }
    const uint32_t g = (w->cur + 1u) % rtc_world::GENS;
    rtc_world::Gen &G = w->gen[g];
    if (G.device_built) HIP_TRY(hipEventSynchronize(G.built)); // its stage may still be the source of the copy of GENS updates ago
    for (uint32_t b = 0; b <= rtc_context::MAX_LANES; ++b)
        if (G.read_mask & (1u << b)) HIP_TRY(hipStreamWaitEvent(bs, G.read[b], 0));
    G.read_mask = 0;
    size_t staged = 0;
    carve_gen(G, n, &staged);
    unsigned char *const base = G.slab;
    auto staged_at = [&](auto *p) { return reinterpret_cast<decltype(p)>(G.stage + (reinterpret_cast<unsigned char *>(p) - base)); };
    flatten_shapes(shapes, n, staged_at(G.isect), staged_at(G.kind), staged_at(G.shade), staged_at(G.idtab), &G.any_refl, &G.any_refr);
    G.n = n;
    G.ngroups = (n + 63u) / 64u;
    set_lights(ctx, G, lights, n_lights);
    if (G.light_table) light_records(G, staged_at(G.ltab));
    else staged = static_cast<size_t>(reinterpret_cast<unsigned char *>(G.ltab) - base); // the table is the last staged block
    G.light_cap = 0;
    G.light_cap_want = light_cap;
    HIP_TRY(hipMemcpyAsync(base, G.stage, staged, hipMemcpyHostToDevice, bs));
    WorldBuildArgs a{};
    a.n = n;
    a.npad = rtc_world_build_npad(n);
    a.light_on = light_cap && w->light_cap_alloc && std::isfinite(light->position[0]) && std::isfinite(light->position[1]) &&
                 std::isfinite(light->position[2]);
    for (int i = 0; i < 3; ++i) a.light[i] = light->position[i];
    a.isect = G.isect; a.kind = G.kind; a.bound = G.bound; a.isect_s = G.isect_s; a.kind_s = G.kind_s; a.bound_s = G.bound_s;
    a.orig_s = G.orig_s; a.gbound = G.gbound; a.pre = G.pre; a.pre_s = G.pre_s; a.hdr = G.d_hdr; a.partial = G.partial;
    a.key = G.key; a.idx = G.idx;
    HIP_TRY(rtc_launch_world_build(&a, bs));
    if (a.light_on) {
        DevTileBundle *cell = w->d_light_cells.get();
        if (!w->light_cells_ready) { // no generation has had lists yet: nothing reads the cone tables
            HIP_TRY(rtc_launch_light_lists(0u, light_cap, G.bound, light->position, 0., cell, cell + LIGHT_CELLS, G.lights,
                                           G.lights + LIGHT_CELLS, bs));
            w->light_cells_ready = true;
        }
        HIP_TRY(rtc_launch_light_lists_built(n, light_cap, G.bound, light->position, G.d_hdr, cell, cell + LIGHT_CELLS, G.lights,
                                             G.lights + LIGHT_CELLS, bs));
    }
    HIP_TRY(hipMemcpyAsync(G.h_hdr, G.d_hdr, sizeof(DevWorldHeader), hipMemcpyDeviceToHost, bs));
    HIP_TRY(hipEventRecord(G.built, bs));
    G.hdr_pending = true;
    G.device_built = true;
    G.ordered = 0;
    w->cur = g;
    w->valid = true;
    return RTC_OK;
}

void rtc_world_destroy(rtc_world *w) {
    if (!w) return;
    if (w->device >= 0) { // the context may already be gone: synchronise the device, not its stream
        (void)hipSetDevice(w->device);
        (void)hipDeviceSynchronize();
    }
    for (rtc_world::BinSet &b : w->bin) {
        if (b.binned) (void)hipEventDestroy(b.binned);
        if (b.traced) (void)hipEventDestroy(b.traced);
    }
    for (rtc_world::Gen &G : w->gen) {
        if (G.built) (void)hipEventDestroy(G.built);
        for (hipEvent_t e : G.read)
            if (e) (void)hipEventDestroy(e);
    }
    if (w->build_stream) (void)hipStreamDestroy(w->build_stream);
    if (w->pinned) (void)hipHostFree(w->pinned);
    delete w; // its device buffers too, the device current and idle
}

// Readies binning set S for a launch: tile lists for the plan's `tiles` (view, tile) entries, grown to `tiles_alloc` when
// they are smaller, and primary-ray records for `prims` (object, view) pairs, grown to `prims_alloc`. A pipelined launch
// (`sync`) first waits for its lane, which may still read the set. False when there is no memory for the lists: they are an
// optimisation, and the launch walks instead (same pixels).
static bool ready_binset(rtc_context *ctx, rtc_world::BinSet &S, const LaunchPlan &plan, bool sync, hipStream_t stream) {
    if (S.tile_list.capacity() < plan.tiles * RTC_TILE_LIST_CAP) {
        if (sync) (void)hipStreamSynchronize(stream);
        S.tile_cnt.reset(); // both old lists go before either new one is allocated
        S.tile_list.reset();
        if (S.tile_cnt.reserve(plan.tiles_alloc + RTC_BIN_ROW_WORDS, &ctx->render_allocs) != RTC_OK ||
            S.tile_list.reserve(plan.tiles_alloc * RTC_TILE_LIST_CAP, &ctx->render_allocs) != RTC_OK) {
            S.tile_cnt.reset();
            return false;
        }
    }
    if (S.prim.capacity() < plan.prims) {
        if (sync) (void)hipStreamSynchronize(stream);
        if (S.prim.reserve(plan.prims_alloc, &ctx->render_allocs) != RTC_OK) return false;
    }
    return true;
}

// k_bin_tiles of the launch's views into set B on `stream` (timed by the event pair `ev`, if any), and the render
// parameters that read the set. `sort` (decided here): the packed lists' short ones sorted (RTC_TILE_SORT_CAP, rtc_device.h), for the
// render kernels' scalar walk: flat one-level worlds (the kernels that have it, trace_scalar_walk), unless RTC_BIN_SORT=0.
static hipError_t bin_tiles(const rtc_context *ctx, RenderParams &P, const rtc_world::Gen &G, const rtc_world::BinSet &B, const LaunchPlan &plan,
                            hipStream_t stream, const hipEvent_t *ev) {
    // the one place that decides it: the worlds whose render kernels have the scalar walk (trace_scalar_walk, rtc_kernels.hip)
    const bool sort = ctx->bin_sort && plan.src == SRC_CULL && !plan.refl;
    const bool sky_rows = ctx->sky_rows;
    uint32_t *cnt = B.tile_cnt.get() + RTC_BIN_ROW_WORDS;
    const hipError_t e = rtc_launch_binning(P.views, P.nviews, P.W, P.H, G.n, G.bound_s, G.gbound, G.orig_s,
                                            G.ngroups, cnt, B.tile_list.get(), P.y0 / 8u, P.band_stride, stream, ev ? ev[0] : nullptr,
                                            ev ? ev[1] : nullptr, G.isect_s, G.kind_s, G.n_unb, B.tile_cnt.get(),
                                            G.isect, B.prim.get(), sort ? 1u : 0u);
    if (e != hipSuccess) return e;
    P.prim = B.prim.get();
    P.tile_rows = sky_rows ? B.tile_cnt.get() : nullptr;
    P.tile_cnt = cnt;
    P.tile_list = B.tile_list.get();
    P.tiles_x = plan.tiles_x;
    P.tiles_y = plan.tiles_y;
    P.bin_packed = RTC_BIN_PACKED(G.n) ? (sort ? 2u : 1u) : 0u;
    P.n_unb = G.n_unb;
    return hipSuccess;
}

// One render launch, as its entry point asks for it. Rows [y0, y1) in tile rows of 8, tile row k at image rows
// y0 + 8*k*band_stride; grid_y tile rows; `nviews` cameras of one size, view v `view_rows` rows further down the outputs.
struct LaunchRequest {
    const rtc_camera *cams = nullptr;
    uint32_t nviews = 1, view_rows = 0;
    uint32_t mode = 0, y0 = 0, y1 = 0, band_stride = 1, grid_y = 0;
    void *d_rgb = nullptr, *d_rgb8 = nullptr;
    uint32_t flags = 0;
    float gamma = 0.f;            // > 0: d_rgb8 receives Canvas::to_imgbuf's RGBA at that gamma (4 B/pixel) instead of Color::scale's RGB
    const rtc_lens *lens = nullptr; // a thin-lens launch (validated by the caller, one view, no gamma)
    const rtc_projection *proj = nullptr; // an orthographic or panorama launch (likewise; never with a lens)
};
// rows [y0, y1) of one camera
static LaunchRequest rows_request(const rtc_camera *cam, uint32_t mode, uint32_t y0, uint32_t y1, void *d_rgb, void *d_rgb8, uint32_t flags) {
    LaunchRequest rq;
    rq.cams = cam; rq.mode = mode; rq.y0 = y0; rq.y1 = y1; rq.grid_y = (y1 - y0 + 7u) / 8u;
    rq.d_rgb = d_rgb; rq.d_rgb8 = d_rgb8; rq.flags = flags;
    return rq;
}
// every band_stride-th band of 8 rows from first_band on: the caller's share of the canvas, packed (rtc_bands.h). False:
// it owns no band of so small a canvas.
static bool bands_request(const rtc_camera *cam, uint32_t mode, uint32_t first_band, uint32_t band_stride, void *d_rgb, void *d_rgb8,
                          uint32_t flags, LaunchRequest &rq) {
    const uint32_t nbands = (cam->vsize + RTC_BAND_ROWS - 1u) / RTC_BAND_ROWS;
    if (first_band >= nbands) return false;
    rq = rows_request(cam, mode, first_band * RTC_BAND_ROWS, cam->vsize, d_rgb, d_rgb8, flags);
    rq.band_stride = band_stride;
    rq.grid_y = (nbands - first_band + band_stride - 1u) / band_stride;
    return true;
}

// rtc_plan_launch for a launch of kind `kind` of generation G on this context: the knobs and the World's facts; the
// caller adds what it asks for.
static LaunchPlanInputs plan_inputs(const rtc_context *ctx, const rtc_world::Gen &G, uint32_t kind, uint32_t flags) {
    LaunchPlanInputs in{};
    in.force_src = ctx->force_src;
    in.tile_cap = ctx->tile_cap;
    in.tiles_per_wg = ctx->tiles_per_wg;
    in.tiles_guided_tenths = ctx->tiles_guided_tenths;
    in.tiles_slots = ctx->tiles_slots;
    in.tiles_kmax = ctx->tiles_kmax;
    in.binning = ctx->binning;
    in.pipelined = ctx->lanes > 1;
    in.bin_small_pixels = ctx->bin_small_pixels;
    in.bin_small_pixels_pipelined = ctx->bin_small_pixels_pipelined;
    in.n = G.n;
    in.n_lights = G.n_lights;
    in.any_refl = G.any_refl;
    in.any_refr = G.any_refr;
    in.kind = kind;
    in.flags = flags;
    return in;
}

// Where every render launch starts: the device current, the World's current generation, the plan of `rq` on it.
static rtc_status plan_request(const rtc_context *ctx, const rtc_world *w, const LaunchRequest &rq, rtc_world::Gen **gen, LaunchPlan &plan) {
    HIP_TRY(hipSetDevice(ctx->device));
    const rtc_status hs = current_gen(w, gen);
    if (hs != RTC_OK) return hs;
    LaunchPlanInputs in = plan_inputs(ctx, **gen, RTC_PLAN_FRAME, rq.flags);
    in.hsize = rq.cams->hsize; in.vsize = rq.cams->vsize; in.samples = rq.cams->samples; in.nviews = rq.nviews;
    in.y0 = rq.y0; in.y1 = rq.y1; in.band_stride = rq.band_stride; in.grid_y = rq.grid_y;
    in.mode = rq.mode;
    in.lens_samples = rq.lens ? rq.lens->usteps * rq.lens->vsteps : rq.proj ? 1u : 0u; // a projection launch is planned as a lens launch of one sample
    rtc_plan_launch(in, plan);
    return RTC_OK;
}

// The parameter block of a planned launch on generation G: the World's tables and what the plan fixes. The caller adds its
// cameras or rays and its outputs.
static void planned_params(const rtc_context *ctx, const rtc_world *w, const rtc_world::Gen &G, const LaunchPlan &plan, RenderParams &P) {
    std::memset(&P, 0, sizeof P);
    fill_world(P, G);
    P.prim = w->d_prim.get();
    if (!ctx->light_lists) P.light_cnt = nullptr;
    P.tile_cap = plan.tile_cap;
    P.flags = plan.flags;
    P.aa_lds_off = plan.aa_lds_off;
    P.resample_n = plan.resample_n;
    P.grid_x = plan.grid_x;
    P.total_blocks = plan.total_blocks;
    P.reps = plan.reps;
    std::memcpy(P.chunk_wgs, plan.chunk_wgs, sizeof P.chunk_wgs);
}
static hipError_t trace_planned(const rtc_context *ctx, const RenderParams &P, const LaunchPlan &plan, const LaunchLights &LL, hipStream_t stream,
                                hipEvent_t e0, hipEvent_t e1, const DevLens *lens, const DevProjection *proj) {
    return rtc_launch_trace(&P, plan.src, (int)plan.refl, (int)plan.refr, plan.grid_wgs, plan.lds_bytes, stream, e0, e1, LL.xl, LL.lt, lens,
                            proj, ctx->one_sample ? 1 : 0, ctx->whole_tiles ? 1 : 0, ctx->uniform_shade ? 1 : 0);
}

// The panorama tables of (cam, proj) in the context's two buffers (include/rtc.h: rtc_projection_tables, keyed by size and
// spans). A launch in flight may still read the tables of another key, so a change of key first waits for every stream of
// the context — the lanes and the in-order stream — and then uploads synchronously; the same key again does nothing.
static rtc_status pano_tables(rtc_context *ctx, const rtc_camera *cam, const rtc_projection *proj) {
    rtc_context::PanoKey key{cam->hsize, cam->vsize, proj->h_span, proj->v_span};
    if (ctx->pano_valid && std::memcmp(&key, &ctx->pano_key, sizeof key) == 0) return RTC_OK;
    std::vector<double> col(2u * (size_t)cam->hsize), row(2u * (size_t)cam->vsize);
    if (rtc_projection_tables(cam, proj, col.data(), row.data()) != RTC_OK) return RTC_ERR_ARG;
    HIP_TRY(drain_lanes(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->pano_valid = false;
    rtc_status st = ctx->d_pano_col.reserve(col.size(), &ctx->render_allocs);
    if (st == RTC_OK) st = ctx->d_pano_row.reserve(row.size(), &ctx->render_allocs);
    if (st == RTC_OK) st = ctx->d_pano_col.upload(col.data(), col.size());
    if (st == RTC_OK) st = ctx->d_pano_row.upload(row.data(), row.size());
    if (st != RTC_OK) return st;
    ctx->pano_key = key;
    ctx->pano_valid = true;
    ++ctx->pano_uploads;
    return RTC_OK;
}

// Carries `plan` (of `rq`, on generation G) out: pick the stream and order it behind the World's build; bin, or prepare the
// brute-force table; trace; keep the books. What only the device knows at run time is decided here and nowhere else: the
// walk when there is no memory for the tile lists, the lane, the timing ring, the gamma table.
static rtc_status launch_planned(rtc_context *ctx, const rtc_world *w, rtc_world::Gen &G, const LaunchRequest &rq, const LaunchPlan &plan) {
    if (plan.status != RTC_OK) return (rtc_status)plan.status;
    RenderParams P;
    planned_params(ctx, w, G, plan, P);
    for (uint32_t v = 0; v < rq.nviews; ++v) fill_camera(P, rq.cams + v, v);
    P.nviews = rq.nviews;
    P.view_rows = rq.view_rows;
    P.y0 = rq.y0;
    P.y1 = rq.y1;
    P.mode = rq.mode;
    P.grid_y = rq.grid_y;
    P.band_stride = rq.band_stride;
    P.out = static_cast<double *>(rq.d_rgb);
    P.out8 = static_cast<unsigned char *>(rq.d_rgb8);
    P.counters = ctx->d_counters.get();
    P.remaining = RTC_MAX_REFLECTIONS; // render_pixel passes Camera::MAX_REFLECTIONS camera.rs:98
    LaunchLights LL;
    lights_of(G, LL);
    DevLens dlens;
    if (const rtc_lens *lens = rq.lens) {
        dlens.aperture = lens->aperture;
        dlens.focal_distance = lens->focal_distance;
        dlens.ucell = (2.0 * lens->aperture) / static_cast<double>(lens->usteps); // include/rtc.h's order (no contraction in this file)
        dlens.vcell = (2.0 * lens->aperture) / static_cast<double>(lens->vsteps);
        dlens.usteps = lens->usteps;
        dlens.vsteps = lens->vsteps;
    }
    DevProjection dproj{};
    if (const rtc_projection *proj = rq.proj) {
        dproj.kind = proj->kind;
        if (proj->kind == RTC_PROJ_ORTHOGRAPHIC) {
            double t[3];
            rtc_projection_ortho_terms(rq.cams->hsize, rq.cams->vsize, proj->width, t);
            dproj.half_w = t[0]; dproj.half_h = t[1]; dproj.pixel = t[2];
        } else {
            const rtc_status ts = pano_tables(ctx, rq.cams, proj);
            if (ts != RTC_OK) return ts;
            dproj.col = ctx->d_pano_col.get();
            dproj.row = ctx->d_pano_row.get();
        }
    }
    // start/stop events cost ~9 us of host time and ~5 us of GPU time per launch (measured): callers
    // that are launch-bound sample every n-th launch instead (rtc_context_set_timing)
    const bool timed = ctx->time_every != 0 && ctx->launches % ctx->time_every == 0;
    const uint32_t slot = (uint32_t)(ctx->timed % rtc_context::EV_RING);
    if (timed && slot >= ctx->ev_created) // next chunk of the ring
        HIP_TRY(create_events(ctx, std::min<uint32_t>(rtc_context::EV_RING, ctx->ev_created + rtc_context::EV_CHUNK)));
    hipEvent_t *pair = ctx->ev[slot], *pair_bin = ctx->ev_bin[slot];
    // Which stream. A pipelined context deals the launches round-robin over its lanes; those the plan keeps in order stay on lane 0.
    const bool piped = ctx->lanes > 1;
    const uint32_t lane = piped && plan.lane_dealt ? (uint32_t)(ctx->lane_next++ % ctx->lanes) : 0u;
    hipStream_t stream = piped ? ctx->lane[lane] : ctx->stream;
    const uint32_t stream_bit = piped ? lane : BIT_STREAM;
    HIP_TRY(order_behind_build(G, stream, stream_bit));
    if (rq.gamma > 0.f) { // the table goes to the device on this launch's own stream (or is waited for there once)
        const rtc_status gs = gamma_table(ctx, rq.gamma, stream, piped ? lane : rtc_context::MAX_LANES, &P.gamma);
        if (gs != RTC_OK) return gs;
    }
    rtc_world::BinSet *binset = nullptr;
    int bin_set = -1; // which of w->bin this launch's lists are in (rtc_debug_tile_counts)
    bool bin_ok = plan.bin != 0u;
    if (bin_ok && piped) {
        // lane-local lists: the binning kernel precedes the render kernel on the lane's own stream and runs beside the other
        // lanes' render kernels — no events. Grow-only; growing waits for the lane.
        rtc_world::BinSet &B = w->bin[lane];
        bin_ok = ready_binset(ctx, B, plan, true, stream);
        if (bin_ok) HIP_TRY(bin_tiles(ctx, P, G, B, plan, stream, timed ? pair_bin : nullptr));
        if (bin_ok) bin_set = (int)lane;
    } else if (bin_ok) {
        if (!ctx->side_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
        // Both sets are made ready by the FIRST binned launch (the plan's tiles_alloc / prims_alloc: a launch sequence must
        // not allocate after its first launch). When there is no memory for them the launch walks instead.
        for (uint32_t k = 0; k < 2u && bin_ok; ++k) {
            rtc_world::BinSet &S = w->bin[k];
            if (!S.binned) {
                HIP_TRY(hipEventCreateWithFlags(&S.binned, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&S.traced, hipEventDisableTiming));
            }
            bin_ok = ready_binset(ctx, S, plan, false, stream);
        }
    }
    if (bin_ok && !piped) {
        bin_set = (int)(w->bin_next & 1u);
        rtc_world::BinSet &B = w->bin[w->bin_next++ & 1u];
        // The binning depends on the World (resident since rtc_world_create) and on this launch's cameras only, so it goes
        // to the side stream: it runs beside the PREVIOUS launch's render kernel, which still reads the other set. It must
        // wait for the render kernel that last read THIS set (two launches ago); the render stream waits for the binning.
        HIP_TRY(hipStreamWaitEvent(ctx->side_stream, B.traced, 0)); // never recorded: no wait
        HIP_TRY(order_behind_build(G, ctx->side_stream, BIT_SIDE));
        HIP_TRY(bin_tiles(ctx, P, G, B, plan, ctx->side_stream, timed ? pair_bin : nullptr));
        HIP_TRY(hipEventRecord(B.binned, ctx->side_stream));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, B.binned, 0));
        binset = &B;
    }
    if (timed) ctx->bin_timed[slot] = P.tile_cnt != nullptr;
    // per-render prologue table of the brute-force variants (the culled and the lens kernels do not use it)
    if (plan.needs_prep) HIP_TRY(rtc_launch_prep(G.isect, w->d_prim.get(), G.n, P.views[0].vinv, stream));
    HIP_TRY(trace_planned(ctx, P, plan, LL, stream, timed ? pair[0] : nullptr, timed ? pair[1] : nullptr, rq.lens ? &dlens : nullptr,
                          rq.proj ? &dproj : nullptr));
    if (binset) HIP_TRY(hipEventRecord(binset->traced, ctx->stream));
    HIP_TRY(record_read(w, G, stream, stream_bit));
    ctx->last = rtc_launch_info{(uint32_t)plan.src, plan.refl, plan.refr, P.tile_cnt ? 1u : 0u, P.light_cnt ? 1u : 0u, lane, plan.block,
                                plan.lds_bytes, plan.reps, plan.chunk_wgs[0] + plan.chunk_wgs[1] + plan.chunk_wgs[2] + plan.chunk_wgs[3],
                                LL.lt ? 1u : 0u, rq.lens ? rq.lens->usteps * rq.lens->vsteps : 0u};
    ctx->last_projection = rq.proj ? rq.proj->kind : 0u;
    ++ctx->launches_total;
    ctx->last_bin = rtc_context::LastBin{};
    if (P.tile_cnt && bin_set >= 0) ctx->last_bin = rtc_context::LastBin{w->serial, (uint32_t)bin_set, rq.nviews, plan.tiles_x, plan.tiles_y};
    ctx->pixels += plan.counted_pixels;
    ++ctx->launches;
    if (timed) ++ctx->timed;
    return RTC_OK;
}

static rtc_status render_launch(rtc_context *ctx, const rtc_world *w, const LaunchRequest &rq) {
    rtc_world::Gen *gen = nullptr;
    LaunchPlan plan;
    const rtc_status st = plan_request(ctx, w, rq, &gen, plan);
    return st != RTC_OK ? st : launch_planned(ctx, w, *gen, rq, plan);
}

// What every render entry checks first: a context with its own World, a camera with a canvas, somewhere to write, a known mode
static rtc_status check_render_args(const rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, const void *d_rgb,
                                    const void *d_rgb8) {
    if (!ctx || !w || !cam || (!d_rgb && !d_rgb8) || w->ctx != ctx) return RTC_ERR_ARG;
    if (mode > RTC_MODE_RENDER_ASYNC || cam->hsize == 0 || cam->vsize == 0) return RTC_ERR_ARG;
    return RTC_OK;
}

rtc_status rtc_render_rows(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t y0,
                           uint32_t y1, void *d_rgb, void *d_rgb8, uint32_t flags) {
    if (check_render_args(ctx, w, cam, mode, d_rgb, d_rgb8) != RTC_OK || y0 > y1 || y1 > cam->vsize) return RTC_ERR_ARG;
    if (cam->samples > 255u) return RTC_ERR_ARG; // antialiasing_samples is a u8 (camera.rs:24)
    if (y0 == y1) return RTC_OK;
    return render_launch(ctx, w, rows_request(cam, mode, y0, y1, d_rgb, d_rgb8, flags));
}

// The checks every lens entry shares (include/rtc.h): a valid lens, one ray per lens sample
static rtc_status check_lens(const rtc_camera *cam, const rtc_lens *lens) {
    if (!cam || rtc_lens_validate(lens) != RTC_OK) return RTC_ERR_ARG;
    if (cam->samples != 1u) return RTC_ERR_ARG; // anti-aliasing and the lens do not compose
    return RTC_OK;
}

rtc_status rtc_render_lens_rows(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_lens *lens, uint32_t mode,
                                uint32_t y0, uint32_t y1, void *d_rgb, void *d_rgb8, uint32_t flags) {
    if (check_render_args(ctx, w, cam, mode, d_rgb, d_rgb8) != RTC_OK || y0 > y1 || y1 > cam->vsize) return RTC_ERR_ARG;
    const rtc_status ls = check_lens(cam, lens);
    if (ls != RTC_OK) return ls;
    if (y0 == y1) return RTC_OK;
    LaunchRequest rq = rows_request(cam, mode, y0, y1, d_rgb, d_rgb8, flags);
    rq.lens = lens;
    return render_launch(ctx, w, rq);
}

// The checks every projection entry shares (include/rtc.h): a valid projection, one ray per pixel
static rtc_status check_projection(const rtc_camera *cam, const rtc_projection *proj) {
    if (!cam || rtc_projection_validate(proj) != RTC_OK) return RTC_ERR_ARG;
    if (cam->samples != 1u) return RTC_ERR_ARG; // anti-aliasing and the projections do not compose
    return RTC_OK;
}

rtc_status rtc_render_projection_rows(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode,
                                      uint32_t y0, uint32_t y1, void *d_rgb, void *d_rgb8, uint32_t flags) {
    if (check_render_args(ctx, w, cam, mode, d_rgb, d_rgb8) != RTC_OK || y0 > y1 || y1 > cam->vsize) return RTC_ERR_ARG;
    const rtc_status ps = check_projection(cam, proj);
    if (ps != RTC_OK) return ps;
    if (y0 == y1) return RTC_OK;
    LaunchRequest rq = rows_request(cam, mode, y0, y1, d_rgb, d_rgb8, flags);
    rq.proj = proj;
    return render_launch(ctx, w, rq);
}

rtc_status rtc_render_bands(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode,
                            uint32_t first_band, uint32_t band_stride, void *d_rgb, void *d_rgb8, uint32_t flags) {
    if (check_render_args(ctx, w, cam, mode, d_rgb, d_rgb8) != RTC_OK || band_stride == 0) return RTC_ERR_ARG;
    if (cam->samples > 255u) return RTC_ERR_ARG;
    LaunchRequest rq;
    if (!bands_request(cam, mode, first_band, band_stride, d_rgb, d_rgb8, flags, rq)) return RTC_OK;
    return render_launch(ctx, w, rq);
}

rtc_status rtc_stats_read(rtc_context *ctx, rtc_stats *out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<unsigned long long> slots((size_t)CNT_N * CNT_SLOTS);
    HIP_TRY(drain_lanes(ctx));
    HIP_TRY(hipMemcpyAsync(slots.data(), ctx->d_counters.get(), sizeof(unsigned long long) * slots.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long h[CNT_N] = {0};
    for (int sl = 0; sl < CNT_SLOTS; ++sl)
        for (int k = 0; k < CNT_N; ++k) h[k] += slots[(size_t)sl * CNT_N + k];
    std::memset(out, 0, sizeof *out);
    out->rays_primary = h[CNT_PRIMARY];
    out->rays_shadow = h[CNT_SHADOW];
    out->rays_reflect = h[CNT_REFLECT];
    out->rays_refract = h[CNT_REFRACT];
    out->pixels = ctx->pixels; // counted at launch time (render_launch)
    out->pixels_resample = h[CNT_RESAMPLE];
    out->rays_primary_proven_miss = h[CNT_SKY];
    return RTC_OK;
}

// Diagnostic (not part of include/rtc.h): device allocations made by the render entry points of this context so far — the
// binning sets and rtc_render's scratch canvas. A frame sequence must stop allocating after its first launch
// (tests/test_gpu_group.py::test_render_paths_stop_allocating_after_the_first_launch).
// Test hook (not in include/rtc.h): how often this context has uploaded panorama tables (pano_tables)
extern "C" rtc_status rtc_debug_projection_uploads(rtc_context *ctx, unsigned long long *out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    *out = ctx->pano_uploads;
    return RTC_OK;
}

extern "C" rtc_status rtc_debug_render_allocs(rtc_context *ctx, unsigned long long *out) {
    if (!ctx || !out) return RTC_ERR_ARG;
    *out = ctx->render_allocs;
    return RTC_OK;
}

// Diagnostic (not part of include/rtc.h): what rtc_world_create derived for the candidate lists of `w`. info = {n_unb,
// ngroups, light_cap (0: no light lists), n}; *light_reach; cell_counts (optional): the 6 * RTC_LIGHT_R * RTC_LIGHT_R
// per-cell counters of the light lists (a counter above light_cap: that cell's list overflowed), untouched when the World
// has no lists; bounds (optional): the n DevBound records {cx, cy, cz, r, k, cn} in insertion order. Copies only.
extern "C" rtc_status rtc_debug_world_lists(const rtc_world *w, uint32_t info[4], double *light_reach, uint32_t *cell_counts, double *bounds) {
    if (!w || !info || !light_reach) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(hipDeviceSynchronize());
    rtc_world::Gen *gen = nullptr;
    const rtc_status hs = current_gen(w, &gen);
    if (hs != RTC_OK) return hs;
    rtc_world::Gen &G = *gen;
    info[0] = G.n_unb; info[1] = G.ngroups; info[2] = G.light_cap; info[3] = G.n;
    *light_reach = G.light_reach;
    static_assert(sizeof(DevBound) == 6 * sizeof(double), "bounds are read back as six doubles per object");
    if (cell_counts && G.light_cap)
        HIP_TRY(hipMemcpy(cell_counts, G.lights, sizeof(uint32_t) * 6u * RTC_LIGHT_R * RTC_LIGHT_R, hipMemcpyDeviceToHost));
    if (bounds && G.n) HIP_TRY(hipMemcpy(bounds, G.bound, sizeof(DevBound) * G.n, hipMemcpyDeviceToHost));
    return RTC_OK;
}

// Diagnostic (not part of include/rtc.h): the tables and scalars of the World's current contents, however they were built.
// info = {n, n_unb, ngroups, light_cap (0: no light lists), any_refl, any_refr}; scalars = {pre_limit, light_reach}; *allocs:
// device allocations made for the World since it was created. Every table pointer is optional and receives max(n, 1) records
// (gbound: max(ngroups, 1); light_cnt: 6 * RTC_LIGHT_R^2 counters and light_list light_cap entries per cell, both only when
// light_cap != 0). Waits for the device first. Copies only.
extern "C" rtc_status rtc_debug_world_tables(const rtc_world *w, uint32_t info[6], double scalars[2], unsigned long long *allocs, void *bound,
                                             void *bound_s, uint32_t *orig_s, uint32_t *kind_s, void *isect_s, void *gbound, void *pre,
                                             void *pre_s, void *idtab, uint32_t *light_cnt, uint32_t *light_list) {
    if (!w || !info || !scalars || !allocs) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(hipDeviceSynchronize());
    rtc_world::Gen *gen = nullptr;
    const rtc_status hs = current_gen(w, &gen);
    if (hs != RTC_OK) return hs;
    rtc_world::Gen &G = *gen;
    info[0] = G.n; info[1] = G.n_unb; info[2] = G.ngroups; info[3] = G.light_cap; info[4] = G.any_refl; info[5] = G.any_refr;
    scalars[0] = G.pre_limit; scalars[1] = G.light_reach;
    *allocs = w->allocs;
    const size_t na = G.n ? G.n : 1u, ng = G.ngroups ? G.ngroups : 1u;
    auto copy = [](void *dst, const void *src, size_t bytes) { return !dst || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
    bool ok = copy(bound, G.bound, sizeof(DevBound) * na) && copy(bound_s, G.bound_s, sizeof(DevBound) * na) &&
              copy(orig_s, G.orig_s, sizeof(uint32_t) * na) && copy(kind_s, G.kind_s, sizeof(uint32_t) * na) &&
              copy(isect_s, G.isect_s, sizeof(DevIsect) * na) && copy(gbound, G.gbound, sizeof(DevBound) * ng) &&
              copy(pre, G.pre, sizeof(DevPre) * na) && copy(pre_s, G.pre_s, sizeof(DevPre) * na) && copy(idtab, G.idtab, sizeof(DevIdEntry) * na);
    if (G.light_cap)
        ok = ok && copy(light_cnt, G.lights, sizeof(uint32_t) * LIGHT_CELLS) &&
             copy(light_list, G.lights + LIGHT_CELLS, sizeof(uint32_t) * LIGHT_CELLS * G.light_cap);
    return ok ? RTC_OK : RTC_ERR_DEVICE;
}

// Diagnostic (not part of include/rtc.h): the tile lists of the context's most recent render launch, which must have been a
// launch of `w`. dims = {binned, nviews, tiles_x, tiles_y}; binned == 0 ("none": that launch read no tile lists) leaves the
// rest untouched. counts (optional, `counts_cap` words, at least nviews * tiles_y * tiles_x): per (view, tile) the list
// count k_bin_tiles wrote, tile (tx, ty) of view v at (v * tiles_y + ty) * tiles_x + tx (above RTC_TILE_LIST_CAP: the list
// overflowed; tile rows the launch did not render hold stale words). rows (optional, `rows_cap` words, at least 2 * nviews):
// per view the two row words. Waits for the context's work first. Copies only.
extern "C" rtc_status rtc_debug_tile_counts(rtc_context *ctx, const rtc_world *w, uint32_t dims[4], uint32_t *counts, size_t counts_cap,
                                            uint32_t *rows, size_t rows_cap) {
    if (!ctx || !w || !dims || w->ctx != ctx) return RTC_ERR_ARG;
    dims[0] = dims[1] = dims[2] = dims[3] = 0u;
    const rtc_context::LastBin &L = ctx->last_bin;
    if (L.world_serial == 0 || L.world_serial != w->serial) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(drain_lanes(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    const rtc_world::BinSet &B = w->bin[L.set];
    const size_t tiles = (size_t)L.nviews * L.tiles_x * L.tiles_y;
    if (!B.tile_cnt.get() || B.tile_cnt.capacity() < RTC_BIN_ROW_WORDS + tiles) return RTC_ERR_ARG;
    if ((counts && counts_cap < tiles) || (rows && rows_cap < 2u * (size_t)L.nviews)) return RTC_ERR_ARG;
    dims[0] = 1u; dims[1] = L.nviews; dims[2] = L.tiles_x; dims[3] = L.tiles_y;
    if (counts) HIP_TRY(hipMemcpy(counts, B.tile_cnt.get() + RTC_BIN_ROW_WORDS, sizeof(uint32_t) * tiles, hipMemcpyDeviceToHost));
    if (rows) HIP_TRY(hipMemcpy(rows, B.tile_cnt.get(), sizeof(uint32_t) * 2u * L.nviews, hipMemcpyDeviceToHost));
    return RTC_OK;
}

// Diagnostic (not part of include/rtc.h), rtc_debug_tile_counts' companion: the lists themselves, of the same launch and under
// the same guards. dims as there. lists (`lists_cap` words, at least nviews * tiles_y * tiles_x * 64): 64 entry slots per
// (view, tile) in the counts' order, of which the first min(count, 64) hold the list — packed entries (key's upper half above
// the object index; ascending in lists of at most RTC_TILE_SORT_CAP entries of a flat one-level world unless RTC_BIN_SORT=0) in
// Worlds of at most 65 536 objects, plain indices above that; the other slots hold stale words. Waits for the context's work first. Copies only.
extern "C" rtc_status rtc_debug_tile_lists(rtc_context *ctx, const rtc_world *w, uint32_t dims[4], uint32_t *lists, size_t lists_cap) {
    if (!ctx || !w || !dims || !lists || w->ctx != ctx) return RTC_ERR_ARG;
    dims[0] = dims[1] = dims[2] = dims[3] = 0u;
    const rtc_context::LastBin &L = ctx->last_bin;
    if (L.world_serial == 0 || L.world_serial != w->serial) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(drain_lanes(ctx));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->side_stream) HIP_TRY(hipStreamSynchronize(ctx->side_stream));
    const rtc_world::BinSet &B = w->bin[L.set];
    const size_t words = (size_t)L.nviews * L.tiles_x * L.tiles_y * RTC_TILE_LIST_CAP;
    if (!B.tile_list.get() || B.tile_list.capacity() < words || lists_cap < words) return RTC_ERR_ARG;
    dims[0] = 1u; dims[1] = L.nviews; dims[2] = L.tiles_x; dims[3] = L.tiles_y;
    HIP_TRY(hipMemcpy(lists, B.tile_list.get(), sizeof(uint32_t) * words, hipMemcpyDeviceToHost));
    return RTC_OK;
}

rtc_status rtc_stats_reset(rtc_context *ctx) {
    if (!ctx) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(drain_lanes(ctx));
    HIP_TRY(hipMemsetAsync(ctx->d_counters.get(), 0, sizeof(unsigned long long) * CNT_N * CNT_SLOTS, ctx->stream));
    if (ctx->lanes > 1) HIP_TRY(hipStreamSynchronize(ctx->stream)); // the lanes are not ordered behind the stream
    ctx->pixels = 0;
    return RTC_OK;
}

rtc_status rtc_context_set_timing(rtc_context *ctx, uint32_t every) {
    if (!ctx) return RTC_ERR_ARG;
    if (every != 0) { // a caller that asks for timings gets the first 64 event pairs now, not 16 at a time in the middle of its timed loop
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(create_events(ctx, std::min<uint32_t>(rtc_context::EV_RING, 64u)));
    }
    ctx->time_every = every;
    ctx->launches = 0; // the next launch is sampled (if any is), and the ring starts afresh
    ctx->timed = 0;
    return RTC_OK;
}

// Waits until the newest `take` timed launches have ended. In order on one stream the newest launch's end follows every
// earlier one; a pipelined context's launches run on several lanes, so each pair's end is waited for (rtc_context_set_pipeline
// drains the lanes, so pairs recorded before a switch back to depth 1 are complete already).
static hipError_t wait_timed(rtc_context *ctx, uint64_t take) {
    if (ctx->lanes <= 1) return hipEventSynchronize(ctx->ev[(ctx->timed - 1) % rtc_context::EV_RING][1]);
    for (uint64_t k = 0; k < take; ++k) {
        const hipError_t e = hipEventSynchronize(ctx->ev[(ctx->timed - take + k) % rtc_context::EV_RING][1]);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

rtc_status rtc_kernel_times_ms(rtc_context *ctx, float *out, uint32_t cap, uint32_t *n) {
    if (!ctx || !n || (cap && !out)) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t have = ctx->timed < rtc_context::EV_RING ? ctx->timed : rtc_context::EV_RING;
    const uint64_t take = have < cap ? have : cap;
    *n = (uint32_t)take;
    if (take == 0) return RTC_OK;
    HIP_TRY(wait_timed(ctx, take));
    for (uint64_t k = 0; k < take; ++k) {
        hipEvent_t *pair = ctx->ev[(ctx->timed - take + k) % rtc_context::EV_RING];
        HIP_TRY(hipEventElapsedTime(&out[k], pair[0], pair[1]));
    }
    return RTC_OK;
}

rtc_status rtc_binning_times_ms(rtc_context *ctx, float *out, uint32_t cap, uint32_t *n) {
    if (!ctx || !n || (cap && !out)) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint64_t have = ctx->timed < rtc_context::EV_RING ? ctx->timed : rtc_context::EV_RING;
    const uint64_t take = have < cap ? have : cap;
    *n = (uint32_t)take;
    if (take == 0) return RTC_OK;
    HIP_TRY(wait_timed(ctx, take)); // each render kernel follows its own binning
    for (uint64_t k = 0; k < take; ++k) {
        const uint64_t sl = (ctx->timed - take + k) % rtc_context::EV_RING;
        out[k] = 0.f;
        if (ctx->bin_timed[sl]) HIP_TRY(hipEventElapsedTime(&out[k], ctx->ev_bin[sl][0], ctx->ev_bin[sl][1]));
    }
    return RTC_OK;
}

rtc_status rtc_last_kernel_ms(rtc_context *ctx, float *ms) {
    uint32_t n = 0;
    if (!ctx || !ms) return RTC_ERR_ARG;
    const rtc_status st = rtc_kernel_times_ms(ctx, ms, 1, &n);
    if (st != RTC_OK) return st;
    return n == 1 ? RTC_OK : RTC_ERR_ARG;
}

static_assert(RTC_MAX_VIEWS == RTC_MAX_VIEWS_PER_LAUNCH, "include/rtc.h and rtc_device.h disagree");

// rtc_render_views and rtc_render_views_rgba8 (gamma > 0: d_rgb8 holds RGBA, 4 B/pixel)
static rtc_status render_views(rtc_context *ctx, const rtc_world *w, const rtc_camera *cams, uint32_t nviews, uint32_t mode,
                               uint32_t first_band, uint32_t band_stride, void *d_rgb, void *d_rgb8, uint32_t view_rows,
                               uint32_t flags, float gamma) {
    if (nviews == 0 || nviews > RTC_MAX_VIEWS_PER_LAUNCH || band_stride == 0) return RTC_ERR_ARG;
    if (check_render_args(ctx, w, cams, mode, d_rgb, d_rgb8) != RTC_OK) return RTC_ERR_ARG;
    for (uint32_t v = 1; v < nviews; ++v)
        if (cams[v].hsize != cams[0].hsize || cams[v].vsize != cams[0].vsize || cams[v].samples != cams[0].samples)
            return RTC_ERR_ARG; // one grid, one sampling pattern per launch
    if (cams[0].samples > 255u) return RTC_ERR_ARG;
    LaunchRequest rq;
    if (!bands_request(cams, mode, first_band, band_stride, d_rgb, d_rgb8, flags, rq)) return RTC_OK;
    if (view_rows < rq.grid_y * RTC_BAND_ROWS) return RTC_ERR_ARG;
    rq.nviews = nviews;
    rq.view_rows = view_rows;
    rq.gamma = gamma;
    rtc_world::Gen *gen = nullptr;
    LaunchPlan plan;
    rtc_status st = plan_request(ctx, w, rq, &gen, plan);
    if (st != RTC_OK) return st;
    if (!plan.needs_prep) return launch_planned(ctx, w, *gen, rq, plan);
    // the brute-force variants keep a per-render table of the camera origin in object space: one view per launch
    rq.nviews = 1u;
    rq.view_rows = 0u;
    for (uint32_t v = 0; v < nviews && st == RTC_OK; ++v) {
        rq.cams = cams + v;
        rq.d_rgb = d_rgb ? static_cast<double *>(d_rgb) + (size_t)v * view_rows * cams[0].hsize * 3u : nullptr;
        rq.d_rgb8 = d_rgb8 ? static_cast<unsigned char *>(d_rgb8) + (size_t)v * view_rows * cams[0].hsize * (gamma > 0.f ? 4u : 3u) : nullptr;
        st = render_launch(ctx, w, rq);
    }
    return st;
}

rtc_status rtc_render_views(rtc_context *ctx, const rtc_world *w, const rtc_camera *cams, uint32_t nviews, uint32_t mode,
                            uint32_t first_band, uint32_t band_stride, void *d_rgb, void *d_rgb8, uint32_t view_rows,
                            uint32_t flags) {
    return render_views(ctx, w, cams, nviews, mode, first_band, band_stride, d_rgb, d_rgb8, view_rows, flags, 0.f);
}

rtc_status rtc_render_views_rgba8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cams, uint32_t nviews, uint32_t mode,
                                  uint32_t first_band, uint32_t band_stride, float gamma, void *d_rgba8, uint32_t view_rows,
                                  uint32_t flags) {
    if (!d_rgba8 || !gamma_ok(gamma)) return RTC_ERR_ARG;
    return render_views(ctx, w, cams, nviews, mode, first_band, band_stride, nullptr, d_rgba8, view_rows, flags, gamma);
}

// rtc_render, rtc_render_rgb8 and rtc_render_rgba8: the whole frame into the context's grow-only canvas (no hipMalloc /
// hipFree, a device sync, per frame), then to `host`. f64: RGB doubles; else 8-bit rows, RGBA at `gamma` when gamma > 0
// and Color::scale's RGB otherwise (only those rows leave the kernel: no f64 canvas is written).
static rtc_status render_frame(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags, bool f64,
                               float gamma, void *host, rtc_stats *stats, const rtc_lens *lens = nullptr, const rtc_projection *proj = nullptr) {
    if (check_render_args(ctx, w, cam, mode, host, nullptr) != RTC_OK || cam->samples > 255u) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)cam->hsize * cam->vsize, bytes = px * (f64 ? 3 * sizeof(double) : gamma > 0.f ? 4u : 3u);
    rtc_status st = f64 ? ctx->d_canvas.reserve(3 * px, &ctx->render_allocs) : ctx->d_canvas8.reserve(bytes, &ctx->render_allocs);
    if (st != RTC_OK) return st;
    void *d = f64 ? (void *)ctx->d_canvas.get() : (void *)ctx->d_canvas8.get();
    if (stats) st = rtc_stats_reset(ctx);
    if (st == RTC_OK) {
        LaunchRequest rq = rows_request(cam, mode, 0, cam->vsize, f64 ? d : nullptr, f64 ? nullptr : d, flags);
        rq.gamma = gamma;
        rq.lens = lens;
        rq.proj = proj;
        st = render_launch(ctx, w, rq);
    }
    if (st == RTC_OK && drain_lanes(ctx) != hipSuccess) st = RTC_ERR_DEVICE; // pipelined context: the copy below is on the stream
    // `host` from rtc_host_alloc (page-locked) is filled by one DMA at link speed; pageable memory
    // goes through the runtime's bounce buffers (several times slower)
    if (st == RTC_OK && hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) st = RTC_ERR_DEVICE;
    if (st == RTC_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = RTC_ERR_DEVICE;
    if (st == RTC_OK && stats) st = rtc_stats_read(ctx, stats);
    return st;
}

rtc_status rtc_render(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                      double *rgb, rtc_stats *stats) {
    return render_frame(ctx, w, cam, mode, flags, true, 0.f, rgb, stats);
}

rtc_status rtc_render_rgb8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                           uint8_t *rgb8, rtc_stats *stats) {
    return render_frame(ctx, w, cam, mode, flags, false, 0.f, rgb8, stats);
}

rtc_status rtc_render_lens(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_lens *lens, uint32_t mode,
                           uint32_t flags, double *rgb, rtc_stats *stats) {
    const rtc_status ls = check_lens(cam, lens);
    if (ls != RTC_OK) return ls;
    return render_frame(ctx, w, cam, mode, flags, true, 0.f, rgb, stats, lens);
}

rtc_status rtc_render_lens_rgb8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_lens *lens, uint32_t mode,
                                uint32_t flags, uint8_t *rgb8, rtc_stats *stats) {
    const rtc_status ls = check_lens(cam, lens);
    if (ls != RTC_OK) return ls;
    return render_frame(ctx, w, cam, mode, flags, false, 0.f, rgb8, stats, lens);
}

rtc_status rtc_render_projection(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode,
                                 uint32_t flags, double *rgb, rtc_stats *stats) {
    const rtc_status ps = check_projection(cam, proj);
    if (ps != RTC_OK) return ps;
    return render_frame(ctx, w, cam, mode, flags, true, 0.f, rgb, stats, nullptr, proj);
}

rtc_status rtc_render_projection_rgb8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode,
                                      uint32_t flags, uint8_t *rgb8, rtc_stats *stats) {
    const rtc_status ps = check_projection(cam, proj);
    if (ps != RTC_OK) return ps;
    return render_frame(ctx, w, cam, mode, flags, false, 0.f, rgb8, stats, nullptr, proj);
}

rtc_status rtc_render_rgba8(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags, float gamma,
                            uint8_t *rgba8, rtc_stats *stats) {
    if (!gamma_ok(gamma)) return RTC_ERR_ARG;
    return render_frame(ctx, w, cam, mode, flags, false, gamma, rgba8, stats);
}

rtc_status rtc_gamma_table_on_stream(rtc_context *ctx, float gamma, const DevGamma **out) {
    if (!ctx || !out || !gamma_ok(gamma)) return RTC_ERR_ARG;
    return gamma_table(ctx, gamma, ctx->stream, rtc_context::MAX_LANES, out);
}

rtc_status rtc_canvas_to_rgba8_device(rtc_context *ctx, const void *d_rgb, uint32_t width, uint32_t rows, float gamma, void *d_rgba8) {
    if (!ctx || !d_rgb || !d_rgba8 || !gamma_ok(gamma) || ((size_t)d_rgb % sizeof(double)) != 0) return RTC_ERR_ARG;
    const size_t n = (size_t)width * rows;
    if (n == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const DevGamma *g = nullptr;
    const rtc_status st = gamma_table(ctx, gamma, ctx->stream, rtc_context::MAX_LANES, &g);
    if (st != RTC_OK) return st;
    HIP_TRY(rtc_launch_canvas_to_rgba8(static_cast<const double *>(d_rgb), n, g, static_cast<unsigned char *>(d_rgba8), ctx->stream));
    return RTC_OK;
}

// ---- AOV planes (include/rtc.h, "arbitrary output variables") ---------------------------------------------------------
static bool aov_any(const rtc_aov_buffers *b) { return b->index || b->depth || b->point || b->normal || b->flags || b->shadow; }

extern "C++" { // (two templates: the entry points around them have C linkage)
// What the device entry points of the three tile passes (k_aov, k_ao, k_gather: one workgroup per 8x8 tile) share behind
// their own argument checks: the tile-count limit, the World's current generation, k_aov's plan (the same grid for all three,
// no dynamic LDS), the World's tables in `P` and the common fields of the pass's zeroed parameter block `A`; then
// fill(G) -> rtc_status, the pass's own set-up and fields, and launch(P, src, proj) -> hipError_t, its rtc_launch_* call, between
// order_behind_build and record_read.
// `proj`: NULL for the pinhole's centre rays, which changes nothing of the above; otherwise the (validated) projection whose
// rays the pass casts (rtc_render_*_projection*): its device block is filled as launch_planned fills k_trace's — the
// orthographic terms, or the panorama's tables through pano_tables, under the same key and the same wait — and handed to
// launch(); the plan, and with it what RTC_FLAG_LDS_TABLE answers, is the pinhole pass's. Such a launch is also the
// context's last one (rtc_context_last_launch_info, rtc_context_last_launch_projection; `LL`: the lights it read, or
// NULL); a pinhole pass leaves that record alone, as it always has.
template <class FILL, class LAUNCH>
static rtc_status tile_pass(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode, uint32_t flags,
                            TileParams &A, const LaunchLights *LL, FILL &&fill, LAUNCH &&launch) {
    if ((unsigned long long)((cam->hsize + 7u) / 8u) * ((cam->vsize + 7u) / 8u) > 0x7fffffffull) return RTC_ERR_ARG; // one workgroup per tile
    HIP_TRY(hipSetDevice(ctx->device));
    rtc_world::Gen *gen = nullptr;
    const rtc_status hs = current_gen(w, &gen);
    if (hs != RTC_OK) return hs;
    rtc_world::Gen &G = *gen;
    LaunchPlanInputs in = plan_inputs(ctx, G, RTC_PLAN_AOV, flags);
    in.hsize = cam->hsize; in.vsize = cam->vsize; in.mode = mode;
    LaunchPlan plan;
    rtc_plan_launch(in, plan);
    if (plan.status != RTC_OK) return (rtc_status)plan.status;
    RenderParams P;
    planned_params(ctx, w, G, plan, P);
    fill_camera(P, cam);
    A.cam = P.views[0];
    A.W = cam->hsize;
    A.H = cam->vsize;
    A.mode = mode;
    A.tiles_x = plan.grid_x;
    A.n = G.n;
    A.ngroups = G.ngroups;
    A.pre_limit = G.pre_limit;
    const rtc_status fs = fill(G);
    if (fs != RTC_OK) return fs;
    DevProjection dproj{};
    if (proj) {
        dproj.kind = proj->kind;
        if (proj->kind == RTC_PROJ_ORTHOGRAPHIC) {
            double t[3];
            rtc_projection_ortho_terms(cam->hsize, cam->vsize, proj->width, t);
            dproj.half_w = t[0]; dproj.half_h = t[1]; dproj.pixel = t[2];
        } else {
            const rtc_status ts = pano_tables(ctx, cam, proj);
            if (ts != RTC_OK) return ts;
            dproj.col = ctx->d_pano_col.get();
            dproj.row = ctx->d_pano_row.get();
        }
    }
    HIP_TRY(order_behind_build(G, ctx->stream, BIT_STREAM));
    HIP_TRY(launch(P, plan.src, proj ? &dproj : nullptr));
    HIP_TRY(record_read(w, G, ctx->stream, BIT_STREAM));
    if (proj) { // (uncounted in rtc_stats, as every tile pass: no pixels, no rays)
        ctx->last = rtc_launch_info{(uint32_t)plan.src, 0u, 0u, 0u, 0u, 0u, 64u, 0u, 1u, 0u, (LL && LL->lt) ? 1u : 0u, 0u};
        ctx->last_projection = proj->kind;
        ++ctx->launches_total;
    }
    return RTC_OK;
}

// The host-buffer twins' way back: each wanted plane (bytes != 0) copied on the context's stream, then the stream's end
// awaited — after a failed copy too, which ends the copying.
struct PlaneCopy {
    void *dst;
    const void *src;
    size_t bytes;
};
template <size_t N> static rtc_status copy_planes_back(rtc_context *ctx, const PlaneCopy (&planes)[N]) {
    rtc_status out = RTC_OK;
    for (const PlaneCopy &c : planes)
        if (out == RTC_OK && c.bytes && hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) out = RTC_ERR_DEVICE;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) out = RTC_ERR_DEVICE;
    return out;
}
} // extern "C++"

// The three device entry points, each behind its two public forms: `proj` NULL is the pinhole entry, whose checks these are;
// the projection entry has made rtc_render_projection's checks (projection_pass_args) first.
static rtc_status aov_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode, uint32_t flags,
                             const rtc_aov_buffers *d) {
    if (check_render_args(ctx, w, cam, mode, d, nullptr) != RTC_OK || !aov_any(d)) return RTC_ERR_ARG;
    if (((size_t)d->depth | (size_t)d->point | (size_t)d->normal) % sizeof(double) != 0 || (size_t)d->index % 4u != 0 || (size_t)d->shadow % 2u != 0)
        return RTC_ERR_ARG;
    AovParams A;
    std::memset(&A, 0, sizeof A);
    LaunchLights LL;
    return tile_pass(ctx, w, cam, proj, mode, flags, A, &LL,
        [&](rtc_world::Gen &G) {
            if (d->shadow) lights_of(G, LL);
            for (int k = 0; k < 3; ++k) A.light_pos[k] = G.light.position[k];
            A.index = d->index; A.depth = d->depth; A.point = d->point; A.normal = d->normal; A.flags = d->flags; A.shadow = d->shadow;
            return RTC_OK;
        },
        [&](const RenderParams &P, int src, const DevProjection *dp) { return rtc_launch_aov(&A, &P, src, LL.xl, LL.lt, dp, ctx->stream); });
}

// What the projection forms of the tile passes check first, in this order (include/rtc.h): rtc_render_projection's own —
// a context with its own World, a camera with a canvas, somewhere to write, a known mode; a valid projection, one ray per
// pixel — and then the pinhole pass's.
static rtc_status projection_pass_args(const rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode,
                                       const void *out) {
    if (check_render_args(ctx, w, cam, mode, out, nullptr) != RTC_OK) return RTC_ERR_ARG;
    return check_projection(cam, proj);
}

rtc_status rtc_render_aov_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                                 const rtc_aov_buffers *d) {
    return aov_device(ctx, w, cam, nullptr, mode, flags, d);
}

rtc_status rtc_render_aov_projection_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode,
                                            uint32_t flags, const rtc_aov_buffers *d) {
    const rtc_status ps = projection_pass_args(ctx, w, cam, proj, mode, d);
    return ps != RTC_OK ? ps : aov_device(ctx, w, cam, proj, mode, flags, d);
}

static rtc_status aov_host(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode, uint32_t flags,
                           const rtc_aov_buffers *host) {
    if (!ctx || !w || !cam || !host || w->ctx != ctx || !aov_any(host)) return RTC_ERR_ARG;
    if (cam->hsize == 0 || cam->vsize == 0) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)cam->hsize * cam->vsize;
    // one grow-only block, the planes in order of alignment: depth, point, normal (8), index (4), shadow (2), flags (1)
    const size_t sizes[6] = {host->depth ? 8u * px : 0u, host->point ? 24u * px : 0u, host->normal ? 24u * px : 0u,
                             host->index ? 4u * px : 0u, host->shadow ? 2u * px : 0u, host->flags ? px : 0u};
    void *const dst[6] = {host->depth, host->point, host->normal, host->index, host->shadow, host->flags};
    size_t off[6], total = 0;
    for (int k = 0; k < 6; ++k) {
        off[k] = total;
        total += (sizes[k] + 7u) & ~(size_t)7u;
    }
    const rtc_status st = ctx->d_aov.reserve(total, &ctx->render_allocs);
    if (st != RTC_OK) return st;
    unsigned char *base = ctx->d_aov.get();
    rtc_aov_buffers d;
    d.depth = host->depth ? reinterpret_cast<double *>(base + off[0]) : nullptr;
    d.point = host->point ? reinterpret_cast<double *>(base + off[1]) : nullptr;
    d.normal = host->normal ? reinterpret_cast<double *>(base + off[2]) : nullptr;
    d.index = host->index ? reinterpret_cast<int32_t *>(base + off[3]) : nullptr;
    d.shadow = host->shadow ? reinterpret_cast<uint16_t *>(base + off[4]) : nullptr;
    d.flags = host->flags ? base + off[5] : nullptr;
    const rtc_status ls = aov_device(ctx, w, cam, proj, mode, flags, &d);
    if (ls != RTC_OK) return ls;
    PlaneCopy back[6];
    for (int k = 0; k < 6; ++k) back[k] = PlaneCopy{dst[k], base + off[k], sizes[k]};
    return copy_planes_back(ctx, back);
}

rtc_status rtc_render_aov(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, uint32_t mode, uint32_t flags,
                          const rtc_aov_buffers *host) {
    return aov_host(ctx, w, cam, nullptr, mode, flags, host);
}

rtc_status rtc_render_aov_projection(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, uint32_t mode,
                                     uint32_t flags, const rtc_aov_buffers *host) {
    const rtc_status ps = projection_pass_args(ctx, w, cam, proj, mode, host);
    return ps != RTC_OK ? ps : aov_host(ctx, w, cam, proj, mode, flags, host);
}

rtc_status rtc_aov_view_rgb8_device(rtc_context *ctx, uint32_t view, const rtc_aov_buffers *d, uint32_t width, uint32_t height, double near,
                                    double far, uint32_t n_lights, void *d_rgb8) {
    if (!ctx || !d_rgb8) return RTC_ERR_ARG;
    const rtc_status st = rtc_aov_view_check(view, d, near, far, n_lights);
    if (st != RTC_OK) return st;
    if (((size_t)d->depth | (size_t)d->normal) % sizeof(double) != 0 || (size_t)d->index % 4u != 0 || (size_t)d->shadow % 2u != 0) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    AovViewParams V;
    std::memset(&V, 0, sizeof V);
    V.view = view;
    V.n_lights = n_lights;
    V.n = (size_t)width * height;
    V.near = near;
    V.far = far;
    V.index = d->index; V.depth = d->depth; V.normal = d->normal; V.shadow = d->shadow;
    V.out = static_cast<unsigned char *>(d_rgb8);
    HIP_TRY(rtc_launch_aov_view(&V, ctx->stream));
    return RTC_OK;
}

// ---- ambient occlusion (include/rtc.h) ------------------------------------------------------------------------------------
// The sample table of `ao`'s grid in the context's buffer, for work enqueued next on the context's stream.
static rtc_status ao_table(rtc_context *ctx, const rtc_ao *ao) {
    const rtc_status rs = ctx->d_ao_dirs.reserve(3u * RTC_MAX_AO_SAMPLES, &ctx->render_allocs);
    if (rs != RTC_OK) return rs;
    if (ctx->ao_usteps == ao->usteps && ctx->ao_vsteps == ao->vsteps) return RTC_OK;
    // another grid: launches in flight read the old table (stream order covers the device side) and an earlier copy may
    // still read ao_host
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->ao_usteps = ctx->ao_vsteps = 0u;
    uint32_t n = 0;
    const rtc_status es = rtc_ao_expand(ao, ctx->ao_host, &n);
    if (es != RTC_OK) return es;
    HIP_TRY(hipMemcpyAsync(ctx->d_ao_dirs.get(), ctx->ao_host, sizeof(double) * 3u * n, hipMemcpyHostToDevice, ctx->stream));
    ctx->ao_usteps = ao->usteps;
    ctx->ao_vsteps = ao->vsteps;
    return RTC_OK;
}

static rtc_status ao_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, const rtc_ao *ao, uint32_t mode,
                            uint32_t flags, uint16_t *d_ao) {
    if (check_render_args(ctx, w, cam, mode, d_ao, nullptr) != RTC_OK || rtc_ao_validate(ao) != RTC_OK) return RTC_ERR_ARG;
    if ((size_t)d_ao % 2u != 0) return RTC_ERR_ARG;
    AoParams A;
    std::memset(&A, 0, sizeof A);
    return tile_pass(ctx, w, cam, proj, mode, flags, A, nullptr,
        [&](rtc_world::Gen &) {
            A.radius = ao->radius;
            A.nsamples = ao->usteps * ao->vsteps;
            A.out = d_ao;
            return ao_table(ctx, ao);
        },
        [&](const RenderParams &P, int src, const DevProjection *dp) { return rtc_launch_ao(&A, ctx->d_ao_dirs.get(), &P, src, dp, ctx->stream); });
}

rtc_status rtc_render_ao_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_ao *ao, uint32_t mode,
                                uint32_t flags, uint16_t *d_ao) {
    return ao_device(ctx, w, cam, nullptr, ao, mode, flags, d_ao);
}

rtc_status rtc_render_ao_projection_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, const rtc_ao *ao,
                                           uint32_t mode, uint32_t flags, uint16_t *d_ao) {
    const rtc_status ps = projection_pass_args(ctx, w, cam, proj, mode, d_ao);
    return ps != RTC_OK ? ps : ao_device(ctx, w, cam, proj, ao, mode, flags, d_ao);
}

static rtc_status ao_host(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, const rtc_ao *ao, uint32_t mode,
                          uint32_t flags, uint16_t *ao_out) {
    if (!ctx || !w || !cam || !ao_out || w->ctx != ctx || rtc_ao_validate(ao) != RTC_OK) return RTC_ERR_ARG;
    if (cam->hsize == 0 || cam->vsize == 0) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t px = (size_t)cam->hsize * cam->vsize;
    const rtc_status st = ctx->d_ao.reserve(px, &ctx->render_allocs);
    if (st != RTC_OK) return st;
    const rtc_status ls = ao_device(ctx, w, cam, proj, ao, mode, flags, ctx->d_ao.get());
    if (ls != RTC_OK) return ls;
    return copy_planes_back(ctx, {{ao_out, ctx->d_ao.get(), sizeof(uint16_t) * px}});
}

rtc_status rtc_render_ao(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_ao *ao, uint32_t mode, uint32_t flags,
                         uint16_t *ao_out) {
    return ao_host(ctx, w, cam, nullptr, ao, mode, flags, ao_out);
}

rtc_status rtc_render_ao_projection(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, const rtc_ao *ao,
                                    uint32_t mode, uint32_t flags, uint16_t *ao_out) {
    const rtc_status ps = projection_pass_args(ctx, w, cam, proj, mode, ao_out);
    return ps != RTC_OK ? ps : ao_host(ctx, w, cam, proj, ao, mode, flags, ao_out);
}

rtc_status rtc_canvas_apply_ao_device(rtc_context *ctx, void *d_rgb, const void *d_ao, uint32_t n_samples, double strength, uint32_t width,
                                      uint32_t height) {
    if (!ctx || !d_rgb || !d_ao || rtc_ao_apply_check(n_samples, strength) != RTC_OK) return RTC_ERR_ARG;
    if (((size_t)d_rgb % sizeof(double)) != 0 || ((size_t)d_ao % 2u) != 0) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    if (n == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(rtc_launch_apply_ao(static_cast<double *>(d_rgb), static_cast<const uint16_t *>(d_ao), n, n_samples, strength, ctx->stream));
    return RTC_OK;
}

// ---- colour bleeding: the one-bounce gather pass (include/rtc.h) ----------------------------------------------------------
static rtc_status gather_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, const rtc_ao *ao,
                                uint32_t mode, uint32_t flags, const rtc_gather_buffers *d) {
    if (check_render_args(ctx, w, cam, mode, d, nullptr) != RTC_OK || rtc_ao_validate(ao) != RTC_OK) return RTC_ERR_ARG;
    if (!d->radiance && !d->bounce) return RTC_ERR_ARG;
    if (((size_t)d->radiance | (size_t)d->bounce) % sizeof(double) != 0) return RTC_ERR_ARG;
    GatherParams A;
    std::memset(&A, 0, sizeof A);
    LaunchLights LL;
    return tile_pass(ctx, w, cam, proj, mode, flags, A, &LL,
        [&](rtc_world::Gen &G) {
            lights_of(G, LL);
            A.radius = ao->radius;
            A.nsamples = ao->usteps * ao->vsteps;
            for (int k = 0; k < 3; ++k) {
                A.light_pos[k] = G.light.position[k];
                A.light_int[k] = G.light.intensity[k];
            }
            A.radiance = d->radiance;
            A.bounce = d->bounce;
            return ao_table(ctx, ao); // the fan is the AO pass's: one table per context, whichever pass filled it
        },
        [&](const RenderParams &P, int src, const DevProjection *dp) {
            return rtc_launch_gather(&A, ctx->d_ao_dirs.get(), &P, src, LL.xl, LL.lt, dp, ctx->stream);
        });
}

rtc_status rtc_render_gather_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_ao *ao, uint32_t mode,
                                    uint32_t flags, const rtc_gather_buffers *d) {
    return gather_device(ctx, w, cam, nullptr, ao, mode, flags, d);
}

rtc_status rtc_render_gather_projection_device(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj,
                                               const rtc_ao *ao, uint32_t mode, uint32_t flags, const rtc_gather_buffers *d) {
    const rtc_status ps = projection_pass_args(ctx, w, cam, proj, mode, d);
    return ps != RTC_OK ? ps : gather_device(ctx, w, cam, proj, ao, mode, flags, d);
}

static rtc_status gather_host(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, const rtc_ao *ao, uint32_t mode,
                              uint32_t flags, const rtc_gather_buffers *host) {
    if (!ctx || !w || !cam || !host || (!host->radiance && !host->bounce) || w->ctx != ctx || rtc_ao_validate(ao) != RTC_OK) return RTC_ERR_ARG;
    if (cam->hsize == 0 || cam->vsize == 0) return RTC_ERR_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t plane = (size_t)cam->hsize * cam->vsize * 3u;
    const rtc_status st = ctx->d_gather.reserve(2u * plane, &ctx->render_allocs);
    if (st != RTC_OK) return st;
    rtc_gather_buffers d;
    d.radiance = host->radiance ? ctx->d_gather.get() : nullptr;
    d.bounce = host->bounce ? ctx->d_gather.get() + plane : nullptr;
    const rtc_status ls = gather_device(ctx, w, cam, proj, ao, mode, flags, &d);
    if (ls != RTC_OK) return ls;
    return copy_planes_back(ctx, {{host->radiance, d.radiance, d.radiance ? sizeof(double) * plane : 0u},
                                  {host->bounce, d.bounce, d.bounce ? sizeof(double) * plane : 0u}});
}

rtc_status rtc_render_gather(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_ao *ao, uint32_t mode, uint32_t flags,
                             const rtc_gather_buffers *host) {
    return gather_host(ctx, w, cam, nullptr, ao, mode, flags, host);
}

rtc_status rtc_render_gather_projection(rtc_context *ctx, const rtc_world *w, const rtc_camera *cam, const rtc_projection *proj, const rtc_ao *ao,
                                        uint32_t mode, uint32_t flags, const rtc_gather_buffers *host) {
    const rtc_status ps = projection_pass_args(ctx, w, cam, proj, mode, host);
    return ps != RTC_OK ? ps : gather_host(ctx, w, cam, proj, ao, mode, flags, host);
}

rtc_status rtc_canvas_add_scaled_device(rtc_context *ctx, void *d_rgb, const void *d_plane, double strength, uint32_t width, uint32_t height) {
    if (!ctx || !d_rgb || !d_plane || rtc_gather_strength_check(strength) != RTC_OK) return RTC_ERR_ARG;
    if (((size_t)d_rgb | (size_t)d_plane) % sizeof(double) != 0) return RTC_ERR_ARG;
    const size_t n = (size_t)width * height;
    if (n == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(rtc_launch_add_scaled(static_cast<double *>(d_rgb), static_cast<const double *>(d_plane), n, strength, ctx->stream));
    return RTC_OK;
}

rtc_status rtc_host_alloc(size_t bytes, void **out) {
    if (!out || bytes == 0) return RTC_ERR_ARG;
    *out = nullptr;
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipErrorOutOfMemory) return RTC_ERR_NOMEM;
    if (e != hipSuccess) return RTC_ERR_DEVICE;
    *out = p;
    return RTC_OK;
}

void rtc_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

rtc_status rtc_host_register(void *p, size_t bytes) {
    if (!p || bytes == 0) return RTC_ERR_ARG;
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e == hipErrorOutOfMemory) return RTC_ERR_NOMEM;
    if (e == hipErrorHostMemoryAlreadyRegistered) { (void)hipGetLastError(); return RTC_OK; }
    return e == hipSuccess ? RTC_OK : RTC_ERR_DEVICE;
}

rtc_status rtc_host_unregister(void *p) {
    if (!p) return RTC_ERR_ARG;
    return hipHostUnregister(p) == hipSuccess ? RTC_OK : RTC_ERR_DEVICE;
}

// (rtc_internal.h) the probe launch of rtc_color_at and of the adaptive pass's refinement: plan, parameters, trace
rtc_status rtc_color_at_device(rtc_context *ctx, const rtc_world *w, const double *d_rays, uint32_t n, uint32_t remaining, uint32_t flags,
                               double *d_rgb, rtc_hit *d_hits, bool record) {
    rtc_world::Gen *gen = nullptr;
    const rtc_status gs = current_gen(w, &gen);
    if (gs != RTC_OK) return gs;
    rtc_world::Gen &G = *gen;
    HIP_TRY(order_behind_build(G, ctx->stream, BIT_STREAM));
    LaunchPlanInputs in = plan_inputs(ctx, G, RTC_PLAN_PROBE, flags);
    in.hsize = n;
    LaunchPlan plan;
    rtc_plan_launch(in, plan);
    if (plan.status != RTC_OK) return (rtc_status)plan.status;
    RenderParams P;
    planned_params(ctx, w, G, plan, P);
    P.W = n; P.H = 1; P.y0 = 0; P.y1 = 1; P.mode = RTC_MODE_RENDER_ASYNC; P.samples = 1;
    P.grid_y = 1;
    P.band_stride = 1;
    P.out = d_rgb;
    P.rays = d_rays;
    P.nrays = n;
    P.remaining = remaining;
    P.hits = d_hits;
    LaunchLights LL;
    lights_of(G, LL);
    if (trace_planned(ctx, P, plan, LL, ctx->stream, nullptr, nullptr, nullptr, nullptr) != hipSuccess) return RTC_ERR_DEVICE;
    if (record) HIP_TRY(record_read(w, G, ctx->stream, BIT_STREAM));
    return RTC_OK;
}

rtc_status rtc_color_at(rtc_context *ctx, const rtc_world *w, const double *rays, uint32_t n, uint32_t remaining,
                        uint32_t flags, double *rgb, rtc_hit *hits) {
    if (!ctx || !w || !rays || !rgb || w->ctx != ctx) return RTC_ERR_ARG;
    if (remaining > RTC_MAX_REFLECTIONS) return RTC_ERR_ARG; // frame stack depth of the kernel = Camera::MAX_REFLECTIONS (camera.rs:31)
    if (n == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<double> d_rays, d_rgb;
    DevBuf<rtc_hit> d_hits;
    rtc_world::Gen *gen = nullptr;
    rtc_status st = current_gen(w, &gen);
    if (st != RTC_OK) return st;
    HIP_TRY(order_behind_build(*gen, ctx->stream, BIT_STREAM));
    if (d_rays.reserve((size_t)6 * n) != RTC_OK || d_rgb.reserve((size_t)3 * n) != RTC_OK || (hits && d_hits.reserve(n) != RTC_OK))
        st = RTC_ERR_DEVICE;
    if (st == RTC_OK && hipMemcpyAsync(d_rays.get(), rays, sizeof(double) * 6 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        st = RTC_ERR_DEVICE;
    if (st == RTC_OK) st = rtc_color_at_device(ctx, w, d_rays.get(), n, remaining, flags, d_rgb.get(), d_hits.get(), false);
    if (st == RTC_OK && hipMemcpyAsync(rgb, d_rgb.get(), sizeof(double) * 3 * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        st = RTC_ERR_DEVICE;
    if (st == RTC_OK && hits && hipMemcpyAsync(hits, d_hits.get(), sizeof(rtc_hit) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        st = RTC_ERR_DEVICE;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) st = RTC_ERR_DEVICE;
    return st;
}

rtc_status rtc_device_arith(rtc_context *ctx, uint32_t op, const double *a, const double *b, uint32_t n, double *out) {
    if (!ctx || !a || !out || op > 9 || (op == 1 && !b) || (op == 2 && !b)) return RTC_ERR_ARG;
    if (n == 0) return RTC_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<double> da, db, dout;
    rtc_status st = RTC_OK;
    if (da.upload(a, n) != RTC_OK || db.upload(b ? b : a, n) != RTC_OK || dout.reserve(n) != RTC_OK) st = RTC_ERR_DEVICE;
    if (st == RTC_OK && rtc_launch_arith(op, da.get(), db.get(), n, dout.get(), ctx->stream) != hipSuccess) st = RTC_ERR_DEVICE;
    if (st == RTC_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = RTC_ERR_DEVICE;
    if (st == RTC_OK && hipMemcpy(out, dout.get(), sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) st = RTC_ERR_DEVICE;
    return st;
}

// Diagnostic (not part of include/rtc.h): rtc_parity.h's even test — the code the patterns run on the device — evaluated on
// the host for n values: out[i] = 1 where it holds. The CPU tests pin it against fmod(x, 2.0) == 0.0.
rtc_status rtc_debug_even_f64(const double *x, size_t n, uint8_t *out) {
    if (!x || !out) return RTC_ERR_ARG;
    for (size_t i = 0; i < n; ++i) out[i] = rtc_even_f64(x[i]) ? 1u : 0u;
    return RTC_OK;
}

} // extern "C"
