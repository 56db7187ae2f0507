// Host-only robustness check of the scene loader, the matrix helpers and the PPM / RGBA8 writers,
// meant to be built with -fsanitize=address,undefined (tests/test_host_cpu.py does that): feeds the
// loader the shipped scene, truncations of it at every byte, and a set of malformed documents; then every one of the 12 text
// entry points gets the shipped scene and the malformed documents, every `_file` twin the scene's path and an absent one. No GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rtc.h"

static int load(const std::string &text) {
    rtc_shape *shapes = nullptr;
    uint32_t n = 0;
    rtc_light light;
    rtc_camera cam;
    char err[256] = {0};
    const int st = rtc_scene_load_yaml(text.c_str(), &shapes, &n, &light, &cam, err, sizeof err);
    if (st == RTC_OK && n > 0 && shapes == nullptr) std::abort();
    rtc_free(shapes);
    return st;
}

// `src` through the 12 text entry points (file: a path through their `_file` twins); what they return is freed.
// -> how many answered RTC_OK
static int load_every_entry(const char *src, bool file) {
    rtc_shape *shapes = nullptr;
    rtc_motion *motions = nullptr;
    uint32_t n = 0, nl = 0, nm = 0, samples = 0, has[4] = {0, 0, 0, 0}, ow = 0, oh = 0;
    rtc_light light, lights[RTC_MAX_LIGHTS];
    rtc_area_light area[RTC_MAX_LIGHT_SAMPLES];
    const uint32_t cap = RTC_MAX_LIGHT_SAMPLES;
    rtc_camera cam;
    rtc_lens lens;
    rtc_projection proj;
    rtc_ao ao, gather;
    rtc_filter filter;
    rtc_adaptive aa;
    rtc_tonemap tonemap;
    rtc_bloom bloom;
    rtc_resize resize;
    char err[256] = {0};
    int ok = 0;
    auto done = [&](rtc_status st) {
        if (st == RTC_OK && n > 0 && shapes == nullptr) std::abort();
        rtc_free(shapes);
        shapes = nullptr;
        ok += st == RTC_OK;
    };
#define ENTRY(name) (file ? rtc_scene_load_yaml##name##_file : rtc_scene_load_yaml##name)
    done(ENTRY()(src, &shapes, &n, &light, &cam, err, sizeof err));
    done(ENTRY(_lights)(src, &shapes, &n, lights, RTC_MAX_LIGHTS, &nl, &cam, err, sizeof err));
    done(ENTRY(_area_lights)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err));
    done(ENTRY(_lens)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &lens, &has[0]));
    done(ENTRY(_motion)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &lens, &has[0], &motions, &nm, &samples));
    rtc_free(motions);
    done(ENTRY(_projection)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &lens, &has[0], &proj, &has[1]));
    done(ENTRY(_ao)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &lens, &has[0], &ao, &has[1]));
    done(ENTRY(_gather)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &lens, &has[0], &ao, &has[1], &gather, &has[2]));
    done(ENTRY(_filter)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &lens, &has[0], &ao, &has[1], &gather, &has[2], &filter, &has[3]));
    done(ENTRY(_adaptive)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &aa, &has[0]));
    done(ENTRY(_post)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &tonemap, &has[0], &bloom, &has[1]));
    done(ENTRY(_resize)(src, &shapes, &n, area, cap, &nl, &cam, err, sizeof err, &lens, &has[0], &proj, &has[1], &resize, &ow, &oh, &has[2]));
#undef ENTRY
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string doc = ss.str();
    if (load(doc) != RTC_OK) { std::puts("shipped scene does not load"); return 1; }
    int ok = 0, bad = 0;
    for (size_t cut = 0; cut < doc.size(); cut += 1) (load(doc.substr(0, cut)) == RTC_OK ? ok : bad)++;
    const char *junk[] = {"", "\n", "- add: sphere", "- add: camera\n  width: -3\n  height: 1e99\n  field-of-view: x",
                          "- add: sphere\n  transform:\n    - [ scale, 0, 0, 0 ]\n", "- define: a\n  extend: a\n  value:\n    color: [1,1,1]\n",
                          "- add: cube\n  material: nosuch\n", "- add: plane\n  transform: [[[[[[[[[[\n", "- add: sphere\n  material: { color: [1, 2 }\n",
                          "- add: light\n  at: [1,2]\n  intensity: [1,1,1,1,1]\n", "\t\t- add: sphere\n", "- add: sphere\n  material:\n    pattern:\n      type: nosuch\n",
                          "- define: t\n  value:\n    - [ translate, 1, 2, 3 ]\n- add: sphere\n  transform:\n    - t\n    - t\n    - [ rotate-x, nan ]\n"};
    for (const char *j : junk) (load(j) == RTC_OK ? ok : bad)++;
    // every entry point: the shipped scene loads through all 12 and their `_file` twins, the junk and an absent path through none
    if (load_every_entry(doc.c_str(), false) != 12 || load_every_entry(argv[1], true) != 12) { std::puts("an entry point rejects the shipped scene"); return 1; }
    for (const char *j : junk)
        if (load_every_entry(j, false) != 0) { std::puts("an entry point accepts a malformed document"); return 1; }
    if (load_every_entry((std::string(argv[1]) + ".absent").c_str(), true) != 0) { std::puts("an entry point loads an absent file"); return 1; }
    std::string big = "- add: camera\n  width: 10\n  height: 5\n  field-of-view: 1.0\n  from: [0, 0, -5]\n  to: [0, 0, 0]\n  up: [0, 1, 0]\n"
                      "- add: light\n  at: [1, 2, 3]\n  intensity: [1, 1, 1]\n";
    for (int i = 0; i < 3000; ++i) big += "- add: sphere\n  transform:\n    - [ translate, " + std::to_string(i) + ", 0, 0 ]\n";
    if (load(big) != RTC_OK) { std::puts("large document rejected"); return 1; }
    // matrix helpers and writers on edge values
    double m[16], inv[16], id[16];
    rtc_matrix_identity(id);
    rtc_matrix_scaling(id, 0., 1., 1., m);
    if (rtc_matrix_inverse(m, inv) != RTC_ERR_SINGULAR) return 1;
    std::vector<double> rgb(7 * 5 * 3, 0.5);
    rgb[0] = 1e308; rgb[1] = -1e308; rgb[2] = 0.0 / 1.0;
    std::vector<uint8_t> rgba(7 * 5 * 4);
    rtc_canvas_to_rgba8(rgb.data(), 7, 5, 2.2f, rgba.data());
    const size_t need = rtc_canvas_format_ppm(rgb.data(), 7, 5, nullptr, 0);
    std::vector<char> buf(need + 1);
    if (rtc_canvas_format_ppm(rgb.data(), 7, 5, buf.data(), buf.size()) != need) return 1;
    std::printf("loader: %d documents accepted, %d rejected, no crash\n", ok, bad);
    return 0;
}
