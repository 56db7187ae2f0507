// host_yaml.cpp — [host] scene loader for the `jamis.yml` vocabulary (ch1/jamis.yml:1-183).
//
// The reference ships jamis.yml as a data file but has no YAML loader (its only loader is
// Lua, ch1/src/lua.rs), so this is written new. It builds the same World /
// Camera the reference's constructors would:
//   - transform lists apply in listed order by LEFT-multiplication, exactly like the fluent
//     builders `identity().scaling(..).translation(..)` (transform.rs:53-69);
//   - materials start from Material::default() (white .1/.9/.9/200 0/0/1.0) as lua.rs:187 does,
//     and an unknown material key is an error as in lua.rs:216;
//   - shapes go through {Sphere,Plane,Cube}::new_with_transform_and_material (inverse +
//     transpose at construction, shape.rs:308-317) and get world ids like World::add_shape
//     (shape.rs:661-667); only the first light is used (lua.rs:148-150);
//   - camera = Camera::new_with_transform(width, height, field-of-view,
//     make_view_transform(from, to, up)) (camera.rs:33, transform.rs:204).
//
// The parser accepts the YAML subset the vocabulary needs: block maps and sequences by
// indentation, "- key: value" items, flow sequences "[a, b]" and flow maps "{k: v}", comments,
// plain scalars.
#include "rtc.h"

#include <cmath>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

struct Node {
    enum Kind { Scalar, Seq, Map } kind = Scalar;
    std::string scalar;
    std::vector<std::shared_ptr<Node>> seq;
    std::vector<std::pair<std::string, std::shared_ptr<Node>>> map;
    int line = 0;

    const Node *get(const std::string &key) const {
        for (const auto &kv : map)
            if (kv.first == key) return kv.second.get();
        return nullptr;
    }
};
using NodeP = std::shared_ptr<Node>;

struct ParseError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

[[noreturn]] void fail(int line, const std::string &msg) {
    throw ParseError("line " + std::to_string(line) + ": " + msg);
}

struct Line {
    int indent;
    std::string text; // without indentation, comments and trailing blanks
    int number;
};

std::string strip(const std::string &s) {
    size_t a = 0, b = s.size();
    while (a < b && (s[a] == ' ' || s[a] == '\t' || s[a] == '\r')) ++a;
    while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t' || s[b - 1] == '\r')) --b;
    return s.substr(a, b - a);
}

std::vector<Line> split_lines(const char *text) {
    std::vector<Line> out;
    int number = 0;
    const char *p = text;
    while (*p) {
        const char *e = std::strchr(p, '\n');
        std::string raw = e ? std::string(p, e) : std::string(p);
        p = e ? e + 1 : p + raw.size();
        ++number;
        // drop comments (a '#' at line start or preceded by whitespace; no quoted strings here)
        for (size_t i = 0; i < raw.size(); ++i)
            if (raw[i] == '#' && (i == 0 || raw[i - 1] == ' ' || raw[i - 1] == '\t')) { raw.resize(i); break; }
        size_t ind = 0;
        while (ind < raw.size() && raw[ind] == ' ') ++ind;
        std::string body = strip(raw);
        if (body.empty() || body == "---") continue;
        if (ind < raw.size() && raw[ind] == '\t') fail(number, "tab indentation is not supported");
        out.push_back(Line{static_cast<int>(ind), body, number});
    }
    return out;
}

// ---- flow values: scalars and [ ... ] -------------------------------------------------
NodeP parse_flow(const std::string &s, size_t &i, int line) {
    while (i < s.size() && s[i] == ' ') ++i;
    auto n = std::make_shared<Node>();
    n->line = line;
    if (i < s.size() && s[i] == '[') {
        n->kind = Node::Seq;
        ++i;
        for (;;) {
            while (i < s.size() && s[i] == ' ') ++i;
            if (i >= s.size()) fail(line, "unterminated '['");
            if (s[i] == ']') { ++i; break; }
            n->seq.push_back(parse_flow(s, i, line));
            while (i < s.size() && s[i] == ' ') ++i;
            if (i < s.size() && s[i] == ',') { ++i; continue; }
            if (i < s.size() && s[i] == ']') { ++i; break; }
            fail(line, "expected ',' or ']' in flow sequence");
        }
        return n;
    }
    if (i < s.size() && s[i] == '{') { // flow map {key: value, ...}
        n->kind = Node::Map;
        ++i;
        for (;;) {
            while (i < s.size() && s[i] == ' ') ++i;
            if (i >= s.size()) fail(line, "unterminated '{'");
            if (s[i] == '}') { ++i; break; }
            const size_t c = s.find(':', i);
            if (c == std::string::npos) fail(line, "expected 'key: value' in flow map");
            const std::string key = strip(s.substr(i, c - i));
            if (key.empty() || key.find_first_of(",{}[]") != std::string::npos) fail(line, "bad key in flow map");
            i = c + 1;
            n->map.emplace_back(key, parse_flow(s, i, line));
            while (i < s.size() && s[i] == ' ') ++i;
            if (i < s.size() && s[i] == ',') { ++i; continue; }
            if (i < s.size() && s[i] == '}') { ++i; break; }
            fail(line, "expected ',' or '}' in flow map");
        }
        return n;
    }
    size_t start = i;
    while (i < s.size() && s[i] != ',' && s[i] != ']' && s[i] != '}') ++i;
    n->kind = Node::Scalar;
    n->scalar = strip(s.substr(start, i - start));
    if (n->scalar.size() >= 2 && ((n->scalar.front() == '"' && n->scalar.back() == '"') ||
                                  (n->scalar.front() == '\'' && n->scalar.back() == '\'')))
        n->scalar = n->scalar.substr(1, n->scalar.size() - 2);
    return n;
}

NodeP parse_inline_value(const std::string &s, int line) {
    size_t i = 0;
    NodeP n = parse_flow(s, i, line);
    while (i < s.size() && s[i] == ' ') ++i;
    if (i != s.size() && n->kind != Node::Scalar) fail(line, "trailing characters after flow value");
    if (n->kind == Node::Scalar) n->scalar = strip(s);
    return n;
}

// ---- block structure --------------------------------------------------------------------
struct Parser {
    std::vector<Line> lines;
    size_t pos = 0;

    static bool split_key(const std::string &t, std::string &key, std::string &rest) {
        if (t.empty() || t[0] == '[' || t[0] == '-') return false;
        size_t c = t.find(':');
        if (c == std::string::npos) return false;
        if (c + 1 < t.size() && t[c + 1] != ' ') return false;
        key = strip(t.substr(0, c));
        rest = strip(t.substr(c + 1));
        return !key.empty();
    }

    NodeP parse_block(int indent) {
        if (pos >= lines.size()) fail(lines.empty() ? 0 : lines.back().number, "unexpected end of document");
        const Line &l = lines[pos];
        if (l.text[0] == '-' && (l.text.size() == 1 || l.text[1] == ' ')) return parse_seq(indent);
        return parse_map(indent);
    }

    NodeP parse_seq(int indent) {
        auto n = std::make_shared<Node>();
        n->kind = Node::Seq;
        n->line = lines[pos].number;
        while (pos < lines.size() && lines[pos].indent == indent && lines[pos].text[0] == '-' &&
               (lines[pos].text.size() == 1 || lines[pos].text[1] == ' ')) {
            Line l = lines[pos];
            std::string rest = strip(l.text.substr(1));
            if (rest.empty()) {
                ++pos;
                if (pos >= lines.size() || lines[pos].indent <= indent) fail(l.number, "empty sequence item");
                n->seq.push_back(parse_block(lines[pos].indent));
                continue;
            }
            std::string key, val;
            if (split_key(rest, key, val)) {
                // "- key: value": a map whose first key sits on the dash line; re-enter it as a
                // map at the column of the key.
                int key_col = indent + static_cast<int>(l.text.size() - strip(l.text.substr(1)).size());
                lines[pos].indent = key_col;
                lines[pos].text = rest;
                n->seq.push_back(parse_map(key_col));
            } else {
                n->seq.push_back(parse_inline_value(rest, l.number));
                ++pos;
            }
        }
        if (pos < lines.size() && lines[pos].indent > indent) fail(lines[pos].number, "bad indentation in sequence");
        return n;
    }

    NodeP parse_map(int indent) {
        auto n = std::make_shared<Node>();
        n->kind = Node::Map;
        n->line = lines[pos].number;
        while (pos < lines.size() && lines[pos].indent == indent) {
            const Line l = lines[pos];
            std::string key, val;
            if (!split_key(l.text, key, val)) {
                if (l.text[0] == '-') break; // next item of an enclosing sequence at this column
                fail(l.number, "expected 'key: value'");
            }
            ++pos;
            NodeP child;
            if (!val.empty()) {
                child = parse_inline_value(val, l.number);
            } else if (pos < lines.size() && (lines[pos].indent > indent ||
                       (lines[pos].indent == indent && lines[pos].text[0] == '-' && indent > 0))) {
                child = parse_block(lines[pos].indent);
            } else {
                child = std::make_shared<Node>(); // empty scalar
                child->line = l.number;
            }
            n->map.emplace_back(key, child);
        }
        if (pos < lines.size() && lines[pos].indent > indent) fail(lines[pos].number, "bad indentation in map");
        return n;
    }
};

// ---- interpretation ---------------------------------------------------------------------
double as_number(const Node *n, const char *what) {
    if (!n || n->kind != Node::Scalar || n->scalar.empty()) fail(n ? n->line : 0, std::string("expected a number for ") + what);
    char *end = nullptr;
    const double v = std::strtod(n->scalar.c_str(), &end);
    if (end == n->scalar.c_str() || *end != 0) fail(n->line, std::string("invalid number for ") + what + ": " + n->scalar);
    return v;
}

void as_triple(const Node *n, const char *what, double out[3]) {
    if (!n || n->kind != Node::Seq || n->seq.size() != 3) fail(n ? n->line : 0, std::string("expected [x, y, z] for ") + what);
    for (int i = 0; i < 3; ++i) out[i] = as_number(n->seq[i].get(), what);
}

struct Defs {
    std::map<std::string, NodeP> values;
};

// Resolve `define`d names and `extend:` chains into a flat key list: base keys first, then the
// map's own keys in listed order (later entries override earlier ones when applied).
void flatten_material(const Defs &defs, const Node *n, std::vector<std::pair<std::string, const Node *>> &out, int depth = 0) {
    if (!n) return;
    if (depth > 16) fail(n->line, "definition recursion too deep");
    if (n->kind == Node::Scalar) {
        auto it = defs.values.find(n->scalar);
        if (it == defs.values.end()) fail(n->line, "unknown material name: " + n->scalar);
        flatten_material(defs, it->second.get(), out, depth + 1);
        return;
    }
    if (n->kind != Node::Map) fail(n->line, "material must be a name or a map");
    if (const Node *ext = n->get("extend")) flatten_material(defs, ext, out, depth + 1);
    for (const auto &kv : n->map)
        if (kv.first != "extend") out.emplace_back(kv.first, kv.second.get());
}

void build_transform(const Defs &defs, const Node *list, double m[16], int depth = 0) {
    if (!list) return;
    if (depth > 16) fail(list->line, "definition recursion too deep");
    if (list->kind != Node::Seq) fail(list->line, "transform must be a list");
    for (const auto &itp : list->seq) {
        const Node *it = itp.get();
        if (it->kind == Node::Scalar) { // reference to a defined transform list
            auto d = defs.values.find(it->scalar);
            if (d == defs.values.end()) fail(it->line, "unknown transform name: " + it->scalar);
            build_transform(defs, d->second.get(), m, depth + 1);
            continue;
        }
        if (it->kind != Node::Seq || it->seq.empty() || it->seq[0]->kind != Node::Scalar) fail(it->line, "bad transform item");
        const std::string &op = it->seq[0]->scalar;
        auto arg = [&](size_t i) { return as_number(i < it->seq.size() ? it->seq[i].get() : nullptr, op.c_str()); };
        auto need = [&](size_t n) { if (it->seq.size() != n + 1) fail(it->line, op + " takes " + std::to_string(n) + " numbers"); };
        if (op == "scale") { need(3); rtc_matrix_scaling(m, arg(1), arg(2), arg(3), m); }
        else if (op == "translate") { need(3); rtc_matrix_translation(m, arg(1), arg(2), arg(3), m); }
        else if (op == "rotate-x") { need(1); rtc_matrix_rotation_x(m, arg(1), m); }
        else if (op == "rotate-y") { need(1); rtc_matrix_rotation_y(m, arg(1), m); }
        else if (op == "rotate-z") { need(1); rtc_matrix_rotation_z(m, arg(1), m); }
        else if (op == "shear") { need(6); rtc_matrix_shearing(m, arg(1), arg(2), arg(3), arg(4), arg(5), arg(6), m); }
        else fail(it->line, "unknown transform: " + op);
    }
}

void apply_pattern(const Defs &defs, const Node *p, rtc_material &mat) {
    if (!p || p->kind != Node::Map) fail(p ? p->line : 0, "pattern must be a map");
    const Node *type = p->get("type");
    if (!type || type->kind != Node::Scalar) fail(p->line, "pattern needs a type");
    uint32_t kind;
    if (type->scalar == "stripes") kind = RTC_PATTERN_STRIPE;
    else if (type->scalar == "checkers") kind = RTC_PATTERN_CHECKER;
    else if (type->scalar == "gradient") kind = RTC_PATTERN_GRADIENT;
    else if (type->scalar == "ring" || type->scalar == "rings") kind = RTC_PATTERN_RING;
    else if (type->scalar == "grid") kind = RTC_PATTERN_GRID;
    else if (type->scalar == "test") kind = RTC_PATTERN_TEST;
    else fail(type->line, "unknown pattern type: " + type->scalar);
    double a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    const Node *colors = p->get("colors");
    if (kind != RTC_PATTERN_TEST) {
        if (!colors || colors->kind != Node::Seq || colors->seq.size() != 2) fail(p->line, "pattern needs colors: [a, b]");
        as_triple(colors->seq[0].get(), "pattern colour", a);
        as_triple(colors->seq[1].get(), "pattern colour", b);
    }
    double xf[16];
    rtc_matrix_identity(xf);
    build_transform(defs, p->get("transform"), xf);
    for (const auto &kv : p->map)
        if (kv.first != "type" && kv.first != "colors" && kv.first != "transform") fail(kv.second->line, "Invalid pattern property: " + kv.first);
    const rtc_status st = rtc_material_set_pattern(&mat, kind, a, b, xf);
    if (st != RTC_OK) fail(p->line, "pattern transform: " + std::string(rtc_strerror(st)));
}

void build_material(const Defs &defs, const Node *n, rtc_material &mat) {
    rtc_material_default(&mat); // lua.rs:187
    std::vector<std::pair<std::string, const Node *>> pairs;
    flatten_material(defs, n, pairs);
    for (const auto &kv : pairs) {
        const std::string &key = kv.first;
        const Node *v = kv.second;
        if (key == "color") { as_triple(v, "color", mat.color); mat.has_color = 1; }
        else if (key == "ambient") mat.ambient = as_number(v, "ambient");
        else if (key == "diffuse") mat.diffuse = as_number(v, "diffuse");
        else if (key == "specular") mat.specular = as_number(v, "specular");
        else if (key == "shininess") mat.shininess = as_number(v, "shininess");
        else if (key == "reflective") mat.reflective = as_number(v, "reflective");
        else if (key == "transparency") mat.transparency = as_number(v, "transparency");
        else if (key == "refractive-index") mat.refractive_index = as_number(v, "refractive-index");
        else if (key == "pattern") apply_pattern(defs, v, mat);
        else fail(v->line, "Invalid material property: " + key); // lua.rs:216
    }
}

// One per-camera record of the scene: its value and the line of the camera entry that has its keys (0: none has). Every
// byte of a record handed out is the loader's, padding included (rtc_projection has some): zeroed here, copied whole there.
template <class T> struct Keyed {
    T value;
    int line;
    Keyed() { reset(); }
    void reset() { std::memset(&value, 0, sizeof value); line = 0; }
};

struct Scene {
    std::vector<rtc_shape> shapes;
    std::vector<rtc_area_light> lights; // every `add: light`, in file order; a point light (`at`) is the degenerate 1x1 area light
    int area_line = 0;                  // line of the first area light (`corner`), 0: the scene has none
    uint64_t samples = 0;               // samples of the lights so far
    rtc_camera camera;
    bool have_camera = false;
    // The camera's records (include/rtc.h), each zeroed without its keys. A later `add: camera` replaces the camera and
    // resets every one of them.
    Keyed<rtc_lens> lens;                   // (the pinhole without lens keys: read_lens)
    Keyed<rtc_projection> proj;
    Keyed<rtc_ao> ao, gather;               // ambient occlusion; the gather pass ("colour bleeding")
    Keyed<rtc_filter> filter;
    Keyed<rtc_adaptive> adaptive;
    bool want_post = false;                 // the entry asked for the post-processing records: only then are their keys read
    Keyed<rtc_tonemap> tonemap;
    Keyed<rtc_bloom> bloom;
    bool want_resize = false;               // the entry asked for the delivered size: only then are the output-* keys read
    Keyed<rtc_resize> resize;
    uint32_t out_w = 0, out_h = 0;          // the delivered size; the camera's own without output-* keys
    std::vector<rtc_motion> motions;        // every shape with a `motion:` key, in file order
    uint32_t shutter_samples = 1;           // the camera's `shutter-samples`
    // Line of the first entry with a motion-blur key (motion / shutter-samples), 0: none. Unlike the records' lines it is NOT
    // reset by a later camera: after a first camera with `shutter-samples: 3` and a second without, every entry but the
    // motion one still refuses the scene, and the motion one returns samples == 1.
    int motion_line = 0;
};

// YAML's spelling of an unbounded value
bool is_inf(const Node *n) { return n && n->kind == Node::Scalar && (n->scalar == ".inf" || n->scalar == "+.inf"); }

double number_or_inf(const Node *n, const char *what) { return is_inf(n) ? std::numeric_limits<double>::infinity() : as_number(n, what); }

// `key`'s value, an integer in lo..hi
uint32_t whole(const Node *n, const std::string &key, uint32_t lo, uint32_t hi) {
    const double v = as_number(n, key.c_str());
    if (!(v >= lo && v <= hi) || v != static_cast<double>(static_cast<uint32_t>(v))) // (NaN fails the first test)
        fail(n->line, key + " must be an integer in " + std::to_string(lo) + ".." + std::to_string(hi));
    return static_cast<uint32_t>(v);
}

uint32_t whole_or(const Node *n, const std::string &key, uint32_t lo, uint32_t hi, uint32_t dflt) { return n ? whole(n, key, lo, hi) : dflt; }

// The readers of an `add: camera` entry, one per key family. read_camera runs them in this order, and the order decides
// which error a document with two mistakes reports. Each resets its record first: a later camera starts afresh.

// projection (include/rtc.h): projection / ortho-width / pano-h-span / pano-v-span; its rays do not read the field of view
void read_projection(const Node &e, Scene &sc) {
    sc.proj.reset();
    const Node *pk = e.get("projection"), *ow = e.get("ortho-width"), *phs = e.get("pano-h-span"), *pvs = e.get("pano-v-span");
    if (!(pk || ow || phs || pvs)) return;
    rtc_projection &proj = sc.proj.value;
    sc.proj.line = e.line;
    if (!pk || pk->kind != Node::Scalar || (pk->scalar != "orthographic" && pk->scalar != "panorama"))
        fail(e.line, "projection must be orthographic or panorama");
    if (pk->scalar == "orthographic") {
        if (phs || pvs) fail(e.line, "pano-h-span / pano-v-span belong to projection: panorama");
        if (!ow) fail(e.line, "an orthographic camera needs an ortho-width");
        proj.kind = RTC_PROJ_ORTHOGRAPHIC;
        proj.width = as_number(ow, "ortho-width");
        if (rtc_projection_validate(&proj) != RTC_OK) fail(ow->line, "ortho-width must be a finite number > 0");
    } else {
        if (ow) fail(e.line, "ortho-width belongs to projection: orthographic");
        proj.kind = RTC_PROJ_PANORAMA;
        proj.h_span = phs ? as_number(phs, "pano-h-span") : 2.0 * M_PI;
        proj.v_span = pvs ? as_number(pvs, "pano-v-span") : M_PI;
        if (rtc_projection_validate(&proj) != RTC_OK) fail(e.line, "pano-h-span must be in (0, 2*pi] and pano-v-span in (0, pi], in radians");
    }
}

// thin lens (include/rtc.h): aperture / focal-distance / lens-usteps / lens-vsteps
void read_lens(const Node &e, Scene &sc) {
    sc.lens.reset();
    rtc_lens &lens = sc.lens.value;
    lens.focal_distance = 1.; // the pinhole (aperture 0, focal distance 1, 1x1) without lens keys
    lens.usteps = lens.vsteps = 1u;
    const Node *ap = e.get("aperture"), *fd = e.get("focal-distance"), *lus = e.get("lens-usteps"), *lvs = e.get("lens-vsteps");
    if (!(ap || fd || lus || lvs)) return;
    sc.lens.line = e.line;
    if (ap) lens.aperture = as_number(ap, "aperture");
    if (ap && !fd) fail(e.line, "a camera with an aperture needs a focal-distance");
    if (fd) lens.focal_distance = as_number(fd, "focal-distance");
    lens.usteps = whole_or(lus, "lens-usteps", 1u, RTC_MAX_LENS_SAMPLES, 1u);
    lens.vsteps = whole_or(lvs, "lens-vsteps", 1u, RTC_MAX_LENS_SAMPLES, 1u);
    if (!(lens.aperture >= 0.) || !std::isfinite(lens.aperture)) fail(e.line, "aperture must be a finite number >= 0");
    if (!(lens.focal_distance > 0.) || !std::isfinite(lens.focal_distance)) fail(e.line, "focal-distance must be a finite number > 0");
    if (rtc_lens_validate(&lens) != RTC_OK)
        fail(e.line, "too many lens samples: lens-usteps x lens-vsteps is at most " + std::to_string(RTC_MAX_LENS_SAMPLES));
    if (sc.proj.line) fail(e.line, "a camera has a lens or a projection, not both");
}

// ambient occlusion and the gather pass (include/rtc.h): PREFIX-radius / PREFIX-usteps / PREFIX-vsteps with PREFIX = ao or
// gather, one rule for both; each asks for a pass and changes no ray of the frame. Like the filter-* and aa-* keys they are
// parsed and range-checked for EVERY entry point, the single-light one included (`ao-usteps` without `ao-radius` fails in
// rtc_scene_load_yaml), and are never a reason to refuse a scene that parses.
void read_fan(const Node &e, const std::string &pre, const char *noun, Keyed<rtc_ao> &out) {
    out.reset();
    const std::string kr = pre + "-radius", ku = pre + "-usteps", kv = pre + "-vsteps";
    const Node *aor = e.get(kr.c_str()), *aou = e.get(ku.c_str()), *aov = e.get(kv.c_str());
    if (!(aor || aou || aov)) return;
    out.line = e.line;
    if (!aor) fail(e.line, ku + " / " + kv + (pre == "ao" ? " need an " : " need a ") + kr);
    out.value.radius = number_or_inf(aor, kr.c_str());
    out.value.usteps = whole_or(aou, ku, 1u, RTC_MAX_AO_SAMPLES, 4u);
    out.value.vsteps = whole_or(aov, kv, 1u, RTC_MAX_AO_SAMPLES, 4u);
    if (!(out.value.radius > 0.)) fail(aor->line, kr + " must be a number > 0 (.inf: unbounded)");
    if (rtc_ao_validate(&out.value) != RTC_OK)
        fail(e.line, std::string("too many ") + noun + " samples: " + ku + " x " + kv + " is at most " + std::to_string(RTC_MAX_AO_SAMPLES));
}

// the edge-aware filter (include/rtc.h): filter-plane-sigma / filter-passes / filter-normal-squarings; asks for a pass too
void read_filter(const Node &e, Scene &sc) {
    sc.filter.reset();
    const Node *fps = e.get("filter-plane-sigma"), *fpa = e.get("filter-passes"), *fns = e.get("filter-normal-squarings");
    if (!(fps || fpa || fns)) return;
    rtc_filter &filter = sc.filter.value;
    sc.filter.line = e.line;
    if (!fps) fail(e.line, "filter-passes / filter-normal-squarings need a filter-plane-sigma");
    filter.plane_sigma = number_or_inf(fps, "filter-plane-sigma");
    if (!(filter.plane_sigma > 0.)) fail(fps->line, "filter-plane-sigma must be a number > 0 (.inf: no plane test)");
    filter.passes = whole_or(fpa, "filter-passes", 1u, RTC_MAX_FILTER_PASSES, RTC_FILTER_DEFAULT_PASSES);
    filter.normal_squarings = whole_or(fns, "filter-normal-squarings", 0u, 8u, RTC_FILTER_DEFAULT_NORMAL_SQUARINGS);
    filter.flags = RTC_FILTER_SAME_OBJECT; // every range of rtc_filter_validate is checked above, key by key
}

// edge-adaptive anti-aliasing (include/rtc.h): aa-threshold / aa-usteps / aa-vsteps, each with a default; asks for a pass
void read_adaptive(const Node &e, Scene &sc) {
    sc.adaptive.reset();
    const Node *aat = e.get("aa-threshold"), *aau = e.get("aa-usteps"), *aav = e.get("aa-vsteps");
    if (!(aat || aau || aav)) return;
    rtc_adaptive &aa = sc.adaptive.value;
    sc.adaptive.line = e.line;
    if (sc.lens.line || sc.proj.line) fail(e.line, "aa-threshold / aa-usteps / aa-vsteps belong to a pinhole camera: not with lens or projection keys");
    aa.threshold = aat ? number_or_inf(aat, "aa-threshold") : RTC_AA_DEFAULT_THRESHOLD;
    if (aa.threshold != aa.threshold) fail(aat->line, "aa-threshold must be a number (.inf: refine nothing)");
    aa.usteps = whole_or(aau, "aa-usteps", 1u, RTC_MAX_AA_SAMPLES, RTC_AA_DEFAULT_STEPS);
    aa.vsteps = whole_or(aav, "aa-vsteps", 1u, RTC_MAX_AA_SAMPLES, RTC_AA_DEFAULT_STEPS);
    if ((uint64_t)aa.usteps * aa.vsteps > RTC_MAX_AA_SAMPLES) // with the checks above: every range of rtc_adaptive_validate
        fail(e.line, "too many anti-aliasing samples: aa-usteps x aa-vsteps is at most " + std::to_string(RTC_MAX_AA_SAMPLES));
}

// exposure, tone mapping and bloom (include/rtc.h): tonemap-* and bloom-*, each with a default. Only the post entry reads
// them: every other entry ignores them, malformed values included (`tonemap-curve: bogus` loads through rtc_scene_load_yaml).
void read_post(const Node &e, Scene &sc) {
    sc.tonemap.reset();
    sc.bloom.reset();
    if (!sc.want_post) return;
    const double inf = std::numeric_limits<double>::infinity();
    const Node *tc = e.get("tonemap-curve"), *te = e.get("tonemap-exposure"), *tk = e.get("tonemap-key"), *tw = e.get("tonemap-white");
    if (tc || te || tk || tw) {
        rtc_tonemap &tm = sc.tonemap.value;
        sc.tonemap.line = e.line;
        if (te && tk) fail(tk->line, "tonemap-key sets the exposure from the frame's mean luminance: not together with tonemap-exposure");
        tm.curve = RTC_TONEMAP_REINHARD;
        if (tc) {
            if (tc->kind != Node::Scalar) fail(tc->line, "tonemap-curve must be linear, reinhard or aces");
            if (tc->scalar == "linear") tm.curve = RTC_TONEMAP_LINEAR;
            else if (tc->scalar == "reinhard") tm.curve = RTC_TONEMAP_REINHARD;
            else if (tc->scalar == "aces") tm.curve = RTC_TONEMAP_ACES;
            else fail(tc->line, "tonemap-curve must be linear, reinhard or aces: " + tc->scalar);
        }
        tm.exposure = tk ? as_number(tk, "tonemap-key") : te ? as_number(te, "tonemap-exposure") : 1.0;
        if (tk) tm.flags |= RTC_TONEMAP_AUTO_EXPOSURE;
        if (!(tm.exposure > 0.0 && tm.exposure < inf))
            fail((tk ? tk : te)->line, std::string(tk ? "tonemap-key" : "tonemap-exposure") + " must be a finite number above 0");
        tm.white = inf;
        if (tw && tw->kind == Node::Scalar && tw->scalar == "auto") {
            tm.flags |= RTC_TONEMAP_AUTO_WHITE;
            tm.white = 1.0; // ignored with the flag; any valid value
        } else if (tw && !is_inf(tw)) {
            tm.white = as_number(tw, "tonemap-white");
            if (!(tm.white > 0.0)) fail(tw->line, "tonemap-white must be a number above 0, .inf or auto");
        }
    }
    const Node *bt = e.get("bloom-threshold"), *bs = e.get("bloom-strength"), *bg = e.get("bloom-sigma"), *br = e.get("bloom-radius");
    if (bt || bs || bg || br) {
        rtc_bloom &bloom = sc.bloom.value;
        sc.bloom.line = e.line;
        bloom.threshold = bt ? as_number(bt, "bloom-threshold") : 1.0;
        bloom.strength = bs ? as_number(bs, "bloom-strength") : 0.5;
        bloom.sigma = bg ? as_number(bg, "bloom-sigma") : 2.0;
        bloom.radius = whole_or(br, "bloom-radius", 1u, RTC_MAX_BLOOM_RADIUS, 6u);
        // with the radius above: every range of rtc_bloom_validate, written out here because this file links with
        // host_math.cpp and host_ppm.cpp alone (without host_post.cpp)
        if (!(bloom.threshold >= 0.0 && bloom.threshold < inf)) fail((bt ? bt : &e)->line, "bloom-threshold must be a finite number of at least 0");
        if (!(bloom.strength >= 0.0 && bloom.strength < inf)) fail((bs ? bs : &e)->line, "bloom-strength must be a finite number of at least 0");
        if (!(bloom.sigma > 0.0 && bloom.sigma < inf) || !((2.0 * bloom.sigma) * bloom.sigma > 0.0))
            fail((bg ? bg : &e)->line, "bloom-sigma must be a finite number above 0");
    }
}

// the delivered size (include/rtc.h): output-width / output-height / output-filter. Only the resize entry reads them: every
// other entry ignores them, malformed values included.
void read_resize(const Node &e, Scene &sc) {
    sc.resize.reset();
    sc.out_w = sc.camera.hsize;
    sc.out_h = sc.camera.vsize;
    if (!sc.want_resize) return;
    const Node *ow = e.get("output-width"), *oh = e.get("output-height"), *of = e.get("output-filter");
    if (!(ow || oh || of)) return;
    sc.resize.line = e.line;
    if (!ow && !oh) fail(of->line, "output-filter needs output-width or output-height");
    // an absent side keeps the frame's aspect, rounded to nearest, at least 1
    auto aspect = [](uint32_t given, uint32_t other_in, uint32_t given_in) {
        const double v = std::floor((static_cast<double>(given) * static_cast<double>(other_in)) / static_cast<double>(given_in) + 0.5);
        return v < 1.0 ? 1u : v > 2147483647.0 ? 2147483647u : static_cast<uint32_t>(v);
    };
    if (ow) sc.out_w = whole(ow, "output-width", 1u, 2147483647u);
    if (oh) sc.out_h = whole(oh, "output-height", 1u, 2147483647u);
    if (!oh) sc.out_h = aspect(sc.out_w, sc.camera.vsize, sc.camera.hsize);
    if (!ow) sc.out_w = aspect(sc.out_h, sc.camera.hsize, sc.camera.vsize);
    sc.resize.value.filter = RTC_RESIZE_LANCZOS3;
    if (of) {
        static const char *const names[] = {"box", "triangle", "catmull-rom", "mitchell", "lanczos3"};
        uint32_t f = 0;
        while (f < 5u && (of->kind != Node::Scalar || of->scalar != names[f])) ++f;
        if (f == 5u) fail(of->line, "output-filter must be box, triangle, catmull-rom, mitchell or lanczos3");
        sc.resize.value.filter = f;
    }
}

// motion blur (include/rtc.h): shutter-samples
void read_shutter(const Node &e, Scene &sc) {
    sc.shutter_samples = whole_or(e.get("shutter-samples"), "shutter-samples", 1u, RTC_MAX_SHUTTER_SAMPLES, 1u);
    if (e.get("shutter-samples") && !sc.motion_line) sc.motion_line = e.line; // (never reset: see Scene)
}

void read_camera(const Node &e, Scene &sc) {
    double from[3], to[3], up[3], view[16];
    as_triple(e.get("from"), "from", from);
    as_triple(e.get("to"), "to", to);
    as_triple(e.get("up"), "up", up);
    const double w = as_number(e.get("width"), "width"), h = as_number(e.get("height"), "height");
    if (w < 1 || h < 1 || w > 2147483647. || h > 2147483647. || w != static_cast<double>(static_cast<uint32_t>(w)) ||
        h != static_cast<double>(static_cast<uint32_t>(h)))
        fail(e.line, "camera width/height must be positive integers"); // lua.rs:159-170
    rtc_view_transform(from, to, up, view);
    read_projection(e, sc);
    const double fov = (sc.proj.line && !e.get("field-of-view")) ? M_PI / 2.0 : as_number(e.get("field-of-view"), "field-of-view");
    const rtc_status st = rtc_camera_init(static_cast<uint32_t>(w), static_cast<uint32_t>(h), fov, view, &sc.camera);
    if (st != RTC_OK) fail(e.line, std::string("camera: ") + rtc_strerror(st));
    if (const Node *s = e.get("samples")) {
        const double sv = as_number(s, "samples");
        if (sv < 0 || sv > 255 || sv != static_cast<double>(static_cast<uint32_t>(sv))) fail(s->line, "samples out of bounds"); // lua.rs:172-183
        sc.camera.samples = static_cast<uint32_t>(sv);
    }
    read_lens(e, sc);
    read_fan(e, "ao", "ambient-occlusion", sc.ao);
    read_fan(e, "gather", "gather", sc.gather);
    read_filter(e, sc);
    read_adaptive(e, sc);
    read_post(e, sc);
    read_resize(e, sc);
    read_shutter(e, sc);
    sc.have_camera = true;
}

void read_light(const Node &e, Scene &sc) {
    rtc_area_light a;
    std::memset(&a, 0, sizeof a);
    a.usteps = a.vsteps = 1u;
    if (e.get("corner")) { // the book's area light: corner / uvec / vvec / usteps / vsteps / intensity
        if (e.get("at")) fail(e.line, "a light has either 'at' (point light) or 'corner' (area light), not both");
        as_triple(e.get("corner"), "corner", a.corner);
        as_triple(e.get("uvec"), "uvec", a.uvec);
        as_triple(e.get("vvec"), "vvec", a.vvec);
        a.usteps = whole(e.get("usteps"), "usteps", 1u, RTC_MAX_LIGHT_SAMPLES); // (both keys are required)
        a.vsteps = whole(e.get("vsteps"), "vsteps", 1u, RTC_MAX_LIGHT_SAMPLES);
        if (const Node *j = e.get("jitter")) {
            if (j->kind != Node::Scalar || (j->scalar != "false" && j->scalar != "true")) fail(j->line, "jitter must be true or false");
            if (j->scalar == "true") fail(j->line, "jitter is not supported: area light samples sit at the cell centres (jitter: false)");
        }
    } else {
        as_triple(e.get("at"), "at", a.corner);
    }
    as_triple(e.get("intensity"), "intensity", a.intensity);
    // a scene of point lights holds RTC_MAX_LIGHTS of them, as ever; one with an area light RTC_MAX_LIGHT_SAMPLES samples
    if (!sc.area_line && sc.lights.size() == RTC_MAX_LIGHTS) fail(e.line, "too many lights: a scene holds at most " + std::to_string(RTC_MAX_LIGHTS));
    sc.samples += static_cast<uint64_t>(a.usteps) * a.vsteps;
    if (sc.samples > RTC_MAX_LIGHT_SAMPLES)
        fail(e.line, "too many light samples: a scene holds at most " + std::to_string(RTC_MAX_LIGHT_SAMPLES) + " (usteps x vsteps, summed over its lights)");
    sc.lights.push_back(a); // (the reference uses lights[1] only, lua.rs:148-150: the single-light entries return that one)
}

void read_shape(const Node &e, const std::string &what, const Defs &defs, Scene &sc) {
    const uint32_t kind = what == "sphere" ? RTC_SPHERE : what == "plane" ? RTC_PLANE : RTC_CUBE;
    double xf[16];
    rtc_matrix_identity(xf);
    build_transform(defs, e.get("transform"), xf);
    rtc_material mat;
    build_material(defs, e.get("material"), mat);
    rtc_shape s;
    const rtc_status st = rtc_shape_init(kind, xf, &mat, &s);
    if (st != RTC_OK) fail(e.line, what + ": " + rtc_strerror(st));
    s.world_id = static_cast<uint32_t>(sc.shapes.size()) + 1; // World::add_shape shape.rs:661-667
    if (const Node *mv = e.get("motion")) { // motion blur: the transform at the shutter's close = this list on top of the shape's
        rtc_motion m;
        std::memset(&m, 0, sizeof m);
        m.shape = static_cast<uint32_t>(sc.shapes.size());
        std::memcpy(m.transform_open, xf, sizeof xf);
        std::memcpy(m.transform_close, xf, sizeof xf);
        build_transform(defs, mv, m.transform_close);
        sc.motions.push_back(m);
        if (!sc.motion_line) sc.motion_line = e.line;
    }
    sc.shapes.push_back(s);
}

void interpret(const Node &root, Scene &sc) {
    if (root.kind != Node::Seq) fail(root.line, "scene must be a sequence of entries");
    Defs defs;
    for (const auto &ep : root.seq) // (read_light needs to know of an area light before it meets it)
        if (ep->kind == Node::Map && !sc.area_line && ep->get("add") && ep->get("add")->kind == Node::Scalar && ep->get("add")->scalar == "light" &&
            ep->get("corner"))
            sc.area_line = ep->line;
    for (const auto &ep : root.seq) {
        const Node &e = *ep;
        if (e.kind != Node::Map) fail(e.line, "scene entry must be a map");
        if (const Node *d = e.get("define")) {
            const Node *val = e.get("value");
            if (!val || d->kind != Node::Scalar) fail(e.line, "define needs a name and a value");
            NodeP stored;
            for (const auto &kv : e.map) if (kv.first == "value") stored = kv.second;
            if (const Node *ext = e.get("extend")) { // Jamis's format: extend sits beside value
                auto merged = std::make_shared<Node>(*stored);
                if (merged->kind != Node::Map) fail(e.line, "extend needs a map value");
                auto extn = std::make_shared<Node>(*ext);
                merged->map.insert(merged->map.begin(), {"extend", extn});
                stored = merged;
            }
            defs.values[d->scalar] = stored;
            continue;
        }
        const Node *add = e.get("add");
        if (!add || add->kind != Node::Scalar) fail(e.line, "entry needs 'add' or 'define'");
        const std::string &what = add->scalar;
        if (what == "camera") read_camera(e, sc);
        else if (what == "light") read_light(e, sc);
        else if (what == "sphere" || what == "plane" || what == "cube") read_shape(e, what, defs, sc);
        else fail(add->line, "Invalid shape type: " + what); // lua.rs:322-326
    }
    if (sc.lights.empty()) fail(root.line, "scene has no light");
    if (!sc.have_camera) fail(root.line, "scene has no camera");
}

void set_err(char *errbuf, size_t len, const std::string &msg) {
    if (errbuf && len) {
        std::snprintf(errbuf, len, "%s", msg.c_str());
    }
}

// One optional record of an entry point: where the record goes, and where "the camera has its keys" goes.
template <class T> struct Slot {
    T *record = nullptr;
    uint32_t *has = nullptr;
    bool half() const { return !record != !has; }
    void hand_out(const Keyed<T> &k) const {
        if (!record) return;
        std::memcpy(record, &k.value, sizeof(T));
        *has = k.line ? 1u : 0u;
    }
};

// What an entry point wants of a document beside shapes and camera. Every entry fills the fields it has, by name; what it
// leaves alone is not wanted.
struct Wanted {
    // the lights: exactly one of `point_lights` (a scene with an area light is refused) and `area_lights` (every light as an
    // rtc_area_light); first_only: the single-light entry's form, lights[1] alone, however many the scene has
    rtc_light *point_lights = nullptr;
    rtc_area_light *area_lights = nullptr;
    uint32_t lights_cap = 0;
    uint32_t *n_lights_out = nullptr;
    bool first_only = false;
    Slot<rtc_lens> lens;
    Slot<rtc_projection> projection;
    Slot<rtc_ao> ao, gather;
    Slot<rtc_filter> filter;
    Slot<rtc_adaptive> adaptive;
    Slot<rtc_tonemap> tonemap; // tonemap and bloom come together or not at all
    Slot<rtc_bloom> bloom;
    Slot<rtc_resize> resize;   // with the delivered size
    uint32_t *out_w = nullptr, *out_h = nullptr;
    rtc_motion **motions_out = nullptr; // motion blur: all three or none (the motion entry checks that)
    uint32_t *n_motions_out = nullptr, *samples_out = nullptr;
};

rtc_status load_yaml(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                     const Wanted &want) {
    // An RTC_ERR_ARG from these checks writes nothing at all. A record / has pair given half is one.
    if (!text || !shapes_out || !n_out || (!want.point_lights && !want.area_lights) || !want.lights_cap || !want.n_lights_out || !camera_out)
        return RTC_ERR_ARG;
    if (want.lens.half() || want.projection.half() || want.ao.half() || want.gather.half() || want.filter.half() || want.adaptive.half() ||
        want.tonemap.half() || want.bloom.half() || want.resize.half() || !want.tonemap.record != !want.bloom.record)
        return RTC_ERR_ARG;
    *shapes_out = nullptr;
    *n_out = 0;
    *want.n_lights_out = 0;
    if (want.motions_out) {
        *want.motions_out = nullptr;
        *want.n_motions_out = 0;
        *want.samples_out = 1u;
    }
    try {
        Parser p;
        p.lines = split_lines(text);
        if (p.lines.empty()) fail(0, "empty document");
        NodeP root = p.parse_block(p.lines[0].indent);
        if (p.pos != p.lines.size()) fail(p.lines[p.pos].number, "unexpected content");
        Scene sc;
        sc.want_post = want.tonemap.record != nullptr;
        sc.want_resize = want.resize.record != nullptr;
        interpret(*root, sc);
        // Refusals, in this order, each naming the entry to use and the line of the entry that has the keys; then a
        // lights_cap too small (RTC_ERR_ARG, no message; the single-light entry returns the first light whatever the
        // count); only then allocations.
        if (sc.area_line && !want.area_lights) fail(sc.area_line, "the scene has an area light: load it with rtc_scene_load_yaml_area_lights");
        if (sc.lens.line && !want.lens.record) fail(sc.lens.line, "the scene's camera has a lens: load it with rtc_scene_load_yaml_lens");
        if (sc.proj.line && !want.projection.record)
            fail(sc.proj.line, "the scene's camera has a projection (projection / ortho-width / pano-h-span / pano-v-span): load it with rtc_scene_load_yaml_projection");
        if (sc.motion_line && !want.motions_out) fail(sc.motion_line, "the scene has motion blur (motion / shutter-samples): load it with rtc_scene_load_yaml_motion");
        if (!want.first_only && sc.lights.size() > want.lights_cap) return RTC_ERR_ARG;
        rtc_motion *marr = nullptr;
        if (want.motions_out) {
            marr = static_cast<rtc_motion *>(std::malloc(sizeof(rtc_motion) * (sc.motions.empty() ? 1 : sc.motions.size())));
            if (!marr) return RTC_ERR_NOMEM;
            if (!sc.motions.empty()) std::memcpy(marr, sc.motions.data(), sizeof(rtc_motion) * sc.motions.size());
        }
        const size_t bytes = sizeof(rtc_shape) * (sc.shapes.empty() ? 1 : sc.shapes.size());
        rtc_shape *arr = static_cast<rtc_shape *>(std::malloc(bytes));
        if (!arr) { std::free(marr); return RTC_ERR_NOMEM; }
        if (want.motions_out) {
            *want.motions_out = marr;
            *want.n_motions_out = static_cast<uint32_t>(sc.motions.size());
            *want.samples_out = sc.shutter_samples;
        }
        if (!sc.shapes.empty()) std::memcpy(arr, sc.shapes.data(), sizeof(rtc_shape) * sc.shapes.size());
        *shapes_out = arr;
        *n_out = static_cast<uint32_t>(sc.shapes.size());
        const uint32_t nl = want.first_only ? 1u : static_cast<uint32_t>(sc.lights.size());
        for (uint32_t i = 0; i < nl; ++i) {
            if (want.area_lights) { want.area_lights[i] = sc.lights[i]; continue; }
            for (int k = 0; k < 3; ++k) { // a point light: corner = position, 1x1
                want.point_lights[i].position[k] = sc.lights[i].corner[k];
                want.point_lights[i].intensity[k] = sc.lights[i].intensity[k];
            }
        }
        *want.n_lights_out = nl;
        *camera_out = sc.camera;
        want.lens.hand_out(sc.lens);
        want.projection.hand_out(sc.proj);
        want.ao.hand_out(sc.ao);
        want.gather.hand_out(sc.gather);
        want.filter.hand_out(sc.filter);
        want.adaptive.hand_out(sc.adaptive);
        want.tonemap.hand_out(sc.tonemap);
        want.bloom.hand_out(sc.bloom);
        want.resize.hand_out(sc.resize);
        if (want.resize.record) {
            *want.out_w = sc.out_w;
            *want.out_h = sc.out_h;
        }
        return RTC_OK;
    } catch (const ParseError &e) {
        set_err(errbuf, errbuf_len, e.what());
        return RTC_ERR_PARSE;
    } catch (const std::bad_alloc &) {
        return RTC_ERR_NOMEM;
    } catch (...) {
        set_err(errbuf, errbuf_len, "internal error");
        return RTC_ERR_PARSE;
    }
}

// The area-light entries' common part of the record.
Wanted area_lights(rtc_area_light *lights_out, uint32_t lights_cap, uint32_t *n_lights_out) {
    Wanted w;
    w.area_lights = lights_out;
    w.lights_cap = lights_cap;
    w.n_lights_out = n_lights_out;
    return w;
}

rtc_status read_file(const char *path, std::string &text, char *errbuf, size_t errbuf_len) {
    if (!path) return RTC_ERR_ARG;
    std::FILE *f = std::fopen(path, "rb");
    if (!f) { set_err(errbuf, errbuf_len, std::string("cannot open ") + path); return RTC_ERR_IO; }
    char buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    std::fclose(f);
    return RTC_OK;
}

// The `_file` entries: the file's text and `rest` through `entry`, the text entry. The file is read before the entry's own
// null checks: a null path is RTC_ERR_ARG, an unopenable one RTC_ERR_IO with `cannot open PATH` in errbuf.
template <class... A>
rtc_status from_file(rtc_status (*entry)(const char *, A...), char *errbuf, size_t errbuf_len, const char *path, A... rest) {
    std::string text;
    const rtc_status st = read_file(path, text, errbuf, errbuf_len);
    return st != RTC_OK ? st : entry(text.c_str(), rest...);
}

} // namespace

extern "C" {

rtc_status rtc_scene_load_yaml(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_light *light_out, rtc_camera *camera_out, char *errbuf,
                               size_t errbuf_len) {
    uint32_t one = 0u;
    Wanted w;
    w.point_lights = light_out;
    w.lights_cap = 1u;
    w.n_lights_out = &one;
    w.first_only = true;
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_lights(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_light *lights_out, uint32_t lights_cap,
                                      uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len) {
    Wanted w;
    w.point_lights = lights_out;
    w.lights_cap = lights_cap;
    w.n_lights_out = n_lights_out;
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_area_lights(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                           uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len) {
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, area_lights(lights_out, lights_cap, n_lights_out));
}

rtc_status rtc_scene_load_yaml_lens(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                    uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                    uint32_t *has_lens_out) {
    if (!lens_out || !has_lens_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.lens = {lens_out, has_lens_out};
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_motion(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                      uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                      uint32_t *has_lens_out, rtc_motion **motions_out, uint32_t *n_motions_out, uint32_t *samples_out) {
    if (!lens_out || !has_lens_out || !motions_out || !n_motions_out || !samples_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.lens = {lens_out, has_lens_out};
    w.motions_out = motions_out;
    w.n_motions_out = n_motions_out;
    w.samples_out = samples_out;
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_projection(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                          uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                          uint32_t *has_lens_out, rtc_projection *proj_out, uint32_t *has_projection_out) {
    if (!lens_out || !has_lens_out || !proj_out || !has_projection_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.lens = {lens_out, has_lens_out};
    w.projection = {proj_out, has_projection_out};
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_ao(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                  uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                  uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out) {
    if (!lens_out || !has_lens_out || !ao_out || !has_ao_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.lens = {lens_out, has_lens_out};
    w.ao = {ao_out, has_ao_out};
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_gather(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                      uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                      uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out, rtc_ao *gather_out, uint32_t *has_gather_out) {
    if (!lens_out || !has_lens_out || !ao_out || !has_ao_out || !gather_out || !has_gather_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.lens = {lens_out, has_lens_out};
    w.ao = {ao_out, has_ao_out};
    w.gather = {gather_out, has_gather_out};
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_filter(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                      uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                      uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out, rtc_ao *gather_out, uint32_t *has_gather_out,
                                      rtc_filter *filter_out, uint32_t *has_filter_out) {
    if (!lens_out || !has_lens_out || !ao_out || !has_ao_out || !gather_out || !has_gather_out || !filter_out || !has_filter_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.lens = {lens_out, has_lens_out};
    w.ao = {ao_out, has_ao_out};
    w.gather = {gather_out, has_gather_out};
    w.filter = {filter_out, has_filter_out};
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_projection_passes(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out,
                                                 uint32_t lights_cap, uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                                 rtc_lens *lens_out, uint32_t *has_lens_out, rtc_projection *proj_out, uint32_t *has_projection_out,
                                                 rtc_ao *ao_out, uint32_t *has_ao_out, rtc_ao *gather_out, uint32_t *has_gather_out,
                                                 rtc_filter *filter_out, uint32_t *has_filter_out) {
    if (!lens_out || !has_lens_out || !proj_out || !has_projection_out || !ao_out || !has_ao_out || !gather_out || !has_gather_out || !filter_out ||
        !has_filter_out)
        return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.lens = {lens_out, has_lens_out};
    w.projection = {proj_out, has_projection_out};
    w.ao = {ao_out, has_ao_out};
    w.gather = {gather_out, has_gather_out};
    w.filter = {filter_out, has_filter_out};
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_adaptive(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                        uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_adaptive *adaptive_out,
                                        uint32_t *has_adaptive_out) {
    if (!adaptive_out || !has_adaptive_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.adaptive = {adaptive_out, has_adaptive_out};
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_post(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                    uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_tonemap *tonemap_out,
                                    uint32_t *has_tonemap_out, rtc_bloom *bloom_out, uint32_t *has_bloom_out) {
    if (!tonemap_out || !has_tonemap_out || !bloom_out || !has_bloom_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.tonemap = {tonemap_out, has_tonemap_out};
    w.bloom = {bloom_out, has_bloom_out};
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_resize(const char *text, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                      uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                      uint32_t *has_lens_out, rtc_projection *proj_out, uint32_t *has_proj_out, rtc_resize *resize_out,
                                      uint32_t *out_w, uint32_t *out_h, uint32_t *has_resize_out) {
    if (!lens_out || !has_lens_out || !proj_out || !has_proj_out || !resize_out || !out_w || !out_h || !has_resize_out) return RTC_ERR_ARG;
    Wanted w = area_lights(lights_out, lights_cap, n_lights_out);
    w.lens = {lens_out, has_lens_out};
    w.projection = {proj_out, has_proj_out};
    w.resize = {resize_out, has_resize_out};
    w.out_w = out_w;
    w.out_h = out_h;
    return load_yaml(text, shapes_out, n_out, camera_out, errbuf, errbuf_len, w);
}

rtc_status rtc_scene_load_yaml_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_light *light_out, rtc_camera *camera_out,
                                    char *errbuf, size_t errbuf_len) {
    return from_file(rtc_scene_load_yaml, errbuf, errbuf_len, path, shapes_out, n_out, light_out, camera_out, errbuf, errbuf_len);
}

rtc_status rtc_scene_load_yaml_lights_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_light *lights_out, uint32_t lights_cap,
                                           uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len) {
    return from_file(rtc_scene_load_yaml_lights, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out,
                     errbuf, errbuf_len);
}

rtc_status rtc_scene_load_yaml_area_lights_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out,
                                                uint32_t lights_cap, uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len) {
    return from_file(rtc_scene_load_yaml_area_lights, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out,
                     errbuf, errbuf_len);
}

rtc_status rtc_scene_load_yaml_lens_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                         uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                         uint32_t *has_lens_out) {
    return from_file(rtc_scene_load_yaml_lens, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out, errbuf,
                     errbuf_len, lens_out, has_lens_out);
}

rtc_status rtc_scene_load_yaml_motion_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                           uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                           uint32_t *has_lens_out, rtc_motion **motions_out, uint32_t *n_motions_out, uint32_t *samples_out) {
    return from_file(rtc_scene_load_yaml_motion, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out,
                     errbuf, errbuf_len, lens_out, has_lens_out, motions_out, n_motions_out, samples_out);
}

rtc_status rtc_scene_load_yaml_projection_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out,
                                               uint32_t lights_cap, uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                               rtc_lens *lens_out, uint32_t *has_lens_out, rtc_projection *proj_out, uint32_t *has_projection_out) {
    return from_file(rtc_scene_load_yaml_projection, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out,
                     errbuf, errbuf_len, lens_out, has_lens_out, proj_out, has_projection_out);
}

rtc_status rtc_scene_load_yaml_ao_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                       uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                       uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out) {
    return from_file(rtc_scene_load_yaml_ao, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out, errbuf,
                     errbuf_len, lens_out, has_lens_out, ao_out, has_ao_out);
}

rtc_status rtc_scene_load_yaml_gather_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                           uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                           uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out, rtc_ao *gather_out, uint32_t *has_gather_out) {
    return from_file(rtc_scene_load_yaml_gather, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out,
                     errbuf, errbuf_len, lens_out, has_lens_out, ao_out, has_ao_out, gather_out, has_gather_out);
}

rtc_status rtc_scene_load_yaml_filter_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                           uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                           uint32_t *has_lens_out, rtc_ao *ao_out, uint32_t *has_ao_out, rtc_ao *gather_out, uint32_t *has_gather_out,
                                           rtc_filter *filter_out, uint32_t *has_filter_out) {
    return from_file(rtc_scene_load_yaml_filter, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out,
                     errbuf, errbuf_len, lens_out, has_lens_out, ao_out, has_ao_out, gather_out, has_gather_out, filter_out, has_filter_out);
}

rtc_status rtc_scene_load_yaml_projection_passes_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out,
                                                      uint32_t lights_cap, uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf,
                                                      size_t errbuf_len, rtc_lens *lens_out, uint32_t *has_lens_out, rtc_projection *proj_out,
                                                      uint32_t *has_projection_out, rtc_ao *ao_out, uint32_t *has_ao_out, rtc_ao *gather_out,
                                                      uint32_t *has_gather_out, rtc_filter *filter_out, uint32_t *has_filter_out) {
    return from_file(rtc_scene_load_yaml_projection_passes, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out,
                     camera_out, errbuf, errbuf_len, lens_out, has_lens_out, proj_out, has_projection_out, ao_out, has_ao_out, gather_out,
                     has_gather_out, filter_out, has_filter_out);
}

rtc_status rtc_scene_load_yaml_adaptive_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out,
                                             uint32_t lights_cap, uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len,
                                             rtc_adaptive *adaptive_out, uint32_t *has_adaptive_out) {
    return from_file(rtc_scene_load_yaml_adaptive, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out,
                     errbuf, errbuf_len, adaptive_out, has_adaptive_out);
}

rtc_status rtc_scene_load_yaml_post_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                         uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_tonemap *tonemap_out,
                                         uint32_t *has_tonemap_out, rtc_bloom *bloom_out, uint32_t *has_bloom_out) {
    return from_file(rtc_scene_load_yaml_post, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out, errbuf,
                     errbuf_len, tonemap_out, has_tonemap_out, bloom_out, has_bloom_out);
}

rtc_status rtc_scene_load_yaml_resize_file(const char *path, rtc_shape **shapes_out, uint32_t *n_out, rtc_area_light *lights_out, uint32_t lights_cap,
                                           uint32_t *n_lights_out, rtc_camera *camera_out, char *errbuf, size_t errbuf_len, rtc_lens *lens_out,
                                           uint32_t *has_lens_out, rtc_projection *proj_out, uint32_t *has_proj_out, rtc_resize *resize_out,
                                           uint32_t *out_w, uint32_t *out_h, uint32_t *has_resize_out) {
    return from_file(rtc_scene_load_yaml_resize, errbuf, errbuf_len, path, shapes_out, n_out, lights_out, lights_cap, n_lights_out, camera_out,
                     errbuf, errbuf_len, lens_out, has_lens_out, proj_out, has_proj_out, resize_out, out_w, out_h, has_resize_out);
}

} // extern "C"
