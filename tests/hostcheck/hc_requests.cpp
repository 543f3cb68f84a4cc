// hc_requests.cpp -- host check, single thread (AddressSanitizer + UndefinedBehaviorSanitizer): every kind of request the suite's generators know, through every
// host path of the C ABI, on the stub runtime (stub_hip.cpp).  Launches are recorded, never executed: this is about what the host computes, allocates, copies,
// caches and returns.
// usage: hc_requests <request file>   -- written by tests/test_hostcheck_cpu.py from tests/dispatch_grid.py, tests/tile_fuzz.py, tests/remap_util.py and
// tests/mesh_util.py, one request per line (the formats are parse_* below; floats travel as the eight hex digits of their bits)
//   plain    tsvpp_describe, tsvpp_convert_batch twice (the second is the replay hit), once more with the outputs moved by 4 bytes, tsvpp_convert_table over a run
//            inside a table of 131 entries, tsvpp_prepare_batch, tsvpp_trim -- one context for all of them, created under TSVPP_DEBUG_KNOBS=1 on the stub's SECOND
//            device while the thread's current device is the first
//   tile     the describe and the convert call of the ROI / AREA-ROI / letterbox / warp / perspective families (tensor forms included) for the same arguments
//   remap, mesh   the same with map / mesh buffers behind the stub's "device" pointers, and the host-side helpers on the host copies
// then the helper entry points on valid inputs and on every refusal the header names, the source limit (plane spans one byte under TSVPP_SOURCE_SPAN_LIMIT and at
// it through every describe / convert pair: source_spans), and last a subset of the requests with the n-th allocation failing,
// n = 1, 2, 3 ... until the call succeeds.
// Exit status 0 only without a failed assertion, a stub violation, or anything the stub still holds at the end.
#include <cmath>
#include <fstream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "hc_common.h"

namespace {

struct Tokens {
    std::vector<std::string> t;
    size_t at = 0;
    std::string line;
    explicit Tokens(const std::string &l) : line(l) {
        std::istringstream in(l);
        std::string w;
        while (in >> w) t.push_back(w);
    }
    const std::string &word() {
        static const std::string none;
        if (at >= t.size()) {
            std::fprintf(stderr, "hc_requests: line too short: %.80s\n", line.c_str());
            std::exit(3);
        }
        return t[at++];
    }
    int i() { return (int)std::strtol(word().c_str(), nullptr, 10); }
    float f() {
        const uint32_t bits = (uint32_t)std::strtoul(word().c_str(), nullptr, 16);
        float v;
        std::memcpy(&v, &bits, 4);
        return v;
    }
};

struct Env {
    tsvpp_ctx *ctx = nullptr; // on device 1
    void *stream = nullptr;
    uint8_t *y = nullptr, *uv = nullptr, *out = nullptr; // every frame of a plain request shares them
};

struct Plain {
    int w, h, py, puv, n, aligned;
    tsvpp_params p;
};
Plain parse_plain(Tokens &k) { // plain w h pitch_y pitch_uv crop_left crop_top crop_right crop_bottom dst_w dst_h resize_type fourcc planes normalization n aligned
    Plain r = {};
    r.w = k.i(), r.h = k.i(), r.py = k.i(), r.puv = k.i();
    r.p.crop_left = k.i(), r.p.crop_top = k.i(), r.p.crop_right = k.i(), r.p.crop_bottom = k.i();
    r.p.dst_width = k.i(), r.p.dst_height = k.i(), r.p.resize_type = k.i(), r.p.fourcc = k.i(), r.p.planes = k.i(), r.p.normalization = k.i();
    r.n = k.i(), r.aligned = k.i();
    return r;
}

std::string last_launch() {
    char buf[512];
    return tsvpp_debug_last_launch(buf, sizeof(buf)) == TSVPP_OK ? buf : "";
}
std::string family_of(const std::string &line) {
    const std::string k = hc::value_of(line, "kernel");
    return k.substr(0, k.find('<'));
}

std::vector<Plain> g_plain; // kept for the allocation-failure part

void run_plain(const Env &e, const Plain &r, const char *text) {
    char desc[512] = "", desc0[512] = "";
    const int ds = tsvpp_describe(&r.p, r.w, r.h, r.py, r.puv, r.n, r.aligned, desc, sizeof(desc));
    HC_CHECK(ds == TSVPP_OK, "describe refuses a request of the grid (%d): %s", ds, text);
    if (ds != TSVPP_OK) return;
    HC_CHECK(tsvpp_describe(&r.p, r.w, r.h, r.py, r.puv, r.n, 0, desc0, sizeof(desc0)) == TSVPP_OK, "describe, outputs not aligned: %s", text);
    std::vector<tsvpp_nv12> in((size_t)r.n, tsvpp_nv12{ e.y, e.uv, r.py, r.puv, r.w, r.h });
    std::vector<void *> outs((size_t)r.n, e.out + (r.aligned ? 0 : 4));
    const bool two_pass = !hc::value_of(desc, "pass2").empty();

    // 2. the conversion; 3. the same call again: the replay hit
    hc_stub_clear_launches();
    const int s1 = tsvpp_convert_batch(e.ctx, r.n, in.data(), &r.p, outs.data(), e.stream);
    const size_t l1 = hc_stub_launch_count();
    const HcLaunch first = l1 ? *hc_stub_launch(0) : HcLaunch{};
    const std::string line1 = last_launch();
    HC_CHECK(s1 == TSVPP_OK, "convert_batch: %d (%s): %s", s1, tsvpp_strerror(s1), text);
    HC_CHECK(hc::current_device() == 0, "convert_batch left the thread on device %d", hc::current_device());
    if (s1 != TSVPP_OK) return;
    hc_stub_clear_launches();
    const int s2 = tsvpp_convert_batch(e.ctx, r.n, in.data(), &r.p, outs.data(), e.stream);
    const size_t l2 = hc_stub_launch_count();
    const std::string line2 = last_launch();
    HC_CHECK(s2 == TSVPP_OK && l2 == l1, "the second call: status %d, %zu launches after %zu: %s", s2, l2, l1, text);
    HC_CHECK(line2 == line1 && !line1.empty(), "the replayed call reports\n    %s\n  the first call\n    %s", line2.c_str(), line1.c_str());
    if (l1 == 1 && l2 == 1) {
        const HcLaunch &again = *hc_stub_launch(0);
        HC_CHECK(again.fn == first.fn && again.lds == first.lds && std::memcmp(again.grid, first.grid, sizeof(first.grid)) == 0 &&
                     std::memcmp(again.block, first.block, sizeof(first.block)) == 0 && again.any_order == first.any_order && again.stream == first.stream,
                 "the replayed launch is not the first one: %s", text);
    }
    // the launch that went out is the described one
    HC_CHECK(hc::signature_of(line1) == hc::signature_of(desc), "launched\n    %s\n  described\n    %s", line1.c_str(), desc);
    HC_CHECK(hc::number_of(line1, "frames") == (r.n < TSVPP_MAX_BATCH ? r.n : TSVPP_MAX_BATCH), "frames= of %s", line1.c_str());
    if (l1 >= 1 && !(two_pass && hc::value_of(desc, "kernel") == "(none)")) {
        HC_CHECK(hc::number_of(line1, "grid") == hc::number_of(desc, "grid") && (long)first.grid[0] == hc::number_of(desc, "grid"),
                 "grid: launched %u, reported %ld, described %ld: %s", first.grid[0], hc::number_of(line1, "grid"), hc::number_of(desc, "grid"), text);
        // include/tsvpp.h: the live line's lds= is the dynamic LDS alone, describe adds the static exchange slabs of some kernels
        HC_CHECK((long)first.lds == hc::number_of(line1, "lds") && hc::number_of(line1, "lds") <= hc::number_of(desc, "lds"),
                 "lds: launched %zu, reported %ld, described %ld: %s", first.lds, hc::number_of(line1, "lds"), hc::number_of(desc, "lds"), text);
    }

    // 4. outputs moved by 4 bytes: the other alignment class (or the same one again, for a request that began there)
    std::vector<void *> moved((size_t)r.n, e.out + (r.aligned ? 4 : 8));
    const int s4 = tsvpp_convert_batch(e.ctx, r.n, in.data(), &r.p, moved.data(), e.stream);
    const std::string line4 = last_launch();
    HC_CHECK(s4 == TSVPP_OK, "outputs moved by 4 bytes: %d: %s", s4, text);
    HC_CHECK(hc::signature_of(line4) == hc::signature_of(desc0), "outputs moved by 4 bytes: launched\n    %s\n  described\n    %s", line4.c_str(), desc0);

    // 5. out of a frame table: a run that starts inside a table of 131 entries
    tsvpp_table *tab = nullptr;
    HC_CHECK(tsvpp_table_create(e.ctx, 131, &tab) == TSVPP_OK && tab, "table_create");
    if (tab) {
        HC_CHECK(tsvpp_table_set(tab, 3, r.n, in.data(), outs.data(), e.stream) == TSVPP_OK, "table_set of entries 3 .. %d", 3 + r.n);
        hc_stub_clear_launches();
        const int s5 = tsvpp_convert_table(e.ctx, tab, 3, r.n, &r.p, e.stream);
        const std::string line5 = last_launch();
        HC_CHECK(s5 == TSVPP_OK && hc_stub_launch_count() >= (two_pass && l1 == 1 ? 1u : (unsigned)(l1 > 0)), "convert_table: %d: %s", s5, text);
        HC_CHECK(family_of(line5) == family_of(desc), "convert_table launched\n    %s\n  described\n    %s", line5.c_str(), desc);
        HC_CHECK(tsvpp_convert_table(e.ctx, tab, 1, 3, &r.p, e.stream) == TSVPP_ERROR, "a run with entries that were never set is TSVPP_ERROR");
        HC_CHECK(tsvpp_convert_table(e.ctx, tab, 130, 2, &r.p, e.stream) == TSVPP_ERROR, "a run past the table's end is TSVPP_ERROR");
        tsvpp_table_destroy(tab);
    }

    // 6. prepare and trim
    HC_CHECK(tsvpp_prepare_batch(e.ctx, &r.p, r.w, r.h, r.n, e.stream) == TSVPP_OK, "prepare_batch: %s", text);
    size_t released = 0;
    HC_CHECK(tsvpp_trim(e.ctx, &released) == TSVPP_OK, "trim");
    HC_CHECK(hc::current_device() == 0, "the thread ends on device %d", hc::current_device());
}

// ---- the tile-pipeline families ------------------------------------------------------------------------------------------------------------------------------
struct DevFrames {
    std::vector<uint8_t *> blocks;
    std::vector<tsvpp_nv12> frames;
    void add(int w, int h, int py, int puv, int off_y, int off_uv) {
        uint8_t *y = hc::dev_alloc((size_t)off_y + (size_t)h * py + 16), *uv = hc::dev_alloc((size_t)off_uv + (size_t)(h / 2) * puv + 16);
        blocks.push_back(y);
        blocks.push_back(uv);
        frames.push_back(tsvpp_nv12{ y + off_y, uv + off_uv, py, puv, w, h });
    }
    ~DevFrames() {
        for (uint8_t *b : blocks) (void)hipFree(b);
    }
};

// describe's answer against what the stub saw
void check_tile_launches(int ds, int cs, const char *desc, const char *text) {
    HC_CHECK(ds == cs, "describe answers %d, convert %d: %s", ds, cs, text);
    if (ds != TSVPP_OK || cs != TSVPP_OK) return;
    const std::string d = desc;
    HC_CHECK((long)hc_stub_launch_count() == hc::number_of(d, "launches"), "%zu launches, described %s", hc_stub_launch_count(), desc);
    if (hc_stub_launch_count() == 0) return;
    const HcLaunch &l = *hc_stub_launch(0);
    HC_CHECK((long)l.grid[0] == hc::number_of(d, "grid"), "the first launch has a grid of %u, described %s", l.grid[0], desc);
    // lds= of the describe calls is the workgroup's LDS: the launch's dynamic bytes plus the static exchange slab of the kernel's store side, which is a property of
    // the kernel instance -- so the difference is one number per kernel name, whatever the request
    static std::map<std::string, long> slab;
    const long extra = hc::number_of(d, "lds") - (long)l.lds;
    const auto seen = slab.emplace(hc::value_of(d, "kernel"), extra).first;
    HC_CHECK(extra >= 0 && extra == seen->second, "the first launch has %zu bytes of dynamic LDS, %ld below the described lds= where other launches of the kernel were %ld below: %s",
             l.lds, extra, seen->second, desc);
    HC_CHECK(!l.any_order, "a tile-pipeline launch is always an ordinary in-order launch");
}

void run_tile(const Env &e, Tokens &k) {
    // tile family resize_type fourcc planes normalization dtype mean*3 scale*3 dst_w dst_h a b c aligned n_frames {w h pitch_y pitch_uv off_y off_uv} total_bytes n_items {start item}
    const std::string family = k.word();
    tsvpp_params p = {};
    p.resize_type = k.i(), p.fourcc = k.i(), p.planes = k.i(), p.normalization = k.i();
    tsvpp_tensor_spec spec = {};
    spec.dtype = k.i();
    for (float &m : spec.mean) m = k.f();
    for (float &s : spec.scale) s = k.f();
    const bool tensor = spec.dtype >= 0;
    p.dst_width = k.i(), p.dst_height = k.i();
    const int a = k.i(), b = k.i(), c = k.i(), aligned = k.i();
    DevFrames fr;
    const int n_frames = k.i();
    for (int f = 0; f < n_frames; f++) {
        const int w = k.i(), h = k.i(), py = k.i(), puv = k.i(), oy = k.i(), ouv = k.i();
        fr.add(w, h, py, puv, oy, ouv);
    }
    const size_t total = (size_t)k.i();
    uint8_t *out = hc::dev_alloc(total);
    const int n = k.i();
    std::vector<void *> outs;
    std::vector<tsvpp_roi> rois;
    std::vector<tsvpp_rect> rects;
    std::vector<tsvpp_nv12> per_item;
    std::vector<tsvpp_warp> warps;
    std::vector<tsvpp_persp> persps;
    bool own_rects = false;
    for (int i = 0; i < n; i++) {
        outs.push_back(out + k.i());
        const int f = k.i();
        if (family == "rois" || family == "rois_area") {
            tsvpp_roi r = { f, 0, 0, 0, 0 };
            r.left = k.i(), r.top = k.i(), r.right = k.i(), r.bottom = k.i();
            rois.push_back(r);
        } else if (family == "letterbox") {
            per_item.push_back(fr.frames[(size_t)f]);
            own_rects = k.i() != 0;
            tsvpp_rect r = {};
            r.left = k.i(), r.top = k.i(), r.width = k.i(), r.height = k.i();
            rects.push_back(r);
        } else if (family == "warp") {
            tsvpp_warp w = {};
            w.frame = f;
            for (float &m : w.m) m = k.f();
            warps.push_back(w);
        } else {
            tsvpp_persp h = {};
            h.frame = f;
            for (float &m : h.h) m = k.f();
            persps.push_back(h);
        }
    }
    char desc[512] = "";
    int ds, cs;
    const char *text = k.line.c_str();
    hc_stub_clear_launches();
    if (family == "rois" || family == "rois_area") {
        if (tensor) {
            ds = tsvpp_describe_rois_tensor(&p, &spec, n_frames, fr.frames.data(), n, rois.data(), aligned, desc, sizeof(desc));
            cs = tsvpp_convert_rois_tensor(e.ctx, n_frames, fr.frames.data(), n, rois.data(), &p, &spec, outs.data(), e.stream);
        } else if (family == "rois") {
            ds = tsvpp_describe_rois(&p, n_frames, fr.frames.data(), n, rois.data(), aligned, desc, sizeof(desc));
            cs = tsvpp_convert_rois(e.ctx, n_frames, fr.frames.data(), n, rois.data(), &p, outs.data(), e.stream);
        } else {
            ds = tsvpp_describe_rois_area(&p, n_frames, fr.frames.data(), n, rois.data(), aligned, desc, sizeof(desc));
            cs = tsvpp_convert_rois_area(e.ctx, n_frames, fr.frames.data(), n, rois.data(), &p, outs.data(), e.stream);
        }
    } else if (family == "letterbox") {
        const tsvpp_rect *rc = own_rects ? rects.data() : nullptr;
        if (tensor) {
            ds = tsvpp_describe_letterbox_tensor(&p, &spec, n, per_item.data(), rc, aligned, desc, sizeof(desc));
            cs = tsvpp_convert_letterbox_tensor(e.ctx, n, per_item.data(), &p, &spec, rc, a, b, c, outs.data(), e.stream);
        } else {
            ds = tsvpp_describe_letterbox(&p, n, per_item.data(), rc, aligned, desc, sizeof(desc));
            cs = tsvpp_convert_letterbox(e.ctx, n, per_item.data(), &p, rc, a, b, c, outs.data(), e.stream);
        }
    } else if (family == "warp") {
        if (tensor) {
            ds = tsvpp_describe_warp_tensor(&p, &spec, n_frames, fr.frames.data(), n, warps.data(), a, b, c, aligned, desc, sizeof(desc));
            cs = tsvpp_convert_warp_tensor(e.ctx, n_frames, fr.frames.data(), n, warps.data(), &p, &spec, a, b, c, outs.data(), e.stream);
        } else {
            ds = tsvpp_describe_warp(&p, n_frames, fr.frames.data(), n, warps.data(), a, b, c, aligned, desc, sizeof(desc));
            cs = tsvpp_convert_warp(e.ctx, n_frames, fr.frames.data(), n, warps.data(), &p, a, b, c, outs.data(), e.stream);
        }
    } else {
        if (tensor) {
            ds = tsvpp_describe_perspective_tensor(&p, &spec, n_frames, fr.frames.data(), n, persps.data(), a, b, c, aligned, desc, sizeof(desc));
            cs = tsvpp_convert_perspective_tensor(e.ctx, n_frames, fr.frames.data(), n, persps.data(), &p, &spec, a, b, c, outs.data(), e.stream);
        } else {
            ds = tsvpp_describe_perspective(&p, n_frames, fr.frames.data(), n, persps.data(), a, b, c, aligned, desc, sizeof(desc));
            cs = tsvpp_convert_perspective(e.ctx, n_frames, fr.frames.data(), n, persps.data(), &p, a, b, c, outs.data(), e.stream);
        }
    }
    HC_CHECK(ds == TSVPP_OK, "the generators draw no call the library refuses, this one is answered %d: %.200s", ds, text);
    check_tile_launches(ds, cs, desc, text);
    HC_CHECK(last_launch().empty(), "tsvpp_debug_last_launch reports fused launches only, not a tile-pipeline call");
    HC_CHECK(hc::current_device() == 0, "the thread ends on device %d", hc::current_device());
    (void)hipFree(out);
}

// remap fw fh dst_w dst_h fourcc planes normalization border*3 pitch lds n n_floats floats      (the map: dst_h rows of dst_w pairs, tight)
// mesh  fw fh dst_w dst_h log2_cw log2_ch fourcc planes normalization border*3 pitch lds n n_floats floats      (the mesh: rows x cols pairs, tight)
void run_map(const Env &e, Tokens &k, bool mesh) {
    const int fw = k.i(), fh = k.i();
    tsvpp_params p = {};
    p.dst_width = k.i(), p.dst_height = k.i();
    p.resize_type = TSVPP_BILINEAR;
    const int l2w = mesh ? k.i() : 0, l2h = mesh ? k.i() : 0;
    p.fourcc = k.i(), p.planes = k.i(), p.normalization = k.i();
    const int by = k.i(), bu = k.i(), bv = k.i(), pitch = k.i(), lds = k.i(), n = k.i(), n_floats = k.i();
    std::vector<float> tight((size_t)n_floats);
    for (float &v : tight) v = k.f();
    const char *text = mesh ? "mesh" : "remap";
    int cols = p.dst_width, rows = p.dst_height;
    if (mesh) HC_CHECK(tsvpp_mesh_dims(p.dst_width, p.dst_height, l2w, l2h, &cols, &rows) == TSVPP_OK, "mesh_dims");
    HC_CHECK((size_t)cols * rows * 2 == tight.size(), "%s of %d x %d entries in %zu floats", text, cols, rows, tight.size());
    if ((size_t)cols * rows * 2 != tight.size()) return;
    // the host copy with the request's pitch (NaN in the padding: no helper may read it), and the "device" copy behind a pointer of the stub's
    const int row_bytes = pitch ? pitch : 8 * cols;
    std::vector<float> host((size_t)row_bytes / 4 * rows, std::numeric_limits<float>::quiet_NaN());
    for (int r = 0; r < rows; r++) std::memcpy(&host[(size_t)r * row_bytes / 4], &tight[(size_t)r * cols * 2], (size_t)cols * 8);
    float *dev = (float *)hc::dev_alloc(host.size() * 4);
    HC_CHECK(hipMemcpy(dev, host.data(), host.size() * 4, hipMemcpyHostToDevice) == hipSuccess, "upload of the %s", text);
    DevFrames fr;
    fr.add(fw, fh, fw + 16, fw, 0, 0);
    const size_t out_bytes = tsvpp_out_bytes(&p, p.dst_width, p.dst_height);
    uint8_t *out = hc::dev_alloc(out_bytes * n + 16);
    std::vector<void *> outs;
    std::vector<tsvpp_remap> remaps;
    for (int i = 0; i < n; i++) {
        outs.push_back(out + (size_t)i * out_bytes);
        remaps.push_back(tsvpp_remap{ 0, 0 });
    }
    const bool aligned = out_bytes % 16 == 0;
    char desc[512] = "";
    int ds, cs;
    hc_stub_clear_launches();
    if (mesh) {
        const tsvpp_mesh m = { dev, pitch, l2w, l2h, lds };
        ds = tsvpp_describe_mesh(&p, 1, fr.frames.data(), 1, &m, n, remaps.data(), by, bu, bv, aligned, desc, sizeof(desc));
        cs = tsvpp_convert_mesh(e.ctx, 1, fr.frames.data(), 1, &m, n, remaps.data(), &p, by, bu, bv, outs.data(), e.stream);
    } else {
        const tsvpp_map m = { dev, pitch, lds };
        ds = tsvpp_describe_remap(&p, 1, fr.frames.data(), 1, &m, n, remaps.data(), by, bu, bv, aligned, desc, sizeof(desc));
        cs = tsvpp_convert_remap(e.ctx, 1, fr.frames.data(), 1, &m, n, remaps.data(), &p, by, bu, bv, outs.data(), e.stream);
    }
    HC_CHECK(ds == TSVPP_OK, "%s request refused: %d", text, ds);
    check_tile_launches(ds, cs, desc, k.line.substr(0, 120).c_str());
    // the helpers on the host copy
    const int dw = p.dst_width, dh = p.dst_height, luma_only = p.fourcc == TSVPP_Y800;
    int32_t box[8];
    std::vector<float> dense;
    const float *map = host.data();
    int map_pitch = pitch;
    if (mesh) {
        dense.assign((size_t)dw * dh * 2, 0.f);
        HC_CHECK(tsvpp_mesh_expand(host.data(), pitch, dw, dh, l2w, l2h, dense.data(), 0) == TSVPP_OK, "mesh_expand");
        std::vector<float> back(host.size(), 0.f);
        float err = -1.f;
        HC_CHECK(tsvpp_mesh_from_map(dense.data(), 0, dw, dh, l2w, l2h, back.data(), pitch) == TSVPP_OK, "mesh_from_map");
        HC_CHECK(tsvpp_mesh_error(dense.data(), 0, dw, dh, host.data(), pitch, l2w, l2h, &err) == TSVPP_OK && err == 0.f, "mesh_error of E(mesh) against the mesh: %g", err);
        const int need = tsvpp_mesh_lds_need(host.data(), pitch, dw, dh, l2w, l2h, fw, fh, luma_only);
        HC_CHECK(need >= 0 && need == tsvpp_remap_lds_need(dense.data(), 0, dw, dh, fw, fh, luma_only), "mesh_lds_need %d is remap_lds_need of E(mesh)", need);
        map = dense.data();
        map_pitch = 0;
    }
    HC_CHECK(tsvpp_remap_footprint(map, map_pitch, dw, dh, fw, fh, 0, dw - 1, 0, dh - 1, box) == TSVPP_OK, "remap_footprint of the whole output");
    HC_CHECK(box[0] >= 0 && box[1] <= fw && box[0] <= box[1] && box[2] >= 0 && box[3] <= fh && box[4] >= 0 && box[5] <= fw / 2 && box[6] >= 0 && box[7] <= fh / 2,
             "the footprint lies inside the frame: %d %d %d %d / %d %d %d %d", box[0], box[1], box[2], box[3], box[4], box[5], box[6], box[7]);
    HC_CHECK(tsvpp_remap_lds_need(map, map_pitch, dw, dh, fw, fh, luma_only) >= 0, "remap_lds_need");
    (void)hipFree(out);
    (void)hipFree(dev);
}

// ---- the helper entry points: valid inputs and every refusal include/tsvpp.h names -------------------------------------------------------------------------------
void helpers() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const double dnan = std::numeric_limits<double>::quiet_NaN();
    int32_t box[8];
    { // tsvpp_letterbox_rect
        tsvpp_rect r = {};
        HC_CHECK(tsvpp_letterbox_rect(1920, 1080, 640, 640, &r) == TSVPP_OK && r.left == 0 && r.top == 140 && r.width == 640 && r.height == 360,
                 "1920 x 1080 into 640 x 640 gives 640 x 360 at (0, 140): %d x %d at (%d, %d)", r.width, r.height, r.left, r.top);
        HC_CHECK(tsvpp_letterbox_rect(2, 100000, 640, 640, &r) == TSVPP_OK && r.width == 2 && r.height == 640, "the width is clamped to 2");
        HC_CHECK(tsvpp_letterbox_rect(1920, 1080, 640, 640, nullptr) == TSVPP_ERROR, "null out");
        HC_CHECK(tsvpp_letterbox_rect(0, 1080, 640, 640, &r) == TSVPP_ERROR && tsvpp_letterbox_rect(1920, -2, 640, 640, &r) == TSVPP_ERROR &&
                     tsvpp_letterbox_rect(1920, 1080, 0, 640, &r) == TSVPP_ERROR && tsvpp_letterbox_rect(1920, 1080, 640, -4, &r) == TSVPP_ERROR,
                 "a size <= 0");
        HC_CHECK(tsvpp_letterbox_rect(1920, 1080, 641, 640, &r) == TSVPP_UNSUPPORTED && tsvpp_letterbox_rect(1920, 1080, 640, 639, &r) == TSVPP_UNSUPPORTED, "an odd canvas");
    }
    { // tsvpp_area_pattern, tsvpp_roi_area_rows
        float tab[4096], rows[4096];
        int taps = 0, rtaps = 0;
        const int n = tsvpp_area_pattern(2.5f, tab, 4096, &taps);
        HC_CHECK(n > 0 && taps == 3, "area_pattern(2.5): %d rows of %d taps", n, taps);
        HC_CHECK(tsvpp_area_pattern(2.5f, nullptr, 0, &taps) == n && tsvpp_area_pattern(2.5f, tab, 1, nullptr) == n, "area_pattern without a buffer / with one too small: the rows");
        HC_CHECK(tsvpp_roi_area_rows(2.5f, 0, 2 * n, rows, 4096, &rtaps) == 2 * n && rtaps == taps, "roi_area_rows(2.5)");
        bool same = true;
        for (int j = 0; j < 2 * n; j++) same = same && std::memcmp(&rows[(size_t)j * taps], &tab[(size_t)(j % n) * taps], sizeof(float) * (size_t)taps) == 0;
        HC_CHECK(same, "row j of roi_area_rows equals row j %% rows of area_pattern");
        HC_CHECK(tsvpp_roi_area_rows(1.0f, 0, 1, rows, 4096, &rtaps) == TSVPP_UNSUPPORTED && tsvpp_roi_area_rows(0.5f, 0, 1, rows, 4096, &rtaps) == TSVPP_UNSUPPORTED, "scale <= 1");
        HC_CHECK(tsvpp_roi_area_rows(40.5f, 0, 1, rows, 4096, &rtaps) == TSVPP_UNSUPPORTED, "more than 40 taps");
        HC_CHECK(tsvpp_roi_area_rows(2.5f, 65530, 7, rows, 4096, &rtaps) == TSVPP_UNSUPPORTED, "first + n > 65536");
        HC_CHECK(tsvpp_roi_area_rows(2.5f, 65530, 6, rows, 4096, &rtaps) == 6, "first + n == 65536");
        HC_CHECK(tsvpp_roi_area_rows(2.5f, 0, 4, nullptr, 4096, &rtaps) == TSVPP_ERROR, "a null buffer");
        HC_CHECK(tsvpp_roi_area_rows(2.5f, 0, 4, rows, 4096, nullptr) == 4, "`taps` is optional, as tsvpp_area_pattern's");
        HC_CHECK(tsvpp_roi_area_rows(2.5f, 0, 0, rows, 4096, &rtaps) == TSVPP_ERROR, "no rows");
        HC_CHECK(tsvpp_roi_area_rows(2.5f, -1, 4, rows, 4096, &rtaps) == TSVPP_ERROR && tsvpp_roi_area_rows(2.5f, 0, -4, rows, 4096, &rtaps) == TSVPP_ERROR, "negative arguments");
        HC_CHECK(tsvpp_roi_area_rows(2.5f, 0, 4, rows, 11, &rtaps) == TSVPP_ERROR && tsvpp_roi_area_rows(2.5f, 0, 4, rows, 12, &rtaps) == 4, "a buffer of 11 floats for 4 rows of 3 taps");
    }
    { // tsvpp_warp_footprint, tsvpp_warp_rotated_box
        tsvpp_warp w = { 0, { 2.f, 0.f, 0.f, 0.f, 2.f, 0.f } };
        HC_CHECK(tsvpp_warp_footprint(&w, 640, 360, 0, 31, 0, 31, box) == TSVPP_OK && box[0] >= 0 && box[1] <= 640 && box[1] >= 62, "warp_footprint: x %d .. %d", box[0], box[1]);
        HC_CHECK(tsvpp_warp_footprint(nullptr, 640, 360, 0, 31, 0, 31, box) == TSVPP_ERROR && tsvpp_warp_footprint(&w, 640, 360, 0, 31, 0, 31, nullptr) == TSVPP_ERROR, "null arguments");
        HC_CHECK(tsvpp_warp_footprint(&w, 0, 360, 0, 31, 0, 31, box) == TSVPP_ERROR && tsvpp_warp_footprint(&w, 640, -1, 0, 31, 0, 31, box) == TSVPP_ERROR, "a frame size <= 0");
        HC_CHECK(tsvpp_warp_footprint(&w, 640, 360, 8, 7, 0, 31, box) == TSVPP_ERROR && tsvpp_warp_footprint(&w, 640, 360, 0, 31, 4, 1, box) == TSVPP_ERROR, "an empty range");
        HC_CHECK(tsvpp_warp_footprint(&w, 640, 360, -2, 31, 0, 31, box) == TSVPP_ERROR && tsvpp_warp_footprint(&w, 640, 360, 0, 31, -2, 31, box) == TSVPP_ERROR, "a negative range");
        tsvpp_warp r = { 7, {} };
        HC_CHECK(tsvpp_warp_rotated_box(320, 180, 640, 360, 0.0, 320, 180, &r) == TSVPP_OK && r.frame == 7 && r.m[0] == 2.f && r.m[1] == 0.f && r.m[2] == 0.f && r.m[4] == 2.f,
                 "angle 0 with the box equal to the frame");
        HC_CHECK(tsvpp_warp_rotated_box(320, 180, 640, 360, 0.0, 320, 180, nullptr) == TSVPP_ERROR && tsvpp_warp_rotated_box(dnan, 180, 640, 360, 0.0, 320, 180, &r) == TSVPP_ERROR &&
                     tsvpp_warp_rotated_box(320, 180, 0, 360, 0.0, 320, 180, &r) == TSVPP_ERROR && tsvpp_warp_rotated_box(320, 180, 640, 360, 0.0, 0, 180, &r) == TSVPP_ERROR,
                 "warp_rotated_box refusals");
    }
    { // tsvpp_persp_footprint, tsvpp_persp_from_quad
        tsvpp_persp h = { 0, { 2.f, 0.f, 0.f, 0.f, 2.f, 0.f, 0.f, 0.f, 1.f } };
        HC_CHECK(tsvpp_persp_footprint(&h, 640, 360, 0, 31, 0, 31, box) == TSVPP_OK && box[0] >= 0 && box[1] <= 640, "persp_footprint");
        HC_CHECK(tsvpp_persp_footprint(nullptr, 640, 360, 0, 31, 0, 31, box) == TSVPP_ERROR && tsvpp_persp_footprint(&h, 640, 360, 0, 31, 0, 31, nullptr) == TSVPP_ERROR, "null arguments");
        HC_CHECK(tsvpp_persp_footprint(&h, 0, 360, 0, 31, 0, 31, box) == TSVPP_ERROR && tsvpp_persp_footprint(&h, 640, 0, 0, 31, 0, 31, box) == TSVPP_ERROR, "a frame size <= 0");
        HC_CHECK(tsvpp_persp_footprint(&h, 640, 360, 8, 7, 0, 31, box) == TSVPP_ERROR && tsvpp_persp_footprint(&h, 640, 360, 0, 31, -2, 31, box) == TSVPP_ERROR, "an empty or negative range");
        tsvpp_persp horizon = { 0, { 2.f, 0.f, 0.f, 0.f, 2.f, 0.f, -0.1f, 0.f, 1.f } }; // the denominator reaches zero at u = 10
        HC_CHECK(tsvpp_persp_footprint(&horizon, 640, 360, 0, 31, 0, 31, box) == TSVPP_UNSUPPORTED, "a denominator below 2^-64 inside the range");
        const double quad[8] = { 0, 0, 640, 0, 640, 360, 0, 360 }, flat[8] = { 0, 0, 10, 0, 20, 0, 30, 0 }, bad[8] = { 0, 0, dnan, 0, 640, 360, 0, 360 };
        tsvpp_persp q = { 3, {} };
        HC_CHECK(tsvpp_persp_from_quad(quad, 320, 180, &q) == TSVPP_OK && q.frame == 3 && q.h[0] == 2.f && q.h[4] == 2.f && q.h[6] == 0.f && q.h[7] == 0.f && q.h[8] == 1.f,
                 "the frame's own corners: a parallelogram, g = h = 0 exactly");
        const double trapezoid[8] = { 100, 0, 540, 0, 640, 360, 0, 360 };
        HC_CHECK(tsvpp_persp_from_quad(trapezoid, 320, 180, &q) == TSVPP_OK && q.h[7] != 0.f, "a trapezoid has a perspective term");
        HC_CHECK(tsvpp_persp_from_quad(nullptr, 320, 180, &q) == TSVPP_ERROR && tsvpp_persp_from_quad(quad, 320, 180, nullptr) == TSVPP_ERROR, "null arguments");
        HC_CHECK(tsvpp_persp_from_quad(bad, 320, 180, &q) == TSVPP_ERROR, "an input that is not finite");
        HC_CHECK(tsvpp_persp_from_quad(quad, 0, 180, &q) == TSVPP_ERROR && tsvpp_persp_from_quad(quad, 320, -1, &q) == TSVPP_ERROR, "dst <= 0");
        HC_CHECK(tsvpp_persp_from_quad(flat, 320, 180, &q) == TSVPP_ERROR, "den == 0");
    }
    { // the map and mesh helpers: refusals (valid inputs: run_map)
        const int dw = 16, dh = 8;
        std::vector<float> map((size_t)dw * dh * 2);
        for (int i = 0; i < dh; i++)
            for (int j = 0; j < dw; j++) map[((size_t)i * dw + j) * 2] = 2.f * j + 0.5f, map[((size_t)i * dw + j) * 2 + 1] = 2.f * i + 0.5f;
        map[5] = nan; // any bits are a legal coordinate
        HC_CHECK(tsvpp_remap_footprint(map.data(), 0, dw, dh, 32, 16, 0, 15, 0, 7, box) == TSVPP_OK, "remap_footprint");
        HC_CHECK(tsvpp_remap_footprint(nullptr, 0, dw, dh, 32, 16, 0, 15, 0, 7, box) == TSVPP_ERROR && tsvpp_remap_footprint(map.data(), 0, dw, dh, 32, 16, 0, 15, 0, 7, nullptr) == TSVPP_ERROR,
                 "null arguments");
        HC_CHECK(tsvpp_remap_footprint(map.data(), 0, 0, dh, 32, 16, 0, 15, 0, 7, box) == TSVPP_ERROR && tsvpp_remap_footprint(map.data(), 0, dw, dh, 32, 0, 0, 15, 0, 7, box) == TSVPP_ERROR,
                 "a size <= 0");
        HC_CHECK(tsvpp_remap_footprint(map.data(), 0, 15, dh, 32, 16, 0, 13, 0, 7, box) == TSVPP_ERROR && tsvpp_remap_footprint(map.data(), 0, dw, dh, 31, 16, 0, 15, 0, 7, box) == TSVPP_ERROR,
                 "an odd size");
        HC_CHECK(tsvpp_remap_footprint(map.data(), 8 * dw - 8, dw, dh, 32, 16, 0, 15, 0, 7, box) == TSVPP_ERROR && tsvpp_remap_footprint(map.data(), 8 * dw + 4, dw, dh, 32, 16, 0, 15, 0, 7, box) == TSVPP_ERROR,
                 "a pitch below 8 * dst_w or no multiple of 8");
        HC_CHECK(tsvpp_remap_footprint(map.data(), 0, dw, dh, 32, 16, 4, 3, 0, 7, box) == TSVPP_ERROR && tsvpp_remap_footprint(map.data(), 0, dw, dh, 32, 16, 0, 17, 0, 7, box) == TSVPP_ERROR &&
                     tsvpp_remap_footprint(map.data(), 0, dw, dh, 32, 16, 0, 15, 0, 9, box) == TSVPP_ERROR && tsvpp_remap_footprint(map.data(), 0, dw, dh, 32, 16, -2, 15, 0, 7, box) == TSVPP_ERROR,
                 "a range that is empty or leaves the map");
        HC_CHECK(tsvpp_remap_lds_need(map.data(), 0, dw, dh, 32, 16, 0) >= 0 && tsvpp_remap_lds_need(map.data(), 0, dw, dh, 32, 16, 1) >= 0, "remap_lds_need");
        HC_CHECK(tsvpp_remap_lds_need(nullptr, 0, dw, dh, 32, 16, 0) < 0 && tsvpp_remap_lds_need(map.data(), 0, 15, dh, 32, 16, 0) < 0 && tsvpp_remap_lds_need(map.data(), 4, dw, dh, 32, 16, 0) < 0 &&
                     tsvpp_remap_lds_need(map.data(), 0, dw, dh, 0, 16, 0) < 0,
                 "remap_lds_need refuses what remap_footprint refuses");
        int cols = 0, rows = 0;
        HC_CHECK(tsvpp_mesh_dims(dw, dh, 2, 2, &cols, &rows) == TSVPP_OK && cols == 5 && rows == 3, "mesh_dims(16, 8, 4 x 4 cells): %d x %d", cols, rows);
        HC_CHECK(tsvpp_mesh_dims(dw, dh, 2, 2, nullptr, &rows) == TSVPP_ERROR && tsvpp_mesh_dims(dw, dh, 2, 2, &cols, nullptr) == TSVPP_ERROR, "mesh_dims: null arguments");
        HC_CHECK(tsvpp_mesh_dims(0, dh, 2, 2, &cols, &rows) == TSVPP_ERROR && tsvpp_mesh_dims(dw, 7, 2, 2, &cols, &rows) == TSVPP_ERROR, "mesh_dims: a size <= 0 or odd");
        HC_CHECK(tsvpp_mesh_dims(dw, dh, 1, 2, &cols, &rows) == TSVPP_UNSUPPORTED && tsvpp_mesh_dims(dw, dh, 2, 9, &cols, &rows) == TSVPP_UNSUPPORTED, "mesh_dims: a cell size outside 2..8");
        std::vector<float> mesh((size_t)5 * 3 * 2), dense((size_t)dw * dh * 2);
        float err = 0.f;
        HC_CHECK(tsvpp_mesh_from_map(map.data(), 0, dw, dh, 2, 2, mesh.data(), 0) == TSVPP_OK, "mesh_from_map");
        HC_CHECK(tsvpp_mesh_expand(mesh.data(), 0, dw, dh, 2, 2, dense.data(), 0) == TSVPP_OK, "mesh_expand");
        HC_CHECK(tsvpp_mesh_error(map.data(), 0, dw, dh, mesh.data(), 0, 2, 2, &err) == TSVPP_OK && err >= 0.f, "mesh_error: %g", err);
        HC_CHECK(tsvpp_mesh_lds_need(mesh.data(), 0, dw, dh, 2, 2, 32, 16, 0) >= 0, "mesh_lds_need");
        HC_CHECK(tsvpp_mesh_expand(nullptr, 0, dw, dh, 2, 2, dense.data(), 0) == TSVPP_ERROR && tsvpp_mesh_expand(mesh.data(), 0, dw, dh, 2, 2, nullptr, 0) == TSVPP_ERROR, "mesh_expand: null arguments");
        HC_CHECK(tsvpp_mesh_expand(mesh.data(), 0, 15, dh, 2, 2, dense.data(), 0) == TSVPP_ERROR && tsvpp_mesh_expand(mesh.data(), 0, dw, 0, 2, 2, dense.data(), 0) == TSVPP_ERROR, "mesh_expand: a size");
        HC_CHECK(tsvpp_mesh_expand(mesh.data(), 32, dw, dh, 2, 2, dense.data(), 0) == TSVPP_ERROR && tsvpp_mesh_expand(mesh.data(), 0, dw, dh, 2, 2, dense.data(), 8 * dw - 8) == TSVPP_ERROR &&
                     tsvpp_mesh_expand(mesh.data(), 44, dw, dh, 2, 2, dense.data(), 0) == TSVPP_ERROR,
                 "mesh_expand: a bad pitch");
        HC_CHECK(tsvpp_mesh_expand(mesh.data(), 0, dw, dh, 1, 2, dense.data(), 0) == TSVPP_UNSUPPORTED, "mesh_expand: a cell size outside 2..8");
        HC_CHECK(tsvpp_mesh_from_map(nullptr, 0, dw, dh, 2, 2, mesh.data(), 0) == TSVPP_ERROR && tsvpp_mesh_from_map(map.data(), 0, dw, dh, 2, 2, nullptr, 0) == TSVPP_ERROR &&
                     tsvpp_mesh_from_map(map.data(), 0, dw, 9, 2, 2, mesh.data(), 0) == TSVPP_ERROR && tsvpp_mesh_from_map(map.data(), 8, dw, dh, 2, 2, mesh.data(), 0) == TSVPP_ERROR &&
                     tsvpp_mesh_from_map(map.data(), 0, dw, dh, 2, 2, mesh.data(), 32) == TSVPP_ERROR,
                 "mesh_from_map: null, odd size, bad pitches");
        HC_CHECK(tsvpp_mesh_from_map(map.data(), 0, dw, dh, 9, 2, mesh.data(), 0) == TSVPP_UNSUPPORTED, "mesh_from_map: a cell size outside 2..8");
        HC_CHECK(tsvpp_mesh_error(nullptr, 0, dw, dh, mesh.data(), 0, 2, 2, &err) == TSVPP_ERROR && tsvpp_mesh_error(map.data(), 0, dw, dh, nullptr, 0, 2, 2, &err) == TSVPP_ERROR &&
                     tsvpp_mesh_error(map.data(), 0, dw, dh, mesh.data(), 0, 2, 2, nullptr) == TSVPP_ERROR && tsvpp_mesh_error(map.data(), 0, -2, dh, mesh.data(), 0, 2, 2, &err) == TSVPP_ERROR &&
                     tsvpp_mesh_error(map.data(), 12, dw, dh, mesh.data(), 0, 2, 2, &err) == TSVPP_ERROR,
                 "mesh_error: null, size, pitch");
        HC_CHECK(tsvpp_mesh_error(map.data(), 0, dw, dh, mesh.data(), 0, 2, 1, &err) == TSVPP_UNSUPPORTED, "mesh_error: a cell size outside 2..8");
        HC_CHECK(tsvpp_mesh_lds_need(nullptr, 0, dw, dh, 2, 2, 32, 16, 0) == TSVPP_ERROR && tsvpp_mesh_lds_need(mesh.data(), 0, dw, dh, 2, 2, 0, 16, 0) == TSVPP_ERROR &&
                     tsvpp_mesh_lds_need(mesh.data(), 0, dw, dh, 2, 2, 32, 15, 0) == TSVPP_ERROR && tsvpp_mesh_lds_need(mesh.data(), 20, dw, dh, 2, 2, 32, 16, 0) == TSVPP_ERROR,
                 "mesh_lds_need: null, size, pitch");
        HC_CHECK(tsvpp_mesh_lds_need(mesh.data(), 0, dw, dh, 0, 2, 32, 16, 0) == TSVPP_UNSUPPORTED, "mesh_lds_need: a cell size outside 2..8");
    }
}

// the argument rules of the conversion itself (include/tsvpp.h and tsvpp_strerror's own words), on a live context
void refusals(const Env &e) {
    tsvpp_params p = {};
    p.dst_width = 320, p.dst_height = 180, p.resize_type = TSVPP_BILINEAR, p.fourcc = TSVPP_RGB24;
    tsvpp_nv12 in[2] = { { e.y, e.uv, 640, 640, 640, 360 }, { e.y, e.uv, 640, 640, 640, 360 } };
    void *outs[2] = { e.out, e.out };
    HC_CHECK(tsvpp_convert_batch(nullptr, 2, in, &p, outs, e.stream) == TSVPP_ERROR && tsvpp_convert_batch(e.ctx, 2, nullptr, &p, outs, e.stream) == TSVPP_ERROR &&
                 tsvpp_convert_batch(e.ctx, 2, in, nullptr, outs, e.stream) == TSVPP_ERROR && tsvpp_convert_batch(e.ctx, 2, in, &p, nullptr, e.stream) == TSVPP_ERROR &&
                 tsvpp_convert_batch(e.ctx, -1, in, &p, outs, e.stream) == TSVPP_ERROR,
             "null arguments and a negative count are TSVPP_ERROR");
    HC_CHECK(tsvpp_convert_batch(e.ctx, 0, in, &p, outs, e.stream) == TSVPP_OK, "no frames is no work");
    void *hole[2] = { e.out, nullptr };
    HC_CHECK(tsvpp_convert_batch(e.ctx, 2, in, &p, hole, e.stream) == TSVPP_ERROR, "a null output");
    tsvpp_nv12 mixed[2] = { in[0], in[1] };
    mixed[1].width = 642;
    HC_CHECK(tsvpp_convert_batch(e.ctx, 2, mixed, &p, outs, e.stream) == TSVPP_UNSUPPORTED, "mixed batch geometry");
    mixed[1] = in[1];
    mixed[1].pitch_uv = 704;
    HC_CHECK(tsvpp_convert_batch(e.ctx, 2, mixed, &p, outs, e.stream) == TSVPP_UNSUPPORTED, "mixed pitches");
    tsvpp_nv12 narrow = { e.y, e.uv, 638, 640, 640, 360 };
    HC_CHECK(tsvpp_convert(e.ctx, &narrow, &p, e.out, e.stream) == TSVPP_ERROR, "a pitch below the width");
    tsvpp_params odd = p;
    odd.dst_width = 321;
    char buf[256];
    const int ds = tsvpp_describe(&odd, 640, 360, 640, 640, 1, 1, buf, sizeof(buf));
    HC_CHECK(ds != TSVPP_OK && tsvpp_convert(e.ctx, in, &odd, e.out, e.stream) == ds, "an odd output width: describe and convert agree on %d", ds);
    HC_CHECK(last_launch().empty(), "a refused conversion leaves no launch record");
    tsvpp_ctx *none = nullptr;
    HC_CHECK(tsvpp_create(2, 1, &none) == (int)hipErrorInvalidDevice && !none && tsvpp_create(-1, 1, &none) == (int)hipErrorInvalidDevice, "a device the runtime does not have");
    HC_CHECK(tsvpp_create(0, -1, &none) == TSVPP_ERROR && tsvpp_create(0, 1, nullptr) == TSVPP_ERROR, "tsvpp_create: a negative pool, a null result");
    void *s = nullptr;
    HC_CHECK(tsvpp_consumer_stream(e.ctx, "second", &s) == TSVPP_OK && tsvpp_consumer_stream(e.ctx, "third", &s) == TSVPP_ERROR && s == nullptr, "the pool of two is exhausted by the third name");
    HC_CHECK(tsvpp_consumer_synchronize(e.ctx, "nobody") == TSVPP_ERROR, "no such consumer");
    tsvpp_table *tab = nullptr;
    HC_CHECK(tsvpp_table_create(e.ctx, 0, &tab) == TSVPP_ERROR && tsvpp_table_create(e.ctx, 4, nullptr) == TSVPP_ERROR && tsvpp_table_create(nullptr, 4, &tab) == TSVPP_ERROR, "table_create refusals");
    int v = 0;
    HC_CHECK(tsvpp_set_option(e.ctx, TSVPP_OPT_INPUTS_READY, 4) == TSVPP_ERROR && tsvpp_set_option(e.ctx, TSVPP_OPT_COLOR_G_TERM, 3) == TSVPP_ERROR &&
                 tsvpp_set_option(e.ctx, 99, 0) == TSVPP_UNSUPPORTED && tsvpp_get_option(e.ctx, 99, &v) == TSVPP_UNSUPPORTED && tsvpp_get_option(e.ctx, TSVPP_OPT_INPUTS_READY, nullptr) == TSVPP_ERROR,
             "option refusals");
    tsvpp_coeffs k;
    tsvpp_default_coeffs(&k);
    k.y_scale = 1.0f;
    HC_CHECK(tsvpp_set_coeffs(e.ctx, &k) == TSVPP_UNSUPPORTED, "a block that differs from the defaults, without TSVPP_OPT_UNSAFE_COEFFS");
}

// ---- the source limit (include/tsvpp.h: TSVPP_SOURCE_SPAN_LIMIT) -------------------------------------------------------------------------------------------------
// Every describe / convert pair on frames whose plane spans lie one byte under the limit (accepted, launched) and at it (TSVPP_UNSUPPORTED, nothing launched), luma
// and chroma separately, and on a small crop / box inside a frame far beyond the limit.  Nothing of these sizes is allocated: the stub records launches, and the
// library's host arithmetic on the pitches is what the sanitizers see.
struct SpanGeom { int w, h, py, puv; };
// an even width and pitches with (rows - 1) * pitch + w == span, for the luma plane (h rows) and the chroma plane (h / 2 rows) each; span 0: an ordinary pitch (wide enough for a frame 128 columns wider)
SpanGeom span_geom(int h, uint64_t span_y, uint64_t span_uv) {
    for (int w = 32; w < 8192; w += 2) {
        if (span_y && (span_y - (uint64_t)w) % (uint64_t)(h - 1)) continue;
        if (span_uv && (span_uv - (uint64_t)w) % (uint64_t)(h / 2 - 1)) continue;
        const uint64_t py = span_y ? (span_y - (uint64_t)w) / (uint64_t)(h - 1) : (uint64_t)((w + 128 + 15) & ~15);
        const uint64_t puv = span_uv ? (span_uv - (uint64_t)w) / (uint64_t)(h / 2 - 1) : (uint64_t)((w + 128 + 15) & ~15);
        if (py < (1ull << 31) && puv < (1ull << 31)) return SpanGeom{ w, h, (int)py, (int)puv };
    }
    std::fprintf(stderr, "hc_requests: no geometry for spans %llu / %llu\n", (unsigned long long)span_y, (unsigned long long)span_uv);
    std::exit(3);
}

void expect_span(int ds, int cs, int want, const char *call, const char *what) {
    HC_CHECK(ds == want && cs == want, "%s, %s: describe answers %d, convert %d, expected %d", call, what, ds, cs, want);
    if (want == TSVPP_OK) HC_CHECK(hc_stub_launch_count() >= 1, "%s, %s: accepted and nothing launched", call, what);
    else HC_CHECK(hc_stub_launch_count() == 0, "%s, %s: refused and %zu launches recorded", call, what, hc_stub_launch_count());
    hc_stub_clear_launches();
}

// tsvpp_describe / tsvpp_convert / _batch / _table on `fr` with the crop of `p`
void plain_span_case(const Env &e, const tsvpp_nv12 &fr, const tsvpp_params &p, int want, const char *what) {
    char desc[512];
    void *out = e.out;
    hc_stub_clear_launches();
    const int ds = tsvpp_describe(&p, fr.width, fr.height, fr.pitch_y, fr.pitch_uv, 1, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert(e.ctx, &fr, &p, e.out, e.stream), want, "tsvpp_convert", what);
    expect_span(ds, tsvpp_convert_batch(e.ctx, 1, &fr, &p, &out, e.stream), want, "tsvpp_convert_batch", what);
    tsvpp_table *tab = nullptr;
    HC_CHECK(tsvpp_table_create(e.ctx, 4, &tab) == TSVPP_OK && tab, "table_create");
    if (!tab) return;
    HC_CHECK(tsvpp_table_set(tab, 1, 1, &fr, &out, e.stream) == TSVPP_OK, "table_set: %s", what);
    hc_stub_clear_launches();
    expect_span(ds, tsvpp_convert_table(e.ctx, tab, 1, 1, &p, e.stream), want, "tsvpp_convert_table", what);
    tsvpp_table_destroy(tab);
}

// the ROI calls on one box of `fr`
void rois_span_case(const Env &e, const tsvpp_nv12 &fr, const tsvpp_roi &box, int want, const char *what) {
    char desc[512];
    void *out = e.out;
    tsvpp_params p = {};
    p.dst_width = 64, p.dst_height = 32, p.resize_type = TSVPP_BILINEAR, p.fourcc = TSVPP_RGB24, p.planes = TSVPP_PLANAR, p.normalization = 1;
    const tsvpp_tensor_spec spec = { TSVPP_F32, { 0.f, 0.f, 0.f }, { 1.f, 1.f, 1.f } };
    hc_stub_clear_launches();
    int ds = tsvpp_describe_rois(&p, 1, &fr, 1, &box, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_rois(e.ctx, 1, &fr, 1, &box, &p, &out, e.stream), want, "tsvpp_convert_rois", what);
    ds = tsvpp_describe_rois_tensor(&p, &spec, 1, &fr, 1, &box, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_rois_tensor(e.ctx, 1, &fr, 1, &box, &p, &spec, &out, e.stream), want, "tsvpp_convert_rois_tensor", what);
    p.resize_type = TSVPP_AREA;
    p.dst_width = 16, p.dst_height = 8;
    ds = tsvpp_describe_rois_area(&p, 1, &fr, 1, &box, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_rois_area(e.ctx, 1, &fr, 1, &box, &p, &out, e.stream), want, "tsvpp_convert_rois_area", what);
}

// the calls that sample the whole frame: letterbox, warp, perspective, remap, mesh and their tensor forms
void frame_span_case(const Env &e, const tsvpp_nv12 &fr, int want, const char *what) {
    char desc[512];
    void *out = e.out;
    tsvpp_params p = {};
    p.dst_width = 64, p.dst_height = 32, p.resize_type = TSVPP_BILINEAR, p.fourcc = TSVPP_RGB24, p.planes = TSVPP_PLANAR, p.normalization = 1;
    const tsvpp_tensor_spec spec = { TSVPP_F32, { 0.f, 0.f, 0.f }, { 1.f, 1.f, 1.f } };
    const tsvpp_warp warp = { 0, { (float)fr.width / 64.f, 0.f, 0.f, 0.f, (float)fr.height / 32.f, 0.f } };
    const tsvpp_persp persp = { 0, { warp.m[0], 0.f, 0.f, 0.f, warp.m[4], 0.f, 0.f, 0.f, 1.f } };
    const tsvpp_map map = { (const float *)e.out, 0, 0 };   // (never read: the stub executes nothing)
    const tsvpp_mesh mesh = { (const float *)e.out, 0, 4, 4, 0 };
    const tsvpp_remap pair = { 0, 0 };
    hc_stub_clear_launches();
    int ds = tsvpp_describe_letterbox(&p, 1, &fr, nullptr, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_letterbox(e.ctx, 1, &fr, &p, nullptr, 114, 128, 128, &out, e.stream), want, "tsvpp_convert_letterbox", what);
    ds = tsvpp_describe_letterbox_tensor(&p, &spec, 1, &fr, nullptr, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_letterbox_tensor(e.ctx, 1, &fr, &p, &spec, nullptr, 114, 128, 128, &out, e.stream), want, "tsvpp_convert_letterbox_tensor", what);
    ds = tsvpp_describe_warp(&p, 1, &fr, 1, &warp, -1, -1, -1, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_warp(e.ctx, 1, &fr, 1, &warp, &p, -1, -1, -1, &out, e.stream), want, "tsvpp_convert_warp", what);
    ds = tsvpp_describe_warp_tensor(&p, &spec, 1, &fr, 1, &warp, 16, 128, 128, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_warp_tensor(e.ctx, 1, &fr, 1, &warp, &p, &spec, 16, 128, 128, &out, e.stream), want, "tsvpp_convert_warp_tensor", what);
    ds = tsvpp_describe_perspective(&p, 1, &fr, 1, &persp, -1, -1, -1, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_perspective(e.ctx, 1, &fr, 1, &persp, &p, -1, -1, -1, &out, e.stream), want, "tsvpp_convert_perspective", what);
    ds = tsvpp_describe_perspective_tensor(&p, &spec, 1, &fr, 1, &persp, 16, 128, 128, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_perspective_tensor(e.ctx, 1, &fr, 1, &persp, &p, &spec, 16, 128, 128, &out, e.stream), want, "tsvpp_convert_perspective_tensor", what);
    ds = tsvpp_describe_remap(&p, 1, &fr, 1, &map, 1, &pair, -1, -1, -1, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_remap(e.ctx, 1, &fr, 1, &map, 1, &pair, &p, -1, -1, -1, &out, e.stream), want, "tsvpp_convert_remap", what);
    ds = tsvpp_describe_remap_tensor(&p, &spec, 1, &fr, 1, &map, 1, &pair, 16, 128, 128, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_remap_tensor(e.ctx, 1, &fr, 1, &map, 1, &pair, &p, &spec, 16, 128, 128, &out, e.stream), want, "tsvpp_convert_remap_tensor", what);
    ds = tsvpp_describe_mesh(&p, 1, &fr, 1, &mesh, 1, &pair, -1, -1, -1, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_mesh(e.ctx, 1, &fr, 1, &mesh, 1, &pair, &p, -1, -1, -1, &out, e.stream), want, "tsvpp_convert_mesh", what);
    ds = tsvpp_describe_mesh_tensor(&p, &spec, 1, &fr, 1, &mesh, 1, &pair, 16, 128, 128, 1, desc, sizeof(desc));
    expect_span(ds, tsvpp_convert_mesh_tensor(e.ctx, 1, &fr, 1, &mesh, 1, &pair, &p, &spec, 16, 128, 128, &out, e.stream), want, "tsvpp_convert_mesh_tensor", what);
}

void source_spans(const Env &e) {
    const uint64_t L = TSVPP_SOURCE_SPAN_LIMIT;
    const struct { uint64_t y, uv; int want; const char *what; } cases[] = {
        { L - 1, L - 1, TSVPP_OK, "both planes one byte under the limit" },
        { (1ull << 31) + 1, (1ull << 31) + 1, TSVPP_OK, "both planes just past 2^31" },
        { L, 0, TSVPP_UNSUPPORTED, "the luma plane at the limit" },
        { 0, L, TSVPP_UNSUPPORTED, "the chroma plane at the limit" },
        { L - 1, L, TSVPP_UNSUPPORTED, "luma one byte under, chroma at the limit" },
        { 1ull << 32, 1ull << 32, TSVPP_UNSUPPORTED, "both planes at 2^32" },
    };
    tsvpp_params whole = {};
    whole.dst_width = 64, whole.dst_height = 32, whole.resize_type = TSVPP_BILINEAR, whole.fourcc = TSVPP_RGB24, whole.planes = TSVPP_PLANAR, whole.normalization = 1;
    for (const auto &c : cases) {
        const SpanGeom g = span_geom(16, c.y, c.uv);
        const tsvpp_nv12 fr = { e.y, e.uv, g.py, g.puv, g.w, g.h };
        plain_span_case(e, fr, whole, c.want, c.what);
        frame_span_case(e, fr, c.want, c.what);
        const tsvpp_roi all = { 0, 0, 0, g.w, g.h };
        rois_span_case(e, fr, all, c.want, c.what);
        // the same planes as rows 100 .. 115, columns 64 .. 64 + w of a frame 400 rows high: the crop / box decides, the frame (beyond the limit in every case) does not
        const tsvpp_nv12 big = { e.y, e.uv, g.py, g.puv, g.w + 128, 400 };
        tsvpp_params crop = whole;
        crop.crop_left = 64, crop.crop_top = 100, crop.crop_right = 64 + g.w, crop.crop_bottom = 100 + g.h;
        plain_span_case(e, big, crop, c.want, c.what);
        const tsvpp_roi box = { 0, 64, 100, 64 + g.w, 100 + g.h };
        rois_span_case(e, big, box, c.want, c.what);
        if (c.want == TSVPP_OK) frame_span_case(e, big, TSVPP_UNSUPPORTED, "a frame beyond the limit whatever the request reads of it");
    }
}

// ---- allocation failures: the n-th allocation of a call fails, n = 1, 2, 3 ... until the call succeeds ---------------------------------------------------------
// Every failing call returns a non-OK status; the context it failed in still converts, and is destroyed.  What must not happen: a leak (the stub's live count and
// the leak check at exit), a stale runtime error that the next launch reports, a half-built cache entry.
void allocation_failures(const Env &e) {
    const long held = hc_stub_live(); // this driver's blocks, the shared context's streams and cached tables
    int walked = 0, deepest = 0;
    const size_t stride = g_plain.size() > 64 ? g_plain.size() / 64 : 1; // about 64 requests, spread over the grid's signatures (sorted: every mode and flavour)
    for (size_t idx = 0; idx < g_plain.size(); idx += stride) {
        const Plain &r = g_plain[idx];
        std::vector<tsvpp_nv12> in((size_t)r.n, tsvpp_nv12{ e.y, e.uv, r.py, r.puv, r.w, r.h });
        std::vector<void *> outs((size_t)r.n, e.out + (r.aligned ? 0 : 4));
        for (int n = 1; n <= 24; n++) {
            tsvpp_ctx *ctx = nullptr;
            hc_stub_fail_alloc_after(n);
            int sts = tsvpp_create(1, 2, &ctx); // (two streams: n = 1, 2 fail here)
            void *stream = nullptr;
            if (sts == TSVPP_OK) sts = tsvpp_consumer_stream(ctx, "a", &stream);
            int step = 0;
            if (sts == TSVPP_OK) step = 1, sts = tsvpp_prepare_batch(ctx, &r.p, r.w, r.h, (n & 1) ? r.n : 0, stream); // (every other depth: the conversion builds its tables itself)
            if (sts == TSVPP_OK) step = 2, sts = tsvpp_convert_batch(ctx, r.n, in.data(), &r.p, outs.data(), stream);
            tsvpp_table *tab = nullptr;
            if (sts == TSVPP_OK) step = 3, sts = tsvpp_table_create(ctx, 131, &tab);
            if (sts == TSVPP_OK) step = 4, sts = tsvpp_table_set(tab, 3, r.n, in.data(), outs.data(), stream);
            if (sts == TSVPP_OK) step = 5, sts = tsvpp_convert_table(ctx, tab, 3, r.n, &r.p, stream);
            hc_stub_fail_alloc_after(0);
            HC_CHECK(sts == TSVPP_OK || sts == (int)hipErrorOutOfMemory || sts == TSVPP_ERROR, "allocation %d failing: step %d answers %d (%s)", n, step, sts, tsvpp_strerror(sts));
            if (ctx) { // the context still converts, tables and all
                void *s = nullptr;
                HC_CHECK(tsvpp_consumer_stream(ctx, "a", &s) == TSVPP_OK, "the consumer's stream after a failure");
                const int again = tsvpp_convert_batch(ctx, r.n, in.data(), &r.p, outs.data(), s);
                HC_CHECK(again == TSVPP_OK, "request %zu: after allocation %d failed in step %d (status %d) the context answers %d (%s) to the same conversion", idx, n, step, sts, again,
                         tsvpp_strerror(again));
                if (!tab) HC_CHECK(tsvpp_table_create(ctx, 131, &tab) == TSVPP_OK, "table_create after a failure");
                if (tab) {
                    HC_CHECK(tsvpp_table_set(tab, 3, r.n, in.data(), outs.data(), s) == TSVPP_OK, "table_set after a failure (allocation %d, step %d)", n, step);
                    HC_CHECK(tsvpp_convert_table(ctx, tab, 3, r.n, &r.p, s) == TSVPP_OK, "convert_table after a failure (allocation %d, step %d)", n, step);
                }
                if (n & 2) {
                    tsvpp_table_destroy(tab);
                    tsvpp_destroy(ctx);
                } else {
                    tsvpp_destroy(ctx);
                    tsvpp_table_destroy(tab);
                }
            } else {
                HC_CHECK(sts != TSVPP_OK && !tab, "no context and no error");
            }
            HC_CHECK(hc_stub_live() == held, "allocation %d failing in step %d leaves %ld blocks, streams and events of the stub's behind", n, step, hc_stub_live() - held);
            if (n > deepest) deepest = n;
            if (sts == TSVPP_OK) break; // nothing failed any more: the call needs fewer than n allocations (or goes on without the one that failed)
        }
        walked++;
    }
    HC_CHECK(walked >= (g_plain.size() > 64 ? 60 : 1) && deepest >= 6, "%d requests walked, the deepest to allocation %d", walked, deepest);
    std::fprintf(stderr, "hc_requests: allocation failures: %d requests, up to %d allocations deep\n", walked, deepest);
}

} // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: hc_requests <request file>\n");
        return 2;
    }
    setenv("TSVPP_DEBUG_KNOBS", "1", 1); // before the context is created: tsvpp_debug_last_launch answers for it
    std::ifstream file(argv[1]);
    if (!file) {
        std::fprintf(stderr, "hc_requests: cannot read %s\n", argv[1]);
        return 2;
    }
    Env e;
    e.y = hc::dev_alloc(4096), e.uv = hc::dev_alloc(4096), e.out = hc::dev_alloc(4096);
    HC_CHECK(tsvpp_create(1, 2, &e.ctx) == TSVPP_OK && e.ctx, "tsvpp_create on the stub's second device");
    if (!e.ctx) return 3;
    HC_CHECK(tsvpp_consumer_stream(e.ctx, "requests", &e.stream) == TSVPP_OK && e.stream, "the consumer's stream");
    HC_CHECK(hc::current_device() == 0, "tsvpp_create left the thread on device %d", hc::current_device());
    int counts[4] = { 0, 0, 0, 0 };
    std::string line;
    while (std::getline(file, line)) {
        if (line.empty() || line[0] == '#') continue;
        Tokens k(line);
        const std::string kind = k.word();
        if (kind == "plain") {
            const Plain r = parse_plain(k);
            g_plain.push_back(r);
            run_plain(e, r, line.c_str());
            counts[0]++;
        } else if (kind == "tile") {
            run_tile(e, k);
            counts[1]++;
        } else if (kind == "remap" || kind == "mesh") {
            run_map(e, k, kind == "mesh");
            counts[kind == "mesh" ? 3 : 2]++;
        } else {
            HC_CHECK(false, "unknown request kind %s", kind.c_str());
        }
    }
    std::fprintf(stderr, "hc_requests: %d plain, %d tile, %d remap, %d mesh requests\n", counts[0], counts[1], counts[2], counts[3]);
    HC_CHECK(counts[0] > 0 && counts[1] > 0 && counts[2] > 0 && counts[3] > 0, "the request file holds every kind of request");
    helpers();
    refusals(e);
    source_spans(e);
    allocation_failures(e);
    tsvpp_destroy(e.ctx);
    (void)hipFree(e.y);
    (void)hipFree(e.uv);
    (void)hipFree(e.out);
    return hc::verdict("hc_requests");
}
