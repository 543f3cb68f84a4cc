// hc_capture.cpp -- host check, single thread (AddressSanitizer + UndefinedBehaviorSanitizer): the library's behaviour while a stream is being captured into a
// graph, on the stub runtime (stub_hip.cpp) whose streams carry a "capturing" flag.  While it is set the stub answers hipMalloc / hipFree / hipMemcpy /
// hipStreamSynchronize with the capture error and an event recorded on the stream cannot be waited for -- what the real runtime does.
//   1. every convert entry point the GPU suite captures runs under capture, then again after it, on the same context;
//   2. tsvpp_table_set under capture is refused (include/tsvpp.h) and leaves the table's staging slots usable: more than four further sets succeed;
//   3. refusals and uploads in turn never leave a staging slot busy, and a slot whose event can no longer be waited for is reset: the table goes on working;
//   4. a request first seen during capture launches, on a later ordinary call, what a fresh context launches for it (tsvpp_debug_last_launch lines): the replay
//      cache does not remember a launch for which a table build was declined.
// Exit status 0 only without a failed assertion and without a stub violation.
#include <string>
#include <vector>

#include "hc_common.h"

namespace {

struct Request {
    int w, h, pitch, dw, dh, rt, fcc, planes, norm;
};

struct Buffers { // every "frame" of a call shares one pair of planes and one output: nothing is ever executed
    uint8_t *y, *uv, *out;
    Buffers() : y(hc::dev_alloc(4096)), uv(hc::dev_alloc(4096)), out(hc::dev_alloc(4096)) {}
    ~Buffers() {
        (void)hipFree(y);
        (void)hipFree(uv);
        (void)hipFree(out);
    }
};

tsvpp_params params_of(const Request &r) {
    tsvpp_params p = {};
    p.dst_width = r.dw;
    p.dst_height = r.dh;
    p.resize_type = r.rt;
    p.fourcc = r.fcc;
    p.planes = r.planes;
    p.normalization = r.norm;
    return p;
}

// one conversion of `r`; the line of tsvpp_debug_last_launch in `line` ("" if it recorded nothing)
int convert(tsvpp_ctx *ctx, const Buffers &b, const Request &r, void *stream, std::string &line) {
    const tsvpp_nv12 in = { b.y, b.uv, r.pitch, r.pitch, r.w, r.h };
    const tsvpp_params p = params_of(r);
    const int sts = tsvpp_convert(ctx, &in, &p, b.out, stream);
    char buf[512];
    line = tsvpp_debug_last_launch(buf, sizeof(buf)) == TSVPP_OK ? buf : "";
    return sts;
}

tsvpp_ctx *fresh_context(void **stream) {
    tsvpp_ctx *ctx = nullptr;
    HC_CHECK(tsvpp_create(0, 1, &ctx) == TSVPP_OK && ctx, "tsvpp_create");
    if (!ctx) std::exit(3);
    HC_CHECK(tsvpp_consumer_stream(ctx, "capture", stream) == TSVPP_OK && *stream, "tsvpp_consumer_stream");
    return ctx;
}

// (4) and the single-frame part of (1)
void replay_after_capture(const Buffers &b) {
    // requests whose first launch builds a device table where it may: geometry tables of the 2x2-tap kernel (uint8, dyadic weights), the BICUBIC column tables
    // (non-dyadic ratios), AREA weight and divisor tables
    const Request reqs[] = {
        { 1920, 1080, 2048, 1536, 864, TSVPP_BILINEAR, TSVPP_RGB24, TSVPP_PLANAR, 0 }, { 1920, 1080, 2048, 1536, 864, TSVPP_BILINEAR, TSVPP_BGR24, TSVPP_MERGED, 0 },
        { 1280, 720, 1280, 1024, 576, TSVPP_BILINEAR, TSVPP_RGB24, TSVPP_PLANAR, 0 },  { 1920, 1080, 2048, 1280, 720, TSVPP_BILINEAR, TSVPP_RGB24, TSVPP_PLANAR, 1 },
        { 1920, 1080, 2048, 854, 480, TSVPP_BICUBIC, TSVPP_RGB24, TSVPP_PLANAR, 1 },   { 1920, 1080, 2048, 1366, 768, TSVPP_BICUBIC, TSVPP_RGB24, TSVPP_MERGED, 0 },
        { 1280, 720, 1280, 300, 300, TSVPP_BICUBIC, TSVPP_BGR24, TSVPP_PLANAR, 1 },    { 1920, 1080, 2048, 800, 450, TSVPP_AREA, TSVPP_RGB24, TSVPP_PLANAR, 1 },
        { 1920, 1080, 2048, 640, 360, TSVPP_AREA, TSVPP_RGB24, TSVPP_MERGED, 0 },      { 1920, 1080, 2048, 2880, 1620, TSVPP_AREA, TSVPP_RGB24, TSVPP_PLANAR, 0 },
    };
    int differed_under_capture = 0;
    for (const Request &r : reqs) {
        std::string fresh, captured, later, again;
        {
            void *s = nullptr;
            tsvpp_ctx *ctx = fresh_context(&s);
            HC_CHECK(convert(ctx, b, r, s, fresh) == TSVPP_OK && !fresh.empty(), "a fresh context converts %dx%d -> %dx%d type %d", r.w, r.h, r.dw, r.dh, r.rt);
            tsvpp_destroy(ctx);
        }
        void *s = nullptr;
        tsvpp_ctx *ctx = fresh_context(&s);
        hc_stub_set_capturing((hipStream_t)s, 1);
        const int sc = convert(ctx, b, r, s, captured); // first seen while capturing: never allocates; a first AREA scale may be refused (it needs its weight table)
        HC_CHECK(sc == TSVPP_OK || r.rt == TSVPP_AREA, "status %d under capture for %dx%d -> %dx%d type %d", sc, r.w, r.h, r.dw, r.dh, r.rt);
        hc_stub_set_capturing((hipStream_t)s, 0);
        if (sc == TSVPP_OK && captured != fresh) differed_under_capture++;
        const int sl = convert(ctx, b, r, s, later);
        HC_CHECK(sl == TSVPP_OK, "the same call after the capture: status %d (%s), %d under capture", sl, tsvpp_strerror(sl), sc);
        HC_CHECK(later == fresh, "%dx%d -> %dx%d type %d, first seen during capture, later launches\n    %s\n  where a fresh context launches\n    %s", r.w, r.h, r.dw,
                 r.dh, r.rt, later.c_str(), fresh.c_str());
        HC_CHECK(convert(ctx, b, r, s, again) == TSVPP_OK && again == fresh, "... and once more (the replay hit):\n    %s", again.c_str());
        tsvpp_destroy(ctx);
    }
    // the check above can see a remembered fallback only if capture changes some launch at all
    HC_CHECK(differed_under_capture > 0, "no request of the list launches anything else under capture: the list no longer tests the replay cache");
}

// an AREA request whose weight tables are cached but whose divisor table is not: built after the capture, not during it
void area_divisor_after_capture(const Buffers &b) {
    void *s = nullptr;
    tsvpp_ctx *ctx = fresh_context(&s);
    std::string line;
    const Request warm = { 1920, 1080, 2048, 800, 432, TSVPP_AREA, TSVPP_RGB24, TSVPP_PLANAR, 1 }; // ratios 2.4 (float weights) and 2.5
    const Request both = { 1920, 1080, 2048, 800, 450, TSVPP_AREA, TSVPP_RGB24, TSVPP_PLANAR, 1 }; // 2.4 on both axes: weight tables cached, divisors not
    HC_CHECK(convert(ctx, b, warm, s, line) == TSVPP_OK, "AREA warm-up");
    const int before = tsvpp_debug_area_tables(ctx);
    hc_stub_set_capturing((hipStream_t)s, 1);
    HC_CHECK(convert(ctx, b, both, s, line) == TSVPP_OK, "AREA with cached weight tables converts under capture");
    HC_CHECK(tsvpp_debug_area_tables(ctx) == before, "nothing was cached during the capture");
    hc_stub_set_capturing((hipStream_t)s, 0);
    HC_CHECK(convert(ctx, b, both, s, line) == TSVPP_OK, "AREA after the capture");
    HC_CHECK(tsvpp_debug_area_tables(ctx) > before, "the divisor table a capture declined is built by the next ordinary call (%d tables before, %d now)", before,
             tsvpp_debug_area_tables(ctx));
    tsvpp_destroy(ctx);
}

// (1): the entry points that take records by value -- legal under capture by the header's words -- and the two-pass formats after tsvpp_prepare_batch
void entry_points(const Buffers &b) {
    void *s = nullptr;
    tsvpp_ctx *ctx = fresh_context(&s);
    const tsvpp_nv12 frame = { b.y, b.uv, 64, 64, 64, 36 };
    void *outs[2] = { b.out, b.out + 2048 };
    tsvpp_params p = {};
    p.dst_width = 16;
    p.dst_height = 8;
    p.resize_type = TSVPP_BILINEAR;
    p.fourcc = TSVPP_RGB24;
    p.planes = TSVPP_PLANAR;
    p.normalization = 1;
    const tsvpp_roi rois[2] = { { 0, 0, 0, 32, 16 }, { 0, 3, 2, 35, 30 } };
    const tsvpp_rect rects[2] = { { 0, 0, 16, 8 }, { 2, 2, 8, 4 } };
    const tsvpp_nv12 two[2] = { frame, frame };
    const tsvpp_warp warps[2] = { { 0, { 4.f, 0.f, 0.f, 0.f, 4.5f, 0.f } }, { 0, { 2.f, 1.f, -3.f, -1.f, 2.f, 9.f } } };
    const tsvpp_persp persps[2] = { { 0, { 4.f, 0.f, 0.f, 0.f, 4.5f, 0.f, 0.f, 0.f, 1.f } }, { 0, { 4.f, 0.2f, 1.f, 0.1f, 4.f, 2.f, 0.001f, 0.002f, 1.f } } };
    const tsvpp_tensor_spec spec = { TSVPP_F16, { 0.485f, 0.456f, 0.406f }, { 4.f, 4.f, 4.f } };
    float *map = (float *)hc::dev_alloc((size_t)16 * 8 * 2 * sizeof(float)), *mesh = (float *)hc::dev_alloc((size_t)5 * 3 * 2 * sizeof(float));
    const tsvpp_map maps[1] = { { map, 0, 0 } };
    const tsvpp_mesh meshes[1] = { { mesh, 0, 2, 2, 0 } }; // 4 x 4 cells: 5 x 3 control points
    const tsvpp_remap remaps[2] = { { 0, 0 }, { 0, 0 } };
    tsvpp_params area = p, uyvy = p;
    area.resize_type = TSVPP_AREA;
    uyvy.fourcc = TSVPP_UYVY;
    uyvy.normalization = 0;
    uyvy.dst_width = 48;
    uyvy.dst_height = 20;
    HC_CHECK(tsvpp_prepare_batch(ctx, &uyvy, 64, 36, 2, s) == TSVPP_OK, "prepare_batch sizes the scratch of the two-pass formats ahead of the capture");
    for (int pass = 0; pass < 3; pass++) { // captured, then twice outside
        hc_stub_set_capturing((hipStream_t)s, pass == 0);
        const char *when = pass == 0 ? "under capture" : "after the capture";
        HC_CHECK(tsvpp_convert_batch(ctx, 2, two, &uyvy, outs, s) == TSVPP_OK, "convert_batch UYVY behind a resize %s", when);
        HC_CHECK(tsvpp_convert_batch(ctx, 2, two, &p, outs, s) == TSVPP_OK, "convert_batch %s", when);
        HC_CHECK(tsvpp_convert_rois(ctx, 1, &frame, 2, rois, &p, outs, s) == TSVPP_OK, "convert_rois %s", when);
        HC_CHECK(tsvpp_convert_rois_area(ctx, 1, &frame, 2, rois, &area, outs, s) == TSVPP_OK, "convert_rois_area %s", when);
        HC_CHECK(tsvpp_convert_rois_tensor(ctx, 1, &frame, 2, rois, &p, &spec, outs, s) == TSVPP_OK, "convert_rois_tensor %s", when);
        HC_CHECK(tsvpp_convert_letterbox(ctx, 2, two, &p, rects, 114, 128, 128, outs, s) == TSVPP_OK, "convert_letterbox %s", when);
        HC_CHECK(tsvpp_convert_letterbox_tensor(ctx, 2, two, &p, &spec, nullptr, 114, 128, 128, outs, s) == TSVPP_OK, "convert_letterbox_tensor %s", when);
        HC_CHECK(tsvpp_convert_warp(ctx, 1, &frame, 2, warps, &p, -1, -1, -1, outs, s) == TSVPP_OK, "convert_warp %s", when);
        HC_CHECK(tsvpp_convert_perspective(ctx, 1, &frame, 2, persps, &p, 16, 128, 128, outs, s) == TSVPP_OK, "convert_perspective %s", when);
        HC_CHECK(tsvpp_convert_remap(ctx, 1, &frame, 1, maps, 2, remaps, &p, -1, -1, -1, outs, s) == TSVPP_OK, "convert_remap %s", when);
        HC_CHECK(tsvpp_convert_mesh(ctx, 1, &frame, 1, meshes, 2, remaps, &p, 0, 128, 128, outs, s) == TSVPP_OK, "convert_mesh %s", when);
        HC_CHECK(tsvpp_convert_mesh_tensor(ctx, 1, &frame, 1, meshes, 2, remaps, &p, &spec, -1, -1, -1, outs, s) == TSVPP_OK, "convert_mesh_tensor %s", when);
    }
    HC_CHECK(tsvpp_consumer_synchronize(ctx, "capture") == TSVPP_OK, "consumer_synchronize after the capture");
    (void)hipFree(map);
    (void)hipFree(mesh);
    tsvpp_destroy(ctx);
}

// (2) and (3), and tsvpp_convert_table under capture
void tables(const Buffers &b) {
    void *s = nullptr;
    tsvpp_ctx *ctx = fresh_context(&s);
    tsvpp_table *tab = nullptr;
    HC_CHECK(tsvpp_table_create(ctx, 16, &tab) == TSVPP_OK && tab, "table_create");
    tsvpp_nv12 in[16];
    void *outs[16];
    for (int i = 0; i < 16; i++) {
        in[i] = tsvpp_nv12{ b.y, b.uv, 64, 64, 64, 36 };
        outs[i] = b.out;
    }
    tsvpp_params p = {};
    p.dst_width = 32;
    p.dst_height = 18;
    p.resize_type = TSVPP_BILINEAR;
    p.fourcc = TSVPP_RGB24;
    HC_CHECK(tsvpp_table_set(tab, 0, 16, in, outs, s) == TSVPP_OK, "table_set before the capture");
    HC_CHECK(tsvpp_prepare_batch(ctx, &p, 64, 36, 16, s) == TSVPP_OK, "prepare_batch");
    hc_stub_set_capturing((hipStream_t)s, 1);
    HC_CHECK(tsvpp_convert_table(ctx, tab, 2, 9, &p, s) == TSVPP_OK, "convert_table under capture");
    // include/tsvpp.h: tsvpp_table_set is refused on a capturing stream, before it touches a staging slot
    for (int k = 0; k < 6; k++) HC_CHECK(tsvpp_table_set(tab, k, 2, in, outs, s) == TSVPP_UNSUPPORTED, "table_set under capture is TSVPP_UNSUPPORTED (call %d)", k);
    hc_stub_set_capturing((hipStream_t)s, 0);
    for (int k = 0; k < 9; k++) HC_CHECK(tsvpp_table_set(tab, k, 3, in, outs, s) == TSVPP_OK, "table_set number %d after the capture", k);
    HC_CHECK(tsvpp_convert_table(ctx, tab, 0, 16, &p, s) == TSVPP_OK, "convert_table after the capture");
    // (3) refusals and uploads in turn: a refusal never leaves a slot busy behind it
    void *s2 = nullptr;
    HC_CHECK(tsvpp_consumer_stream(ctx, "capture", &s2) == TSVPP_OK && s2 == s, "one consumer, one stream");
    for (int round = 0; round < 3; round++) {
        hc_stub_set_capturing((hipStream_t)s, 1);
        HC_CHECK(tsvpp_table_set(tab, 0, 1, in, outs, s) == TSVPP_UNSUPPORTED, "refused again (round %d)", round);
        hc_stub_set_capturing((hipStream_t)s, 0);
        for (int k = 0; k < 5; k++) HC_CHECK(tsvpp_table_set(tab, k, 1, in, outs, s) == TSVPP_OK, "five sets after a refusal (round %d, %d)", round, k);
    }
    // a slot whose event can no longer be waited for: the upload that finds it reports the error once, the slot is reset, and the table goes on working -- every
    // slot comes round twice more
    hc_stub_poison_next_wait();
    const int failed = tsvpp_table_set(tab, 0, 1, in, outs, s);
    HC_CHECK(failed > 0, "the upload that meets the unwaitable event reports the runtime's error: %d", failed);
    for (int k = 0; k < 9; k++) HC_CHECK(tsvpp_table_set(tab, k, 1, in, outs, s) == TSVPP_OK, "table_set number %d after a failed event wait", k);
    HC_CHECK(tsvpp_convert_table(ctx, tab, 0, 16, &p, s) == TSVPP_OK, "convert_table after a failed event wait (no stale error either)");
    tsvpp_table_destroy(tab);
    tsvpp_destroy(ctx);
}

} // namespace

int main() {
    setenv("TSVPP_DEBUG_KNOBS", "1", 1); // tsvpp_debug_last_launch answers only under the gate
    {
        Buffers b;
        entry_points(b);
        tables(b);
        area_divisor_after_capture(b);
        replay_after_capture(b);
    }
    return hc::verdict("hc_capture");
}
