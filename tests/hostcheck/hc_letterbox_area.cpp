// hc_letterbox_area.cpp -- host check, single thread (AddressSanitizer + UndefinedBehaviorSanitizer): tsvpp_convert_letterbox_area / tsvpp_describe_letterbox_area,
// with and without a tensor spec, tsvpp_letterbox_area_rows and VideoProcessor::ConvertLetterboxArea on the stub runtime (stub_hip.cpp).  Launches are recorded and
// range-checked by the stub, never executed.  The requests are stated below (no input file).
// Every request goes through describe (outputs aligned / not) and convert with all outputs aligned and with none, then on a capturing stream and with the n-th
// allocation from now failing for n = 1 .. 4: the path allocates nothing, so every one succeeds and the stub's count of live blocks does not move.  The launches
// the stub saw are the described ones: ceil(n / 32) of them, the first grid, 128 threads, in order, the dynamic LDS = the described lds= without the store side's
// static slab.  Then every refusal on the live context (no launch goes out), and the adapter: its two methods launch what the entry point launches.
// Exit status 0 only without a failed assertion, a stub violation, or anything the stub still holds at the end.
#include <array>
#include <cstring>
#include <string>
#include <vector>

#include "VideoProcessor.h"
#include "hc_common.h"

namespace {

struct Request {
    const char *what;
    int dst_w, dst_h, fourcc, planes, normalization, dtype; // dtype -1: no spec
    std::vector<std::array<int, 3>> geo;                    // w, h, pitch per frame
    std::vector<tsvpp_rect> rects;                          // empty: the default rectangles
};

struct Live {
    tsvpp_params p = {};
    tsvpp_tensor_spec spec = { TSVPP_F16, { 0.485f, 0.456f, 0.406f }, { 4.0f, 4.5f, 5.0f } };
    bool tensor = false;
    std::vector<tsvpp_nv12> frames;
    std::vector<tsvpp_rect> rects;
    std::vector<uint8_t *> blocks;
    uint8_t *out = nullptr;
    size_t stride = 0, esz = 1;

    const tsvpp_rect *rc() const { return rects.empty() ? nullptr : rects.data(); }
    int n() const { return (int)frames.size(); }
    int describe(int aligned, char *buf, size_t len) const {
        return tsvpp_describe_letterbox_area(&p, tensor ? &spec : nullptr, n(), frames.data(), rc(), aligned, buf, len);
    }
    int convert(tsvpp_ctx *ctx, void *const *outs, void *stream, int pad_y = 114) const {
        return tsvpp_convert_letterbox_area(ctx, n(), frames.data(), &p, tensor ? &spec : nullptr, rc(), pad_y, 128, 128, outs, stream);
    }
    std::vector<void *> outs(bool aligned) const {
        std::vector<void *> o;
        for (int i = 0; i < n(); i++) o.push_back(out + (size_t)i * stride + (aligned ? 0 : esz));
        return o;
    }
    ~Live() {
        for (uint8_t *b : blocks) (void)hipFree(b);
        if (out) (void)hipFree(out);
    }
};

void make(const Request &q, Live &r) {
    r.p.dst_width = q.dst_w, r.p.dst_height = q.dst_h, r.p.resize_type = TSVPP_AREA, r.p.fourcc = q.fourcc, r.p.planes = q.planes, r.p.normalization = q.normalization;
    r.tensor = q.dtype >= 0;
    r.spec.dtype = r.tensor ? q.dtype : TSVPP_F32;
    r.esz = r.tensor ? (q.dtype == TSVPP_F32 ? 4 : 2) : (q.normalization ? 4 : 1);
    for (const auto &g : q.geo) {
        uint8_t *y = hc::dev_alloc((size_t)g[1] * g[2]), *uv = hc::dev_alloc((size_t)(g[1] / 2) * g[2]);
        r.blocks.push_back(y), r.blocks.push_back(uv);
        r.frames.push_back(tsvpp_nv12{ y, uv, g[2], g[2], g[0], g[1] });
    }
    r.rects = q.rects;
    const size_t bytes = (size_t)(q.fourcc == TSVPP_Y800 ? 1 : 3) * q.dst_w * q.dst_h * r.esz;
    r.stride = (bytes + 16 + 255) & ~(size_t)255;
    r.out = hc::dev_alloc(r.stride * r.frames.size());
}

// what the stub saw of one convert call against the described launch
void check_launches(const Live &r, const char *desc, const char *what, int captured) {
    const long want = (r.n() + TSVPP_MAX_LETTERBOX - 1) / TSVPP_MAX_LETTERBOX;
    HC_CHECK((long)hc_stub_launch_count() == want && want == hc::number_of(desc, "launches"), "%s: %zu launches, expected %ld, described %s", what, hc_stub_launch_count(), want, desc);
    const long tiles = (long)((r.p.dst_width + 31) / 32) * ((r.p.dst_height + 31) / 32);
    long grids = 0;
    for (size_t l = 0; l < hc_stub_launch_count(); l++) {
        const HcLaunch &k = *hc_stub_launch(l);
        grids += k.grid[0];
        HC_CHECK(k.block[0] == 128 && k.block[1] == 1 && k.grid[1] == 1 && !k.any_order && !k.refused && k.captured == captured,
                 "%s: launch %zu: block %u x %u, grid y %u, any_order %d, refused %d, captured %d", what, l, k.block[0], k.block[1], k.grid[1], k.any_order, k.refused, k.captured);
        HC_CHECK(std::string(k.name).find("vpp_letterbox_area_kernel") != std::string::npos, "%s: launch %zu is %s", what, l, k.name);
    }
    HC_CHECK(grids == tiles * r.n(), "%s: the grids sum to %ld, the canvases' tiles to %ld", what, grids, tiles * r.n());
    if (!hc_stub_launch_count()) return;
    HC_CHECK((long)hc_stub_launch(0)->grid[0] == hc::number_of(desc, "grid"), "%s: the first grid is %u, described %s", what, hc_stub_launch(0)->grid[0], desc);
    const long extra = hc::number_of(desc, "lds") - (long)hc_stub_launch(0)->lds; // describe adds the static exchange slab of the kernel's store side
    HC_CHECK(extra == 0 || extra == 3072 || extra == 12288, "%s: the first launch has %zu bytes of dynamic LDS, described %s", what, hc_stub_launch(0)->lds, desc);
}

void run(tsvpp_ctx *ctx, void *stream, const Request &q) {
    Live r;
    make(q, r);
    char desc1[512] = "", desc0[512] = "";
    const int d1 = r.describe(1, desc1, sizeof(desc1)), d0 = r.describe(0, desc0, sizeof(desc0));
    HC_CHECK(d1 == TSVPP_OK && d0 == TSVPP_OK, "%s: describe answers %d / %d", q.what, d1, d0);
    if (d1 != TSVPP_OK || d0 != TSVPP_OK) return;
    HC_CHECK(hc::value_of(desc1, "mode") == "area" && hc::number_of(desc1, "frames") == r.n() && hc::number_of(desc1, "limit") == TSVPP_MAX_LETTERBOX &&
                 hc::value_of(desc1, "kernel").find(r.tensor ? "vpp_letterbox_area_tensor<" : "vpp_letterbox_area<") == 0 && hc::number_of(desc1, "chain") >= 0,
             "%s: describe line: %s", q.what, desc1);
    const long held = hc_stub_live();
    for (int aligned = 1; aligned >= 0; aligned--) {
        const std::vector<void *> outs = r.outs(aligned != 0);
        hc_stub_clear_launches();
        const int cs = r.convert(ctx, outs.data(), stream);
        HC_CHECK(cs == TSVPP_OK, "%s: convert, aligned %d: %d (%s)", q.what, aligned, cs, tsvpp_strerror(cs));
        if (cs == TSVPP_OK) check_launches(r, aligned ? desc1 : desc0, aligned ? "aligned" : "unaligned", 0);
    }
    const std::vector<void *> outs = r.outs(true);
    // on a capturing stream: no allocation, no copy, no synchronisation -- the stub would answer each with the capture error
    hc_stub_set_capturing((hipStream_t)stream, 1);
    hc_stub_clear_launches();
    const int cap = r.convert(ctx, outs.data(), stream);
    hc_stub_set_capturing((hipStream_t)stream, 0);
    HC_CHECK(cap == TSVPP_OK, "%s: convert on a capturing stream: %d (%s)", q.what, cap, tsvpp_strerror(cap));
    if (cap == TSVPP_OK) check_launches(r, desc1, "capturing", 1);
    // with the n-th allocation from now failing, at every depth: there is none to fail
    for (long depth = 1; depth <= 4; depth++) {
        hc_stub_fail_alloc_after(depth);
        hc_stub_clear_launches();
        const int oom = r.convert(ctx, outs.data(), stream);
        hc_stub_fail_alloc_after(0);
        HC_CHECK(oom == TSVPP_OK, "%s: convert with allocation %ld failing: %d (%s): the path allocates", q.what, depth, oom, tsvpp_strerror(oom));
        if (oom == TSVPP_OK) check_launches(r, desc1, "failing allocation", 0);
    }
    HC_CHECK(hc_stub_live() == held, "%s: the conversions left %ld blocks, streams or events of the stub's behind", q.what, hc_stub_live() - held);
    HC_CHECK(hc::current_device() == 0, "the thread ends on device %d", hc::current_device());

    // refusals on the live context: nothing goes out
    hc_stub_clear_launches();
    std::vector<void *> hole = outs;
    hole[hole.size() / 2] = nullptr;
    HC_CHECK(r.convert(ctx, hole.data(), stream) == TSVPP_ERROR && r.convert(nullptr, outs.data(), stream) == TSVPP_ERROR && r.convert(ctx, nullptr, stream) == TSVPP_ERROR,
             "%s: a null output, a null context, null outs", q.what);
    {
        Live bad;
        make(q, bad);
        const std::vector<void *> o = bad.outs(true);
        bad.frames[0].uv = nullptr;
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR, "%s: a null plane", q.what);
        bad.frames[0].uv = bad.blocks[1];
        for (int rt : { (int)TSVPP_NEAREST, (int)TSVPP_BILINEAR, (int)TSVPP_BICUBIC, 9 }) {
            bad.p.resize_type = rt;
            HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_UNSUPPORTED, "%s: resize type %d", q.what, rt);
        }
        bad.p.resize_type = TSVPP_AREA;
        bad.p.crop_right = 2;
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR, "%s: a crop", q.what);
        bad.p.crop_right = 0;
        bad.rects.assign(bad.frames.size(), tsvpp_rect{ 0, 0, q.dst_w, q.dst_h });
        bad.rects[0] = tsvpp_rect{ 0, 0, q.dst_w + 2, 2 };
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_ERROR, "%s: a rectangle outside the canvas", q.what);
        bad.rects[0] = tsvpp_rect{ 0, 1, 2, 2 };
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED, "%s: an odd rectangle", q.what);
        // the limit of 40 taps: the first frame (its planes hold at least 84 x 64) as 84 x 64 and as 80 x 64 into 2 x 2
        bad.frames[0].width = 84, bad.frames[0].height = 64;
        bad.rects[0] = tsvpp_rect{ 0, 0, 2, 2 }; // ratio 42 on x
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_UNSUPPORTED, "%s: 42 taps", q.what);
        bad.frames[0].width = 80; // ratio 40 on x, 32 on y
        HC_CHECK(bad.describe(1, desc0, sizeof(desc0)) == TSVPP_OK && hc::value_of(desc0, "taps").find("40x") == 0, "%s: 40 taps pass: %s", q.what, desc0);
        HC_CHECK(bad.convert(ctx, o.data(), stream, 300) == TSVPP_ERROR, "%s: a pad of 300", q.what);
        if (bad.tensor) {
            bad.spec.scale[0] = 0.0f;
            HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_ERROR, "%s: a scale of zero", q.what);
            bad.spec.scale[0] = 1.0f;
            bad.spec.dtype = 7;
            HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED, "%s: an unknown dtype", q.what);
            bad.spec.dtype = TSVPP_F16;
            const std::vector<void *> odd = bad.outs(false);
            std::vector<void *> off1 = odd;
            for (void *&v : off1) v = (uint8_t *)v - bad.esz + 1; // one byte past a boundary: not aligned to the element
            HC_CHECK(bad.convert(ctx, off1.data(), stream) == TSVPP_ERROR, "%s: outputs off the element's alignment", q.what);
        }
    }
    HC_CHECK(hc_stub_launch_count() == 0, "%s: the refusals launched %zu kernels", q.what, hc_stub_launch_count());
}

// the adapter's two methods launch what the entry point launches
void adapter(tsvpp_ctx *ctx, void *stream, const Request &q) {
    Live r;
    make(q, r);
    const std::vector<void *> outs = r.outs(true);
    hc_stub_clear_launches();
    HC_CHECK(r.convert(ctx, outs.data(), stream) == TSVPP_OK && hc_stub_launch_count() >= 1, "%s: the entry point", q.what);
    std::vector<HcLaunch> want;
    for (size_t l = 0; l < hc_stub_launch_count(); l++) want.push_back(*hc_stub_launch(l));

    VideoProcessor vpp;
    HC_CHECK(vpp.Init(nullptr, 2, false, 0) == VREADER_OK, "VideoProcessor::Init");
    std::vector<AVFrame> av(r.frames.size());
    std::vector<AVFrame *> in;
    for (size_t f = 0; f < av.size(); f++) {
        av[f].data[0] = (uint8_t *)r.frames[f].y, av[f].data[1] = (uint8_t *)r.frames[f].uv;
        av[f].linesize[0] = r.frames[f].pitch_y, av[f].linesize[1] = r.frames[f].pitch_uv;
        av[f].width = r.frames[f].width, av[f].height = r.frames[f].height;
        in.push_back(&av[f]);
    }
    FrameParameters fp(ResizeOptions(q.dst_w, q.dst_h), ColorOptions((FourCC)q.fourcc));
    fp.resize.type = ResizeType::AREA;
    fp.color.planesPos = (Planes)q.planes;
    fp.color.normalization = q.normalization != 0;
    hc_stub_clear_launches();
    const int sts = r.tensor ? vpp.ConvertLetterboxArea(in.data(), r.n(), r.rc(), 114, 128, 128, outs.data(), fp, &r.spec, "hc")
                             : vpp.ConvertLetterboxArea(in.data(), r.n(), r.rc(), 114, 128, 128, outs.data(), fp, "hc");
    HC_CHECK(sts == VREADER_OK && hc_stub_launch_count() == want.size(), "%s: ConvertLetterboxArea: %d, %zu launches, the entry point %zu", q.what, sts, hc_stub_launch_count(), want.size());
    for (size_t l = 0; l < want.size() && l < hc_stub_launch_count(); l++) {
        const HcLaunch &k = *hc_stub_launch(l);
        HC_CHECK(k.fn == want[l].fn && k.grid[0] == want[l].grid[0] && k.block[0] == want[l].block[0] && k.lds == want[l].lds && !k.refused,
                 "%s: launch %zu of the adapter is %s grid %u lds %zu, the entry point's %s grid %u lds %zu", q.what, l, k.name, k.grid[0], k.lds, want[l].name, want[l].grid[0], want[l].lds);
    }
    // a refusal comes back with the reference's status convention, and nothing is launched
    hc_stub_clear_launches();
    fp.resize.type = ResizeType::BILINEAR;
    HC_CHECK(vpp.ConvertLetterboxArea(in.data(), r.n(), r.rc(), 114, 128, 128, outs.data(), fp, "hc") == VREADER_UNSUPPORTED && hc_stub_launch_count() == 0, "%s: the adapter refuses BILINEAR", q.what);
    HC_CHECK(vpp.ConvertLetterboxArea(nullptr, r.n(), r.rc(), 114, 128, 128, outs.data(), fp, "hc") == VREADER_ERROR, "%s: the adapter refuses null inputs", q.what);
    vpp.Close();
}

} // namespace

int main() {
    tsvpp_ctx *ctx = nullptr;
    void *stream = nullptr;
    HC_CHECK(tsvpp_create(1, 1, &ctx) == TSVPP_OK && ctx, "tsvpp_create on the stub's second device");
    if (!ctx) return 3;
    HC_CHECK(tsvpp_consumer_stream(ctx, "letterbox_area", &stream) == TSVPP_OK && stream, "the consumer's stream");
    std::vector<std::array<int, 3>> many;
    for (int k = 0; k < TSVPP_MAX_LETTERBOX + 1; k++) many.push_back(k % 3 == 0 ? std::array<int, 3>{ 128, 72, 192 } : k % 3 == 1 ? std::array<int, 3>{ 72, 128, 96 } : std::array<int, 3>{ 64, 64, 80 });
    const std::vector<Request> requests = {
        { "1080p and 1366 x 768 into 640 x 640, fp32 planar", 640, 640, TSVPP_BGR24, TSVPP_PLANAR, 1, -1, { { 1920, 1080, 2048 }, { 1366, 768, 1408 }, { 320, 180, 320 } }, {} },
        { "33 frames, two launches, uint8 merged", 70, 66, TSVPP_RGB24, TSVPP_MERGED, 0, -1, many, {} },
        { "rectangles of the caller, fp32 merged", 100, 100, TSVPP_RGB24, TSVPP_MERGED, 1, -1, { { 240, 180, 256 }, { 64, 64, 64 } }, { { 0, 12, 100, 76 }, { 14, 2, 20, 10 } } },
        { "narrow canvas, Y800 uint8", 30, 34, TSVPP_Y800, TSVPP_MERGED, 0, -1, { { 128, 72, 128 }, { 64, 64, 64 } }, {} },
        { "fp16 planar tensor", 608, 608, TSVPP_RGB24, TSVPP_PLANAR, 1, TSVPP_F16, { { 1920, 1080, 2048 }, { 128, 72, 192 } }, {} },
        { "bf16 Y800 tensor", 64, 64, TSVPP_Y800, TSVPP_MERGED, 1, TSVPP_BF16, { { 322, 182, 384 }, { 72, 128, 96 } }, {} },
        { "fp32 planar tensor, 33 frames", 64, 64, TSVPP_BGR24, TSVPP_PLANAR, 1, TSVPP_F32, many, {} },
    };
    for (const Request &q : requests) run(ctx, stream, q);
    adapter(ctx, stream, requests[0]);
    adapter(ctx, stream, requests[1]);
    adapter(ctx, stream, requests[4]);

    // the debug export: the jump start is a multiple of the period and the rows are the generator's
    float a[4 * 8], b[4 * 8];
    int taps = 0, start = -1;
    const float scale = 1920.0f / 608.0f;
    HC_CHECK(tsvpp_letterbox_area_rows(scale, 100, 8, a, 32, &taps, &start) == 8 && taps == 4 && start == 57, "rows of 1920 -> 608 at 100: taps %d start %d", taps, start);
    HC_CHECK(tsvpp_roi_area_rows(scale, 100, 8, b, 32, &taps) == 8 && std::memcmp(a, b, sizeof(a)) == 0, "the rows from the jump start are the rows from 0");
    HC_CHECK(tsvpp_letterbox_area_rows(scale, 100, 9, a, 32, &taps, &start) == TSVPP_ERROR && tsvpp_letterbox_area_rows(scale, 0, 8, nullptr, 32, &taps, &start) == TSVPP_ERROR,
             "a buffer that is too small, a null buffer");

    std::fprintf(stderr, "hc_letterbox_area: %zu requests, 3 through the adapter\n", requests.size());
    tsvpp_destroy(ctx);
    return hc::verdict("hc_letterbox_area");
}
