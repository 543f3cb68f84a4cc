// hc_coord_bicubic.cpp -- host check, single thread (AddressSanitizer + UndefinedBehaviorSanitizer): tsvpp_convert_warp_bicubic / tsvpp_describe_warp_bicubic and
// tsvpp_convert_perspective_bicubic / tsvpp_describe_perspective_bicubic, with and without a tensor spec, their footprint exports and the four methods of the
// VideoProcessor adapter, on the stub runtime (stub_hip.cpp).  Launches are recorded and range-checked by the stub, never executed.  The requests are stated
// below (no input file).
// Every request goes through describe (outputs aligned / not) and convert with all outputs aligned and with none, then on a capturing stream and with the n-th
// allocation from now failing for n = 1 .. 4: the paths allocate nothing, so every one succeeds and the stub's count of live blocks does not move.  The launches
// the stub saw are the described ones: ceil(n / 32) of them, the first grid, 128 threads, in order, the dynamic LDS = the described lds= without the store side's
// static slab, the kernel a vpp_coord_bicubic_kernel.  Then every refusal on the live context (no launch goes out), and the adapter: its methods launch what the
// entry points launch.  Exit status 0 only without a failed assertion, a stub violation, or anything the stub still holds at the end.
#include <array>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "VideoProcessor.h"
#include "hc_common.h"

namespace {

struct Request {
    const char *what;
    bool persp;
    int dst_w, dst_h, fourcc, planes, normalization, dtype; // dtype -1: no spec
    int border;                                             // -1: replicate, else the luma component (chroma 128, 128)
    std::vector<std::array<int, 3>> geo;                    // w, h, pitch per frame
    int n;                                                  // outputs: output k samples frame k % frames through item k of the set below
};

// item k of a frame of w x h into dw x dh: a rotation about the centre by 11 k degrees at scale 0.6 + 0.1 (k % 9), every fourth one pushed half out of the
// frame, every seventh far outside; the perspective form adds a keystone to all but every third
void item(int k, int w, int h, int dw, int dh, float m[6], float g[2]) {
    const double ang = 11.0 * k * 3.14159265358979323846 / 180.0, s = 0.6 + 0.1 * (k % 9), c = std::cos(ang), sn = std::sin(ang);
    const double cx = w / 2.0 + (k % 4 == 3 ? -0.5 * w : 0.0) + (k % 7 == 6 ? 5000.0 : 0.0), cy = h / 2.0 + (k % 7 == 6 ? -3000.0 : 0.0);
    const double a = s * c, b = -s * sn, d = s * sn, e = s * c;
    const double v[6] = { a, b, cx - a * dw / 2 - b * dh / 2, d, e, cy - d * dw / 2 - e * dh / 2 };
    for (int i = 0; i < 6; i++) m[i] = (float)v[i];
    g[0] = k % 3 ? (float)(0.3 / dw) : 0.0f;
    g[1] = k % 3 ? (float)(0.15 / dh) : 0.0f;
}

struct Live {
    tsvpp_params p = {};
    tsvpp_tensor_spec spec = { TSVPP_F16, { 0.485f, 0.456f, 0.406f }, { 4.0f, 4.5f, 5.0f } };
    bool tensor = false, persp = false;
    int by = -1, bu = -1, bv = -1;
    std::vector<tsvpp_nv12> frames;
    std::vector<tsvpp_warp> warps;
    std::vector<tsvpp_persp> persps;
    std::vector<uint8_t *> blocks;
    uint8_t *out = nullptr;
    size_t stride = 0, esz = 1;

    int n() const { return (int)(persp ? persps.size() : warps.size()); }
    int nf() const { return (int)frames.size(); }
    const tsvpp_tensor_spec *sp() const { return tensor ? &spec : nullptr; }
    int describe(int aligned, char *buf, size_t len) const {
        return persp ? tsvpp_describe_perspective_bicubic(&p, sp(), nf(), frames.data(), n(), persps.data(), by, bu, bv, aligned, buf, len)
                     : tsvpp_describe_warp_bicubic(&p, sp(), nf(), frames.data(), n(), warps.data(), by, bu, bv, aligned, buf, len);
    }
    int convert(tsvpp_ctx *ctx, void *const *outs, void *stream) const {
        return persp ? tsvpp_convert_perspective_bicubic(ctx, nf(), frames.data(), n(), persps.data(), &p, sp(), by, bu, bv, outs, stream)
                     : tsvpp_convert_warp_bicubic(ctx, nf(), frames.data(), n(), warps.data(), &p, sp(), by, bu, bv, outs, stream);
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
    r.p.dst_width = q.dst_w, r.p.dst_height = q.dst_h, r.p.resize_type = TSVPP_BICUBIC, r.p.fourcc = q.fourcc, r.p.planes = q.planes, r.p.normalization = q.normalization;
    r.tensor = q.dtype >= 0;
    r.persp = q.persp;
    r.spec.dtype = r.tensor ? q.dtype : TSVPP_F32;
    r.esz = r.tensor ? (q.dtype == TSVPP_F32 ? 4 : 2) : (q.normalization ? 4 : 1);
    if (q.border >= 0) r.by = q.border, r.bu = 128, r.bv = 128;
    for (const auto &g : q.geo) {
        uint8_t *y = hc::dev_alloc((size_t)g[1] * g[2]), *uv = hc::dev_alloc((size_t)(g[1] / 2) * g[2]);
        r.blocks.push_back(y), r.blocks.push_back(uv);
        r.frames.push_back(tsvpp_nv12{ y, uv, g[2], g[2], g[0], g[1] });
    }
    for (int k = 0; k < q.n; k++) {
        const int f = k % (int)q.geo.size();
        float m[6], g[2];
        item(k, q.geo[f][0], q.geo[f][1], q.dst_w, q.dst_h, m, g);
        if (q.persp) {
            tsvpp_persp t = {};
            t.frame = f;
            for (int i = 0; i < 6; i++) t.h[i] = m[i];
            t.h[6] = g[0], t.h[7] = g[1], t.h[8] = 1.0f;
            r.persps.push_back(t);
        } else {
            tsvpp_warp t = {};
            t.frame = f;
            for (int i = 0; i < 6; i++) t.m[i] = m[i];
            r.warps.push_back(t);
        }
    }
    const size_t bytes = (size_t)(q.fourcc == TSVPP_Y800 ? 1 : 3) * q.dst_w * q.dst_h * r.esz;
    r.stride = (bytes + 16 + 255) & ~(size_t)255;
    r.out = hc::dev_alloc(r.stride * (size_t)q.n);
}

// what the stub saw of one convert call against the described launch
void check_launches(const Live &r, const char *desc, const char *what, int captured) {
    const int limit = r.persp ? TSVPP_MAX_PERSP : TSVPP_MAX_WARPS;
    const long want = (r.n() + limit - 1) / limit;
    HC_CHECK((long)hc_stub_launch_count() == want && want == hc::number_of(desc, "launches"), "%s: %zu launches, expected %ld, described %s", what, hc_stub_launch_count(), want, desc);
    const long tiles = (long)((r.p.dst_width + 31) / 32) * ((r.p.dst_height + 31) / 32);
    long grids = 0;
    for (size_t l = 0; l < hc_stub_launch_count(); l++) {
        const HcLaunch &k = *hc_stub_launch(l);
        grids += k.grid[0];
        HC_CHECK(k.block[0] == 128 && k.block[1] == 1 && k.grid[1] == 1 && !k.any_order && !k.refused && k.captured == captured,
                 "%s: launch %zu: block %u x %u, grid y %u, any_order %d, refused %d, captured %d", what, l, k.block[0], k.block[1], k.grid[1], k.any_order, k.refused, k.captured);
        HC_CHECK(std::string(k.name).find("vpp_coord_bicubic_kernel") != std::string::npos, "%s: launch %zu is %s", what, l, k.name);
    }
    HC_CHECK(grids == tiles * r.n(), "%s: the grids sum to %ld, the outputs' tiles to %ld", what, grids, tiles * r.n());
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
    const std::string kernel = std::string(q.persp ? "vpp_persp_bicubic" : "vpp_warp_bicubic") + (r.tensor ? "_tensor<" : "<");
    HC_CHECK(hc::value_of(desc1, "mode") == (q.persp ? "persp_bicubic" : "warp_bicubic") && hc::number_of(desc1, "frames") == r.nf() && hc::number_of(desc1, "warps") == r.n() &&
                 hc::number_of(desc1, "limit") == 32 && hc::value_of(desc1, "kernel").find(kernel) == 0 &&
                 hc::value_of(desc1, "border") == (q.border < 0 ? "replicate" : std::to_string(q.border) + ",128,128"),
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
        for (int rt : { (int)TSVPP_NEAREST, (int)TSVPP_BILINEAR, (int)TSVPP_AREA, 9 }) {
            bad.p.resize_type = rt;
            HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_UNSUPPORTED, "%s: resize type %d", q.what, rt);
        }
        bad.p.resize_type = TSVPP_BICUBIC;
        bad.p.crop_right = 2;
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR, "%s: a crop", q.what);
        bad.p.crop_right = 0;
        bad.p.dst_width += 1;
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED, "%s: an odd output width", q.what);
        bad.p.dst_width -= 1;
        bad.by = 300, bad.bu = 0, bad.bv = 0;
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_ERROR, "%s: a border of 300", q.what);
        bad.by = 114, bad.bu = -1, bad.bv = 128;
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR, "%s: a border that mixes -1 and a sample", q.what);
        bad.by = bad.bu = bad.bv = -1;
        float &entry = bad.persp ? bad.persps[0].h[1] : bad.warps[0].m[1];
        int &frame = bad.persp ? bad.persps[0].frame : bad.warps[0].frame;
        const float keep = entry;
        entry = std::nanf("");
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_ERROR, "%s: an entry that is not a number", q.what);
        entry = 33554432.0f;
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_UNSUPPORTED, "%s: an entry of 2^25", q.what);
        entry = keep;
        frame = bad.nf();
        HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_ERROR, "%s: a frame index out of range", q.what);
        frame = 0;
        if (bad.persp) {
            const float g = bad.persps[0].h[6];
            bad.persps[0].h[6] = -1.0f / 16.0f; // the horizon crosses the output
            HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_UNSUPPORTED, "%s: the horizon rule", q.what);
            bad.persps[0].h[6] = g;
        }
        if (bad.tensor) {
            bad.spec.scale[0] = 0.0f;
            HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_ERROR && bad.describe(1, desc0, sizeof(desc0)) == TSVPP_ERROR, "%s: a scale of zero", q.what);
            bad.spec.scale[0] = 1.0f;
            bad.spec.dtype = 7;
            HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED, "%s: an unknown dtype", q.what);
            bad.spec.dtype = q.dtype;
            bad.p.planes = TSVPP_MERGED;
            if (q.fourcc != TSVPP_Y800) HC_CHECK(bad.convert(ctx, o.data(), stream) == TSVPP_UNSUPPORTED, "%s: a merged tensor", q.what);
            bad.p.planes = q.planes;
            std::vector<void *> off1 = bad.outs(false);
            for (void *&v : off1) v = (uint8_t *)v - bad.esz + 1; // one byte past a boundary: not aligned to the element
            HC_CHECK(bad.convert(ctx, off1.data(), stream) == TSVPP_ERROR, "%s: outputs off the element's alignment", q.what);
        }
        HC_CHECK(bad.describe(1, desc0, sizeof(desc0)) == TSVPP_OK, "%s: the request is whole again: %s", q.what, desc0);
    }
    HC_CHECK(hc_stub_launch_count() == 0, "%s: the refusals launched %zu kernels", q.what, hc_stub_launch_count());
}

// the adapter's methods launch what the entry points launch
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
    fp.resize.type = ResizeType::BICUBIC;
    fp.color.planesPos = (Planes)q.planes;
    fp.color.normalization = q.normalization != 0;
    const auto call = [&](AVFrame *const *inputs) {
        if (r.persp)
            return r.tensor ? vpp.ConvertPerspectiveBicubic(inputs, r.nf(), r.persps.data(), r.n(), r.by, r.bu, r.bv, outs.data(), fp, &r.spec, "hc")
                            : vpp.ConvertPerspectiveBicubic(inputs, r.nf(), r.persps.data(), r.n(), r.by, r.bu, r.bv, outs.data(), fp, "hc");
        return r.tensor ? vpp.ConvertWarpBicubic(inputs, r.nf(), r.warps.data(), r.n(), r.by, r.bu, r.bv, outs.data(), fp, &r.spec, "hc")
                        : vpp.ConvertWarpBicubic(inputs, r.nf(), r.warps.data(), r.n(), r.by, r.bu, r.bv, outs.data(), fp, "hc");
    };
    hc_stub_clear_launches();
    const int sts = call(in.data());
    HC_CHECK(sts == VREADER_OK && hc_stub_launch_count() == want.size(), "%s: the adapter: %d, %zu launches, the entry point %zu", q.what, sts, hc_stub_launch_count(), want.size());
    for (size_t l = 0; l < want.size() && l < hc_stub_launch_count(); l++) {
        const HcLaunch &k = *hc_stub_launch(l);
        HC_CHECK(k.fn == want[l].fn && k.grid[0] == want[l].grid[0] && k.block[0] == want[l].block[0] && k.lds == want[l].lds && !k.refused,
                 "%s: launch %zu of the adapter is %s grid %u lds %zu, the entry point's %s grid %u lds %zu", q.what, l, k.name, k.grid[0], k.lds, want[l].name, want[l].grid[0], want[l].lds);
    }
    // a refusal comes back with the reference's status convention, and nothing is launched
    hc_stub_clear_launches();
    fp.resize.type = ResizeType::BILINEAR;
    HC_CHECK(call(in.data()) == VREADER_UNSUPPORTED && hc_stub_launch_count() == 0, "%s: the adapter refuses BILINEAR", q.what);
    HC_CHECK(call(nullptr) == VREADER_ERROR, "%s: the adapter refuses null inputs", q.what);
    vpp.Close();
}

} // namespace

int main() {
    tsvpp_ctx *ctx = nullptr;
    void *stream = nullptr;
    HC_CHECK(tsvpp_create(1, 1, &ctx) == TSVPP_OK && ctx, "tsvpp_create on the stub's second device");
    if (!ctx) return 3;
    HC_CHECK(tsvpp_consumer_stream(ctx, "coord_bicubic", &stream) == TSVPP_OK && stream, "the consumer's stream");
    const std::vector<std::array<int, 3>> three = { { 322, 182, 384 }, { 32, 18, 48 }, { 4, 2, 4 } };
    const std::vector<Request> requests = {
        { "warp: 1080p to 112 x 112, fp32 planar", false, 112, 112, TSVPP_BGR24, TSVPP_PLANAR, 1, -1, -1, { { 1920, 1080, 2048 } }, 16 },
        { "warp: 33 outputs, two launches, uint8 merged, border", false, 70, 66, TSVPP_RGB24, TSVPP_MERGED, 0, -1, 114, three, 33 },
        { "warp: narrow output, Y800 uint8", false, 30, 34, TSVPP_Y800, TSVPP_MERGED, 0, -1, -1, three, 5 },
        { "warp: fp16 planar tensor, border", false, 112, 112, TSVPP_RGB24, TSVPP_PLANAR, 1, TSVPP_F16, 3, three, 7 },
        { "warp: fp32 Y800 tensor, 33 outputs", false, 64, 64, TSVPP_Y800, TSVPP_MERGED, 1, TSVPP_F32, -1, three, 33 },
        { "perspective: 1080p to 112 x 112, fp32 merged", true, 112, 112, TSVPP_RGB24, TSVPP_MERGED, 1, -1, -1, { { 1920, 1080, 2048 } }, 16 },
        { "perspective: 33 outputs, two launches, uint8 planar, border", true, 70, 66, TSVPP_BGR24, TSVPP_PLANAR, 0, -1, 114, three, 33 },
        { "perspective: bf16 planar tensor", true, 30, 34, TSVPP_BGR24, TSVPP_PLANAR, 1, TSVPP_BF16, -1, three, 6 },
        { "perspective: fp16 Y800 tensor, 33 outputs, border", true, 64, 64, TSVPP_Y800, TSVPP_MERGED, 1, TSVPP_F16, 250, three, 33 },
    };
    for (const Request &q : requests) run(ctx, stream, q);
    adapter(ctx, stream, requests[1]);
    adapter(ctx, stream, requests[3]);
    adapter(ctx, stream, requests[6]);
    adapter(ctx, stream, requests[8]);

    // the footprint exports: inside the frame, never smaller than the BILINEAR box, and the statuses of the BILINEAR exports
    int32_t box[8], plain[8];
    for (int k = 0; k < 12; k++) {
        float m[6], g[2];
        item(k, 322, 182, 70, 66, m, g);
        tsvpp_warp w = {};
        tsvpp_persp t = {};
        for (int i = 0; i < 6; i++) w.m[i] = t.h[i] = m[i];
        t.h[6] = g[0], t.h[7] = g[1], t.h[8] = 1.0f;
        const int a = tsvpp_warp_bicubic_footprint(&w, 322, 182, 38, 69, 32, 63, box), b = tsvpp_warp_footprint(&w, 322, 182, 38, 69, 32, 63, plain);
        HC_CHECK(a == TSVPP_OK && b == TSVPP_OK && box[0] >= 0 && box[1] < 322 && box[2] >= 0 && box[3] < 182 && box[4] >= 0 && box[5] < 161 && box[6] >= 0 && box[7] < 91, "warp footprint %d", k);
        for (int i = 0; i < 8; i += 2) HC_CHECK(box[i] <= plain[i] && box[i + 1] >= plain[i + 1], "warp footprint %d: axis %d is [%d, %d], BILINEAR's [%d, %d]", k, i / 2, box[i], box[i + 1], plain[i], plain[i + 1]);
        const int c = tsvpp_persp_bicubic_footprint(&t, 322, 182, 38, 69, 32, 63, box), d = tsvpp_persp_footprint(&t, 322, 182, 38, 69, 32, 63, plain);
        HC_CHECK(c == TSVPP_OK && d == TSVPP_OK, "perspective footprint %d", k);
        for (int i = 0; i < 8; i += 2) HC_CHECK(box[i] <= plain[i] && box[i + 1] >= plain[i + 1], "perspective footprint %d: axis %d", k, i / 2);
    }
    tsvpp_warp w0 = {};
    HC_CHECK(tsvpp_warp_bicubic_footprint(nullptr, 322, 182, 0, 31, 0, 31, box) == TSVPP_ERROR && tsvpp_warp_bicubic_footprint(&w0, 322, 182, 0, 31, 0, 31, nullptr) == TSVPP_ERROR &&
                 tsvpp_warp_bicubic_footprint(&w0, 0, 182, 0, 31, 0, 31, box) == TSVPP_ERROR && tsvpp_warp_bicubic_footprint(&w0, 322, 182, 4, 3, 0, 31, box) == TSVPP_ERROR &&
                 tsvpp_persp_bicubic_footprint(nullptr, 322, 182, 0, 31, 0, 31, box) == TSVPP_ERROR,
             "the footprint exports' refusals");

    std::fprintf(stderr, "hc_coord_bicubic: %zu requests, 4 through the adapter\n", requests.size());
    tsvpp_destroy(ctx);
    return hc::verdict("hc_coord_bicubic");
}
