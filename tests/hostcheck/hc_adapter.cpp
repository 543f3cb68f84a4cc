// hc_adapter.cpp -- host check, single thread (AddressSanitizer + UndefinedBehaviorSanitizer): the fifteen tile methods of cpp/VideoProcessor.h -- ConvertRois,
// ConvertRoisArea, ConvertRoisSized, ConvertLetterbox, ConvertWarp, ConvertPerspective, ConvertRemap, ConvertMesh and the seven overloads that take a
// tsvpp_tensor_spec -- on the stub runtime (stub_hip.cpp).  Launches are recorded and range-checked by the stub, never executed: the launch log is the observable.
//   forwarding  a method on consumer "a" launches, field by field of HcLaunch, what its tsvpp_convert_* entry point launches when called on vpp.context() with
//               the stream of tsvpp_consumer_stream(ctx, "a") and the same frames (two, of different size and pitch), items, parameters, spec, border or pad and
//               outputs.  TSVPP_OPT_INPUTS_READY is set and the consumer's alternation stands at its SECOND stream: the tile calls still take the first.
//   AREA        ConvertRoisArea launches what tsvpp_convert_rois_area launches; ConvertRois refuses that request with the library's status; the tensor
//               ConvertRois takes it.
//   guards      VREADER_ERROR and no launch: a processor never Init()ed or Close()d, null inputs, nInputs <= 0, a null inputs[1], a null item array, an item
//               count <= 0 (ConvertRemap / ConvertMesh: the maps / meshes and the remap list separately), null deviceOuts.  ConvertLetterbox with null rects
//               is legal and launches.
//   refusals    the library's status for a box outside its frame, a rectangle outside the canvas, a matrix / homography of a frame not given, a map / mesh index
//               not given, a set resize.width of the sized call comes back unchanged, and nothing is launched.
//   teardown    after Close() the stub holds nothing.
// usage: hc_adapter.  Exit status 0 only without a failed assertion, a stub violation, or anything the stub still holds at the end.
#include <functional>
#include <vector>

#include "VideoProcessor.h"
#include "hc_common.h"

namespace {

constexpr int kW = 32, kH = 32;        // every uniform output, and the sized call's first box
constexpr size_t kOutBytes = 64 << 10; // more than any output here: 3 x 64 x 64 fp32

// one request, in the adapter's terms and in the C ABI's
struct Args {
    AVFrame *const *inputs;
    int nInputs;
    const tsvpp_nv12 *frames;
    const void *items; // rois, rects, warps, persps; ConvertRemap / ConvertMesh: the maps / meshes
    int nItems;
    const tsvpp_remap *remaps; // ConvertRemap / ConvertMesh only
    int nRemaps;
    void *const *outs;
    FrameParameters options;
    tsvpp_params p;
    const tsvpp_tensor_spec *spec;
};

enum Kind { ROIS, ROIS_AREA, ROIS_SIZED, LETTERBOX, WARP, PERSP, REMAP, MESH };
struct Method {
    const char *name;
    Kind kind;
    bool tensor;
    std::function<int(VideoProcessor &, Args &)> method;
    std::function<int(tsvpp_ctx *, void *, const Args &)> direct;
    bool rects_optional() const { return kind == LETTERBOX; }
    bool two_lists() const { return kind == REMAP || kind == MESH; }
};

constexpr int kBorder[3] = { 16, 128, 128 };

template <class T> const T *as(const Args &a) { return static_cast<const T *>(a.items); }

std::vector<HcLaunch> take_log() {
    std::vector<HcLaunch> log;
    for (size_t i = 0; i < hc_stub_launch_count(); i++) log.push_back(*hc_stub_launch(i));
    hc_stub_clear_launches();
    return log;
}

bool same_launch(const HcLaunch &a, const HcLaunch &b) {
    return a.fn == b.fn && std::strcmp(a.name, b.name) == 0 && std::memcmp(a.grid, b.grid, sizeof(a.grid)) == 0 && std::memcmp(a.block, b.block, sizeof(a.block)) == 0 &&
           a.lds == b.lds && a.stream == b.stream && a.any_order == b.any_order && a.captured == b.captured && a.refused == b.refused;
}

FrameParameters options_of(int w, int h, ResizeType type) {
    ColorOptions color(FourCC::RGB24);
    color.planesPos = Planes::PLANAR;
    color.normalization = true; // what the tensor forms need; the plain forms then store fp32
    ResizeOptions resize(w, h);
    resize.type = type;
    return FrameParameters(resize, color);
}
tsvpp_params flat_of(const FrameParameters &o) {
    return tsvpp_params{ 0, 0, 0, 0, (int)o.resize.width, (int)o.resize.height, (int)o.resize.type, (int)o.color.dstFourCC, (int)o.color.planesPos, o.color.normalization ? 1 : 0 };
}

// the consumer's alternation (tsvpp_consumer_next_stream under TSVPP_OPT_INPUTS_READY) is left at its second stream: an adapter that asked for the "next" stream
// would launch there
void *first_stream_with_second_up_next(tsvpp_ctx *ctx) {
    void *first = nullptr, *next = nullptr;
    HC_CHECK(tsvpp_consumer_stream(ctx, "a", &first) == TSVPP_OK && first, "the consumer's stream");
    for (int k = 0; k < 2 && next != first; k++) HC_CHECK(tsvpp_consumer_next_stream(ctx, "a", 0, &next) == TSVPP_OK, "the consumer's next stream");
    HC_CHECK(next == first, "two calls of tsvpp_consumer_next_stream pass the first stream");
    return first;
}

// method and entry point launch the same; returns the number of launches
size_t forwards(VideoProcessor &vpp, const Method &m, Args a, const char *what) {
    void *stream = first_stream_with_second_up_next(vpp.context());
    hc_stub_clear_launches();
    const int via = m.method(vpp, a);
    const std::vector<HcLaunch> got = take_log();
    const int direct = m.direct(vpp.context(), stream, a);
    const std::vector<HcLaunch> want = take_log();
    HC_CHECK(via == VREADER_OK && direct == TSVPP_OK, "%s, %s: the method answers %d, the entry point %d", m.name, what, via, direct);
    HC_CHECK(got.size() == want.size() && !want.empty(), "%s, %s: the method launched %zu kernels, the entry point %zu", m.name, what, got.size(), want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); i++)
        HC_CHECK(same_launch(got[i], want[i]), "%s, %s: launch %zu is %s grid %u lds %zu stream %p any_order %d, the entry point's %s grid %u lds %zu stream %p any_order %d", m.name,
                 what, i, got[i].name, got[i].grid[0], got[i].lds, (void *)got[i].stream, got[i].any_order, want[i].name, want[i].grid[0], want[i].lds, (void *)want[i].stream,
                 want[i].any_order);
    return got.size();
}

void refused_with(VideoProcessor &vpp, const Method &m, Args a, int status, const char *what) {
    hc_stub_clear_launches();
    const int got = m.method(vpp, a);
    HC_CHECK(got == status && hc_stub_launch_count() == 0, "%s, %s: status %d (expected %d), %zu launches", m.name, what, got, status, hc_stub_launch_count());
    hc_stub_clear_launches();
}

void guards(VideoProcessor &vpp, const Method &m, const Args &good) {
    Args a = good;
    a.inputs = nullptr;
    refused_with(vpp, m, a, VREADER_ERROR, "inputs == nullptr");
    a = good, a.nInputs = 0;
    refused_with(vpp, m, a, VREADER_ERROR, "nInputs == 0");
    a = good, a.nInputs = -1;
    refused_with(vpp, m, a, VREADER_ERROR, "nInputs < 0");
    AVFrame *hole[2] = { good.inputs[0], nullptr };
    a = good, a.inputs = hole;
    refused_with(vpp, m, a, VREADER_ERROR, "a null inputs[1]");
    a = good, a.outs = nullptr;
    refused_with(vpp, m, a, VREADER_ERROR, "deviceOuts == nullptr");
    if (m.rects_optional()) {
        a = good, a.items = nullptr;
        forwards(vpp, m, a, "rects == nullptr");
    } else {
        a = good, a.items = nullptr;
        refused_with(vpp, m, a, VREADER_ERROR, "a null item array");
        a = good, a.nItems = 0;
        refused_with(vpp, m, a, VREADER_ERROR, "an item count of 0");
        a = good, a.nItems = -1;
        refused_with(vpp, m, a, VREADER_ERROR, "a negative item count");
    }
    if (m.two_lists()) {
        a = good, a.remaps = nullptr;
        refused_with(vpp, m, a, VREADER_ERROR, "a null remap list");
        a = good, a.nRemaps = 0;
        refused_with(vpp, m, a, VREADER_ERROR, "a remap count of 0");
        a = good, a.nRemaps = -1;
        refused_with(vpp, m, a, VREADER_ERROR, "a negative remap count");
    }
}

} // namespace

int main() {
    // two frames of different size and pitch; planes, maps, meshes and outputs are the stub's blocks, never read
    uint8_t *planes[4] = { hc::dev_alloc(48 * 64), hc::dev_alloc(24 * 64), hc::dev_alloc(64 * 128), hc::dev_alloc(32 * 128) };
    AVFrame f0, f1;
    f0.data[0] = planes[0], f0.data[1] = planes[1], f0.linesize[0] = f0.linesize[1] = 64, f0.width = 64, f0.height = 48;
    f1.data[0] = planes[2], f1.data[1] = planes[3], f1.linesize[0] = f1.linesize[1] = 128, f1.width = 96, f1.height = 64;
    AVFrame *inputs[2] = { &f0, &f1 };
    const tsvpp_nv12 frames[2] = { { planes[0], planes[1], 64, 64, 64, 48 }, { planes[2], planes[3], 128, 128, 96, 64 } };
    uint8_t *out_blocks[3] = { hc::dev_alloc(kOutBytes), hc::dev_alloc(kOutBytes), hc::dev_alloc(kOutBytes) };
    void *outs[3] = { out_blocks[0], out_blocks[1], out_blocks[2] };
    int mesh_cols = 0, mesh_rows = 0;
    HC_CHECK(tsvpp_mesh_dims(kW, kH, 4, 4, &mesh_cols, &mesh_rows) == TSVPP_OK, "tsvpp_mesh_dims");
    uint8_t *map_blocks[2] = { hc::dev_alloc((size_t)kW * kH * 8), hc::dev_alloc((size_t)kW * kH * 8) };
    uint8_t *mesh_blocks[2] = { hc::dev_alloc((size_t)mesh_cols * mesh_rows * 8), hc::dev_alloc((size_t)mesh_cols * mesh_rows * 8) };

    // three items that address both frames
    const tsvpp_roi rois[3] = { { 0, 0, 0, 32, 32 }, { 1, 16, 16, 80, 48 }, { 0, 8, 8, 56, 40 } };
    const tsvpp_roi_sized sized[3] = { { 0, 0, 0, 32, 32, kW, kH }, { 1, 16, 16, 80, 48, 48, 16 }, { 0, 8, 8, 56, 40, 20, 64 } };
    const tsvpp_rect rects[2] = { { 0, 8, 64, 48 }, { 8, 0, 48, 32 } };
    const tsvpp_warp warps[3] = { { 0, { 1, 0, 4, 0, 1, 2 } }, { 1, { 2, 0, 0, 0, 2, 0 } }, { 0, { 0.5f, -0.5f, 20, 0.5f, 0.5f, 3 } } };
    const tsvpp_persp persps[3] = { { 0, { 1, 0, 4, 0, 1, 2, 0, 0, 1 } }, { 1, { 2, 0, 0, 0, 2, 0, 0, 0, 1 } }, { 0, { 1, 0.25f, 0, 0, 1, 0, 0.001f, 0, 1 } } };
    const tsvpp_map maps[2] = { { (const float *)map_blocks[0], 0, 0 }, { (const float *)map_blocks[1], 0, 0 } };
    const tsvpp_mesh meshes[2] = { { (const float *)mesh_blocks[0], 0, 4, 4, 0 }, { (const float *)mesh_blocks[1], 0, 4, 4, 0 } };
    const tsvpp_remap remaps[3] = { { 0, 0 }, { 1, 1 }, { 0, 1 } };
    const tsvpp_tensor_spec spec = { TSVPP_F16, { 0.485f, 0.456f, 0.406f }, { 4.0f, 4.5f, 5.0f } };

    // the request each check program provokes a refusal with
    const tsvpp_roi bad_roi = { 0, 0, 0, 64 + 2, 2 };
    const tsvpp_rect bad_rects[2] = { { 0, 0, 64 + 2, 2 }, { 0, 0, 64, 64 } };
    const tsvpp_warp bad_warp = { 2, { 1, 0, 0, 0, 1, 0 } };
    const tsvpp_persp bad_persp = { 2, { 1, 0, 0, 0, 1, 0, 0, 0, 1 } };
    const tsvpp_remap bad_remap = { 0, 2 };

#define BORDER kBorder[0], kBorder[1], kBorder[2]
    const Method methods[15] = {
        { "ConvertRois", ROIS, false, [](VideoProcessor &v, Args &a) { return v.ConvertRois(a.inputs, a.nInputs, as<tsvpp_roi>(a), a.nItems, a.outs, a.options, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_rois(c, a.nInputs, a.frames, a.nItems, as<tsvpp_roi>(a), &a.p, a.outs, s); } },
        { "ConvertRois (tensor)", ROIS, true, [](VideoProcessor &v, Args &a) { return v.ConvertRois(a.inputs, a.nInputs, as<tsvpp_roi>(a), a.nItems, a.outs, a.options, a.spec, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_rois_tensor(c, a.nInputs, a.frames, a.nItems, as<tsvpp_roi>(a), &a.p, a.spec, a.outs, s); } },
        { "ConvertRoisArea", ROIS_AREA, false, [](VideoProcessor &v, Args &a) { return v.ConvertRoisArea(a.inputs, a.nInputs, as<tsvpp_roi>(a), a.nItems, a.outs, a.options, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_rois_area(c, a.nInputs, a.frames, a.nItems, as<tsvpp_roi>(a), &a.p, a.outs, s); } },
        { "ConvertRoisSized", ROIS_SIZED, false,
          [](VideoProcessor &v, Args &a) { return v.ConvertRoisSized(a.inputs, a.nInputs, as<tsvpp_roi_sized>(a), a.nItems, a.outs, a.options, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_rois_sized(c, a.nInputs, a.frames, a.nItems, as<tsvpp_roi_sized>(a), &a.p, a.outs, s); } },
        { "ConvertRoisSized (tensor)", ROIS_SIZED, true,
          [](VideoProcessor &v, Args &a) { return v.ConvertRoisSized(a.inputs, a.nInputs, as<tsvpp_roi_sized>(a), a.nItems, a.outs, a.options, a.spec, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_rois_sized_tensor(c, a.nInputs, a.frames, a.nItems, as<tsvpp_roi_sized>(a), &a.p, a.spec, a.outs, s); } },
        { "ConvertLetterbox", LETTERBOX, false, [](VideoProcessor &v, Args &a) { return v.ConvertLetterbox(a.inputs, a.nInputs, as<tsvpp_rect>(a), BORDER, a.outs, a.options, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_letterbox(c, a.nInputs, a.frames, &a.p, as<tsvpp_rect>(a), BORDER, a.outs, s); } },
        { "ConvertLetterbox (tensor)", LETTERBOX, true,
          [](VideoProcessor &v, Args &a) { return v.ConvertLetterbox(a.inputs, a.nInputs, as<tsvpp_rect>(a), BORDER, a.outs, a.options, a.spec, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_letterbox_tensor(c, a.nInputs, a.frames, &a.p, a.spec, as<tsvpp_rect>(a), BORDER, a.outs, s); } },
        { "ConvertWarp", WARP, false, [](VideoProcessor &v, Args &a) { return v.ConvertWarp(a.inputs, a.nInputs, as<tsvpp_warp>(a), a.nItems, BORDER, a.outs, a.options, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_warp(c, a.nInputs, a.frames, a.nItems, as<tsvpp_warp>(a), &a.p, BORDER, a.outs, s); } },
        { "ConvertWarp (tensor)", WARP, true,
          [](VideoProcessor &v, Args &a) { return v.ConvertWarp(a.inputs, a.nInputs, as<tsvpp_warp>(a), a.nItems, BORDER, a.outs, a.options, a.spec, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_warp_tensor(c, a.nInputs, a.frames, a.nItems, as<tsvpp_warp>(a), &a.p, a.spec, BORDER, a.outs, s); } },
        { "ConvertPerspective", PERSP, false,
          [](VideoProcessor &v, Args &a) { return v.ConvertPerspective(a.inputs, a.nInputs, as<tsvpp_persp>(a), a.nItems, BORDER, a.outs, a.options, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_perspective(c, a.nInputs, a.frames, a.nItems, as<tsvpp_persp>(a), &a.p, BORDER, a.outs, s); } },
        { "ConvertPerspective (tensor)", PERSP, true,
          [](VideoProcessor &v, Args &a) { return v.ConvertPerspective(a.inputs, a.nInputs, as<tsvpp_persp>(a), a.nItems, BORDER, a.outs, a.options, a.spec, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_perspective_tensor(c, a.nInputs, a.frames, a.nItems, as<tsvpp_persp>(a), &a.p, a.spec, BORDER, a.outs, s); } },
        { "ConvertRemap", REMAP, false,
          [](VideoProcessor &v, Args &a) { return v.ConvertRemap(a.inputs, a.nInputs, as<tsvpp_map>(a), a.nItems, a.remaps, a.nRemaps, BORDER, a.outs, a.options, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_remap(c, a.nInputs, a.frames, a.nItems, as<tsvpp_map>(a), a.nRemaps, a.remaps, &a.p, BORDER, a.outs, s); } },
        { "ConvertRemap (tensor)", REMAP, true,
          [](VideoProcessor &v, Args &a) { return v.ConvertRemap(a.inputs, a.nInputs, as<tsvpp_map>(a), a.nItems, a.remaps, a.nRemaps, BORDER, a.outs, a.options, a.spec, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) {
              return tsvpp_convert_remap_tensor(c, a.nInputs, a.frames, a.nItems, as<tsvpp_map>(a), a.nRemaps, a.remaps, &a.p, a.spec, BORDER, a.outs, s);
          } },
        { "ConvertMesh", MESH, false,
          [](VideoProcessor &v, Args &a) { return v.ConvertMesh(a.inputs, a.nInputs, as<tsvpp_mesh>(a), a.nItems, a.remaps, a.nRemaps, BORDER, a.outs, a.options, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) { return tsvpp_convert_mesh(c, a.nInputs, a.frames, a.nItems, as<tsvpp_mesh>(a), a.nRemaps, a.remaps, &a.p, BORDER, a.outs, s); } },
        { "ConvertMesh (tensor)", MESH, true,
          [](VideoProcessor &v, Args &a) { return v.ConvertMesh(a.inputs, a.nInputs, as<tsvpp_mesh>(a), a.nItems, a.remaps, a.nRemaps, BORDER, a.outs, a.options, a.spec, "a"); },
          [](tsvpp_ctx *c, void *s, const Args &a) {
              return tsvpp_convert_mesh_tensor(c, a.nInputs, a.frames, a.nItems, as<tsvpp_mesh>(a), a.nRemaps, a.remaps, &a.p, a.spec, BORDER, a.outs, s);
          } },
    };
#undef BORDER
    const Method &plain_rois = methods[0], &tensor_rois = methods[1], &area_rois = methods[2];

    const auto request_of = [&](const Method &m) {
        Args a = { inputs, 2, frames, rois, 3, nullptr, 0, outs, options_of(kW, kH, ResizeType::BILINEAR), {}, m.tensor ? &spec : nullptr };
        switch (m.kind) {
        case ROIS: break;
        case ROIS_AREA: a.options.resize.type = ResizeType::AREA; break;
        case ROIS_SIZED: a.items = sized, a.options = options_of(0, 0, ResizeType::BILINEAR); break; // the sizes are the boxes'
        case LETTERBOX: a.items = rects, a.nItems = 2, a.options = options_of(64, 64, ResizeType::BILINEAR); break; // one rectangle per frame: nItems is not passed
        case WARP: a.items = warps; break;
        case PERSP: a.items = persps; break;
        case REMAP: a.items = maps, a.nItems = 2, a.remaps = remaps, a.nRemaps = 3; break;
        case MESH: a.items = meshes, a.nItems = 2, a.remaps = remaps, a.nRemaps = 3; break;
        }
        a.p = flat_of(a.options);
        return a;
    };
    const auto spoilt = [&](const Method &m) {
        Args a = request_of(m);
        switch (m.kind) {
        case ROIS:
        case ROIS_AREA: a.items = &bad_roi, a.nItems = 1; break;                             // a box outside its frame
        case ROIS_SIZED: a.options.resize.width = kW, a.options.resize.height = kH; break;   // the parameters' own output size, set
        case LETTERBOX: a.items = bad_rects; break;                                          // a rectangle outside the canvas
        case WARP: a.items = &bad_warp, a.nItems = 1; break;                                 // a matrix of a frame not given
        case PERSP: a.items = &bad_persp, a.nItems = 1; break;
        case REMAP:
        case MESH: a.remaps = &bad_remap, a.nRemaps = 1; break;                              // a map / mesh index not given
        }
        a.p = flat_of(a.options);
        return a;
    };

    VideoProcessor vpp;
    for (const Method &m : methods) refused_with(vpp, m, request_of(m), VREADER_ERROR, "a processor that was never Init()ed");
    const long held = hc_stub_live();
    HC_CHECK(vpp.Init(nullptr, 2, false, 0) == VREADER_OK && vpp.context(), "VideoProcessor::Init");
    if (!vpp.context()) return 3;
    HC_CHECK(tsvpp_set_option(vpp.context(), TSVPP_OPT_INPUTS_READY, 1) == TSVPP_OK, "set_option inputs-ready");

    for (const Method &m : methods) {
        const Args good = request_of(m);
        forwards(vpp, m, good, "the valid request");
        guards(vpp, m, good);
        // a refusal of the library's: its status, unchanged
        const Args bad = spoilt(m);
        hc_stub_clear_launches();
        const int status = m.direct(vpp.context(), first_stream_with_second_up_next(vpp.context()), bad);
        HC_CHECK(status != TSVPP_OK && hc_stub_launch_count() == 0, "%s: the entry point answers %d to the spoilt request, after %zu launches", m.name, status, hc_stub_launch_count());
        HC_CHECK(status == TSVPP_ERROR, "%s: the spoilt request is the one the check program provokes, TSVPP_ERROR, not %d", m.name, status);
        refused_with(vpp, m, bad, status, "the request the library refuses");
    }

    { // AREA: ConvertRois refuses it with the library's status, ConvertRoisArea and the tensor ConvertRois take it
        Args area = request_of(area_rois);
        const int status = tsvpp_convert_rois(vpp.context(), 2, frames, 3, rois, &area.p, outs, first_stream_with_second_up_next(vpp.context()));
        HC_CHECK(status == TSVPP_UNSUPPORTED, "tsvpp_convert_rois answers %d to AREA", status);
        refused_with(vpp, plain_rois, area, status, "AREA");
        const size_t plain = forwards(vpp, area_rois, area, "AREA");
        area.spec = &spec;
        const size_t tensor = forwards(vpp, tensor_rois, area, "AREA");
        HC_CHECK(plain == 1 && tensor == 1, "three boxes are one launch: %zu, %zu", plain, tensor);
        Args bilinear = request_of(plain_rois);
        const int other = tsvpp_convert_rois_area(vpp.context(), 2, frames, 3, rois, &bilinear.p, outs, first_stream_with_second_up_next(vpp.context()));
        HC_CHECK(other != TSVPP_OK, "tsvpp_convert_rois_area answers %d to BILINEAR", other);
        refused_with(vpp, area_rois, bilinear, other, "BILINEAR");
    }

    vpp.Close();
    for (const Method &m : methods) refused_with(vpp, m, request_of(m), VREADER_ERROR, "a processor that was Close()d");
    HC_CHECK(hc_stub_live() == held, "Close() left %ld streams, events or blocks of the processor's behind", hc_stub_live() - held);
    for (uint8_t *b : planes) (void)hipFree(b);
    for (uint8_t *b : out_blocks) (void)hipFree(b);
    for (uint8_t *b : map_blocks) (void)hipFree(b);
    for (uint8_t *b : mesh_blocks) (void)hipFree(b);
    return hc::verdict("hc_adapter");
}
