// tsvpp_letterbox.cpp -- aspect-preserving resize into a padded canvas (include/tsvpp.h): tsvpp_letterbox_rect, tsvpp_convert_letterbox, tsvpp_describe_letterbox and
// their tensor forms (tsvpp_convert_letterbox_tensor / tsvpp_describe_letterbox_tensor: `spec`, null for the first pair; kernel vpp_letterbox_tensor.hip);
// TSVPP_MAX_LETTERBOX frames per launch, kernel vpp_letterbox.hip.  The request rules are letterbox_plan's (tsvpp_plan.cpp), the spec's tensor_spec_status's.
#include "tsvpp_tiles.h"
#include "vpp_letterbox.h"

using namespace tsvpp;

namespace {

// The request of one call, as tsvpp_tiles.h asks for it
struct LbPath {
    using Launch = LbLaunch;
    static constexpr bool kInnerRect = true; // a frame fills its inner rectangle: tiles that miss it stage nothing
    static constexpr bool kOwnBudget = false;
    static constexpr bool kCountsStaged = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // (may carry null planes: the describe calls)
    const tsvpp_rect *rects;
    int pad_y, pad_u, pad_v;

    int plan(RoiPlan &pl) const { return letterbox_plan(p, n_frames, frames, rects, pad_y, pad_u, pad_v, pl); }
    int items() const { return n_frames; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_LETTERBOX; }
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, LbLaunch &L) const {
        L.n_frames = cnt;
        L.pad_y = (float)pad_y;
        L.pad_u = (float)pad_u;
        L.pad_v = (float)pad_v;
        for (int i = 0; i < cnt; i++) {
            const tsvpp_nv12 &fr = frames[base + i];
            const tsvpp_rect rc = letterbox_rect_of(frames, rects, base + i, pl.dst_w, pl.dst_h);
            LbRec &r = L.r[i];
            r.y = (uint64_t)(uintptr_t)fr.y;
            r.uv = (uint64_t)(uintptr_t)fr.uv;
            r.out = outs ? (uint64_t)(uintptr_t)outs[base + i] : 0;
            r.pitch_y = pitch_or_width(fr.pitch_y, fr.width);
            r.pitch_uv = pitch_or_width(fr.pitch_uv, fr.width);
            r.src_w = fr.width;
            r.src_h = fr.height;
            r.xr = (float)r.src_w / (float)rc.width; // src/Resize.cu:418-419, the rectangle as the output
            r.yr = (float)r.src_h / (float)rc.height;
            r.left = rc.left;
            r.top = rc.top;
            r.width = rc.width;
            r.height = rc.height;
        }
    }
    TileItem item(const RoiPlan &pl, const LbLaunch &L, int i) const {
        const LbRec &r = L.r[i];
        return TileItem{ (int)pl.mode, r.src_w, r.src_h, r.xr, r.yr, r.left, r.top, r.width, r.height };
    }
    int front_lds(const LbLaunch &) const { return 0; }
    hipError_t launch(const RoiPlan &pl, bool vec, bool staged, const LbLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_frames);
        return (tensor ? launch_letterbox_tensor : launch_letterbox)(pl.mode, pl.out, vec, staged, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_letterbox%s n=%d ->%dx%d mode=%d fourcc=%d stream=%p", tensor ? "_tensor" : "", n_frames, pl.dst_w, pl.dst_h, (int)pl.mode, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "frames=%d", n_frames); }
    const char *mode_name(const RoiPlan &pl) const { return mode_names[pl.mode]; }
    void suffix(char *buf, size_t len, const RoiPlan &pl) const {
        const tsvpp_rect r0 = letterbox_rect_of(frames, rects, 0, pl.dst_w, pl.dst_h);
        std::snprintf(buf, len, " inner=%dx%d+%d+%d", r0.width, r0.height, r0.left, r0.top);
    }
};

} // namespace

extern "C" {

int tsvpp_letterbox_rect(int in_w, int in_h, int dst_w, int dst_h, tsvpp_rect *out) {
    if (!out || in_w <= 0 || in_h <= 0 || dst_w <= 0 || dst_h <= 0) return TSVPP_ERROR;
    if ((dst_w | dst_h) & 1) return TSVPP_UNSUPPORTED;
    const int64_t iw = in_w, ih = in_h, dw = dst_w, dh = dst_h;
    int64_t w, h;
    if (iw * dh >= ih * dw) {
        w = dw;
        h = std::min(std::max<int64_t>(2 * ((ih * dw + iw) / (2 * iw)), 2), dh);
    } else {
        h = dh;
        w = std::min(std::max<int64_t>(2 * ((iw * dh + ih) / (2 * ih)), 2), dw);
    }
    out->width = (int32_t)w;
    out->height = (int32_t)h;
    out->left = (int32_t)(((dw - w) / 2) & ~(int64_t)1);
    out->top = (int32_t)(((dh - h) / 2) & ~(int64_t)1);
    return TSVPP_OK;
}

int tsvpp_convert_letterbox(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v,
                            void *const *outs, void *stream) {
    return tile_convert(LbPath{ false, p, nullptr, n, in, rects, pad_y, pad_u, pad_v }, ctx, outs, stream);
}

int tsvpp_describe_letterbox(const tsvpp_params *p, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(LbPath{ false, p, nullptr, n, in, rects, 0, 0, 0 }, aligned_outputs, buf, buf_len); // (the pad is no part of what is launched)
}

int tsvpp_convert_letterbox_tensor(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec, const tsvpp_rect *rects,
                                   int pad_y, int pad_u, int pad_v, void *const *outs, void *stream) {
    return tile_convert(LbPath{ true, p, spec, n, in, rects, pad_y, pad_u, pad_v }, ctx, outs, stream);
}

int tsvpp_describe_letterbox_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects,
                                    int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(LbPath{ true, p, spec, n, in, rects, 0, 0, 0 }, aligned_outputs, buf, buf_len);
}

} // extern "C"
