// tsvpp_letterbox_p010_bicubic.cpp -- the P010 letterbox call with the separable integer cubic (include/tsvpp.h): tsvpp_convert_letterbox_p010_bicubic /
// tsvpp_describe_letterbox_p010_bicubic, one pair whose `spec` may be null (the plain flavours) or given (the tensor flavours); TSVPP_MAX_LETTERBOX_P010 frames
// per launch, kernels vpp_letterbox_p010_bicubic.hip and vpp_letterbox_p010_bicubic_tensor.hip.  The request rules are the P010 letterbox call's with BICUBIC in
// the place of NEAREST / BILINEAR and the P010 BICUBIC ROI call's limits behind them, per frame on its rectangle; the skeletons of both calls are tsvpp_tiles.h's.
// Nothing here builds a table: the kernel computes every tap and weight in closed form from N and n, and what the host adds to the records is the LDS carve-up
// of the launch.  (The contract's executable form, tsvpp_cubic_p010_plane, is tsvpp_rois_p010_bicubic.cpp's.)
#include "tsvpp_cubic_p010.h"
#include "tsvpp_p010.h"
#include "tsvpp_tiles.h"
#include "vpp_letterbox_p010_bicubic.h"

using namespace tsvpp;

namespace {

// The status of a request, in the order that is part of the ABI: tsvpp_convert_letterbox_p010's (tsvpp_letterbox_p010.cpp), asked with a resize type that call
// accepts so that every rule in front of the type is its own; then the type, then this call's limits
int cubic_plan(const tsvpp_params *p, int n, const tsvpp_nv12 *fr, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, bool converting, RoiPlan &pl) {
    if (!p || !fr || n <= 0) return TSVPP_ERROR;
    if (p010_frames_error(n, fr) != TSVPP_OK) return TSVPP_ERROR;
    if (pad_y < 0 || pad_y > 1023 || pad_u < 0 || pad_u > 1023 || pad_v < 0 || pad_v > 1023) return TSVPP_ERROR;
    if (converting && p010_planes_error(n, fr) != TSVPP_OK) return TSVPP_ERROR;
    tsvpp_params q = *p;
    q.resize_type = TSVPP_BILINEAR;
    const int sts = letterbox_plan(&q, n, fr, rects, 0, 0, 0, pl);
    if (sts != TSVPP_OK) return sts;
    if (p->resize_type != TSVPP_BICUBIC) return TSVPP_UNSUPPORTED;
    pl.mode = M_BICUBIC;
    for (int f = 0; f < n; f++) {
        if (!plane_span_ok(fr[f].height, fr[f].pitch_y, 2 * fr[f].width) || !plane_span_ok(fr[f].height >> 1, fr[f].pitch_uv, 2 * fr[f].width)) return TSVPP_UNSUPPORTED;
        const tsvpp_rect rc = letterbox_rect_of(fr, rects, f, pl.dst_w, pl.dst_h);
        if (std::max(std::max(fr[f].width, fr[f].height), std::max(rc.width, rc.height)) > CUBIC_P010_MAX_SIDE) return TSVPP_UNSUPPORTED;
        // N <= 8 n on both axes of both planes (chroma: halves of even numbers)
        if (fr[f].width > CUBIC_P010_MAX_RATIO * rc.width || fr[f].height > CUBIC_P010_MAX_RATIO * rc.height) return TSVPP_UNSUPPORTED;
        if ((fr[f].width >> 1) > CUBIC_P010_MAX_RATIO * (rc.width >> 1) || (fr[f].height >> 1) > CUBIC_P010_MAX_RATIO * (rc.height >> 1)) return TSVPP_UNSUPPORTED;
    }
    return TSVPP_OK;
}

// The request of one call, as tsvpp_tiles.h asks for it
struct LbCubicPath {
    using Launch = LbCubicLaunch;
    static constexpr bool kOwnBudget = true; // no footprint is staged whole: the budget buys Hbuf and band rows
    static constexpr bool kCountsStaged = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // byte-plane view of the P010 frames (may carry null planes: the describe call)
    const tsvpp_rect *rects;
    int pad_y, pad_u, pad_v;
    bool converting;
    int *band; // the describe call: receives the first launch's band height

    int plan(RoiPlan &pl) const { return cubic_plan(p, n_frames, frames, rects, pad_y, pad_u, pad_v, converting, pl); }
    int items() const { return n_frames; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_LETTERBOX_P010; }
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, LbCubicLaunch &L) const {
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
            r.pitch_y = fr.pitch_y;
            r.pitch_uv = fr.pitch_uv;
            r.src_w = fr.width;
            r.src_h = fr.height;
            r.xr = (float)r.src_w / (float)rc.width; // (not read by the kernel: its ratios are the integer pairs)
            r.yr = (float)r.src_h / (float)rc.height;
            r.left = rc.left;
            r.top = rc.top;
            r.width = rc.width;
            r.height = rc.height;
        }
    }
    // The LDS of a launch: Hbuf for the tallest footprint and band buffers for the widest footprint row among the tile parts -- a tile's columns and rows inside
    // a frame's rectangle (tile_inner_range) -- of its frames, either plane: the numbers the kernel computes (columns and rows are independent).  A tile column
    // or row that misses the rectangle is pad alone and adds nothing.  L.band = 0: not even one-row bands fit the budget.  Every frame walks its footprints
    // through these buffers: the count is all of them.
    int stage_budget(const RoiPlan &pl, LbCubicLaunch &L, int budget, bool luma_only) const {
        int cpr = 1, hrows = 1, a0, a1, lo, hi;
        for (int i = 0; i < L.n_frames; i++) {
            const LbRec &r = L.r[i];
            const CubicDiv ax = cubic_div_of(r.src_w, r.width), ay = cubic_div_of(r.src_h, r.height);
            const CubicDiv cx = cubic_div_of(r.src_w >> 1, r.width >> 1), cy = cubic_div_of(r.src_h >> 1, r.height >> 1);
            for (int tx = 0; tx < L.tiles_x; tx++) {
                const int j0 = roi_tile_col0(tx, pl.dst_w, L.last_col0);
                tile_inner_range(j0, tile_last(j0, ROI_TILE_W, pl.dst_w), r.left, r.width, a0, a1);
                if (a0 > a1) continue;
                cubic_span(a0, a1, ax, lo, hi);
                cpr = std::max(cpr, roi_chunks(2 * (hi - lo + 1)));
                if (luma_only) continue;
                cubic_span(a0 >> 1, a1 >> 1, cx, lo, hi);
                cpr = std::max(cpr, roi_chunks(4 * (hi - lo + 1)));
            }
            for (int ty = 0; ty < L.tiles_y; ty++) {
                const int i0 = ty * ROI_TILE_H;
                tile_inner_range(i0, tile_last(i0, ROI_TILE_H, pl.dst_h), r.top, r.height, a0, a1);
                if (a0 > a1) continue;
                cubic_span(a0, a1, ay, lo, hi);
                hrows = std::max(hrows, hi - lo + 1);
                if (luma_only) continue;
                cubic_span(a0 >> 1, a1 >> 1, cy, lo, hi);
                hrows = std::max(hrows, hi - lo + 1);
            }
        }
        L.band = cubic_band_rows(budget, hrows, cpr);
        L.band_cpr = cpr;
        L.hrows = hrows;
        L.lds_bytes = cubic_lds(hrows, std::max(L.band, 1), cpr);
        if (band) *band = L.band;
        return L.n_frames;
    }
    int front_lds(const LbCubicLaunch &) const { return 0; }
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const LbCubicLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        if (L.band < 1) return hipErrorNotSupported; // (cubic_fit_status has answered such a request before the skeleton runs)
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_frames);
        return (tensor ? launch_letterbox_p010_bicubic_tensor : launch_letterbox_p010_bicubic)(pl.out, vec, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_letterbox_p010_bicubic%s n=%d ->%dx%d fourcc=%d stream=%p", tensor ? " tensor" : "", n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "src=p010 frames=%d", n_frames); }
    const char *mode_name(const RoiPlan &) const { return "bicubic"; }
    void suffix(char *buf, size_t len, const RoiPlan &pl) const {
        const tsvpp_rect r0 = letterbox_rect_of(frames, rects, 0, pl.dst_w, pl.dst_h);
        std::snprintf(buf, len, " inner=%dx%d+%d+%d band=%d", r0.width, r0.height, r0.left, r0.top, band ? *band : 0);
    }
};

} // namespace

extern "C" {

int tsvpp_convert_letterbox_p010_bicubic(tsvpp_ctx *ctx, int n, const tsvpp_p010 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec, const tsvpp_rect *rects,
                                         int pad_y, int pad_u, int pad_v, void *const *outs, void *stream) {
    const P010Frames<TSVPP_MAX_LETTERBOX_P010> fr(n, in);
    const LbCubicPath path{ spec != nullptr, p, spec, n, fr.data, rects, pad_y, pad_u, pad_v, true, nullptr };
    if (ctx && outs && cubic_fit_status(path, ctx->knobs, outs, false) != TSVPP_OK) {
        clear_last_launch();
        return TSVPP_UNSUPPORTED;
    }
    return tile_convert(path, ctx, outs, stream);
}

int tsvpp_describe_letterbox_p010_bicubic(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n, const tsvpp_p010 *in, const tsvpp_rect *rects, int aligned_outputs,
                                          char *buf, size_t buf_len) {
    const P010Frames<TSVPP_MAX_LETTERBOX_P010> fr(n, in);
    int band = 0;
    const LbCubicPath path{ spec != nullptr, p, spec, n, fr.data, rects, 0, 0, 0, false, &band }; // (the pad is no part of what is launched)
    if (buf && buf_len) {
        Knobs kn; // as tile_describe's: no context
        read_env_knobs(kn);
        if (cubic_fit_status(path, kn, nullptr, aligned_outputs != 0) != TSVPP_OK) {
            buf[0] = 0;
            return TSVPP_UNSUPPORTED;
        }
    }
    return tile_describe(path, aligned_outputs, buf, buf_len);
}

} // extern "C"
