// tsvpp_letterbox_p010_area.cpp -- the P010 letterbox call with the exact box filter (include/tsvpp.h): tsvpp_convert_letterbox_p010_area /
// tsvpp_describe_letterbox_p010_area, one pair whose `spec` may be null (the plain flavours) or given (the tensor flavours), and tsvpp_box_p010_plane, the
// contract's executable form on the host; TSVPP_MAX_LETTERBOX_P010 frames per launch, kernels vpp_letterbox_p010_area.hip and vpp_letterbox_p010_area_tensor.hip.
// The request rules are the P010 letterbox call's with AREA in the place of NEAREST / BILINEAR and this call's two limits behind them; the skeletons of both calls
// are tsvpp_tiles.h's.  Nothing here builds a table: the kernel computes every tap and weight in closed form, and what the host adds to the records is the band
// height of the launch.
#include "tsvpp_p010.h"
#include "tsvpp_tiles.h"
#include "vpp_letterbox_p010_area.h"

using namespace tsvpp;

namespace {

// The status of a request, in the order that is part of the ABI: tsvpp_convert_letterbox_p010's (tsvpp_letterbox_p010.cpp), asked with a resize type that call
// accepts so that every rule in front of the type is its own; then the type, then this call's limits.  pl.taps_x / taps_y: the largest tap counts of the request
int box_plan(const tsvpp_params *p, int n, const tsvpp_nv12 *fr, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, bool converting, RoiPlan &pl) {
    if (!p || !fr || n <= 0) return TSVPP_ERROR;
    if (p010_frames_error(n, fr) != TSVPP_OK) return TSVPP_ERROR;
    if (pad_y < 0 || pad_y > 1023 || pad_u < 0 || pad_u > 1023 || pad_v < 0 || pad_v > 1023) return TSVPP_ERROR;
    if (converting && p010_planes_error(n, fr) != TSVPP_OK) return TSVPP_ERROR;
    tsvpp_params q = *p;
    q.resize_type = TSVPP_BILINEAR;
    const int sts = letterbox_plan(&q, n, fr, rects, 0, 0, 0, pl);
    if (sts != TSVPP_OK) return sts;
    if (p->resize_type != TSVPP_AREA) return TSVPP_UNSUPPORTED;
    pl.mode = M_AREA_DOWN;
    for (int f = 0; f < n; f++) {
        if (!plane_span_ok(fr[f].height, fr[f].pitch_y, 2 * fr[f].width) || !plane_span_ok(fr[f].height >> 1, fr[f].pitch_uv, 2 * fr[f].width)) return TSVPP_UNSUPPORTED;
        const tsvpp_rect rc = letterbox_rect_of(fr, rects, f, pl.dst_w, pl.dst_h);
        if (std::max(std::max(fr[f].width, fr[f].height), std::max(rc.width, rc.height)) > BOX_P010_MAX_SIDE) return TSVPP_UNSUPPORTED;
        const int tx = std::max(box_max_taps(fr[f].width, rc.width), box_max_taps(fr[f].width >> 1, rc.width >> 1));
        const int ty = std::max(box_max_taps(fr[f].height, rc.height), box_max_taps(fr[f].height >> 1, rc.height >> 1));
        if (tx > BOX_P010_MAX_TAPS || ty > BOX_P010_MAX_TAPS) return TSVPP_UNSUPPORTED;
        pl.taps_x = std::max(pl.taps_x, tx);
        pl.taps_y = std::max(pl.taps_y, ty);
    }
    return TSVPP_OK;
}

// The request of one call, as tsvpp_tiles.h asks for it
struct LbBoxPath {
    using Launch = LbBoxLaunch;
    static constexpr bool kOwnBudget = true; // no footprint is staged whole: the budget buys band rows
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

    int plan(RoiPlan &pl) const { return box_plan(p, n_frames, frames, rects, pad_y, pad_u, pad_v, converting, pl); }
    int items() const { return n_frames; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_LETTERBOX_P010; }
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, LbBoxLaunch &L) const {
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
    // The band height of a launch: what the budget holds at the widest footprint row among the tile columns that touch a frame's rectangle, either plane -- the
    // numbers the kernel computes.  Every frame of the launch walks its footprints through these buffers: the count is all of them.
    int stage_budget(const RoiPlan &pl, LbBoxLaunch &L, int budget, bool luma_only) const {
        int cpr = 1, lo, hi;
        for (int i = 0; i < L.n_frames; i++) {
            const LbRec &r = L.r[i];
            for (int tx = 0; tx < L.tiles_x; tx++) {
                lo = roi_tile_col0(tx, pl.dst_w, L.last_col0);
                tile_inner_range(lo, tile_last(lo, ROI_TILE_W, pl.dst_w), r.left, r.width, lo, hi);
                if (lo > hi) continue;
                cpr = std::max(cpr, box_cpr_y(lo, hi, r.src_w, r.width));
                if (!luma_only) cpr = std::max(cpr, box_cpr_uv(lo, hi, r.src_w, r.width));
            }
        }
        L.band = box_band_rows(budget, cpr);
        L.band_cpr = cpr;
        L.lds_bytes = box_band_lds(L.band, cpr);
        if (band) *band = L.band;
        return L.n_frames;
    }
    int front_lds(const LbBoxLaunch &) const { return 0; }
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const LbBoxLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_frames);
        return (tensor ? launch_letterbox_p010_area_tensor : launch_letterbox_p010_area)(pl.out, vec, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_letterbox_p010_area%s n=%d ->%dx%d fourcc=%d stream=%p", tensor ? " tensor" : "", n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "src=p010 frames=%d", n_frames); }
    const char *mode_name(const RoiPlan &) const { return "area"; }
    void suffix(char *buf, size_t len, const RoiPlan &pl) const {
        const tsvpp_rect r0 = letterbox_rect_of(frames, rects, 0, pl.dst_w, pl.dst_h);
        std::snprintf(buf, len, " inner=%dx%d+%d+%d taps=%dx%d band=%d", r0.width, r0.height, r0.left, r0.top, pl.taps_x, pl.taps_y, band ? *band : 0);
    }
};

} // namespace

extern "C" {

int tsvpp_convert_letterbox_p010_area(tsvpp_ctx *ctx, int n, const tsvpp_p010 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec, const tsvpp_rect *rects,
                                      int pad_y, int pad_u, int pad_v, void *const *outs, void *stream) {
    const P010Frames<TSVPP_MAX_LETTERBOX_P010> fr(n, in);
    return tile_convert(LbBoxPath{ spec != nullptr, p, spec, n, fr.data, rects, pad_y, pad_u, pad_v, true, nullptr }, ctx, outs, stream);
}

int tsvpp_describe_letterbox_p010_area(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n, const tsvpp_p010 *in, const tsvpp_rect *rects, int aligned_outputs,
                                       char *buf, size_t buf_len) {
    const P010Frames<TSVPP_MAX_LETTERBOX_P010> fr(n, in);
    int band = 0;
    return tile_describe(LbBoxPath{ spec != nullptr, p, spec, n, fr.data, rects, 0, 0, 0, false, &band }, aligned_outputs, buf, buf_len); // (the pad is no part of what is launched)
}

// One plane of samples through the kernel's own functions, in the kernel's order of passes: the row means of every source row, then the columns
int tsvpp_box_p010_plane(const uint16_t *src, int src_w, int src_h, uint16_t *dst, int dst_w, int dst_h) {
    if (!src || !dst || src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0) return TSVPP_ERROR;
    if (std::max(std::max(src_w, src_h), std::max(dst_w, dst_h)) > BOX_P010_MAX_SIDE) return TSVPP_UNSUPPORTED; // (the tap limit is the kernel's, not the arithmetic's)
    const uint32_t Nx = (uint32_t)src_w, nx = (uint32_t)dst_w, Ny = (uint32_t)src_h, ny = (uint32_t)dst_h;
    const BoxDiv dnx = box_div_of(nx), dny = box_div_of(ny), dNx = box_div_of(Nx), d64Ny = box_div_of(64u * Ny);
    std::vector<uint32_t> r;
    try {
        r.resize((size_t)src_h * dst_w);
    } catch (...) { // no exception crosses the C boundary
        return TSVPP_ERROR;
    }
    for (uint32_t j = 0; j < nx; j++) {
        const BoxTaps t = box_taps(j, Nx, nx, dnx);
        for (uint32_t y = 0; y < Ny; y++) {
            const uint16_t *s = src + (size_t)y * Nx + t.first;
            uint32_t hx = t.w_first * s[0];
            for (uint32_t e = 1; e + 1 < t.count; e++) hx += nx * s[e];
            if (t.count > 1) hx += t.w_last * s[t.count - 1];
            r[(size_t)y * nx + j] = box_row_mean(hx, dNx);
        }
    }
    for (uint32_t i = 0; i < ny; i++) {
        const BoxTaps t = box_taps(i, Ny, ny, dny);
        for (uint32_t j = 0; j < nx; j++) {
            uint32_t v = 0;
            for (uint32_t e = 0; e < t.count; e++) v += box_overlap(t.first + e, i, Ny, ny) * r[(size_t)(t.first + e) * nx + j];
            dst[(size_t)i * nx + j] = (uint16_t)box_sample(v, Ny, d64Ny);
        }
    }
    return TSVPP_OK;
}

} // extern "C"
