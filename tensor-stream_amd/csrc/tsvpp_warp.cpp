// tsvpp_warp.cpp -- rotated and affine-warped boxes (include/tsvpp.h): tsvpp_convert_warp / tsvpp_describe_warp, their tensor forms (`spec`, null for the first
// pair; kernel vpp_warp_tensor.hip), tsvpp_warp_rotated_box and the DEBUG export of the footprint function; TSVPP_MAX_WARPS outputs per launch, kernel
// vpp_warp.hip.  The body is tsvpp_tiles.h's; WarpPath below says what differs: the request rules (warp_plan, tsvpp_plan.cpp), the record, and the staging budget --
// a warped tile's footprint is a bounding box of its own (warp_footprint, vpp_warp.h), no product of a column span and a row span.
#include <cmath>

#include "tsvpp_tiles.h"
#include "vpp_warp.h"

using namespace tsvpp;

namespace {

// the record's geometry: everything the footprint function and the sampler read (planes and output apart)
void warp_rec_geometry(const tsvpp_warp &w, int frame_w, int frame_h, WarpRec &r) {
    r.src_w = frame_w;
    r.src_h = frame_h;
    r.m0 = w.m[0];
    r.m1 = w.m[1];
    r.m3 = w.m[3];
    r.m4 = w.m[4];
    warp_translations(w.m[2], w.m[5], r);
}

// The request of one call, as tsvpp_tiles.h asks for it
struct WarpPath {
    using Launch = WarpLaunch;
    static constexpr bool kOwnBudget = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // (may carry null planes: the describe calls)
    int n_warps;
    const tsvpp_warp *warps;
    int border_y, border_u, border_v;

    bool border() const { return border_y >= 0; }
    int plan(RoiPlan &pl) const { return warp_plan(p, n_frames, frames, n_warps, warps, border_y, border_u, border_v, pl); }
    int items() const { return n_warps; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_WARPS; }
    void fill_items(const RoiPlan &, void *const *outs, int base, int cnt, WarpLaunch &L) const {
        L.n_warps = cnt;
        L.border_y = (float)border_y;
        L.border_u = (float)border_u;
        L.border_v = (float)border_v;
        for (int i = 0; i < cnt; i++) {
            const tsvpp_warp &w = warps[base + i];
            const tsvpp_nv12 &fr = frames[w.frame];
            WarpRec &r = L.r[i];
            r.y = (uint64_t)(uintptr_t)fr.y;
            r.uv = (uint64_t)(uintptr_t)fr.uv;
            r.out = outs ? (uint64_t)(uintptr_t)outs[base + i] : 0;
            r.pitch_y = pitch_or_width(fr.pitch_y, fr.width);
            r.pitch_uv = pitch_or_width(fr.pitch_uv, fr.width);
            warp_rec_geometry(w, fr.width, fr.height, r);
        }
    }
    // Every tile's bounding box, from the numbers the kernel computes.  The kernel decides per tile (need <= L.lds_bytes), so the launch takes the largest box that
    // fits the budget -- a launch may mix staged and gathering tiles -- and the count is of the warps whose every tile stages.
    int stage_budget(const RoiPlan &pl, WarpLaunch &L, int budget, bool luma_only) const {
        int staged = 0, lds = 0;
        for (int i = 0; i < L.n_warps; i++) {
            bool all = true;
            for (int ty = 0; ty < L.tiles_y; ty++)
                for (int tx = 0; tx < L.tiles_x; tx++) {
                    const int j0 = roi_tile_col0(tx, pl.dst_w, L.last_col0), i0 = ty * ROI_TILE_H;
                    RoiFootprint f;
                    warp_footprint(L.r[i], j0, tile_last(j0, ROI_TILE_W, pl.dst_w), i0, tile_last(i0, ROI_TILE_H, pl.dst_h), f);
                    const int need = roi_lds_need(f, luma_only);
                    if (roi_stageable(f) && need <= budget) lds = std::max(lds, need);
                    else all = false;
                }
            staged += all ? 1 : 0;
        }
        L.lds_bytes = lds;
        return staged;
    }
    int front_lds(const WarpLaunch &) const { return 0; }
    // (vpp_warp.hip and its tensor twin) one launch group, or only its kernel's name.  The staged kernel wherever ANY tile stages: `staged` counts whole warps
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const WarpLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_warps);
        return (tensor ? launch_warp_tensor : launch_warp)(pl.out, vec, L.lds_bytes > 0, border(), L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_warp%s n=%d frames=%d ->%dx%d fourcc=%d stream=%p", tensor ? "_tensor" : "", n_warps, n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "warps=%d frames=%d", n_warps, n_frames); }
    void suffix(char *buf, size_t len, const RoiPlan &) const {
        if (border()) std::snprintf(buf, len, " border=%d,%d,%d", border_y, border_u, border_v);
        else std::snprintf(buf, len, " border=replicate");
    }
    const char *mode_name(const RoiPlan &) const { return "warp_bilinear"; }
};

} // namespace

extern "C" {

int tsvpp_convert_warp(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, const tsvpp_params *p, int border_y, int border_u,
                       int border_v, void *const *outs, void *stream) {
    return tile_convert(WarpPath{ false, p, nullptr, n_frames, frames, n_warps, warps, border_y, border_u, border_v }, ctx, outs, stream);
}

int tsvpp_describe_warp(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, int border_y, int border_u, int border_v,
                        int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(WarpPath{ false, p, nullptr, n_frames, frames, n_warps, warps, border_y, border_u, border_v }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_warp_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, const tsvpp_params *p,
                              const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return tile_convert(WarpPath{ true, p, spec, n_frames, frames, n_warps, warps, border_y, border_u, border_v }, ctx, outs, stream);
}

int tsvpp_describe_warp_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps,
                               int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(WarpPath{ true, p, spec, n_frames, frames, n_warps, warps, border_y, border_u, border_v }, aligned_outputs, buf, buf_len);
}

int tsvpp_warp_rotated_box(double cx, double cy, double box_w, double box_h, double angle_rad, int dst_w, int dst_h, tsvpp_warp *out) {
    if (!out || !std::isfinite(cx) || !std::isfinite(cy) || !std::isfinite(box_w) || !std::isfinite(box_h) || !std::isfinite(angle_rad)) return TSVPP_ERROR;
    if (!(box_w > 0.0) || !(box_h > 0.0) || dst_w <= 0 || dst_h <= 0) return TSVPP_ERROR;
    const double c = std::cos(angle_rad), s = std::sin(angle_rad);
    const double m[6] = { box_w * c / dst_w, -box_h * s / dst_h, cx - 0.5 * box_w * c + 0.5 * box_h * s, box_w * s / dst_w, box_h * c / dst_h, cy - 0.5 * box_w * s - 0.5 * box_h * c };
    for (int k = 0; k < 6; k++) out->m[k] = (float)(m[k] + 0.0); // (+ 0.0: a zero entry is +0 whatever the signs of its factors)
    return TSVPP_OK;
}

int tsvpp_warp_footprint(const tsvpp_warp *warp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8) {
    if (!warp || !out8 || frame_w <= 0 || frame_h <= 0 || j_first < 0 || i_first < 0 || j_last < j_first || i_last < i_first) return TSVPP_ERROR;
    WarpRec r = {};
    warp_rec_geometry(*warp, frame_w, frame_h, r);
    RoiFootprint f;
    warp_footprint(r, j_first, j_last, i_first, i_last, f);
    const int32_t v[8] = { f.xlo, f.xhi, f.ylo, f.yhi, f.cxlo, f.cxhi, f.cylo, f.cyhi };
    for (int k = 0; k < 8; k++) out8[k] = v[k];
    return TSVPP_OK;
}

} // extern "C"
