// tsvpp_warp.cpp -- rotated and affine-warped boxes (include/tsvpp.h): tsvpp_convert_warp / tsvpp_describe_warp, their tensor forms (`spec`, null for the first
// pair; kernel vpp_warp_tensor.hip), tsvpp_convert_warp_bicubic / tsvpp_describe_warp_bicubic (BICUBIC: `spec` null or not; kernels
// vpp_warp_bicubic.hip / vpp_warp_bicubic_tensor.hip), tsvpp_warp_rotated_box and the DEBUG exports of the footprint functions; TSVPP_MAX_WARPS outputs per launch, kernel
// vpp_warp.hip.  The body is tsvpp_tiles.h's, and so is what the four coordinate paths share (CoordRequest); WarpPath below says what differs: the request rules
// (warp_plan, tsvpp_plan.cpp), the record's geometry, and the footprint function of the staging budget -- a warped tile's footprint is a bounding box of its own
// (warp_footprint, vpp_warp.h), no product of a column span and a row span.
#include <cmath>

#include "tsvpp_tiles.h"
#include "vpp_coord_bicubic.h"

using namespace tsvpp;

namespace {

// the record's geometry: everything the footprint function and the sampler read beyond the frame's size
void warp_rec_geometry(const tsvpp_warp &w, WarpRec &r) {
    r.m0 = w.m[0];
    r.m1 = w.m[1];
    r.m3 = w.m[3];
    r.m4 = w.m[4];
    warp_translations(w.m[2], w.m[5], r);
}

// The request of one call, as tsvpp_tiles.h asks for it.  CUBIC: the *_bicubic entry points -- the plan's resize type, the footprint function (the box with the 4-tap
// halo, vpp_coord_bicubic.h), the launchers and the names differ; the records and everything else are the BILINEAR call's
template <bool CUBIC> struct WarpPathT : CoordRequest {
    using Launch = WarpLaunch;
    static constexpr bool kCountsStaged = true;
    int n_warps;
    const tsvpp_warp *warps;

    int plan(RoiPlan &pl) const { return warp_plan(p, n_frames, frames, n_warps, warps, border_y, border_u, border_v, pl, CUBIC ? M_BICUBIC : M_BILINEAR); }
    int items() const { return n_warps; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_WARPS; }
    void fill_items(const RoiPlan &, void *const *outs, int base, int cnt, WarpLaunch &L) const {
        fill_launch(cnt, L);
        for (int i = 0; i < cnt; i++) {
            fill_rec(warps[base + i].frame, outs ? outs[base + i] : nullptr, L.r[i]);
            warp_rec_geometry(warps[base + i], L.r[i]);
        }
    }
    // every tile's bounding box (warp_footprint, vpp_warp.h; warp_bicubic_footprint, vpp_coord_bicubic.h)
    int stage_budget(const RoiPlan &pl, WarpLaunch &L, int budget, bool luma_only) const {
        if constexpr (CUBIC) return coord_box_budget<warp_bicubic_footprint>(pl, L, budget, luma_only);
        else return coord_box_budget<warp_footprint>(pl, L, budget, luma_only);
    }
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const WarpLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        return launch_with(CUBIC ? launch_warp_bicubic : launch_warp, CUBIC ? launch_warp_bicubic_tensor : launch_warp_tensor, pl, vec, L, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_warp%s%s n=%d frames=%d ->%dx%d fourcc=%d stream=%p", CUBIC ? "_bicubic" : "", tensor ? "_tensor" : "", n_warps, n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "warps=%d frames=%d", n_warps, n_frames); }
    const char *mode_name(const RoiPlan &) const { return CUBIC ? "warp_bicubic" : "warp_bilinear"; }
};
using WarpPath = WarpPathT<false>;
using WarpBicubicPath = WarpPathT<true>;

// the DEBUG exports: FOOTPRINT of one tile of `warp` on a frame of frame_w x frame_h
template <auto FOOTPRINT> int warp_footprint_export(const tsvpp_warp *warp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8) {
    if (!warp || !out8 || frame_w <= 0 || frame_h <= 0 || j_first < 0 || i_first < 0 || j_last < j_first || i_last < i_first) return TSVPP_ERROR;
    WarpRec r = {};
    r.src_w = frame_w;
    r.src_h = frame_h;
    warp_rec_geometry(*warp, r);
    RoiFootprint f;
    FOOTPRINT(r, j_first, j_last, i_first, i_last, f);
    footprint_export(f, out8);
    return TSVPP_OK;
}

} // namespace

extern "C" {

int tsvpp_convert_warp(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, const tsvpp_params *p, int border_y, int border_u,
                       int border_v, void *const *outs, void *stream) {
    return tile_convert(WarpPath{ { false, p, nullptr, n_frames, frames, border_y, border_u, border_v }, n_warps, warps }, ctx, outs, stream);
}

int tsvpp_describe_warp(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, int border_y, int border_u, int border_v,
                        int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(WarpPath{ { false, p, nullptr, n_frames, frames, border_y, border_u, border_v }, n_warps, warps }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_warp_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, const tsvpp_params *p,
                              const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return tile_convert(WarpPath{ { true, p, spec, n_frames, frames, border_y, border_u, border_v }, n_warps, warps }, ctx, outs, stream);
}

int tsvpp_describe_warp_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps,
                               int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(WarpPath{ { true, p, spec, n_frames, frames, border_y, border_u, border_v }, n_warps, warps }, aligned_outputs, buf, buf_len);
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
    return warp_footprint_export<warp_footprint>(warp, frame_w, frame_h, j_first, j_last, i_first, i_last, out8);
}

int tsvpp_convert_warp_bicubic(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps, const tsvpp_params *p,
                               const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return tile_convert(WarpBicubicPath{ { spec != nullptr, p, spec, n_frames, frames, border_y, border_u, border_v }, n_warps, warps }, ctx, outs, stream);
}

int tsvpp_describe_warp_bicubic(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_warps, const tsvpp_warp *warps,
                                int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(WarpBicubicPath{ { spec != nullptr, p, spec, n_frames, frames, border_y, border_u, border_v }, n_warps, warps }, aligned_outputs, buf, buf_len);
}

int tsvpp_warp_bicubic_footprint(const tsvpp_warp *warp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8) {
    return warp_footprint_export<warp_bicubic_footprint>(warp, frame_w, frame_h, j_first, j_last, i_first, i_last, out8);
}

} // extern "C"
