// tsvpp_persp.cpp -- homography-warped outputs (include/tsvpp.h): tsvpp_convert_perspective / tsvpp_describe_perspective, their tensor forms (`spec`, null for the
// first pair; kernel vpp_persp_tensor.hip), tsvpp_convert_perspective_bicubic / tsvpp_describe_perspective_bicubic (BICUBIC: `spec` null or not;
// kernels vpp_persp_bicubic.hip / vpp_persp_bicubic_tensor.hip), tsvpp_persp_from_quad and the DEBUG exports of the footprint functions; TSVPP_MAX_PERSP outputs per launch, kernel
// vpp_persp.hip.  The body is tsvpp_tiles.h's, and so is what the four coordinate paths share (CoordRequest); PerspPath below says what differs: the request
// rules (persp_plan, tsvpp_plan.cpp), the record's geometry, and the footprint function of the staging budget -- a tile's footprint is its interval box
// (persp_footprint, vpp_persp.h).
#include <cmath>

#include "tsvpp_tiles.h"
#include "vpp_coord_bicubic.h"

using namespace tsvpp;

namespace {

// The request of one call, as tsvpp_tiles.h asks for it.  CUBIC: the *_bicubic entry points, as WarpPathT's (tsvpp_warp.cpp)
template <bool CUBIC> struct PerspPathT : CoordRequest {
    using Launch = PerspLaunch;
    static constexpr bool kCountsStaged = true;
    int n_persp;
    const tsvpp_persp *persps;

    int plan(RoiPlan &pl) const { return persp_plan(p, n_frames, frames, n_persp, persps, border_y, border_u, border_v, pl, CUBIC ? M_BICUBIC : M_BILINEAR); }
    int items() const { return n_persp; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_PERSP; }
    // (the record's geometry is persp_terms: everything the footprint function and the sampler read beyond the frame's size)
    void fill_items(const RoiPlan &, void *const *outs, int base, int cnt, PerspLaunch &L) const {
        fill_launch(cnt, L);
        for (int i = 0; i < cnt; i++) {
            fill_rec(persps[base + i].frame, outs ? outs[base + i] : nullptr, L.r[i]);
            persp_terms(persps[base + i].h, L.r[i].luma, L.r[i].chroma);
        }
    }
    // every tile's interval box (persp_footprint, vpp_persp.h; persp_bicubic_footprint, vpp_coord_bicubic.h)
    int stage_budget(const RoiPlan &pl, PerspLaunch &L, int budget, bool luma_only) const {
        if constexpr (CUBIC) return coord_box_budget<persp_bicubic_footprint>(pl, L, budget, luma_only);
        else return coord_box_budget<persp_footprint>(pl, L, budget, luma_only);
    }
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const PerspLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        return launch_with(CUBIC ? launch_persp_bicubic : launch_persp, CUBIC ? launch_persp_bicubic_tensor : launch_persp_tensor, pl, vec, L, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_perspective%s%s n=%d frames=%d ->%dx%d fourcc=%d stream=%p", CUBIC ? "_bicubic" : "", tensor ? "_tensor" : "", n_persp, n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "warps=%d frames=%d", n_persp, n_frames); } // (warps=: describe_warp's keys)
    const char *mode_name(const RoiPlan &) const { return CUBIC ? "persp_bicubic" : "persp_bilinear"; }
};
using PerspPath = PerspPathT<false>;
using PerspBicubicPath = PerspPathT<true>;

// the DEBUG exports: FOOTPRINT of one tile of `persp` on a frame of frame_w x frame_h
template <auto FOOTPRINT> int persp_footprint_export(const tsvpp_persp *persp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8) {
    if (!persp || !out8 || frame_w <= 0 || frame_h <= 0 || j_first < 0 || i_first < 0 || j_last < j_first || i_last < i_first) return TSVPP_ERROR;
    PerspRec r = {};
    r.src_w = frame_w;
    r.src_h = frame_h;
    persp_terms(persp->h, r.luma, r.chroma);
    if (!(persp_min_denominator(r.luma, j_first, j_last, i_first, i_last) >= PERSP_MIN_DENOMINATOR)) return TSVPP_UNSUPPORTED;
    if (!(persp_min_denominator(r.chroma, j_first >> 1, j_last >> 1, i_first >> 1, i_last >> 1) >= PERSP_MIN_DENOMINATOR)) return TSVPP_UNSUPPORTED;
    RoiFootprint f;
    FOOTPRINT(r, j_first, j_last, i_first, i_last, f);
    footprint_export(f, out8);
    return TSVPP_OK;
}

} // namespace

extern "C" {

int tsvpp_convert_perspective(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, const tsvpp_params *p, int border_y,
                              int border_u, int border_v, void *const *outs, void *stream) {
    return tile_convert(PerspPath{ { false, p, nullptr, n_frames, frames, border_y, border_u, border_v }, n, persps }, ctx, outs, stream);
}

int tsvpp_describe_perspective(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, int border_y, int border_u,
                               int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(PerspPath{ { false, p, nullptr, n_frames, frames, border_y, border_u, border_v }, n, persps }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_perspective_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, const tsvpp_params *p,
                                     const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return tile_convert(PerspPath{ { true, p, spec, n_frames, frames, border_y, border_u, border_v }, n, persps }, ctx, outs, stream);
}

int tsvpp_describe_perspective_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps,
                                      int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(PerspPath{ { true, p, spec, n_frames, frames, border_y, border_u, border_v }, n, persps }, aligned_outputs, buf, buf_len);
}

int tsvpp_persp_from_quad(const double quad[8], int dst_w, int dst_h, tsvpp_persp *out) {
    if (!quad || !out || dst_w <= 0 || dst_h <= 0) return TSVPP_ERROR;
    for (int k = 0; k < 8; k++)
        if (!std::isfinite(quad[k])) return TSVPP_ERROR;
    const double x0 = quad[0], y0 = quad[1], x1 = quad[2], y1 = quad[3], x2 = quad[4], y2 = quad[5], x3 = quad[6], y3 = quad[7];
    const double sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3;
    double g = 0.0, h = 0.0;
    if (sx != 0.0 || sy != 0.0) { // (else a parallelogram: the map is affine)
        const double dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
        const double den = dx1 * dy2 - dx2 * dy1;
        if (den == 0.0) return TSVPP_ERROR;
        g = (sx * dy2 - dx2 * sy) / den;
        h = (dx1 * sy - sx * dy1) / den;
    }
    const double m[9] = { (x1 - x0 + g * x1) / dst_w, (x3 - x0 + h * x3) / dst_h, x0, (y1 - y0 + g * y1) / dst_w, (y3 - y0 + h * y3) / dst_h, y0, g / dst_w, h / dst_h, 1.0 };
    for (int k = 0; k < 9; k++) out->h[k] = (float)(m[k] + 0.0); // (+ 0.0: a zero entry is +0 whatever the signs of its factors)
    return TSVPP_OK;
}

int tsvpp_persp_footprint(const tsvpp_persp *persp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8) {
    return persp_footprint_export<persp_footprint>(persp, frame_w, frame_h, j_first, j_last, i_first, i_last, out8);
}

int tsvpp_convert_perspective_bicubic(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, const tsvpp_params *p,
                                      const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return tile_convert(PerspBicubicPath{ { spec != nullptr, p, spec, n_frames, frames, border_y, border_u, border_v }, n, persps }, ctx, outs, stream);
}

int tsvpp_describe_perspective_bicubic(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps,
                                       int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(PerspBicubicPath{ { spec != nullptr, p, spec, n_frames, frames, border_y, border_u, border_v }, n, persps }, aligned_outputs, buf, buf_len);
}

int tsvpp_persp_bicubic_footprint(const tsvpp_persp *persp, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last, int32_t *out8) {
    return persp_footprint_export<persp_bicubic_footprint>(persp, frame_w, frame_h, j_first, j_last, i_first, i_last, out8);
}

} // extern "C"
