// tsvpp_persp.cpp -- homography-warped outputs (include/tsvpp.h): tsvpp_convert_perspective / tsvpp_describe_perspective, their tensor forms (`spec`, null for the
// first pair; kernel vpp_persp_tensor.hip), tsvpp_persp_from_quad and the DEBUG export of the footprint function; TSVPP_MAX_PERSP outputs per launch, kernel
// vpp_persp.hip.  The body is tsvpp_tiles.h's; PerspPath below says what differs, as WarpPath (tsvpp_warp.cpp) does: the request rules (persp_plan,
// tsvpp_plan.cpp), the record, and the staging budget -- a tile's footprint is its interval box (persp_footprint, vpp_persp.h).
#include <cmath>

#include "tsvpp_tiles.h"
#include "vpp_persp.h"

using namespace tsvpp;

namespace {

// the record's geometry: everything the footprint function and the sampler read (planes and output apart)
void persp_rec_geometry(const tsvpp_persp &q, int frame_w, int frame_h, PerspRec &r) {
    r.src_w = frame_w;
    r.src_h = frame_h;
    persp_terms(q.h, r.luma, r.chroma);
}

// The request of one call, as tsvpp_tiles.h asks for it
struct PerspPath {
    using Launch = PerspLaunch;
    static constexpr bool kOwnBudget = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // (may carry null planes: the describe calls)
    int n_persp;
    const tsvpp_persp *persps;
    int border_y, border_u, border_v;

    bool border() const { return border_y >= 0; }
    int plan(RoiPlan &pl) const { return persp_plan(p, n_frames, frames, n_persp, persps, border_y, border_u, border_v, pl); }
    int items() const { return n_persp; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_PERSP; }
    void fill_items(const RoiPlan &, void *const *outs, int base, int cnt, PerspLaunch &L) const {
        L.n_persp = cnt;
        L.border_y = (float)border_y;
        L.border_u = (float)border_u;
        L.border_v = (float)border_v;
        for (int i = 0; i < cnt; i++) {
            const tsvpp_persp &q = persps[base + i];
            const tsvpp_nv12 &fr = frames[q.frame];
            PerspRec &r = L.r[i];
            r.y = (uint64_t)(uintptr_t)fr.y;
            r.uv = (uint64_t)(uintptr_t)fr.uv;
            r.out = outs ? (uint64_t)(uintptr_t)outs[base + i] : 0;
            r.pitch_y = pitch_or_width(fr.pitch_y, fr.width);
            r.pitch_uv = pitch_or_width(fr.pitch_uv, fr.width);
            persp_rec_geometry(q, fr.width, fr.height, r);
        }
    }
    // Every tile's interval box, from the numbers the kernel computes.  The kernel decides per tile (need <= L.lds_bytes), so the launch takes the largest box that
    // fits the budget -- a launch may mix staged and gathering tiles -- and the count is of the outputs whose every tile stages.
    int stage_budget(const RoiPlan &pl, PerspLaunch &L, int budget, bool luma_only) const {
        int staged = 0, lds = 0;
        for (int i = 0; i < L.n_persp; i++) {
            bool all = true;
            for (int ty = 0; ty < L.tiles_y; ty++)
                for (int tx = 0; tx < L.tiles_x; tx++) {
                    const int j0 = roi_tile_col0(tx, pl.dst_w, L.last_col0), i0 = ty * ROI_TILE_H;
                    RoiFootprint f;
                    persp_footprint(L.r[i], j0, tile_last(j0, ROI_TILE_W, pl.dst_w), i0, tile_last(i0, ROI_TILE_H, pl.dst_h), f);
                    const int need = roi_lds_need(f, luma_only);
                    if (roi_stageable(f) && need <= budget) lds = std::max(lds, need);
                    else all = false;
                }
            staged += all ? 1 : 0;
        }
        L.lds_bytes = lds;
        return staged;
    }
    int front_lds(const PerspLaunch &) const { return 0; }
    // (vpp_persp.hip and its tensor twin) one launch group, or only its kernel's name.  The staged kernel wherever ANY tile stages: `staged` counts whole outputs
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const PerspLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_persp);
        return (tensor ? launch_persp_tensor : launch_persp)(pl.out, vec, L.lds_bytes > 0, border(), L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_perspective%s n=%d frames=%d ->%dx%d fourcc=%d stream=%p", tensor ? "_tensor" : "", n_persp, n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "warps=%d frames=%d", n_persp, n_frames); }
    void suffix(char *buf, size_t len, const RoiPlan &) const {
        if (border()) std::snprintf(buf, len, " border=%d,%d,%d", border_y, border_u, border_v);
        else std::snprintf(buf, len, " border=replicate");
    }
    const char *mode_name(const RoiPlan &) const { return "persp_bilinear"; }
};

} // namespace

extern "C" {

int tsvpp_convert_perspective(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, const tsvpp_params *p, int border_y,
                              int border_u, int border_v, void *const *outs, void *stream) {
    return tile_convert(PerspPath{ false, p, nullptr, n_frames, frames, n, persps, border_y, border_u, border_v }, ctx, outs, stream);
}

int tsvpp_describe_perspective(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, int border_y, int border_u,
                               int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(PerspPath{ false, p, nullptr, n_frames, frames, n, persps, border_y, border_u, border_v }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_perspective_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps, const tsvpp_params *p,
                                     const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return tile_convert(PerspPath{ true, p, spec, n_frames, frames, n, persps, border_y, border_u, border_v }, ctx, outs, stream);
}

int tsvpp_describe_perspective_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n, const tsvpp_persp *persps,
                                      int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(PerspPath{ true, p, spec, n_frames, frames, n, persps, border_y, border_u, border_v }, aligned_outputs, buf, buf_len);
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
    if (!persp || !out8 || frame_w <= 0 || frame_h <= 0 || j_first < 0 || i_first < 0 || j_last < j_first || i_last < i_first) return TSVPP_ERROR;
    PerspRec r = {};
    persp_rec_geometry(*persp, frame_w, frame_h, r);
    if (!(persp_min_denominator(r.luma, j_first, j_last, i_first, i_last) >= PERSP_MIN_DENOMINATOR)) return TSVPP_UNSUPPORTED;
    if (!(persp_min_denominator(r.chroma, j_first >> 1, j_last >> 1, i_first >> 1, i_last >> 1) >= PERSP_MIN_DENOMINATOR)) return TSVPP_UNSUPPORTED;
    RoiFootprint f;
    persp_footprint(r, j_first, j_last, i_first, i_last, f);
    const int32_t v[8] = { f.xlo, f.xhi, f.ylo, f.yhi, f.cxlo, f.cxhi, f.cylo, f.cyhi };
    for (int k = 0; k < 8; k++) out8[k] = v[k];
    return TSVPP_OK;
}

} // extern "C"
