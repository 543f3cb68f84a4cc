// tsvpp_rois.cpp -- regions of interest (include/tsvpp.h): many boxes of a few frames to one size, TSVPP_MAX_ROIS per launch.  Three pairs of entry points over one
// body: tsvpp_convert_rois / tsvpp_describe_rois (NEAREST, BILINEAR, BICUBIC; kernel vpp_rois.hip), tsvpp_convert_rois_area / tsvpp_describe_rois_area (AREA;
// kernel vpp_rois_area.hip) and tsvpp_convert_rois_tensor / tsvpp_describe_rois_tensor (all four; the tensor instantiations of both kernels, vpp_rois_tensor.hip /
// vpp_rois_area_tensor.hip).  The body is tsvpp_tiles.h's; RoiPath below says what differs: which resize types rois_plan lets through (`area`), the mode of a box (AREA:
// per box), and -- `tensor`, `spec` null for the first two pairs -- the launcher, the element size and the spec check behind the plan.
#include "tsvpp_tiles.h"

using namespace tsvpp;

namespace {

// The request of one call, as tsvpp_tiles.h asks for it
struct RoiPath {
    using Launch = RoiLaunch;
    static constexpr bool kInnerRect = false; // a box fills the whole output
    static constexpr bool kOwnBudget = false;
    static constexpr bool kCountsStaged = true;
    bool area, tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // (may carry null planes -- the describe calls: then the records hold the bare crop offsets)
    int n_rois;
    const tsvpp_roi *rois;

    int plan(RoiPlan &pl) const { return rois_plan(p, n_frames, frames, n_rois, rois, pl, area); }
    int items() const { return n_rois; }
    int limit(const RoiPlan &) const { return area ? (int)TSVPP_MAX_ROIS_AREA : (int)TSVPP_MAX_ROIS; }
    // L.area_lds = the bytes of the AREA kernel's weight rows in front of the staged footprint: the largest tap counts among the group's down-scale boxes (they
    // count against the LDS budget)
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, RoiLaunch &L) const {
        L.n_rois = cnt;
        L.area_lds = 0;
        for (int i = 0; i < cnt; i++) {
            const tsvpp_roi &b = rois[base + i];
            const tsvpp_nv12 &fr = frames[b.frame];
            RoiRec &r = L.r[i];
            r.pitch_y = pitch_or_width(fr.pitch_y, fr.width);
            r.pitch_uv = pitch_or_width(fr.pitch_uv, fr.width);
            const CropOff off = plane_offsets(b.left, b.top, r.pitch_y, r.pitch_uv); // the box is the crop
            r.y = (uint64_t)(uintptr_t)fr.y + off.y;
            r.uv = (uint64_t)(uintptr_t)fr.uv + off.uv;
            r.out = outs ? (uint64_t)(uintptr_t)outs[base + i] : 0;
            r.src_w = b.right - b.left;
            r.src_h = b.bottom - b.top;
            r.xr = (float)r.src_w / (float)pl.dst_w; // src/Resize.cu:418-419
            r.yr = (float)r.src_h / (float)pl.dst_h;
            if (area && roi_area_mode(r.xr, r.yr) == M_AREA_DOWN) L.area_lds = std::max(L.area_lds, roi_area_lds(roi_area_taps(r.xr), roi_area_taps(r.yr)));
        }
    }
    // AREA: the mode per box
    TileItem item(const RoiPlan &pl, const RoiLaunch &L, int i) const {
        const RoiRec &r = L.r[i];
        return TileItem{ area ? roi_area_mode(r.xr, r.yr) : (int)pl.mode, r.src_w, r.src_h, r.xr, r.yr, 0, 0, pl.dst_w, pl.dst_h };
    }
    int front_lds(const RoiLaunch &L) const { return L.area_lds; }
    // (vpp_rois.hip / vpp_rois_area.hip and their tensor twins) one launch group, or only its kernel's name
    hipError_t launch(const RoiPlan &pl, bool vec, bool staged, const RoiLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_rois);
        const size_t lds = (size_t)(L.area_lds + L.lds_bytes);
        if (area) return (tensor ? launch_rois_area_tensor : launch_rois_area)(pl.out, vec, staged, L, grid, lds, stream, name, name_len, dry_run);
        return (tensor ? launch_rois_tensor : launch_rois)(pl.mode, pl.out, vec, staged, L, grid, lds, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_rois%s n=%d frames=%d ->%dx%d mode=%d fourcc=%d stream=%p", tensor ? "_tensor" : (area ? "_area" : ""), n_rois, n_frames, pl.dst_w,
                      pl.dst_h, (int)pl.mode, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "rois=%d frames=%d", n_rois, n_frames); }
    const char *mode_name(const RoiPlan &pl) const { return pl.mode == M_AREA_DOWN ? "area" : mode_names[pl.mode]; }
    void suffix(char *buf, size_t len, const RoiPlan &pl) const {
        if (area) std::snprintf(buf, len, " down=%d taps=%dx%d", pl.down, pl.taps_x, pl.taps_y);
    }
};

// All four resize types behind the tensor entry points: AREA takes the AREA plan, kernel and launch limit, anything else tsvpp_convert_rois's.
bool tensor_area(const tsvpp_params *p) { return p && p->resize_type == TSVPP_AREA; }

} // namespace

extern "C" {

int tsvpp_convert_rois(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p, void *const *outs,
                       void *stream) {
    return tile_convert(RoiPath{ false, false, p, nullptr, n_frames, frames, n_rois, rois }, ctx, outs, stream);
}

int tsvpp_describe_rois(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, int aligned_outputs, char *buf,
                        size_t buf_len) {
    return tile_describe(RoiPath{ false, false, p, nullptr, n_frames, frames, n_rois, rois }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_rois_area(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p, void *const *outs,
                            void *stream) {
    return tile_convert(RoiPath{ true, false, p, nullptr, n_frames, frames, n_rois, rois }, ctx, outs, stream);
}

int tsvpp_describe_rois_area(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, int aligned_outputs, char *buf,
                             size_t buf_len) {
    return tile_describe(RoiPath{ true, false, p, nullptr, n_frames, frames, n_rois, rois }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_rois_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p,
                              const tsvpp_tensor_spec *spec, void *const *outs, void *stream) {
    return tile_convert(RoiPath{ tensor_area(p), true, p, spec, n_frames, frames, n_rois, rois }, ctx, outs, stream);
}

int tsvpp_describe_rois_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois,
                               int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(RoiPath{ tensor_area(p), true, p, spec, n_frames, frames, n_rois, rois }, aligned_outputs, buf, buf_len);
}

// The generator of vpp_rois_area.hip's weight rows (roi_area_step, vpp_rois.h), evaluated on the host: rows of output indices first .. first + n - 1.
int tsvpp_roi_area_rows(float scale, int first, int n, float *out, int max_floats, int *taps) {
    if (!out || first < 0 || n <= 0) return TSVPP_ERROR;
    if (!(scale > 1.0f) || (long)first + n > ROI_AREA_MAX_DST) return TSVPP_UNSUPPORTED;
    const int t = roi_area_taps(scale);
    if (t > ROI_AREA_MAX_TAPS) return TSVPP_UNSUPPORTED;
    if (taps) *taps = t;
    if ((long)n * t > (long)max_floats) return TSVPP_ERROR;
    RoiAreaGen g;
    for (int k = 0; k < first + n; k++) {
        const RoiAreaRow r = roi_area_step(scale, g);
        for (int e = 0; k >= first && e < t; e++) out[(long)(k - first) * t + e] = roi_area_weight(r, e);
    }
    return n;
}

} // extern "C"
