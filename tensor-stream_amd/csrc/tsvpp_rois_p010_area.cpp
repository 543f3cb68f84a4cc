// tsvpp_rois_p010_area.cpp -- the P010 region-of-interest call with the exact box filter (include/tsvpp.h): tsvpp_convert_rois_p010_area /
// tsvpp_describe_rois_p010_area, one pair whose `spec` may be null (the plain flavours) or given (the tensor flavours); TSVPP_MAX_ROIS_P010 boxes per launch,
// kernels vpp_rois_p010_area.hip and vpp_rois_p010_area_tensor.hip.  The request rules are the P010 ROI call's with AREA in the place of NEAREST / BILINEAR and
// the box filter's two limits behind them; the skeletons of both calls are tsvpp_tiles.h's.  Nothing here builds a table: the kernel computes every tap and
// weight in closed form from N and n, and what the host adds to the records is the band height of the launch.
#include "tsvpp_p010.h"
#include "tsvpp_tiles.h"
#include "vpp_rois_p010_area.h"

using namespace tsvpp;

namespace {

// The status of a request, in the order that is part of the ABI: tsvpp_convert_rois_p010's (tsvpp_rois_p010.cpp), asked with a resize type that call accepts so
// that every rule in front of the type is its own; then the type, then the box filter's limits.  pl.taps_x / taps_y: the largest tap counts of the request
int box_rois_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *fr, int n_rois, const tsvpp_roi *rois, bool converting, RoiPlan &pl) {
    if (!p) return TSVPP_ERROR;
    tsvpp_params q = *p;
    q.resize_type = TSVPP_BILINEAR;
    const int sts = p010_rois_plan(&q, n_frames, fr, n_rois, rois, converting, pl);
    if (sts != TSVPP_OK) return sts;
    if (p->resize_type != TSVPP_AREA) return TSVPP_UNSUPPORTED;
    pl.mode = M_AREA_DOWN;
    pl.taps_x = pl.taps_y = 0;
    if (std::max(pl.dst_w, pl.dst_h) > BOX_P010_MAX_SIDE) return TSVPP_UNSUPPORTED;
    for (int i = 0; i < n_rois; i++)
        if (std::max(rois[i].right - rois[i].left, rois[i].bottom - rois[i].top) > BOX_P010_MAX_SIDE) return TSVPP_UNSUPPORTED;
    for (int i = 0; i < n_rois; i++) { // both planes (chroma: halves of even numbers)
        const int bw = rois[i].right - rois[i].left, bh = rois[i].bottom - rois[i].top;
        const int tx = std::max(box_max_taps(bw, pl.dst_w), box_max_taps(bw >> 1, pl.dst_w >> 1));
        const int ty = std::max(box_max_taps(bh, pl.dst_h), box_max_taps(bh >> 1, pl.dst_h >> 1));
        if (tx > BOX_P010_MAX_TAPS || ty > BOX_P010_MAX_TAPS) return TSVPP_UNSUPPORTED;
        pl.taps_x = std::max(pl.taps_x, tx);
        pl.taps_y = std::max(pl.taps_y, ty);
    }
    return TSVPP_OK;
}

// The request of one call, as tsvpp_tiles.h asks for it
struct RoiBoxPath {
    using Launch = RoiBoxLaunch;
    static constexpr bool kOwnBudget = true; // no footprint is staged whole: the budget buys band rows
    static constexpr bool kCountsStaged = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // byte-plane view of the P010 frames (may carry null planes -- the describe call: then the records hold the bare box offsets)
    int n_rois;
    const tsvpp_roi *rois;
    bool converting;
    int *band; // the describe call: receives the band height of the launch group filled last

    int plan(RoiPlan &pl) const { return box_rois_plan(p, n_frames, frames, n_rois, rois, converting, pl); }
    int items() const { return n_rois; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_ROIS_P010; }
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, RoiBoxLaunch &L) const {
        L.n_rois = cnt;
        L.area_lds = 0;
        for (int i = 0; i < cnt; i++) {
            const tsvpp_roi &b = rois[base + i];
            const tsvpp_nv12 &fr = frames[b.frame];
            RoiRec &r = L.r[i];
            r.pitch_y = fr.pitch_y;
            r.pitch_uv = fr.pitch_uv;
            // the box origin in BYTES (left and top are even): luma word (top, left), chroma pair (top / 2, left / 2) -- 4 bytes per pair, i.e. 2 * left again
            r.y = (uint64_t)(uintptr_t)fr.y + (size_t)b.top * (size_t)fr.pitch_y + 2 * (size_t)b.left;
            r.uv = (uint64_t)(uintptr_t)fr.uv + (size_t)(b.top / 2) * (size_t)fr.pitch_uv + 2 * (size_t)b.left;
            r.out = outs ? (uint64_t)(uintptr_t)outs[base + i] : 0;
            r.src_w = b.right - b.left;
            r.src_h = b.bottom - b.top;
            r.xr = (float)r.src_w / (float)pl.dst_w; // (not read by the kernel: its ratios are the integer pairs)
            r.yr = (float)r.src_h / (float)pl.dst_h;
        }
    }
    // The band height of a launch: what the budget holds at the widest footprint row among the tile columns of its boxes, either plane -- the numbers the kernel
    // computes.  0 where not even one row fits: the request is refused before a launch (box_fit_status).  Every box walks its footprints through these buffers:
    // the count is all of them.
    int stage_budget(const RoiPlan &pl, RoiBoxLaunch &L, int budget, bool luma_only) const {
        int widest = 1;
        for (int i = 0; i < L.n_rois; i++) {
            const RoiRec &r = L.r[i];
            for (int tx = 0; tx < L.tiles_x; tx++) {
                const int j0 = roi_tile_col0(tx, pl.dst_w, L.last_col0), j1 = tile_last(j0, ROI_TILE_W, pl.dst_w);
                int cpr = roi_box_cpr_y(j0, j1, r.src_w, pl.dst_w);
                if (!luma_only) cpr = std::max(cpr, roi_box_cpr_uv(j0, j1, r.src_w, pl.dst_w));
                widest = std::max(widest, cpr);
            }
        }
        L.band = roi_box_band(budget, widest);
        L.band_cpr = widest;
        L.lds_bytes = box_band_lds(std::max(L.band, 1), widest);
        if (band) *band = L.band;
        return L.n_rois;
    }
    int front_lds(const RoiBoxLaunch &) const { return 0; }
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const RoiBoxLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        if (L.band < 1) return hipErrorNotSupported; // (box_fit_status has answered such a request before the skeleton runs)
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_rois);
        return (tensor ? launch_rois_p010_area_tensor : launch_rois_p010_area)(pl.out, vec, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_rois_p010_area%s n=%d frames=%d ->%dx%d fourcc=%d stream=%p", tensor ? " tensor" : "", n_rois, n_frames, pl.dst_w, pl.dst_h,
                      p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "src=p010 rois=%d frames=%d", n_rois, n_frames); }
    const char *mode_name(const RoiPlan &) const { return "area"; }
    void suffix(char *buf, size_t len, const RoiPlan &pl) const { std::snprintf(buf, len, " taps=%dx%d band=%d", pl.taps_x, pl.taps_y, band ? *band : 0); }
};

// TSVPP_UNSUPPORTED where the widest tile of a launch does not fit the workgroup's LDS budget even with one-row bands; decided on the host, before the skeleton
// touches a device.  The default budget holds every request within the limits: the widest footprint row is 17 taps x 32 columns of luma words (or x 16 chroma
// pairs of two words) = 1088 bytes = ROI_BOX_MAX_CPR chunks, and one-row bands of it take 4224 bytes (vpp_rois_p010_area.h) behind at most 12 KiB of the store
// side's static LDS -- so the launch groups are only walked where a knob has shrunk the budget.  `outs`: the convert call's (null: describe, which says
// `aligned`).  A request the plan refuses is left to the skeleton.
int box_fit_status(const RoiBoxPath &path, const Knobs &kn, void *const *outs, bool aligned) {
    if (!kn.force_gather && kn.lds_budget_kb * 1024 - roi_static_lds(O_F32_MERGED, true) >= box_band_lds(1, ROI_BOX_MAX_CPR)) return TSVPP_OK;
    RoiPlan pl;
    if (tile_request(path, pl) != TSVPP_OK) return TSVPP_OK;
    const int n = path.items(), limit = path.limit(pl);
    for (int base = 0; base < n; base += limit) {
        const int cnt = std::min(n - base, limit);
        const bool vec = (outs ? outs_aligned16(outs + base, cnt) : aligned) && !narrow_tail(pl);
        RoiBoxLaunch L;
        tile_fill(path, kn, pl, nullptr, base, cnt, vec, L);
        if (L.band < 1) return TSVPP_UNSUPPORTED;
    }
    return TSVPP_OK;
}

} // namespace

extern "C" {

int tsvpp_convert_rois_p010_area(tsvpp_ctx *ctx, int n_frames, const tsvpp_p010 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p,
                                 const tsvpp_tensor_spec *spec, void *const *outs, void *stream) {
    const P010Frames<TSVPP_MAX_ROIS_P010> fr(n_frames, frames);
    const RoiBoxPath path{ spec != nullptr, p, spec, n_frames, fr.data, n_rois, rois, true, nullptr };
    if (ctx && outs && box_fit_status(path, ctx->knobs, outs, false) != TSVPP_OK) {
        clear_last_launch();
        return TSVPP_UNSUPPORTED;
    }
    return tile_convert(path, ctx, outs, stream);
}

int tsvpp_describe_rois_p010_area(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_p010 *frames, int n_rois, const tsvpp_roi *rois,
                                  int aligned_outputs, char *buf, size_t buf_len) {
    const P010Frames<TSVPP_MAX_ROIS_P010> fr(n_frames, frames);
    int band = 0;
    const RoiBoxPath path{ spec != nullptr, p, spec, n_frames, fr.data, n_rois, rois, false, &band };
    if (buf && buf_len) {
        Knobs kn; // as tile_describe's: no context
        read_env_knobs(kn);
        if (box_fit_status(path, kn, nullptr, aligned_outputs != 0) != TSVPP_OK) {
            buf[0] = 0;
            return TSVPP_UNSUPPORTED;
        }
    }
    return tile_describe(path, aligned_outputs, buf, buf_len);
}

} // extern "C"
