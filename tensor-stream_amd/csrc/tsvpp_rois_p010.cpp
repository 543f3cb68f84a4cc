// tsvpp_rois_p010.cpp -- the region-of-interest call for 10-bit P010 sources (include/tsvpp.h): tsvpp_convert_rois_p010 / tsvpp_describe_rois_p010, one pair whose
// `spec` may be null (the plain flavours) or given (the tensor flavours); TSVPP_MAX_ROIS_P010 boxes per launch, kernels vpp_rois_p010.hip and
// vpp_rois_p010_tensor.hip.  The request rules are rois_plan's (tsvpp_plan.cpp) on the frames seen as byte planes, with this file's additions in front of and
// behind them; the skeletons of both calls are tsvpp_tiles.h's.
#include "tsvpp_p010.h"
#include "tsvpp_tiles.h"
#include "vpp_rois_p010.h"

using namespace tsvpp;

namespace tsvpp {

// The status of a request, in the order that is part of the ABI: the ROI call's, with the P010 rules in its two classes
// (`converting`: the planes are read, so their addresses must hold 16-bit words).  Declared in tsvpp_p010.h: the BICUBIC call asks it too
int p010_rois_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *fr, int n_rois, const tsvpp_roi *rois, bool converting, RoiPlan &pl) {
    if (!p || !fr || !rois || n_frames <= 0 || n_rois <= 0) return TSVPP_ERROR;
    if (p010_frames_error(n_frames, fr) != TSVPP_OK) return TSVPP_ERROR;
    if (converting && p010_planes_error(n_frames, fr) != TSVPP_OK) return TSVPP_ERROR;
    const int sts = rois_plan(p, n_frames, fr, n_rois, rois, pl); // (its pitch and span rules are weaker than the ones here)
    if (sts != TSVPP_OK) return sts;
    for (int i = 0; i < n_rois; i++) // a chroma pair has no half: the 8-bit call's U / V swap at an odd `left` is not part of this contract
        if ((rois[i].left | rois[i].top) & 1) return TSVPP_UNSUPPORTED;
    if (pl.mode != M_NEAREST && pl.mode != M_BILINEAR) return TSVPP_UNSUPPORTED; // BICUBIC (AREA and unknown types: rois_plan's answer)
    for (int i = 0; i < n_rois; i++) { // the source limit, per box, rows counted in 2 * width bytes: the kernel is handed the planes advanced to the box's origin
        const tsvpp_nv12 &f = fr[rois[i].frame];
        const int bw = rois[i].right - rois[i].left, bh = rois[i].bottom - rois[i].top;
        if (!plane_span_ok(bh, f.pitch_y, 2 * bw) || !plane_span_ok(bh >> 1, f.pitch_uv, 2 * bw)) return TSVPP_UNSUPPORTED;
    }
    return TSVPP_OK;
}

} // namespace tsvpp

namespace {

// The request of one call, as tsvpp_tiles.h asks for it
struct RoiP010Path {
    using Launch = RoiLaunch;
    static constexpr bool kOwnBudget = true; // footprints of 16-bit words: p010_lds_need, not the byte planes' roi_lds_need
    static constexpr bool kCountsStaged = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // byte-plane view of the P010 frames (may carry null planes -- the describe call: then the records hold the bare box offsets)
    int n_rois;
    const tsvpp_roi *rois;
    bool converting;

    int plan(RoiPlan &pl) const { return p010_rois_plan(p, n_frames, frames, n_rois, rois, converting, pl); }
    int items() const { return n_rois; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_ROIS_P010; }
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, RoiLaunch &L) const {
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
            r.xr = (float)r.src_w / (float)pl.dst_w;
            r.yr = (float)r.src_h / (float)pl.dst_h;
        }
    }
    // tile_item_need (tsvpp_tiles.h) in 16-bit words: the largest staged footprint among the tiles of a box, from the numbers the kernel computes (columns and rows
    // are independent, and p010_lds_bytes grows with each).  The kernel decides per tile, so the launch takes the largest need that fits the budget; the count is
    // of the boxes whose every tile stages.
    int stage_budget(const RoiPlan &pl, RoiLaunch &L, int budget, bool luma_only) const {
        int staged = 0, lds = 0;
        for (int i = 0; i < L.n_rois; i++) {
            const RoiRec &r = L.r[i];
            RoiFootprint f;
            int cy = 0, cuv = 0, ny = 0, nuv = 0;
            for (int tx = 0; tx < L.tiles_x; tx++) {
                const int lo = roi_tile_col0(tx, pl.dst_w, L.last_col0);
                tile_span_x(pl.mode, lo, tile_last(lo, ROI_TILE_W, pl.dst_w), r.src_w, r.xr, f);
                cy = std::max(cy, roi_chunks(p010_span_y(f.xhi - f.xlo + 1)));
                cuv = std::max(cuv, roi_chunks(p010_span_uv(f.cxhi - f.cxlo + 1)));
            }
            for (int ty = 0; ty < L.tiles_y; ty++) {
                const int lo = ty * ROI_TILE_H;
                tile_span_y(pl.mode, lo, tile_last(lo, ROI_TILE_H, pl.dst_h), r.src_h, r.yr, f);
                ny = std::max(ny, f.yhi - f.ylo + 1);
                nuv = std::max(nuv, luma_only ? 0 : f.cyhi - f.cylo + 1);
            }
            const long need = p010_lds_bytes(ny, cy, nuv, cuv);
            if (cy <= ROI_THREADS && cuv <= ROI_THREADS && need <= budget) {
                staged++;
                lds = std::max(lds, (int)need);
            }
        }
        L.lds_bytes = lds;
        return staged;
    }
    int front_lds(const RoiLaunch &) const { return 0; }
    hipError_t launch(const RoiPlan &pl, bool vec, bool staged, const RoiLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_rois);
        return (tensor ? launch_rois_p010_tensor : launch_rois_p010)(pl.mode, pl.out, vec, staged, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_rois_p010%s n=%d frames=%d ->%dx%d mode=%d fourcc=%d stream=%p", tensor ? " tensor" : "", n_rois, n_frames, pl.dst_w, pl.dst_h,
                      (int)pl.mode, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "src=p010 rois=%d frames=%d", n_rois, n_frames); }
    const char *mode_name(const RoiPlan &pl) const { return mode_names[pl.mode]; }
    void suffix(char *, size_t, const RoiPlan &) const {}
};

} // namespace

extern "C" {

int tsvpp_convert_rois_p010(tsvpp_ctx *ctx, int n_frames, const tsvpp_p010 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p,
                            const tsvpp_tensor_spec *spec, void *const *outs, void *stream) {
    const P010Frames<TSVPP_MAX_ROIS_P010> fr(n_frames, frames);
    return tile_convert(RoiP010Path{ spec != nullptr, p, spec, n_frames, fr.data, n_rois, rois, true }, ctx, outs, stream);
}

int tsvpp_describe_rois_p010(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_p010 *frames, int n_rois, const tsvpp_roi *rois,
                             int aligned_outputs, char *buf, size_t buf_len) {
    const P010Frames<TSVPP_MAX_ROIS_P010> fr(n_frames, frames);
    return tile_describe(RoiP010Path{ spec != nullptr, p, spec, n_frames, fr.data, n_rois, rois, false }, aligned_outputs, buf, buf_len);
}

} // extern "C"
