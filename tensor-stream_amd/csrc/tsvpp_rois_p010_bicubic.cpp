// tsvpp_rois_p010_bicubic.cpp -- the P010 region-of-interest call with the separable integer cubic (include/tsvpp.h): tsvpp_convert_rois_p010_bicubic /
// tsvpp_describe_rois_p010_bicubic, one pair whose `spec` may be null (the plain flavours) or given (the tensor flavours), and tsvpp_cubic_p010_plane, the
// contract's executable form on the host; TSVPP_MAX_ROIS_P010 boxes per launch, kernels vpp_rois_p010_bicubic.hip and vpp_rois_p010_bicubic_tensor.hip.  The
// request rules are the P010 ROI call's with BICUBIC in the place of NEAREST / BILINEAR and this call's limits behind them; the skeletons of both calls are
// tsvpp_tiles.h's.  Nothing here builds a table: the kernel computes every tap and weight in closed form from N and n, and what the host adds to the records
// is the LDS carve-up of the launch.
#include "tsvpp_cubic_p010.h"
#include "tsvpp_p010.h"
#include "tsvpp_tiles.h"
#include "vpp_rois_p010_bicubic.h"

using namespace tsvpp;

namespace {

// The status of a request, in the order that is part of the ABI: tsvpp_convert_rois_p010's (tsvpp_rois_p010.cpp), asked with a resize type that call accepts so
// that every rule in front of the type is its own; then the type, then this call's limits
int cubic_plan(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *fr, int n_rois, const tsvpp_roi *rois, bool converting, RoiPlan &pl) {
    if (!p) return TSVPP_ERROR;
    tsvpp_params q = *p;
    q.resize_type = TSVPP_BILINEAR;
    const int sts = p010_rois_plan(&q, n_frames, fr, n_rois, rois, converting, pl);
    if (sts != TSVPP_OK) return sts;
    if (p->resize_type != TSVPP_BICUBIC) return TSVPP_UNSUPPORTED;
    pl.mode = M_BICUBIC;
    if (std::max(pl.dst_w, pl.dst_h) > CUBIC_P010_MAX_SIDE) return TSVPP_UNSUPPORTED;
    for (int i = 0; i < n_rois; i++) {
        const int bw = rois[i].right - rois[i].left, bh = rois[i].bottom - rois[i].top;
        if (std::max(bw, bh) > CUBIC_P010_MAX_SIDE) return TSVPP_UNSUPPORTED;
        // N <= 8 n on both axes of both planes (chroma: halves of even numbers)
        if (bw > CUBIC_P010_MAX_RATIO * pl.dst_w || bh > CUBIC_P010_MAX_RATIO * pl.dst_h) return TSVPP_UNSUPPORTED;
        if ((bw >> 1) > CUBIC_P010_MAX_RATIO * (pl.dst_w >> 1) || (bh >> 1) > CUBIC_P010_MAX_RATIO * (pl.dst_h >> 1)) return TSVPP_UNSUPPORTED;
    }
    return TSVPP_OK;
}

// The request of one call, as tsvpp_tiles.h asks for it
struct RoiCubicPath {
    using Launch = RoiCubicLaunch;
    static constexpr bool kOwnBudget = true; // no footprint is staged whole: the budget buys Hbuf and band rows
    static constexpr bool kCountsStaged = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // byte-plane view of the P010 frames (may carry null planes -- the describe call: then the records hold the bare box offsets)
    int n_rois;
    const tsvpp_roi *rois;
    bool converting;
    int *band; // the describe call: receives the first launch's band height

    int plan(RoiPlan &pl) const { return cubic_plan(p, n_frames, frames, n_rois, rois, converting, pl); }
    int items() const { return n_rois; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_ROIS_P010; }
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, RoiCubicLaunch &L) const {
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
    // The LDS of a launch: Hbuf for the tallest footprint and band buffers for the widest footprint row among the tiles of its boxes, either plane -- the numbers
    // the kernel computes (columns and rows are independent).  L.band = 0: not even one-row bands fit the budget.  Every box walks its footprints through these
    // buffers: the count is all of them.
    int stage_budget(const RoiPlan &pl, RoiCubicLaunch &L, int budget, bool luma_only) const {
        int cpr = 1, hrows = 1, lo, hi;
        for (int i = 0; i < L.n_rois; i++) {
            const RoiRec &r = L.r[i];
            const CubicDiv ax = cubic_div_of(r.src_w, pl.dst_w), ay = cubic_div_of(r.src_h, pl.dst_h);
            const CubicDiv cx = cubic_div_of(r.src_w >> 1, pl.dst_w >> 1), cy = cubic_div_of(r.src_h >> 1, pl.dst_h >> 1);
            for (int tx = 0; tx < L.tiles_x; tx++) {
                const int j0 = roi_tile_col0(tx, pl.dst_w, L.last_col0), j1 = tile_last(j0, ROI_TILE_W, pl.dst_w);
                cubic_span(j0, j1, ax, lo, hi);
                cpr = std::max(cpr, roi_chunks(2 * (hi - lo + 1)));
                if (luma_only) continue;
                cubic_span(j0 >> 1, j1 >> 1, cx, lo, hi);
                cpr = std::max(cpr, roi_chunks(4 * (hi - lo + 1)));
            }
            for (int ty = 0; ty < L.tiles_y; ty++) {
                const int i0 = ty * ROI_TILE_H, i1 = tile_last(i0, ROI_TILE_H, pl.dst_h);
                cubic_span(i0, i1, ay, lo, hi);
                hrows = std::max(hrows, hi - lo + 1);
                if (luma_only) continue;
                cubic_span(i0 >> 1, i1 >> 1, cy, lo, hi);
                hrows = std::max(hrows, hi - lo + 1);
            }
        }
        L.band = cubic_band_rows(budget, hrows, cpr);
        L.band_cpr = cpr;
        L.hrows = hrows;
        L.lds_bytes = cubic_lds(hrows, std::max(L.band, 1), cpr);
        if (band) *band = L.band;
        return L.n_rois;
    }
    int front_lds(const RoiCubicLaunch &) const { return 0; }
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const RoiCubicLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        if (L.band < 1) return hipErrorNotSupported; // (cubic_fit_status has answered such a request before the skeleton runs)
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_rois);
        return (tensor ? launch_rois_p010_bicubic_tensor : launch_rois_p010_bicubic)(pl.out, vec, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_rois_p010_bicubic%s n=%d frames=%d ->%dx%d fourcc=%d stream=%p", tensor ? " tensor" : "", n_rois, n_frames, pl.dst_w, pl.dst_h,
                      p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "src=p010 rois=%d frames=%d", n_rois, n_frames); }
    const char *mode_name(const RoiPlan &) const { return "bicubic"; }
    void suffix(char *buf, size_t len, const RoiPlan &) const { std::snprintf(buf, len, " band=%d", band ? *band : 0); }
};

} // namespace

extern "C" {

int tsvpp_convert_rois_p010_bicubic(tsvpp_ctx *ctx, int n_frames, const tsvpp_p010 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p,
                                    const tsvpp_tensor_spec *spec, void *const *outs, void *stream) {
    const P010Frames<TSVPP_MAX_ROIS_P010> fr(n_frames, frames);
    const RoiCubicPath path{ spec != nullptr, p, spec, n_frames, fr.data, n_rois, rois, true, nullptr };
    if (ctx && outs && cubic_fit_status(path, ctx->knobs, outs, false) != TSVPP_OK) {
        clear_last_launch();
        return TSVPP_UNSUPPORTED;
    }
    return tile_convert(path, ctx, outs, stream);
}

int tsvpp_describe_rois_p010_bicubic(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_p010 *frames, int n_rois, const tsvpp_roi *rois,
                                     int aligned_outputs, char *buf, size_t buf_len) {
    const P010Frames<TSVPP_MAX_ROIS_P010> fr(n_frames, frames);
    int band = 0;
    const RoiCubicPath path{ spec != nullptr, p, spec, n_frames, fr.data, n_rois, rois, false, &band };
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

// One plane of samples through the kernel's own functions, in the kernel's order of passes: every source row horizontally, then the columns
int tsvpp_cubic_p010_plane(const uint16_t *src, int src_w, int src_h, uint16_t *dst, int dst_w, int dst_h) {
    if (!src || !dst || src_w <= 0 || src_h <= 0 || dst_w <= 0 || dst_h <= 0) return TSVPP_ERROR;
    if (std::max(std::max(src_w, src_h), std::max(dst_w, dst_h)) > CUBIC_P010_MAX_SIDE) return TSVPP_UNSUPPORTED; // (the ratio limit is the kernel's, not the arithmetic's)
    const CubicDiv ax = cubic_div_of(src_w, dst_w), ay = cubic_div_of(src_h, dst_h);
    std::vector<int16_t> h;
    try {
        h.resize((size_t)src_h * dst_w);
    } catch (...) { // no exception crosses the C boundary
        return TSVPP_ERROR;
    }
    int w[4];
    for (int j = 0; j < dst_w; j++) {
        const CubicTerm t = cubic_term(j, ax);
        cubic_weights(t.F, w);
        const int x0 = cubic_tap(t.p, 0, src_w), x1 = cubic_tap(t.p, 1, src_w), x2 = cubic_tap(t.p, 2, src_w), x3 = cubic_tap(t.p, 3, src_w);
        for (int y = 0; y < src_h; y++) {
            const uint16_t *s = src + (size_t)y * src_w;
            h[(size_t)y * dst_w + j] = (int16_t)cubic_round_h(cubic_sum(w, s[x0], s[x1], s[x2], s[x3]));
        }
    }
    for (int i = 0; i < dst_h; i++) {
        const CubicTerm t = cubic_term(i, ay);
        cubic_weights(t.F, w);
        const int16_t *r0 = h.data() + (size_t)cubic_tap(t.p, 0, src_h) * dst_w, *r1 = h.data() + (size_t)cubic_tap(t.p, 1, src_h) * dst_w;
        const int16_t *r2 = h.data() + (size_t)cubic_tap(t.p, 2, src_h) * dst_w, *r3 = h.data() + (size_t)cubic_tap(t.p, 3, src_h) * dst_w;
        for (int j = 0; j < dst_w; j++) dst[(size_t)i * dst_w + j] = (uint16_t)cubic_round_v(cubic_sum(w, r0[j], r1[j], r2[j], r3[j]));
    }
    return TSVPP_OK;
}

} // extern "C"
