// tsvpp_letterbox_area.cpp -- the letterbox call with AREA (include/tsvpp.h): tsvpp_convert_letterbox_area / tsvpp_describe_letterbox_area -- one pair, `spec` null for
// the library's flavours and set for the tensor form -- and the debug export tsvpp_letterbox_area_rows; TSVPP_MAX_LETTERBOX frames per launch, kernels
// vpp_letterbox_area.hip / vpp_letterbox_area_tensor.hip.  The request rules are letterbox_area_plan's (tsvpp_plan.cpp), the spec's tensor_spec_status's.  The body is
// tsvpp_tiles.h's; the path below is tsvpp_letterbox.cpp's with the mode of a frame chosen per frame and the weight rows in front of the staged footprint, as
// tsvpp_rois.cpp's AREA path has them.  Nothing here searches a period or plans a tile on the way to a launch: the kernel does both.  The describe call alone
// walks the first launch's tiles, for its chain= key.
#include "tsvpp_tiles.h"
#include "vpp_letterbox_area.h"

using namespace tsvpp;

namespace {

// Steps the longer of a tile axis's two chains runs IN FRONT of its first row: inner indices [lo, ..] of an axis with ratio `scale` -- the luma chain from its
// jump start to lo, the chroma chain from its own to lo >> 1
int chain_lead(float scale, int lo) {
    const int period = lb_area_period(scale, lo);
    return std::max(lo - lb_area_start_of(period, lo), (lo >> 1) - lb_area_start_of(period, lo >> 1));
}

// The request of one call, as tsvpp_tiles.h asks for it
struct LbAreaPath {
    using Launch = LbAreaLaunch;
    static constexpr bool kInnerRect = true; // a frame fills its inner rectangle: tiles that miss it stage nothing
    static constexpr bool kOwnBudget = false;
    static constexpr bool kCountsStaged = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // (may carry null planes: the describe call)
    const tsvpp_rect *rects;
    int pad_y, pad_u, pad_v;
    int *chain; // the describe call: receives the longest chain lead of the first launch's tiles.  Null when converting: no host work per tile

    int plan(RoiPlan &pl) const { return letterbox_area_plan(p, n_frames, frames, rects, pad_y, pad_u, pad_v, pl); }
    int items() const { return n_frames; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_LETTERBOX; }
    // L.area_lds = the bytes of the weight rows in front of the staged footprint: the largest tap counts among the group's down-scale frames
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, LbAreaLaunch &L) const {
        L.n_frames = cnt;
        L.pad_y = (float)pad_y;
        L.pad_u = (float)pad_u;
        L.pad_v = (float)pad_v;
        L.area_lds = 0;
        for (int i = 0; i < cnt; i++) {
            const tsvpp_nv12 &fr = frames[base + i];
            const tsvpp_rect rc = letterbox_rect_of(frames, rects, base + i, pl.dst_w, pl.dst_h);
            LbRec &r = L.r[i];
            r.y = (uint64_t)(uintptr_t)fr.y;
            r.uv = (uint64_t)(uintptr_t)fr.uv;
            r.out = outs ? (uint64_t)(uintptr_t)outs[base + i] : 0;
            r.pitch_y = pitch_or_width(fr.pitch_y, fr.width);
            r.pitch_uv = pitch_or_width(fr.pitch_uv, fr.width);
            r.src_w = fr.width;
            r.src_h = fr.height;
            r.xr = (float)r.src_w / (float)rc.width; // src/Resize.cu:418-419, the rectangle as the output
            r.yr = (float)r.src_h / (float)rc.height;
            r.left = rc.left;
            r.top = rc.top;
            r.width = rc.width;
            r.height = rc.height;
            if (roi_area_mode(r.xr, r.yr) == M_AREA_DOWN) L.area_lds = std::max(L.area_lds, roi_area_lds(roi_area_taps(r.xr), roi_area_taps(r.yr)));
        }
        if (chain && base == 0) *chain = longest_chain(pl, L, cnt);
    }
    // the tiles of a launch as the kernel walks them: every tile column / row that touches a down-scale frame's rectangle
    static int longest_chain(const RoiPlan &pl, const LbAreaLaunch &L, int cnt) {
        int longest = 0, lo, hi;
        for (int i = 0; i < cnt; i++) {
            const LbRec &r = L.r[i];
            if (roi_area_mode(r.xr, r.yr) != M_AREA_DOWN) continue;
            for (int tx = 0; tx < L.tiles_x; tx++) {
                const int j = roi_tile_col0(tx, pl.dst_w, L.last_col0);
                tile_inner_range(j, tile_last(j, ROI_TILE_W, pl.dst_w), r.left, r.width, lo, hi);
                if (lo <= hi) longest = std::max(longest, chain_lead(r.xr, lo));
            }
            for (int ty = 0; ty < L.tiles_y; ty++) {
                tile_inner_range(ty * ROI_TILE_H, tile_last(ty * ROI_TILE_H, ROI_TILE_H, pl.dst_h), r.top, r.height, lo, hi);
                if (lo <= hi) longest = std::max(longest, chain_lead(r.yr, lo));
            }
        }
        return longest;
    }
    // the mode per frame
    TileItem item(const RoiPlan &, const LbAreaLaunch &L, int i) const {
        const LbRec &r = L.r[i];
        return TileItem{ roi_area_mode(r.xr, r.yr), r.src_w, r.src_h, r.xr, r.yr, r.left, r.top, r.width, r.height };
    }
    int front_lds(const LbAreaLaunch &L) const { return L.area_lds; }
    hipError_t launch(const RoiPlan &pl, bool vec, bool staged, const LbAreaLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_frames);
        return (tensor ? launch_letterbox_area_tensor : launch_letterbox_area)(pl.out, vec, staged, L, grid, (size_t)(L.area_lds + L.lds_bytes), stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_letterbox_area%s n=%d ->%dx%d fourcc=%d stream=%p", tensor ? " tensor" : "", n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "frames=%d", n_frames); }
    const char *mode_name(const RoiPlan &) const { return "area"; }
    void suffix(char *buf, size_t len, const RoiPlan &pl) const {
        const tsvpp_rect r0 = letterbox_rect_of(frames, rects, 0, pl.dst_w, pl.dst_h);
        std::snprintf(buf, len, " inner=%dx%d+%d+%d down=%d taps=%dx%d chain=%d", r0.width, r0.height, r0.left, r0.top, pl.down, pl.taps_x, pl.taps_y, chain ? *chain : 0);
    }
};

} // namespace

extern "C" {

int tsvpp_convert_letterbox_area(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec, const tsvpp_rect *rects, int pad_y,
                                 int pad_u, int pad_v, void *const *outs, void *stream) {
    return tile_convert(LbAreaPath{ spec != nullptr, p, spec, n, in, rects, pad_y, pad_u, pad_v, nullptr }, ctx, outs, stream);
}

int tsvpp_describe_letterbox_area(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int aligned_outputs,
                                  char *buf, size_t buf_len) {
    int chain = 0;
    return tile_describe(LbAreaPath{ spec != nullptr, p, spec, n, in, rects, 0, 0, 0, &chain }, aligned_outputs, buf, buf_len); // (the pad is no part of what is launched)
}

// The generator of vpp_letterbox_area.hip's weight rows, evaluated on the host as a chain lane of the kernel runs it: begun at the jump start of (scale, first) with
// the initial state, stepped to first + n - 1.
int tsvpp_letterbox_area_rows(float scale, int first, int n, float *out, int max_floats, int *taps, int *start) {
    if (!out || first < 0 || n <= 0) return TSVPP_ERROR;
    if (!(scale > 1.0f) || (long)first + n > ROI_AREA_MAX_DST) return TSVPP_UNSUPPORTED;
    const int t = roi_area_taps(scale);
    if (t > ROI_AREA_MAX_TAPS) return TSVPP_UNSUPPORTED;
    if (taps) *taps = t;
    if ((long)n * t > (long)max_floats) return TSVPP_ERROR;
    const int s = lb_area_chain_start(scale, first);
    if (start) *start = s;
    RoiAreaGen g;
    for (int k = s; k < first + n; k++) {
        const RoiAreaRow r = roi_area_step(scale, g);
        for (int e = 0; k >= first && e < t; e++) out[(long)(k - first) * t + e] = roi_area_weight(r, e);
    }
    return n;
}

} // extern "C"
