// tsvpp_letterbox_p010.cpp -- the letterbox call for 10-bit P010 sources (include/tsvpp.h): tsvpp_convert_letterbox_p010 / tsvpp_describe_letterbox_p010, one pair
// whose `spec` may be null (the plain flavours) or given (the tensor flavours); TSVPP_MAX_LETTERBOX_P010 frames per launch, kernels vpp_letterbox_p010.hip and
// vpp_letterbox_p010_tensor.hip.  The request rules are letterbox_plan's (tsvpp_plan.cpp) on the frames seen as byte planes, with this file's additions in front of
// and behind them; the skeletons of both calls are tsvpp_tiles.h's.
#include "tsvpp_p010.h"
#include "tsvpp_tiles.h"
#include "vpp_letterbox_p010.h"

using namespace tsvpp;

static_assert(TSVPP_MAX_LETTERBOX_P010 == TSVPP_MAX_LETTERBOX, "the P010 entry point fills the letterbox launch block");

namespace {

// The status of a request, in the order that is part of the ABI: the letterbox call's, with the P010 rules in its two classes
// (`converting`: the planes are read, so their addresses must hold 16-bit words)
int p010_plan(const tsvpp_params *p, int n, const tsvpp_nv12 *fr, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, bool converting, RoiPlan &pl) {
    if (!p || !fr || n <= 0) return TSVPP_ERROR;
    if (p010_frames_error(n, fr) != TSVPP_OK) return TSVPP_ERROR;
    if (pad_y < 0 || pad_y > 1023 || pad_u < 0 || pad_u > 1023 || pad_v < 0 || pad_v > 1023) return TSVPP_ERROR;
    if (converting && p010_planes_error(n, fr) != TSVPP_OK) return TSVPP_ERROR;
    const int sts = letterbox_plan(p, n, fr, rects, 0, 0, 0, pl); // (its pitch and span rules are weaker than the ones here)
    if (sts != TSVPP_OK) return sts;
    if (pl.mode != M_NEAREST && pl.mode != M_BILINEAR) return TSVPP_UNSUPPORTED; // BICUBIC (AREA and unknown types: letterbox_plan's answer)
    for (int f = 0; f < n; f++)
        if (!plane_span_ok(fr[f].height, fr[f].pitch_y, 2 * fr[f].width) || !plane_span_ok(fr[f].height >> 1, fr[f].pitch_uv, 2 * fr[f].width)) return TSVPP_UNSUPPORTED;
    return TSVPP_OK;
}

// The request of one call, as tsvpp_tiles.h asks for it
struct LbP010Path {
    using Launch = LbLaunch;
    static constexpr bool kOwnBudget = true; // footprints of 16-bit words: p010_lds_need, not the byte planes' roi_lds_need
    static constexpr bool kCountsStaged = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // byte-plane view of the P010 frames (may carry null planes: the describe call)
    const tsvpp_rect *rects;
    int pad_y, pad_u, pad_v;
    bool converting;

    int plan(RoiPlan &pl) const { return p010_plan(p, n_frames, frames, rects, pad_y, pad_u, pad_v, converting, pl); }
    int items() const { return n_frames; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_LETTERBOX_P010; }
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, LbLaunch &L) const {
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
            r.xr = (float)r.src_w / (float)rc.width;
            r.yr = (float)r.src_h / (float)rc.height;
            r.left = rc.left;
            r.top = rc.top;
            r.width = rc.width;
            r.height = rc.height;
        }
    }
    // tile_item_need (tsvpp_tiles.h) in 16-bit words: the largest staged footprint among the tiles of a frame that touch its rectangle, from the numbers the kernel
    // computes (columns and rows are independent, and p010_lds_bytes grows with each).  The kernel decides per tile, so the launch takes the largest need that fits
    // the budget; the count is of the frames whose every tile stages.
    int stage_budget(const RoiPlan &pl, LbLaunch &L, int budget, bool luma_only) const {
        int staged = 0, lds = 0;
        for (int i = 0; i < L.n_frames; i++) {
            const LbRec &r = L.r[i];
            RoiFootprint f;
            int cy = 0, cuv = 0, ny = 0, nuv = 0, lo, hi;
            for (int tx = 0; tx < L.tiles_x; tx++) {
                lo = roi_tile_col0(tx, pl.dst_w, L.last_col0);
                tile_inner_range(lo, tile_last(lo, ROI_TILE_W, pl.dst_w), r.left, r.width, lo, hi);
                if (lo > hi) continue;
                tile_span_x(pl.mode, lo, hi, r.src_w, r.xr, f);
                cy = std::max(cy, roi_chunks(p010_span_y(f.xhi - f.xlo + 1)));
                cuv = std::max(cuv, roi_chunks(p010_span_uv(f.cxhi - f.cxlo + 1)));
            }
            for (int ty = 0; ty < L.tiles_y; ty++) {
                lo = ty * ROI_TILE_H;
                tile_inner_range(lo, tile_last(lo, ROI_TILE_H, pl.dst_h), r.top, r.height, lo, hi);
                if (lo > hi) continue;
                tile_span_y(pl.mode, lo, hi, r.src_h, r.yr, f);
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
    int front_lds(const LbLaunch &) const { return 0; }
    hipError_t launch(const RoiPlan &pl, bool vec, bool staged, const LbLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_frames);
        return (tensor ? launch_letterbox_p010_tensor : launch_letterbox_p010)(pl.mode, pl.out, vec, staged, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_letterbox_p010%s n=%d ->%dx%d mode=%d fourcc=%d stream=%p", tensor ? " tensor" : "", n_frames, pl.dst_w, pl.dst_h, (int)pl.mode, p->fourcc, stream);
    }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "src=p010 frames=%d", n_frames); }
    const char *mode_name(const RoiPlan &pl) const { return mode_names[pl.mode]; }
    void suffix(char *buf, size_t len, const RoiPlan &pl) const {
        const tsvpp_rect r0 = letterbox_rect_of(frames, rects, 0, pl.dst_w, pl.dst_h);
        std::snprintf(buf, len, " inner=%dx%d+%d+%d", r0.width, r0.height, r0.left, r0.top);
    }
};

} // namespace

extern "C" {

int tsvpp_convert_letterbox_p010(tsvpp_ctx *ctx, int n, const tsvpp_p010 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec, const tsvpp_rect *rects, int pad_y,
                                 int pad_u, int pad_v, void *const *outs, void *stream) {
    const P010Frames<TSVPP_MAX_LETTERBOX_P010> fr(n, in);
    return tile_convert(LbP010Path{ spec != nullptr, p, spec, n, fr.data, rects, pad_y, pad_u, pad_v, true }, ctx, outs, stream);
}

int tsvpp_describe_letterbox_p010(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n, const tsvpp_p010 *in, const tsvpp_rect *rects, int aligned_outputs,
                                  char *buf, size_t buf_len) {
    const P010Frames<TSVPP_MAX_LETTERBOX_P010> fr(n, in);
    return tile_describe(LbP010Path{ spec != nullptr, p, spec, n, fr.data, rects, 0, 0, 0, false }, aligned_outputs, buf, buf_len); // (the pad is no part of what is launched)
}

} // extern "C"
