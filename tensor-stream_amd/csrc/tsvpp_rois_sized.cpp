// tsvpp_rois_sized.cpp -- regions of interest, each to its own output size (include/tsvpp.h): tsvpp_convert_rois_sized / tsvpp_describe_rois_sized, their tensor
// forms, tsvpp_rois_sized_tile.  Kernels vpp_rois_sized.hip / vpp_rois_sized_tensor.hip, request rules rois_sized_plan's (tsvpp_plan.cpp).
//
// Not a path of tsvpp_tiles.h's skeletons: those cut a call into consecutive groups of one output size, one tiles_x x tiles_y and one store class per group.  Here
// the store class is a property of the BOX -- a 16-byte aligned output that is not a narrow tail takes vector stores -- and outputs of different sizes packed tightly
// are misaligned all the time, so the boxes of a call are first split into the vector-eligible ones and the rest (order kept inside each class) and each class goes
// out in chunks of TSVPP_MAX_ROIS_SIZED.  What IS shared: the staging budget of one box (tile_item_need, tsvpp_tiles.h), asked with the box's own output size; the
// store-policy rule; the checks around a conversion.  No allocation on the convert side: a chunk's box indices live in a stack array.
#include "tsvpp_tiles.h"
#include "vpp_rois_sized.h"

using namespace tsvpp;

namespace {

struct SizedReq {
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec; // null unless a tensor entry point was called -- where it may be null too: its TSVPP_ERROR
    int n_frames;
    const tsvpp_nv12 *frames;
    int n_rois;
    const tsvpp_roi_sized *rois;
};

// the request first (the same status the describe call answers, context or not): the plan's status, then -- tensor entry points -- the spec's
int sized_request(const SizedReq &rq, RoiPlan &pl) {
    const int sts = rois_sized_plan(rq.p, rq.n_frames, rq.frames, rq.n_rois, rq.rois, pl);
    return (sts == TSVPP_OK && rq.tensor) ? tensor_spec_status(rq.p, rq.spec) : sts;
}

// The store class of box i: `outs` null (describe, tile) takes every output as aligned or not, as the caller says
bool box_vec(const SizedReq &rq, void *const *outs, bool aligned, int i) {
    return (outs ? aligned16(outs[i]) : aligned) && !narrow_tail(rq.rois[i].dst_width);
}

// The launches of a request in the order they are issued: the vector class in chunks of TSVPP_MAX_ROIS_SIZED, then the element-wise class.  f(vec, idx, cnt)
// receives the chunk's box indices and returns false to stop.
template <class F> void for_each_launch(const SizedReq &rq, void *const *outs, bool aligned, F &&f) {
    int idx[TSVPP_MAX_ROIS_SIZED];
    for (int cls = 1; cls >= 0; cls--) {
        const bool vec = cls != 0;
        int cnt = 0;
        for (int i = 0; i < rq.n_rois; i++) {
            if (box_vec(rq, outs, aligned, i) != vec) continue;
            idx[cnt++] = i;
            if (cnt == TSVPP_MAX_ROIS_SIZED) {
                if (!f(vec, idx, cnt)) return;
                cnt = 0;
            }
        }
        if (cnt && !f(vec, idx, cnt)) return;
    }
}

// One launch: boxes idx[0 .. cnt) as a launch block (`outs` null: a dry run, the records hold the bare crop offsets and no output).  Returns how many of them stage
// EVERY tile in LDS; L.lds_bytes = the dynamic LDS the launch needs for them (0: the gather kernel).
int sized_fill(const SizedReq &rq, const Knobs &kn, const RoiPlan &pl, void *const *outs, const int *idx, int cnt, bool vec, SizedLaunch &L) {
    L.spec = rq.spec ? *rq.spec : tsvpp_tensor_spec{};
    L.swap_rb = pl.swap_rb;
    L.color_g = kn.color_g;
    L.k = kn.coeffs;
    L.n_rois = cnt;
    // store policy as tile_fill's (tsvpp_tiles.h): it depends on (vec, out) and the knobs only, so it stays per launch
    L.nt_stores = kn.nt_stores >= 0 ? kn.nt_stores : ((!vec && pl.out == O_F32_MERGED) ? 0 : 1);
    L.u8_xchg = kn.u8_xchg;
    const bool luma_only = out_luma_only(pl.out);
    const int budget = kn.force_gather ? 0 : kn.lds_budget_kb * 1024 - roi_static_lds(pl.out, vec);
    int staged = 0, lds = 0;
    uint32_t tiles = 0;
    for (int i = 0; i < cnt; i++) {
        const tsvpp_roi_sized &b = rq.rois[idx[i]];
        const tsvpp_nv12 &fr = rq.frames[b.frame];
        SizedRec &r = L.r[i];
        r.pitch_y = pitch_or_width(fr.pitch_y, fr.width);
        r.pitch_uv = pitch_or_width(fr.pitch_uv, fr.width);
        const CropOff off = plane_offsets(b.left, b.top, r.pitch_y, r.pitch_uv); // the box is the crop
        r.y = (outs ? (uint64_t)(uintptr_t)fr.y : 0) + off.y;
        r.uv = (outs ? (uint64_t)(uintptr_t)fr.uv : 0) + off.uv;
        r.out = outs ? (uint64_t)(uintptr_t)outs[idx[i]] : 0;
        r.src_w = b.right - b.left;
        r.src_h = b.bottom - b.top;
        r.dst_w = b.dst_width;
        r.dst_h = b.dst_height;
        r.xr = (float)r.src_w / (float)r.dst_w; // src/Resize.cu:418-419
        r.yr = (float)r.src_h / (float)r.dst_h;
        r.tiles_x = (r.dst_w + ROI_TILE_W - 1) / ROI_TILE_W;
        const int tiles_y = (r.dst_h + ROI_TILE_H - 1) / ROI_TILE_H;
        r.tile0 = (int32_t)tiles;
        tiles += (uint32_t)r.tiles_x * (uint32_t)tiles_y; // (below 2^31 for a full launch: rois_sized_plan)
        L.tile_end[i] = tiles;
        // the staging budget: a box stages if the largest footprint among ITS tiles fits what the workgroup's LDS budget leaves
        bool ok;
        const TileItem it{ (int)pl.mode, r.src_w, r.src_h, r.xr, r.yr, 0, 0, r.dst_w, r.dst_h };
        const long need = tile_item_need<false>(it, r.tiles_x, tiles_y, r.dst_w, r.dst_h, sized_last_col0(vec, r.dst_w), luma_only, ok);
        if (ok && need <= budget) {
            staged++;
            lds = std::max(lds, (int)need);
        }
    }
    for (int i = cnt; i < TSVPP_MAX_ROIS_SIZED; i++) {
        L.r[i] = {};
        L.tile_end[i] = 0xffffffffu; // above every workgroup index: sized_tile never counts it
    }
    L.lds_bytes = lds;
    return staged;
}

unsigned sized_grid(const SizedLaunch &L) { return L.tile_end[L.n_rois - 1]; }

hipError_t sized_launch(const SizedReq &rq, const RoiPlan &pl, bool vec, bool staged, const SizedLaunch &L, hipStream_t stream, char *name, size_t name_len,
                        bool dry_run) {
    return (rq.tensor ? launch_rois_sized_tensor : launch_rois_sized)(pl.mode, pl.out, vec, staged, L, sized_grid(L), (size_t)L.lds_bytes, stream, name, name_len,
                                                                       dry_run);
}

int sized_convert(const SizedReq &rq, tsvpp_ctx *ctx, void *const *outs, void *stream) {
    clear_last_launch();
    RoiPlan pl;
    const int sts = sized_request(rq, pl);
    if (sts != TSVPP_OK) return sts;
    if (!ctx || !outs) return TSVPP_ERROR;
    for (int f = 0; f < rq.n_frames; f++)
        if (!rq.frames[f].y || !rq.frames[f].uv) return TSVPP_ERROR;
    for (int i = 0; i < rq.n_rois; i++)
        if (!outs[i]) return TSVPP_ERROR;
    if (rq.tensor && !outs_aligned_to(outs, rq.n_rois, tensor_elem_bytes(rq.spec->dtype))) return TSVPP_ERROR;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    char label[96] = "";
    const bool markers = ctx->markers != 0;
    if (markers)
        std::snprintf(label, sizeof(label), "tsvpp_convert_rois_sized%s n=%d frames=%d mode=%d fourcc=%d stream=%p", rq.tensor ? "_tensor" : "", rq.n_rois, rq.n_frames,
                      (int)pl.mode, rq.p->fourcc, stream);
    RangeGuard range(markers, label);
    int result = TSVPP_OK;
    for_each_launch(rq, outs, false, [&](bool vec, const int *idx, int cnt) {
        SizedLaunch L;
        const int staged = sized_fill(rq, ctx->knobs, pl, outs, idx, cnt, vec, L);
        const hipError_t e = sized_launch(rq, pl, vec, staged > 0, L, (hipStream_t)stream, nullptr, 0, false);
        if (e != hipSuccess) result = (int)e;
        return e == hipSuccess;
    });
    return result;
}

int sized_describe(const SizedReq &rq, int aligned_outputs, char *buf, size_t buf_len) {
    if (!buf || buf_len == 0) return TSVPP_ERROR;
    buf[0] = 0;
    RoiPlan pl;
    const int sts = sized_request(rq, pl);
    if (sts != TSVPP_OK) return sts;
    Knobs kn; // no context: no device, no streams
    read_env_knobs(kn);
    int staged = 0, lds0 = 0, launches = 0, n_vec = 0, nt0 = 0, result = TSVPP_OK;
    unsigned grid0 = 0;
    char kname[128] = "(none)";
    for_each_launch(rq, nullptr, aligned_outputs != 0, [&](bool vec, const int *idx, int cnt) {
        SizedLaunch L;
        const int s = sized_fill(rq, kn, pl, nullptr, idx, cnt, vec, L);
        staged += s;
        n_vec += vec ? cnt : 0;
        if (launches++ == 0) {
            lds0 = L.lds_bytes + roi_static_lds(pl.out, vec);
            grid0 = sized_grid(L);
            nt0 = L.nt_stores;
            const hipError_t e = sized_launch(rq, pl, vec, s > 0, L, nullptr, kname, sizeof(kname), true);
            if (e != hipSuccess) result = (int)e;
            return e == hipSuccess;
        }
        return true;
    });
    if (result != TSVPP_OK) return result;
    std::set<std::pair<int, int>> sizes;
    int max_w = 0, max_h = 0;
    for (int i = 0; i < rq.n_rois; i++) {
        sizes.insert({ rq.rois[i].dst_width, rq.rois[i].dst_height });
        max_w = std::max(max_w, rq.rois[i].dst_width);
        max_h = std::max(max_h, rq.rois[i].dst_height);
    }
    std::snprintf(buf, buf_len, "mode=%s out=%s dst=var rois=%d frames=%d launches=%d kernel=%s shape=%dx%d lds=%d grid=%u sizes=%d maxdst=%dx%d staged=%d vec=%d nt=%d limit=%d",
                  mode_names[pl.mode], rq.tensor ? tensor_out_name(rq.spec->dtype, pl.out == O_Y800_F32) : out_names[pl.out], rq.n_rois, rq.n_frames, launches, kname,
                  ROI_TX, ROI_TY, lds0, grid0, (int)sizes.size(), max_w, max_h, staged, n_vec, nt0, (int)TSVPP_MAX_ROIS_SIZED);
    return TSVPP_OK;
}

} // namespace

extern "C" {

int tsvpp_convert_rois_sized(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, const tsvpp_params *p,
                             void *const *outs, void *stream) {
    return sized_convert(SizedReq{ false, p, nullptr, n_frames, frames, n_rois, rois }, ctx, outs, stream);
}

int tsvpp_describe_rois_sized(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, int aligned_outputs,
                              char *buf, size_t buf_len) {
    return sized_describe(SizedReq{ false, p, nullptr, n_frames, frames, n_rois, rois }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_rois_sized_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, const tsvpp_params *p,
                                    const tsvpp_tensor_spec *spec, void *const *outs, void *stream) {
    return sized_convert(SizedReq{ true, p, spec, n_frames, frames, n_rois, rois }, ctx, outs, stream);
}

int tsvpp_describe_rois_sized_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_rois,
                                     const tsvpp_roi_sized *rois, int aligned_outputs, char *buf, size_t buf_len) {
    return sized_describe(SizedReq{ true, p, spec, n_frames, frames, n_rois, rois }, aligned_outputs, buf, buf_len);
}

// The first launch's block, filled as the convert call fills it, and the kernel's own lookup on it
int tsvpp_rois_sized_tile(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi_sized *rois, int aligned_outputs, unsigned wg,
                          int32_t *out5) {
    const SizedReq rq{ false, p, nullptr, n_frames, frames, n_rois, rois };
    RoiPlan pl;
    const int sts = sized_request(rq, pl);
    if (sts != TSVPP_OK) return sts;
    if (!out5) return TSVPP_ERROR;
    Knobs kn;
    read_env_knobs(kn);
    int result = TSVPP_ERROR;
    for_each_launch(rq, nullptr, aligned_outputs != 0, [&](bool vec, const int *idx, int cnt) {
        SizedLaunch L;
        (void)sized_fill(rq, kn, pl, nullptr, idx, cnt, vec, L);
        if (wg < sized_grid(L)) {
            const SizedTile t = sized_tile(L, wg);
            const SizedRec &r = L.r[t.box];
            out5[0] = idx[t.box];
            out5[1] = t.txi;
            out5[2] = t.tyi;
            out5[3] = roi_tile_col0(t.txi, r.dst_w, sized_last_col0(vec, r.dst_w));
            out5[4] = t.tyi * ROI_TILE_H;
            result = TSVPP_OK;
        }
        return false; // the first launch only
    });
    return result;
}

} // extern "C"
