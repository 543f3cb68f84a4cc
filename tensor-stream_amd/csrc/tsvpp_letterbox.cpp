// tsvpp_letterbox.cpp -- aspect-preserving resize into a padded canvas (include/tsvpp.h): tsvpp_letterbox_rect, tsvpp_convert_letterbox, tsvpp_describe_letterbox and
// their tensor forms (tsvpp_convert_letterbox_tensor / tsvpp_describe_letterbox_tensor: `spec`, null for the first pair; kernel vpp_letterbox_tensor.hip);
// TSVPP_MAX_LETTERBOX frames per launch, kernel vpp_letterbox.hip.  The request rules are letterbox_plan's (tsvpp_plan.cpp), the spec's tensor_spec_status's.
#include <algorithm>
#include <cstdio>

#include "tsvpp_host.h"
#include "vpp_letterbox.h"

using namespace tsvpp;

// 4 k + 2 columns, narrower than a tile: no tile column to shift, so no vector stores
static bool narrow_tail(const RoiPlan &pl) { return (pl.dst_w & 3) != 0 && pl.dst_w < ROI_TILE_W; }

// One launch group: frames [base, base + cnt) as an LbLaunch.  `in` may carry null planes (the describe call).  Returns how many of the group's frames stage EVERY
// tile in LDS; L.lds_bytes = the dynamic LDS the launch needs for them (0: the gather kernel).
static int letterbox_fill(const Knobs &kn, const RoiPlan &pl, const tsvpp_nv12 *in, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v, void *const *outs, int base,
                          int cnt, bool vec, const tsvpp_tensor_spec *spec, LbLaunch &L) {
    L.spec = spec ? *spec : tsvpp_tensor_spec{};
    L.dst_w = pl.dst_w;
    L.dst_h = pl.dst_h;
    L.swap_rb = pl.swap_rb;
    L.color_g = kn.color_g;
    L.k = kn.coeffs;
    L.tiles_x = (pl.dst_w + ROI_TILE_W - 1) / ROI_TILE_W;
    L.tiles_y = (pl.dst_h + ROI_TILE_H - 1) / ROI_TILE_H;
    L.n_frames = cnt;
    // store policy and the shifted last tile column: as rois_fill (tsvpp_rois.cpp)
    L.nt_stores = kn.nt_stores >= 0 ? kn.nt_stores : ((!vec && pl.out == O_F32_MERGED) ? 0 : 1);
    L.last_col0 = (vec && (pl.dst_w & 3) != 0 && pl.dst_w >= ROI_TILE_W) ? pl.dst_w - ROI_TILE_W : 0;
    L.u8_xchg = kn.u8_xchg;
    L.pad_y = (float)pad_y;
    L.pad_u = (float)pad_u;
    L.pad_v = (float)pad_v;
    for (int i = 0; i < cnt; i++) {
        const tsvpp_nv12 &fr = in[base + i];
        const tsvpp_rect rc = letterbox_rect_of(in, rects, base + i, pl.dst_w, pl.dst_h);
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
    }
    for (int i = cnt; i < TSVPP_MAX_LETTERBOX; i++) L.r[i] = LbRec{};
    const bool luma_only = pl.out == O_Y800_U8 || pl.out == O_Y800_F32;
    const int budget = kn.force_gather ? 0 : kn.lds_budget_kb * 1024 - roi_static_lds(pl.out, vec);
    int staged = 0, lds = 0;
    for (int i = 0; i < cnt; i++) {
        const LbRec &r = L.r[i];
        // the frame's largest tile footprint, from the numbers the kernel computes for the tiles that touch the rectangle (columns and rows are independent: the
        // maximum over tiles is the maximum of each)
        RoiFootprint f;
        int cy = 0, cuv = 0, ny = 0, nuv = 0, lo, hi;
        for (int tx = 0; tx < L.tiles_x; tx++) {
            const int j_first = roi_tile_col0(tx, pl.dst_w, L.last_col0);
            lb_inner_range(j_first, lb_tile_last(j_first, ROI_TILE_W, pl.dst_w), r.left, r.width, lo, hi);
            if (lo > hi) continue;
            lb_span_x(pl.mode, lo, hi, r.src_w, r.xr, f);
            cy = std::max(cy, roi_chunks(f.xhi - f.xlo + 1));
            cuv = std::max(cuv, roi_chunks(2 * (f.cxhi - f.cxlo + 1)));
        }
        for (int ty = 0; ty < L.tiles_y; ty++) {
            const int i_first = ty * ROI_TILE_H;
            lb_inner_range(i_first, lb_tile_last(i_first, ROI_TILE_H, pl.dst_h), r.top, r.height, lo, hi);
            if (lo > hi) continue;
            lb_span_y(pl.mode, lo, hi, r.src_h, r.yr, f);
            ny = std::max(ny, f.yhi - f.ylo + 1);
            nuv = std::max(nuv, luma_only ? 0 : f.cyhi - f.cylo + 1);
        }
        const bool ok = cy <= ROI_THREADS && cuv <= ROI_THREADS;
        const long need = 16L * ((long)ny * cy + (long)nuv * cuv);
        if (ok && need <= budget) {
            staged++;
            lds = std::max(lds, (int)need);
        }
    }
    L.lds_bytes = lds;
    return staged;
}

static hipError_t launch_group(const RoiPlan &pl, bool vec, bool staged, bool tensor, const LbLaunch &L, hipStream_t stream, char *name, size_t name_len,
                               bool dry_run) {
    const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_frames);
    if (tensor) return launch_letterbox_tensor(pl.mode, pl.out, vec, staged, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    return launch_letterbox(pl.mode, pl.out, vec, staged, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
}

// `tensor`: tsvpp_convert_letterbox_tensor (then `spec` is checked behind the plan, and may be null: that is its TSVPP_ERROR)
static int convert_letterbox(bool tensor, tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec, const tsvpp_rect *rects,
                             int pad_y, int pad_u, int pad_v, void *const *outs, void *stream) {
    clear_last_launch();
    RoiPlan pl;
    int sts = letterbox_plan(p, n, in, rects, pad_y, pad_u, pad_v, pl); // the request first: the same status the describe call answers, context or not
    if (sts == TSVPP_OK && tensor) sts = tensor_spec_status(p, spec);
    if (sts != TSVPP_OK) return sts;
    if (!ctx || !outs) return TSVPP_ERROR;
    for (int f = 0; f < n; f++)
        if (!in[f].y || !in[f].uv || !outs[f]) return TSVPP_ERROR;
    if (tensor && !outs_aligned_to(outs, n, tensor_elem_bytes(spec->dtype))) return TSVPP_ERROR;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    char label[96] = "";
    const bool markers = ctx->markers != 0;
    if (markers)
        std::snprintf(label, sizeof(label), "tsvpp_convert_letterbox%s n=%d ->%dx%d mode=%d fourcc=%d stream=%p", tensor ? "_tensor" : "", n, pl.dst_w, pl.dst_h, (int)pl.mode, p->fourcc, stream);
    RangeGuard range(markers, label);
    for (int base = 0; base < n; base += TSVPP_MAX_LETTERBOX) {
        const int cnt = std::min(n - base, (int)TSVPP_MAX_LETTERBOX);
        const bool vec = outs_aligned16(outs + base, cnt) && !narrow_tail(pl); // per launch group, as tsvpp_convert_batch
        LbLaunch L;
        const int staged = letterbox_fill(ctx->knobs, pl, in, rects, pad_y, pad_u, pad_v, outs, base, cnt, vec, tensor ? spec : nullptr, L);
        const hipError_t e = launch_group(pl, vec, staged > 0, tensor, L, (hipStream_t)stream, nullptr, 0, false);
        if (e != hipSuccess) return (int)e;
    }
    return TSVPP_OK;
}

static int describe_letterbox(bool tensor, const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects,
                              int aligned_outputs, char *buf, size_t buf_len) {
    if (!buf || buf_len == 0) return TSVPP_ERROR;
    buf[0] = 0;
    RoiPlan pl;
    int sts = letterbox_plan(p, n, in, rects, 0, 0, 0, pl); // (the pad is no part of what is launched)
    if (sts == TSVPP_OK && tensor) sts = tensor_spec_status(p, spec);
    if (sts != TSVPP_OK) return sts;
    Knobs kn; // no context: no device, no streams
    read_env_knobs(kn);
    std::vector<tsvpp_nv12> fr(in, in + n); // the geometry only: plane pointers are not read
    for (tsvpp_nv12 &f : fr) f.y = f.uv = nullptr;
    const bool vec = aligned_outputs != 0 && !narrow_tail(pl);
    int staged = 0, lds0 = 0, grid0 = 0, launches = 0;
    char kname[128] = "(none)";
    LbLaunch L;
    for (int base = 0; base < n; base += TSVPP_MAX_LETTERBOX, launches++) {
        const int cnt = std::min(n - base, (int)TSVPP_MAX_LETTERBOX);
        const int s = letterbox_fill(kn, pl, fr.data(), rects, 0, 0, 0, nullptr, base, cnt, vec, tensor ? spec : nullptr, L);
        staged += s;
        if (base == 0) {
            lds0 = L.lds_bytes;
            grid0 = L.tiles_x * L.tiles_y * cnt;
            const hipError_t e = launch_group(pl, vec, s > 0, tensor, L, nullptr, kname, sizeof(kname), true);
            if (e != hipSuccess) return (int)e;
        }
    }
    const tsvpp_rect r0 = letterbox_rect_of(in, rects, 0, pl.dst_w, pl.dst_h);
    std::snprintf(buf, buf_len, "mode=%s out=%s dst=%dx%d frames=%d launches=%d kernel=%s shape=%dx%d lds=%d grid=%d tiles=%dx%d staged=%d tail=%d nt=%d limit=%d inner=%dx%d+%d+%d",
                  mode_names[pl.mode], tensor ? tensor_out_name(spec->dtype, pl.out == O_Y800_F32) : out_names[pl.out], pl.dst_w, pl.dst_h, n, launches, kname, ROI_TX, ROI_TY, lds0 + roi_static_lds(pl.out, vec), grid0, L.tiles_x,
                  L.tiles_y, staged, L.last_col0 > 0 ? 2 : 0, L.nt_stores, (int)TSVPP_MAX_LETTERBOX, r0.width, r0.height, r0.left, r0.top);
    return TSVPP_OK;
}

extern "C" {

int tsvpp_letterbox_rect(int in_w, int in_h, int dst_w, int dst_h, tsvpp_rect *out) {
    if (!out || in_w <= 0 || in_h <= 0 || dst_w <= 0 || dst_h <= 0) return TSVPP_ERROR;
    if ((dst_w | dst_h) & 1) return TSVPP_UNSUPPORTED;
    const int64_t iw = in_w, ih = in_h, dw = dst_w, dh = dst_h;
    int64_t w, h;
    if (iw * dh >= ih * dw) {
        w = dw;
        h = std::min(std::max<int64_t>(2 * ((ih * dw + iw) / (2 * iw)), 2), dh);
    } else {
        h = dh;
        w = std::min(std::max<int64_t>(2 * ((iw * dh + ih) / (2 * ih)), 2), dw);
    }
    out->width = (int32_t)w;
    out->height = (int32_t)h;
    out->left = (int32_t)(((dw - w) / 2) & ~(int64_t)1);
    out->top = (int32_t)(((dh - h) / 2) & ~(int64_t)1);
    return TSVPP_OK;
}

int tsvpp_convert_letterbox(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_rect *rects, int pad_y, int pad_u, int pad_v,
                            void *const *outs, void *stream) {
    return convert_letterbox(false, ctx, n, in, p, nullptr, rects, pad_y, pad_u, pad_v, outs, stream);
}

int tsvpp_describe_letterbox(const tsvpp_params *p, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects, int aligned_outputs, char *buf, size_t buf_len) {
    return describe_letterbox(false, p, nullptr, n, in, rects, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_letterbox_tensor(tsvpp_ctx *ctx, int n, const tsvpp_nv12 *in, const tsvpp_params *p, const tsvpp_tensor_spec *spec, const tsvpp_rect *rects,
                                   int pad_y, int pad_u, int pad_v, void *const *outs, void *stream) {
    return convert_letterbox(true, ctx, n, in, p, spec, rects, pad_y, pad_u, pad_v, outs, stream);
}

int tsvpp_describe_letterbox_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n, const tsvpp_nv12 *in, const tsvpp_rect *rects,
                                    int aligned_outputs, char *buf, size_t buf_len) {
    return describe_letterbox(true, p, spec, n, in, rects, aligned_outputs, buf, buf_len);
}

} // extern "C"
