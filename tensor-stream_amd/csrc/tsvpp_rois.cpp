// tsvpp_rois.cpp -- regions of interest (include/tsvpp.h): many boxes of a few frames to one size, TSVPP_MAX_ROIS per launch.  Three pairs of entry points over one
// body: tsvpp_convert_rois / tsvpp_describe_rois (NEAREST, BILINEAR, BICUBIC; kernel vpp_rois.hip), tsvpp_convert_rois_area / tsvpp_describe_rois_area (AREA;
// kernel vpp_rois_area.hip) and tsvpp_convert_rois_tensor / tsvpp_describe_rois_tensor (all four; the tensor instantiations of both kernels, vpp_rois_tensor.hip /
// vpp_rois_area_tensor.hip).  What differs is which resize types rois_plan lets through (`area`), the mode of a box (AREA: per box), and -- `spec`, null for the
// first two pairs -- the launcher, the element size and the spec check behind the plan.
#include <algorithm>
#include <cstdio>

#include "tsvpp_host.h"
#include "vpp_rois.h"

using namespace tsvpp;

// 4 k + 2 columns, narrower than a tile: no tile column to shift, so no vector stores
static bool narrow_tail(const RoiPlan &pl) { return (pl.dst_w & 3) != 0 && pl.dst_w < ROI_TILE_W; }
static bool is_area(const RoiPlan &pl) { return pl.mode == M_AREA_DOWN; }
static int launch_limit(const RoiPlan &pl) { return is_area(pl) ? (int)TSVPP_MAX_ROIS_AREA : (int)TSVPP_MAX_ROIS; }

// One launch group: boxes [base, base + cnt) as a RoiLaunch.  `frames` may carry null planes (the describe calls): then the records hold the bare crop offsets.
// Returns how many of the group's boxes stage EVERY tile in LDS; L.lds_bytes = the dynamic LDS the launch needs for them (0: the gather kernel), L.area_lds = the
// bytes of the AREA kernel's weight rows in front of it (the largest tap counts among the group's down-scale boxes; they count against the LDS budget).
static int rois_fill(const Knobs &kn, const RoiPlan &pl, const tsvpp_nv12 *frames, const tsvpp_roi *rois, void *const *outs, int base, int cnt, bool vec,
                     const tsvpp_tensor_spec *spec, RoiLaunch &L) {
    L.spec = spec ? *spec : tsvpp_tensor_spec{};
    L.dst_w = pl.dst_w;
    L.dst_h = pl.dst_h;
    L.swap_rb = pl.swap_rb;
    L.color_g = kn.color_g;
    L.k = kn.coeffs;
    L.tiles_x = (pl.dst_w + ROI_TILE_W - 1) / ROI_TILE_W;
    L.tiles_y = (pl.dst_h + ROI_TILE_H - 1) / ROI_TILE_H;
    L.n_rois = cnt;
    // store policy as launch_fused's for a resize kernel: non-temporal, except the element-wise merged fp32 stores (partial lines: L2 combines them).  The tensor
    // stores take the fp32 planar choice (profiles/tensor_ab.txt)
    L.nt_stores = kn.nt_stores >= 0 ? kn.nt_stores : ((!vec && pl.out == O_F32_MERGED) ? 0 : 1);
    // outputs 4 k + 2 columns wide: the last tile column is shifted to the right edge so that every thread tile has its four columns (tile_col0, vpp_device.h)
    L.last_col0 = (vec && (pl.dst_w & 3) != 0 && pl.dst_w >= ROI_TILE_W) ? pl.dst_w - ROI_TILE_W : 0;
    L.u8_xchg = kn.u8_xchg;
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
        if (is_area(pl) && roi_area_mode(r.xr, r.yr) == M_AREA_DOWN) L.area_lds = std::max(L.area_lds, roi_area_lds(roi_area_taps(r.xr), roi_area_taps(r.yr)));
    }
    for (int i = cnt; i < TSVPP_MAX_ROIS; i++) L.r[i] = RoiRec{};
    const bool luma_only = pl.out == O_Y800_U8 || pl.out == O_Y800_F32;
    const int budget = kn.force_gather ? 0 : kn.lds_budget_kb * 1024 - roi_static_lds(pl.out, vec) - L.area_lds;
    int staged = 0, lds = 0;
    for (int i = 0; i < cnt; i++) {
        const RoiRec &r = L.r[i];
        const int mode = is_area(pl) ? roi_area_mode(r.xr, r.yr) : (int)pl.mode;
        // the box's largest tile footprint, from the numbers the kernel computes (columns and rows are independent: the maximum over tiles is the maximum of each)
        RoiFootprint f;
        int cy = 0, cuv = 0, ny = 0, nuv = 0;
        for (int tx = 0; tx < L.tiles_x; tx++) {
            roi_span_x(mode, roi_tile_col0(tx, pl.dst_w, L.last_col0), pl.dst_w, r.src_w, r.xr, f);
            cy = std::max(cy, roi_chunks(f.xhi - f.xlo + 1));
            cuv = std::max(cuv, roi_chunks(2 * (f.cxhi - f.cxlo + 1)));
        }
        for (int ty = 0; ty < L.tiles_y; ty++) {
            roi_span_y(mode, ty * ROI_TILE_H, pl.dst_h, r.src_h, r.yr, f);
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

// (vpp_rois.hip / vpp_rois_area.hip) one launch group, or only its kernel's name
static hipError_t launch_group(const RoiPlan &pl, bool vec, bool staged, bool tensor, const RoiLaunch &L, hipStream_t stream, char *name, size_t name_len,
                               bool dry_run) {
    const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n_rois);
    if (tensor) {
        if (is_area(pl)) return launch_rois_area_tensor(pl.out, vec, staged, L, grid, (size_t)(L.area_lds + L.lds_bytes), stream, name, name_len, dry_run);
        return launch_rois_tensor(pl.mode, pl.out, vec, staged, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
    if (is_area(pl)) return launch_rois_area(pl.out, vec, staged, L, grid, (size_t)(L.area_lds + L.lds_bytes), stream, name, name_len, dry_run);
    return launch_rois(pl.mode, pl.out, vec, staged, L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
}

// `tensor`: tsvpp_convert_rois_tensor (then `spec` is checked behind the plan, and may be null: that is its TSVPP_ERROR)
static int convert_rois(bool area, bool tensor, tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p,
                        const tsvpp_tensor_spec *spec, void *const *outs, void *stream) {
    clear_last_launch();
    RoiPlan pl;
    int sts = rois_plan(p, n_frames, frames, n_rois, rois, pl, area); // the request first: the same status the describe call answers, context or not
    if (sts == TSVPP_OK && tensor) sts = tensor_spec_status(p, spec);
    if (sts != TSVPP_OK) return sts;
    if (!ctx || !outs) return TSVPP_ERROR;
    for (int f = 0; f < n_frames; f++)
        if (!frames[f].y || !frames[f].uv) return TSVPP_ERROR;
    for (int i = 0; i < n_rois; i++)
        if (!outs[i]) return TSVPP_ERROR;
    if (tensor && !outs_aligned_to(outs, n_rois, tensor_elem_bytes(spec->dtype))) return TSVPP_ERROR;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    char label[96] = "";
    const bool markers = ctx->markers != 0;
    if (markers)
        std::snprintf(label, sizeof(label), "tsvpp_convert_rois%s n=%d frames=%d ->%dx%d mode=%d fourcc=%d stream=%p", tensor ? "_tensor" : (area ? "_area" : ""), n_rois, n_frames, pl.dst_w,
                      pl.dst_h, (int)pl.mode, p->fourcc, stream);
    RangeGuard range(markers, label);
    const int limit = launch_limit(pl);
    for (int base = 0; base < n_rois; base += limit) {
        const int cnt = std::min(n_rois - base, limit);
        const bool vec = outs_aligned16(outs + base, cnt) && !narrow_tail(pl); // per launch group, as tsvpp_convert_batch
        RoiLaunch L;
        const int staged = rois_fill(ctx->knobs, pl, frames, rois, outs, base, cnt, vec, tensor ? spec : nullptr, L);
        const hipError_t e = launch_group(pl, vec, staged > 0, tensor, L, (hipStream_t)stream, nullptr, 0, false);
        if (e != hipSuccess) return (int)e;
    }
    return TSVPP_OK;
}

static int describe_rois(bool area, bool tensor, const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_rois,
                         const tsvpp_roi *rois, int aligned_outputs, char *buf, size_t buf_len) {
    if (!buf || buf_len == 0) return TSVPP_ERROR;
    buf[0] = 0;
    RoiPlan pl;
    int sts = rois_plan(p, n_frames, frames, n_rois, rois, pl, area);
    if (sts == TSVPP_OK && tensor) sts = tensor_spec_status(p, spec);
    if (sts != TSVPP_OK) return sts;
    Knobs kn; // no context: no device, no streams
    read_env_knobs(kn);
    std::vector<tsvpp_nv12> fr(frames, frames + n_frames); // the geometry only: plane pointers are not read (taken as 256-byte aligned)
    for (tsvpp_nv12 &f : fr) f.y = f.uv = nullptr;
    const bool vec = aligned_outputs != 0 && !narrow_tail(pl);
    int staged = 0, lds0 = 0, grid0 = 0, launches = 0;
    char kname[128] = "(none)";
    RoiLaunch L;
    const int limit = launch_limit(pl);
    for (int base = 0; base < n_rois; base += limit, launches++) {
        const int cnt = std::min(n_rois - base, limit);
        const int s = rois_fill(kn, pl, fr.data(), rois, nullptr, base, cnt, vec, tensor ? spec : nullptr, L);
        staged += s;
        if (base == 0) {
            lds0 = L.area_lds + L.lds_bytes;
            grid0 = L.tiles_x * L.tiles_y * cnt;
            const hipError_t e = launch_group(pl, vec, s > 0, tensor, L, nullptr, kname, sizeof(kname), true);
            if (e != hipSuccess) return (int)e;
        }
    }
    const int n = std::snprintf(buf, buf_len, "mode=%s out=%s dst=%dx%d rois=%d frames=%d launches=%d kernel=%s shape=%dx%d lds=%d grid=%d tiles=%dx%d staged=%d tail=%d nt=%d limit=%d",
                                area ? "area" : mode_names[pl.mode], tensor ? tensor_out_name(spec->dtype, pl.out == O_Y800_F32) : out_names[pl.out], pl.dst_w, pl.dst_h, n_rois, n_frames, launches, kname, ROI_TX, ROI_TY,
                                lds0 + roi_static_lds(pl.out, vec), grid0, L.tiles_x, L.tiles_y, staged, L.last_col0 > 0 ? 2 : 0, L.nt_stores, limit);
    if (area && n > 0 && (size_t)n < buf_len) std::snprintf(buf + n, buf_len - (size_t)n, " down=%d taps=%dx%d", pl.down, pl.taps_x, pl.taps_y);
    return TSVPP_OK;
}

extern "C" {

int tsvpp_convert_rois(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p, void *const *outs,
                       void *stream) {
    return convert_rois(false, false, ctx, n_frames, frames, n_rois, rois, p, nullptr, outs, stream);
}

int tsvpp_describe_rois(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, int aligned_outputs, char *buf,
                        size_t buf_len) {
    return describe_rois(false, false, p, nullptr, n_frames, frames, n_rois, rois, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_rois_area(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p, void *const *outs,
                            void *stream) {
    return convert_rois(true, false, ctx, n_frames, frames, n_rois, rois, p, nullptr, outs, stream);
}

int tsvpp_describe_rois_area(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, int aligned_outputs, char *buf,
                             size_t buf_len) {
    return describe_rois(true, false, p, nullptr, n_frames, frames, n_rois, rois, aligned_outputs, buf, buf_len);
}

// All four resize types behind one name: AREA takes the AREA plan, kernel and launch limit, anything else tsvpp_convert_rois's.
int tsvpp_convert_rois_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p,
                              const tsvpp_tensor_spec *spec, void *const *outs, void *stream) {
    return convert_rois(p && p->resize_type == TSVPP_AREA, true, ctx, n_frames, frames, n_rois, rois, p, spec, outs, stream);
}

int tsvpp_describe_rois_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois,
                               int aligned_outputs, char *buf, size_t buf_len) {
    return describe_rois(p && p->resize_type == TSVPP_AREA, true, p, spec, n_frames, frames, n_rois, rois, aligned_outputs, buf, buf_len);
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
