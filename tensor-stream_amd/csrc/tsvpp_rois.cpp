// tsvpp_rois.cpp -- regions of interest (include/tsvpp.h; kernel: vpp_rois.hip): many boxes of a few frames to one size, TSVPP_MAX_ROIS per launch.
#include <algorithm>
#include <cstdio>

#include "tsvpp_host.h"
#include "vpp_rois.h"

using namespace tsvpp;

// 4 k + 2 columns, narrower than a tile: no tile column to shift, so no vector stores
static bool narrow_tail(const RoiPlan &pl) { return (pl.dst_w & 3) != 0 && pl.dst_w < ROI_TILE_W; }

// One launch group: boxes [base, base + cnt) as a RoiLaunch.  `frames` may carry null planes (tsvpp_describe_rois): then the records hold the bare crop offsets.
// Returns how many of the group's boxes stage EVERY tile in LDS; L.lds_bytes = the dynamic LDS the launch needs for them (0: the gather kernel).
static int rois_fill(const Knobs &kn, const RoiPlan &pl, const tsvpp_nv12 *frames, const tsvpp_roi *rois, void *const *outs, int base, int cnt, bool vec, RoiLaunch &L) {
    L.dst_w = pl.dst_w;
    L.dst_h = pl.dst_h;
    L.swap_rb = pl.swap_rb;
    L.color_g = kn.color_g;
    L.k = kn.coeffs;
    L.tiles_x = (pl.dst_w + ROI_TILE_W - 1) / ROI_TILE_W;
    L.tiles_y = (pl.dst_h + ROI_TILE_H - 1) / ROI_TILE_H;
    L.n_rois = cnt;
    // store policy as launch_fused's for a resize kernel: non-temporal, except the element-wise merged fp32 stores (partial lines: L2 combines them)
    L.nt_stores = kn.nt_stores >= 0 ? kn.nt_stores : ((!vec && pl.out == O_F32_MERGED) ? 0 : 1);
    // outputs 4 k + 2 columns wide: the last tile column is shifted to the right edge so that every thread tile has its four columns (tile_col0, vpp_device.h)
    L.last_col0 = (vec && (pl.dst_w & 3) != 0 && pl.dst_w >= ROI_TILE_W) ? pl.dst_w - ROI_TILE_W : 0;
    L.u8_xchg = kn.u8_xchg;
    L.pad = 0;
    const bool luma_only = pl.out == O_Y800_U8 || pl.out == O_Y800_F32;
    const int budget = kn.force_gather ? 0 : kn.lds_budget_kb * 1024 - roi_static_lds(pl.out, vec);
    int staged = 0, lds = 0;
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
        // the box's largest tile footprint, from the numbers the kernel computes (columns and rows are independent: the maximum over tiles is the maximum of each)
        RoiFootprint f;
        int cy = 0, cuv = 0, ny = 0, nuv = 0;
        for (int tx = 0; tx < L.tiles_x; tx++) {
            roi_span_x(pl.mode, roi_tile_col0(tx, pl.dst_w, L.last_col0), pl.dst_w, r.src_w, r.xr, f);
            cy = std::max(cy, roi_chunks(f.xhi - f.xlo + 1));
            cuv = std::max(cuv, roi_chunks(2 * (f.cxhi - f.cxlo + 1)));
        }
        for (int ty = 0; ty < L.tiles_y; ty++) {
            roi_span_y(pl.mode, ty * ROI_TILE_H, pl.dst_h, r.src_h, r.yr, f);
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
    for (int i = cnt; i < TSVPP_MAX_ROIS; i++) L.r[i] = RoiRec{};
    L.lds_bytes = lds;
    return staged;
}

extern "C" {

int tsvpp_convert_rois(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, const tsvpp_params *p, void *const *outs,
                       void *stream) {
    clear_last_launch();
    RoiPlan pl;
    int sts = rois_plan(p, n_frames, frames, n_rois, rois, pl); // the request first: the same status tsvpp_describe_rois answers, context or not
    if (sts != TSVPP_OK) return sts;
    if (!ctx || !outs) return TSVPP_ERROR;
    for (int f = 0; f < n_frames; f++)
        if (!frames[f].y || !frames[f].uv) return TSVPP_ERROR;
    for (int i = 0; i < n_rois; i++)
        if (!outs[i]) return TSVPP_ERROR;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    char label[96] = "";
    const bool markers = ctx->markers != 0;
    if (markers)
        std::snprintf(label, sizeof(label), "tsvpp_convert_rois n=%d frames=%d ->%dx%d mode=%d fourcc=%d stream=%p", n_rois, n_frames, pl.dst_w, pl.dst_h, (int)pl.mode,
                      p->fourcc, stream);
    RangeGuard range(markers, label);
    for (int base = 0; base < n_rois; base += TSVPP_MAX_ROIS) {
        const int cnt = std::min(n_rois - base, (int)TSVPP_MAX_ROIS);
        const bool vec = outs_aligned16(outs + base, cnt) && !narrow_tail(pl); // per launch group, as tsvpp_convert_batch
        RoiLaunch L;
        const int staged = rois_fill(ctx->knobs, pl, frames, rois, outs, base, cnt, vec, L);
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * cnt);
        const hipError_t e = launch_rois(pl.mode, pl.out, vec, staged > 0, L, grid, (size_t)L.lds_bytes, (hipStream_t)stream, nullptr, 0, false);
        if (e != hipSuccess) return (int)e;
    }
    return TSVPP_OK;
}

int tsvpp_describe_rois(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_rois, const tsvpp_roi *rois, int aligned_outputs, char *buf,
                        size_t buf_len) {
    if (!buf || buf_len == 0) return TSVPP_ERROR;
    buf[0] = 0;
    RoiPlan pl;
    const int sts = rois_plan(p, n_frames, frames, n_rois, rois, pl);
    if (sts != TSVPP_OK) return sts;
    Knobs kn; // no context: no device, no streams
    read_env_knobs(kn);
    std::vector<tsvpp_nv12> fr(frames, frames + n_frames); // the geometry only: plane pointers are not read (taken as 256-byte aligned)
    for (tsvpp_nv12 &f : fr) f.y = f.uv = nullptr;
    const bool vec = aligned_outputs != 0 && !narrow_tail(pl);
    int staged = 0, lds0 = 0, grid0 = 0, launches = 0;
    char kname[128] = "(none)";
    RoiLaunch L;
    for (int base = 0; base < n_rois; base += TSVPP_MAX_ROIS, launches++) {
        const int cnt = std::min(n_rois - base, (int)TSVPP_MAX_ROIS);
        const int s = rois_fill(kn, pl, fr.data(), rois, nullptr, base, cnt, vec, L);
        staged += s;
        if (base == 0) {
            lds0 = L.lds_bytes;
            grid0 = L.tiles_x * L.tiles_y * cnt;
            const hipError_t e = launch_rois(pl.mode, pl.out, vec, s > 0, L, (unsigned)grid0, (size_t)lds0, nullptr, kname, sizeof(kname), true);
            if (e != hipSuccess) return (int)e;
        }
    }
    std::snprintf(buf, buf_len, "mode=%s out=%s dst=%dx%d rois=%d frames=%d launches=%d kernel=%s shape=%dx%d lds=%d grid=%d tiles=%dx%d staged=%d tail=%d nt=%d limit=%d",
                  mode_names[pl.mode], out_names[pl.out], pl.dst_w, pl.dst_h, n_rois, n_frames, launches, kname, ROI_TX, ROI_TY, lds0 + roi_static_lds(pl.out, vec), grid0,
                  L.tiles_x, L.tiles_y, staged, L.last_col0 > 0 ? 2 : 0, L.nt_stores, (int)TSVPP_MAX_ROIS);
    return TSVPP_OK;
}

} // extern "C"
