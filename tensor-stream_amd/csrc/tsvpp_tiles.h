// tsvpp_tiles.h -- the host side of the tile paths, once (tsvpp_rois.cpp: boxes, NEAREST / BILINEAR / BICUBIC and AREA; tsvpp_letterbox.cpp: frames into a padded
// canvas; both with their tensor forms).  All of them launch one 32 x 32 output tile per workgroup (vpp_tile_core.h) for up to a fixed number of items -- boxes,
// frames -- per launch.  Here: the launch fields they share, the staging budget, and the skeletons of the convert and the describe call.  A path is a small struct
// that holds its request and answers what differs:
//     using Launch                          RoiLaunch / LbLaunch / WarpLaunch
//     kOwnBudget                            false: a tile's footprint is a column span times a row span (item(), below); true: the path sizes the staged
//                                           footprints itself -- stage_budget(pl, L, budget, luma_only) sets L.lds_bytes and returns the items that stage every tile
//     p, spec, tensor, n_frames, frames     the request (spec: null unless the tensor entry point was called -- where it may be null too: its TSVPP_ERROR)
//     plan(pl), items(), limit(pl)          the request's status and RoiPlan; how many items it has; how many go into one launch
//     fill_items(pl, outs, base, cnt, L)    the count, the records and the path's own fields of one launch group (outs: null in a dry run)
//     item(pl, L, i)                        record i as a TileItem (paths without kOwnBudget)
//     front_lds(L)                          dynamic LDS in front of the staged footprint (the AREA kernel's weight rows)
//     launch(pl, vec, staged, L, ...)       the launcher
//     label(...), counts(...), suffix(...)  the marker label; "rois=8 frames=1" and what follows the common keys in the describe line (with its blank)
//     mode_name(pl)                         the describe line's mode=
#pragma once
#include <algorithm>
#include <cstdio>

#include "tsvpp_host.h"
#include "vpp_rois.h"

namespace tsvpp {

// 4 k + 2 columns, narrower than a tile: no tile column to shift, so no vector stores
inline bool narrow_tail(int dst_w) { return (dst_w & 3) != 0 && dst_w < ROI_TILE_W; }
inline bool narrow_tail(const RoiPlan &pl) { return narrow_tail(pl.dst_w); }

// What the staging budget needs to know of one item: its sampler, source size and ratios, and -- a path with kInnerRect -- the rectangle of the output its
// samples fill, the inner rectangle of a letterbox frame.  A box fills the whole output: the ROI paths say kInnerRect = false and their loop does not ask (with
// the rectangle asked per tile, 64 boxes to 224 x 224 took 0.3 us longer per call on the host: profiles/tile_core_ab.txt).
struct TileItem {
    int mode, src_w, src_h;
    float xr, yr;
    int left, top, width, height;
};

template <class PATH> int tile_separable_budget(const PATH &path, const RoiPlan &pl, typename PATH::Launch &L, int cnt, int budget, bool luma_only);

// One launch group: items [base, base + cnt) as a launch block.  Returns how many of the group's items stage EVERY tile in LDS; L.lds_bytes = the dynamic LDS
// the launch needs for them (0: the gather kernel).
template <class PATH> int tile_fill(const PATH &path, const Knobs &kn, const RoiPlan &pl, void *const *outs, int base, int cnt, bool vec, typename PATH::Launch &L) {
    L.spec = path.spec ? *path.spec : tsvpp_tensor_spec{};
    L.dst_w = pl.dst_w;
    L.dst_h = pl.dst_h;
    L.swap_rb = pl.swap_rb;
    L.color_g = kn.color_g;
    L.k = kn.coeffs;
    L.tiles_x = (pl.dst_w + ROI_TILE_W - 1) / ROI_TILE_W;
    L.tiles_y = (pl.dst_h + ROI_TILE_H - 1) / ROI_TILE_H;
    // store policy as launch_fused's for a resize kernel: non-temporal, except the element-wise merged fp32 stores (partial lines: L2 combines them).  The tensor
    // stores take the fp32 planar choice (profiles/tensor_ab.txt)
    L.nt_stores = kn.nt_stores >= 0 ? kn.nt_stores : ((!vec && pl.out == O_F32_MERGED) ? 0 : 1);
    // outputs 4 k + 2 columns wide: the last tile column is shifted to the right edge so that every thread tile has its four columns (tile_col0, vpp_device.h)
    L.last_col0 = (vec && (pl.dst_w & 3) != 0 && pl.dst_w >= ROI_TILE_W) ? pl.dst_w - ROI_TILE_W : 0;
    L.u8_xchg = kn.u8_xchg;
    path.fill_items(pl, outs, base, cnt, L);
    for (int i = cnt; i < (int)(sizeof(L.r) / sizeof(L.r[0])); i++) L.r[i] = {};
    // the staging budget: an item stages if the largest footprint among its tiles fits what the workgroup's LDS budget leaves
    const bool luma_only = out_luma_only(pl.out);
    const int budget = kn.force_gather ? 0 : kn.lds_budget_kb * 1024 - roi_static_lds(pl.out, vec) - path.front_lds(L);
    if constexpr (PATH::kOwnBudget) return path.stage_budget(pl, L, budget, luma_only);
    else return tile_separable_budget(path, pl, L, cnt, budget, luma_only);
}

// ... of a path whose tiles tap a column span times a row span of the source: an item stages if the largest footprint among its tiles fits the budget
// The largest staged footprint among the tiles of ONE item whose output is dst_w x dst_h in tiles_x x tiles_y tiles: its LDS bytes, from the numbers the kernel
// computes for the tiles that touch the item's rectangle (columns and rows are independent: the maximum over tiles is the maximum of each); `ok`: the staging
// loop can serve every such tile (roi_stageable).  The tile paths ask with their launch's output, tsvpp_rois_sized.cpp with each box's own.
template <bool INNER_RECT>
inline long tile_item_need(const TileItem &it, int tiles_x, int tiles_y, int dst_w, int dst_h, int last_col0, bool luma_only, bool &ok) {
    RoiFootprint f;
    int cy = 0, cuv = 0, ny = 0, nuv = 0, lo, hi;
    for (int tx = 0; tx < tiles_x; tx++) {
        lo = roi_tile_col0(tx, dst_w, last_col0);
        hi = tile_last(lo, ROI_TILE_W, dst_w);
        if constexpr (INNER_RECT) {
            tile_inner_range(lo, hi, it.left, it.width, lo, hi);
            if (lo > hi) continue;
        }
        tile_span_x(it.mode, lo, hi, it.src_w, it.xr, f);
        cy = std::max(cy, roi_chunks(f.xhi - f.xlo + 1));
        cuv = std::max(cuv, roi_chunks(2 * (f.cxhi - f.cxlo + 1)));
    }
    for (int ty = 0; ty < tiles_y; ty++) {
        lo = ty * ROI_TILE_H;
        hi = tile_last(lo, ROI_TILE_H, dst_h);
        if constexpr (INNER_RECT) {
            tile_inner_range(lo, hi, it.top, it.height, lo, hi);
            if (lo > hi) continue;
        }
        tile_span_y(it.mode, lo, hi, it.src_h, it.yr, f);
        ny = std::max(ny, f.yhi - f.ylo + 1);
        nuv = std::max(nuv, luma_only ? 0 : f.cyhi - f.cylo + 1);
    }
    ok = cy <= ROI_THREADS && cuv <= ROI_THREADS;
    return 16L * ((long)ny * cy + (long)nuv * cuv);
}

template <class PATH> int tile_separable_budget(const PATH &path, const RoiPlan &pl, typename PATH::Launch &L, int cnt, int budget, bool luma_only) {
    int staged = 0, lds = 0;
    for (int i = 0; i < cnt; i++) {
        bool ok;
        const long need = tile_item_need<PATH::kInnerRect>(path.item(pl, L, i), L.tiles_x, L.tiles_y, pl.dst_w, pl.dst_h, L.last_col0, luma_only, ok);
        if (ok && need <= budget) {
            staged++;
            lds = std::max(lds, (int)need);
        }
    }
    L.lds_bytes = lds;
    return staged;
}

// the request first (the same status the describe call answers, context or not): the plan's status, then -- tensor entry points -- the spec's
template <class PATH> int tile_request(const PATH &path, RoiPlan &pl) {
    const int sts = path.plan(pl);
    return (sts == TSVPP_OK && path.tensor) ? tensor_spec_status(path.p, path.spec) : sts;
}

template <class PATH> int tile_convert(const PATH &path, tsvpp_ctx *ctx, void *const *outs, void *stream) {
    clear_last_launch();
    RoiPlan pl;
    const int sts = tile_request(path, pl);
    if (sts != TSVPP_OK) return sts;
    if (!ctx || !outs) return TSVPP_ERROR;
    for (int f = 0; f < path.n_frames; f++)
        if (!path.frames[f].y || !path.frames[f].uv) return TSVPP_ERROR;
    const int n = path.items();
    for (int i = 0; i < n; i++)
        if (!outs[i]) return TSVPP_ERROR;
    if (path.tensor && !outs_aligned_to(outs, n, tensor_elem_bytes(path.spec->dtype))) return TSVPP_ERROR;
    DeviceGuard guard(ctx);
    if (guard.status != TSVPP_OK) return guard.status;
    char label[96] = "";
    const bool markers = ctx->markers != 0;
    if (markers) path.label(label, sizeof(label), pl, stream);
    RangeGuard range(markers, label);
    const int limit = path.limit(pl);
    for (int base = 0; base < n; base += limit) {
        const int cnt = std::min(n - base, limit);
        const bool vec = outs_aligned16(outs + base, cnt) && !narrow_tail(pl); // per launch group, as tsvpp_convert_batch
        typename PATH::Launch L;
        const int staged = tile_fill(path, ctx->knobs, pl, outs, base, cnt, vec, L);
        const hipError_t e = path.launch(pl, vec, staged > 0, L, (hipStream_t)stream, nullptr, 0, false);
        if (e != hipSuccess) return (int)e;
    }
    return TSVPP_OK;
}

// (`path` by value: its frames are replaced by a copy without planes)
template <class PATH> int tile_describe(PATH path, int aligned_outputs, char *buf, size_t buf_len) {
    if (!buf || buf_len == 0) return TSVPP_ERROR;
    buf[0] = 0;
    RoiPlan pl;
    const int sts = tile_request(path, pl);
    if (sts != TSVPP_OK) return sts;
    Knobs kn; // no context: no device, no streams
    read_env_knobs(kn);
    std::vector<tsvpp_nv12> fr(path.frames, path.frames + path.n_frames); // the geometry only: plane pointers are not read (taken as 256-byte aligned)
    for (tsvpp_nv12 &f : fr) f.y = f.uv = nullptr;
    path.frames = fr.data();
    const bool vec = aligned_outputs != 0 && !narrow_tail(pl);
    int staged = 0, lds0 = 0, grid0 = 0, launches = 0;
    char kname[128] = "(none)", counts[64] = "", suffix[96] = "";
    typename PATH::Launch L;
    const int n = path.items(), limit = path.limit(pl);
    for (int base = 0; base < n; base += limit, launches++) {
        const int cnt = std::min(n - base, limit);
        const int s = tile_fill(path, kn, pl, nullptr, base, cnt, vec, L);
        staged += s;
        if (base == 0) {
            lds0 = path.front_lds(L) + L.lds_bytes;
            grid0 = L.tiles_x * L.tiles_y * cnt;
            const hipError_t e = path.launch(pl, vec, s > 0, L, nullptr, kname, sizeof(kname), true);
            if (e != hipSuccess) return (int)e;
        }
    }
    path.counts(counts, sizeof(counts));
    path.suffix(suffix, sizeof(suffix), pl);
    std::snprintf(buf, buf_len, "mode=%s out=%s dst=%dx%d %s launches=%d kernel=%s shape=%dx%d lds=%d grid=%d tiles=%dx%d staged=%d tail=%d nt=%d limit=%d%s",
                  path.mode_name(pl), path.tensor ? tensor_out_name(path.spec->dtype, pl.out == O_Y800_F32) : out_names[pl.out], pl.dst_w,
                  pl.dst_h, counts, launches, kname, ROI_TX, ROI_TY, lds0 + roi_static_lds(pl.out, vec), grid0, L.tiles_x, L.tiles_y, staged, L.last_col0 > 0 ? 2 : 0, L.nt_stores,
                  limit, suffix);
    return TSVPP_OK;
}

// tile_describe for the paths whose coordinates live in device memory (tsvpp_remap.cpp, tsvpp_mesh.cpp): the line without staged= (the host cannot count what it
// cannot see) and with lds= the dynamic LDS alone, non-zero iff the kernel is the staged one.  The path says mode_name() and counts() ("remaps=8 maps=1 frames=8")
template <class PATH> int tile_describe_unplanned(PATH path, int aligned_outputs, char *buf, size_t buf_len) {
    if (!buf || buf_len == 0) return TSVPP_ERROR;
    buf[0] = 0;
    RoiPlan pl;
    const int sts = tile_request(path, pl);
    if (sts != TSVPP_OK) return sts;
    Knobs kn; // no context: no device, no streams
    read_env_knobs(kn);
    const bool vec = aligned_outputs != 0 && !narrow_tail(pl);
    int lds0 = 0, grid0 = 0, launches = 0;
    char kname[128] = "(none)", border[40] = "replicate", counts[96] = "";
    typename PATH::Launch L;
    const int limit = path.limit(pl);
    for (int base = 0; base < path.n; base += limit, launches++) {
        const int cnt = std::min(path.n - base, limit);
        (void)tile_fill(path, kn, pl, nullptr, base, cnt, vec, L);
        if (base == 0) {
            lds0 = L.lds_bytes;
            grid0 = L.tiles_x * L.tiles_y * cnt;
            const hipError_t e = path.launch(pl, vec, lds0 > 0, L, nullptr, kname, sizeof(kname), true);
            if (e != hipSuccess) return (int)e;
        }
    }
    if (path.border()) std::snprintf(border, sizeof(border), "%d,%d,%d", path.border_y, path.border_u, path.border_v);
    path.counts(counts, sizeof(counts));
    std::snprintf(buf, buf_len, "mode=%s out=%s dst=%dx%d %s launches=%d kernel=%s shape=%dx%d lds=%d grid=%d tiles=%dx%d tail=%d nt=%d limit=%d border=%s",
                  path.mode_name(), path.tensor ? tensor_out_name(path.spec->dtype, pl.out == O_Y800_F32) : out_names[pl.out], pl.dst_w, pl.dst_h, counts, launches,
                  kname, ROI_TX, ROI_TY, lds0, grid0, L.tiles_x, L.tiles_y, L.last_col0 > 0 ? 2 : 0, L.nt_stores, limit, border);
    return TSVPP_OK;
}

} // namespace tsvpp
