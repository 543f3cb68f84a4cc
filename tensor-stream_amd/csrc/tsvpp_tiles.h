// tsvpp_tiles.h -- the host side of the tile paths, once (tsvpp_rois.cpp: boxes, NEAREST / BILINEAR / BICUBIC and AREA; tsvpp_letterbox.cpp: frames into a padded
// canvas; the coordinate paths tsvpp_warp.cpp, tsvpp_persp.cpp, tsvpp_remap.cpp, tsvpp_mesh.cpp; all with their tensor forms).  All of them launch one 32 x 32
// output tile per workgroup (vpp_tile_core.h) for up to a fixed number of items -- boxes, frames, outputs -- per launch.  Here: the launch fields they share, the
// staging budgets, and the skeletons of the convert and the describe call; behind them what the four coordinate paths share beyond that (CoordRequest).  A path
// is a small struct that holds its request and answers what differs:
//     using Launch                          RoiLaunch / LbLaunch / WarpLaunch / ...
//     kOwnBudget                            false: a tile's footprint is a column span times a row span (item(), below); true: the path sizes the staged
//                                           footprints itself -- stage_budget(pl, L, budget, luma_only) sets L.lds_bytes and returns the items that stage every tile
//     kCountsStaged                         true: the host sees every footprint -- the describe line says staged= and lds= is everything the workgroup holds;
//                                           false (coordinates in device memory): no staged=, lds= is the launch's dynamic LDS alone
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
#include <climits>
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

// (`path` by value: its frames are replaced by a copy without planes)  The line has two formats (kCountsStaged, above): a path whose coordinates live in device
// memory cannot count what stages, and its lds= is non-zero iff the kernel is the staged one.
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
    char kname[128] = "(none)", counts[96] = "", suffix[96] = "", staged_key[24] = "";
    typename PATH::Launch L;
    const int n = path.items(), limit = path.limit(pl);
    for (int base = 0; base < n; base += limit, launches++) {
        const int cnt = std::min(n - base, limit);
        const int s = tile_fill(path, kn, pl, nullptr, base, cnt, vec, L);
        staged += s;
        if (base == 0) {
            lds0 = PATH::kCountsStaged ? path.front_lds(L) + L.lds_bytes + roi_static_lds(pl.out, vec) : L.lds_bytes;
            grid0 = L.tiles_x * L.tiles_y * cnt;
            const hipError_t e = path.launch(pl, vec, s > 0, L, nullptr, kname, sizeof(kname), true);
            if (e != hipSuccess) return (int)e;
        }
    }
    path.counts(counts, sizeof(counts));
    path.suffix(suffix, sizeof(suffix), pl);
    if (PATH::kCountsStaged) std::snprintf(staged_key, sizeof(staged_key), " staged=%d", staged);
    std::snprintf(buf, buf_len, "mode=%s out=%s dst=%dx%d %s launches=%d kernel=%s shape=%dx%d lds=%d grid=%d tiles=%dx%d%s tail=%d nt=%d limit=%d%s",
                  path.mode_name(pl), path.tensor ? tensor_out_name(path.spec->dtype, pl.out == O_Y800_F32) : out_names[pl.out], pl.dst_w,
                  pl.dst_h, counts, launches, kname, ROI_TX, ROI_TY, lds0, grid0, L.tiles_x, L.tiles_y, staged_key, L.last_col0 > 0 ? 2 : 0, L.nt_stores, limit, suffix);
    return TSVPP_OK;
}

// ---- the coordinate paths ----------------------------------------------------------------------------------------------------------------------------------
// tsvpp_warp.cpp, tsvpp_persp.cpp, tsvpp_remap.cpp and tsvpp_mesh.cpp are one path with a different source coordinate: BILINEAR through a coordinate per output
// pixel, a constant border or the replicated edge, a launch block that differs in its record alone (CoordLaunch, vpp_warp.h).  What they share beyond the
// skeletons above is here; a path's own file keeps its record's geometry, its footprint function or hint, its labels and its entry points.

// a launcher of vpp_warp.hip ... vpp_mesh_tensor.hip
template <class LAUNCH>
using CoordLauncher = hipError_t(OutKind, bool vec, bool staged, bool border, const LAUNCH &, unsigned grid, size_t lds_bytes, hipStream_t, char *name, size_t name_len, bool dry_run);

// The request fields of a coordinate path and the answers that do not depend on the coordinate: the base of WarpPath, PerspPath, RemapPath, MeshPath
struct CoordRequest {
    static constexpr bool kOwnBudget = true;
    bool tensor;
    const tsvpp_params *p;
    const tsvpp_tensor_spec *spec;
    int n_frames;
    const tsvpp_nv12 *frames; // (may carry null planes: the describe calls)
    int border_y, border_u, border_v;

    bool border() const { return border_y >= 0; }
    template <class LAUNCH> int front_lds(const LAUNCH &) const { return 0; }
    void suffix(char *buf, size_t len, const RoiPlan &) const {
        if (border()) std::snprintf(buf, len, " border=%d,%d,%d", border_y, border_u, border_v);
        else std::snprintf(buf, len, " border=replicate");
    }
    // of one launch group: the count and the border sample
    template <class LAUNCH> void fill_launch(int cnt, LAUNCH &L) const {
        L.n = cnt;
        L.border_y = (float)border_y;
        L.border_u = (float)border_u;
        L.border_v = (float)border_v;
    }
    // of one record: the planes, pitches and size of its frame, and its output (null in a dry run)
    template <class REC> void fill_rec(int frame, void *out, REC &r) const {
        const tsvpp_nv12 &fr = frames[frame];
        r.y = (uint64_t)(uintptr_t)fr.y;
        r.uv = (uint64_t)(uintptr_t)fr.uv;
        r.out = (uint64_t)(uintptr_t)out;
        r.pitch_y = pitch_or_width(fr.pitch_y, fr.width);
        r.pitch_uv = pitch_or_width(fr.pitch_uv, fr.width);
        r.src_w = fr.width;
        r.src_h = fr.height;
    }
    // One launch group, or only its kernel's name, through the path's pair of launchers.  The staged kernel wherever ANY tile may stage (L.lds_bytes > 0): the
    // kernel decides per tile, and what tile_fill counts is whole outputs
    template <class LAUNCH>
    hipError_t launch_with(CoordLauncher<LAUNCH> *colour, CoordLauncher<LAUNCH> *tensor_unit, const RoiPlan &pl, bool vec, const LAUNCH &L, hipStream_t stream, char *name,
                           size_t name_len, bool dry_run) const {
        const unsigned grid = (unsigned)(L.tiles_x * L.tiles_y * L.n);
        return (tensor ? tensor_unit : colour)(pl.out, vec, L.lds_bytes > 0, border(), L, grid, (size_t)L.lds_bytes, stream, name, name_len, dry_run);
    }
};

// The staging budget of a path whose host knows every coordinate (warp, perspective): FOOTPRINT(record, j0, j1, i0, i1, f) is the footprint function the kernel
// evaluates, so these are every tile's numbers as the kernel will compute them.  The kernel decides per tile (need <= L.lds_bytes), so the launch takes the
// largest box that fits the budget -- a launch may mix staged and gathering tiles -- and the count is of the outputs whose every tile stages.
// (always_inline: this loop IS the host cost of a warp call with large outputs -- 2040 tiles per 1080p output.  Inlined, tile_fill compiles to the instructions
// it had when each path carried its own copy of the loop, three field offsets apart; as a function of its own it did not.  profiles/coord_paths_ab.txt has
// both measurements)
template <auto FOOTPRINT, class LAUNCH> __attribute__((always_inline)) inline int coord_box_budget(const RoiPlan &pl, LAUNCH &L, int budget, bool luma_only) {
    int staged = 0, lds = 0;
    for (int i = 0; i < L.n; i++) {
        bool all = true;
        for (int ty = 0; ty < L.tiles_y; ty++)
            for (int tx = 0; tx < L.tiles_x; tx++) {
                const int j0 = roi_tile_col0(tx, pl.dst_w, L.last_col0), i0 = ty * ROI_TILE_H;
                RoiFootprint f;
                FOOTPRINT(L.r[i], j0, tile_last(j0, ROI_TILE_W, pl.dst_w), i0, tile_last(i0, ROI_TILE_H, pl.dst_h), f);
                const int need = roi_lds_need(f, luma_only);
                if (roi_stageable(f) && need <= budget) lds = std::max(lds, need);
                else all = false;
            }
        staged += all ? 1 : 0;
    }
    L.lds_bytes = lds;
    return staged;
}

// ... and of a path whose coordinates live in device memory (coordinate maps, control grids): no per-tile loop, every workgroup finds its own footprint.  The
// launch's dynamic LDS is its hint -- which fill_items left in L.lds_bytes: coord_hint() over the grids the launch uses -- capped by what the workgroup's budget
// leaves behind `reduce_lds`, the static words of the kernel's footprint reduction.  Returns the outputs that MAY stage: all of the launch or none
inline int coord_hint(int hint, int lds_bytes) { return std::max(hint, lds_bytes > 0 ? lds_bytes : INT_MAX); } // (a grid without a hint: whatever the budget leaves)
template <class LAUNCH> int coord_hint_budget(LAUNCH &L, int budget, int reduce_lds) {
    budget -= reduce_lds;
    L.lds_bytes = budget > 0 ? std::min(L.lds_bytes, budget) : 0;
    return L.lds_bytes > 0 ? L.n : 0;
}

// tile_convert behind the one rule it does not know: grids -- path.grids() of them, grid m at path.grid_xy(m) -- the kernel can address
template <class PATH> int coord_grid_convert(const PATH &path, tsvpp_ctx *ctx, void *const *outs, void *stream) {
    RoiPlan pl;
    if (tile_request(path, pl) == TSVPP_OK) {
        for (int m = 0; m < path.grids(); m++)
            if (!path.grid_xy(m) || ((uintptr_t)path.grid_xy(m) & 7)) {
                clear_last_launch();
                return TSVPP_ERROR;
            }
    }
    return tile_convert(path, ctx, outs, stream);
}

// a footprint as the eight numbers the DEBUG exports hand out (tsvpp_warp_footprint, tsvpp_persp_footprint, tsvpp_remap_footprint)
inline void footprint_export(const RoiFootprint &f, int32_t *out8) {
    const int32_t v[8] = { f.xlo, f.xhi, f.ylo, f.yhi, f.cxlo, f.cxhi, f.cylo, f.cyhi };
    for (int k = 0; k < 8; k++) out8[k] = v[k];
}

} // namespace tsvpp
