// tsvpp_remap.cpp -- per-pixel coordinate maps (include/tsvpp.h): tsvpp_convert_remap / tsvpp_describe_remap, their tensor forms (`spec`, null for the first pair;
// kernel vpp_remap_tensor.hip) and the two host-only functions on a HOST copy of a map, tsvpp_remap_footprint and tsvpp_remap_lds_need; TSVPP_MAX_REMAPS outputs
// per launch, kernel vpp_remap.hip.  The body is tsvpp_tiles.h's, and so is what the four coordinate paths share (CoordRequest); RemapPath below says what
// differs: the request rules (remap_plan, tsvpp_plan.cpp), the record, and where a launch's LDS hint comes from -- the maps live in device memory, so there is
// NO per-tile loop on the convert path: the launch asks for the budget or for the caller's hint (coord_hint_budget), and every workgroup finds its own footprint.
#include <climits>
#include <cmath>

#include "tsvpp_tiles.h"
#include "vpp_remap.h"

using namespace tsvpp;

namespace {

// The request of one call, as tsvpp_tiles.h asks for it
struct RemapPath : CoordRequest {
    using Launch = RemapLaunch;
    static constexpr bool kCountsStaged = false;
    int n_maps;
    const tsvpp_map *maps;    // (may carry null xy: the describe calls)
    int n;
    const tsvpp_remap *remaps;

    int plan(RoiPlan &pl) const { return remap_plan(p, n_frames, frames, n_maps, maps, n, remaps, border_y, border_u, border_v, pl); }
    int items() const { return n; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_REMAPS; }
    int grids() const { return n_maps; }
    const void *grid_xy(int m) const { return maps[m].xy; }
    // (leaves the launch's hint in L.lds_bytes -- the largest over the maps it uses -- for stage_budget, which tile_fill calls next)
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, RemapLaunch &L) const {
        fill_launch(cnt, L);
        int hint = 0;
        for (int i = 0; i < cnt; i++) {
            const tsvpp_map &m = maps[remaps[base + i].map];
            RemapRec &r = L.r[i];
            fill_rec(remaps[base + i].frame, outs ? outs[base + i] : nullptr, r);
            r.xy = (uint64_t)(uintptr_t)m.xy;
            r.map_pitch = m.pitch ? m.pitch : 8 * pl.dst_w;
            r.pad_ = 0;
            hint = coord_hint(hint, m.lds_bytes);
        }
        L.lds_bytes = hint;
    }
    int stage_budget(const RoiPlan &, RemapLaunch &L, int budget, bool) const { return coord_hint_budget(L, budget, REMAP_REDUCE_LDS); }
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const RemapLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        return launch_with(launch_remap, launch_remap_tensor, pl, vec, L, stream, name, name_len, dry_run);
    }
    const char *mode_name(const RoiPlan &) const { return "remap_bilinear"; }
    void counts(char *buf, size_t len) const { std::snprintf(buf, len, "remaps=%d maps=%d frames=%d", n, n_maps, n_frames); }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_remap%s n=%d maps=%d frames=%d ->%dx%d fourcc=%d stream=%p", tensor ? "_tensor" : "", n, n_maps, n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
};

// ---- a HOST copy of a map ----
struct HostMap {
    const uint8_t *xy;
    long pitch;
    int dst_w, dst_h, frame_w, frame_h;
    float x(int i, int j) const { return ((const float *)(xy + i * pitch))[2 * j]; }
    float y(int i, int j) const { return ((const float *)(xy + i * pitch))[2 * j + 1]; }
};
int host_map(const float *host_xy, int pitch, int dst_w, int dst_h, int frame_w, int frame_h, HostMap &m) {
    if (!host_xy || dst_w <= 0 || dst_h <= 0 || frame_w <= 0 || frame_h <= 0 || ((dst_w | dst_h | frame_w | frame_h) & 1)) return TSVPP_ERROR;
    if (pitch != 0 && ((long)pitch < 8L * dst_w || (pitch & 7))) return TSVPP_ERROR;
    m = HostMap{ (const uint8_t *)host_xy, pitch ? (long)pitch : 8L * dst_w, dst_w, dst_h, frame_w, frame_h };
    return TSVPP_OK;
}
// The footprint of output columns [j0, j1] / rows [i0, i1] (even first, odd last): the extremes the workgroup reduces, accumulated in a loop, through THE
// footprint function
void host_footprint(const HostMap &m, int j0, int j1, int i0, int i1, RoiFootprint &f) {
    const float inf = INFINITY;
    RemapExtremes e = { inf, -inf, inf, -inf, inf, -inf, inf, -inf };
    for (int i = i0; i <= i1; i++)
        for (int j = j0; j <= j1; j++) {
            const float cx = remap_clamp(m.x(i, j), m.frame_w), cy = remap_clamp(m.y(i, j), m.frame_h);
            e.x_lo = fminf(e.x_lo, cx);
            e.x_hi = fmaxf(e.x_hi, cx);
            e.y_lo = fminf(e.y_lo, cy);
            e.y_hi = fmaxf(e.y_hi, cy);
        }
    for (int ci = i0 >> 1; ci <= i1 >> 1; ci++)
        for (int cj = j0 >> 1; cj <= j1 >> 1; cj++) {
            const int i = 2 * ci, j = 2 * cj;
            const float cx = remap_clamp(remap_chroma(m.x(i, j), m.x(i, j + 1), m.x(i + 1, j), m.x(i + 1, j + 1)), m.frame_w >> 1);
            const float cy = remap_clamp(remap_chroma(m.y(i, j), m.y(i, j + 1), m.y(i + 1, j), m.y(i + 1, j + 1)), m.frame_h >> 1);
            e.cx_lo = fminf(e.cx_lo, cx);
            e.cx_hi = fmaxf(e.cx_hi, cx);
            e.cy_lo = fminf(e.cy_lo, cy);
            e.cy_hi = fmaxf(e.cy_hi, cy);
        }
    remap_footprint(e, m.frame_w, m.frame_h, f);
}

} // namespace

extern "C" {

int tsvpp_convert_remap(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps, int n, const tsvpp_remap *remaps,
                        const tsvpp_params *p, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return coord_grid_convert(RemapPath{ { false, p, nullptr, n_frames, frames, border_y, border_u, border_v }, n_maps, maps, n, remaps }, ctx, outs, stream);
}

int tsvpp_describe_remap(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps, int n, const tsvpp_remap *remaps,
                         int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(RemapPath{ { false, p, nullptr, n_frames, frames, border_y, border_u, border_v }, n_maps, maps, n, remaps }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_remap_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps, int n, const tsvpp_remap *remaps,
                               const tsvpp_params *p, const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return coord_grid_convert(RemapPath{ { true, p, spec, n_frames, frames, border_y, border_u, border_v }, n_maps, maps, n, remaps }, ctx, outs, stream);
}

int tsvpp_describe_remap_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_maps, const tsvpp_map *maps,
                                int n, const tsvpp_remap *remaps, int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(RemapPath{ { true, p, spec, n_frames, frames, border_y, border_u, border_v }, n_maps, maps, n, remaps }, aligned_outputs, buf, buf_len);
}

int tsvpp_remap_footprint(const float *host_xy, int pitch, int dst_w, int dst_h, int frame_w, int frame_h, int j_first, int j_last, int i_first, int i_last,
                          int32_t *out8) {
    HostMap m;
    if (!out8 || host_map(host_xy, pitch, dst_w, dst_h, frame_w, frame_h, m) != TSVPP_OK) return TSVPP_ERROR;
    if (j_first < 0 || i_first < 0 || j_last < j_first || i_last < i_first || j_last >= dst_w || i_last >= dst_h) return TSVPP_ERROR;
    if ((j_first & 1) || (i_first & 1) || !(j_last & 1) || !(i_last & 1)) return TSVPP_ERROR; // whole pairs: even first, odd last
    RoiFootprint f;
    host_footprint(m, j_first, j_last, i_first, i_last, f);
    footprint_export(f, out8);
    return TSVPP_OK;
}

int tsvpp_remap_lds_need(const float *host_xy, int pitch, int dst_w, int dst_h, int frame_w, int frame_h, int luma_only) {
    HostMap m;
    if (host_map(host_xy, pitch, dst_w, dst_h, frame_w, frame_h, m) != TSVPP_OK) return TSVPP_ERROR;
    const int tiles_x = (dst_w + ROI_TILE_W - 1) / ROI_TILE_W, tiles_y = (dst_h + ROI_TILE_H - 1) / ROI_TILE_H;
    const int shifted = ((dst_w & 3) != 0 && dst_w >= ROI_TILE_W) ? dst_w - ROI_TILE_W : 0; // the vector flavour's last tile column (tile_fill, tsvpp_tiles.h)
    int need = 0;
    for (int ty = 0; ty < tiles_y; ty++)
        for (int tx = 0; tx < tiles_x + (shifted ? 1 : 0); tx++) {
            const int j0 = tx < tiles_x ? tx * ROI_TILE_W : shifted, i0 = ty * ROI_TILE_H;
            RoiFootprint f;
            host_footprint(m, j0, tile_last(j0, ROI_TILE_W, dst_w), i0, tile_last(i0, ROI_TILE_H, dst_h), f);
            // (in 64 bits: a tile that folds a huge frame into itself)
            const long ny = f.yhi - f.ylo + 1, nuv = luma_only ? 0 : f.cyhi - f.cylo + 1;
            const long bytes = 16L * (ny * roi_chunks(f.xhi - f.xlo + 1) + nuv * roi_chunks(2 * (f.cxhi - f.cxlo + 1)));
            need = (int)std::max((long)need, std::min(bytes, (long)INT_MAX));
        }
    return need;
}

} // extern "C"
