// tsvpp_mesh.cpp -- sparse control-grid warps (include/tsvpp.h): tsvpp_convert_mesh / tsvpp_describe_mesh, their tensor forms (`spec`, null for the first pair;
// kernel vpp_mesh_tensor.hip) and the host-only functions on HOST copies of a mesh and a map: tsvpp_mesh_dims, tsvpp_mesh_expand, tsvpp_mesh_from_map,
// tsvpp_mesh_error, tsvpp_mesh_lds_need; TSVPP_MAX_MESHES outputs per launch, kernel vpp_mesh.hip.  The body is tsvpp_tiles.h's, and so is what the four
// coordinate paths share (CoordRequest): MeshPath says what differs -- the request rules (mesh_plan, tsvpp_plan.cpp) and the record.  The launch's LDS is the
// budget or the caller's hint (coord_hint_budget), as the dense call's: the meshes live in device memory and the host plans nothing per tile.
#include <climits>
#include <cmath>
#include <vector>

#include "tsvpp_tiles.h"
#include "vpp_mesh.h"

using namespace tsvpp;

namespace {

// The request of one call, as tsvpp_tiles.h asks for it
struct MeshPath : CoordRequest {
    using Launch = MeshLaunch;
    static constexpr bool kCountsStaged = false;
    int n_meshes;
    const tsvpp_mesh *meshes; // (may carry null xy: the describe calls)
    int n;
    const tsvpp_remap *remaps;

    int plan(RoiPlan &pl) const { return mesh_plan(p, n_frames, frames, n_meshes, meshes, n, remaps, border_y, border_u, border_v, pl); }
    int items() const { return n; }
    int limit(const RoiPlan &) const { return (int)TSVPP_MAX_MESHES; }
    int grids() const { return n_meshes; }
    const void *grid_xy(int m) const { return meshes[m].xy; }
    // (leaves the launch's hint in L.lds_bytes -- the largest over the meshes it uses -- for stage_budget, which tile_fill calls next)
    void fill_items(const RoiPlan &pl, void *const *outs, int base, int cnt, MeshLaunch &L) const {
        fill_launch(cnt, L);
        int hint = 0;
        for (int i = 0; i < cnt; i++) {
            const tsvpp_mesh &m = meshes[remaps[base + i].map];
            MeshRec &r = L.r[i];
            fill_rec(remaps[base + i].frame, outs ? outs[base + i] : nullptr, r);
            r.xy = (uint64_t)(uintptr_t)m.xy;
            r.mesh_pitch = m.pitch ? m.pitch : 8 * mesh_points(pl.dst_w, m.log2_cw);
            r.log2_cw = m.log2_cw;
            r.log2_ch = m.log2_ch;
            r.pad_ = 0;
            hint = coord_hint(hint, m.lds_bytes);
        }
        L.lds_bytes = hint;
    }
    int stage_budget(const RoiPlan &, MeshLaunch &L, int budget, bool) const { return coord_hint_budget(L, budget, REMAP_REDUCE_LDS); }
    hipError_t launch(const RoiPlan &pl, bool vec, bool, const MeshLaunch &L, hipStream_t stream, char *name, size_t name_len, bool dry_run) const {
        return launch_with(launch_mesh, launch_mesh_tensor, pl, vec, L, stream, name, name_len, dry_run);
    }
    const char *mode_name(const RoiPlan &) const { return "mesh_bilinear"; }
    void counts(char *buf, size_t len) const {
        std::snprintf(buf, len, "remaps=%d meshes=%d cell=%dx%d frames=%d", n, n_meshes, 1 << meshes[0].log2_cw, 1 << meshes[0].log2_ch, n_frames);
    }
    void label(char *buf, size_t len, const RoiPlan &pl, void *stream) const {
        std::snprintf(buf, len, "tsvpp_convert_mesh%s n=%d meshes=%d frames=%d ->%dx%d fourcc=%d stream=%p", tensor ? "_tensor" : "", n, n_meshes, n_frames, pl.dst_w, pl.dst_h, p->fourcc, stream);
    }
};

// ---- HOST copies ----
// A grid of (x, y) fp32 pairs, rows `pitch` bytes apart: a control grid or a dense map
struct HostGrid {
    const uint8_t *xy;
    long pitch;
    float at(int i, int j, int comp) const { return ((const float *)(xy + i * pitch))[2 * j + comp]; }
};
struct HostMesh {
    HostGrid g;
    int dst_w, dst_h, l_cw, l_ch, cols, rows;
    // THE coordinate of output pixel (i, j): mesh_frac and mesh_lerp, as mesh_load calls them
    float coord(int i, int j, int comp) const {
        const int r = i >> l_ch, c = j >> l_cw;
        return mesh_lerp(g.at(r, c, comp), g.at(r, c + 1, comp), g.at(r + 1, c, comp), g.at(r + 1, c + 1, comp), mesh_frac(j, l_cw), mesh_frac(i, l_ch));
    }
};
// a size and a cell: TSVPP_ERROR before TSVPP_UNSUPPORTED, as everywhere
int mesh_geometry(int dst_w, int dst_h, int l_cw, int l_ch) {
    if (dst_w <= 0 || dst_h <= 0 || ((dst_w | dst_h) & 1)) return TSVPP_ERROR;
    if (l_cw < MESH_LOG2_MIN || l_cw > MESH_LOG2_MAX || l_ch < MESH_LOG2_MIN || l_ch > MESH_LOG2_MAX) return TSVPP_UNSUPPORTED;
    return TSVPP_OK;
}
// a pitch for `per_row` pairs: 0 = tight; TSVPP_ERROR for one that is too small, no multiple of 8, or -- tight -- beyond 32 bits
int host_pitch(int pitch, int per_row, long &out) {
    if (pitch != 0 && ((long)pitch < 8L * per_row || (pitch & 7))) return TSVPP_ERROR;
    if (8L * per_row > 0x7fffffffL) return TSVPP_ERROR;
    out = pitch ? (long)pitch : 8L * per_row;
    return TSVPP_OK;
}
int host_mesh(const float *mesh, int pitch, int dst_w, int dst_h, int l_cw, int l_ch, HostMesh &m) {
    const int sts = mesh_geometry(dst_w, dst_h, l_cw, l_ch);
    if (!mesh) return TSVPP_ERROR;
    if (sts != TSVPP_OK) return sts;
    m = HostMesh{ { (const uint8_t *)mesh, 0 }, dst_w, dst_h, l_cw, l_ch, mesh_points(dst_w, l_cw), mesh_points(dst_h, l_ch) };
    return host_pitch(pitch, m.cols, m.g.pitch);
}
void expand(const HostMesh &m, uint8_t *out, long out_pitch) {
    for (int i = 0; i < m.dst_h; i++) {
        float *row = (float *)(out + i * out_pitch);
        for (int j = 0; j < m.dst_w; j++) {
            row[2 * j] = m.coord(i, j, 0);
            row[2 * j + 1] = m.coord(i, j, 1);
        }
    }
}

} // namespace

extern "C" {

int tsvpp_convert_mesh(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes, int n, const tsvpp_remap *remaps,
                       const tsvpp_params *p, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return coord_grid_convert(MeshPath{ { false, p, nullptr, n_frames, frames, border_y, border_u, border_v }, n_meshes, meshes, n, remaps }, ctx, outs, stream);
}

int tsvpp_describe_mesh(const tsvpp_params *p, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes, int n, const tsvpp_remap *remaps,
                        int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(MeshPath{ { false, p, nullptr, n_frames, frames, border_y, border_u, border_v }, n_meshes, meshes, n, remaps }, aligned_outputs, buf, buf_len);
}

int tsvpp_convert_mesh_tensor(tsvpp_ctx *ctx, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes, int n, const tsvpp_remap *remaps,
                              const tsvpp_params *p, const tsvpp_tensor_spec *spec, int border_y, int border_u, int border_v, void *const *outs, void *stream) {
    return coord_grid_convert(MeshPath{ { true, p, spec, n_frames, frames, border_y, border_u, border_v }, n_meshes, meshes, n, remaps }, ctx, outs, stream);
}

int tsvpp_describe_mesh_tensor(const tsvpp_params *p, const tsvpp_tensor_spec *spec, int n_frames, const tsvpp_nv12 *frames, int n_meshes, const tsvpp_mesh *meshes,
                               int n, const tsvpp_remap *remaps, int border_y, int border_u, int border_v, int aligned_outputs, char *buf, size_t buf_len) {
    return tile_describe(MeshPath{ { true, p, spec, n_frames, frames, border_y, border_u, border_v }, n_meshes, meshes, n, remaps }, aligned_outputs, buf, buf_len);
}

int tsvpp_mesh_dims(int dst_w, int dst_h, int log2_cw, int log2_ch, int *cols, int *rows) {
    if (!cols || !rows) return TSVPP_ERROR;
    const int sts = mesh_geometry(dst_w, dst_h, log2_cw, log2_ch);
    if (sts != TSVPP_OK) return sts;
    *cols = mesh_points(dst_w, log2_cw);
    *rows = mesh_points(dst_h, log2_ch);
    return TSVPP_OK;
}

int tsvpp_mesh_expand(const float *host_mesh_xy, int pitch, int dst_w, int dst_h, int log2_cw, int log2_ch, float *out_xy, int out_pitch) {
    HostMesh m;
    if (!out_xy) return TSVPP_ERROR;
    const int sts = host_mesh(host_mesh_xy, pitch, dst_w, dst_h, log2_cw, log2_ch, m);
    if (sts != TSVPP_OK) return sts;
    long op;
    if (host_pitch(out_pitch, dst_w, op) != TSVPP_OK) return TSVPP_ERROR;
    expand(m, (uint8_t *)out_xy, op);
    return TSVPP_OK;
}

int tsvpp_mesh_from_map(const float *host_xy, int pitch, int dst_w, int dst_h, int log2_cw, int log2_ch, float *out_mesh, int out_pitch) {
    if (!host_xy || !out_mesh) return TSVPP_ERROR;
    const int sts = mesh_geometry(dst_w, dst_h, log2_cw, log2_ch);
    if (sts != TSVPP_OK) return sts;
    const int cols = mesh_points(dst_w, log2_cw), rows = mesh_points(dst_h, log2_ch);
    HostGrid map{ (const uint8_t *)host_xy, 0 };
    long op;
    if (host_pitch(pitch, dst_w, map.pitch) != TSVPP_OK || host_pitch(out_pitch, cols, op) != TSVPP_OK) return TSVPP_ERROR;
    // the map at row i < dst_h, column j: an entry, or -- j past the last pixel -- the line through the row's last two entries
    const auto along_x = [&](int i, int j, int comp) -> double {
        if (j < dst_w) return (double)map.at(i, j, comp);
        const double last = map.at(i, dst_w - 1, comp), prev = map.at(i, dst_w - 2, comp);
        return last + (double)(j - (dst_w - 1)) * (last - prev);
    };
    for (int r = 0; r < rows; r++) {
        float *row = (float *)((uint8_t *)out_mesh + r * op);
        const int i = r << log2_ch;
        for (int c = 0; c < cols; c++) {
            const int j = c << log2_cw;
            for (int comp = 0; comp < 2; comp++) {
                double v;
                if (i < dst_h) v = along_x(i, j, comp);
                else { // x first, then y: the line through the last two rows' values at column j
                    const double last = along_x(dst_h - 1, j, comp), prev = along_x(dst_h - 2, j, comp);
                    v = last + (double)(i - (dst_h - 1)) * (last - prev);
                }
                row[2 * c + comp] = (float)v;
            }
        }
    }
    return TSVPP_OK;
}

int tsvpp_mesh_error(const float *host_xy, int pitch, int dst_w, int dst_h, const float *host_mesh_xy, int mesh_pitch, int log2_cw, int log2_ch, float *max_abs) {
    HostMesh m;
    if (!host_xy || !max_abs) return TSVPP_ERROR;
    const int sts = host_mesh(host_mesh_xy, mesh_pitch, dst_w, dst_h, log2_cw, log2_ch, m);
    if (sts != TSVPP_OK) return sts;
    HostGrid map{ (const uint8_t *)host_xy, 0 };
    if (host_pitch(pitch, dst_w, map.pitch) != TSVPP_OK) return TSVPP_ERROR;
    float worst = 0.0f;
    for (int i = 0; i < dst_h; i++)
        for (int j = 0; j < dst_w; j++)
            for (int comp = 0; comp < 2; comp++) {
                const float e = m.coord(i, j, comp), v = map.at(i, j, comp);
                if (std::isfinite(e) && std::isfinite(v)) worst = std::max(worst, std::fabs(e - v));
            }
    *max_abs = worst;
    return TSVPP_OK;
}

int tsvpp_mesh_lds_need(const float *host_mesh_xy, int pitch, int dst_w, int dst_h, int log2_cw, int log2_ch, int frame_w, int frame_h, int luma_only) {
    HostMesh m;
    const int sts = host_mesh(host_mesh_xy, pitch, dst_w, dst_h, log2_cw, log2_ch, m);
    if (sts != TSVPP_OK) return sts;
    std::vector<float> dense((size_t)2 * dst_w * dst_h);
    expand(m, (uint8_t *)dense.data(), 8L * dst_w);
    return tsvpp_remap_lds_need(dense.data(), 0, dst_w, dst_h, frame_w, frame_h, luma_only);
}

} // extern "C"
