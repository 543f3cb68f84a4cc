// vpp_mesh_core.h -- the control-grid kernel itself (see vpp_mesh.hip for what it does), as a template that two translation units instantiate: vpp_mesh.hip with the
// library's colour back end (EL_LIB: every flavour of tsvpp_convert_mesh) and vpp_mesh_tensor.hip with the tensor store (EL_F32 / EL_HALF:
// tsvpp_convert_mesh_tensor, vpp_tensor_store.h).
//
// It is the coordinate-map kernel (vpp_remap_core.h) with one function exchanged: mesh_load COMPUTES the sixteen luma entries of a thread tile from the control
// points of its cells where remap_load reads them.  From the entries on -- remap_coords (chroma, clamp), remap_reduce, remap_footprint, stage_planes,
// remap_thread_tile and the store -- it IS the dense kernel, so it is the dense kernel on the expanded map E(mesh), bit for bit: both calls instantiate one kernel
// template, vpp_coord_map_kernel, over the policy that names the load (MeshCoordLoad, below).
#pragma once
#include "vpp_remap_core.h"
#include "vpp_mesh.h"

#pragma clang fp contract(off)

namespace tsvpp {

// The entries E(mesh) of the thread tile at output (i0, j0), through remap_coords.  Rows and columns are clamped into the output exactly as remap_load clamps
// them, so every lane -- with pixels or without -- computes entries of E(mesh) that remap_load would have read there.
//   Cells: the two rows of a thread tile lie in one cell row (i0 is even, a cell is at least 4 rows high).  Its columns are taken as two PAIRS: a pair starts at
// an even column and a cell is at least 4 columns wide, so a pair never straddles.  The four columns lie in one cell wherever the tile starts at a multiple of 4;
// in the shifted last tile column of a 4 k + 2 wide output they start at 4 m + 2 and the second pair may belong to the next cell: then, and only then, a lane
// fetches a second set of control points.
//   Control points: A B / C D of a cell are 2 x 16 contiguous bytes, fetched per lane.  The lanes of a wave cover 32 columns x 16 rows, i.e. at cell 16 x 16 at most
// 3 x 2 distinct cells: the requests of a row of lanes fall into one or two 64-byte lines, which the vector cache serves.  Staging the tile's (<= 9 x 9) points in
// LDS instead would cost a barrier in front of the reduction's own, LDS words the gather kernel does not otherwise have, and an LDS read where the cached load is
// (2 x 16 bytes per lane against the dense kernel's 2 x 32): not taken.
//   Bounds: r <= (dst_h - 1) >> log2_ch and c <= (dst_w - 1) >> log2_cw, so rows r, r + 1 and bytes [8 c, 8 c + 16) lie inside rows x 8 * cols bytes of the mesh.
template <bool VEC> __device__ __forceinline__ void mesh_load(const uint8_t *xy, int mesh_pitch, int log2_cw, int log2_ch, int dst_w, int dst_h, int src_w, int src_h, int i0, int j0,
                                                              RemapCoords &c) {
    static_assert(PXH == 2 && PXW == 4, "a thread tile is two rows of two pairs");
    struct __attribute__((aligned(8))) Pts { float v[4]; }; // two control points: x, y, x, y -- 16 contiguous bytes, 8-byte aligned
    const int ic = min(i0, dst_h - PXH); // (dst_h is even, i0 is even)
    int col[PXW];
#pragma unroll
    for (int k = 0; k < PXW; k++) col[k] = VEC ? min(j0, dst_w - PXW) + k : min(j0 + k, dst_w - 1);
    const uint8_t *const row = xy + (size_t)(ic >> log2_ch) * (size_t)mesh_pitch;
    const int cell0 = col[0] >> log2_cw, cell1 = col[2] >> log2_cw;
    Pts top[2], bot[2];
    top[0] = *(const Pts *)(row + 8 * (size_t)cell0);
    bot[0] = *(const Pts *)(row + (size_t)mesh_pitch + 8 * (size_t)cell0);
    top[1] = top[0];
    bot[1] = bot[0];
    if (cell1 != cell0) {
        top[1] = *(const Pts *)(row + 8 * (size_t)cell1);
        bot[1] = *(const Pts *)(row + (size_t)mesh_pitch + 8 * (size_t)cell1);
    }
    float ex[PXH][PXW], ey[PXH][PXW];
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
        const float ty = mesh_frac(ic + rr, log2_ch);
#pragma unroll
        for (int k = 0; k < PXW; k++) {
            const float tx = mesh_frac(col[k], log2_cw);
            const Pts &t = top[k >> 1], &b = bot[k >> 1];
            ex[rr][k] = mesh_lerp(t.v[0], t.v[2], b.v[0], b.v[2], tx, ty);
            ey[rr][k] = mesh_lerp(t.v[1], t.v[3], b.v[1], b.v[3], tx, ty);
        }
    }
    remap_coords<VEC>(ex, ey, dst_w, src_w, src_h, j0, c);
}

// The control-grid call's policy for vpp_coord_map_kernel (vpp_remap_core.h): the coordinates of a thread tile are interpolated from record r's mesh
struct MeshCoordLoad {
    using Launch = MeshLaunch;
    template <bool VEC> static __device__ __forceinline__ void load(const MeshRec &r, const uint8_t *xy, int dst_w, int dst_h, int i0, int j0, RemapCoords &c) {
        mesh_load<VEC>(xy, r.mesh_pitch, r.log2_cw, r.log2_ch, dst_w, dst_h, r.src_w, r.src_h, i0, j0, c);
    }
};

// The path's tag for launch_coord / launch_coord_tensor (vpp_tile_launch.h)
struct MeshKernels {
    using Launch = MeshLaunch;
    static constexpr const char *kName = "vpp_mesh";
    template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL> static constexpr auto kernel() { return &vpp_coord_map_kernel<MeshCoordLoad, OUT, VEC, STAGED, BORDER, EL>; }
};

} // namespace tsvpp
