// vpp_mesh_core.h -- the control-grid kernel itself (see vpp_mesh.hip for what it does), as a template that two translation units instantiate: vpp_mesh.hip with the
// library's colour back end (EL_LIB: every flavour of tsvpp_convert_mesh) and vpp_mesh_tensor.hip with the tensor store (EL_F32 / EL_HALF:
// tsvpp_convert_mesh_tensor, vpp_tensor_store.h).
//
// It is the coordinate-map kernel (vpp_remap_core.h) with one function exchanged: mesh_load COMPUTES the sixteen luma entries of a thread tile from the control
// points of its cells where remap_load reads them.  From the entries on -- remap_coords (chroma, clamp), remap_reduce, remap_footprint, stage_planes,
// remap_thread_tile and the store -- it calls the dense kernel's functions, so it is the dense kernel on the expanded map E(mesh), bit for bit.  The kernel function
// below repeats vpp_remap_kernel's few lines of orchestration rather than sharing them: with the body behind a common function the dense kernels' register
// allocation changed, and they are to stay as they are (profiles/mesh_resources.txt).
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

// (launch bounds: as vpp_remap_kernel's -- at most 128 VGPRs: profiles/mesh_resources.txt)
template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS, 4) void vpp_mesh_kernel(const MeshLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int item = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (item >= L.n_remaps) return;
    const MeshRec &r = L.r[item]; // wave-uniform index: scalar loads

    // the colour back end and the staging loop read their request from a LaunchDesc (the samplers' fields stay zero: the mesh is the sampler)
    LaunchDesc d = {};
    d.src_w = r.src_w;
    d.src_h = r.src_h;
    d.pitch_y = r.pitch_y;
    d.pitch_uv = r.pitch_uv;
    d.dst_w = L.dst_w;
    d.dst_h = L.dst_h;
    d.swap_rb = L.swap_rb;
    d.color_g = L.color_g;
    d.k = L.k;
    d.tx = ROI_TX;
    d.ty = ROI_TY;
    d.tx_shift = ROI_TX_SHIFT;
    d.rpt = 1;
    d.nt_stores = L.nt_stores;
    d.last_col0 = VEC ? L.last_col0 : 0;
    d.u8_xchg = L.u8_xchg;
    d.luma_only = kLumaOnly<OUT> ? 1 : 0;

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    const uint8_t *const mesh_xy = (const uint8_t *)(GP)(uintptr_t)r.xy;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));

    RemapCoords c;
    mesh_load<VEC>(mesh_xy, r.mesh_pitch, r.log2_cw, r.log2_ch, L.dst_w, L.dst_h, r.src_w, r.src_h, i0, j0, c);

    if constexpr (STAGED) {
        // the tile's source bounding box, from the extremes of its own coordinates: the dense kernel's decision on E(mesh), which tsvpp_remap_footprint describes
        __shared__ float red[2][8];
        static_assert(sizeof(red) == REMAP_REDUCE_LDS, "the budget accounts for the reduction's words");
        const RemapExtremes e = remap_reduce(c, active, red);
        RoiFootprint f;
        remap_footprint(e, r.src_w, r.src_h, f);
        if (roi_stageable(f) && roi_lds_need(f, kLumaOnly<OUT>) <= L.lds_bytes) { // (wave-uniform)
            const int span_y = f.xhi - f.xlo + 1, span_uv = 2 * (f.cxhi - f.cxlo + 1);
            const int ny = f.yhi - f.ylo + 1, nuv = kLumaOnly<OUT> ? 0 : f.cyhi - f.cylo + 1;
            d.lds_cpr_y = roi_chunks(span_y);
            d.lds_cpr_uv = roi_chunks(span_uv);
            d.lds_slot_y = 32 - __builtin_clz(((unsigned)d.lds_cpr_y - 1u) | 1u); // log2 of the lanes that serve one staged row (>= chunks per row)
            d.lds_slot_uv = 32 - __builtin_clz(((unsigned)d.lds_cpr_uv - 1u) | 1u);
            uint8_t *lds_y = lds_raw, *lds_uv = lds_raw + ny * d.lds_cpr_y * 16;
            const uint8_t *ay, *auv;
            LdsSrc s;
            s.py_ = describe_plane(lds_y, plane_y, r.pitch_y, f.ylo, f.xlo, d.lds_cpr_y, ay);
            s.puv_ = describe_plane(lds_uv, plane_uv, r.pitch_uv, f.cylo, 2 * f.cxlo, d.lds_cpr_uv, auv);
            s.w = r.src_w;
            s.h = r.src_h;
            stage_planes<2, 1>(d, lds_y, ay, s.py_, ny, span_y, lds_uv, auv, s.puv_, nuv, span_uv, ROI_THREADS);
            __syncthreads();
            if (active) remap_thread_tile<OUT, VEC, BORDER, EL>(s, d, L, c, out, i0, j0);
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    tile_global_src(s, r, plane_y, plane_uv);
    remap_thread_tile<OUT, VEC, BORDER, EL>(s, d, L, c, out, i0, j0);
}

} // namespace tsvpp
