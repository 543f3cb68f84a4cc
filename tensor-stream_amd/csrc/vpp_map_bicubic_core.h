// vpp_map_bicubic_core.h -- BICUBIC through a coordinate that is READ or INTERPOLATED: the kernel of tsvpp_convert_remap_bicubic and tsvpp_convert_mesh_bicubic
// (include/tsvpp.h), as ONE template over the coordinate policy (RemapCoordLoad, MeshCoordLoad) that four translation units instantiate: vpp_remap_bicubic.hip /
// vpp_mesh_bicubic.hip with the library's colour back end (EL_LIB) and their *_tensor.hip twins with the tensor store (EL_F32 / EL_HALF).  The existing kernels
// (vpp_remap_core.h, vpp_mesh_core.h, vpp_coord_bicubic_core.h) are not touched: their units compile to the code they had.
//
// What is the BILINEAR map kernel's: the tile and its index, the records and launch blocks, COORD::load (entries, chroma coordinate, THE clamp: the coordinate has
// the BILINEAR call's bits), the reduction of the tile's extremes (remap_reduce), staging (describe_plane, stage_planes), the staged-or-gather decision per tile
// and the store.  What is the matrix paths' BICUBIC: the sampler from the clamped coordinate on (cubic_luma2, cubic_chroma: axis, taps, sums, border test).
// What is new is what joins them:
//   - the footprint: remap_bicubic_footprint (vpp_map_bicubic.h), the reduced extremes through the span rule with the 4-tap halo;
//   - the thread tile: the coordinates come out of registers, one chroma pair's 32 taps, then two luma samples' 32 taps at a time, each group fenced;
//   - the register plan, below at the kernel.
#pragma once
#include "vpp_mesh_core.h"
#include "vpp_coord_bicubic_core.h"
#include "vpp_map_bicubic.h"

#pragma clang fp contract(off)

namespace tsvpp {

// remap_thread_tile with the cubic sampler: 2 x 4 luma samples and 2 chroma pairs of the virtual NV12 frame at the tile's clamped coordinates, then the one
// colour back end.  (A pair or a column that does not exist carries the coordinate of one that does -- remap_coords -- and is never stored.)
template <int OUT, bool VEC, bool BORDER, int EL, class S, class LT>
__device__ __forceinline__ void map_cubic_thread_tile(const S &s, const LaunchDesc &d, const LT &L, const RemapCoords &c, typename OutT<OUT>::type *out, int i0, int j0) {
    const int ncol = VEC ? PXW : min(PXW, d.dst_w - j0);
    float Uf[2] = { 128.0f, 128.0f }, Vf[2] = { 128.0f, 128.0f }, Yf[PXH][PXW];
    if constexpr (!kLumaOnly<OUT>) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            // one pair's 32 taps at a time, as cubic_thread_tile fences them
            __builtin_amdgcn_sched_barrier(0);
            cubic_chroma<BORDER>(s, c.cx[p], c.cy[p], L.border_u, L.border_v, Uf[p], Vf[p]);
        }
    }
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
#pragma unroll
        for (int k = 0; k < PXW; k += 2) {
            // two samples' 32 taps are consumed before the next two samples' are issued
            __builtin_amdgcn_sched_barrier(0);
            const float fx[2] = { c.x[rr][k], c.x[rr][k + 1] }, fy[2] = { c.y[rr][k], c.y[rr][k + 1] };
            cubic_luma2<BORDER>(s, fx, fy, L.border_y, Yf[rr][k], Yf[rr][k + 1]);
        }
    }
    store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

// vpp_coord_map_kernel with the cubic thread tile and footprint, once for both policies.  Launch bounds as its: at least four waves per SIMD, i.e. at most 128
// VGPRs.  Register plan: the thread tile's 20 clamped coordinates stay in registers from the load across the reduction, the staging barrier and into the sampler,
// as the BILINEAR kernel keeps them.  They are consumed group by group -- a fenced group reads 2 or 4 of them -- so what the sampler's peak (the first chroma
// pair: 32 taps, 8 fp64-capable sums) sees beside it is the 20, and the compiler allocates both without scratch: 79 to 102 VGPRs, profiles/map_bicubic_resources.txt.
//   The body is vpp_coord_map_kernel's (vpp_remap_core.h), restated because that template has no sampler parameter and its objects are pinned.  Exactly two
// lines differ, both marked "<- differs": the footprint function and the thread tile.  A fix to the descriptor set-up or the staging block belongs in both.
template <class COORD, int OUT, bool VEC, bool STAGED, bool BORDER, int EL>
__global__ __launch_bounds__(ROI_THREADS, 4) void vpp_map_bicubic_kernel(const typename COORD::Launch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int item = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (item >= L.n) return;
    const auto &r = L.r[item]; // wave-uniform index: scalar loads

    // the colour back end and the staging loop read their request from a LaunchDesc (the samplers' fields stay zero: the map, or the mesh, is the sampler)
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
    const uint8_t *const map_xy = (const uint8_t *)(GP)(uintptr_t)r.xy;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));

    RemapCoords c;
    COORD::template load<VEC>(r, map_xy, L.dst_w, L.dst_h, i0, j0, c);

    if constexpr (STAGED) {
        // the tile's source bounding box with the 4-tap halo, from the extremes of its own coordinates (remap_bicubic_footprint: the function
        // tsvpp_remap_bicubic_footprint evaluates on the host); every tap of every sample of the tile lies inside it
        __shared__ float red[2][8];
        static_assert(sizeof(red) == REMAP_REDUCE_LDS, "the budget accounts for the reduction's words");
        const RemapExtremes e = remap_reduce(c, active, red);
        RoiFootprint f;
        remap_bicubic_footprint(e, r.src_w, r.src_h, f); // <- differs: remap_footprint there
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
            if (active) map_cubic_thread_tile<OUT, VEC, BORDER, EL>(s, d, L, c, out, i0, j0); // <- differs: remap_thread_tile there
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    tile_global_src(s, r, plane_y, plane_uv);
    map_cubic_thread_tile<OUT, VEC, BORDER, EL>(s, d, L, c, out, i0, j0); // <- differs (the same call, gathering)
}

// The paths' tags for launch_coord / launch_coord_tensor (vpp_tile_launch.h)
struct RemapBicubicKernels {
    using Launch = RemapLaunch;
    static constexpr const char *kName = "vpp_remap_bicubic";
    template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL> static constexpr auto kernel() { return &vpp_map_bicubic_kernel<RemapCoordLoad, OUT, VEC, STAGED, BORDER, EL>; }
};
struct MeshBicubicKernels {
    using Launch = MeshLaunch;
    static constexpr const char *kName = "vpp_mesh_bicubic";
    template <int OUT, bool VEC, bool STAGED, bool BORDER, int EL> static constexpr auto kernel() { return &vpp_map_bicubic_kernel<MeshCoordLoad, OUT, VEC, STAGED, BORDER, EL>; }
};

} // namespace tsvpp
