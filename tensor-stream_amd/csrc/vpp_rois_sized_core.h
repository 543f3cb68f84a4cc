// vpp_rois_sized_core.h -- the region-of-interest kernel with per-box output sizes (see vpp_rois_sized.hip), as a template that two translation units instantiate:
// vpp_rois_sized.hip with the library's colour back end (EL_LIB) and vpp_rois_sized_tensor.hip with the tensor store (EL_F32 / EL_HALF).  It is vpp_rois_kernel
// (vpp_rois_core.h) with its output side -- dst_w, dst_h, last_col0, the workgroup's (box, tile) -- read from the box's record instead of the launch; the footprint,
// the staged / gather decision, stage_planes<2, 1> and the thread tiles are the shared ones, called as there.
#pragma once
#include "vpp_tile_core.h"
#include "vpp_rois_sized.h"

#pragma clang fp contract(off)

namespace tsvpp {

template <int MODE, int OUT, bool VEC, bool STAGED, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS) void vpp_rois_sized_kernel(const SizedLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    // workgroup -> (box, tile): the grid is exactly the sum of the boxes' tile counts, so every workgroup has a tile (sized_tile, vpp_rois_sized.h)
    const SizedTile tix = sized_tile(L, blockIdx.x);
    const int box = tix.box, tyi = tix.tyi, txi = tix.txi;
    if (box >= L.n_rois) return; // (never for the grid the host launches: keeps a stray workgroup off the records)
    const SizedRec &r = L.r[box]; // wave-uniform index: scalar loads

    // the samplers and the colour back end read their request from a LaunchDesc: this box's, output side included (written out as in vpp_rois_kernel)
    LaunchDesc d = {};
    d.src_w = r.src_w;
    d.src_h = r.src_h;
    d.pitch_y = r.pitch_y;
    d.pitch_uv = r.pitch_uv;
    d.dst_w = r.dst_w;
    d.dst_h = r.dst_h;
    d.xr = r.xr;
    d.yr = r.yr;
    d.swap_rb = L.swap_rb;
    d.color_g = L.color_g;
    d.k = L.k;
    d.tx = ROI_TX;
    d.ty = ROI_TY;
    d.tx_shift = ROI_TX_SHIFT;
    d.rpt = 1;
    d.nt_stores = L.nt_stores;
    d.last_col0 = sized_last_col0(VEC, r.dst_w);
    d.u8_xchg = L.u8_xchg;
    d.luma_only = kLumaOnly<OUT> ? 1 : 0;

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, r.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < r.dst_w && i0 < r.dst_h && !(VEC && is_row_tail(d, j0));

    if constexpr (STAGED) {
        RoiFootprint f;
        tile_span_x(MODE, j_first, tile_last(j_first, ROI_TILE_W, r.dst_w), r.src_w, r.xr, f);
        tile_span_y(MODE, i_first, tile_last(i_first, ROI_TILE_H, r.dst_h), r.src_h, r.yr, f);
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
            if (active) {
                if constexpr (EL == EL_LIB) convert_thread_tile<MODE, OUT, VEC>(s, d, out, i0, j0);
                else tensor_thread_tile<MODE, OUT, VEC, EL>(s, d, L.spec, (uint8_t *)out, i0, j0);
            }
            return;
        }
    }
    if (!active) return;
    GlobalSrc s;
    s.y = plane_y;
    s.uv = plane_uv;
    s.py = r.pitch_y;
    s.puv = r.pitch_uv;
    s.w = r.src_w;
    s.h = r.src_h;
    if constexpr (EL == EL_LIB) convert_thread_tile<MODE, OUT, VEC>(s, d, out, i0, j0);
    else tensor_thread_tile<MODE, OUT, VEC, EL>(s, d, L.spec, (uint8_t *)out, i0, j0);
}

} // namespace tsvpp
