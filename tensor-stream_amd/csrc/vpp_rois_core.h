// vpp_rois_core.h -- the region-of-interest kernel itself (see vpp_rois.hip for what it does), as a template that two translation units instantiate: vpp_rois.hip
// with the library's colour back end (EL_LIB: every flavour of tsvpp_convert_rois) and vpp_rois_tensor.hip with the tensor store (EL_F32 / EL_HALF:
// tsvpp_convert_rois_tensor, vpp_tensor_store.h).  Nothing but the store call differs between them.
#pragma once
#include "vpp_tile_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

template <int MODE, int OUT, bool VEC, bool STAGED, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS) void vpp_rois_kernel(const RoiLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses (PtrCol, vpp_kernels.h)
    // workgroup -> (box, tile): all tiles of a box are neighbours in the grid, so the lines that adjacent tiles share meet in L2
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int box = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (box >= L.n_rois) return;
    const RoiRec &r = L.r[box]; // wave-uniform index: scalar loads

    // the samplers and the colour back end read their request from a LaunchDesc: this box's (written out, like the GlobalSrc fill below: with tile_desc /
    // tile_global_src of vpp_tile_core.h the BILINEAR Y800 element-wise gather kernels of this template compile to other instructions)
    LaunchDesc d = {};
    d.src_w = r.src_w;
    d.src_h = r.src_h;
    d.pitch_y = r.pitch_y;
    d.pitch_uv = r.pitch_uv;
    d.dst_w = L.dst_w;
    d.dst_h = L.dst_h;
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
    d.last_col0 = VEC ? L.last_col0 : 0;
    d.u8_xchg = L.u8_xchg;
    d.luma_only = kLumaOnly<OUT> ? 1 : 0;

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    // (the coordinates are written out in all three tile kernels: as a helper of vpp_tile_core.h they moved VGPRs in vpp_rois_kernel and vpp_letterbox_kernel)
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));

    if constexpr (STAGED) {
        RoiFootprint f;
        tile_span_x(MODE, j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), r.src_w, r.xr, f);
        tile_span_y(MODE, i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), r.src_h, r.yr, f);
        if (roi_stageable(f) && roi_lds_need(f, kLumaOnly<OUT>) <= L.lds_bytes) { // (wave-uniform)
            // (the staging block is written out in all three tile kernels: as a helper it changed their instructions and measured slower, profiles/tile_core_ab.txt)
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
            // two luma + one chroma chunk per lane in flight per round.  More was measured and not kept: with 16 + 8 in flight a single 112 x 112 box (16 tiles of up to
            // 36 KiB) went from 6.8 to 6.4 us, but the kernels grew from ~100 to 186 VGPRs and a 224 x 224 box (49 small tiles) from 5.1 to 6.1 us, 64 of them from 15.8 to 22 us
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
