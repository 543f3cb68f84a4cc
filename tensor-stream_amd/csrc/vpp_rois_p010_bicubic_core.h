// vpp_rois_p010_bicubic_core.h -- the P010 BICUBIC region-of-interest kernel (see vpp_rois_p010_bicubic.hip for what it does), as a template that two translation
// units instantiate: vpp_rois_p010_bicubic.hip with the library's output flavours (EL_LIB) and vpp_rois_p010_bicubic_tensor.hip with the tensor store.
//
// Called, not copied: the grid (tile_index), the descriptor fill (tile_desc), the shifted last tile column (roi_tile_col0), describe_plane and the LDS-DMA loop
// (stage_plane_dma), the chroma pair reader (p010_pair), and everything behind the samples (p010_store_tile, vpp_letterbox_p010_core.h) -- on integer-valued
// Yf / Uf / Vf, as the NEAREST / BILINEAR kernel hands them over.  The arithmetic is vpp_cubic_p010.h's, shared with the host.  The sampling stage is a
// separable filter in two phases through LDS (cubic_walk_plane, cubic_vertical: vpp_cubic_p010_walk.h, shared with the P010 BICUBIC letterbox kernel).
#pragma once
#include "vpp_cubic_p010_walk.h"
#include "vpp_rois_p010_bicubic.h"

#pragma clang fp contract(off)

namespace tsvpp {

// ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------------
template <int OUT, bool VEC, int EL = EL_LIB> __global__ __launch_bounds__(ROI_THREADS) void vpp_rois_p010_bicubic_kernel(const RoiCubicLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int box = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (box >= L.n_rois) return;
    const RoiRec &r = L.r[box]; // wave-uniform index: scalar loads

    LaunchDesc d = {};
    tile_desc<OUT, VEC>(L, r, d);
    d.k.y_offset = 4.0f * d.k.y_offset; // the contract's scaled offsets (exact)
    d.k.c_offset = 4.0f * d.k.c_offset;

    const bool uv4 = (((uint32_t)r.uv | (uint32_t)r.pitch_uv) & 3u) == 0u;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j_last = tile_last(j_first, ROI_TILE_W, L.dst_w), i_last = tile_last(i_first, ROI_TILE_H, L.dst_h);
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));
    const int ncol = VEC ? PXW : min(PXW, L.dst_w - j0);
    const int buf_bytes = box_band_buffer(L.band, L.band_cpr);
    float Uf[2] = { 0.0f, 0.0f }, Vf[2] = { 0.0f, 0.0f }, Yf[PXH][PXW]; // (Y800 stores neither U nor V)

    { // luma
        CubicPlane pl = { (const uint8_t *)(GP)(uintptr_t)r.y, r.pitch_y, 0, 0, 0, 0, cubic_div_of(r.src_w, L.dst_w), cubic_div_of(r.src_h, L.dst_h), j_first, j_last - j_first + 1 };
        cubic_span(j_first, j_last, pl.ax, pl.xlo, pl.xhi);
        cubic_span(i_first, i_last, pl.ay, pl.ylo, pl.yhi);
        pl.yhi = min(pl.yhi, pl.ylo + L.hrows - 1); // (never for a launch the host sized: Hbuf holds the launch's tallest footprint)
        cubic_walk_plane<false>(pl, uv4, L.band, buf_bytes, L.hrows);
#pragma unroll
        for (int rr = 0; rr < PXH; rr++) {
            int k[4];
            cubic_vertical(pl, min(i0 + rr, i_last), 8 * lx, 8 * lx + 4, k);
#pragma unroll
            for (int c = 0; c < PXW; c++) Yf[rr][c] = (float)k[c];
        }
    }
    if constexpr (!kLumaOnly<OUT>) {
        CubicPlane pl = { (const uint8_t *)(GP)(uintptr_t)r.uv, r.pitch_uv, 0, 0, 0, 0, cubic_div_of(r.src_w >> 1, L.dst_w >> 1), cubic_div_of(r.src_h >> 1, L.dst_h >> 1), j_first >> 1, (j_last >> 1) - (j_first >> 1) + 1 };
        cubic_span(j_first >> 1, j_last >> 1, pl.ax, pl.xlo, pl.xhi);
        cubic_span(i_first >> 1, i_last >> 1, pl.ay, pl.ylo, pl.yhi);
        pl.yhi = min(pl.yhi, pl.ylo + L.hrows - 1);
        cubic_walk_plane<true>(pl, uv4, L.band, buf_bytes, L.hrows); // (its first barrier stands behind every lane's luma reads of Hbuf)
        int k[4];
        cubic_vertical(pl, min(i0, i_last) >> 1, 8 * lx, 8 * lx + 4, k);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            Uf[c] = (float)k[2 * c];
            Vf[c] = (float)k[2 * c + 1];
        }
    }
    if (active) p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

} // namespace tsvpp
