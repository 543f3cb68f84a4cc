// vpp_letterbox_p010_bicubic_core.h -- the P010 BICUBIC letterbox kernel (see vpp_letterbox_p010_bicubic.hip for what it does), as a template that two translation
// units instantiate: vpp_letterbox_p010_bicubic.hip with the library's output flavours (EL_LIB) and vpp_letterbox_p010_bicubic_tensor.hip with the tensor store.
//
// Called, not copied: the canvas grid (tile_index), the descriptor fill (tile_desc), the rectangle's part of a tile (tile_inner_range), the shifted last tile
// column (roi_tile_col0), and everything behind the samples (p010_store_tile, vpp_letterbox_p010_core.h) -- on integer-valued Yf / Uf / Vf, as the NEAREST /
// BILINEAR kernel hands them over.  The arithmetic is vpp_cubic_p010.h's, shared with the host.  The sampling stage is the two-phase walk of
// vpp_cubic_p010_walk.h (cubic_walk_plane, cubic_vertical: shared with the P010 BICUBIC region-of-interest kernel) on the rectangle's part of the tile.  New
// here: where a lane's columns lie in an Hbuf row, and the pad.
#pragma once
#include "vpp_cubic_p010_walk.h"
#include "vpp_letterbox_p010_bicubic.h"

#pragma clang fp contract(off)

namespace tsvpp {

template <int OUT, bool VEC, int EL = EL_LIB> __global__ __launch_bounds__(ROI_THREADS) void vpp_letterbox_p010_bicubic_kernel(const LbCubicLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int frame = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (frame >= L.n_frames) return;
    const LbRec &r = L.r[frame]; // wave-uniform index: scalar loads

    LaunchDesc d = {};
    tile_desc<OUT, VEC>(L, r, d);
    d.k.y_offset = 4.0f * d.k.y_offset; // the contract's scaled offsets (exact)
    d.k.c_offset = 4.0f * d.k.c_offset;

    const bool uv4 = (((uint32_t)r.uv | (uint32_t)r.pitch_uv) & 3u) == 0u;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));
    const int ncol = VEC ? PXW : min(PXW, L.dst_w - j0);

    // the part of the rectangle this tile covers (wave-uniform), in the rectangle's own indices
    LbPart t;
    tile_inner_range(j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), r.left, r.width, t.a0, t.a1);
    tile_inner_range(i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), r.top, r.height, t.b0, t.b1);
    float Uf[2] = { L.pad_u, L.pad_u }, Vf[2] = { L.pad_v, L.pad_v }, Yf[PXH][PXW];
#pragma unroll
    for (int rr = 0; rr < PXH; rr++)
#pragma unroll
        for (int c = 0; c < PXW; c++) Yf[rr][c] = L.pad_y;
    if (t.a0 > t.a1 || t.b0 > t.b1) { // none of it: pad, through the colour expression and store of every sample
        if (active) p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
        return;
    }

    // Which column pairs of this lane's thread tile lie inside the rectangle: left, width and every tile origin are even, so columns (0, 1) and (2, 3) are each
    // wholly in or out, and so are the thread tile's two rows.  A lane outside still filters its rows of phase A and stands at every barrier.
    const bool rows_in = i0 >= r.top && i0 < r.top + r.height;
    bool in[2];
#pragma unroll
    for (int c = 0; c < 2; c++) in[c] = rows_in && j0 + 2 * c >= r.left && j0 + 2 * c < r.left + r.width;
    const int buf_bytes = box_band_buffer(L.band, L.band_cpr);
    const int cj = j0 - r.left - t.a0, ci = i0 - r.top; // the thread tile's first column as a column of Hbuf (even), its first row as a row of the rectangle

    { // luma: Hbuf column 0 is column t.a0 of the rectangle; a pair of columns is one dword of an Hbuf row.  Pairs outside the part read its nearest pair
        CubicPlane pl = { (const uint8_t *)(GP)(uintptr_t)r.y, r.pitch_y, 0, 0, 0, 0, cubic_div_of(r.src_w, r.width), cubic_div_of(r.src_h, r.height), t.a0, t.a1 - t.a0 + 1 };
        cubic_span(t.a0, t.a1, pl.ax, pl.xlo, pl.xhi); // taps clamp at the frame: the axis is all of it
        cubic_span(t.b0, t.b1, pl.ay, pl.ylo, pl.yhi);
        pl.yhi = min(pl.yhi, pl.ylo + L.hrows - 1); // (never for a launch the host sized: Hbuf holds the launch's tallest footprint)
        cubic_walk_plane<false>(pl, uv4, L.band, buf_bytes, L.hrows);
        const int o0 = 2 * clampi(cj, 0, pl.ncols - 2), o1 = 2 * clampi(cj + 2, 0, pl.ncols - 2);
#pragma unroll
        for (int rr = 0; rr < PXH; rr++) {
            int k[4];
            cubic_vertical(pl, clampi(ci + rr, t.b0, t.b1), o0, o1, k);
#pragma unroll
            for (int c = 0; c < PXW; c++) Yf[rr][c] = in[c >> 1] ? (float)k[c] : L.pad_y;
        }
    }
    if constexpr (!kLumaOnly<OUT>) { // chroma: Hbuf dword 0 is pair t.a0 / 2 of the rectangle's chroma plane
        CubicPlane pl = { (const uint8_t *)(GP)(uintptr_t)r.uv, r.pitch_uv, 0, 0, 0, 0, cubic_div_of(r.src_w >> 1, r.width >> 1), cubic_div_of(r.src_h >> 1, r.height >> 1), t.a0 >> 1, (t.a1 >> 1) - (t.a0 >> 1) + 1 };
        cubic_span(t.a0 >> 1, t.a1 >> 1, pl.ax, pl.xlo, pl.xhi);
        cubic_span(t.b0 >> 1, t.b1 >> 1, pl.ay, pl.ylo, pl.yhi);
        pl.yhi = min(pl.yhi, pl.ylo + L.hrows - 1);
        cubic_walk_plane<true>(pl, uv4, L.band, buf_bytes, L.hrows); // (its first barrier stands behind every lane's luma reads of Hbuf)
        const int o0 = 4 * clampi(cj >> 1, 0, pl.ncols - 1), o1 = 4 * clampi((cj >> 1) + 1, 0, pl.ncols - 1);
        int k[4];
        cubic_vertical(pl, clampi(ci >> 1, t.b0 >> 1, t.b1 >> 1), o0, o1, k);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            Uf[c] = in[c] ? (float)k[2 * c] : L.pad_u;
            Vf[c] = in[c] ? (float)k[2 * c + 1] : L.pad_v;
        }
    }
    if (active) p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

} // namespace tsvpp
