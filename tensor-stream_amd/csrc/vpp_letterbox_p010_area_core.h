// vpp_letterbox_p010_area_core.h -- the P010 AREA letterbox kernel (see vpp_letterbox_p010_area.hip for what it does), as a template that two translation units
// instantiate: vpp_letterbox_p010_area.hip with the library's output flavours (EL_LIB) and vpp_letterbox_p010_area_tensor.hip with the tensor store.
//
// Called, not copied: the canvas grid (tile_index), the descriptor fill (tile_desc), the rectangle's part of a tile (tile_inner_range), the shifted last tile
// column (roi_tile_col0), describe_plane and the LDS-DMA loop (stage_plane_dma), the chroma pair reader (p010_pair), and everything behind the samples
// (p010_store_tile, vpp_letterbox_p010_core.h) -- on integer-valued Yf / Uf / Vf, as the NEAREST / BILINEAR kernel hands them over.  The arithmetic is
// vpp_box_p010.h's, shared with the host.  The sampling stage is a walk over the tile's source footprint in bands of rows (box_walk_plane, vpp_box_p010_walk.h:
// shared with the P010 AREA region-of-interest kernel).
#pragma once
#include "vpp_box_p010_walk.h"
#include "vpp_letterbox_p010_area.h"

#pragma clang fp contract(off)

namespace tsvpp {

template <int OUT, bool VEC, int EL = EL_LIB> __global__ __launch_bounds__(ROI_THREADS) void vpp_letterbox_p010_area_kernel(const LbBoxLaunch L) {
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

    // the part of the rectangle this tile covers (wave-uniform)
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

    // which chroma pairs of this lane's thread tile lie inside the rectangle; a thread tile wholly outside adds up nothing
    const bool rows_in = i0 >= r.top && i0 < r.top + r.height;
    bool in[2];
#pragma unroll
    for (int c = 0; c < 2; c++) in[c] = rows_in && j0 + 2 * c >= r.left && j0 + 2 * c < r.left + r.width;
    const bool sample = active && (in[0] || in[1]);
    const int buf_bytes = box_band_buffer(L.band, L.band_cpr);

    { // luma
        BoxPlane pl = { (const uint8_t *)(GP)(uintptr_t)r.y, r.pitch_y, 0, 0, 0, 0, (uint32_t)r.src_w, (uint32_t)r.width, (uint32_t)r.src_h, (uint32_t)r.height, t.a0, t.a1 - t.a0 + 1 };
        box_span(t.a0, t.a1, r.src_w, r.width, pl.xlo, pl.xhi);
        box_span(t.b0, t.b1, r.src_h, r.height, pl.ylo, pl.yhi);
        roi_clamp(pl.xlo, pl.xhi, r.src_w);
        roi_clamp(pl.ylo, pl.yhi, r.src_h);
        int jr[PXH], col[PXW];
#pragma unroll
        for (int rr = 0; rr < PXH; rr++) jr[rr] = clampi(i0 - r.top + rr, t.b0, t.b1);
#pragma unroll
        for (int c = 0; c < PXW; c++) col[c] = clampi(j0 - r.left + c, t.a0, t.a1) - t.a0;
        uint32_t acc[PXH][PXW] = {};
        box_walk_plane<false, PXH>(pl, uv4, L.band, buf_bytes, sample, jr, col, acc);
        const BoxDiv dv = box_div_of(64u * pl.Ny);
#pragma unroll
        for (int rr = 0; rr < PXH; rr++)
#pragma unroll
            for (int c = 0; c < PXW; c++) Yf[rr][c] = in[c >> 1] ? (float)box_sample(acc[rr][c], pl.Ny, dv) : L.pad_y;
    }
    if constexpr (!kLumaOnly<OUT>) {
        BoxPlane pl = { (const uint8_t *)(GP)(uintptr_t)r.uv, r.pitch_uv, 0, 0, 0, 0, (uint32_t)r.src_w >> 1, (uint32_t)r.width >> 1, (uint32_t)r.src_h >> 1, (uint32_t)r.height >> 1, t.a0 >> 1, (t.a1 >> 1) - (t.a0 >> 1) + 1 };
        box_span(t.a0 >> 1, t.a1 >> 1, r.src_w >> 1, r.width >> 1, pl.xlo, pl.xhi);
        box_span(t.b0 >> 1, t.b1 >> 1, r.src_h >> 1, r.height >> 1, pl.ylo, pl.yhi);
        roi_clamp(pl.xlo, pl.xhi, r.src_w >> 1);
        roi_clamp(pl.ylo, pl.yhi, r.src_h >> 1);
        const int jr[1] = { clampi((i0 - r.top) >> 1, t.b0 >> 1, t.b1 >> 1) }, cj0 = (j0 - r.left) >> 1;
        int col[4];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            col[2 * c] = 2 * (clampi(cj0 + c, t.a0 >> 1, t.a1 >> 1) - (t.a0 >> 1));
            col[2 * c + 1] = col[2 * c] + 1;
        }
        uint32_t acc[1][4] = {};
        box_walk_plane<true, 1>(pl, uv4, L.band, buf_bytes, sample, jr, col, acc);
        const BoxDiv dv = box_div_of(64u * pl.Ny);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            Uf[c] = in[c] ? (float)box_sample(acc[0][2 * c], pl.Ny, dv) : L.pad_u;
            Vf[c] = in[c] ? (float)box_sample(acc[0][2 * c + 1], pl.Ny, dv) : L.pad_v;
        }
    }
    if (active) p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

} // namespace tsvpp
