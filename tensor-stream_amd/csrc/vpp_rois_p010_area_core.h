// vpp_rois_p010_area_core.h -- the P010 AREA region-of-interest kernel (see vpp_rois_p010_area.hip for what it does), as a template that two translation units
// instantiate: vpp_rois_p010_area.hip with the library's output flavours (EL_LIB) and vpp_rois_p010_area_tensor.hip with the tensor store.
//
// Called, not copied: the grid (tile_index), the descriptor fill (tile_desc), the shifted last tile column (roi_tile_col0), the band walk with its LDS-DMA
// staging (box_walk_plane, vpp_box_p010_walk.h: the P010 AREA letterbox kernel's), and everything behind the samples (p010_store_tile,
// vpp_letterbox_p010_core.h) -- on integer-valued Yf / Uf / Vf, as the NEAREST / BILINEAR kernel hands them over.  The arithmetic is vpp_box_p010.h's, shared
// with the host.  New here: the tile's footprint inside the BOX's plane, with no canvas, pad or rectangle around it.
#pragma once
#include "vpp_box_p010_walk.h"
#include "vpp_rois_p010_area.h"

#pragma clang fp contract(off)

namespace tsvpp {

// The tile's footprint in one plane of its box: output columns [a0, a1] x rows [b0, b1] of an N -> n resize per axis, exact, and clamped into the box's plane
// (Nx x Ny samples / pairs) -- never the frame's: the records' plane addresses start at the box origin and no word outside the box may be read into a sum.
__device__ __forceinline__ BoxPlane roi_box_plane(const uint8_t *base, int pitch, int Nx, int nx, int Ny, int ny, int a0, int a1, int b0, int b1) {
    BoxPlane pl = { base, pitch, 0, 0, 0, 0, (uint32_t)Nx, (uint32_t)nx, (uint32_t)Ny, (uint32_t)ny, a0, a1 - a0 + 1 };
    box_span(a0, a1, Nx, nx, pl.xlo, pl.xhi);
    box_span(b0, b1, Ny, ny, pl.ylo, pl.yhi);
    roi_clamp(pl.xlo, pl.xhi, Nx); // (for every valid request the clamps never fire)
    roi_clamp(pl.ylo, pl.yhi, Ny);
    return pl;
}

template <int OUT, bool VEC, int EL = EL_LIB> __global__ __launch_bounds__(ROI_THREADS) void vpp_rois_p010_area_kernel(const RoiBoxLaunch L) {
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
    float Uf[2] = { 0.0f, 0.0f }, Vf[2] = { 0.0f, 0.0f }, Yf[PXH][PXW]; // (Y800 stores neither U nor V)

    const int buf_bytes = box_band_buffer(L.band, L.band_cpr);
    const BoxPlane py = roi_box_plane((const uint8_t *)(GP)(uintptr_t)r.y, r.pitch_y, r.src_w, L.dst_w, r.src_h, L.dst_h, j_first, j_last, i_first, i_last);

    { // luma
        int jr[PXH], col[PXW];
#pragma unroll
        for (int rr = 0; rr < PXH; rr++) jr[rr] = clampi(i0 + rr, i_first, i_last);
#pragma unroll
        for (int c = 0; c < PXW; c++) col[c] = clampi(j0 + c, j_first, j_last) - j_first;
        uint32_t acc[PXH][PXW] = {};
        box_walk_plane<false, PXH>(py, uv4, L.band, buf_bytes, active, jr, col, acc);
        const BoxDiv dv = box_div_of(64u * py.Ny);
#pragma unroll
        for (int rr = 0; rr < PXH; rr++)
#pragma unroll
            for (int c = 0; c < PXW; c++) Yf[rr][c] = (float)box_sample(acc[rr][c], py.Ny, dv);
    }
    if constexpr (!kLumaOnly<OUT>) {
        const BoxPlane puv = roi_box_plane((const uint8_t *)(GP)(uintptr_t)r.uv, r.pitch_uv, r.src_w >> 1, L.dst_w >> 1, r.src_h >> 1, L.dst_h >> 1, j_first >> 1,
                                           j_last >> 1, i_first >> 1, i_last >> 1);
        const int jr[1] = { clampi(i0, i_first, i_last) >> 1 }, cj0 = j0 >> 1;
        int col[4];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            col[2 * c] = 2 * (clampi(cj0 + c, j_first >> 1, j_last >> 1) - (j_first >> 1));
            col[2 * c + 1] = col[2 * c] + 1;
        }
        uint32_t acc[1][4] = {};
        box_walk_plane<true, 1>(puv, uv4, L.band, buf_bytes, active, jr, col, acc);
        const BoxDiv dv = box_div_of(64u * puv.Ny);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            Uf[c] = (float)box_sample(acc[0][2 * c], puv.Ny, dv);
            Vf[c] = (float)box_sample(acc[0][2 * c + 1], puv.Ny, dv);
        }
    }
    if (active) p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

} // namespace tsvpp
