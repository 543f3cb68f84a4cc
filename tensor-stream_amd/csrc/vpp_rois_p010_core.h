// vpp_rois_p010_core.h -- the P010 region-of-interest kernel (see vpp_rois_p010.hip for what it does), as a template that two translation units instantiate:
// vpp_rois_p010.hip with the library's output flavours (EL_LIB) and vpp_rois_p010_tensor.hip with the tensor store (EL_F32 / EL_HALF).
//
// The shape is the ROI kernel's (vpp_rois_core.h): RoiLaunch with up to 64 RoiRec records by value, workgroup -> (box, tile) by tile_index, 32 x 32 output tiles of
// 128 lanes with 4 x 2 thread tiles, the shifted last tile column for the vector flavours.  The 16-bit side is the P010 letterbox kernel's
// (vpp_letterbox_p010_core.h), called, not copied: the word readers (P010Global / P010Lds), the axis terms (p010_axis), the 10-bit colour and store side
// (p010_store_tile), the LDS need (p010_lds_need / p010_stageable); and, as there, tile_span_x / tile_span_y, describe_plane, stage_plane_dma and bilerp2.
// Written out: the thread tile.  p010_sample_tile is built around the letterbox rectangle (LbRec / LbPart / LbLaunch: the pad, the per-pair inside test, the
// clamp into the rectangle's part of the tile); a box fills its whole output, so none of that exists here and the function takes the two ratios alone.
#pragma once
#include "vpp_rois_p010.h"
#include "vpp_letterbox_p010_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// The thread tile at output (i0, j0) of a box: PXH x PXW luma samples and two chroma pairs, integer-valued floats 0..1023.  `s` reads the BOX (s.w x s.h samples,
// row 0 / column 0 at the box origin): every edge rule clamps to the box, never to the frame around it.  The axis terms are computed once per column and once per
// row of the thread tile; U and V share their weights and run as one pair through bilerp2, luma columns pair up the same way; the neighbouring words of luma taps
// A / B and C / D sit in one register each.  `j_last` is the output's last column: the element-wise flavours store 2 of the 4 columns where the output is 4 k + 2
// wide, and the two that do not exist sample the last one again instead of a coordinate outside the staged footprint.
template <int MODE, int OUT, class S>
__device__ __forceinline__ void p010_roi_sample_tile(const S &s, float xr, float yr, int i0, int j0, int j_last, float Yf[PXH][PXW], float Uf[2], float Vf[2]) {
#pragma unroll
    for (int c = 0; c < 2; c++) Uf[c] = Vf[c] = 0.0f; // (Y800 stores neither)
    if constexpr (!kLumaOnly<OUT>) {
        const P010Tap ty = p010_axis<MODE>(i0 >> 1, yr, s.h, s.h >> 1);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            P010Tap tx = p010_axis<MODE>(min((j0 >> 1) + c, j_last >> 1), xr, s.w, 0);
            if constexpr (MODE == M_NEAREST) {
                const uint32_t a = s.UV(ty.p, tx.p);
                Uf[c] = p010_lo(a);
                Vf[c] = p010_hi(a);
            } else {
                tx.step = (2 * tx.p + 2 >= s.w) ? 0 : 1; // (pairs, counted as sample_chroma counts them)
                const uint32_t a = s.UV(ty.p, tx.p), b = s.UV(ty.p, tx.p + tx.step), cc = s.UV(ty.p + ty.step, tx.p), dd = s.UV(ty.p + ty.step, tx.p + tx.step);
                const f2 wx = { tx.w, tx.w }, wy = { ty.w, ty.w };
                const f2 uv = trunc2(bilerp2((f2){ p010_lo(a), p010_hi(a) }, (f2){ p010_lo(b), p010_hi(b) }, (f2){ p010_lo(cc), p010_hi(cc) },
                                             (f2){ p010_lo(dd), p010_hi(dd) }, wx, (f2){ 1.0f, 1.0f } - wx, wy, (f2){ 1.0f, 1.0f } - wy));
                Uf[c] = uv.x;
                Vf[c] = uv.y;
            }
        }
    }
    P010Tap tx[PXW];
#pragma unroll
    for (int c = 0; c < PXW; c++) tx[c] = p010_axis<MODE>(min(j0 + c, j_last), xr, s.w, s.w);
#pragma unroll
    for (int rr = 0; rr < PXH; rr++) {
        const P010Tap ty = p010_axis<MODE>(i0 + rr, yr, s.h, s.h);
#pragma unroll
        for (int c = 0; c < PXW; c += 2) {
            if constexpr (MODE == M_NEAREST) {
                Yf[rr][c] = p010_lo(s.Y2(ty.p, tx[c].p, 0));
                Yf[rr][c + 1] = p010_lo(s.Y2(ty.p, tx[c + 1].p, 0));
            } else {
                const uint32_t ab0 = s.Y2(ty.p, tx[c].p, tx[c].step), cd0 = s.Y2(ty.p + ty.step, tx[c].p, tx[c].step);
                const uint32_t ab1 = s.Y2(ty.p, tx[c + 1].p, tx[c + 1].step), cd1 = s.Y2(ty.p + ty.step, tx[c + 1].p, tx[c + 1].step);
                const f2 wx = { tx[c].w, tx[c + 1].w }, wy = { ty.w, ty.w };
                const f2 v = trunc2(bilerp2((f2){ p010_lo(ab0), p010_lo(ab1) }, (f2){ p010_hi(ab0), p010_hi(ab1) }, (f2){ p010_lo(cd0), p010_lo(cd1) },
                                            (f2){ p010_hi(cd0), p010_hi(cd1) }, wx, (f2){ 1.0f, 1.0f } - wx, wy, (f2){ 1.0f, 1.0f } - wy));
                Yf[rr][c] = v.x;
                Yf[rr][c + 1] = v.y;
            }
        }
    }
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------------
template <int MODE, int OUT, bool VEC, bool STAGED, int EL = EL_LIB>
__global__ __launch_bounds__(ROI_THREADS) void vpp_rois_p010_kernel(const RoiLaunch L) {
    using T = typename OutT<OUT>::type;
    typedef __attribute__((address_space(1))) uint8_t *GP; // the records hold GLOBAL addresses
    // workgroup -> (box, tile): all tiles of a box are neighbours in the grid, so the lines that adjacent tiles share meet in L2
    const TileIndex tix = tile_index(L.tiles_x, L.tiles_y);
    const int box = tix.item, tyi = tix.tyi, txi = tix.txi;
    if (box >= L.n_rois) return;
    const RoiRec &r = L.r[box]; // wave-uniform index: scalar loads

    LaunchDesc d = {};
    tile_desc<OUT, VEC>(L, r, d);
    d.k.y_offset = 4.0f * d.k.y_offset; // the contract's scaled offsets (exact)
    d.k.c_offset = 4.0f * d.k.c_offset;

    const uint8_t *const plane_y = (const uint8_t *)(GP)(uintptr_t)r.y, *const plane_uv = (const uint8_t *)(GP)(uintptr_t)r.uv;
    // one dword per chroma pair: per BOX, from the advanced address and the pitch (with an even `left` the advance is a multiple of 4 bytes: it holds wherever it
    // holds for the frame)
    const bool uv4 = (((uint32_t)r.uv | (uint32_t)r.pitch_uv) & 3u) == 0u;
    T *const out = (T *)(GP)(uintptr_t)r.out;
    const int lx = threadIdx.x & (ROI_TX - 1), ly = threadIdx.x >> ROI_TX_SHIFT;
    const int j_first = roi_tile_col0(txi, L.dst_w, d.last_col0), i_first = tyi * ROI_TILE_H;
    const int j0 = j_first + lx * PXW, i0 = i_first + ly * PXH;
    const bool active = j0 < L.dst_w && i0 < L.dst_h && !(VEC && is_row_tail(d, j0));
    const int ncol = VEC ? PXW : min(PXW, L.dst_w - j0);
    float Uf[2], Vf[2], Yf[PXH][PXW];

    if constexpr (STAGED) {
        RoiFootprint f;
        tile_span_x(MODE, j_first, tile_last(j_first, ROI_TILE_W, L.dst_w), r.src_w, r.xr, f);
        tile_span_y(MODE, i_first, tile_last(i_first, ROI_TILE_H, L.dst_h), r.src_h, r.yr, f);
        if (p010_stageable(f) && p010_lds_need(f, kLumaOnly<OUT>) <= L.lds_bytes) { // (wave-uniform; per tile: one launch mixes staged and gathering tiles)
            // the footprint as raw words, 16-byte chunks straight from global memory into LDS: 8 luma samples or 4 chroma pairs per chunk
            const int span_y = p010_span_y(f.xhi - f.xlo + 1), span_uv = p010_span_uv(f.cxhi - f.cxlo + 1);
            const int ny = f.yhi - f.ylo + 1, nuv = kLumaOnly<OUT> ? 0 : f.cyhi - f.cylo + 1;
            const int cpr_y = roi_chunks(span_y), cpr_uv = roi_chunks(span_uv);
            uint8_t *lds_y = lds_raw, *lds_uv = lds_raw + 16 * p010_slots(ny * cpr_y);
            const uint8_t *ay, *auv;
            P010Lds s;
            s.py_ = describe_plane(lds_y, plane_y, r.pitch_y, f.ylo, 2 * f.xlo, cpr_y, ay);
            s.puv_ = describe_plane(lds_uv, plane_uv, r.pitch_uv, f.cylo, 4 * f.cxlo, cpr_uv, auv);
            s.w = r.src_w;
            s.h = r.src_h;
            s.uv4 = uv4;
            // slot -> (row, chunk) by multiply-high: one division per workgroup, on wave-uniform values
            stage_plane_dma(lds_y, ay, s.py_, r.pitch_y, ny, span_y, 0xFFFFFFFFu / (uint32_t)cpr_y + 1u, ROI_THREADS);
            if constexpr (!kLumaOnly<OUT>) stage_plane_dma(lds_uv, auv, s.puv_, r.pitch_uv, nuv, span_uv, 0xFFFFFFFFu / (uint32_t)cpr_uv + 1u, ROI_THREADS);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // LDS-DMA chunks have landed
            __syncthreads();
            if (!active) return;
            p010_roi_sample_tile<MODE, OUT>(s, r.xr, r.yr, i0, j0, L.dst_w - 1, Yf, Uf, Vf);
            p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
            return;
        }
    }
    if (!active) return;
    const P010Global s = { plane_y, plane_uv, r.pitch_y, r.pitch_uv, r.src_w, r.src_h, uv4 };
    p010_roi_sample_tile<MODE, OUT>(s, r.xr, r.yr, i0, j0, L.dst_w - 1, Yf, Uf, Vf);
    p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

} // namespace tsvpp
