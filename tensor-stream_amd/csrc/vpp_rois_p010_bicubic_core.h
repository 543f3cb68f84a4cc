// vpp_rois_p010_bicubic_core.h -- the P010 BICUBIC region-of-interest kernel (see vpp_rois_p010_bicubic.hip for what it does), as a template that two translation
// units instantiate: vpp_rois_p010_bicubic.hip with the library's output flavours (EL_LIB) and vpp_rois_p010_bicubic_tensor.hip with the tensor store.
//
// Called, not copied: the grid (tile_index), the descriptor fill (tile_desc), the shifted last tile column (roi_tile_col0), describe_plane and the LDS-DMA loop
// (stage_plane_dma), the chroma pair reader (p010_pair), and everything behind the samples (p010_store_tile, vpp_letterbox_p010_core.h) -- on integer-valued
// Yf / Uf / Vf, as the NEAREST / BILINEAR kernel hands them over.  The arithmetic is vpp_cubic_p010.h's, shared with the host.  New here: the sampling stage, a
// separable filter in two phases through LDS.
#pragma once
#include "vpp_rois_p010_bicubic.h"
#include "vpp_letterbox_p010_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// What one plane's two phases need to know of the box's plane and of the tile.  Luma: columns are samples of 2 bytes; chroma: (U, V) pairs of 4 bytes, and a
// column of Hbuf is a pair's U or V -- 16 pairs x 2 fill the 32 columns that 32 luma outputs fill.
struct CubicPlane {
    const uint8_t *base;
    int pitch;
    int xlo, xhi, ylo, yhi; // the footprint, in samples / pairs and rows, clamped into the box's plane
    CubicDiv ax, ay;        // the plane's two axes, box -> output
    int c0, ncols;          // first output column / pair of the tile, and how many
};

// One band: rows [row_lo, row_lo + nrows) of the footprint as raw words into `buf`, 16-byte chunks by LDS-DMA.  The caller waits and barriers.
template <int BYTES> __device__ __forceinline__ LdsPlane cubic_issue_band(const CubicPlane &pl, uint8_t *buf, int row_lo, int nrows, int cpr, uint32_t magic) {
    const uint8_t *a0;
    const LdsPlane lp = describe_plane(buf, pl.base, pl.pitch, row_lo, BYTES * pl.xlo, cpr, a0);
    stage_plane_dma(buf, a0, lp, pl.pitch, nrows, BYTES * (pl.xhi - pl.xlo + 1), magic, ROI_THREADS);
    return lp;
}

// Phase A, horizontal: the footprint's rows, band by band, into Hbuf[row - ylo][32] as 16-bit integers.  A lane keeps one output column (chroma: one pair) through
// the whole walk -- axis term, four clamped tap offsets and four weights once, in registers -- and takes the rows `tid >> 5` + 4 k of each band (chroma
// `tid >> 4` + 8 k): the lanes of a wave read neighbouring taps of two (four) rows.  Columns past the tile's last one filter that one again, so every Hbuf word
// that phase B may read is written.  Band b + 1 is issued before band b is filtered; one barrier per band orders the two buffers, the last one Hbuf.
template <bool CHROMA> __device__ __forceinline__ void cubic_walk_plane(const CubicPlane &pl, bool uv4, int band, int buf_bytes, int hrows) {
    constexpr int BYTES = CHROMA ? 4 : 2, LANES = CHROMA ? 16 : 32, RSTEP = ROI_THREADS / LANES;
    uint8_t *const buf0 = lds_raw + cubic_hbuf_bytes(hrows);
    const int cpr = roi_chunks(BYTES * (pl.xhi - pl.xlo + 1));
    band = min(band, (buf_bytes >> 4) / cpr); // (never smaller for a launch the host sized: the buffers hold `band` rows of the launch's widest footprint)
    if (band >= 1) {
        const uint32_t magic = 0xFFFFFFFFu / (uint32_t)cpr + 1u;
        const int hc = (int)threadIdx.x & (LANES - 1), hr0 = (int)threadIdx.x / LANES;
        const CubicTerm tx = cubic_term(pl.c0 + min(hc, pl.ncols - 1), pl.ax);
        int wx[4], off[4];
        cubic_weights(tx.F, wx);
#pragma unroll
        for (int k = 0; k < 4; k++) off[k] = BYTES * (clampi(cubic_tap(tx.p, k, pl.ax.N), pl.xlo, pl.xhi) - pl.xlo); // (the second clamp never fires: no read leaves the row)

        const int rows = pl.yhi - pl.ylo + 1, bands = (rows + band - 1) / band;
        LdsPlane lp = cubic_issue_band<BYTES>(pl, buf0, pl.ylo, min(band, rows), cpr, magic), lp_next = lp;
        for (int b = 0; b < bands; b++) {
            const int y0 = pl.ylo + b * band, nr = min(band, pl.yhi + 1 - y0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // band b has landed; behind the barrier: for both waves, and band b - 1 is filtered
            __syncthreads();
            if (b + 1 < bands) lp_next = cubic_issue_band<BYTES>(pl, buf0 + ((b + 1) & 1) * buf_bytes, y0 + band, min(band, pl.yhi + 1 - (y0 + band)), cpr, magic);
            for (int r = hr0; r < nr; r += RSTEP) {
                const uint8_t *p = lp.base + r * lp.lp + ((lp.m0 + r * lp.pm) & 15);
                const int hrow = y0 - pl.ylo + r;
                if constexpr (!CHROMA) {
                    const int s0 = *(const uint16_t *)(p + off[0]) >> 6, s1 = *(const uint16_t *)(p + off[1]) >> 6;
                    const int s2 = *(const uint16_t *)(p + off[2]) >> 6, s3 = *(const uint16_t *)(p + off[3]) >> 6;
                    ((int16_t *)lds_raw)[hrow * 32 + hc] = (int16_t)cubic_round_h(cubic_sum(wx, s0, s1, s2, s3));
                } else { // U and V of a pair: one dword per tap where the plane is 4-byte aligned
                    const uint32_t a0 = p010_pair(p + off[0], uv4), a1 = p010_pair(p + off[1], uv4), a2 = p010_pair(p + off[2], uv4), a3 = p010_pair(p + off[3], uv4);
                    const int hu = cubic_round_h(cubic_sum(wx, (int)((a0 >> 6) & 1023u), (int)((a1 >> 6) & 1023u), (int)((a2 >> 6) & 1023u), (int)((a3 >> 6) & 1023u)));
                    const int hv = cubic_round_h(cubic_sum(wx, (int)(a0 >> 22), (int)(a1 >> 22), (int)(a2 >> 22), (int)(a3 >> 22)));
                    ((uint32_t *)lds_raw)[hrow * 16 + hc] = ((uint32_t)hu & 0xFFFFu) | ((uint32_t)hv << 16);
                }
            }
            lp = lp_next;
        }
    }
    __syncthreads(); // Hbuf is complete
}

// Phase B, vertical: output row i of the plane for the lane's four Hbuf columns 4 lx .. 4 lx + 3 (luma: its four output columns; chroma: U, V of its two pairs).
// Four rows of Hbuf, clamped to the box, one 8-byte LDS read each.
__device__ __forceinline__ void cubic_vertical(const CubicPlane &pl, int i, int lx, int out[4]) {
    const CubicTerm ty = cubic_term(i, pl.ay);
    int wy[4];
    cubic_weights(ty.F, wy);
    uint2 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = *(const uint2 *)(lds_raw + CUBIC_HROW_BYTES * (clampi(cubic_tap(ty.p, k, pl.ay.N), pl.ylo, pl.yhi) - pl.ylo) + 8 * lx);
    out[0] = cubic_round_v(cubic_sum(wy, (int)(v[0].x << 16) >> 16, (int)(v[1].x << 16) >> 16, (int)(v[2].x << 16) >> 16, (int)(v[3].x << 16) >> 16));
    out[1] = cubic_round_v(cubic_sum(wy, (int)v[0].x >> 16, (int)v[1].x >> 16, (int)v[2].x >> 16, (int)v[3].x >> 16));
    out[2] = cubic_round_v(cubic_sum(wy, (int)(v[0].y << 16) >> 16, (int)(v[1].y << 16) >> 16, (int)(v[2].y << 16) >> 16, (int)(v[3].y << 16) >> 16));
    out[3] = cubic_round_v(cubic_sum(wy, (int)v[0].y >> 16, (int)v[1].y >> 16, (int)v[2].y >> 16, (int)v[3].y >> 16));
}

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
            cubic_vertical(pl, min(i0 + rr, i_last), lx, k);
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
        cubic_vertical(pl, min(i0, i_last) >> 1, lx, k);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            Uf[c] = (float)k[2 * c];
            Vf[c] = (float)k[2 * c + 1];
        }
    }
    if (active) p010_store_tile<OUT, VEC, EL>(Yf, Uf, Vf, d, L.spec, out, i0, j0, ncol);
}

} // namespace tsvpp
