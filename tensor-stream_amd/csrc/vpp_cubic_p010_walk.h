// vpp_cubic_p010_walk.h -- the two-phase walk of the P010 BICUBIC kernels, once: the region-of-interest kernel (vpp_rois_p010_bicubic_core.h) and the letterbox
// kernel (vpp_letterbox_p010_bicubic_core.h) both filter one plane of a tile's source footprint with it.  The footprint is walked in bands of source rows through
// two LDS buffers filled by LDS-DMA (describe_plane, stage_plane_dma) into the tile-resident Hbuf, from which each lane forms its thread tile vertically; the
// arithmetic is vpp_cubic_p010.h's.  The callers differ in what the output columns of Hbuf are -- the ROI kernel's tile, the letterbox kernel's part of the
// rectangle inside its tile -- and so in where a lane's columns lie in an Hbuf row.
#pragma once
#include "vpp_cubic_p010.h"
#include "vpp_letterbox_p010_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// What one plane's two phases need to know of the source plane and of the tile.  Luma: columns are samples of 2 bytes; chroma: (U, V) pairs of 4 bytes, and a
// column of Hbuf is a pair's U or V -- 16 pairs x 2 fill the 32 columns that 32 luma outputs fill.
struct CubicPlane {
    const uint8_t *base;
    int pitch;
    int xlo, xhi, ylo, yhi; // the footprint, in samples / pairs and rows, clamped into the source plane
    CubicDiv ax, ay;        // the plane's two axes, source -> output
    int c0, ncols;          // first output column / pair of the tile (of the tile's part), and how many
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

// Phase B, vertical: output row i of the plane for four Hbuf columns of the lane, as two pairs of neighbours: the dwords at byte offsets o0 and o1 of an Hbuf row
// (luma: two of its output columns each; chroma: U, V of one pair each).  The ROI kernel's columns are 4 lx .. 4 lx + 3 of the tile (o0 = 8 lx, o1 = o0 + 4), the
// letterbox kernel's lie where the rectangle puts them.  Four rows of Hbuf, clamped to the footprint, two 4-byte LDS reads each.
__device__ __forceinline__ void cubic_vertical(const CubicPlane &pl, int i, int o0, int o1, int out[4]) {
    const CubicTerm ty = cubic_term(i, pl.ay);
    int wy[4];
    cubic_weights(ty.F, wy);
    uint2 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint8_t *row = lds_raw + CUBIC_HROW_BYTES * (clampi(cubic_tap(ty.p, k, pl.ay.N), pl.ylo, pl.yhi) - pl.ylo);
        v[k].x = *(const uint32_t *)(row + o0);
        v[k].y = *(const uint32_t *)(row + o1);
    }
    out[0] = cubic_round_v(cubic_sum(wy, (int)(v[0].x << 16) >> 16, (int)(v[1].x << 16) >> 16, (int)(v[2].x << 16) >> 16, (int)(v[3].x << 16) >> 16));
    out[1] = cubic_round_v(cubic_sum(wy, (int)v[0].x >> 16, (int)v[1].x >> 16, (int)v[2].x >> 16, (int)v[3].x >> 16));
    out[2] = cubic_round_v(cubic_sum(wy, (int)(v[0].y << 16) >> 16, (int)(v[1].y << 16) >> 16, (int)(v[2].y << 16) >> 16, (int)(v[3].y << 16) >> 16));
    out[3] = cubic_round_v(cubic_sum(wy, (int)v[0].y >> 16, (int)v[1].y >> 16, (int)v[2].y >> 16, (int)v[3].y >> 16));
}

} // namespace tsvpp
