// vpp_box_p010_walk.h -- the band walk of the P010 AREA kernels, once: the letterbox kernel (vpp_letterbox_p010_area_core.h) and the region-of-interest kernel
// (vpp_rois_p010_area_core.h) both reduce one plane of a tile's source footprint with it.  The footprint is walked in bands of source rows through two LDS
// buffers filled by LDS-DMA (describe_plane, stage_plane_dma); the arithmetic is vpp_box_p010.h's.  The callers differ in where the footprint, the band height
// and the buffer size come from: the letterbox kernel takes the latter two from its launch, the ROI kernel derives them per tile.
#pragma once
#include "vpp_box_p010.h"
#include "vpp_letterbox_p010_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// What one plane's walk needs to know of its plane and of the tile's part of it.  Luma: columns are samples of 2 bytes; chroma: (U, V) pairs of 4 bytes, and an
// "output column" of the row means is a pair's U or V -- 16 pairs x 2 fill the 32 columns that 32 luma outputs fill.
struct BoxPlane {
    const uint8_t *base;
    int pitch;
    int xlo, xhi, ylo, yhi; // the footprint, in samples / pairs and rows: exact, clamped into the plane
    uint32_t Nx, nx, Ny, ny; // the plane's two axes, source -> rectangle
    int c0, ncols;           // first output column / pair of the tile's part, and how many
};

// One band: rows [row_lo, row_lo + nrows) of the footprint as raw words into `buf`, 16-byte chunks by LDS-DMA.  The caller waits and barriers.
template <int BYTES> __device__ __forceinline__ LdsPlane box_issue_band(const BoxPlane &pl, uint8_t *buf, int row_lo, int nrows, int cpr, uint32_t magic) {
    const uint8_t *a0;
    const LdsPlane lp = describe_plane(buf, pl.base, pl.pitch, row_lo, BYTES * pl.xlo, cpr, a0);
    stage_plane_dma(buf, a0, lp, pl.pitch, nrows, BYTES * (pl.xhi - pl.xlo + 1), magic, ROI_THREADS);
    return lp;
}

// The walk of one plane.  NR = output rows of a lane's thread tile in this plane (luma 2, chroma 1); jr[] = those rows, col[] = the four columns of the row
// means the lane adds up (luma: its four output columns; chroma: U, V of its two pairs), both as indices of the tile's part; acc[][] = sum o_y r.
//
// Per band: (1) all 128 lanes form r for (source row x output column): lane -> column `tid & 31` (chroma: pair `tid & 15`), rows `tid >> 5` + 4 k (chroma
// `tid >> 4` + 8 k) -- a lane keeps its column through the whole walk, so its first tap and its two edge weights are computed once, in front of the first band,
// and the lanes of a wave read neighbouring taps of the same one or two rows.  (2) each lane adds the band's rows that overlap its own output rows, times the
// overlap, into acc.  Band b + 1 is issued before band b is reduced; two barriers per band order the buffers and the row means.
template <bool CHROMA, int NR>
__device__ __forceinline__ void box_walk_plane(const BoxPlane &pl, bool uv4, int band, int buf_bytes, bool sample, const int jr[NR], const int col[4], uint32_t acc[NR][4]) {
    constexpr int BYTES = CHROMA ? 4 : 2, LANES = CHROMA ? 16 : 32, RSTEP = ROI_THREADS / LANES;
    uint32_t *const rbuf = (uint32_t *)lds_raw;
    uint8_t *const buf0 = lds_raw + band * 128;
    const int cpr = roi_chunks(BYTES * (pl.xhi - pl.xlo + 1));
    band = min(band, (buf_bytes >> 4) / cpr); // (never smaller for a launch the host sized: the buffers hold `band` rows of the launch's widest footprint)
    if (band < 1) return;
    const uint32_t magic = 0xFFFFFFFFu / (uint32_t)cpr + 1u;
    const BoxDiv dnx = box_div_of(pl.nx), dny = box_div_of(pl.ny), dNx = box_div_of(pl.Nx);

    // horizontal: this lane's column
    const int hc = (int)threadIdx.x & (LANES - 1), hr0 = (int)threadIdx.x / LANES;
    const bool hon = hc < pl.ncols;
    BoxTaps tx = box_taps((uint32_t)(pl.c0 + min(hc, pl.ncols - 1)), pl.Nx, pl.nx, dnx);
    tx.first = (uint32_t)clampi((int)tx.first, pl.xlo, pl.xhi); // (no input can make a read leave the band buffer; for every valid request the clamps never fire)
    tx.count = min(min(tx.count, (uint32_t)BOX_P010_MAX_TAPS), (uint32_t)pl.xhi - tx.first + 1u);
    // vertical: this lane's rows
    BoxTaps ty[NR];
#pragma unroll
    for (int rr = 0; rr < NR; rr++) ty[rr] = box_taps((uint32_t)jr[rr], pl.Ny, pl.ny, dny);

    const int rows = pl.yhi - pl.ylo + 1, bands = (rows + band - 1) / band;
    LdsPlane lp = box_issue_band<BYTES>(pl, buf0, pl.ylo, min(band, rows), cpr, magic), lp_next = lp;
    for (int b = 0; b < bands; b++) {
        const int y0 = pl.ylo + b * band, nr = min(band, pl.yhi + 1 - y0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // band b has landed; behind the barrier: for both waves, and band b - 1 is reduced
        __syncthreads();
        if (b + 1 < bands) lp_next = box_issue_band<BYTES>(pl, buf0 + ((b + 1) & 1) * buf_bytes, y0 + band, min(band, pl.yhi + 1 - (y0 + band)), cpr, magic);
        if (hon) {
            for (int r = hr0; r < nr; r += RSTEP) {
                const uint8_t *p = lp.base + r * lp.lp + ((lp.m0 + r * lp.pm) & 15) + BYTES * ((int)tx.first - pl.xlo);
                if constexpr (!CHROMA) {
                    uint32_t mid = 0, s0 = (uint32_t)(*(const uint16_t *)p >> 6), s1 = 0;
                    for (uint32_t t = 1; t + 1 < tx.count; t++) mid += (uint32_t)(*(const uint16_t *)(p + 2 * t) >> 6);
                    if (tx.count > 1) s1 = (uint32_t)(*(const uint16_t *)(p + 2 * (tx.count - 1)) >> 6);
                    rbuf[r * 32 + hc] = box_row_mean(tx.w_first * s0 + pl.nx * mid + tx.w_last * s1, dNx);
                } else { // U and V of a pair: one dword where the plane is 4-byte aligned
                    const uint32_t a = p010_pair(p, uv4);
                    uint32_t mu = 0, mv = 0, u1 = 0, v1 = 0;
                    for (uint32_t t = 1; t + 1 < tx.count; t++) {
                        const uint32_t m = p010_pair(p + 4 * t, uv4);
                        mu += (m >> 6) & 1023u;
                        mv += m >> 22;
                    }
                    if (tx.count > 1) {
                        const uint32_t z = p010_pair(p + 4 * (tx.count - 1), uv4);
                        u1 = (z >> 6) & 1023u;
                        v1 = z >> 22;
                    }
                    rbuf[r * 32 + 2 * hc] = box_row_mean(tx.w_first * ((a >> 6) & 1023u) + pl.nx * mu + tx.w_last * u1, dNx);
                    rbuf[r * 32 + 2 * hc + 1] = box_row_mean(tx.w_first * (a >> 22) + pl.nx * mv + tx.w_last * v1, dNx);
                }
            }
        }
        __syncthreads();
        if (sample) {
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                const int f = max((int)ty[rr].first, y0), l = min((int)(ty[rr].first + ty[rr].count) - 1, y0 + nr - 1);
                for (int y = f; y <= l; y++) {
                    const uint32_t o = box_overlap((uint32_t)y, (uint32_t)jr[rr], pl.Ny, pl.ny);
                    const uint32_t *row = rbuf + (y - y0) * 32;
#pragma unroll
                    for (int c = 0; c < 4; c++) acc[rr][c] += o * row[col[c]];
                }
            }
        }
        lp = lp_next;
    }
}

} // namespace tsvpp
