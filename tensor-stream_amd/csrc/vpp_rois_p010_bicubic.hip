// vpp_rois_p010_bicubic.hip -- tsvpp_convert_rois_p010_bicubic (include/tsvpp.h): the P010 region-of-interest call with a separable Keys cubic in 32-bit integers
// (vpp_cubic_p010.h) -- the filter a 40-80 pixel face, plate or text box should get on its way UP to 112 or 224 squared, on all ten bits.
//
// Grid, records and everything behind the samples (p010_store_tile) are the P010 ROI kernel's: a 48-byte record per box with the plane addresses advanced to the
// box origin, 32 x 32 output tiles of 128 lanes with 4 x 2 thread tiles.  The sampling stage is new: not 16 taps gathered per output sample (5 four-tap sums per
// sample, 5120 per tile), but two phases through LDS (rows_fp x 32 + 1024 sums: 1632 at an exact 2 x up-scale, 3168 at a ratio of 2):
//   stage       the tile's source footprint -- rows [p_y(first) - 1, p_y(last) + 2] x columns alike, clamped into the BOX -- is walked in bands of rows: band b + 1
//               goes from global memory into one of two LDS buffers as raw words, 16-byte chunks by LDS-DMA (stage_plane_dma), while band b is filtered
//   horizontal  a lane keeps ONE output column for the whole walk (`tid & 31`; chroma: the pair `tid & 15`, one dword per tap where the plane is 4-byte aligned):
//               axis term, four clamped tap offsets and four weights once, in registers; per (row, column) four 24-bit multiply-adds on `word >> 6`, one rounding
//               shift, one 16-bit store into the tile-resident Hbuf[row][32]
//   vertical    behind a barrier, each lane forms its 4 x 2 thread tile from Hbuf: its four columns of a row are one 8-byte LDS read, four rows per output row,
//               four multiply-adds, a rounding shift and a clamp per sample
// Luma first, then chroma through the same LDS.  Hbuf is bounded by the ratio limit (32 * 8 + 3 rows of 64 bytes); the band height comes with the launch
// (RoiCubicLaunch::band: what the LDS budget leaves behind Hbuf at the launch's widest footprint).  No float reaches a sample: fp32 only guesses the quotients
// of the axis terms (box_quot).  No matrix instructions: the contraction is over four taps whose weights differ per output column.
// This unit and its tensor twin are compiled without packed fp32 instructions, as the other P010 units (Makefile).  Written for wave64 / CDNA4 only.

#include "vpp_rois_p010_bicubic_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_rois_p010_bicubic(OutKind out, bool vec, const RoiCubicLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                                    bool dry_run) {
    if (!tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_rois_p010_bicubic<%s,%s>", kOutNames[out], vec_name(vec));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        if (vec) hipLaunchKernelGGL((vpp_rois_p010_bicubic_kernel<decltype(O)::value, true>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        else hipLaunchKernelGGL((vpp_rois_p010_bicubic_kernel<decltype(O)::value, false>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        return hipGetLastError();
    });
}

} // namespace tsvpp
