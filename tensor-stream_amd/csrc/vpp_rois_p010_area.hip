// vpp_rois_p010_area.hip -- tsvpp_convert_rois_p010_area (include/tsvpp.h): the P010 region-of-interest call with the exact box filter in unsigned 32-bit
// integers (vpp_box_p010.h) -- the filter a 300 x 700 person box should get on its way DOWN to 128 x 256, or a 500-pixel vehicle box to 224 squared, on all
// ten bits.
//
// Grid, records and everything behind the samples (p010_store_tile) are the P010 ROI kernel's: a 48-byte record per box with the plane addresses advanced to the
// box origin, 32 x 32 output tiles of 128 lanes with 4 x 2 thread tiles, every tile wholly inside its box's output -- no canvas, no pad, no rectangle.  The
// sampling stage is the P010 AREA letterbox kernel's band walk (box_walk_plane), called: two phases through LDS cannot hold a tile's intermediate rows here
// (512 rows x 128 bytes at 16 : 1), so the walk accumulates:
//   stage       the tile's source footprint -- first tap of its first output to last tap of its last, per axis, inside the BOX's plane -- is walked in bands of
//               rows: band b + 1 goes from global memory into one of two LDS buffers as raw words, 16-byte chunks by LDS-DMA, while band b is reduced
//   horizontal  a lane keeps ONE output column for the whole walk (`tid & 31`; chroma: the pair `tid & 15`): first tap and the two edge weights once, then per
//               (row, column) the row mean in 1/64 sample steps (box_row_mean) into the band's 32-column row-mean buffer
//   vertical    every lane adds the band's rows that overlap its own 4 x 2 outputs, times box_overlap, into its eight accumulators; box_sample ends the walk
// Luma first, then chroma through the same LDS.
// The band height comes with the launch (RoiBoxLaunch::band: what the LDS budget holds at the launch's widest footprint row); a height per tile was measured
// and lost (vpp_rois_p010_area.h).  The footprint and every clamp are the tile's own, to its box's plane.
// No float reaches a sample: fp32 only guesses quotients (box_quot).  No matrix instructions: the contraction is over a per-column tap count with two edge
// weights that differ per output column, not a dense product.
// This unit and its tensor twin are compiled without packed fp32 instructions, as the other P010 units (Makefile).  Written for wave64 / CDNA4 only.

#include "vpp_rois_p010_area_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_rois_p010_area(OutKind out, bool vec, const RoiBoxLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                                 bool dry_run) {
    if (!tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_rois_p010_area<%s,%s>", kOutNames[out], vec_name(vec));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        if (vec) hipLaunchKernelGGL((vpp_rois_p010_area_kernel<decltype(O)::value, true>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        else hipLaunchKernelGGL((vpp_rois_p010_area_kernel<decltype(O)::value, false>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        return hipGetLastError();
    });
}

} // namespace tsvpp
