// vpp_letterbox_p010_bicubic.hip -- tsvpp_convert_letterbox_p010_bicubic (include/tsvpp.h): the P010 letterbox call with a separable Keys cubic in 32-bit
// integers (vpp_cubic_p010.h) -- the filter a 640 x 360 or 720p 10-bit frame should get on its way UP into a 1280 x 1280 canvas, on all ten bits.
//
// Grid, records, rectangle logic, pad tiles and everything behind the samples (p010_store_tile) are the P010 letterbox kernel's: a 64-byte record per frame,
// 32 x 32 canvas tiles of 128 lanes with 4 x 2 thread tiles; a tile that holds none of the rectangle stores pad and returns.  A tile that holds some of it runs
// the P010 BICUBIC region-of-interest kernel's two phases (vpp_cubic_p010_walk.h) on the rectangle's part of the tile, columns t.a0 .. t.a1 and rows
// t.b0 .. t.b1 of the rectangle:
//   stage       the part's source footprint -- first tap of its first index to last tap of its last, per axis, clamped into the FRAME -- is walked in bands of
//               rows: band b + 1 goes from global memory into one of two LDS buffers as raw words, 16-byte chunks by LDS-DMA, while band b is filtered
//   horizontal  a lane keeps ONE output column of the part for the whole walk (chroma: one pair): axis term, four clamped tap offsets and four weights once, in
//               registers; per (row, column) four 24-bit multiply-adds, one rounding shift, one 16-bit store into the tile-resident Hbuf[row][32], whose column 0
//               is column t.a0 of the rectangle
//   vertical    behind a barrier, each lane forms its 4 x 2 thread tile from Hbuf.  The rectangle, the tile origins and the canvas width are even, so the thread
//               tile's column pairs (0, 1) and (2, 3) are each wholly inside the rectangle or wholly outside and each starts at an even Hbuf column: one dword
//               per pair and row at `2 * (j0 - left + 2 c - t.a0)`, which is 2 mod 4 where the rectangle starts inside a thread tile.  Pairs outside read the
//               part's nearest pair and take the pad instead; a lane wholly outside still filters its share of phase A and stands at every barrier
// Luma first, then chroma through the same LDS (one Hbuf dword per (U, V) pair).  Hbuf is bounded by the ratio limit (32 * 8 + 3 rows of 64 bytes); the band
// height, the band buffers' row size and Hbuf's rows come with the launch (LbCubicLaunch: taken over the tile parts of every frame of the launch).  No float
// reaches a sample: fp32 only guesses the quotients of the axis terms (box_quot).  No matrix instructions: the contraction is over four taps whose weights
// differ per output column.
// This unit and its tensor twin are compiled without packed fp32 instructions, as the other P010 units (Makefile).  Written for wave64 / CDNA4 only.

#include "vpp_letterbox_p010_bicubic_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_letterbox_p010_bicubic(OutKind out, bool vec, const LbCubicLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                         size_t name_len, bool dry_run) {
    if (!tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_letterbox_p010_bicubic<%s,%s>", kOutNames[out], vec_name(vec));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        if (vec) hipLaunchKernelGGL((vpp_letterbox_p010_bicubic_kernel<decltype(O)::value, true>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        else hipLaunchKernelGGL((vpp_letterbox_p010_bicubic_kernel<decltype(O)::value, false>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        return hipGetLastError();
    });
}

} // namespace tsvpp
