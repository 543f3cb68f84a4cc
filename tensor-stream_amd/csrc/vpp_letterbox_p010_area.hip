// vpp_letterbox_p010_area.hip -- tsvpp_convert_letterbox_p010_area (include/tsvpp.h): the P010 letterbox call with an exact box filter -- every source sample of a
// frame is averaged into the output sample whose interval it overlaps, in unsigned 32-bit integers (vpp_box_p010.h), where NEAREST / BILINEAR point-sample one
// source sample in nine at 1080p -> 640 and one in 36 at 4K.
//
// Grid, records, rectangle logic, pad tiles and everything behind the samples (p010_store_tile) are the P010 letterbox kernel's.  The sampling stage is new and
// has another shape than the "stage the footprint or gather" split of the other tile kernels: a tile's footprint grows with the ratio (192 x 192 luma words,
// 72 KiB, at 6) and a box filter's footprints are disjoint, so LDS serves coalescing, not reuse.  The workgroup walks the footprint in bands of source rows:
//   stage      band b + 1 goes from global memory into one of two LDS buffers as raw words, 16-byte chunks by LDS-DMA (stage_plane_dma), while band b is reduced
//   horizontal all 128 lanes form the normalised row means r for (source row x output column) of band b into 32 words per row: a lane keeps one output column
//              through the whole walk (first tap and edge weights in closed form, once), its rows are 4 apart (chroma: a lane keeps one (U, V) pair -- one dword
//              per tap where the plane is 4-byte aligned -- and its rows are 8 apart)
//   vertical   each lane adds the band's rows times their overlap with its own output rows into the accumulators of its 4 x 2 thread tile, and normalises after
//              the last band
// Luma first, then chroma through the same buffers.  The band height comes with the launch (LbBoxLaunch::band: what the LDS budget holds at the launch's widest
// footprint), so LDS use is bounded whatever the ratio.  No float reaches a sample: fp32 only guesses the quotients of the three divisions by per-frame constants
// (box_quot).  No matrix instructions: the contraction is over 1 .. 17 taps of integer weights that differ per output column.
// This unit and its tensor twin are compiled without packed fp32 instructions, as the other P010 units (Makefile).  Written for wave64 / CDNA4 only.

#include "vpp_letterbox_p010_area_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_letterbox_p010_area(OutKind out, bool vec, const LbBoxLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name, size_t name_len,
                                      bool dry_run) {
    if (!tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_letterbox_p010_area<%s,%s>", kOutNames[out], vec_name(vec));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        if (vec) hipLaunchKernelGGL((vpp_letterbox_p010_area_kernel<decltype(O)::value, true>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        else hipLaunchKernelGGL((vpp_letterbox_p010_area_kernel<decltype(O)::value, false>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
        return hipGetLastError();
    });
}

} // namespace tsvpp
