// vpp_letterbox_area.hip -- the letterbox call with AREA (tsvpp_convert_letterbox_area, include/tsvpp.h): n frames, each resized with its aspect kept into an inner
// rectangle of ONE canvas size by the AREA rules, the rest of the canvas filled with a constant, in one launch.
//
// Two kernels put together.  From vpp_letterbox.hip: the grid over the canvas, the 64-byte record per frame read with scalar loads out of the kernarg segment, the
// part of a tile inside the rectangle (tile_inner_range), sampling at inner coordinates clamped into that part, the select between sample and pad in front of the
// one call of the colour back end.  From vpp_rois_area.hip: AREA's two rules chosen per frame (roi_area_mode, a wave-uniform branch on the record) -- the 2 x 2
// blend through the shared M_AREA_UP samplers and the weighted box of the down-scale --, the weight rows GENERATED inside the tile (roi_area_step: no device
// table, no allocation, no copy, nothing cached), their layout in front of the staged footprint (32 luma + 17 chroma rows per axis at a stride of taps | 1,
// 12-byte records written by the chain lanes and expanded by 98 lanes), and the samplers area_luma / area_chroma.  The rows are those of the INNER indices
// [a0, a1] x [b0, b1] the tile covers, which is why the canvas offset of the rectangle costs nothing.
//
// What is new is where the chains start.  In vpp_rois_area.hip one lane walks the generator from index 0 to the tile's last index: ~75 ns per index in front of
// every tile, ~45 us in front of column 608 of a 640-wide canvas.  The generator resets to its initial state wherever its closing test passes, and that test
// depends on the pattern index and the scale alone (vpp_letterbox_area.h): the resets are periodic, so a chain may start at the last multiple of the period P
// in front of the tile and produce the same rows, bit for bit.  The second wave first finds P of each axis -- the tests of k = 1 .. first are independent, 64 per
// ballot round -- and then four of its lanes run four chains side by side: x and y, luma and chroma each (the chroma range [a0 >> 1, a1 >> 1] begins below the luma
// start, so it has a start of its own).  1920 -> 640, 3840 -> 640 and 1280 -> 640 have P = 1: every chain starts at its tile.  Where the pattern does not close in
// front of the tile the chain starts at 0 as before; the result is the same, only the time differs.  The first wave stages the footprint meanwhile.
// A tile outside the rectangle stores the pad and generates nothing.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_letterbox_area_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel: vpp_letterbox_area_core.h, shared with vpp_letterbox_area_tensor.hip)

hipError_t launch_letterbox_area(OutKind out, bool vec, bool staged, const LbAreaLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                 size_t name_len, bool dry_run) {
    if (!tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_letterbox_area<%s,%s,%s>", kOutNames[out], vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) { // (lds_bytes either way: the weight rows need LDS in the gather kernel too)
            hipLaunchKernelGGL((vpp_letterbox_area_kernel<decltype(O)::value, decltype(V)::value, decltype(S)::value>), dim3(grid), dim3(ROI_THREADS), lds_bytes, stream, L);
            return hipGetLastError();
        });
    });
}

} // namespace tsvpp
