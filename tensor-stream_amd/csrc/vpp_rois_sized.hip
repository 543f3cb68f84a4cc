// vpp_rois_sized.hip -- many regions of interest, each resized to ITS OWN output size, in one launch (tsvpp_convert_rois_sized, include/tsvpp.h): text lines of one
// height and their own widths, the levels of a pyramid, the inputs of several heads behind one detector pass.
//
// The kernel is vpp_rois.hip's with the output side per box.  There every box becomes dst_w x dst_h and a workgroup finds its (box, tile) with one division; here
// the boxes' tile counts differ, so the launch carries their running sum (SizedLaunch::tile_end) and a workgroup counts the entries at or below its index
// (sized_tile, vpp_rois_sized.h: scalar loads and scalar compares, no dependent loads).  dst_w, dst_h, the shifted last tile column and the row-tail rule come
// from the box's 64-byte record (RoiRec's 48 bytes + dst_w, dst_h, tiles_x, tile0).  The grid is exactly the sum of the tile counts: no workgroup without a tile.
// Source side, staging and per-pixel arithmetic: vpp_rois.hip's, through the same functions.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off.  Written for wave64 / CDNA4 only.

#include "vpp_rois_sized_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel: vpp_rois_sized_core.h, shared with vpp_rois_sized_tensor.hip)

hipError_t launch_rois_sized(Mode mode, OutKind out, bool vec, bool staged, const SizedLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                             size_t name_len, bool dry_run) {
    if (!tile_mode(mode) || !tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_rois_sized<%s,%s,%s,%s>", kModeNames[mode], kOutNames[out], vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_mode(mode, [&](auto M) {
        return with_tile_flavour(out, [&](auto O) {
            return with_vec_staged(vec, staged, [&](auto V, auto S) {
                constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
                hipLaunchKernelGGL((vpp_rois_sized_kernel<decltype(M)::value, decltype(O)::value, decltype(V)::value, STAGED>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
                return hipGetLastError();
            });
        });
    });
}

} // namespace tsvpp
