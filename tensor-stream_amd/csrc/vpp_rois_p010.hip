// vpp_rois_p010.hip -- tsvpp_convert_rois_p010 (include/tsvpp.h): the region-of-interest call for 10-bit P010 sources -- many boxes of a few frames of 16-bit
// words, the sample in the ten high bits, each cut out and resized to ONE output size, in one launch of up to 64 boxes.
//
// Grid, records and the staged / gathered decision per tile are the ROI kernel's (vpp_rois.hip): a 48-byte record per box with the plane addresses advanced to the
// box origin, read with scalar loads out of the kernarg segment; all tiles of a box are neighbours in the grid.  The 16-bit side is the P010 letterbox kernel's:
//   staging   the tile's footprint inside the box goes into LDS as raw words, 16-byte chunks by LDS-DMA (global_load_lds_dwordx4: no VGPR round trip); a chunk is
//             8 luma samples or 4 chroma pairs, the LDS need is p010_lds_need (vpp_letterbox_p010.h) -- twice the 8-bit call's, so a tile of a 300-500 pixel box
//             shrunk to 112 x 112 passes the default budget near a ratio of 3 and gathers its taps from global memory instead (a wave-uniform branch per tile)
//   taps      a chroma pair is one dword where the box's advanced plane address and pitch are 4-byte aligned, U and V leave it with one bit-field extract each,
//             which IS the contract's `>> 6`; luma taps A / B and C / D share a register; every edge clamp is to the BOX
//   blend     the fused pattern of the 8-bit calls on the values 0..1023, U with V and luma column with luma column as one pair
//   colour    p010_store_tile: the library's expression with the two offsets scaled by four, clamped to 0..1023; k / 1023 by a reciprocal pair, correctly rounded;
//             bytes as min(255, (k + 2) >> 2)
// No matrix instructions: there is no contraction in this operation.  This unit and its tensor twin are compiled without packed fp32 instructions (Makefile).
//
// Arithmetic contract (include/tsvpp.h): single IEEE-754 operations in the stated order, contraction off; the only fused operations are the
// explicit ones.  Written for wave64 / CDNA4 only.

#include "vpp_rois_p010_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_rois_p010(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                            size_t name_len, bool dry_run) {
    if ((mode != M_NEAREST && mode != M_BILINEAR) || !tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_rois_p010<%s,%s,%s,%s>", kModeNames[mode], kOutNames[out], vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) {
            constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
            if (mode == M_NEAREST) hipLaunchKernelGGL((vpp_rois_p010_kernel<M_NEAREST, decltype(O)::value, decltype(V)::value, STAGED>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
            else hipLaunchKernelGGL((vpp_rois_p010_kernel<M_BILINEAR, decltype(O)::value, decltype(V)::value, STAGED>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
            return hipGetLastError();
        });
    });
}

} // namespace tsvpp
