// vpp_letterbox_p010.hip -- tsvpp_convert_letterbox_p010 (include/tsvpp.h): the letterbox call for 10-bit P010 sources -- n frames of 16-bit words, the sample in
// the ten high bits, each resized with its aspect kept into an inner rectangle of ONE canvas size, the rest of the canvas filled with a constant, in one launch.
//
// Grid, records, rectangle logic and the staged / gathered decision per tile are the letterbox kernel's (vpp_letterbox.hip).  New for 16-bit sources:
//   staging   the footprint of the part of the tile inside the rectangle goes into LDS as raw words, 16-byte chunks by LDS-DMA (global_load_lds_dwordx4: no VGPR
//             round trip); a chunk is 8 luma samples or 4 chroma pairs, the LDS need is p010_lds_need (vpp_letterbox_p010.h) -- twice the 8-bit call's
//   taps      a chroma pair is one dword where the plane is 4-byte aligned, U and V leave it with one bit-field extract each, which IS the contract's `>> 6`;
//             luma taps A / B and C / D share a register
//   blend     the letterbox call's fused pattern on the values 0..1023, U with V and luma column with luma column as one pair
//   colour    the library's expression with the two offsets scaled by four, clamped to 0..1023; k / 1023 by a reciprocal pair, correctly rounded; bytes as
//             min(255, (k + 2) >> 2) through the existing packers
// No matrix instructions: there is no contraction in this operation.  This unit and its tensor twin are compiled without packed fp32 instructions (Makefile).
//
// Arithmetic contract (include/tsvpp.h): single IEEE-754 operations in the stated order, contraction off; the only fused operations are the
// explicit ones.  Written for wave64 / CDNA4 only.

#include "vpp_letterbox_p010_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

hipError_t launch_letterbox_p010(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                                 size_t name_len, bool dry_run) {
    if ((mode != M_NEAREST && mode != M_BILINEAR) || !tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_letterbox_p010<%s,%s,%s,%s>", kModeNames[mode], kOutNames[out], vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_flavour(out, [&](auto O) {
        return with_vec_staged(vec, staged, [&](auto V, auto S) {
            constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
            if (mode == M_NEAREST) hipLaunchKernelGGL((vpp_letterbox_p010_kernel<M_NEAREST, decltype(O)::value, decltype(V)::value, STAGED>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
            else hipLaunchKernelGGL((vpp_letterbox_p010_kernel<M_BILINEAR, decltype(O)::value, decltype(V)::value, STAGED>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
            return hipGetLastError();
        });
    });
}

} // namespace tsvpp
