// vpp_letterbox.hip -- n frames, each resized with its aspect kept into an inner rectangle of ONE canvas size, the rest of the canvas filled with a constant, in one
// launch (tsvpp_convert_letterbox, include/tsvpp.h).
//
// The grid runs over the CANVAS: a workgroup finds its (frame, canvas tile) with one division, and LaunchDesc::dst_w / dst_h are the canvas, so a tile goes out
// through the library's colour back end unchanged (color_store_tile: vector stores for 16-byte aligned outputs, element-wise stores otherwise, the shifted last
// tile column for widths 4 k + 2).  What differs per frame -- planes, pitches, size, ratios, rectangle, canvas pointer -- is a 64-byte record indexed by the
// workgroup's frame: wave-uniform, read with scalar loads out of the kernarg segment.
//
// Every field of the rectangle is even.  A thread tile is 2 rows x 4 columns at an even origin, so its two rows are both inside the rectangle or both outside, and
// each of its two 2-column chroma pairs is wholly in or out: canvas pixel (i, j) inside the rectangle is inner pixel (i - top, j - left), canvas pair (i >> 1,
// j >> 1) is inner pair ((i - top) >> 1, (j - left) >> 1).  The thread tile samples at those inner coordinates -- clamped into the part of the rectangle its
// workgroup's tile covers, so every access stays inside the staged footprint whatever the lane -- and then selects, per pair, between the samples and the pad
// sample before the one call of the colour back end: the pad runs through the same colour arithmetic as every sample, in every flavour.
//
// Source side: the ROI kernel's (vpp_rois.hip).  The footprint of the part of the tile inside the rectangle is staged in LDS with 16-byte loads (stage_planes) and
// sampled through LdsSrc; a tile whose footprint does not fit the launch's LDS gathers from global memory (GlobalSrc), a wave-uniform branch; a tile that does not
// touch the rectangle stages nothing, samples nothing and stores pad.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off; the only fused operations are the explicit ones of the
// shared samplers.  Written for wave64 / CDNA4 only.

#include "vpp_letterbox_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel: vpp_letterbox_core.h, shared with vpp_letterbox_tensor.hip)

hipError_t launch_letterbox(Mode mode, OutKind out, bool vec, bool staged, const LbLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                            size_t name_len, bool dry_run) {
    if (!tile_mode(mode) || !tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_letterbox<%s,%s,%s,%s>", kModeNames[mode], kOutNames[out], vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_mode(mode, [&](auto M) {
        return with_tile_flavour(out, [&](auto O) {
            return with_vec_staged(vec, staged, [&](auto V, auto S) {
                constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
                hipLaunchKernelGGL((vpp_letterbox_kernel<decltype(M)::value, decltype(O)::value, decltype(V)::value, STAGED>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
                return hipGetLastError();
            });
        });
    });
}

} // namespace tsvpp
