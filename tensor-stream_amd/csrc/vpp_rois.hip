// vpp_rois.hip -- many regions of interest, each resized to ONE output size, in one launch (tsvpp_convert_rois, include/tsvpp.h).
//
// The output side is uniform -- every box becomes dst_w x dst_h -- so a workgroup finds its (box, output tile) with one division and stores its tile through the
// library's colour back end (color_store_tile: vector stores for 16-byte aligned outputs, element-wise stores otherwise, the shifted last tile column for widths
// 4 k + 2).  What differs per box -- plane origins, pitches, size, ratios, output pointer -- is a 48-byte record indexed by the workgroup's box: wave-uniform, read
// with scalar loads out of the kernarg segment, never re-derived per lane.  The per-pixel arithmetic is the shared samplers' (vpp_device.h: coordinates from
// vpp_axis.h, bilerp, the mixed-precision cubic with its tie test); this file adds the per-box geometry around them.
//
// Source side: a tile's footprint is small and neighbouring lanes tap overlapping bytes, so the workgroup stages the luma and chroma footprints of its tile in LDS
// with 16-byte loads (stage_planes) and samples through LdsSrc.  The footprint follows from the box's ratios, i.e. it differs per box: it is computed in the
// kernel from wave-uniform values (tile_span_x / tile_span_y: the numbers the host sized the launch's LDS with), and a tile whose footprint does not fit the
// launch's LDS -- a large box against the LDS budget -- gathers its taps from global memory instead (GlobalSrc), a wave-uniform branch.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off; the only fused operations are the explicit ones of the
// shared samplers.  Written for wave64 / CDNA4 only.

#include "vpp_rois_core.h"
#include "vpp_tile_launch.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel: vpp_rois_core.h, shared with vpp_rois_tensor.hip)

hipError_t launch_rois(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                       size_t name_len, bool dry_run) {
    if (!tile_mode(mode) || !tile_flavour(out)) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_rois<%s,%s,%s,%s>", kModeNames[mode], kOutNames[out], vec_name(vec), staged_name(staged));
    if (dry_run) return hipSuccess;
    return with_tile_mode(mode, [&](auto M) {
        return with_tile_flavour(out, [&](auto O) {
            return with_vec_staged(vec, staged, [&](auto V, auto S) {
                constexpr bool STAGED = decltype(S)::value; // (the gather kernel takes no dynamic LDS)
                hipLaunchKernelGGL((vpp_rois_kernel<decltype(M)::value, decltype(O)::value, decltype(V)::value, STAGED>), dim3(grid), dim3(ROI_THREADS), STAGED ? lds_bytes : 0, stream, L);
                return hipGetLastError();
            });
        });
    });
}

} // namespace tsvpp
