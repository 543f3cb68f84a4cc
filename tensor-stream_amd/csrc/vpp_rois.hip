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
// kernel from wave-uniform values (roi_span_x / roi_span_y: the numbers the host sized the launch's LDS with), and a tile whose footprint does not fit the
// launch's LDS -- a large box against the LDS budget -- gathers its taps from global memory instead (GlobalSrc), a wave-uniform branch.
//
// Arithmetic contract as everywhere: single IEEE-754 operations in the reference's order, contraction off; the only fused operations are the explicit ones of the
// shared samplers.  Written for wave64 / CDNA4 only.

#include "vpp_rois_core.h"

#pragma clang fp contract(off)

namespace tsvpp {

// (the kernel: vpp_rois_core.h, shared with vpp_rois_tensor.hip)

namespace {

const char *const kModeNames[M_COUNT] = { "M_NONE", "M_NEAREST", "M_BILINEAR", "M_BICUBIC", "M_AREA_DOWN", "M_AREA_UP" };
const char *const kOutNames[O_COUNT] = { "O_U8_PLANAR", "O_U8_MERGED", "O_F32_PLANAR", "O_F32_MERGED", "O_NV12_U8", "O_NV12_F32", "O_Y800_U8", "O_Y800_F32", "O_HSV_F32" };

template <int MODE, int OUT, bool VEC, bool STAGED>
hipError_t launch_k(const RoiLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((vpp_rois_kernel<MODE, OUT, VEC, STAGED>), dim3(grid), dim3(ROI_THREADS), lds, stream, L);
    return hipGetLastError();
}
template <int MODE, int OUT>
hipError_t launch_mo(bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    if (vec) return staged ? launch_k<MODE, OUT, true, true>(L, grid, lds, stream) : launch_k<MODE, OUT, true, false>(L, grid, 0, stream);
    return staged ? launch_k<MODE, OUT, false, true>(L, grid, lds, stream) : launch_k<MODE, OUT, false, false>(L, grid, 0, stream);
}
// the flavours this kernel is instantiated for: RGB / BGR planar and merged, Y800
constexpr bool roi_flavour(int out) { return out == O_U8_PLANAR || out == O_U8_MERGED || out == O_F32_PLANAR || out == O_F32_MERGED || out == O_Y800_U8 || out == O_Y800_F32; }
template <int MODE>
hipError_t launch_m(OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds, hipStream_t stream) {
    return with_out_kind(out, [&](auto O) {
        constexpr int OUT = decltype(O)::value;
        if constexpr (roi_flavour(OUT)) return launch_mo<MODE, OUT>(vec, staged, L, grid, lds, stream);
        else return hipErrorNotSupported; // a missing kernel is an error, never a fallback
    });
}

} // namespace

hipError_t launch_rois(Mode mode, OutKind out, bool vec, bool staged, const RoiLaunch &L, unsigned grid, size_t lds_bytes, hipStream_t stream, char *name,
                       size_t name_len, bool dry_run) {
    const bool known = (mode == M_NEAREST || mode == M_BILINEAR || mode == M_BICUBIC) && roi_flavour(out);
    if (!known) return hipErrorNotSupported;
    if (name && name_len) snprintf(name, name_len, "vpp_rois<%s,%s,%s,%s>", kModeNames[mode], kOutNames[out], vec ? "vec" : "elem", staged ? "staged" : "gather");
    if (dry_run) return hipSuccess;
    switch (mode) {
    case M_NEAREST: return launch_m<M_NEAREST>(out, vec, staged, L, grid, lds_bytes, stream);
    case M_BILINEAR: return launch_m<M_BILINEAR>(out, vec, staged, L, grid, lds_bytes, stream);
    default: return launch_m<M_BICUBIC>(out, vec, staged, L, grid, lds_bytes, stream);
    }
}

} // namespace tsvpp
